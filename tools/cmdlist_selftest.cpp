// Host-only check of the command list's storage and argument packing (torch-ngp_amd/csrc/cmdlist_core.h) under the host sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I torch-ngp_amd/csrc tools/cmdlist_selftest.cpp
//       -o cmdlist_selftest && ./cmdlist_selftest
// No HIP, no GPU, not loaded into Python: a stub launcher stands where cmdlist.cpp puts hipLaunchKernel, and checks on every replay that
// each argument it is handed has the bytes and the alignment it was recorded with -- after the caller's own copies were overwritten.
#include "cmdlist_core.h"

#include <stdio.h>

using namespace ngp::cmdlist;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: FAILED: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

struct alignas(8) Arg24 { uint64_t a; uint32_t b; float c; uint8_t d; };
struct alignas(16) Arg900 { unsigned char bytes[912]; };   // ~900 bytes by value, as BinPlan / OptTensors are passed
struct alignas(64) Arg64 { unsigned char bytes[64]; };
static_assert(sizeof(Arg24) == 24, "24-byte argument");

static int fake_kernel_a, fake_kernel_b, fake_kernel_c;   // their addresses stand for kernel handles

struct Expect {
    const void* fn;
    uint32_t lds;
    std::vector<std::vector<unsigned char>> args;
    std::vector<size_t> aligns;
};
struct Stub {
    std::vector<Expect> expect;   // the launches, in order
    size_t next = 0;
    int launches = 0, memsets = 0, memcpys = 0, marks = 0, fail_at = -1;
    std::vector<uint32_t> mark_positions;   // launches + memsets + memcpys issued before each mark
};
static int stub_launch(void* ctx, const void* fn, Dim grid, Dim block, void** args, uint32_t lds, void* stream) {
    Stub* s = static_cast<Stub*>(ctx);
    if (s->fail_at == s->launches) return 1;
    if (s->next >= s->expect.size()) return 1;
    const Expect& e = s->expect[s->next++];
    if (fn != e.fn || lds != e.lds || grid.x != 7 || grid.y != 2 || grid.z != 1 || block.x != 256 || stream != (void*)s) return 1;
    for (size_t i = 0; i < e.args.size(); i++) {
        if ((uintptr_t)args[i] % e.aligns[i]) return 1;
        if (memcmp(args[i], e.args[i].data(), e.args[i].size())) return 1;
    }
    s->launches++;
    return 0;
}
static int stub_memset(void* ctx, void* dst, int value, size_t bytes, void*) {
    Stub* s = static_cast<Stub*>(ctx);
    s->memsets++;
    return !(dst == (void*)0x1000 && value == 0 && bytes == 4096);
}
static int stub_memcpy(void* ctx, void* dst, const void* src, size_t bytes, int kind, void*) {
    Stub* s = static_cast<Stub*>(ctx);
    s->memcpys++;
    return !(dst == (void*)0x2000 && src == (const void*)0x3000 && bytes == 12 && kind == 3);
}
static int stub_mark(void* ctx, uint32_t, void*) {
    Stub* s = static_cast<Stub*>(ctx);
    s->marks++;
    s->mark_positions.push_back((uint32_t)(s->launches + s->memsets + s->memcpys));
    return 0;
}

// record one launch the way common.h's helper does: pointers to the CALLER's copies, which die right after
template <typename... A>
static void record(List* l, Stub& s, const void* fn, uint32_t lds, A... a) {
    void* argv[] = {static_cast<void*>(&a)..., nullptr};
    const size_t sizes[] = {sizeof(A)..., 0}, aligns[] = {alignof(A)..., 0};
    Expect e{fn, lds, {std::vector<unsigned char>((unsigned char*)&a, (unsigned char*)&a + sizeof(A))...}, {alignof(A)...}};
    s.expect.push_back(e);
    l->record_launch(fn, "fake", Dim{7, 2, 1}, Dim{256, 1, 1}, lds, (uint32_t)sizeof...(A), argv, sizes, aligns);
    int scrub[] = {(memset((void*)&a, 0xEE, sizeof(A)), 0)..., 0};   // the list must not point at these
    (void)scrub;
}

static bool refused_with(int rc, const char* message) {
    if (rc != REFUSED || strcmp(last_error(), message)) {
        fprintf(stderr, "rc %d, message \"%s\", expected \"%s\"\n", rc, last_error(), message);
        return false;
    }
    return true;
}

int main() {
    Stub stub;
    const Launcher launcher{&stub, stub_launch, stub_memset, stub_memcpy, stub_mark};
    void* const stream = &stub;
    uint32_t n = 99, k = 0;

    // ---- refusals on handles that are not lists ----
    List* l = nullptr;
    CHECK(refused_with(create(nullptr), "ngp_cmdlist_create: out_list is NULL"));
    CHECK(refused_with(begin(nullptr), "ngp_cmdlist_begin: the list is NULL or was destroyed"));
    CHECK(refused_with(end(reinterpret_cast<List*>(&stub)), "ngp_cmdlist_end: the list is NULL or was destroyed"));
    CHECK(create(&l) == OK && l);
    CHECK(count(l, &n) == OK && n == 0);
    CHECK(refused_with(end(l), "ngp_cmdlist_end: no recording is open on this thread"));
    CHECK(refused_with(replay(l, launcher, stream), "ngp_cmdlist_replay: the list is empty"));
    CHECK(refused_with(find_mark(l, 5, &k), "ngp_cmdlist_wait_mark: mark 5 was never recorded"));

    // ---- record: 1, 8, 24 and ~900 bytes at mixed alignments, a 64-byte aligned block, enough launches to cross storage chunks ----
    CHECK(begin(l) == OK && recording() == l);
    List* other = nullptr;
    CHECK(create(&other) == OK);
    CHECK(refused_with(begin(other), "ngp_cmdlist_begin: a recording is already open on this thread"));
    CHECK(refused_with(end(other), "ngp_cmdlist_end: another list is recording on this thread"));
    CHECK(refused_with(replay(l, launcher, stream), "ngp_cmdlist_replay: the list is still recording"));
    CHECK(refused_with(find_mark(l, 5, &k), "ngp_cmdlist_wait_mark: the list is still recording"));
    CHECK(refused_with(destroy(l), "ngp_cmdlist_destroy: the list is still recording"));
    Arg24 a24{0x0123456789abcdefull, 77u, 1.5f, 9};
    Arg900 a900;
    for (size_t i = 0; i < sizeof(a900.bytes); i++) a900.bytes[i] = (unsigned char)(i * 7 + 3);
    Arg64 a64;
    for (size_t i = 0; i < sizeof(a64.bytes); i++) a64.bytes[i] = (unsigned char)(255 - i);
    record(l, stub, &fake_kernel_a, 0u, (unsigned char)0x5a, (uint64_t)0x1122334455667788ull, a24, a900);
    CHECK(mark(l, 5, -1) == OK);                      // behind the first launch
    l->record_memset((void*)0x1000, 0, 4096);
    record(l, stub, &fake_kernel_b, 1024u, true, a900, (char)3, (double)2.25, (uint16_t)513, a64, (const void*)&stub);
    l->record_memcpy((void*)0x2000, (const void*)0x3000, 12, 3);
    for (int i = 0; i < 40; i++) {                    // 40 x ~1.8 KB: several storage chunks
        a900.bytes[5] = (unsigned char)i;
        record(l, stub, &fake_kernel_c, (uint32_t)i, (unsigned char)i, a900, (uint32_t)(i * 1000), a900, a24);
    }
    CHECK(refused_with(mark(l, 5, -1), "ngp_cmdlist_mark: mark 5 exists already"));
    CHECK(refused_with(mark(l, 6, 1000), "ngp_cmdlist_mark: position 1000 is past the end of the list"));
    CHECK(end(l) == OK && recording() == nullptr);
    CHECK(mark(l, 9, 3) == OK);                       // on the closed list: behind launch, memset, launch
    CHECK(mark(l, 11, -1) == OK);                     // the end
    CHECK(refused_with(begin(l), "ngp_cmdlist_begin: the list has been recorded already (a list is recorded once)"));
    CHECK(count(l, &n) == OK && n == 44);
    CHECK(find_mark(l, 9, &k) == OK && k == 1);
    CHECK(refused_with(find_mark(l, 6, &k), "ngp_cmdlist_wait_mark: mark 6 was never recorded"));

    // ---- replay twice: the stub compares every argument with what was recorded ----
    for (int pass = 1; pass <= 2; pass++) {
        stub.next = 0;
        stub.mark_positions.clear();
        CHECK(replay(l, launcher, stream) == OK);
        CHECK(stub.launches == 42 * pass && stub.memsets == pass && stub.memcpys == pass && stub.marks == 3 * pass);
        CHECK(stub.mark_positions.size() == 3 && stub.mark_positions[0] == 1u + 44u * (pass - 1) && stub.mark_positions[1] == 3u + 44u * (pass - 1) &&
              stub.mark_positions[2] == 44u * pass);
    }
    // a launcher that fails ends the replay there and says so
    stub.next = 0;
    stub.fail_at = stub.launches + 1;
    CHECK(replay(l, launcher, stream) == LAUNCHER_FAILED && !strcmp(last_error(), "ngp_cmdlist_replay: an operation of the list could not be issued"));
    stub.fail_at = -1;

    // ---- a list that was poisoned while it recorded, an argument the storage cannot hold ----
    CHECK(begin(other) == OK);
    record(other, stub, &fake_kernel_a, 0u, (uint32_t)1);
    other->poison();
    CHECK(end(other) == OK);
    CHECK(refused_with(replay(other, launcher, stream), "ngp_cmdlist_replay: the list is unusable: an entry failed while it was recording"));
    CHECK(refused_with(find_mark(other, 1, &k), "ngp_cmdlist_wait_mark: mark 1 was never recorded"));
    List* third = nullptr;
    CHECK(create(&third) == OK && begin(third) == OK);
    {
        char big = 0;
        void* argv[] = {&big};
        const size_t sizes[] = {1}, aligns[] = {128};   // over-aligned: refused, not misplaced
        third->record_launch(&fake_kernel_a, "fake", Dim{1, 1, 1}, Dim{1, 1, 1}, 0, 1, argv, sizes, aligns);
    }
    CHECK(end(third) == OK && third->poisoned() && third->count() == 0);

    // ---- destroy; a destroyed handle is refused everywhere ----
    CHECK(destroy(l) == OK && destroy(other) == OK && destroy(third) == OK);
    CHECK(refused_with(destroy(l), "ngp_cmdlist_destroy: the list is NULL or was destroyed"));
    CHECK(refused_with(count(l, &n), "ngp_cmdlist_count: the list is NULL or was destroyed"));
    CHECK(refused_with(replay(l, launcher, stream), "ngp_cmdlist_replay: the list is NULL or was destroyed"));
    CHECK(refused_with(find_mark(l, 5, &k), "ngp_cmdlist_wait_mark: the list is NULL or was destroyed"));
    CHECK(refused_with(mark(l, 1, -1), "ngp_cmdlist_mark: the list is NULL or was destroyed"));
    printf("cmdlist_selftest: ok (%d launches replayed)\n", stub.launches);
    return 0;
}
