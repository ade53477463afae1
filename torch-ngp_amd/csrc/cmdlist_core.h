// Native command list: storage, argument packing, marks and the refusals -- host C++ only, NO HIP call in this file.  Everything that touches
// the device goes through an injected Launcher (cmdlist.cpp: hipLaunchKernel / hipMemsetAsync / hipMemcpyAsync / hipEventRecord;
// tools/cmdlist_selftest.cpp: a stub that checks what it is handed), so the packing can run under the host sanitizers.
//
// A list is recorded on ONE thread between begin() and end(): while it is open there, the launch helpers of common.h append every stream
// operation the library's C entries issue (the operation is still issued as before).  replay() issues the recorded operations in order.
// A mark is a position in the list; replay() asks the launcher to record the mark's event there.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <unordered_set>
#include <vector>

namespace ngp {
namespace cmdlist {

struct Dim { uint32_t x, y, z; };
enum OpKind : uint32_t { OP_LAUNCH, OP_MEMSET, OP_MEMCPY };

struct Op {
    OpKind kind;
    const void* fn;        // OP_LAUNCH: the kernel's host handle;  OP_MEMCPY: the source
    const char* name;      // OP_LAUNCH: the kernel as the launch site spells it (a string literal)
    Dim grid, block;
    uint32_t lds;
    uint32_t n_args, first_arg;   // OP_LAUNCH: argv_[first_arg .. first_arg + n_args)
    void* dst;             // OP_MEMSET / OP_MEMCPY
    int value;             // OP_MEMSET: the byte;  OP_MEMCPY: the copy kind
    size_t bytes;
};

// what replay() calls; every function returns 0 on success (anything else ends the replay and is handed back)
struct Launcher {
    void* ctx;
    int (*launch)(void* ctx, const void* fn, Dim grid, Dim block, void** args, uint32_t lds, void* stream);
    int (*memset)(void* ctx, void* dst, int value, size_t bytes, void* stream);
    int (*memcpy)(void* ctx, void* dst, const void* src, size_t bytes, int kind, void* stream);
    int (*mark)(void* ctx, uint32_t mark_index, void* stream);   // record the event of marks_[mark_index] on the stream
};

enum { OK = 0, REFUSED = 1, LAUNCHER_FAILED = 2 };
constexpr size_t MAX_ALIGN = 64, CHUNK_BYTES = 16384;

struct Mark { uint32_t id, after; };   // the event is recorded behind `after` operations

class List;
inline thread_local List* t_open = nullptr;     // the list recording on this thread
inline thread_local char t_error[192] = "";     // message of the last refusal on this thread
inline const char* last_error() { return t_error; }

class List {
public:
    ~List() { for (char* c : chunks_) free(c); }

    // ---- recording (called by the launch helpers while this list is t_open) ----
    // a private copy of every argument, at the argument's own alignment
    void record_launch(const void* fn, const char* name, Dim grid, Dim block, uint32_t lds, uint32_t n_args, void* const* args, const size_t* sizes,
                       const size_t* aligns) {
        Op op{};
        op.kind = OP_LAUNCH; op.fn = fn; op.name = name; op.grid = grid; op.block = block; op.lds = lds;
        op.n_args = n_args; op.first_arg = (uint32_t)argv_.size();
        for (uint32_t i = 0; i < n_args; i++) {
            void* p = store(args[i], sizes[i], aligns[i]);
            if (!p) { poisoned_ = true; argv_.resize(op.first_arg); return; }
            argv_.push_back(p);
        }
        ops_.push_back(op);
    }
    void record_memset(void* dst, int value, size_t bytes) {
        Op op{};
        op.kind = OP_MEMSET; op.dst = dst; op.value = value; op.bytes = bytes;
        ops_.push_back(op);
    }
    void record_memcpy(void* dst, const void* src, size_t bytes, int kind) {
        Op op{};
        op.kind = OP_MEMCPY; op.dst = dst; op.fn = src; op.bytes = bytes; op.value = kind;
        ops_.push_back(op);
    }
    void poison() { poisoned_ = true; }

    bool open() const { return open_; }
    bool poisoned() const { return poisoned_; }
    uint32_t count() const { return (uint32_t)ops_.size(); }
    const Op& op(uint32_t i) const { return ops_[i]; }
    const std::vector<Mark>& marks() const { return marks_; }
    int mark_index(uint32_t id) const {
        for (size_t i = 0; i < marks_.size(); i++)
            if (marks_[i].id == id) return (int)i;
        return -1;
    }

    int replay(const Launcher& l, void* stream) {
        const uint32_t n = count();
        for (uint32_t i = 0; i <= n; i++) {
            for (size_t k = 0; k < marks_.size(); k++)
                if (marks_[k].after == i && l.mark(l.ctx, (uint32_t)k, stream)) return LAUNCHER_FAILED;
            if (i == n) break;
            const Op& op = ops_[i];
            int rc;
            if (op.kind == OP_LAUNCH) rc = l.launch(l.ctx, op.fn, op.grid, op.block, argv_.data() + op.first_arg, op.lds, stream);
            else if (op.kind == OP_MEMSET) rc = l.memset(l.ctx, op.dst, op.value, op.bytes, stream);
            else rc = l.memcpy(l.ctx, op.dst, op.fn, op.bytes, op.value, stream);
            if (rc) return LAUNCHER_FAILED;
        }
        return OK;
    }

private:
    friend int begin(List*);
    friend int end(List*);
    friend int mark(List*, uint32_t, int);

    void* store(const void* src, size_t size, size_t align) {
        if (align == 0 || align > MAX_ALIGN || (align & (align - 1)) || size > CHUNK_BYTES) return nullptr;
        size_t at = (used_ + align - 1) & ~(align - 1);
        if (chunks_.empty() || at + size > CHUNK_BYTES) {
            char* c = (char*)aligned_alloc(MAX_ALIGN, CHUNK_BYTES);
            if (!c) return nullptr;
            chunks_.push_back(c);
            at = 0;
        }
        char* p = chunks_.back() + at;
        if (size) memcpy(p, src, size);
        used_ = at + size;
        return p;
    }

    std::vector<Op> ops_;
    std::vector<void*> argv_;      // pointers into chunks_ (which never move)
    std::vector<char*> chunks_;
    size_t used_ = 0;
    std::vector<Mark> marks_;
    bool open_ = false, recorded_ = false, poisoned_ = false;
};

inline List* recording() { return t_open; }

// ---- the registry of live lists: a destroyed (or never created) handle is refused, not dereferenced ----
inline std::mutex& registry_mutex() { static std::mutex m; return m; }
inline std::unordered_set<const void*>& registry() { static std::unordered_set<const void*> s; return s; }
inline bool alive(const void* l) {
    if (!l) return false;
    std::lock_guard<std::mutex> g(registry_mutex());
    return registry().count(l) != 0;
}

inline int refuse(const char* fmt, const char* entry, unsigned v = 0) {
    snprintf(t_error, sizeof(t_error), fmt, entry, v);
    return REFUSED;
}
#define NGP_CMDLIST_ALIVE(l, entry) \
    if (!::ngp::cmdlist::alive(l)) return ::ngp::cmdlist::refuse("ngp_cmdlist_%s: the list is NULL or was destroyed", entry)

inline int create(List** out) {
    if (!out) return refuse("ngp_cmdlist_%s: out_list is NULL", "create");
    List* l = new List();
    std::lock_guard<std::mutex> g(registry_mutex());
    registry().insert(l);
    *out = l;
    return OK;
}
inline int begin(List* l) {
    NGP_CMDLIST_ALIVE(l, "begin");
    if (t_open) return refuse("ngp_cmdlist_%s: a recording is already open on this thread", "begin");
    if (l->open_ || l->recorded_) return refuse("ngp_cmdlist_%s: the list has been recorded already (a list is recorded once)", "begin");
    l->open_ = true;
    t_open = l;
    return OK;
}
// after < 0: the current end of the list (while it records: behind what has been issued so far), else behind `after` operations
inline int mark(List* l, uint32_t id, int after) {
    NGP_CMDLIST_ALIVE(l, "mark");
    if (l->open_ && t_open != l) return refuse("ngp_cmdlist_%s: the list is recording on another thread", "mark");
    if (after > (int)l->count()) return refuse("ngp_cmdlist_%s: position %u is past the end of the list", "mark", (unsigned)after);
    if (l->mark_index(id) >= 0) return refuse("ngp_cmdlist_%s: mark %u exists already", "mark", id);
    l->marks_.push_back(Mark{id, after < 0 ? l->count() : (uint32_t)after});
    return OK;
}
inline int end(List* l) {
    NGP_CMDLIST_ALIVE(l, "end");
    if (!t_open) return refuse("ngp_cmdlist_%s: no recording is open on this thread", "end");
    if (t_open != l) return refuse("ngp_cmdlist_%s: another list is recording on this thread", "end");
    l->open_ = false;
    l->recorded_ = true;
    t_open = nullptr;
    return OK;
}
inline int count(const List* l, uint32_t* out) {
    NGP_CMDLIST_ALIVE(l, "count");
    if (!out) return refuse("ngp_cmdlist_%s: out_count is NULL", "count");
    *out = l->count();
    return OK;
}
// the checks shared by replay and wait_mark
inline int replayable(const List* l, const char* entry) {
    if (l->open()) return refuse("ngp_cmdlist_%s: the list is still recording", entry);
    if (l->poisoned()) return refuse("ngp_cmdlist_%s: the list is unusable: an entry failed while it was recording", entry);
    if (l->count() == 0) return refuse("ngp_cmdlist_%s: the list is empty", entry);
    return OK;
}
inline int replay(List* l, const Launcher& launcher, void* stream) {
    NGP_CMDLIST_ALIVE(l, "replay");
    if (int rc = replayable(l, "replay")) return rc;
    if (l->replay(launcher, stream)) return refuse("ngp_cmdlist_%s: an operation of the list could not be issued", "replay"), LAUNCHER_FAILED;
    return OK;
}
// *out_index: the mark's index for the launcher's event table
inline int find_mark(const List* l, uint32_t id, uint32_t* out_index) {
    NGP_CMDLIST_ALIVE(l, "wait_mark");
    if (l->open()) return refuse("ngp_cmdlist_%s: the list is still recording", "wait_mark");
    const int k = l->mark_index(id);
    if (k < 0) return refuse("ngp_cmdlist_%s: mark %u was never recorded", "wait_mark", id);
    if (int rc = replayable(l, "wait_mark")) return rc;
    *out_index = (uint32_t)k;
    return OK;
}
inline int destroy(List* l) {
    NGP_CMDLIST_ALIVE(l, "destroy");
    if (l->open()) return refuse("ngp_cmdlist_%s: the list is still recording", "destroy");
    {
        std::lock_guard<std::mutex> g(registry_mutex());
        registry().erase(l);
    }
    delete l;
    return OK;
}

}  // namespace cmdlist
}  // namespace ngp
