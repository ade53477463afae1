// The C entries of the native command list (include/ngp_hip.h: ngp_cmdlist_*) and its HIP launcher.  Storage, packing, marks and every
// refusal live in cmdlist_core.h, which makes no HIP call; this file adds what touches the device: hipLaunchKernel / hipMemsetAsync /
// hipMemcpyAsync for the recorded operations and one list-owned event (timing disabled) per mark.
#include "common.h"
#include <unordered_map>

namespace ngp {
namespace {

using cmdlist::Dim;
using cmdlist::List;

struct Events {
    std::vector<hipEvent_t> ev;   // by mark index; created by the first replay that reaches the mark
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
// the events of the live lists (a list is replayed by one thread at a time; the table itself is shared)
std::mutex g_events_mutex;
std::unordered_map<const List*, Events*>& events_table() {
    static std::unordered_map<const List*, Events*> t;
    return t;
}
Events* events_of(const List* l, bool create) {
    std::lock_guard<std::mutex> g(g_events_mutex);
    auto& t = events_table();
    auto it = t.find(l);
    if (it != t.end()) return it->second;
    return create ? (t[l] = new Events()) : nullptr;
}

int hip_launch(void*, const void* fn, Dim g, Dim b, void** args, uint32_t lds, void* st) {
    return hipLaunchKernel(fn, dim3(g.x, g.y, g.z), dim3(b.x, b.y, b.z), args, lds, static_cast<hipStream_t>(st)) != hipSuccess;
}
int hip_memset(void*, void* dst, int value, size_t bytes, void* st) { return hipMemsetAsync(dst, value, bytes, static_cast<hipStream_t>(st)) != hipSuccess; }
int hip_memcpy(void*, void* dst, const void* src, size_t bytes, int kind, void* st) {
    return hipMemcpyAsync(dst, src, bytes, static_cast<hipMemcpyKind>(kind), static_cast<hipStream_t>(st)) != hipSuccess;
}
int hip_mark(void* ctx, uint32_t k, void* st) {
    Events* e = static_cast<Events*>(ctx);
    if (e->ev.size() <= k) e->ev.resize(k + 1, nullptr);
    if (!e->ev[k] && hipEventCreateWithFlags(&e->ev[k], hipEventDisableTiming) != hipSuccess) return 1;
    return hipEventRecord(e->ev[k], static_cast<hipStream_t>(st)) != hipSuccess;
}

int refused(int rc) {
    set_error_message(cmdlist::last_error());
    return rc == cmdlist::LAUNCHER_FAILED ? NGP_ERR_LAUNCH : NGP_ERR_INVALID;
}

}  // namespace
}  // namespace ngp

using namespace ngp;

extern "C" int ngp_cmdlist_create(void** out_list) {
    List* l = nullptr;
    if (int rc = cmdlist::create(out_list ? &l : nullptr)) return refused(rc);
    *out_list = l;
    return NGP_OK;
}
extern "C" int ngp_cmdlist_begin(void* list) {
    const int rc = cmdlist::begin(static_cast<List*>(list));
    return rc ? refused(rc) : NGP_OK;
}
extern "C" int ngp_cmdlist_mark(void* list, uint32_t mark_id, int after) {
    const int rc = cmdlist::mark(static_cast<List*>(list), mark_id, after);
    return rc ? refused(rc) : NGP_OK;
}
extern "C" int ngp_cmdlist_end(void* list) {
    const int rc = cmdlist::end(static_cast<List*>(list));
    return rc ? refused(rc) : NGP_OK;
}
extern "C" int ngp_cmdlist_count(const void* list, uint32_t* out_count) {
    const int rc = cmdlist::count(static_cast<const List*>(list), out_count);
    return rc ? refused(rc) : NGP_OK;
}
extern "C" int ngp_cmdlist_entry_name(const void* list, uint32_t index, char* out_name, uint32_t out_bytes) {
    const List* l = static_cast<const List*>(list);
    if (!cmdlist::alive(l)) return refused(cmdlist::refuse("ngp_cmdlist_%s: the list is NULL or was destroyed", "entry_name"));
    const uint32_t n = l->count();
    NGP_REQUIRE(out_name && out_bytes, NGP_ERR_INVALID, "ngp_cmdlist_entry_name: out_name is NULL or has no room");
    NGP_REQUIRE(index < n, NGP_ERR_INVALID, "ngp_cmdlist_entry_name: index %u is past the end of the list (%u entries)", index, n);
    const cmdlist::Op& op = l->op(index);
    const char* name = op.kind == cmdlist::OP_MEMSET ? "memset" : op.kind == cmdlist::OP_MEMCPY ? "memcpy" : nullptr;
    if (!name) {
        name = hipKernelNameRefByPtr(op.fn, nullptr);   // the kernel's (mangled) symbol: what a timeline shows
        if (!name) name = op.name;
    }
    snprintf(out_name, out_bytes, "%s", name);
    return NGP_OK;
}
extern "C" int ngp_cmdlist_replay(void* list, ngp_stream_t stream) {
    List* l = static_cast<List*>(list);
    cmdlist::Launcher hip{nullptr, hip_launch, hip_memset, hip_memcpy, hip_mark};
    if (cmdlist::alive(l) && !l->marks().empty()) hip.ctx = events_of(l, true);
    const int rc = cmdlist::replay(l, hip, stream);
    return rc ? refused(rc) : NGP_OK;
}
extern "C" int ngp_cmdlist_wait_mark(void* list, uint32_t mark_id, ngp_stream_t stream) {
    const List* l = static_cast<const List*>(list);
    uint32_t k = 0;
    if (int rc = cmdlist::find_mark(l, mark_id, &k)) return refused(rc);
    Events* e = events_of(l, false);
    NGP_REQUIRE(e && k < e->ev.size() && e->ev[k], NGP_ERR_INVALID, "ngp_cmdlist_wait_mark: the list has not been replayed since mark %u was set", mark_id);
    const hipError_t err = hipStreamWaitEvent(as_stream(stream), e->ev[k], 0);
    NGP_REQUIRE(err == hipSuccess, NGP_ERR_LAUNCH, "ngp_cmdlist_wait_mark: hipStreamWaitEvent failed: %s", hipGetErrorString(err));
    return NGP_OK;
}
extern "C" int ngp_cmdlist_destroy(void* list) {
    List* l = static_cast<List*>(list);
    if (int rc = cmdlist::destroy(l)) return refused(rc);
    Events* e = nullptr;
    {
        std::lock_guard<std::mutex> g(g_events_mutex);
        auto it = events_table().find(l);
        if (it != events_table().end()) {
            e = it->second;
            events_table().erase(it);
        }
    }
    delete e;
    return NGP_OK;
}
