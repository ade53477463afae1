// libngp_hip.so runtime glue: thread-local error message, ABI/arch queries.
#include "common.h"
#include <string>

namespace ngp {
static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (cmdlist::List* l = cmdlist::recording()) l->poison();   // an entry failed while a list records: the list holds half a chain
}
void set_error_message(const char* message) { g_last_error = message; }

// the row bound armed on the calling thread (ngp_training_row_bound, include/ngp_hip.h); NULL: none
static thread_local const uint32_t* g_row_bound = nullptr;
const uint32_t* armed_row_bound() { return g_row_bound; }
}  // namespace ngp

extern "C" int ngp_training_row_bound(const uint32_t* rows_dev) {
    ngp::g_row_bound = rows_dev;
    return NGP_OK;
}

extern "C" const char* ngp_last_error(void) { return ngp::g_last_error.c_str(); }
extern "C" int ngp_abi_version(void) { return 11; }
extern "C" const char* ngp_target_arch(void) { return "gfx950"; }
