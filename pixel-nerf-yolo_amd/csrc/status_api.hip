// The calling thread's error state (include/pnyolo.h pny_last_error) and the library's version.
#include <string>

#include "api_internal.h"

namespace pny {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int hip_fail(hipError_t e, const char* what) {
    g_err = std::string("HIP error: ") + hipGetErrorString(e) + " in " + what;
    return PNY_ERR_HIP;
}
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace pny

using namespace pny;

extern "C" {

int pny_version(void) { return PNY_ABI_VERSION; }
const char* pny_last_error(void) { return g_err.c_str(); }

}  // extern "C"
