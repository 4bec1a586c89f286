// Shared by every source of libv3d_recon.so (all of csrc_recon/*.hip, directly or through bvh_walk.h and mesh_lists.h): the host helpers
// behind every entry (return codes, the one error string behind v3d_recon_last_error(), the launch check) and the two launch-shape constants
// that kernels and launches of these files agree on (TILE, NT).  No device functions.
#ifndef V3D_RECON_HOST_H
#define V3D_RECON_HOST_H
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

constexpr int TILE = 16;           // pixels on a side of a screen tile (kernels and their launches)
constexpr int NT = 256;            // threads per block everywhere (4 waves)
constexpr int RC_OK = 0, RC_ARG = -1, RC_LAUNCH = -2;

namespace recon_host {

inline thread_local char g_err[512] = "";      // (C++17 inline variable: one string per thread for the whole library)

inline void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return RC_LAUNCH;
    }
    return RC_OK;
}

inline unsigned nblk(long long n) { return (unsigned)((n + NT - 1) / NT); }

}  // namespace recon_host

using recon_host::check_launch;
using recon_host::nblk;
using recon_host::set_error;

#define RECON_REQUIRE(cond, ...)      \
    do {                              \
        if (!(cond)) {                \
            set_error(__VA_ARGS__);   \
            return RC_ARG;            \
        }                             \
    } while (0)

#endif
