// What the host translation units (umlh_api.cpp, umlh_ops.cpp, umlh_encoder.cpp) share, and nothing else.  Host only: no
// .hip file, and no header a .hip file includes, includes this one.
#pragma once
#include <hip/hip_runtime.h>

#include "umlh.h"
#include "umlh_common.h"

// Writes the message behind umlh_last_error (one thread_local buffer, in umlh_api.cpp) and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3), visibility("hidden")));

#define HIPCHK(expr, what)                                                                  \
    do {                                                                                    \
        int _e = (expr);                                                                    \
        if (_e != 0) return fail(UMLH_E_HIP, "%s: HIP error %d (%s)", what, _e, hipGetErrorString((hipError_t)_e)); \
    } while (0)

#define RC(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

inline long long round_up(long long x, long long m) { return (x + m - 1) / m * m; }

// the optimizer constants of one step (umlh_api.cpp): the head step and the standalone optimizer entry points
OptArgs make_opt(const umlh_config_t& c, const umlh_hyper_t& hy) __attribute__((visibility("hidden")));
