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

// Split-K factor of an [m, n] result over k reduction rows (the encoder layers' GEMMs, the sequence decoder's dW): these GEMMs
// have few 64x64 output tiles and are bound by the latency of the K walk (one staged chunk per iteration), so K is cut until
// ~768 workgroups (3 per CU, co-resident) with at least 64 reduction rows each.  Whoever sizes slabs and whoever fills them
// both ask this one function.
__attribute__((visibility("hidden"))) inline int splits_for(int m, int n, int k) {
    static const int target = env_int("UMLH_ENC_SPLIT_WGS", 768);
    const long long tiles = (long long)((m + 63) / 64) * ((n + 63) / 64);
    if (k < 128 || tiles >= target) return 1;
    long long s = (target + tiles - 1) / tiles;
    if (s > k / 64) s = k / 64;
    if (s > 32) s = 32;
    return (int)(s < 1 ? 1 : s);
}
// rows per chunk of the column-sum partials over M rows: <= 64 row chunks of >= 64 rows
inline int row_chunk(long long M) { long long c = (M + 63) / 64; return (int)(c < 64 ? 64 : c); }

// the optimizer constants of one step (umlh_api.cpp): the head step and the standalone optimizer entry points
OptArgs make_opt(const umlh_config_t& c, const umlh_hyper_t& hy) __attribute__((visibility("hidden")));
