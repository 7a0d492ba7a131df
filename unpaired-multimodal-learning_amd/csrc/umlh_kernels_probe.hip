// The linear probes of the reference's MultiBench evaluate() (MultiBench/train.py:31-91,93-240) for gfx950: masked mean
// pooling, StandardScaler statistics, an L2-regularised binary logistic regression fitted on the device, and its score.
//
//   pb_masked_mean   out[b, :] = sum_{t < min(len_b, T)} z[b, t, :] / min(len_b, T): one fp32 chain per element, t ascending
//   pb_colsum        column sums (pass 0) / sums of squared deviations from the mean (pass 1) in double, per row chunk
//                    (colsum_chunk of umlh_gram.h)
//   pb_stats_final   fixed-order sum of the chunks -> mean | scale (population std, or 1 below 10 eps)
//   pb_init          w = 0, z = 0, f = N log 2
//   pb_residual      z += t_prev * u;  p = sigmoid(z);  r = p - y;  s = p (1 - p)
//   pb_grad          X~^T r per row chunk: 32-column tiles on v_mfma_f32_32x32x2_f32, flushed to double every 64 rows
//   pb_gram          X~^T diag(s) X~ per row chunk: upper-triangle 32x32 tiles on the f32 MFMA (mfma32_rows_tile of umlh_gram.h,
//                    the tile body of cka_cross, on the standardising loader)
//   pb_hess          chunks summed in double (fixed order, slab_total) + the ridge -> H, mirrored
//   pb_solve         g = sum of chunks + R w in double (fixed order); stop tests; Cholesky of H; delta = -H^-1 g
//   pb_matvec        u = X~ delta on the f32 MFMA (also the decision values and the integer hit count of the score)
//   pb_linesearch    sum_i log(1 + exp(-t_i (z_i + a u_i))) for a = 1, 1/2, ..., 2^-11, in double, per block
//   pb_update        fixed-order sums -> f(a); largest a with sufficient decrease; w += a delta; the relative-gain stop test
//
// X~ = [x, 1] is standardised on load when statistics are given ((x - mean) * (1 / scale) in double, rounded to fp32 once);
// no standardised copy exists.  The Hessian is inexact (fp32 products and accumulation): it only shapes the step.  Where
// the iteration stops is decided by the gradient and by the objective, both summed in double in a fixed order.  z is
// carried in double and advanced by the accepted step, so the objective the line search accepted is bitwise the objective
// of the next iterate: the recorded sequence never increases.  A fit is a fixed train of launches in stream order; after
// `halt` is set every remaining launch returns at its first instruction.  Nothing uses a float atomic, a grid barrier or
// a host read.
#include "umlh_common.h"
#include "umlh_gram.h"
#include "umlh_launch.h"
#include <cfloat>
#include <cmath>

namespace {

constexpr int PB_LS = 12;               // line-search candidates a = 2^-j
constexpr int PB_EBLOCKS = 1024;        // most workgroups of an element-wise pass
constexpr int PB_GCHUNKS = 512;         // most row chunks of the gradient
constexpr int PB_TARGET_WG = 1024;      // Gram: tiles x row chunks
constexpr int PB_STAT_CHUNKS = 64;      // row chunks of the column statistics
constexpr int PB_MAXD = 1024;
constexpr double PB_ARMIJO = 1e-4;
constexpr double PB_DEC_TOL = 8.0 * DBL_EPSILON;    // predicted decrease below 8 ulp of the objective: nothing left to gain
constexpr double PB_FTOL = 1e-11;                   // an accepted step that gained less than this (relative) was the last useful one:
                                                    // Newton's decrease is ~ lambda^2 / 2 and the next one ~ lambda^4
constexpr double PB_STALL_TOL = 1e-10;              // a failed line search counts as the floor only this close to it

struct ProbeState {
    int halt;            // != 0: every later launch of this fit returns at once
    int iter;            // accepted steps
    int pending;         // != 0: the step just taken was the last; the next gradient pass records this code and halts
    double f;            // objective at w
    double gd;           // g . delta
    double max_grad;     // max |g| at w
};

struct ProbeArgs {
    const float* x;
    const int* y;
    const double* stats;             // NULL or mean[d] | scale[d]
    long long n;
    int d, ldx, D;                   // D = d + 1 (the intercept column)
    int kind, max_iter;
    double inv_c, gtol;
    int eblocks, gchunks, nt, tiles, rchunks;
    ProbeState* st;
    double* w;                       // the iterate: the caller's coef[d + 1]
    double* delta;
    double* tstep;                   // [max_iter] accepted step lengths
    double* z;                       // [n] margins w . x~_i
    float *u, *r, *s;                // [n] X~ delta, p - y, p (1 - p)
    double* gpart;                   // [gchunks][D]
    double* lspart;                  // [eblocks][PB_LS]
    double* cross;                   // [tiles][rchunks][1024]
    double* H;                       // [D][D]
    umlh_probe_record_t* rec;
    double* objectives;              // NULL or [max_iter + 1]
};

__device__ __forceinline__ double pb_ridge(const ProbeArgs& g, int c) {
    return (c < g.d || g.kind == UMLH_PROBE_LIBLINEAR) ? g.inv_c : 0.0;
}

// column c of x~ at row r (r < n, c <= d): the feature, standardised when statistics are given, or the intercept's 1
__device__ __forceinline__ float pb_load(const float* __restrict__ x, const double* __restrict__ stats, long long r, int c, int d,
                                         int ldx) {
    if (c == d) return 1.f;
    const float v = x[r * (long long)ldx + c];
    if (!stats) return v;
    return (float)(((double)v - stats[c]) * (1.0 / stats[d + c]));
}

__device__ __forceinline__ void pb_record(const ProbeArgs& g, int converged) {
    ProbeState* st = g.st;
    st->halt = 1;
    g.rec->iterations = st->iter;
    g.rec->converged = converged;
    g.rec->max_grad = st->max_grad;
    g.rec->objective = st->f;
}

// ---- pooling ----
__global__ __launch_bounds__(256) void pb_masked_mean(const float* __restrict__ z, int B, int T, int Z, long long ldb, long long ldt,
                                                      const long long* __restrict__ lengths, float* __restrict__ out, int ldo) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * Z) return;
    const int b = (int)(idx / Z), c = (int)(idx % Z);
    long long len = lengths ? lengths[b] : T;
    len = len < 0 ? 0 : (len > T ? T : len);
    const float* p = z + b * ldb + c;
    float acc = 0.f;
    for (long long t = 0; t < len; ++t) acc += p[t * ldt];
    out[(long long)b * ldo + c] = acc / (float)len;       // len = 0: 0 / 0 = NaN, as the reference's mask arithmetic
}

// ---- StandardScaler statistics ----
__global__ __launch_bounds__(256) void pb_colsum(const float* __restrict__ x, long long n, int d, int ldx, int chunks,
                                                 const double* __restrict__ mean, double* __restrict__ partial) {
    colsum_chunk([=](int c) {
        const double m = mean ? mean[c] : 0.0;
        return [=](long long r) {
            const double v = (double)x[r * ldx + c] - m;
            return mean ? v * v : v;
        };
    }, d, n, chunks, partial);
}

__global__ __launch_bounds__(256) void pb_stats_final(const double* __restrict__ partial, long long n, int d, int chunks, int pass,
                                                      double* __restrict__ stats) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    const double s = chunk_total(partial, chunks, d, c);
    if (pass == 0) {
        stats[c] = s / (double)n;
    } else {
        const double sd = sqrt(s / (double)n);
        stats[d + c] = sd < 10.0 * DBL_EPSILON ? 1.0 : sd;     // sklearn's _handle_zeros_in_scale
    }
}

// ---- fit ----
__global__ __launch_bounds__(256) void pb_init(ProbeArgs g) {
    const int tid = threadIdx.x;
    const long long rs = (long long)blockIdx.x * g.n / g.eblocks, re = (long long)(blockIdx.x + 1) * g.n / g.eblocks;
    for (long long i = rs + tid; i < re; i += 256) g.z[i] = 0.0;
    if (blockIdx.x != 0) return;
    for (int c = tid; c < g.D; c += 256) g.w[c] = 0.0;
    const double f0 = (double)g.n * 0.6931471805599453;
    if (g.objectives)
        for (int k = tid; k <= g.max_iter; k += 256) g.objectives[k] = k ? __builtin_nan("") : f0;
    if (tid == 0) {
        g.st->halt = 0;
        g.st->iter = 0;
        g.st->pending = 0;
        g.st->f = f0;
        g.st->gd = 0.0;
        g.st->max_grad = 0.0;
        g.rec->iterations = 0;
        g.rec->converged = 0;
        g.rec->max_grad = 0.0;
        g.rec->objective = f0;
    }
}

__global__ __launch_bounds__(256) void pb_residual(ProbeArgs g, int k) {
    if (g.st->halt) return;
    const double t = k > 0 ? g.tstep[k - 1] : 0.0;
    const long long rs = (long long)blockIdx.x * g.n / g.eblocks, re = (long long)(blockIdx.x + 1) * g.n / g.eblocks;
    for (long long i = rs + threadIdx.x; i < re; i += 256) {
        double z = g.z[i];
        if (k > 0) {
            z += t * (double)g.u[i];
            g.z[i] = z;
        }
        const double p = 1.0 / (1.0 + exp(-z));
        g.r[i] = (float)(p - (double)g.y[i]);
        g.s[i] = (float)(p * (1.0 - p));
    }
}

// Column tile blockIdx.x of X~^T r, rows of chunk blockIdx.y (whole 8-row groups).  Wave w takes the groups w, w+4, ...;
// lane half h supplies rows 4h + s to MFMA step s; B is r broadcast over the 32 output columns, so every column of the
// accumulator holds the tile's 32 sums.  The fp32 accumulator is flushed into double every 8 groups (64 rows).
__global__ __launch_bounds__(256) void pb_grad(ProbeArgs g) {
    if (g.st->halt) return;
    __shared__ double red[4][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c32 = lane & 31;
    const int cx = blockIdx.x * 32 + c32;
    const bool vx = cx < g.D, feat = cx < g.d;
    const double mean = (g.stats && feat) ? g.stats[cx] : 0.0, inv = (g.stats && feat) ? 1.0 / g.stats[g.d + cx] : 1.0;
    const long long ng = (g.n + 7) / 8;
    const long long gs = (long long)blockIdx.y * ng / g.gchunks, ge = (long long)(blockIdx.y + 1) * ng / g.gchunks;
    double accd[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) accd[q] = 0.0;
    f32x16 acc = {};
    int cnt = 0;
    for (long long grp = gs + wave; grp < ge; grp += 4) {
        float a[4], b[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long long r = grp * 8 + 4 * h + s;
            const bool vr = r < g.n;
            b[s] = vr ? g.r[r] : 0.f;
            float v = 0.f;
            if (vr && vx) v = feat ? (g.stats ? (float)(((double)g.x[r * g.ldx + cx] - mean) * inv) : g.x[r * g.ldx + cx]) : 1.f;
            a[s] = v;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
        if (++cnt == 8) {
#pragma unroll
            for (int q = 0; q < 16; ++q) { accd[q] += (double)acc[q]; acc[q] = 0.f; }
            cnt = 0;
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) accd[q] += (double)acc[q];
    if (c32 == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) red[wave][8 * (q >> 2) + 4 * h + (q & 3)] = accd[q];
    }
    __syncthreads();
    if (tid < 32 && blockIdx.x * 32 + tid < g.D)
        g.gpart[(long long)blockIdx.y * g.D + blockIdx.x * 32 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// Upper-triangle tile blockIdx.x = (ti <= tj) of X~^T diag(s) X~, rows of chunk blockIdx.y (whole 32-row blocks):
// mfma32_rows_tile (umlh_gram.h) on a = x~ s, b = x~; lane (h, c32) loads column c32 of the tile, rows 4h ..
__global__ __launch_bounds__(256) void pb_gram(ProbeArgs g) {
    if (g.st->halt) return;
    const int lane = threadIdx.x & 63, c32 = lane & 31;
    int ti, tj;
    tri_tile(blockIdx.x, g.nt, ti, tj);
    const int cx = ti * 32 + c32, cy = tj * 32 + c32;
    const bool vx = cx < g.D, vy = cy < g.D, fx = cx < g.d, fy = cy < g.d;
    const bool st = g.stats != nullptr;
    const double mx = (st && fx) ? g.stats[cx] : 0.0, ix = (st && fx) ? 1.0 / g.stats[g.d + cx] : 1.0;
    const double my = (st && fy) ? g.stats[cy] : 0.0, iy = (st && fy) ? 1.0 / g.stats[g.d + cy] : 1.0;
    long long rs, re;
    chunk_rows32(g.n, blockIdx.y, g.rchunks, rs, re);
    const auto x_tilde = [&](long long r, int c, bool feat, double m, double inv) {      // column c <= d of x~ at row r < n
        if (!feat) return 1.f;
        float v = g.x[r * g.ldx + c];
        if (st) {
            asm volatile("");                                      // keeps this a (uniform) branch: no fp64 work without statistics
            v = (float)(((double)v - m) * inv);
        }
        return v;
    };
    mfma32_rows_tile<false>([&](long long r0, float* a, float* b) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long long r = r0 + s;
            const bool vr = r < re;
            a[s] = vr ? ((vx ? x_tilde(r, cx, fx, mx, ix) : 0.f) * g.s[r]) : 0.f;
            b[s] = (vr && vy) ? x_tilde(r, cy, fy, my, iy) : 0.f;
        }
    }, rs, re, g.cross + ((long long)blockIdx.x * g.rchunks + blockIdx.y) * 1024);
}

__global__ __launch_bounds__(256) void pb_hess(ProbeArgs g) {
    if (g.st->halt) return;
    int ti, tj;
    tri_tile(blockIdx.x, g.nt, ti, tj);
    const double* p = g.cross + (long long)blockIdx.x * g.rchunks * 1024;
    for (int e = threadIdx.x; e < 1024; e += 256) {
        const int i = e >> 5, j = e & 31, ci = ti * 32 + i, cj = tj * 32 + j;
        if (ci >= g.D || cj >= g.D || ci > cj) continue;         // a diagonal tile keeps its upper half: H is symmetric by construction
        double v = slab_total(p, g.rchunks, e);
        if (ci == cj) v += pb_ridge(g, ci);
        g.H[(long long)ci * g.D + cj] = v;
        g.H[(long long)cj * g.D + ci] = v;
    }
}

// NaN-keeping max
__device__ __forceinline__ double pb_nanmax(double a, double b) { return (a != a || a > b) ? a : b; }

// One workgroup.  g = sum of the chunk partials (ascending) + R w; max |g| decides convergence.  Otherwise H = L L^T in place
// (left-looking; column j of L lives in row j of H, so the inner loop reads rows: lanes take consecutive i), two triangular
// solves for delta = -H^-1 g, and the stop test on the predicted decrease -g.delta / 2.
__global__ __launch_bounds__(1024) void pb_solve(ProbeArgs g, int last) {
    ProbeState* st = g.st;
    if (st->halt) return;
    __shared__ double gv[PB_MAXD + 8], yv[PB_MAXD + 8], red[1024], part[16][256];
    __shared__ double piv, diag0;
    __shared__ int stop;
    const int tid = threadIdx.x, D = g.D;
    double mg = 0.0;
    for (int c = tid; c < D; c += 1024) {
        double s = chunk_total(g.gpart, g.gchunks, D, c);
        s += pb_ridge(g, c) * g.w[c];
        gv[c] = s;
        mg = pb_nanmax(fabs(s), mg);
    }
    mg = block_reduce<1024>(mg, red, [](double a, double b) { return pb_nanmax(a, b); });
    if (tid == 0) {
        st->max_grad = mg;
        stop = 0;
        if (mg != mg) { pb_record(g, 0); stop = 1; }
        else if (mg <= g.gtol) { pb_record(g, 1); stop = 1; }
        else if (st->pending) { pb_record(g, st->pending); stop = 1; }
        else if (last) { pb_record(g, 0); stop = 1; }
    }
    __syncthreads();
    if (stop) return;
    double* H = g.H;
    const int lane = tid & 63, wave = tid >> 6;
    for (int j = 0; j < D; ++j) {
        // column j, 256 rows i at a time: wave w sums k = w, w + 16, ... < j for its 4 x 64 rows (five independent loads per
        // k keep the L2 latency covered), the 16 partial sums of a row are added in wave order
        for (int i0 = j; i0 < D; i0 += 256) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            int ic[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) ic[q] = min(i0 + lane + 64 * q, D - 1);
#pragma unroll 4
            for (int k = wave; k < j; k += 16) {
                const double* rk = H + (long long)k * D;
                const double lkj = rk[j];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] += rk[ic[q]] * lkj;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) part[wave][lane + 64 * q] = acc[q];
            __syncthreads();
            const int i = i0 + tid;
            if (tid < 256 && i < D) {
                double sum = 0.0;
#pragma unroll
                for (int w = 0; w < 16; ++w) sum += part[w][tid];
                const double h = H[(long long)j * D + i], v = h - sum;
                if (i == j) { diag0 = h; piv = v; }
                H[(long long)j * D + i] = v;
            }
            __syncthreads();
        }
        const double floorv = 1e-14 * fabs(diag0) + 1e-300;      // a lost pivot (saturated probabilities) only lengthens the step
        const double ljj = sqrt(piv > floorv ? piv : floorv);
        for (int i = j + tid; i < D; i += 1024) H[(long long)j * D + i] = (i == j) ? ljj : H[(long long)j * D + i] / ljj;
        __syncthreads();
    }
    for (int c = tid; c < D; c += 1024) yv[c] = -gv[c];
    __syncthreads();
    for (int j = 0; j < D; ++j) {                                  // L y = -g
        if (tid == 0) yv[j] /= H[(long long)j * D + j];
        __syncthreads();
        const double yj = yv[j];
        for (int i = j + 1 + tid; i < D; i += 1024) yv[i] -= H[(long long)j * D + i] * yj;
        __syncthreads();
    }
    for (int j = D - 1; j >= 0; --j) {                             // L^T delta = y
        if (tid == 0) yv[j] /= H[(long long)j * D + j];
        __syncthreads();
        const double dj = yv[j];
        for (int k = tid; k < j; k += 1024) yv[k] -= H[(long long)k * D + j] * dj;
        __syncthreads();
    }
    double gd = 0.0;
    for (int c = tid; c < D; c += 1024) {
        g.delta[c] = yv[c];
        gd += gv[c] * yv[c];
    }
    gd = block_reduce<1024>(gd, red, OpSum());
    if (tid == 0) {
        st->gd = gd;
        const double scale = fabs(st->f) > 1.0 ? fabs(st->f) : 1.0;
        if (!(gd < 0.0)) pb_record(g, gd == 0.0 ? 2 : 0);          // no descent direction: only the exact optimum counts
        else if (-gd <= PB_DEC_TOL * scale) pb_record(g, 2);
    }
}

// 32 rows per wave: lane half h supplies columns k0 + 4h + s to MFMA step s, B is v broadcast over the output columns.
// fit: out = u (halt != NULL).  score: out = decision values or NULL, y / hits optional.
__global__ __launch_bounds__(256) void pb_matvec(const float* __restrict__ x, const double* __restrict__ stats, long long n, int d,
                                                 int ldx, const double* __restrict__ v, const int* __restrict__ halt,
                                                 float* __restrict__ out, const int* __restrict__ y,
                                                 unsigned long long* __restrict__ hits) {
    if (halt && *halt) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c32 = lane & 31;
    const long long row0 = ((long long)blockIdx.x * 4 + wave) * 32;
    if (row0 >= n) return;
    const long long r = row0 + c32;
    const bool vr = r < n;
    f32x16 acc = {};
    for (int k0 = 0; k0 < d; k0 += 8) {
        float a[4], b[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int c = k0 + 4 * h + s;
            const bool vc = c < d;
            b[s] = vc ? (float)v[c] : 0.f;
            a[s] = (vc && vr) ? pb_load(x, stats, r, c, d, ldx) : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    }
    if (c32 != 0) return;
    const double bias = v[d];
    unsigned long long ok = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const long long row = row0 + 8 * (q >> 2) + 4 * h + (q & 3);
        if (row >= n) continue;
        const float dec = (float)((double)acc[q] + bias);
        if (out) out[row] = dec;
        if (y) ok += (unsigned long long)((dec > 0.f ? 1 : 0) == y[row]);
    }
    if (hits && ok) atomicAdd(hits, ok);                           // an integer count: exact in any order
}

__global__ __launch_bounds__(256) void pb_linesearch(ProbeArgs g) {
    if (g.st->halt) return;
    __shared__ double red[PB_LS][256];
    const int tid = threadIdx.x;
    const long long rs = (long long)blockIdx.x * g.n / g.eblocks, re = (long long)(blockIdx.x + 1) * g.n / g.eblocks;
    double acc[PB_LS];
#pragma unroll
    for (int j = 0; j < PB_LS; ++j) acc[j] = 0.0;
    for (long long i = rs + tid; i < re; i += 256) {
        const double sg = g.y[i] ? -1.0 : 1.0, z = g.z[i], u = (double)g.u[i];
        double a = 1.0;
#pragma unroll
        for (int j = 0; j < PB_LS; ++j) {
            const double m = sg * (z + a * u);                     // log(1 + exp(m)), overflow-safe
            acc[j] += (m > 0.0 ? m : 0.0) + log1p(exp(-fabs(m)));
            a *= 0.5;
        }
    }
#pragma unroll
    for (int j = 0; j < PB_LS; ++j) red[j][tid] = acc[j];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
            for (int j = 0; j < PB_LS; ++j) red[j][tid] += red[j][tid + w];
        __syncthreads();
    }
    if (tid < PB_LS) g.lspart[(long long)blockIdx.x * PB_LS + tid] = red[tid][0];
}

__global__ __launch_bounds__(256) void pb_update(ProbeArgs g, int k) {
    ProbeState* st = g.st;
    if (st->halt) return;
    __shared__ double red[3][256];
    __shared__ double loss[PB_LS];
    __shared__ double tsel;
    const int tid = threadIdx.x;
    double ww = 0.0, wd = 0.0, dd = 0.0;
    for (int c = tid; c < g.D; c += 256) {
        const double rc = pb_ridge(g, c), w = g.w[c], dl = g.delta[c];
        ww += rc * w * w;
        wd += rc * w * dl;
        dd += rc * dl * dl;
    }
    red[0][tid] = ww; red[1][tid] = wd; red[2][tid] = dd;
    if (tid < PB_LS) {
        double s = 0.0;
        for (int b = 0; b < g.eblocks; ++b) s += g.lspart[(long long)b * PB_LS + tid];
        loss[tid] = s;
    }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
            for (int j = 0; j < 3; ++j) red[j][tid] += red[j][tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const double f0 = st->f, gd = st->gd;
        double a = 1.0, t = 0.0, ft = f0;
        for (int j = 0; j < PB_LS; ++j, a *= 0.5) {
            const double fj = loss[j] + 0.5 * (red[0][0] + 2.0 * a * red[1][0] + a * a * red[2][0]);
            if (fj < f0 && fj <= f0 + PB_ARMIJO * a * gd) { t = a; ft = fj; break; }
        }
        tsel = t;
        const double scale = fabs(f0) > 1.0 ? fabs(f0) : 1.0;
        if (t != 0.0 && f0 - ft <= PB_FTOL * scale) st->pending = 2;
        if (t == 0.0) {          // no representable decrease along a Newton direction: the floor, if the direction promised next to nothing
            pb_record(g, -gd <= PB_STALL_TOL * scale ? 2 : 0);
        } else {
            st->f = ft;
            st->iter = k + 1;
            g.tstep[k] = t;
            if (g.objectives) g.objectives[k + 1] = ft;
        }
    }
    __syncthreads();
    const double t = tsel;
    if (t == 0.0) return;
    for (int c = tid; c < g.D; c += 256) g.w[c] += t * g.delta[c];
}

struct ProbePlan {
    int eblocks, gchunks, nt, tiles, rchunks;
    long long st, delta, tstep, z, u, r, s, gpart, lspart, cross, H, total;
};
static_assert(sizeof(ProbeState) <= 256, "the state region is one 256-byte unit");

ProbePlan probe_plan(long long n, int d, int max_iter) {
    ProbePlan p;
    const int D = d + 1;
    p.eblocks = (int)std::min<long long>(PB_EBLOCKS, (n + 255) / 256);
    p.gchunks = (int)std::min<long long>(PB_GCHUNKS, (n + 255) / 256);
    p.nt = (D + 31) / 32;
    p.tiles = tri_tiles(p.nt);
    const long long nb = (n + 31) / 32;
    p.rchunks = (int)std::max<long long>(1, std::min<long long>(PB_TARGET_WG / p.tiles, (nb + 3) / 4));
    ScratchLayout lay;
    p.st = lay.take(sizeof(ProbeState));
    p.delta = lay.take(8LL * D), p.tstep = lay.take(8LL * (max_iter + 1));
    p.z = lay.take(8LL * n);
    p.u = lay.take(4LL * n), p.r = lay.take(4LL * n), p.s = lay.take(4LL * n);
    p.gpart = lay.take(8LL * p.gchunks * D), p.lspart = lay.take(8LL * p.eblocks * PB_LS);
    p.cross = lay.take(8LL * 1024 * p.tiles * p.rchunks);
    p.H = lay.take(8LL * D * D);
    p.total = lay.end;
    return p;
}

}  // namespace

// ---- plans and launchers (validation is the caller's: umlh_ops.cpp) ----
extern "C" {

unsigned long long umlh_probe_fit_bytes(long long n, int d, int max_iter) { return (unsigned long long)probe_plan(n, d, max_iter).total; }
unsigned long long umlh_probe_stats_bytes(int d) { return (unsigned long long)align_up(8LL * PB_STAT_CHUNKS * d); }

int umlh_probe_launch_masked_mean(const float* z, int B, int T, int Z, long long ldb, long long ldt, const long long* lengths,
                                  float* out, int ldo, hipStream_t st) {
    const long long total = (long long)B * Z;
    hipLaunchKernelGGL(pb_masked_mean, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, z, B, T, Z, ldb, ldt, lengths, out, ldo);
    return (int)hipGetLastError();
}

// pass 0: stats[0, d) = column means; pass 1: stats[d, 2d) = column scales about those means
static void launch_stats_pass(int pass, const float* x, long long n, int d, int ldx, double* stats, void* scratch, hipStream_t st) {
    double* partial = at<double>(scratch, 0);
    const int chunks = (int)std::min<long long>(PB_STAT_CHUNKS, n);
    const dim3 grid((unsigned)((d + 63) / 64), (unsigned)chunks);
    hipLaunchKernelGGL(pb_colsum, grid, dim3(256), 0, st, x, n, d, ldx, chunks, pass ? (const double*)stats : nullptr, partial);
    hipLaunchKernelGGL(pb_stats_final, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, (const double*)partial, n, d, chunks, pass, stats);
}

int umlh_probe_launch_stats(const float* x, long long n, int d, int ldx, double* stats, void* scratch, hipStream_t st) {
    launch_stats_pass(0, x, n, d, ldx, stats, scratch, st);
    launch_stats_pass(1, x, n, d, ldx, stats, scratch, st);
    return (int)hipGetLastError();
}

int umlh_probe_launch_means(const float* x, long long n, int d, int ldx, double* mean, void* scratch, hipStream_t st) {
    launch_stats_pass(0, x, n, d, ldx, mean, scratch, st);
    return (int)hipGetLastError();
}

int umlh_probe_launch_fit(const float* x, long long n, int d, int ldx, const int* y, const double* stats, int kind, double c,
                          int max_iter, double gtol, double* coef, umlh_probe_record_t* rec, double* objectives, void* scratch,
                          hipStream_t st) {
    const ProbePlan p = probe_plan(n, d, max_iter);
    ProbeArgs g;
    g.x = x; g.y = y; g.stats = stats; g.n = n; g.d = d; g.ldx = ldx; g.D = d + 1;
    g.kind = kind; g.max_iter = max_iter; g.inv_c = 1.0 / c; g.gtol = gtol;
    g.eblocks = p.eblocks; g.gchunks = p.gchunks; g.nt = p.nt; g.tiles = p.tiles; g.rchunks = p.rchunks;
    g.st = at<ProbeState>(scratch, p.st);
    g.w = coef;
    g.delta = at<double>(scratch, p.delta); g.tstep = at<double>(scratch, p.tstep); g.z = at<double>(scratch, p.z);
    g.u = at<float>(scratch, p.u); g.r = at<float>(scratch, p.r); g.s = at<float>(scratch, p.s);
    g.gpart = at<double>(scratch, p.gpart); g.lspart = at<double>(scratch, p.lspart);
    g.cross = at<double>(scratch, p.cross); g.H = at<double>(scratch, p.H);
    g.rec = rec;
    g.objectives = objectives;
    const dim3 eb((unsigned)p.eblocks), b256(256);
    const unsigned mvb = (unsigned)((n + 127) / 128);
    hipLaunchKernelGGL(pb_init, eb, b256, 0, st, g);
    for (int k = 0; k <= max_iter; ++k) {
        hipLaunchKernelGGL(pb_residual, eb, b256, 0, st, g, k);
        hipLaunchKernelGGL(pb_grad, dim3((unsigned)p.nt, (unsigned)p.gchunks), b256, 0, st, g);
        if (k == max_iter) {
            hipLaunchKernelGGL(pb_solve, dim3(1), dim3(1024), 0, st, g, 1);
            break;
        }
        hipLaunchKernelGGL(pb_gram, dim3((unsigned)p.tiles, (unsigned)p.rchunks), b256, 0, st, g);
        hipLaunchKernelGGL(pb_hess, dim3((unsigned)p.tiles), b256, 0, st, g);
        hipLaunchKernelGGL(pb_solve, dim3(1), dim3(1024), 0, st, g, 0);
        hipLaunchKernelGGL(pb_matvec, dim3(mvb), b256, 0, st, x, stats, n, d, ldx, (const double*)g.delta, (const int*)&g.st->halt,
                           g.u, (const int*)nullptr, (unsigned long long*)nullptr);
        hipLaunchKernelGGL(pb_linesearch, eb, b256, 0, st, g);
        hipLaunchKernelGGL(pb_update, dim3(1), b256, 0, st, g, k);
    }
    return (int)hipGetLastError();
}

int umlh_probe_launch_score(const float* x, long long n, int d, int ldx, const double* stats, const double* coef, const int* y,
                            long long* correct, float* decision, hipStream_t st) {
    if (correct) {
        const hipError_t e = hipMemsetAsync(correct, 0, 8, st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(pb_matvec, dim3((unsigned)((n + 127) / 128)), dim3(256), 0, st, x, stats, n, d, ldx, coef, (const int*)nullptr,
                       decision, correct ? y : nullptr, (unsigned long long*)correct);
    return (int)hipGetLastError();
}

}  // extern "C"
