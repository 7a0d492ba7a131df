// Singular values and effective rank of fp32 feature matrices for gfx950 (MultiBench/utilis.py:27-36, the diagnostic of
// MultiBench/train.py:386-389).  sigma(A) = sqrt(eig(A^T A)); the d x d Gram is accumulated in fp64 (a product of two fp32
// numbers is exact there), which is what makes the route as accurate as an fp32 SVD: see DESIGN section 12.
//
//   spectral_gram    a 64 x 64 tile of the upper triangle of G = sum over valid rows of a a^T for one row chunk: fp32 rows
//                    staged through LDS, converted on use, 4 x 4 fp64 FMA accumulators per thread, rows ascending.  Invalid
//                    rows (the sequence predicate t < clamp(len_b, 0, T) - drop_last) are staged as zeros: no compaction.
//   spectral_reduce  G[i][j] = G[j][i] = sum of the chunk slabs in chunk order
//   spectral_eig     one workgroup per matrix: scale by a power of two, Householder tridiagonalisation in place (global, L2
//                    resident), bisection on Sturm counts with one eigenvalue per thread and a fixed iteration count, then the
//                    top min(rows, d) values -> sigma = sqrt(max(lambda, 0)), p = sigma / sum sigma, exp(-sum p log(p + eps))
//
// No float atomics, every sum in a fixed order: results are bitwise reproducible for given arguments.
#include <cfloat>

#include "umlh_common.h"
#include "umlh_launch.h"

namespace {

constexpr int SP_MAX_D = 512;
constexpr int SP_TILE = 64;               // Gram tile edge
constexpr int SP_KR = 32;                 // rows staged per step
constexpr int SP_CHUNK_ROWS = 256;        // target rows of a chunk
constexpr int SP_MAX_CHUNKS = 128;        // chunks over all matrices of a call (at least one per matrix)
constexpr int SP_EIG_THREADS = 1024;
constexpr int SP_EIG_WAVES = SP_EIG_THREADS / 64;
constexpr int SP_BISECT_PASSES = 30;      // interval 4^-30 of the Gershgorin width: below an ulp of any eigenvalue that matters

inline long long align_up(long long x) { return (x + 255) / 256 * 256; }
template <typename T>
inline T* at(void* base, long long off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }

// How row r of matrix m is addressed: a + m * sm + (r / period) * so + (r % period) * si.  Dense: period = n (so unused);
// sequence block: one matrix of b * t_len rows, period = t_len, so = ldb, si = ldt.
struct RowMap {
    const float* a;
    long long sm, so, si;
    const long long* lengths;   // NULL: every row counts
    unsigned rows, period;
    int drop_last;
};

__device__ __forceinline__ int valid_len(const RowMap& m, unsigned outer) {
    if (!m.lengths) return (int)m.period - m.drop_last;
    long long l = m.lengths[outer];
    l = l < 0 ? 0 : (l > (long long)m.period ? (long long)m.period : l);
    return (int)l - m.drop_last;
}

__global__ __launch_bounds__(256) void spectral_gram(RowMap map, int d, int chunks, double* __restrict__ slabs) {
    __shared__ __align__(16) float sa[SP_KR][SP_TILE];
    __shared__ __align__(16) float sb[SP_KR][SP_TILE];
    // upper-triangular tile pair (ti <= tj) of blockIdx.x
    const int nt = (d + SP_TILE - 1) / SP_TILE;
    int ti = 0, rem = blockIdx.x;
    while (rem >= nt - ti) { rem -= nt - ti; ++ti; }
    const int tj = ti + rem;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lc = tid & 63, lr = tid >> 6;
    const unsigned chunk = blockIdx.y, mat = blockIdx.z;
    const unsigned r0 = (unsigned)((unsigned long long)map.rows * chunk / chunks);
    const unsigned r1 = (unsigned)((unsigned long long)map.rows * (chunk + 1) / chunks);
    const float* base = map.a + (long long)mat * map.sm;
    const int ca = ti * SP_TILE + lc, cb = tj * SP_TILE + lc;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (unsigned rs = r0; rs < r1; rs += SP_KR) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SP_KR / 4; ++q) {
            const unsigned r = rs + lr + 4 * q;
            float va = 0.f, vb = 0.f;
            if (r < r1) {
                const unsigned outer = r / map.period, inner = r - outer * map.period;
                if ((int)inner < valid_len(map, outer)) {
                    const float* row = base + (long long)outer * map.so + (long long)inner * map.si;
                    if (ca < d) va = row[ca];
                    if (cb < d) vb = row[cb];
                }
            }
            sa[lr + 4 * q][lc] = va;
            sb[lr + 4 * q][lc] = vb;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < SP_KR; ++k) {
            const float4 fa = *reinterpret_cast<const float4*>(&sa[k][ty * 4]);
            const float4 fb = *reinterpret_cast<const float4*>(&sb[k][tx * 4]);
            const double a4[4] = {(double)fa.x, (double)fa.y, (double)fa.z, (double)fa.w};
            const double b4[4] = {(double)fb.x, (double)fb.y, (double)fb.z, (double)fb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(a4[i], b4[j], acc[i][j]);
        }
    }
    double* slab = slabs + ((long long)mat * chunks + chunk) * d * d;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gi = ti * SP_TILE + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gj = tj * SP_TILE + tx * 4 + j;
            if (gi < d && gj < d) slab[(long long)gi * d + gj] = acc[i][j];
        }
    }
}

__global__ __launch_bounds__(256) void spectral_reduce(const double* __restrict__ slabs, int d, int chunks, double* __restrict__ g) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= d * d) return;
    const int i = idx / d, j = idx - i * d;
    if (i > j) return;
    const long long dd = (long long)d * d;
    const double* s = slabs + (long long)blockIdx.y * chunks * dd + idx;
    double v = 0.0;
    for (int c = 0; c < chunks; ++c) v += s[(long long)c * dd];
    double* gm = g + (long long)blockIdx.y * dd;
    gm[idx] = v;
    gm[(long long)j * d + i] = v;
}

// Sum over the wave in a fixed butterfly; every lane gets it.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct EigOut {
    double* erank;        // NULL or [batch]
    long long erank_ld;
    double* rows_out;     // NULL or one double (the sequence form)
    double* sv;           // NULL or [batch, sv_ld]
    int sv_ld;            // values written per matrix: min(rows, d) of them, then zeros up to sv_ld
    double eps;
};

__global__ __launch_bounds__(SP_EIG_THREADS) void spectral_eig(double* __restrict__ gall, int d, RowMap map, int n_outer, EigOut out) {
    __shared__ double v[SP_MAX_D], w[SP_MAX_D], dg[SP_MAX_D], e2[SP_MAX_D], lam[SP_MAX_D];
    __shared__ double red[SP_EIG_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* A = gall + (long long)blockIdx.x * d * d;

    // valid rows: an integer sum (any order gives the same value)
    long long cnt = 0;
    for (int b = tid; b < n_outer; b += SP_EIG_THREADS) {
        const int l = valid_len(map, (unsigned)b);
        cnt += l > 0 ? l : 0;
    }
    // power-of-two scale from the largest diagonal entry (G is PSD: no entry exceeds it); a NaN or Inf in a column of the
    // input shows on the diagonal and makes the whole spectrum NaN
    double mx = 0.0;
    for (int i = tid; i < d; i += SP_EIG_THREADS) {
        const double x = A[(long long)i * d + i];
        mx = (x - x == 0.0) ? (x > mx ? x : mx) : INFINITY;
    }
    red[tid] = mx;
    __shared__ long long cred[SP_EIG_THREADS];
    cred[tid] = cnt;
    __syncthreads();
    for (int s = SP_EIG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[tid] = red[tid] > red[tid + s] ? red[tid] : red[tid + s];
            cred[tid] += cred[tid + s];
        }
        __syncthreads();
    }
    mx = red[0];
    const long long rows = cred[0];
    const bool degenerate = !(mx > 0.0 && mx <= DBL_MAX);      // all-zero matrix (every sigma exactly 0), or not finite
    const int ex = degenerate ? 0 : ilogb(mx);
    const double scale = ldexp(1.0, -ex), unscale = ldexp(1.0, ex);
    for (int idx = tid; idx < d * d; idx += SP_EIG_THREADS) A[idx] *= scale;
    __syncthreads();

    // Householder tridiagonalisation (LAPACK dsytd2 on full symmetric storage): step k annihilates row k right of k + 1
    for (int k = 0; k + 2 < d && !degenerate; ++k) {
        const int m = d - k - 1;
        const double* x = A + (long long)k * d + k + 1;
        double ss = 0.0;
        for (int i = 1 + lane; i < m; i += 64) ss = fma(x[i], x[i], ss);
        ss = wave_sum(ss);                                     // every wave forms the same value
        const double alpha = x[0];
        double tau = 0.0, beta = alpha, inv = 0.0;
        if (ss > 0.0) {
            beta = -copysign(sqrt(alpha * alpha + ss), alpha);
            tau = (beta - alpha) / beta;
            inv = 1.0 / (alpha - beta);
        }
        for (int i = tid; i < m; i += SP_EIG_THREADS) v[i] = i == 0 ? 1.0 : x[i] * inv;
        if (tid == 0) { dg[k] = A[(long long)k * d + k]; e2[k] = beta; }
        __syncthreads();
        if (tau != 0.0) {                                      // uniform over the workgroup
            const double* T = A + (long long)(k + 1) * d + k + 1;
            // p = tau * T v, four rows per wave in flight
            for (int r = wave * 4; r < m; r += SP_EIG_WAVES * 4) {
                double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
                const double* t0 = T + (long long)r * d;
                const bool h1 = r + 1 < m, h2 = r + 2 < m, h3 = r + 3 < m;
                for (int c = lane; c < m; c += 64) {
                    const double vc = v[c];
                    s0 = fma(t0[c], vc, s0);
                    if (h1) s1 = fma(t0[d + c], vc, s1);
                    if (h2) s2 = fma(t0[2 * d + c], vc, s2);
                    if (h3) s3 = fma(t0[3 * d + c], vc, s3);
                }
                s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
                if (lane == 0) {
                    w[r] = tau * s0;
                    if (h1) w[r + 1] = tau * s1;
                    if (h2) w[r + 2] = tau * s2;
                    if (h3) w[r + 3] = tau * s3;
                }
            }
            __syncthreads();
            double pv = 0.0;
            for (int i = lane; i < m; i += 64) pv = fma(w[i], v[i], pv);
            pv = wave_sum(pv);
            const double c2 = 0.5 * tau * pv;
            __syncthreads();                                   // every wave has read w before it changes
            for (int i = tid; i < m; i += SP_EIG_THREADS) w[i] = w[i] - c2 * v[i];
            __syncthreads();
            // T -= v w^T + w v^T
            for (int r = wave * 4; r < m; r += SP_EIG_WAVES * 4) {
                double* t0 = const_cast<double*>(T) + (long long)r * d;
                const int nr = m - r < 4 ? m - r : 4;
                for (int c = lane; c < m; c += 64) {
                    const double vc = v[c], wc = w[c];
                    for (int q = 0; q < nr; ++q) t0[(long long)q * d + c] -= fma(v[r + q], wc, w[r + q] * vc);
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (d >= 2) {
            dg[d - 2] = A[(long long)(d - 2) * d + d - 2];
            e2[d - 2] = A[(long long)(d - 2) * d + d - 1];
        }
        dg[d - 1] = A[(long long)d * d - 1];
        e2[d - 1] = 0.0;
    }
    __syncthreads();
    // Gershgorin interval and the pivot floor; e2 becomes the squared off-diagonal
    double lo = DBL_MAX, hi = -DBL_MAX, emax = 0.0;
    if (tid < d) {
        const double el = tid > 0 ? fabs(e2[tid - 1]) : 0.0, er = fabs(e2[tid]);
        lo = dg[tid] - el - er;
        hi = dg[tid] + el + er;
        emax = er * er;
    }
    __syncthreads();
    if (tid < d) e2[tid] = emax;
    red[tid] = lo;
    __syncthreads();
    for (int s = SP_EIG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] < red[tid + s] ? red[tid] : red[tid + s];
        __syncthreads();
    }
    const double glo = red[0];
    __syncthreads();
    red[tid] = hi;
    __syncthreads();
    for (int s = SP_EIG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] > red[tid + s] ? red[tid] : red[tid + s];
        __syncthreads();
    }
    const double ghi = red[0];
    __syncthreads();
    red[tid] = emax;
    __syncthreads();
    for (int s = SP_EIG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] > red[tid + s] ? red[tid] : red[tid + s];
        __syncthreads();
    }
    const double pivmin = DBL_MIN * (red[0] > 1.0 ? red[0] : 1.0);
    __syncthreads();
    // thread j: the j-th largest eigenvalue = ascending index d - 1 - j; count(x) = #eigenvalues < x
    if (tid < d) {
        const int want = d - tid;                              // smallest x with count(x) >= want
        const double span = ghi - glo, pad = 2.0 * DBL_EPSILON * (fabs(glo) > fabs(ghi) ? fabs(glo) : fabs(ghi)) + 2.0 * pivmin;
        double a = glo - pad - span * DBL_EPSILON, b = ghi + pad + span * DBL_EPSILON;
        for (int it = 0; it < SP_BISECT_PASSES && !degenerate; ++it) {   // three probes a pass: the interval shrinks 4x
            const double h = 0.5 * (a + b), m1 = 0.5 * (a + h), m3 = 0.5 * (h + b);
            double q1 = dg[0] - m1, q2 = dg[0] - h, q3 = dg[0] - m3;
            if (fabs(q1) < pivmin) q1 = -pivmin;
            if (fabs(q2) < pivmin) q2 = -pivmin;
            if (fabs(q3) < pivmin) q3 = -pivmin;
            int c1 = q1 < 0.0, c2 = q2 < 0.0, c3 = q3 < 0.0;
            for (int i = 1; i < d; ++i) {
                const double di = dg[i], ei = e2[i - 1];
                q1 = di - m1 - ei / q1;
                q2 = di - h - ei / q2;
                q3 = di - m3 - ei / q3;
                if (fabs(q1) < pivmin) q1 = -pivmin;
                if (fabs(q2) < pivmin) q2 = -pivmin;
                if (fabs(q3) < pivmin) q3 = -pivmin;
                c1 += q1 < 0.0;
                c2 += q2 < 0.0;
                c3 += q3 < 0.0;
            }
            if (c1 >= want) b = m1;
            else if (c2 >= want) { a = m1; b = h; }
            else if (c3 >= want) { a = h; b = m3; }
            else a = m3;
        }
        lam[tid] = degenerate ? (mx == 0.0 ? 0.0 : NAN) : 0.5 * (a + b) * unscale;
    }
    __syncthreads();
    // finalize: top min(rows, d)
    const int keep = rows < (long long)d ? (int)rows : d;
    double sg = 0.0;
    if (tid < keep) {
        const double l = lam[tid];
        sg = sqrt(l > 0.0 ? l : (l == l ? 0.0 : l));
    }
    if (out.sv && tid < out.sv_ld) out.sv[(long long)blockIdx.x * out.sv_ld + tid] = tid < keep ? sg : 0.0;
    if (out.rows_out && tid == 0) out.rows_out[0] = (double)rows;
    if (!out.erank) return;                                    // uniform
    red[tid] = sg;
    __syncthreads();
    for (int s = SP_EIG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    double term = 0.0;
    if (tid < keep) {
        const double p = sg / total;
        term = p * log(p + out.eps);
    }
    red[tid] = term;
    __syncthreads();
    for (int s = SP_EIG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) out.erank[(long long)blockIdx.x * out.erank_ld] = exp(-red[0]);
}

}  // namespace

extern "C" {

int umlh_spectral_chunks(int batch, long long n) {
    long long c = (n + SP_CHUNK_ROWS - 1) / SP_CHUNK_ROWS;
    const long long cap = SP_MAX_CHUNKS / batch > 1 ? SP_MAX_CHUNKS / batch : 1;
    c = c > cap ? cap : c;
    return (int)(c < 1 ? 1 : c);
}

unsigned long long umlh_spectral_bytes(int batch, long long n, int d) {
    const long long dd = (long long)d * d * 8;
    return (unsigned long long)(align_up(dd * batch * umlh_spectral_chunks(batch, n)) + align_up(dd * batch));
}

// Dense: period = rows = n, batch matrices `sm` apart.  Sequence block: batch = 1, rows = n_outer * period.
int umlh_spectral_launch(const float* a, int batch, long long rows, int period, long long sm, long long so, long long si,
                         const long long* lengths, int drop_last, int d, double eps, double* erank, double* rows_out, double* sv,
                         int sv_ld, void* scratch, hipStream_t st) {
    const int chunks = umlh_spectral_chunks(batch, rows);
    const long long dd = (long long)d * d * 8;
    double* slabs = at<double>(scratch, 0);
    double* g = at<double>(scratch, align_up(dd * batch * chunks));
    RowMap map{a, sm, so, si, lengths, (unsigned)rows, (unsigned)period, drop_last};
    const int nt = (d + SP_TILE - 1) / SP_TILE;
    hipLaunchKernelGGL(spectral_gram, dim3(nt * (nt + 1) / 2, chunks, batch), dim3(256), 0, st, map, d, chunks, slabs);
    hipLaunchKernelGGL(spectral_reduce, dim3((d * d + 255) / 256, batch), dim3(256), 0, st, slabs, d, chunks, g);
    EigOut out{erank, 1, rows_out, sv, sv_ld, eps};
    hipLaunchKernelGGL(spectral_eig, dim3(batch), dim3(SP_EIG_THREADS), 0, st, g, d, map, (int)(rows / period), out);
    return (int)hipGetLastError();
}

}  // extern "C"
