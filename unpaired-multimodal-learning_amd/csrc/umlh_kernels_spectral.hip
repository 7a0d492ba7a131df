// Singular values and effective rank of fp32 feature matrices for gfx950 (MultiBench/utilis.py:27-36, the diagnostic of
// MultiBench/train.py:386-389).  sigma(A) = sqrt(eig(A^T A)); the d x d Gram is accumulated in fp64 (a product of two fp32
// numbers is exact there), which is what makes the route as accurate as an fp32 SVD: see DESIGN section 12.
//
//   spectral_gram    a 64 x 64 tile of the upper triangle of G = sum over valid rows of a a^T for one row chunk: fp32 rows
//                    staged through LDS, converted on use, 4 x 4 fp64 FMA accumulators per thread, rows ascending (gram64_tile
//                    of umlh_gram.h on the RowMap loader).  Invalid rows (the sequence predicate t < clamp(len_b, 0, T) -
//                    drop_last) are staged as zeros: no compaction.
//   spectral_reduce  G[i][j] = G[j][i] = sum of the chunk slabs in chunk order (slab_sum<true>)
//   spectral_eig     one workgroup per matrix: scale by a power of two, Householder tridiagonalisation in place (global, L2
//                    resident), bisection on Sturm counts with one eigenvalue per thread and a fixed iteration count, then the
//                    top min(rows, d) values -> sigma = sqrt(max(lambda, 0)), p = sigma / sum sigma, exp(-sum p log(p + eps))
//
// Principal subspaces and SVCCA (MultiBench/metrics.py:129-160 in closed form) on the same machinery:
//   subspace_gram         the two-operand form of spectral_gram on centred columns: Gc = (A - mu)^T (A - mu) or the cross-Gram
//                         (the same gram64_tile, fp64 staging); subspace_reduce_rect: its chunk sum (slab_sum<false>)
//   subspace_standardise  D Gc D with D_j = 1 / (std_j + 1e-8)
//   subspace_eig          spectral_eig's tridiagonalisation with the reflectors kept, bisection, inverse iteration for the q
//                         largest eigenvalues, the reflectors applied in reverse: top-q eigenpairs
//   svcca_tail            M = L_a^(-1/2) V_a^T C V_b L_b^(-1/2), rho = sqrt(eig(M^T M)), their mean
//
// No float atomics, every sum in a fixed order: results are bitwise reproducible for given arguments.
#include <cfloat>

#include "umlh_common.h"
#include "umlh_gram.h"
#include "umlh_launch.h"

namespace {

constexpr int SP_MAX_D = 512;
constexpr int SP_CHUNK_ROWS = 256;        // target rows of a chunk
constexpr int SP_MAX_CHUNKS = 128;        // chunks over all matrices of a call (at least one per matrix)
constexpr int SP_EIG_THREADS = 1024;
constexpr int SP_EIG_WAVES = SP_EIG_THREADS / 64;
constexpr int SP_BISECT_PASSES = 30;      // interval 4^-30 of the Gershgorin width: below an ulp of any eigenvalue that matters

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

// gram64_tile (umlh_gram.h) on the RowMap loader: upper-triangular tile pair blockIdx.x, row chunk blockIdx.y, matrix blockIdx.z
__global__ __launch_bounds__(256) void spectral_gram(RowMap map, int d, int chunks, double* __restrict__ slabs) {
    int ti, tj;
    tri_tile(blockIdx.x, (d + G64_TILE - 1) / G64_TILE, ti, tj);
    const unsigned chunk = blockIdx.y, mat = blockIdx.z;
    const unsigned r0 = (unsigned)((unsigned long long)map.rows * chunk / chunks);
    const unsigned r1 = (unsigned)((unsigned long long)map.rows * (chunk + 1) / chunks);
    const float* base = map.a + (long long)mat * map.sm;
    const auto cols = [&](int ca, int cb) {
        return [&map, base, ca, cb, d](unsigned r, float& va, float& vb) {
            const unsigned outer = r / map.period, inner = r - outer * map.period;
            if ((int)inner < valid_len(map, outer)) {
                const float* row = base + (long long)outer * map.so + (long long)inner * map.si;
                if (ca < d) va = row[ca];
                if (cb < d) vb = row[cb];
            }
        };
    };
    gram64_tile<float>(cols, ti, tj, r0, r1, slabs + ((long long)mat * chunks + chunk) * d * d, d, d);
}

// G[i][j] = G[j][i] = sum of the chunk slabs of matrix blockIdx.y in chunk order
__global__ __launch_bounds__(256) void spectral_reduce(const double* __restrict__ slabs, int d, int chunks, double* __restrict__ g) {
    const long long dd = (long long)d * d;
    slab_sum<true>(slabs + (long long)blockIdx.y * chunks * dd, dd, d, chunks, g + (long long)blockIdx.y * dd);
}

struct EigOut {
    double* erank;        // NULL or [batch]
    long long erank_ld;
    double* rows_out;     // NULL or one double (the sequence form)
    double* sv;           // NULL or [batch, sv_ld]
    int sv_ld;            // values written per matrix: min(rows, d) of them, then zeros up to sv_ld
    double eps;
};

// The three stages of the symmetric eigenvalue path, shared by spectral_eig, subspace_eig and svcca_tail: one workgroup of
// SP_EIG_THREADS threads calls each of them with uniform arguments; v, w, dg, e2, lam, red, cred are its LDS arrays.

// Scales A by a power of two taken from its largest diagonal entry and sums `cnt` over the workgroup (-> rows).  Returns
// whether the matrix is degenerate (all zero, or not finite); mx is the largest diagonal entry, ex its exponent.
__device__ __forceinline__ bool sp_prescale(double* A, int d, long long cnt, double* red, long long* cred, double& mx_out,
                                            long long& rows_out, int& ex_out) {
    const int tid = threadIdx.x;
    // power-of-two scale from the largest diagonal entry (G is PSD: no entry exceeds it); a NaN or Inf in a column of the
    // input shows on the diagonal and makes the whole spectrum NaN
    double mx = 0.0;
    for (int i = tid; i < d; i += SP_EIG_THREADS) {
        const double x = A[(long long)i * d + i];
        mx = (x - x == 0.0) ? (x > mx ? x : mx) : INFINITY;
    }
    red[tid] = mx;
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
    const double scale = ldexp(1.0, -ex);
    for (int idx = tid; idx < d * d; idx += SP_EIG_THREADS) A[idx] *= scale;
    __syncthreads();
    mx_out = mx;
    rows_out = rows;
    ex_out = ex;
    return degenerate;
}

// Householder tridiagonalisation (LAPACK dsytd2 on full symmetric storage): step k annihilates row k right of k + 1.  On
// return dg holds the diagonal and e2 the off-diagonal of T.  KEEP: reflector k (its leading 1 included) is left in row k
// right of the diagonal and its tau in taus[k], as LAPACK keeps them, for the reverse application in subspace_eig; the arithmetic of T is the same.
template <bool KEEP>
__device__ __forceinline__ void sp_tridiag(double* A, int d, bool degenerate, double* v, double* w, double* dg, double* e2,
                                           double* taus) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = 0; k + 2 < d && !degenerate; ++k) {
        const int m = d - k - 1;
        const double* x = A + (long long)k * d + k + 1;
        double ss = 0.0;
        for (int i = 1 + lane; i < m; i += 64) ss = fma(x[i], x[i], ss);
        ss = wave_sum_f64(ss);                                     // every wave forms the same value
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
        if (KEEP) {                                            // every wave is past its reads of row k
            for (int i = tid; i < m; i += SP_EIG_THREADS) A[(long long)k * d + k + 1 + i] = v[i];
            if (tid == 0) taus[k] = tau;
        }
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
                s0 = wave_sum_f64(s0); s1 = wave_sum_f64(s1); s2 = wave_sum_f64(s2); s3 = wave_sum_f64(s3);
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
            pv = wave_sum_f64(pv);
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
}

// Every eigenvalue of the tridiagonal (dg, e2) by bisection on Sturm counts, one per thread and a fixed pass count:
// lam[j] = the j-th largest, times `unscale`.  e2 becomes the squared off-diagonal.
__device__ __forceinline__ void sp_bisect(int d, bool degenerate, double mx, double unscale, const double* dg, double* e2,
                                          double* lam, double* red) {
    const int tid = threadIdx.x;
    // Gershgorin interval and the pivot floor; e2 becomes the squared off-diagonal
    double lo = DBL_MAX, hi = -DBL_MAX, emax = 0.0;
    if (tid < d) {
        const double el = tid > 0 ? fabs(e2[tid - 1]) : 0.0, er = fabs(e2[tid]);
        lo = dg[tid] - el - er;
        hi = dg[tid] + el + er;
        emax = er * er;
    }
    const double glo = block_reduce<SP_EIG_THREADS>(lo, red, OpMin());
    if (tid < d) e2[tid] = emax;                               // behind the reduction's barriers: every neighbour has read e2
    const double ghi = block_reduce<SP_EIG_THREADS>(hi, red, OpMax());
    const double emx = block_reduce<SP_EIG_THREADS>(emax, red, OpMax());
    const double pivmin = DBL_MIN * (emx > 1.0 ? emx : 1.0);
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
}

__global__ __launch_bounds__(SP_EIG_THREADS) void spectral_eig(double* __restrict__ gall, int d, RowMap map, int n_outer, EigOut out) {
    __shared__ double v[SP_MAX_D], w[SP_MAX_D], dg[SP_MAX_D], e2[SP_MAX_D], lam[SP_MAX_D];
    __shared__ double red[SP_EIG_THREADS];
    __shared__ long long cred[SP_EIG_THREADS];
    const int tid = threadIdx.x;
    double* A = gall + (long long)blockIdx.x * d * d;

    // valid rows: an integer sum (any order gives the same value)
    long long cnt = 0;
    for (int b = tid; b < n_outer; b += SP_EIG_THREADS) {
        const int l = valid_len(map, (unsigned)b);
        cnt += l > 0 ? l : 0;
    }
    double mx;
    long long rows;
    int ex;
    const bool degenerate = sp_prescale(A, d, cnt, red, cred, mx, rows, ex);
    sp_tridiag<false>(A, d, degenerate, v, w, dg, e2, nullptr);
    sp_bisect(d, degenerate, mx, ldexp(1.0, ex), dg, e2, lam, red);
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
    const double total = block_reduce<SP_EIG_THREADS>(sg, red, OpSum());
    double term = 0.0;
    if (tid < keep) {
        const double p = sg / total;
        term = p * log(p + out.eps);
    }
    const double ent = block_reduce<SP_EIG_THREADS>(term, red, OpSum());
    if (tid == 0) out.erank[(long long)blockIdx.x * out.erank_ld] = exp(-ent);
}


// ---- principal subspaces and SVCCA ----
constexpr int SS_MAX_Q = 64;              // eigenvectors per matrix: one lane of a wave each in the tridiagonal solves
constexpr int SS_INVIT_PASSES = 4;        // inverse-iteration solves per vector (LAPACK dstein stops after 3 as a rule)

struct Operand {
    const float* x;
    long long ld;
    const double* mu;     // column means
    int d;
};

// The two-operand form of spectral_gram on centred columns: a 64 x 64 tile of sum over the rows of one chunk of
// (a - mu_a)(b - mu_b)^T.  The centred values are fp64, so they are staged as fp64.  TRI: a == b, upper-triangular tile pairs
// only (spectral_reduce mirrors them); else every tile of the d_a x d_b product.
template <bool TRI>
__global__ __launch_bounds__(256) void subspace_gram(Operand A, Operand B, unsigned rows, int chunks, double* __restrict__ slabs) {
    int ti, tj;
    if (TRI) {
        tri_tile(blockIdx.x, (A.d + G64_TILE - 1) / G64_TILE, ti, tj);
    } else {
        const int ntb = (B.d + G64_TILE - 1) / G64_TILE;
        ti = blockIdx.x / ntb;
        tj = blockIdx.x - ti * ntb;
    }
    const unsigned chunk = blockIdx.y;
    const unsigned r0 = (unsigned)((unsigned long long)rows * chunk / chunks);
    const unsigned r1 = (unsigned)((unsigned long long)rows * (chunk + 1) / chunks);
    const auto cols = [&](int ca, int cb) {
        const double ma = ca < A.d ? A.mu[ca] : 0.0, mb = cb < B.d ? B.mu[cb] : 0.0;
        return [&A, &B, ca, cb, ma, mb](unsigned r, double& va, double& vb) {
            if (ca < A.d) va = (double)A.x[(long long)r * A.ld + ca] - ma;
            if (cb < B.d) vb = (double)B.x[(long long)r * B.ld + cb] - mb;
        };
    };
    gram64_tile<double>(cols, ti, tj, r0, r1, slabs + (long long)chunk * A.d * B.d, A.d, B.d);
}

// the rectangular form of spectral_reduce: c = sum of the chunk slabs in chunk order
__global__ __launch_bounds__(256) void subspace_reduce_rect(const double* __restrict__ slabs, long long total, int chunks,
                                                            double* __restrict__ c) {
    slab_sum<false>(slabs, total, 1, chunks, c);
}

// dst = D_r src D_c with D_j = 1 / (std_j + 1e-8), std_j = sqrt(Gc_jj / (n - 1)) read from the diagonals of the two centred
// Grams gr (rows) and gc (columns).  dst may be src when src is neither gr nor gc.
__global__ __launch_bounds__(256) void subspace_standardise(const double* src, int rows, int cols, const double* gr, const double* gc,
                                                            double nm1, double* dst) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * cols) return;
    const int i = idx / cols, j = idx - i * cols;
    const double di = 1.0 / (sqrt(gr[(long long)i * rows + i] / nm1) + 1e-8);
    const double dj = 1.0 / (sqrt(gc[(long long)j * cols + j] / nm1) + 1e-8);
    dst[idx] = (di * dj) * src[idx];
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

struct EigJob {
    double* g;            // [d, d], destroyed
    double* evals;        // [q]
    double* evecs;        // [d, q] row-major
    double* work;         // 4 * d * SS_MAX_Q doubles
    int d;
};
struct EigJobs {
    EigJob j[2];
    int q;
};

// component i of the start vector of eigenvector j: a fixed hash, uniform in (-1, 1), never zero
__device__ __forceinline__ double ss_start(int i, int j) {
    unsigned h = (unsigned)i * 2654435761u ^ ((unsigned)j + 1u) * 2246822519u;
    h ^= h >> 15; h *= 2654435761u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    return ((double)(h >> 8) + 0.5) * (1.0 / 8388608.0) - 1.0;
}

// Top-q eigenpairs of one symmetric matrix per workgroup: tridiagonalisation with the reflectors kept, bisection, inverse
// iteration on the tridiagonal (one vector per thread: Gaussian elimination with partial pivoting; vectors whose eigenvalues
// lie within 1e-3 |T| of each other are orthogonalised against the earlier ones of their cluster after every solve, LAPACK
// dstein's rule), the reflectors applied in reverse, the sign fixed by the largest component.
__global__ __launch_bounds__(SP_EIG_THREADS) void subspace_eig(EigJobs jobs) {
    __shared__ double v[SP_MAX_D], w[SP_MAX_D], dg[SP_MAX_D], e2[SP_MAX_D], lam[SP_MAX_D], taus[SP_MAX_D], ef[SP_MAX_D];
    __shared__ double red[SP_EIG_THREADS];
    __shared__ long long cred[SP_EIG_THREADS];
    __shared__ double shift[SS_MAX_Q];
    __shared__ int cstart[SS_MAX_Q];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const EigJob job = jobs.j[blockIdx.x];
    const int d = job.d, q = jobs.q;
    double* A = job.g;
    double mx;
    long long rows;
    int ex;
    const bool degenerate = sp_prescale(A, d, 0, red, cred, mx, rows, ex);
    sp_tridiag<true>(A, d, degenerate, v, w, dg, e2, taus);
    if (tid < d) ef[tid] = e2[tid];
    __syncthreads();
    sp_bisect(d, degenerate, mx, ldexp(1.0, ex), dg, e2, lam, red);
    if (tid < q) job.evals[tid] = lam[tid];
    if (degenerate) {                                          // uniform.  Zero matrix: unit vectors; not finite: NaN
        for (int idx = tid; idx < d * q; idx += SP_EIG_THREADS) {
            const int i = idx / q, j = idx - i * q;
            job.evecs[idx] = mx == 0.0 ? (i == j ? 1.0 : 0.0) : NAN;
        }
        return;
    }
    // |T|: the largest absolute row sum
    double rs = 0.0;
    if (tid < d) rs = fabs(dg[tid]) + (tid > 0 ? fabs(ef[tid - 1]) : 0.0) + fabs(ef[tid]);
    const double tnorm = block_reduce<SP_EIG_THREADS>(rs, red, OpMax());
    const double floor_piv = DBL_EPSILON * tnorm;              // tnorm >= 1: the scaled matrix has a diagonal entry in [1, 2)
    // shifts (in the scaled units of T), equal ones pushed 10 ulp apart, and the first member of each vector's cluster
    if (tid == 0) {
        const double scale = ldexp(1.0, -ex);
        for (int j = 0; j < q; ++j) {
            double s = lam[j] * scale;
            int first = j;
            if (j > 0) {
                const double pertol = 10.0 * DBL_EPSILON * fabs(s);
                if (shift[j - 1] - s < pertol) s = shift[j - 1] - pertol;
                if (shift[j - 1] - s <= 1e-3 * tnorm) first = cstart[j - 1];
            }
            shift[j] = s;
            cstart[j] = first;
        }
    }
    __syncthreads();
    double* u0 = job.work;
    double* u1 = u0 + (long long)d * SS_MAX_Q;
    double* u2 = u1 + (long long)d * SS_MAX_Q;
    double* z = u2 + (long long)d * SS_MAX_Q;
    for (int pass = 0; pass < SS_INVIT_PASSES; ++pass) {
        if (tid < q) {
            // (T - s I) x = rhs: forward elimination with row exchanges, the transformed right-hand side kept in z
            const double s = shift[tid];
            double p = dg[0] - s, pq = d > 1 ? ef[0] : 0.0, y = pass ? z[tid] : ss_start(0, tid);
            for (int i = 0; i + 1 < d; ++i) {
                const long long o = (long long)i * SS_MAX_Q + tid;
                const double ei = ef[i], a1 = dg[i + 1] - s, e1 = i + 2 < d ? ef[i + 1] : 0.0;
                const double b1 = pass ? z[o + SS_MAX_Q] : ss_start(i + 1, tid);
                if (fabs(ei) <= fabs(p)) {
                    const double m = p != 0.0 ? ei / p : 0.0;
                    u0[o] = p; u1[o] = pq; u2[o] = 0.0; z[o] = y;
                    p = a1 - m * pq; pq = e1; y = b1 - m * y;
                } else {
                    const double m = p / ei;
                    u0[o] = ei; u1[o] = a1; u2[o] = e1; z[o] = b1;
                    p = pq - m * a1; pq = -m * e1; y = y - m * b1;
                }
            }
            // back substitution, a pivot below eps |T| replaced by it
            double x1 = 0.0, x2 = 0.0;
            for (int i = d - 1; i >= 0; --i) {
                const long long o = (long long)i * SS_MAX_Q + tid;
                double piv, c1 = 0.0, c2 = 0.0, r;
                if (i == d - 1) { piv = p; r = y; }
                else { piv = u0[o]; c1 = u1[o]; c2 = u2[o]; r = z[o]; }
                if (fabs(piv) < floor_piv) piv = copysign(floor_piv, piv);
                const double x = (r - c1 * x1 - c2 * x2) / piv;
                z[o] = x;
                x2 = x1;
                x1 = x;
            }
        }
        __syncthreads();
        // each cluster belongs to one wave, which takes its vectors in order: modified Gram-Schmidt against the earlier
        // ones, then the norm (scaled by the largest component: a solve can grow a vector by 1 / eps)
        for (int j = 0; j < q; ++j) {
            if (cstart[j] % SP_EIG_WAVES != wave) continue;
            double zr[SP_MAX_D / 64];
#pragma unroll
            for (int m = 0; m < SP_MAX_D / 64; ++m) {
                const int i = lane + 64 * m;
                zr[m] = i < d ? z[(long long)i * SS_MAX_Q + j] : 0.0;
            }
            double big = 0.0;
#pragma unroll
            for (int m = 0; m < SP_MAX_D / 64; ++m) big = fabs(zr[m]) > big ? fabs(zr[m]) : big;
            big = wave_max(big);
            const double pre = big > 0.0 && big <= DBL_MAX ? 1.0 / big : 1.0;
#pragma unroll
            for (int m = 0; m < SP_MAX_D / 64; ++m) zr[m] *= pre;
            for (int c = cstart[j]; c < j; ++c) {
                double zc[SP_MAX_D / 64], dot = 0.0;
#pragma unroll
                for (int m = 0; m < SP_MAX_D / 64; ++m) {
                    const int i = lane + 64 * m;
                    zc[m] = i < d ? z[(long long)i * SS_MAX_Q + c] : 0.0;
                    dot = fma(zc[m], zr[m], dot);
                }
                dot = wave_sum_f64(dot);
#pragma unroll
                for (int m = 0; m < SP_MAX_D / 64; ++m) zr[m] = fma(-dot, zc[m], zr[m]);
            }
            double nn = 0.0;
#pragma unroll
            for (int m = 0; m < SP_MAX_D / 64; ++m) nn = fma(zr[m], zr[m], nn);
            nn = wave_sum_f64(nn);
            const double inv = 1.0 / sqrt(nn);
#pragma unroll
            for (int m = 0; m < SP_MAX_D / 64; ++m) {
                const int i = lane + 64 * m;
                if (i < d) z[(long long)i * SS_MAX_Q + j] = zr[m] * inv;
            }
        }
        __syncthreads();
    }
    // eigenvectors of G = H_0 ... H_{d-3} (those of T): reflectors in reverse, one wave per vector
    for (int j = wave; j < q; j += SP_EIG_WAVES) {
        double zr[SP_MAX_D / 64];
#pragma unroll
        for (int m = 0; m < SP_MAX_D / 64; ++m) {
            const int i = lane + 64 * m;
            zr[m] = i < d ? z[(long long)i * SS_MAX_Q + j] : 0.0;
        }
        for (int k = d - 3; k >= 0; --k) {
            const double* hv = A + (long long)k * d;
            double hr[SP_MAX_D / 64], dot = 0.0;
#pragma unroll
            for (int m = 0; m < SP_MAX_D / 64; ++m) {
                const int i = lane + 64 * m;
                hr[m] = i > k && i < d ? hv[i] : 0.0;
                dot = fma(hr[m], zr[m], dot);
            }
            dot = wave_sum_f64(dot) * taus[k];
#pragma unroll
            for (int m = 0; m < SP_MAX_D / 64; ++m) zr[m] = fma(-dot, hr[m], zr[m]);
        }
        // sign: the largest-magnitude component positive, the first one on ties
        double ba = -1.0, bv = 0.0;
        int bi = 0;
#pragma unroll
        for (int m = 0; m < SP_MAX_D / 64; ++m) {
            const int i = lane + 64 * m;
            if (i < d && fabs(zr[m]) > ba) { ba = fabs(zr[m]); bv = zr[m]; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double oa = __shfl_xor(ba, o, 64), ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oa > ba || (oa == ba && oi < bi)) { ba = oa; bv = ov; bi = oi; }
        }
        const double sg = bv < 0.0 ? -1.0 : 1.0;
#pragma unroll
        for (int m = 0; m < SP_MAX_D / 64; ++m) {
            const int i = lane + 64 * m;
            if (i < d) job.evecs[(long long)i * q + j] = sg * zr[m];
        }
    }
}

struct TailArgs {
    const double* c;      // [d_a, d_b] standardised cross-Gram
    const double* va;     // [d_a, q]
    const double* vb;     // [d_b, q]
    const double* evals;  // [2, q]
    double* w;            // [d_a, q]
    double* m;            // [q, q]
    double* s;            // [q, q]
    double* out;          // [1]
    double* rho;          // NULL or [q]
    double* evals_out;    // NULL or [2, q]
    int da, db, q;
};

// M = L_a^(-1/2) V_a^T C V_b L_b^(-1/2), rho = sqrt(eig(M^T M)) clamped to [0, 1], out = mean rho; NaN when either view has
// numerical rank below q (lambda_q <= d 2^-53 lambda_1) or is not finite.
__global__ __launch_bounds__(SP_EIG_THREADS) void svcca_tail(TailArgs t) {
    __shared__ double v[SP_MAX_D], w[SP_MAX_D], dg[SP_MAX_D], e2[SP_MAX_D], lam[SP_MAX_D];
    __shared__ double red[SP_EIG_THREADS];
    __shared__ long long cred[SP_EIG_THREADS];
    const int tid = threadIdx.x, q = t.q;
    for (int idx = tid; idx < t.da * q; idx += SP_EIG_THREADS) {
        const int i = idx / q, k = idx - i * q;
        double acc = 0.0;
        for (int j = 0; j < t.db; ++j) acc = fma(t.c[(long long)i * t.db + j], t.vb[(long long)j * q + k], acc);
        t.w[idx] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < q * q; idx += SP_EIG_THREADS) {
        const int k = idx / q, l = idx - k * q;
        double acc = 0.0;
        for (int i = 0; i < t.da; ++i) acc = fma(t.va[(long long)i * q + k], t.w[(long long)i * q + l], acc);
        t.m[idx] = acc / (sqrt(t.evals[k]) * sqrt(t.evals[q + l]));
    }
    __syncthreads();
    for (int idx = tid; idx < q * q; idx += SP_EIG_THREADS) {
        const int k = idx / q, l = idx - k * q;
        double acc = 0.0;
        for (int i = 0; i < q; ++i) acc = fma(t.m[i * q + k], t.m[i * q + l], acc);
        t.s[idx] = acc;
    }
    __syncthreads();
    double mx;
    long long rows;
    int ex;
    const bool degenerate = sp_prescale(t.s, q, 0, red, cred, mx, rows, ex);
    sp_tridiag<false>(t.s, q, degenerate, v, w, dg, e2, nullptr);
    sp_bisect(q, degenerate, mx, ldexp(1.0, ex), dg, e2, lam, red);
    const double tiny = ldexp(1.0, -53);
    const bool full_rank = t.evals[q - 1] > t.da * tiny * t.evals[0] && t.evals[2 * q - 1] > t.db * tiny * t.evals[q];
    if (tid < q) {
        const double l = lam[tid];
        const double r = sqrt(l > 1.0 ? 1.0 : (l > 0.0 ? l : (l == l ? 0.0 : l)));
        lam[tid] = full_rank ? r : NAN;
        if (t.rho) t.rho[tid] = lam[tid];
    }
    if (t.evals_out && tid < 2 * q) t.evals_out[tid] = t.evals[tid];
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int k = 0; k < q; ++k) sum += lam[k];
        t.out[0] = sum / (double)q;
    }
}

}  // namespace

extern "C" {

int umlh_spectral_chunks(int batch, long long n) {
    long long c = (n + SP_CHUNK_ROWS - 1) / SP_CHUNK_ROWS;
    const long long cap = SP_MAX_CHUNKS / batch > 1 ? SP_MAX_CHUNKS / batch : 1;
    c = c > cap ? cap : c;
    return (int)(c < 1 ? 1 : c);
}

struct SpectralPlan { int chunks; long long slabs, g, total; };

static SpectralPlan spectral_plan(int batch, long long n, int d) {
    const long long dd = (long long)d * d * 8;
    SpectralPlan p;
    ScratchLayout lay;
    p.chunks = umlh_spectral_chunks(batch, n);
    p.slabs = lay.take(dd * batch * p.chunks), p.g = lay.take(dd * batch), p.total = lay.end;
    return p;
}

unsigned long long umlh_spectral_bytes(int batch, long long n, int d) { return (unsigned long long)spectral_plan(batch, n, d).total; }

// Dense: period = rows = n, batch matrices `sm` apart.  Sequence block: batch = 1, rows = n_outer * period.
int umlh_spectral_launch(const float* a, int batch, long long rows, int period, long long sm, long long so, long long si,
                         const long long* lengths, int drop_last, int d, double eps, double* erank, double* rows_out, double* sv,
                         int sv_ld, void* scratch, hipStream_t st) {
    const SpectralPlan p = spectral_plan(batch, rows, d);
    double *slabs = at<double>(scratch, p.slabs), *g = at<double>(scratch, p.g);
    RowMap map{a, sm, so, si, lengths, (unsigned)rows, (unsigned)period, drop_last};
    hipLaunchKernelGGL(spectral_gram, dim3(tri_tiles((d + G64_TILE - 1) / G64_TILE), p.chunks, batch), dim3(256), 0, st, map, d, p.chunks, slabs);
    hipLaunchKernelGGL(spectral_reduce, dim3((d * d + 255) / 256, batch), dim3(256), 0, st, slabs, d, p.chunks, g);
    EigOut out{erank, 1, rows_out, sv, sv_ld, eps};
    hipLaunchKernelGGL(spectral_eig, dim3(batch), dim3(SP_EIG_THREADS), 0, st, g, d, map, (int)(rows / period), out);
    return (int)hipGetLastError();
}

}  // extern "C"

// ---- principal subspaces and SVCCA ----
namespace {
struct SubspacePlan {
    long long stats_a, stats_b, stat_scr, slabs, gc_a, gc_b, g_a, g_b, c, work_a, work_b, ev, vec_a, vec_b, w, m, s, total;
    int chunks;
};

// d_b = 0: the single-matrix op
SubspacePlan subspace_plan(long long n, int da, int db, int q) {
    SubspacePlan p;
    const long long dm = da > db ? da : db;
    p.chunks = umlh_spectral_chunks(1, n);
    ScratchLayout lay;
    p.stats_a = lay.take(8LL * da), p.stats_b = lay.take(8LL * db);
    p.stat_scr = lay.take((long long)umlh_probe_stats_bytes((int)dm)), p.slabs = lay.take(8LL * p.chunks * dm * dm);
    p.gc_a = lay.take(8LL * da * da), p.gc_b = lay.take(8LL * db * db);
    p.g_a = lay.take(8LL * da * da), p.g_b = lay.take(8LL * db * db);
    p.c = lay.take(8LL * da * db);
    p.work_a = lay.take(8LL * 4 * da * SS_MAX_Q), p.work_b = lay.take(8LL * 4 * db * SS_MAX_Q);
    p.ev = lay.take(db ? 16LL * q : 0);
    p.vec_a = lay.take(db ? 8LL * da * q : 0), p.vec_b = lay.take(8LL * db * q);
    p.w = lay.take(db ? 8LL * da * q : 0);
    p.m = lay.take(db ? 8LL * q * q : 0), p.s = lay.take(db ? 8LL * q * q : 0);
    p.total = lay.end;
    return p;
}

// the standardised Gram D Gc D of one view: column means, centred Gram slabs, their sum, the scaling
void standardised_gram(const float* x, long long n, int d, long long ld, double* stats, void* stat_scr, double* slabs, int chunks,
                       double* gc, double* g, hipStream_t st) {
    umlh_probe_launch_means(x, n, d, (int)ld, stats, stat_scr, st);
    const Operand op{x, ld, stats, d};
    hipLaunchKernelGGL((subspace_gram<true>), dim3(tri_tiles((d + G64_TILE - 1) / G64_TILE), chunks), dim3(256), 0, st, op, op, (unsigned)n, chunks, slabs);
    hipLaunchKernelGGL(spectral_reduce, dim3((d * d + 255) / 256, 1), dim3(256), 0, st, slabs, d, chunks, gc);
    hipLaunchKernelGGL(subspace_standardise, dim3((d * d + 255) / 256), dim3(256), 0, st, gc, d, d, gc, gc, (double)(n - 1), g);
}
}  // namespace

extern "C" {

unsigned long long umlh_subspace_bytes(long long n, int da, int db, int q) { return (unsigned long long)subspace_plan(n, da, db, q).total; }

int umlh_subspace_launch(const float* a, long long n, int d, long long ld, int q, int standardize, double* evals, double* evecs,
                         void* scratch, hipStream_t st) {
    const SubspacePlan p = subspace_plan(n, d, 0, q);
    double* slabs = at<double>(scratch, p.slabs);
    double* g = at<double>(scratch, p.g_a);
    if (standardize) {
        standardised_gram(a, n, d, ld, at<double>(scratch, p.stats_a), at<void>(scratch, p.stat_scr), slabs, p.chunks,
                          at<double>(scratch, p.gc_a), g, st);
    } else {                                                   // the Gram of umlh_svdvals, bit for bit
        RowMap map{a, 0, 0, ld, nullptr, (unsigned)n, (unsigned)n, 0};
        hipLaunchKernelGGL(spectral_gram, dim3(tri_tiles((d + G64_TILE - 1) / G64_TILE), p.chunks, 1), dim3(256), 0, st, map, d, p.chunks, slabs);
        hipLaunchKernelGGL(spectral_reduce, dim3((d * d + 255) / 256, 1), dim3(256), 0, st, slabs, d, p.chunks, g);
    }
    EigJobs jobs{};
    jobs.j[0] = EigJob{g, evals, evecs, at<double>(scratch, p.work_a), d};
    jobs.q = q;
    hipLaunchKernelGGL(subspace_eig, dim3(1), dim3(SP_EIG_THREADS), 0, st, jobs);
    return (int)hipGetLastError();
}

int umlh_svcca_launch(const float* a, const float* b, long long n, int da, int db, long long lda, long long ldb, int q, double* out,
                      double* rho, double* evals, void* scratch, hipStream_t st) {
    const SubspacePlan p = subspace_plan(n, da, db, q);
    double* slabs = at<double>(scratch, p.slabs);
    double *sta = at<double>(scratch, p.stats_a), *stb = at<double>(scratch, p.stats_b);
    double *gca = at<double>(scratch, p.gc_a), *gcb = at<double>(scratch, p.gc_b), *c = at<double>(scratch, p.c);
    standardised_gram(a, n, da, lda, sta, at<void>(scratch, p.stat_scr), slabs, p.chunks, gca, at<double>(scratch, p.g_a), st);
    standardised_gram(b, n, db, ldb, stb, at<void>(scratch, p.stat_scr), slabs, p.chunks, gcb, at<double>(scratch, p.g_b), st);
    const Operand oa{a, lda, sta, da}, ob{b, ldb, stb, db};
    const int nta = (da + G64_TILE - 1) / G64_TILE, ntb = (db + G64_TILE - 1) / G64_TILE;
    const long long total = (long long)da * db;
    hipLaunchKernelGGL((subspace_gram<false>), dim3(nta * ntb, p.chunks), dim3(256), 0, st, oa, ob, (unsigned)n, p.chunks, slabs);
    hipLaunchKernelGGL(subspace_reduce_rect, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, slabs, total, p.chunks, c);
    hipLaunchKernelGGL(subspace_standardise, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, c, da, db, gca, gcb,
                       (double)(n - 1), c);
    double* ev = at<double>(scratch, p.ev);
    EigJobs jobs{};
    jobs.j[0] = EigJob{at<double>(scratch, p.g_a), ev, at<double>(scratch, p.vec_a), at<double>(scratch, p.work_a), da};
    jobs.j[1] = EigJob{at<double>(scratch, p.g_b), ev + q, at<double>(scratch, p.vec_b), at<double>(scratch, p.work_b), db};
    jobs.q = q;
    hipLaunchKernelGGL(subspace_eig, dim3(2), dim3(SP_EIG_THREADS), 0, st, jobs);
    TailArgs t{c, jobs.j[0].evecs, jobs.j[1].evecs, ev, at<double>(scratch, p.w), at<double>(scratch, p.m), at<double>(scratch, p.s),
               out, rho, evals, da, db, q};
    hipLaunchKernelGGL(svcca_tail, dim3(1), dim3(SP_EIG_THREADS), 0, st, t);
    return (int)hipGetLastError();
}

}  // extern "C"
