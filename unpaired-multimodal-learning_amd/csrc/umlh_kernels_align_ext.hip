// The remaining alignment metrics of the reference (vision_language/metrics.py:39-51,88-92,96-119,164-176,180-249,258-269,
// 288-308) for gfx950: unbiased linear CKA, RBF CKA (biased and unbiased), CKNNA and the k-NN list statistics.
//
//   ext_means        column means of A | B as fp32, from cka_colsum's chunk partials (the value cka_cross centres with)
//   ext_center_sums  column sums of the ROUNDED centred values (not exactly zero in fp32), per row chunk, in double
//                    (colsum_chunk of umlh_gram.h on the fl(x - mean) transform)
//   ext_colfin       fixed-order sum of those chunks
//   ext_rows<0>      per row |x_i|^2, |y_i|^2 and (K~1)_i = x_i . (sum_j x_j) - |x_i|^2 (fp32 products, double sums) -> block
//                    partials of the twelve HSIC sums;  ext_rows<1>: only the squared norms, as fp32, for the RBF distances
//   rbf_tiles        a 32-row strip x a chunk of 256-column tiles: both views' Gram tiles on v_mfma_f32_32x32x2_f32 from
//                    column-centred operands, d^2 = |x_i|^2 + |x_j|^2 - 2 x_i.x_j clamped at 0, K = expf(-d^2 / 2 sigma^2);
//                    K.L, K.K, L.L and the row sums K1, L1 are formed and summed in double (the fp32 kernel values are exact there)
//   rbf_rows         K1, L1 per row (the chunks' partials in fixed order) -> block partials of the twelve HSIC sums
//   cknna_rowsum     per row the sums of M = K [j in S(i)], P = L [j in S(i)] for S = knn_a n knn_b, knn_a, knn_b
//   cknna_rows       per row sum_j M_ij P_ji (M, P are not symmetric) and sum_j M_ij rowsum_P(j) -> block partials
//   ext_final        fixed-order sums -> hsic (unbiased: Song et al. eq. 5 as metrics.py:230-249; biased: trace(K H L H))
//                    -> {hsic_kl / (sqrt(hsic_kk hsic_ll) + 1e-6), hsic_kl, hsic_kk, hsic_ll}
//   list_rows        thread per row: cycle hit, LCS length and Levenshtein distance of the two k-lists; integer block sums
//   list_final       fixed-order integer sums -> {mean hit, mean LCS length, 1 - mean distance / k}
//
// The twelve HSIC sums are, for each of (K,L), (K,K), (L,L): sum M~ . P~^T, 1^T M~ 1, 1^T P~ 1, 1^T M~ P~ 1.
// Nothing here forms an N x N array and no reduction uses a float atomic: results are bitwise reproducible for a given `splits`.
#include "umlh_common.h"
#include "umlh_gram.h"
#include "umlh_launch.h"
#include "umlh_topk.h"

namespace {

constexpr int NSUM = 12;
constexpr int LS_KMAX = 32;
constexpr int LS_LD = LS_KMAX + 1;

inline int up4(int d) { return (d + 3) / 4 * 4; }

// mean[0 .. da4) for A, mean[da4 .. da4 + db4) for B (d rounded up to 4, zero past d): (float)(sum / n) as cka_cross forms it.
__global__ __launch_bounds__(256) void ext_means(const double* __restrict__ colsum, int chunks, int da, int db, int n,
                                                 float* __restrict__ mean) {
    const int da4 = (da + 3) / 4 * 4, db4 = (db + 3) / 4 * 4, idx = blockIdx.x * 256 + threadIdx.x, dt = da + db;
    if (idx >= da4 + db4) return;
    int c = -1;
    if (idx < da) c = idx;
    else if (idx >= da4 && idx - da4 < db) c = da + idx - da4;
    mean[idx] = c >= 0 ? (float)(chunk_total(colsum, chunks, dt, c) / (double)n) : 0.f;
}

// Column c of A | B, rows of chunk blockIdx.y: sum of fl(x - mean) in double (colsum_chunk, umlh_gram.h, as cka_colsum).
__global__ __launch_bounds__(256) void ext_center_sums(const float* __restrict__ a, int lda, int da, const float* __restrict__ b,
                                                       int ldb, int db, int n, int chunks, const float* __restrict__ mean,
                                                       double* __restrict__ partial) {
    const int da4 = (da + 3) / 4 * 4;
    colsum_chunk([=](int c) {
        const float* p = c < da ? a + c : b + (c - da);
        const long long ld = c < da ? lda : ldb;
        const float m = c < da ? mean[c] : mean[da4 + c - da];
        return [=](long long r) { return (double)(p[r * ld] - m); };
    }, da + db, n, chunks, partial);
}

__global__ __launch_bounds__(256) void ext_colfin(const double* __restrict__ partial, int chunks, int dt, double* __restrict__ csum) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < dt) csum[c] = chunk_total(partial, chunks, dt, c);
}

struct RowArgs {
    const float* a;
    const float* b;
    int lda, ldb, da, db;
    long long n;
    const float* mean;                       // [da4 + db4]
    const double* csum;                      // [da + db]   (MODE 0)
    float* norms;                            // [2][n]      (MODE 1)
    double* part;                            // [blocks][12] (MODE 0)
};

// 64 rows per workgroup, a wave per row (16 rows each): lanes stride the columns, the products are fp32, every sum is double.
template <int MODE>
__global__ __launch_bounds__(256) void ext_rows(RowArgs g) {
    __shared__ double rv[64][4];
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, da4 = (g.da + 3) / 4 * 4;
    const long long r0 = (long long)blockIdx.x * 64;
    for (int k = 0; k < 16; ++k) {
        const int lr = wave * 16 + k;
        const long long r = r0 + lr;
        double nx = 0.0, kx = 0.0, ny = 0.0, ky = 0.0;
        if (r < g.n) {
            const float* pa = g.a + r * g.lda;
            const float* pb = g.b + r * g.ldb;
            for (int c = lane; c < g.da; c += 64) {
                const float xc = pa[c] - g.mean[c];
                nx += (double)(xc * xc);
                if (MODE == 0) kx += (double)xc * g.csum[c];
            }
            for (int c = lane; c < g.db; c += 64) {
                const float yc = pb[c] - g.mean[da4 + c];
                ny += (double)(yc * yc);
                if (MODE == 0) ky += (double)yc * g.csum[g.da + c];
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            nx += __shfl_xor(nx, off);
            ny += __shfl_xor(ny, off);
            if (MODE == 0) {
                kx += __shfl_xor(kx, off);
                ky += __shfl_xor(ky, off);
            }
        }
        if (lane == 0) { rv[lr][0] = nx; rv[lr][1] = kx - nx; rv[lr][2] = ny; rv[lr][3] = ky - ny; }
    }
    __syncthreads();
    const bool valid = tid < 64 && r0 + tid < g.n;
    if (MODE == 1) {
        if (valid) {
            g.norms[r0 + tid] = (float)rv[tid][0];
            g.norms[g.n + r0 + tid] = (float)rv[tid][2];
        }
        return;
    }
    double v[NSUM];
#pragma unroll
    for (int s = 0; s < NSUM; ++s) v[s] = 0.0;
    if (valid) {   // the diagonal of the linear kernels leaves the Frobenius terms; K~1 and L~1 are exact per row
        const double nx = rv[tid][0], kx = rv[tid][1], ny = rv[tid][2], ky = rv[tid][3];
        v[0] = -nx * ny; v[1] = kx; v[2] = ky; v[3] = kx * ky;
        v[4] = -nx * nx; v[5] = kx; v[6] = kx; v[7] = kx * kx;
        v[8] = -ny * ny; v[9] = ky; v[10] = ky; v[11] = ky * ky;
    }
#pragma unroll
    for (int s = 0; s < NSUM; ++s) {
        const double t = block_reduce<256>(v[s], red, OpSum());
        if (tid == 0) g.part[(long long)blockIdx.x * NSUM + s] = t;
    }
}

// x[row][k .. k+3] - mean[k .. k+3], zero outside [0, n) x [0, d); mean is padded to a multiple of 4 and 16-byte aligned
template <bool VEC>
__device__ __forceinline__ f32x4v rb_load4(const float* __restrict__ x, const float* __restrict__ mean, long long row, long long n,
                                           int k, int d, int ldx) {
    f32x4v v = {0.f, 0.f, 0.f, 0.f};
    if (row < n && k < d) {
        const float* p = x + row * (long long)ldx + k;
        const f32x4v m = *reinterpret_cast<const f32x4v*>(mean + k);
        if (VEC) {
            v = *reinterpret_cast<const f32x4v*>(p) - m;
        } else {
            v[0] = p[0] - m[0];
            if (k + 1 < d) v[1] = p[1] - m[1];
            if (k + 2 < d) v[2] = p[2] - m[2];
            if (k + 3 < d) v[3] = p[3] - m[3];
        }
    }
    return v;
}

// The 32 x 64 block of centred inner products of one view: the k loop of the k-NN tiles (gram_32x64, umlh_topk.h) on the
// mean-centring loader.  The strips and tiles are the k-NN pass's as well (TK_ROWS x TK_COLS, umlh_align_knn_splits).
template <bool VEC>
__device__ __forceinline__ void rb_gram(const float* __restrict__ x, const float* __restrict__ mean, long long n, int d, int ldx,
                                        long long ra, long long rb0, long long rb1, int h, f32x16& acc0, f32x16& acc1) {
    const auto load = [&](long long row, int k) { return rb_load4<VEC>(x, mean, row, n, k, d, ldx); };
    gram_32x64(load, load, d, ra, rb0, rb1, h, acc0, acc1);
}

struct RbfArgs {
    const float* a;
    const float* b;
    const float* mean;                       // [da4 + db4]
    const float* norms;                      // [2][n] squared norms of the centred rows
    int lda, ldb, da, db, n, ntiles, splits, strips, unbiased;
    float gamma;                             // 1 / (2 sigma^2)
    double* pair;                            // [3][splits * strips]
    double* rowpart;                         // [splits][strips * 32][2]
};

// One kernel value: acc = x_i . x_j of the centred rows; the diagonal is exact (1 biased, left out unbiased); 0 outside n.
__device__ __forceinline__ float rb_value(float acc, float ni, float nj, float gamma, long long gi, long long gj, int n, float diag) {
    const float d2 = fmaxf(0.f, (ni + nj) - 2.f * acc);
    float k = expf(-d2 * gamma);
    if (gi == gj) k = diag;
    return (gi < n && gj < n) ? k : 0.f;
}

template <bool VEC>
__global__ __launch_bounds__(256) void rbf_tiles(RbfArgs g) {
    __shared__ float rn[2][TK_ROWS];
    __shared__ double rs[4][TK_ROWS][2];
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c32 = lane & 31;
    const int n = g.n, da4 = (g.da + 3) / 4 * 4;
    const long long r0 = (long long)blockIdx.x * TK_ROWS;
    const int split = blockIdx.y;
    const int t0 = (int)((long long)split * g.ntiles / g.splits), t1 = (int)((long long)(split + 1) * g.ntiles / g.splits);
    if (tid < 2 * TK_ROWS) {
        const int v = tid >> 5, i = tid & 31;
        rn[v][i] = r0 + i < n ? g.norms[(long long)v * n + r0 + i] : 0.f;
    }
    __syncthreads();
    const float diag = g.unbiased ? 0.f : 1.f, gamma = g.gamma;
    double skl = 0.0, skk = 0.0, sll = 0.0, rowk[16], rowl[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { rowk[q] = 0.0; rowl[q] = 0.0; }
    for (int t = t0; t < t1; ++t) {
        const long long ra = r0 + c32, rb0 = (long long)t * TK_COLS + wave * 64 + c32, rb1 = rb0 + 32;
        float kv0[16], kv1[16];
        {
            f32x16 acc0 = {}, acc1 = {};
            rb_gram<VEC>(g.a, g.mean, n, g.da, g.lda, ra, rb0, rb1, h, acc0, acc1);
            const float n0 = rb0 < n ? g.norms[rb0] : 0.f, n1 = rb1 < n ? g.norms[rb1] : 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) {           // acc[q]: row 8(q/4) + 4h + q%4, column c32
                const int i = 8 * (q >> 2) + 4 * h + (q & 3);
                kv0[q] = rb_value(acc0[q], rn[0][i], n0, gamma, r0 + i, rb0, n, diag);
                kv1[q] = rb_value(acc1[q], rn[0][i], n1, gamma, r0 + i, rb1, n, diag);
            }
        }
        f32x16 acc0 = {}, acc1 = {};
        rb_gram<VEC>(g.b, g.mean + da4, n, g.db, g.ldb, ra, rb0, rb1, h, acc0, acc1);
        const float n0 = rb0 < n ? g.norms[(long long)n + rb0] : 0.f, n1 = rb1 < n ? g.norms[(long long)n + rb1] : 0.f;
        // K and L are fp32 values; every product and sum of them is double.  HSIC is linear in K with the CENTRED L as its
        // coefficient, so the rounding of K itself is harmless, but a rounding of K.L or of a partial sum is not: with
        // K ~ L ~ 1 (near-coincident rows) the three sums cancel to 1e-8 of their size.
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int i = 8 * (q >> 2) + 4 * h + (q & 3);
            const double l0 = (double)rb_value(acc0[q], rn[1][i], n0, gamma, r0 + i, rb0, n, diag);
            const double l1 = (double)rb_value(acc1[q], rn[1][i], n1, gamma, r0 + i, rb1, n, diag);
            const double k0 = (double)kv0[q], k1 = (double)kv1[q];
            skl = fma(k0, l0, fma(k1, l1, skl));
            skk = fma(k0, k0, fma(k1, k1, skk));
            sll = fma(l0, l0, fma(l1, l1, sll));
            rowk[q] += k0 + k1;
            rowl[q] += l0 + l1;
        }
    }
    // row sums: the 32 column lanes of a half wave (xor butterfly), then the four waves in order
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        for (int off = 16; off > 0; off >>= 1) {
            rowk[q] += __shfl_xor(rowk[q], off);
            rowl[q] += __shfl_xor(rowl[q], off);
        }
        if (c32 == 0) {
            const int i = 8 * (q >> 2) + 4 * h + (q & 3);
            rs[wave][i][0] = rowk[q];
            rs[wave][i][1] = rowl[q];
        }
    }
    __syncthreads();
    if (tid < 2 * TK_ROWS) {
        const int i = tid >> 1, v = tid & 1;
        g.rowpart[(((long long)split * g.strips) * TK_ROWS + r0 + i) * 2 + v] = ((rs[0][i][v] + rs[1][i][v]) + rs[2][i][v]) + rs[3][i][v];
    }
    const long long nwg = (long long)g.splits * g.strips, wg = (long long)split * g.strips + blockIdx.x;
    const double pkl = block_reduce<256>(skl, red, OpSum()), pkk = block_reduce<256>(skk, red, OpSum()), pll = block_reduce<256>(sll, red, OpSum());
    if (tid == 0) {
        g.pair[wg] = pkl;
        g.pair[nwg + wg] = pkk;
        g.pair[2 * nwg + wg] = pll;
    }
}

__global__ __launch_bounds__(256) void rbf_rows(const double* __restrict__ rowpart, int splits, long long npad, int n,
                                                double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    double k1 = 0.0, l1 = 0.0;
    if (i < n)
        for (int s = 0; s < splits; ++s) {
            k1 += rowpart[((long long)s * npad + i) * 2];
            l1 += rowpart[((long long)s * npad + i) * 2 + 1];
        }
    const double v[NSUM] = {0.0, k1, l1, k1 * l1, 0.0, k1, k1, k1 * k1, 0.0, l1, l1, l1 * l1};
#pragma unroll
    for (int s = 0; s < NSUM; ++s) {
        const double t = block_reduce<256>(v[s], red, OpSum());
        if (tid == 0) part[(long long)blockIdx.x * NSUM + s] = t;
    }
}

// rsum[i] = {sum_{j in S(i)} K_ij, sum_{j in S(i)} L_ij, sum_{j in knn_a(i)} K_ij, sum_{j in knn_b(i)} L_ij}, S = knn_a n knn_b
__global__ __launch_bounds__(256) void cknna_rowsum(const int* __restrict__ ka, const float* __restrict__ sa, const int* __restrict__ kb,
                                                    const float* __restrict__ sb, int n, int topk, double* __restrict__ rsum) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int* a = ka + i * topk;
    const int* b = kb + i * topk;
    const float* va = sa + i * topk;
    const float* vb = sb + i * topk;
    double rm = 0.0, rp = 0.0, rk = 0.0, rl = 0.0;
    for (int p = 0; p < topk; ++p) {
        const int j = a[p];
        rk += (double)va[p];
        rl += (double)vb[p];
        for (int q = 0; q < topk; ++q)
            if (b[q] == j) { rm += (double)va[p]; rp += (double)vb[q]; break; }
    }
    rsum[i * 4] = rm; rsum[i * 4 + 1] = rp; rsum[i * 4 + 2] = rk; rsum[i * 4 + 3] = rl;
}

// position of `want` in the k-list `l`, or -1
__device__ __forceinline__ int list_find(const int* __restrict__ l, int topk, int want) {
    for (int q = 0; q < topk; ++q)
        if (l[q] == want) return q;
    return -1;
}

// Thread per row i.  First term: sum_j M_ij P_ji with P_ji = L_ji [i in S(j)] (metrics.py:243: K~ * L~^T; the masked kernels are
// not symmetric); third term: sum_j M_ij rowsum_P(j).  Neighbours outside [0, n) are ignored.
__global__ __launch_bounds__(256) void cknna_rows(const int* __restrict__ ka, const float* __restrict__ sa, const int* __restrict__ kb,
                                                  const float* __restrict__ sb, int n, int topk, const double* __restrict__ rsum,
                                                  double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    double v[NSUM];
#pragma unroll
    for (int s = 0; s < NSUM; ++s) v[s] = 0.0;
    if (i < n) {
        const int* a = ka + i * topk;
        const int* b = kb + i * topk;
        v[1] = rsum[i * 4]; v[2] = rsum[i * 4 + 1];
        v[5] = v[6] = rsum[i * 4 + 2];
        v[9] = v[10] = rsum[i * 4 + 3];
        for (int p = 0; p < topk; ++p) {
            const int j = a[p];
            if (j < 0 || j >= n) continue;
            const double s = (double)sa[i * topk + p];
            const int pa = list_find(ka + (long long)j * topk, topk, (int)i);
            v[7] += s * rsum[(long long)j * 4 + 2];
            if (pa >= 0) v[4] += s * (double)sa[(long long)j * topk + pa];
            if (list_find(b, topk, j) >= 0) {
                v[3] += s * rsum[(long long)j * 4 + 1];
                const int pb = pa >= 0 ? list_find(kb + (long long)j * topk, topk, (int)i) : -1;
                if (pb >= 0) v[0] += s * (double)sb[(long long)j * topk + pb];
            }
        }
        for (int q = 0; q < topk; ++q) {
            const int j = b[q];
            if (j < 0 || j >= n) continue;
            const double s = (double)sb[i * topk + q];
            const int pb = list_find(kb + (long long)j * topk, topk, (int)i);
            v[11] += s * rsum[(long long)j * 4 + 3];
            if (pb >= 0) v[8] += s * (double)sb[(long long)j * topk + pb];
        }
    }
#pragma unroll
    for (int s = 0; s < NSUM; ++s) {
        const double t = block_reduce<256>(v[s], red, OpSum());
        if (tid == 0) part[(long long)blockIdx.x * NSUM + s] = t;
    }
}

// seg: three consecutive runs of len0, len1, len2 doubles added to the first terms of (K,L), (K,K), (L,L); part: [nblocks][12].
__global__ __launch_bounds__(256) void ext_final(const double* __restrict__ seg, long long len0, long long len1, long long len2,
                                                 const double* __restrict__ part, long long nblocks, double m, int unbiased,
                                                 double* __restrict__ out4) {
    __shared__ double red[256];
    __shared__ double tot[NSUM];
    const int tid = threadIdx.x;
    const long long lo[3] = {0, len0, len0 + len1}, len[3] = {len0, len1, len2};
    for (int s = 0; s < NSUM; ++s) {
        double acc = 0.0;
        for (long long b = tid; b < nblocks; b += 256) acc += part[b * NSUM + s];
        if ((s & 3) == 0)
            for (long long e = tid; e < len[s >> 2]; e += 256) acc += seg[lo[s >> 2] + e];
        const double t = block_reduce<256>(acc, red, OpSum());
        if (tid == 0) tot[s] = t;
    }
    if (tid == 0) {
        double hs[3];
        for (int p = 0; p < 3; ++p) {
            const double tr = tot[4 * p], sm = tot[4 * p + 1], sp = tot[4 * p + 2], d = tot[4 * p + 3];
            if (unbiased) hs[p] = (tr + sm * sp / ((m - 1.0) * (m - 2.0)) - 2.0 * d / (m - 2.0)) / (m * (m - 3.0));   // metrics.py:242-248
            else hs[p] = tr - 2.0 * d / m + sm * sp / (m * m);                                                      // trace(K H L H)
        }
        out4[0] = hs[0] / (sqrt(hs[1] * hs[2]) + 1e-6);   // metrics.py:118, :227; a negative product gives NaN as there
        out4[1] = hs[0];
        out4[2] = hs[1];
        out4[3] = hs[2];
    }
}

// Thread per row, 64 rows per workgroup.  cycle (metrics.py:39-51,258-269): is i among knn_a[knn_b[i, p], q]; LCS length
// (:288-308) and unit-cost Levenshtein distance (:164-176) of knn_a[i, :] and knn_b[i, :], one DP row each.
__global__ __launch_bounds__(64) void list_rows(const int* __restrict__ ka, const int* __restrict__ kb, int n, int topk,
                                                int* __restrict__ rows, long long* __restrict__ part) {
    __shared__ int la[64 * LS_LD], lb[64 * LS_LD], dp[64 * LS_LD];
    __shared__ long long red[3][64];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * 64 + tid;
    int hit = 0, lcs = 0, dist = 0;
    if (i < n) {
        int* a = la + tid * LS_LD;
        int* b = lb + tid * LS_LD;
        int* w = dp + tid * LS_LD;
        for (int p = 0; p < topk; ++p) { a[p] = ka[i * topk + p]; b[p] = kb[i * topk + p]; }
        for (int p = 0; p < topk; ++p) {
            const int j = b[p];
            if (j < 0 || j >= n) continue;
            hit |= list_find(ka + (long long)j * topk, topk, (int)i) >= 0;
        }
        for (int y = 0; y <= topk; ++y) w[y] = 0;
        for (int x = 1; x <= topk; ++x) {
            int diag = 0;
            for (int y = 1; y <= topk; ++y) {
                const int up = w[y];
                w[y] = a[x - 1] == b[y - 1] ? diag + 1 : max(up, w[y - 1]);
                diag = up;
            }
        }
        lcs = w[topk];
        for (int y = 0; y <= topk; ++y) w[y] = y;
        for (int x = 1; x <= topk; ++x) {
            int diag = w[0];
            w[0] = x;
            for (int y = 1; y <= topk; ++y) {
                const int up = w[y];
                w[y] = min(min(up, w[y - 1]) + 1, diag + (a[x - 1] != b[y - 1]));
                diag = up;
            }
        }
        dist = w[topk];
        if (rows) { rows[i * 3] = hit; rows[i * 3 + 1] = lcs; rows[i * 3 + 2] = dist; }
    }
    red[0][tid] = hit; red[1][tid] = lcs; red[2][tid] = dist;
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
        if (tid < w) { red[0][tid] += red[0][tid + w]; red[1][tid] += red[1][tid + w]; red[2][tid] += red[2][tid + w]; }
        __syncthreads();
    }
    if (tid < 3) part[(long long)blockIdx.x * 3 + tid] = red[tid][0];
}

__global__ __launch_bounds__(256) void list_final(const long long* __restrict__ part, long long nblocks, int n, int topk,
                                                  double* __restrict__ out3) {
    __shared__ long long red[256];
    const int tid = threadIdx.x;
    for (int s = 0; s < 3; ++s) {
        long long c = 0;
        for (long long b = tid; b < nblocks; b += 256) c += part[b * 3 + s];
        c = block_reduce<256>(c, red, OpSum());
        if (tid == 0) {
            const double mean = (double)c / (double)n;
            out3[s] = s < 2 ? mean : 1.0 - mean / (double)topk;   // metrics.py:51, :91 (not divided by k), :176
        }
    }
}

struct UnbiasedPlan { int chunks; long long base, mean, part2, csum, part, nblocks, total; };

UnbiasedPlan unbiased_plan(long long n, int da, int db, int splits) {
    UnbiasedPlan p;
    const long long dt = (long long)da + db;
    p.chunks = umlh_align_cka_sum_chunks(n);
    p.base = (long long)umlh_align_cka_bytes(n, da, db, splits);
    p.nblocks = (n + 63) / 64;
    ScratchLayout lay(p.base);                       // behind the CKA layout, whose products the launcher runs first
    p.mean = lay.take((long long)(up4(da) + up4(db)) * 4);
    p.part2 = lay.take(p.chunks * dt * 8);
    p.csum = lay.take(dt * 8), p.part = lay.take(p.nblocks * NSUM * 8), p.total = lay.end;
    return p;
}

struct RbfPlan { int chunks, splits, ntiles; long long strips, colsum, mean, norms, pair, rowpart, part, nblocks, total; };

RbfPlan rbf_plan(long long n, int da, int db, int splits) {
    RbfPlan p;
    const long long dt = (long long)da + db;
    p.chunks = umlh_align_cka_sum_chunks(n);
    p.splits = umlh_align_knn_splits(n, splits);     // the same strips and tiles as the k-NN pass
    p.ntiles = (int)((n + TK_COLS - 1) / TK_COLS);
    p.strips = (n + TK_ROWS - 1) / TK_ROWS;
    p.nblocks = (n + 255) / 256;
    ScratchLayout lay;
    p.colsum = lay.take(p.chunks * dt * 8), p.mean = lay.take((long long)(up4(da) + up4(db)) * 4), p.norms = lay.take(2 * n * 4);
    p.pair = lay.take(3 * p.splits * p.strips * 8);
    p.rowpart = lay.take(p.splits * p.strips * TK_ROWS * 2 * 8);
    p.part = lay.take(p.nblocks * NSUM * 8), p.total = lay.end;
    return p;
}

struct CknnaPlan { long long nblocks, rsum, part, total; };

CknnaPlan cknna_plan(long long n) {
    CknnaPlan p;
    ScratchLayout lay;
    p.nblocks = (n + 255) / 256;
    p.rsum = lay.take(n * 4 * 8), p.part = lay.take(p.nblocks * NSUM * 8), p.total = lay.end;
    return p;
}

}  // namespace

// ---- plans and launchers (validation is the caller's: umlh_ops.cpp) ----
extern "C" {

unsigned long long umlh_align_ext_cka_unbiased_bytes(long long n, int da, int db, int splits) {
    return (unsigned long long)unbiased_plan(n, da, db, splits).total;
}

unsigned long long umlh_align_ext_rbf_bytes(long long n, int da, int db, int splits) {
    return (unsigned long long)rbf_plan(n, da, db, splits).total;
}

unsigned long long umlh_align_ext_cknna_bytes(long long n) { return (unsigned long long)cknna_plan(n).total; }

unsigned long long umlh_align_ext_list_bytes(long long n) { return (unsigned long long)align_up((n + 63) / 64 * 3 * 8); }

int umlh_align_ext_launch_cka_unbiased(const float* a, int lda, int da, const float* b, int ldb, int db, long long n, int splits,
                                       double* out4, void* scratch, hipStream_t st) {
    const UnbiasedPlan p = unbiased_plan(n, da, db, splits);
    const int dt = da + db, ta = (da + 31) / 32, tb = (db + 31) / 32;
    const int e = umlh_align_launch_cka_products(a, lda, da, b, ldb, db, n, splits, scratch, st);
    if (e) return e;
    const double* colsum = at<double>(scratch, 0);
    float* mean = at<float>(scratch, p.mean);
    hipLaunchKernelGGL(ext_means, dim3((unsigned)((up4(da) + up4(db) + 255) / 256)), dim3(256), 0, st, colsum, p.chunks, da, db, (int)n,
                       mean);
    hipLaunchKernelGGL(ext_center_sums, dim3((unsigned)((dt + 63) / 64), (unsigned)p.chunks), dim3(256), 0, st, a, lda, da, b, ldb, db,
                       (int)n, p.chunks, mean, at<double>(scratch, p.part2));
    hipLaunchKernelGGL(ext_colfin, dim3((unsigned)((dt + 255) / 256)), dim3(256), 0, st, at<double>(scratch, p.part2), p.chunks, dt,
                       at<double>(scratch, p.csum));
    RowArgs g;
    g.a = a; g.b = b; g.lda = lda; g.ldb = ldb; g.da = da; g.db = db; g.n = n; g.mean = mean;
    g.csum = at<double>(scratch, p.csum); g.norms = nullptr; g.part = at<double>(scratch, p.part);
    hipLaunchKernelGGL(ext_rows<0>, dim3((unsigned)p.nblocks), dim3(256), 0, st, g);
    hipLaunchKernelGGL(ext_final, dim3(1), dim3(256), 0, st,
                       at<double>(scratch, umlh_align_cka_tile_sq_offset(n, da, db, splits)), (long long)ta * tb, (long long)ta * ta,
                       (long long)tb * tb, g.part, p.nblocks, (double)n, 1, out4);
    return (int)hipGetLastError();
}

int umlh_align_ext_launch_rbf(const float* a, int lda, int da, const float* b, int ldb, int db, long long n, double sigma,
                              int unbiased, int splits, double* out4, void* scratch, hipStream_t st) {
    const RbfPlan p = rbf_plan(n, da, db, splits);
    int e = umlh_align_launch_colsum(a, lda, da, b, ldb, db, n, at<double>(scratch, p.colsum), st);
    if (e) return e;
    float* mean = at<float>(scratch, p.mean);
    hipLaunchKernelGGL(ext_means, dim3((unsigned)((up4(da) + up4(db) + 255) / 256)), dim3(256), 0, st, at<double>(scratch, p.colsum),
                       p.chunks, da, db, (int)n, mean);
    RowArgs r;
    r.a = a; r.b = b; r.lda = lda; r.ldb = ldb; r.da = da; r.db = db; r.n = n; r.mean = mean;
    r.csum = nullptr; r.norms = at<float>(scratch, p.norms); r.part = nullptr;
    hipLaunchKernelGGL(ext_rows<1>, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, r);
    RbfArgs g;
    g.a = a; g.b = b; g.mean = mean; g.norms = r.norms; g.lda = lda; g.ldb = ldb; g.da = da; g.db = db; g.n = (int)n;
    g.ntiles = p.ntiles; g.splits = p.splits; g.strips = (int)p.strips; g.unbiased = unbiased;
    g.gamma = (float)(1.0 / (2.0 * sigma * sigma));
    g.pair = at<double>(scratch, p.pair); g.rowpart = at<double>(scratch, p.rowpart);
    const dim3 grid((unsigned)p.strips, (unsigned)p.splits);
    const bool vec = da % 4 == 0 && db % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
    if (vec) hipLaunchKernelGGL(rbf_tiles<true>, grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(rbf_tiles<false>, grid, dim3(256), 0, st, g);
    double* part = at<double>(scratch, p.part);
    hipLaunchKernelGGL(rbf_rows, dim3((unsigned)p.nblocks), dim3(256), 0, st, g.rowpart, p.splits, p.strips * TK_ROWS, (int)n, part);
    const long long nwg = p.splits * p.strips;
    hipLaunchKernelGGL(ext_final, dim3(1), dim3(256), 0, st, g.pair, nwg, nwg, nwg, part, p.nblocks, (double)n, unbiased, out4);
    return (int)hipGetLastError();
}

int umlh_align_ext_launch_cknna(const int* ka, const float* sa, const int* kb, const float* sb, long long n, int topk, double* out4,
                                void* scratch, hipStream_t st) {
    const CknnaPlan p = cknna_plan(n);
    double *rsum = at<double>(scratch, p.rsum), *part = at<double>(scratch, p.part);
    hipLaunchKernelGGL(cknna_rowsum, dim3((unsigned)p.nblocks), dim3(256), 0, st, ka, sa, kb, sb, (int)n, topk, rsum);
    hipLaunchKernelGGL(cknna_rows, dim3((unsigned)p.nblocks), dim3(256), 0, st, ka, sa, kb, sb, (int)n, topk, rsum, part);
    hipLaunchKernelGGL(ext_final, dim3(1), dim3(256), 0, st, part, 0LL, 0LL, 0LL, part, p.nblocks, (double)n, 1, out4);
    return (int)hipGetLastError();
}

int umlh_align_ext_launch_list_stats(const int* ka, const int* kb, long long n, int topk, int* rows, double* out3, void* scratch,
                                     hipStream_t st) {
    const long long nblocks = (n + 63) / 64;
    long long* part = at<long long>(scratch, 0);
    hipLaunchKernelGGL(list_rows, dim3((unsigned)nblocks), dim3(64), 0, st, ka, kb, (int)n, topk, rows, part);
    hipLaunchKernelGGL(list_final, dim3(1), dim3(256), 0, st, part, nblocks, (int)n, topk, out3);
    return (int)hipGetLastError();
}

}  // extern "C"
