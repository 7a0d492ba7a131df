// The Gram tile bodies and the column-sum body that the metric kernels share: the fp64-FMA 64 x 64 tile of spectral_gram and
// subspace_gram (umlh_kernels_spectral.hip), the fp32-MFMA 32 x 32 row-chunk tile of cka_cross (umlh_kernels_align.hip) and
// pb_gram (umlh_kernels_probe.hip), and the per-row-chunk column sums of cka_colsum, ext_center_sums (umlh_kernels_align_ext.hip)
// and pb_colsum.  Device code for the .hip files only; the kernels stay where they are launched and plug in how an element is
// fetched.  No body branches on its caller, and every sum runs in one fixed order: a kernel's bits depend on its loader alone.
#pragma once
#include "umlh_common.h"

// ---- upper-triangular tile pairs: tile t of the nt (nt + 1) / 2 pairs (ti <= tj), row by row ----
inline int tri_tiles(int nt) { return nt * (nt + 1) / 2; }

__device__ __forceinline__ void tri_tile(int t, int nt, int& ti, int& tj) {
    ti = 0;
    while (t >= nt - ti) { t -= nt - ti; ++ti; }
    tj = ti + t;
}

// ---- fp64-FMA tile ----
constexpr int G64_TILE = 64;              // tile edge
constexpr int G64_KR = 32;                // rows staged per step

// One workgroup (256 threads): the G64_TILE x G64_TILE tile (ti, tj) of sum over rows [r0, r1) of a_row^T b_row, rows ascending,
// 4 x 4 fp64 fma accumulators per thread, written to slab [rows_out, cols_out] where it lies inside.  cols(ca, cb) gives the
// fetch of the thread's two columns (what is loop-invariant for them is set up once there): a functor load(row, va, vb) that
// sets va = a[row][ca], vb = b[row][cb] and leaves them as they come (zero) for a column outside the matrix or a row that
// does not count.  T is the LDS staging type, converted to double on use.
template <class T, class C>
__device__ __forceinline__ void gram64_tile(const C& cols, int ti, int tj, unsigned r0, unsigned r1, double* __restrict__ slab,
                                            int rows_out, int cols_out) {
    __shared__ __align__(16) T sa[G64_KR][G64_TILE];
    __shared__ __align__(16) T sb[G64_KR][G64_TILE];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lc = tid & 63, lr = tid >> 6;
    const auto load = cols(ti * G64_TILE + lc, tj * G64_TILE + lc);
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (unsigned rs = r0; rs < r1; rs += G64_KR) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < G64_KR / 4; ++q) {
            const unsigned r = rs + lr + 4 * q;
            T va = 0, vb = 0;
            if (r < r1) load(r, va, vb);
            sa[lr + 4 * q][lc] = va;
            sb[lr + 4 * q][lc] = vb;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < G64_KR; ++k) {
            double a4[4], b4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a4[i] = (double)sa[k][ty * 4 + i]; b4[i] = (double)sb[k][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(a4[i], b4[j], acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gi = ti * G64_TILE + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gj = tj * G64_TILE + tx * 4 + j;
            if (gi < rows_out && gj < cols_out) slab[(long long)gi * cols_out + gj] = acc[i][j];
        }
    }
}

// Thread per element idx of a matrix of `total` elements: the sum of its `chunks` slabs (`total` apart) in chunk order.
// MIRROR (square, cols x cols; cols is unused otherwise): only i <= j is summed, and stored at (j, i) as well.
template <bool MIRROR>
__device__ __forceinline__ void slab_sum(const double* __restrict__ slabs, long long total, int cols, int chunks,
                                         double* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int i = MIRROR ? (int)idx / cols : 0, j = MIRROR ? (int)idx - i * cols : 0;     // MIRROR: total = cols^2 < 2^31
    if (MIRROR && i > j) return;
    double v = 0.0;
    for (int c = 0; c < chunks; ++c) v += slabs[(long long)c * total + idx];
    out[idx] = v;
    if (MIRROR) out[(long long)j * cols + i] = v;
}

// ---- fp32-MFMA row-chunk tile ----
// Rows of chunk y of `rchunks` over n rows, in whole 32-row blocks: [rs, re).
__device__ __forceinline__ void chunk_rows32(long long n, int y, int rchunks, long long& rs, long long& re) {
    const long long nb = (n + 31) / 32;
    rs = (long long)y * nb / rchunks * 32;
    re = (long long)(y + 1) * nb / rchunks * 32;
    if (re > n) re = n;
}

// One workgroup (256 threads): the 32 x 32 tile sum over rows [rs, re) of a_row^T b_row on v_mfma_f32_32x32x2_f32 -> out[1024]
// in double.  Wave w takes the 8-row groups w, w+4, ... of the chunk; lane half h supplies rows 4h + s to MFMA step s;
// load(r, xv, yv) gives the lane's (a, b) values of rows r .. r+3 (zero at or past re, or outside the matrix; r may lie one
// group past re).  PREFETCH: the next group is in registers before the current one is multiplied (the loads and the MFMA
// order are the same either way; a loader that needs many registers per value may lose a wave of occupancy to it).  The
// four waves' tiles are exchanged through LDS and added in wave order in double.
template <bool PREFETCH, class L>
__device__ __forceinline__ void mfma32_rows_tile(const L& load, long long rs, long long re, double* __restrict__ out) {
    __shared__ float red[4][1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c32 = lane & 31;
    f32x16 acc = {};
    long long base = rs + wave * 8;
    float xv[4], yv[4], xn[4], yn[4];
    if (PREFETCH) load(base + 4 * h, xv, yv);
    for (; base < re; base += 32) {
        if (PREFETCH) load(base + 32 + 4 * h, xn, yn);
        else load(base + 4 * h, xv, yv);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[s], yv[s], acc, 0, 0, 0);
        if (PREFETCH) {
#pragma unroll
            for (int s = 0; s < 4; ++s) { xv[s] = xn[s]; yv[s] = yn[s]; }
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) red[wave][(8 * (q >> 2) + 4 * h + (q & 3)) * 32 + c32] = acc[q];
    __syncthreads();
    for (int e = tid; e < 1024; e += 256)
        out[e] = (((double)red[0][e] + (double)red[1][e]) + (double)red[2][e]) + (double)red[3][e];
}

// element e of a tile: its `rchunks` slabs (1024 apart) in chunk order
__device__ __forceinline__ double slab_total(const double* __restrict__ p, int rchunks, int e) {
    double v = 0.0;
    for (int r = 0; r < rchunks; ++r) v += p[(long long)r * 1024 + e];
    return v;
}

// ---- column sums per row chunk ----
// One workgroup (256 threads): columns [64 blockIdx.x, +64) x the rows of chunk blockIdx.y of `chunks` over n rows, 4 row
// lanes per column, in double -> partial[chunk][ncols].  col(c) gives column c's term: a functor row -> double (its source,
// stride and element transform).
template <class C>
__device__ __forceinline__ void colsum_chunk(const C& col, int ncols, long long n, int chunks, double* __restrict__ partial) {
    __shared__ double red[256];
    const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6, c = blockIdx.x * 64 + cl;
    const long long rs = (long long)blockIdx.y * n / chunks, re = (long long)(blockIdx.y + 1) * n / chunks;
    double s = 0.0;
    if (c < ncols) {
        const auto term = col(c);
        for (long long r = rs + rl; r < re; r += 4) s += term(r);
    }
    red[tid] = s;
    __syncthreads();
    if (rl == 0 && c < ncols) partial[(long long)blockIdx.y * ncols + c] = ((red[cl] + red[64 + cl]) + red[128 + cl]) + red[192 + cl];
}

// column c: its `chunks` partials (`stride` apart) in chunk order
__device__ __forceinline__ double chunk_total(const double* __restrict__ partial, int chunks, long long stride, int c) {
    double s = 0.0;
    for (int q = 0; q < chunks; ++q) s += partial[(long long)q * stride + c];
    return s;
}
