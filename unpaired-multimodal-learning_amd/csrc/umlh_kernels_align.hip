// Representation-alignment metrics of the reference (vision_language/metrics.py:55-84,96-119,252-255,272-285) for gfx950.
//
//   knn_tiles      fused Gram tile x_i . x_j on v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma chain) + a streaming
//                  per-row top-k under the strict order (score desc, index asc); one partial list per column chunk
//   knn_merge      merges the chunks' lists of a row -> knn int32 [N, k] (+ scores fp32 [N, k])
//   mutual_count   |knn_a(i) n knn_b(i)| per row, integer block sums
//   mutual_final   fixed-order sum of the block counts -> mean as double
//   cka_colsum     column sums of A | B in double, per row chunk (colsum_chunk, umlh_gram.h)
//   cka_cross      the centred cross products Ac^T Bc, Ac^T Ac, Bc^T Bc as 32x32 tiles on the f32 MFMA, per row chunk
//                  (centred on load: never X^T Y - N mu mu^T): mfma32_rows_tile of umlh_gram.h on the centring loader
//   cka_tile_sq    each finished tile (its row chunks summed in double, fixed order), squared and summed
//   cka_final      fixed-order Frobenius sums -> {cka, hsic_kl, hsic_kk, hsic_ll}
//
// Nothing here forms an N x N array, and no reduction uses a float atomic: every result is bitwise reproducible for a
// given `splits`.  knn is bitwise independent of `splits` as well: column chunks start on 256-column tile boundaries,
// every score is the same fma chain wherever it is computed, and the kept lists are exact top-k under a strict order.
// The tile, column-sum and chunk-sum bodies are those of umlh_gram.h (shared with umlh_kernels_probe.hip,
// umlh_kernels_align_ext.hip and umlh_kernels_spectral.hip), the block reductions block_reduce of umlh_common.h.
#include "umlh_common.h"
#include "umlh_gram.h"
#include "umlh_launch.h"
#include "umlh_topk.h"
#include <climits>

namespace {

constexpr int CK_TARGET_WG = 512;
constexpr int CK_SUM_CHUNKS = 64;        // row chunks of the column sums
constexpr int CK_MAX_RCHUNKS = 4096;     // (grid y)

// One matrix against itself: raw inner products, column i left out of row i's list.
struct KnnSelf : TopkOperands {
    static constexpr bool EXCLUDE_SELF = true;
    __device__ float col_term(long long) const { return 0.f; }
    __device__ static float score(float acc, float) { return acc; }
};

// Stage 1 (topk_tiles, umlh_topk.h): rows [32 blockIdx.x, +32) x the column tiles of chunk blockIdx.y -> one partial list.
template <bool VEC>
__global__ __launch_bounds__(256) void knn_tiles(const float* __restrict__ x, int n, int d, int ldx, int topk, int ntiles,
                                                 int splits, float* __restrict__ part_s, int* __restrict__ part_i) {
    topk_tiles<VEC>(KnnSelf{{x, x, n, ldx, n, ldx, d, topk}}, ntiles, splits, part_s, part_i);
}

// Stage 2 (topk_merge).  A list entry that no column filled (a row of NaN scores) is published as INT_MAX - e, e >= 0: never
// a row index, since n <= 2^30.
__global__ __launch_bounds__(64) void knn_merge(const float* __restrict__ part_s, const int* __restrict__ part_i, int n, int topk,
                                                int splits, int* __restrict__ knn, float* __restrict__ scores) {
    topk_merge(part_s, part_i, n, topk, splits, [=](long long o, float s, int j) {
        knn[o] = j < 0 ? INT_MAX - (-1 - j) : j;
        if (scores) scores[o] = s;
    });
}

__global__ __launch_bounds__(256) void mutual_count(const int* __restrict__ ka, const int* __restrict__ kb, int n, int topk,
                                                    long long* __restrict__ partial) {
    __shared__ int red[256];
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x * 256 + tid;
    int c = 0;
    if (row < n) {
        const int* a = ka + row * topk;
        const int* b = kb + row * topk;
        for (int p = 0; p < topk; ++p) {
            const int ja = a[p];
            int hit = 0;
            for (int q = 0; q < topk; ++q) hit |= (b[q] == ja);
            c += hit;
        }
    }
    c = block_reduce<256>(c, red, OpSum());
    if (tid == 0) partial[blockIdx.x] = c;
}

__global__ __launch_bounds__(256) void mutual_final(const long long* __restrict__ partial, int nblocks, int n, int topk,
                                                    double* __restrict__ out) {
    __shared__ long long red[256];
    const int tid = threadIdx.x;
    long long c = 0;
    for (int b = tid; b < nblocks; b += 256) c += partial[b];
    c = block_reduce<256>(c, red, OpSum());
    if (tid == 0) out[0] = (double)c / ((double)n * (double)topk);
}

// Column c of A | B (c < da: A), rows of chunk blockIdx.y, in double (colsum_chunk, umlh_gram.h).
__global__ __launch_bounds__(256) void cka_colsum(const float* __restrict__ a, int lda, int da, const float* __restrict__ b, int ldb,
                                                  int db, int n, int chunks, double* __restrict__ partial) {
    colsum_chunk([=](int c) {
        const float* p = c < da ? a + c : b + (c - da);
        const long long ld = c < da ? lda : ldb;
        return [=](long long r) { return (double)p[r * ld]; };
    }, da + db, n, chunks, partial);
}

struct CkaArgs {
    const float* a;
    const float* b;
    int lda, ldb, da, db, ta, tb;            // ta, tb: 32-column tiles of A and B
    int n, sum_chunks, rchunks;
    const double* colsum;                    // [sum_chunks][da + db]
    double* cross;                           // [tiles][rchunks][1024]
    double* tile_sq;                         // [tiles]
};

// Tile blockIdx.x of the three products (A^T B: ta*tb tiles, A^T A: ta*ta, B^T B: tb*tb), rows of chunk blockIdx.y (whole
// 32-row blocks): mfma32_rows_tile (umlh_gram.h) on mean-centred columns; lane (h, c32) loads column c32 of the tile, rows 4h ..
__global__ __launch_bounds__(256) void cka_cross(CkaArgs g) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c32 = lane & 31;
    int t = blockIdx.x, ti, tj;
    const float *X, *Y;
    int ldx, ldy, dx, dy, ox, oy;            // ox, oy: offsets of X's / Y's columns in the column sums
    if (t < g.ta * g.tb) {
        X = g.a; ldx = g.lda; dx = g.da; ox = 0; Y = g.b; ldy = g.ldb; dy = g.db; oy = g.da; ti = t / g.tb; tj = t % g.tb;
    } else if ((t -= g.ta * g.tb) < g.ta * g.ta) {
        X = g.a; ldx = g.lda; dx = g.da; ox = 0; Y = g.a; ldy = g.lda; dy = g.da; oy = 0; ti = t / g.ta; tj = t % g.ta;
    } else {
        t -= g.ta * g.ta;
        X = g.b; ldx = g.ldb; dx = g.db; ox = g.da; Y = g.b; ldy = g.ldb; dy = g.db; oy = g.da; ti = t / g.tb; tj = t % g.tb;
    }
    const int cx = ti * 32 + c32, cy = tj * 32 + c32, dt = g.da + g.db;
    // column means (fixed-order double sums of the chunk partials): lanes 0-31 for X's column, 32-63 for Y's
    float mean;
    {
        const int col = h ? cy : cx, lim = h ? dy : dx, off = h ? oy : ox;
        mean = (float)((col < lim ? chunk_total(g.colsum, g.sum_chunks, dt, off + col) : 0.0) / (double)g.n);
    }
    const float mx = __shfl(mean, c32), my = __shfl(mean, 32 + c32);
    const bool vx = cx < dx, vy = cy < dy;
    long long rs, re;
    chunk_rows32(g.n, blockIdx.y, g.rchunks, rs, re);
    mfma32_rows_tile<true>([&](long long r0, float* xv, float* yv) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long long r = r0 + s;
            const bool vr = r < re;
            xv[s] = (vr && vx) ? X[r * ldx + cx] - mx : 0.f;
            yv[s] = (vr && vy) ? Y[r * ldy + cy] - my : 0.f;
        }
    }, rs, re, g.cross + ((long long)blockIdx.x * g.rchunks + blockIdx.y) * 1024);
}

__global__ __launch_bounds__(256) void cka_tile_sq(const double* __restrict__ cross, int rchunks, double* __restrict__ tile_sq) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const double* p = cross + (long long)blockIdx.x * rchunks * 1024;
    double sq = 0.0;
    for (int e = tid; e < 1024; e += 256) {
        const double v = slab_total(p, rchunks, e);
        sq += v * v;
    }
    sq = block_reduce<256>(sq, red, OpSum());
    if (tid == 0) tile_sq[blockIdx.x] = sq;
}

__global__ __launch_bounds__(256) void cka_final(const double* __restrict__ tile_sq, int ta, int tb, double* __restrict__ out4) {
    __shared__ double red[256];
    double hs[3];
    const int tid = threadIdx.x;
    const int lo[3] = {0, ta * tb, ta * tb + ta * ta}, hi[3] = {ta * tb, ta * tb + ta * ta, ta * tb + ta * ta + tb * tb};
    for (int p = 0; p < 3; ++p) {
        double s = 0.0;
        for (int t = lo[p] + tid; t < hi[p]; t += 256) s += tile_sq[t];
        hs[p] = block_reduce<256>(s, red, OpSum());
    }
    if (tid == 0) {   // metrics.py:116: hsic_kl / (sqrt(hsic_kk * hsic_ll) + 1e-6)
        out4[0] = hs[0] / (sqrt(hs[1] * hs[2]) + 1e-6);
        out4[1] = hs[0];
        out4[2] = hs[1];
        out4[3] = hs[2];
    }
}

}  // namespace

// ---- plans and launchers (validation is the caller's: umlh_ops.cpp) ----
extern "C" {

int umlh_align_knn_splits(long long n, int splits) { return topk_splits(n, n, splits); }

// One stage, margin 0 (topk < n): the scratch is the two list slabs, which end where candidates would start.
unsigned long long umlh_align_knn_bytes(long long n, int topk, int splits) {
    return (unsigned long long)topk_plan(n, n, topk, 0, splits, 0).cand;
}

unsigned long long umlh_align_mutual_bytes(long long n) { return (unsigned long long)align_up((n + 255) / 256 * 8); }

struct CkaPlan { int ta, tb, tiles, rchunks, sum_chunks; long long colsum, cross, tile_sq, total; };

static CkaPlan cka_plan(long long n, int da, int db, int splits) {
    CkaPlan p;
    p.ta = (da + 31) / 32;
    p.tb = (db + 31) / 32;
    p.tiles = p.ta * p.tb + p.ta * p.ta + p.tb * p.tb;
    const long long nb = (n + 31) / 32;
    long long r = splits > 0 ? splits : (p.tiles >= CK_TARGET_WG ? 1 : (CK_TARGET_WG + p.tiles - 1) / p.tiles);
    if (splits <= 0 && r > nb / 4) r = nb / 4;   // auto: at least 128 rows per chunk
    if (r > CK_MAX_RCHUNKS) r = CK_MAX_RCHUNKS;
    p.rchunks = (int)(r < 1 ? 1 : (r > nb ? nb : r));
    p.sum_chunks = umlh_align_cka_sum_chunks(n);
    ScratchLayout lay;
    p.colsum = lay.take((long long)p.sum_chunks * (da + db) * 8);
    p.cross = lay.take((long long)p.tiles * p.rchunks * 1024 * 8);
    p.tile_sq = lay.take((long long)p.tiles * 8), p.total = lay.end;
    return p;
}

unsigned long long umlh_align_cka_bytes(long long n, int da, int db, int splits) {
    return (unsigned long long)cka_plan(n, da, db, splits).total;
}

int umlh_align_launch_knn(const float* x, long long n, int d, int ldx, int topk, int splits, int* knn, float* scores, void* scratch,
                          hipStream_t st) {
    const TopkPlan p = topk_plan(n, n, topk, 0, splits, 0);
    float* ps = at<float>(scratch, p.part_s);
    int* pi = at<int>(scratch, p.part_i);
    topk_launch_tiles(knn_tiles<true>, knn_tiles<false>, topk_vec_ok(d, ldx, ldx, x, x), n, p.splits, st, x, (int)n, d, ldx, topk,
                      p.ntiles, p.splits, ps, pi);
    hipLaunchKernelGGL(knn_merge, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, ps, pi, (int)n, topk, p.splits, knn, scores);
    return (int)hipGetLastError();
}

int umlh_align_launch_mutual(const int* ka, const int* kb, long long n, int topk, double* out, void* scratch, hipStream_t st) {
    const int nblocks = (int)((n + 255) / 256);
    long long* partial = at<long long>(scratch, 0);
    hipLaunchKernelGGL(mutual_count, dim3((unsigned)nblocks), dim3(256), 0, st, ka, kb, (int)n, topk, partial);
    hipLaunchKernelGGL(mutual_final, dim3(1), dim3(256), 0, st, partial, nblocks, (int)n, topk, out);
    return (int)hipGetLastError();
}

int umlh_align_cka_sum_chunks(long long n) { return (int)(n < CK_SUM_CHUNKS * 64 ? (n + 63) / 64 : CK_SUM_CHUNKS); }

long long umlh_align_cka_tile_sq_offset(long long n, int da, int db, int splits) { return cka_plan(n, da, db, splits).tile_sq; }

int umlh_align_launch_colsum(const float* a, int lda, int da, const float* b, int ldb, int db, long long n, double* partial,
                             hipStream_t st) {
    const int chunks = umlh_align_cka_sum_chunks(n);
    hipLaunchKernelGGL(cka_colsum, dim3((unsigned)((da + db + 63) / 64), (unsigned)chunks), dim3(256), 0, st, a, lda, da, b, ldb, db,
                       (int)n, chunks, partial);
    return (int)hipGetLastError();
}

// The column sums (scratch + 0: [sum_chunks][da + db]) and the squared Frobenius sum of every 32x32 tile of Ac^T Bc, Ac^T Ac,
// Bc^T Bc (scratch + tile_sq offset: ta*tb, then ta*ta, then tb*tb tiles); cka_final or the unbiased form finishes from them.
int umlh_align_launch_cka_products(const float* a, int lda, int da, const float* b, int ldb, int db, long long n, int splits,
                                   void* scratch, hipStream_t st) {
    const CkaPlan p = cka_plan(n, da, db, splits);
    CkaArgs g;
    g.a = a; g.b = b; g.lda = lda; g.ldb = ldb; g.da = da; g.db = db; g.ta = p.ta; g.tb = p.tb;
    g.n = (int)n; g.sum_chunks = p.sum_chunks; g.rchunks = p.rchunks;
    g.colsum = at<double>(scratch, p.colsum);
    g.cross = at<double>(scratch, p.cross);
    g.tile_sq = at<double>(scratch, p.tile_sq);
    hipLaunchKernelGGL(cka_colsum, dim3((unsigned)((da + db + 63) / 64), (unsigned)p.sum_chunks), dim3(256), 0, st, a, lda, da, b, ldb,
                       db, (int)n, p.sum_chunks, (double*)g.colsum);
    hipLaunchKernelGGL(cka_cross, dim3((unsigned)p.tiles, (unsigned)p.rchunks), dim3(256), 0, st, g);
    hipLaunchKernelGGL(cka_tile_sq, dim3((unsigned)p.tiles), dim3(256), 0, st, g.cross, p.rchunks, g.tile_sq);
    return (int)hipGetLastError();
}

int umlh_align_launch_cka(const float* a, int lda, int da, const float* b, int ldb, int db, long long n, int splits, double* out4,
                          void* scratch, hipStream_t st) {
    const CkaPlan p = cka_plan(n, da, db, splits);
    const int e = umlh_align_launch_cka_products(a, lda, da, b, ldb, db, n, splits, scratch, st);
    if (e) return e;
    hipLaunchKernelGGL(cka_final, dim3(1), dim3(256), 0, st, (const double*)at<double>(scratch, p.tile_sq), p.ta, p.tb, out4);
    return (int)hipGetLastError();
}

}  // extern "C"
