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
//   *_pairs        the same eight over the members of umlh_align_pairs, one launch each: member (x view) = blockIdx.z, then the
//                  single kernel's body on that member's entry of a device descriptor table
//
// Nothing here forms an N x N array, and no reduction uses a float atomic: every result is bitwise reproducible for a
// given `splits`.  knn is bitwise independent of `splits` as well: column chunks start on 256-column tile boundaries,
// every score is the same fma chain wherever it is computed, and the kept lists are exact top-k under a strict order.
// The tile, column-sum and chunk-sum bodies are those of umlh_gram.h (shared with umlh_kernels_probe.hip,
// umlh_kernels_align_ext.hip and umlh_kernels_spectral.hip), the block reductions block_reduce of umlh_common.h.
#include "umlh_common.h"
#include "umlh_gram.h"
#include "umlh_launch.h"
#include "umlh_stage.h"
#include "umlh_topk.h"
#include <algorithm>
#include <climits>
#include <cstring>

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

__device__ __forceinline__ void mutual_count_body(const int* __restrict__ ka, const int* __restrict__ kb, int n, int topk,
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

__global__ __launch_bounds__(256) void mutual_count(const int* __restrict__ ka, const int* __restrict__ kb, int n, int topk,
                                                    long long* __restrict__ partial) {
    mutual_count_body(ka, kb, n, topk, partial);
}

__device__ __forceinline__ void mutual_final_body(const long long* __restrict__ partial, int nblocks, int n, int topk,
                                                  double* __restrict__ out) {
    __shared__ long long red[256];
    const int tid = threadIdx.x;
    long long c = 0;
    for (int b = tid; b < nblocks; b += 256) c += partial[b];
    c = block_reduce<256>(c, red, OpSum());
    if (tid == 0) out[0] = (double)c / ((double)n * (double)topk);
}

__global__ __launch_bounds__(256) void mutual_final(const long long* __restrict__ partial, int nblocks, int n, int topk,
                                                    double* __restrict__ out) {
    mutual_final_body(partial, nblocks, n, topk, out);
}

// Column c of A | B (c < da: A), rows of chunk blockIdx.y, in double (colsum_chunk, umlh_gram.h).
__device__ __forceinline__ void cka_colsum_body(const float* __restrict__ a, int lda, int da, const float* __restrict__ b, int ldb,
                                                int db, int n, int chunks, double* __restrict__ partial) {
    colsum_chunk([=](int c) {
        const float* p = c < da ? a + c : b + (c - da);
        const long long ld = c < da ? lda : ldb;
        return [=](long long r) { return (double)p[r * ld]; };
    }, da + db, n, chunks, partial);
}

__global__ __launch_bounds__(256) void cka_colsum(const float* __restrict__ a, int lda, int da, const float* __restrict__ b, int ldb,
                                                  int db, int n, int chunks, double* __restrict__ partial) {
    cka_colsum_body(a, lda, da, b, ldb, db, n, chunks, partial);
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
__device__ __forceinline__ void cka_cross_body(const CkaArgs& g) {
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

__global__ __launch_bounds__(256) void cka_cross(CkaArgs g) { cka_cross_body(g); }

__device__ __forceinline__ void cka_tile_sq_body(const double* __restrict__ cross, int rchunks, double* __restrict__ tile_sq) {
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

__global__ __launch_bounds__(256) void cka_tile_sq(const double* __restrict__ cross, int rchunks, double* __restrict__ tile_sq) {
    cka_tile_sq_body(cross, rchunks, tile_sq);
}

__device__ __forceinline__ void cka_final_body(const double* __restrict__ tile_sq, int ta, int tb, double* __restrict__ out4) {
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

__global__ __launch_bounds__(256) void cka_final(const double* __restrict__ tile_sq, int ta, int tb, double* __restrict__ out4) {
    cka_final_body(tile_sq, ta, tb, out4);
}

// ---- grouped forms (umlh_align_pairs): the eight kernels above over many pairs in one launch each ----
// A workgroup takes its member (for the k-NN kernels its member x view) from blockIdx.z, copies that entry of a device descriptor
// table into locals, leaves -- the whole workgroup, before any barrier -- when (blockIdx.x, blockIdx.y) lies outside the entry's
// own grid, and then runs the very body the single kernel runs with the entry's operands, plan pointers and chunk counts: the
// bodies read blockIdx.x and .y alone.  Per entry the words written are those of the single launches.
struct PairCka {                             // one member that asks for the CKA
    CkaArgs g;
    int tiles;
    double* out;                             // out5
};

struct PairView {                            // one view of a member that asks for lists
    const float* x;
    int n, d, ldx, topk, ntiles, splits;
    float* part_s;
    int* part_i;
    int* knn;
    float* scores;
};

struct PairMutual {                          // one member that asks for lists
    const int* ka;
    const int* kb;
    int n, topk, nblocks;
    long long* partial;
    double* out;                             // out5 + 4
};

__global__ __launch_bounds__(256) void cka_colsum_pairs(const PairCka* __restrict__ tab) {
    const CkaArgs g = tab[blockIdx.z].g;
    if ((int)blockIdx.x >= (g.da + g.db + 63) / 64 || (int)blockIdx.y >= g.sum_chunks) return;
    cka_colsum_body(g.a, g.lda, g.da, g.b, g.ldb, g.db, g.n, g.sum_chunks, const_cast<double*>(g.colsum));
}

__global__ __launch_bounds__(256) void cka_cross_pairs(const PairCka* __restrict__ tab) {
    const CkaArgs g = tab[blockIdx.z].g;
    if ((int)blockIdx.x >= tab[blockIdx.z].tiles || (int)blockIdx.y >= g.rchunks) return;
    cka_cross_body(g);
}

__global__ __launch_bounds__(256) void cka_tile_sq_pairs(const PairCka* __restrict__ tab) {
    const double* cross = tab[blockIdx.z].g.cross;
    double* tile_sq = tab[blockIdx.z].g.tile_sq;
    const int rchunks = tab[blockIdx.z].g.rchunks;
    if ((int)blockIdx.x >= tab[blockIdx.z].tiles) return;
    cka_tile_sq_body(cross, rchunks, tile_sq);
}

__global__ __launch_bounds__(256) void cka_final_pairs(const PairCka* __restrict__ tab) {   // out[4] is not touched
    const double* tile_sq = tab[blockIdx.z].g.tile_sq;
    cka_final_body(tile_sq, tab[blockIdx.z].g.ta, tab[blockIdx.z].g.tb, tab[blockIdx.z].out);
}

// One kernel per load form: topk_tiles' static LDS would count twice in a kernel that held both.
template <bool VEC>
__global__ __launch_bounds__(256) void knn_tiles_pairs(const PairView* __restrict__ tab) {
    const PairView v = tab[blockIdx.z];
    if ((int)blockIdx.x >= (v.n + TK_ROWS - 1) / TK_ROWS || (int)blockIdx.y >= v.splits) return;
    topk_tiles<VEC>(KnnSelf{{v.x, v.x, v.n, v.ldx, v.n, v.ldx, v.d, v.topk}}, v.ntiles, v.splits, v.part_s, v.part_i);
}

__global__ __launch_bounds__(64) void knn_merge_pairs(const PairView* __restrict__ tab) {
    const PairView v = tab[blockIdx.z];
    if ((int)blockIdx.x >= (v.n + 63) / 64) return;
    int* knn = v.knn;
    float* scores = v.scores;
    topk_merge(v.part_s, v.part_i, v.n, v.topk, v.splits, [=](long long o, float s, int j) {
        knn[o] = j < 0 ? INT_MAX - (-1 - j) : j;
        if (scores) scores[o] = s;
    });
}

__global__ __launch_bounds__(256) void mutual_count_pairs(const PairMutual* __restrict__ tab) {
    const PairMutual m = tab[blockIdx.z];
    if ((int)blockIdx.x >= m.nblocks) return;
    mutual_count_body(m.ka, m.kb, m.n, m.topk, m.partial);
}

__global__ __launch_bounds__(256) void mutual_final_pairs(const PairMutual* __restrict__ tab) {
    const PairMutual m = tab[blockIdx.z];
    mutual_final_body(m.partial, m.nblocks, m.n, m.topk, m.out);
}

StageRings g_pairs_stage;

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

// ---- umlh_align_pairs: one plan for the size query and the launcher ----
// The head (what one upload fills): the three descriptor tables.  Then per member, in member order: its cka_plan region, the two
// topk_plan list slabs of its views, the lists themselves where the caller gave no knn_a / knn_b, the mutual partials.  Every
// region starts on a 256-byte boundary, as in the single plans.  knn_splits: what every view's topk_plan is asked for -- `splits`
// as given, or (0) the topk_splits rule on the strips of all views of the group; topk_plan clamps it to the view's own tiles.
struct PairsPlan {
    int n_cka, n_views, n_mut, knn_splits;
    long long tab_cka, tab_view, tab_mut, head, total;
    CkaPlan cka[UMLH_ALIGN_MAX_PAIRS];
    TopkPlan tk[UMLH_ALIGN_MAX_PAIRS];
    long long cka_at[UMLH_ALIGN_MAX_PAIRS], tk_at[UMLH_ALIGN_MAX_PAIRS][2], list_at[UMLH_ALIGN_MAX_PAIRS][2], mut_at[UMLH_ALIGN_MAX_PAIRS];
};

static void pairs_plan(PairsPlan& p, const umlh_align_pair_t* items, int n, int splits) {
    p.n_cka = p.n_mut = 0;
    long long strips = 0;
    for (int i = 0; i < n; ++i) {
        p.n_cka += items[i].cka != 0;
        if (items[i].topk > 0) { ++p.n_mut; strips += 2 * ((items[i].n + TK_ROWS - 1) / TK_ROWS); }
    }
    p.n_views = 2 * p.n_mut;
    p.knn_splits = topk_splits_for_strips(strips, splits);
    ScratchLayout lay;
    p.tab_cka = lay.take((long long)p.n_cka * (long long)sizeof(PairCka));
    p.tab_view = lay.take((long long)p.n_views * (long long)sizeof(PairView));
    p.tab_mut = lay.take((long long)p.n_mut * (long long)sizeof(PairMutual));
    p.head = lay.end;
    for (int i = 0; i < n; ++i) {
        const umlh_align_pair_t& it = items[i];
        if (it.cka) {
            p.cka[i] = cka_plan(it.n, it.d_a, it.d_b, splits);
            p.cka_at[i] = lay.take(p.cka[i].total);
        }
        if (it.topk > 0) {
            p.tk[i] = topk_plan(it.n, it.n, it.topk, 0, p.knn_splits, 0);
            const int32_t* given[2] = {it.knn_a, it.knn_b};
            for (int v = 0; v < 2; ++v) {
                p.tk_at[i][v] = lay.take(p.tk[i].cand);
                p.list_at[i][v] = given[v] ? -1 : lay.take(it.n * it.topk * 4);
            }
            p.mut_at[i] = lay.take((long long)umlh_align_mutual_bytes(it.n));
        }
    }
    p.total = lay.end;
}

unsigned long long umlh_align_pairs_bytes(const umlh_align_pair_t* items, int n, int splits) {
    PairsPlan p;
    pairs_plan(p, items, n, splits);
    return (unsigned long long)p.total;
}

// One upload of the tables, then at most ten launches whatever n is; a stage no member needs is not launched.
int umlh_align_launch_pairs(const umlh_align_pair_t* items, int n, int splits, void* scratch, hipStream_t st) {
    PairsPlan p;
    pairs_plan(p, items, n, splits);
    PairCka hc[UMLH_ALIGN_MAX_PAIRS];
    PairView hv[2][2 * UMLH_ALIGN_MAX_PAIRS];      // [0]: the views that take the vector load form, [1]: the others
    PairMutual hm[UMLH_ALIGN_MAX_PAIRS];
    int nc = 0, nv[2] = {0, 0}, nm = 0;
    unsigned cs_x = 1, cs_y = 1, cr_x = 1, cr_y = 1, tl_x[2] = {1, 1}, tl_y[2] = {1, 1}, mg_x = 1, mc_x = 1;
    for (int i = 0; i < n; ++i) {
        const umlh_align_pair_t& it = items[i];
        if (it.cka) {
            const CkaPlan& c = p.cka[i];
            PairCka& d = hc[nc++];
            d.g.a = it.a; d.g.b = it.b; d.g.lda = it.lda; d.g.ldb = it.ldb; d.g.da = it.d_a; d.g.db = it.d_b; d.g.ta = c.ta; d.g.tb = c.tb;
            d.g.n = (int)it.n; d.g.sum_chunks = c.sum_chunks; d.g.rchunks = c.rchunks;
            d.g.colsum = at<double>(scratch, p.cka_at[i] + c.colsum);
            d.g.cross = at<double>(scratch, p.cka_at[i] + c.cross);
            d.g.tile_sq = at<double>(scratch, p.cka_at[i] + c.tile_sq);
            d.tiles = c.tiles;
            d.out = it.out5;
            cs_x = std::max(cs_x, (unsigned)((it.d_a + it.d_b + 63) / 64)), cs_y = std::max(cs_y, (unsigned)c.sum_chunks);
            cr_x = std::max(cr_x, (unsigned)c.tiles), cr_y = std::max(cr_y, (unsigned)c.rchunks);
        }
        if (it.topk > 0) {
            const TopkPlan& t = p.tk[i];
            const float* x[2] = {it.a, it.b};
            const int ld[2] = {it.lda, it.ldb}, dd[2] = {it.d_a, it.d_b};
            int32_t* knn[2] = {it.knn_a, it.knn_b};
            float* sc[2] = {it.scores_a, it.scores_b};
            for (int v = 0; v < 2; ++v) {
                if (!knn[v]) knn[v] = at<int32_t>(scratch, p.list_at[i][v]);
                const int f = topk_vec_ok(dd[v], ld[v], ld[v], x[v], x[v]) ? 0 : 1;
                PairView& d = hv[f][nv[f]++];
                d.x = x[v]; d.n = (int)it.n; d.d = dd[v]; d.ldx = ld[v]; d.topk = it.topk; d.ntiles = t.ntiles; d.splits = t.splits;
                d.part_s = at<float>(scratch, p.tk_at[i][v] + t.part_s);
                d.part_i = at<int>(scratch, p.tk_at[i][v] + t.part_i);
                d.knn = knn[v];
                d.scores = sc[v];
                tl_x[f] = std::max(tl_x[f], (unsigned)((it.n + TK_ROWS - 1) / TK_ROWS)), tl_y[f] = std::max(tl_y[f], (unsigned)t.splits);
            }
            PairMutual& m = hm[nm++];
            m.ka = knn[0]; m.kb = knn[1]; m.n = (int)it.n; m.topk = it.topk; m.nblocks = (int)((it.n + 255) / 256);
            m.partial = at<long long>(scratch, p.mut_at[i]);
            m.out = it.out5 + 4;
            mg_x = std::max(mg_x, (unsigned)((it.n + 63) / 64)), mc_x = std::max(mc_x, (unsigned)m.nblocks);
        }
    }
    const int e = g_pairs_stage.upload(scratch, (size_t)p.head, st, [&](unsigned char* h) {
        memcpy(h + p.tab_cka, hc, (size_t)nc * sizeof(PairCka));
        memcpy(h + p.tab_view, hv[0], (size_t)nv[0] * sizeof(PairView));
        memcpy(h + p.tab_view + (size_t)nv[0] * sizeof(PairView), hv[1], (size_t)nv[1] * sizeof(PairView));
        memcpy(h + p.tab_mut, hm, (size_t)nm * sizeof(PairMutual));
    });
    if (e) return e;
    const PairCka* tc = at<PairCka>(scratch, p.tab_cka);
    const PairView* tv = at<PairView>(scratch, p.tab_view);
    const PairMutual* tm = at<PairMutual>(scratch, p.tab_mut);
    if (nc) {
        hipLaunchKernelGGL(cka_colsum_pairs, dim3(cs_x, cs_y, (unsigned)nc), dim3(256), 0, st, tc);
        hipLaunchKernelGGL(cka_cross_pairs, dim3(cr_x, cr_y, (unsigned)nc), dim3(256), 0, st, tc);
        hipLaunchKernelGGL(cka_tile_sq_pairs, dim3(cr_x, 1, (unsigned)nc), dim3(256), 0, st, tc);
        hipLaunchKernelGGL(cka_final_pairs, dim3(1, 1, (unsigned)nc), dim3(256), 0, st, tc);
    }
    if (nm) {
        if (nv[0]) hipLaunchKernelGGL(knn_tiles_pairs<true>, dim3(tl_x[0], tl_y[0], (unsigned)nv[0]), dim3(256), 0, st, tv);
        if (nv[1]) hipLaunchKernelGGL(knn_tiles_pairs<false>, dim3(tl_x[1], tl_y[1], (unsigned)nv[1]), dim3(256), 0, st, tv + nv[0]);
        hipLaunchKernelGGL(knn_merge_pairs, dim3(mg_x, 1, (unsigned)(nv[0] + nv[1])), dim3(64), 0, st, tv);
        hipLaunchKernelGGL(mutual_count_pairs, dim3(mc_x, 1, (unsigned)nm), dim3(256), 0, st, tm);
        hipLaunchKernelGGL(mutual_final_pairs, dim3(1, 1, (unsigned)nm), dim3(256), 0, st, tm);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
