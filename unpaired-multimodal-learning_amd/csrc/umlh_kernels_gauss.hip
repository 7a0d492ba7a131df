// The Gaussian toy's SharedAutoencoder (reference: Gaussian_experiment/model.py:5-59, main.py:33-91) for gfx950: the forward of
// either or both views, and one whole training step (both views, forward, MSE, backward, optimizer update) as two launches.
//
// Per view v in {x, y}, row r of that view:
//     a0 = table_v[idx_v[r]]      a1 = W_in_v a0 + b      a2 = relu(W_e0 a1 + b)   a3 = W_e2 a2 + b   (a3: the embedding)
//     a4 = relu(W_d0 a3 + b)      a5 = W_d2 a4 + b        rec = W_out_v a5 + b     loss_v = mean over rows_v * D of (rec - a0)^2
//
// ae_rows (launch A).  One workgroup of 512 threads per (view, 16-row tile); it reads nothing another workgroup writes.  The rows
//   are gathered into LDS, the six products run forward with the activation of the moment in one of two LDS buffers, the residual
//   is formed against the table's own values, and (training, a view with a backward) the five dA products run backward:
//       dz6 = scale_v (rec - a0)   dz5 = W_out^T dz6   dz4 = (W_d2^T dz5) [a4 > 0]   dz3 = W_d0^T dz4   dz2 = (W_e2^T dz3) [a2 > 0]
//       dz1 = W_e0^T dz2                                         scale_v = (float)(alpha_v * 2 / (rows_v * D)), formed on the host
//   a0 .. a5 and dz1 .. dz6 of the tile's rows go to scratch as they are produced (dense row-major [rows_v][width]), where launch B
//   reads them; the relu masks are read back from there by the workgroup that wrote them, behind a workgroup barrier.
//   products      the form of rollout_rows (umlh_kernels_rollout.hip): v_mfma_f32_16x16x4_f32, A operand = 16 output columns x 4 k
//                 of the weight matrix (for a backward product the transposed element W[k][column]), B operand = 4 k x the 16 rows.
//                 A wave owns the output tiles wave, wave + 8, ... and walks K in blocks of 16: MFMA i of a block takes
//                 k = k0 + i, k0 + 4 + i, k0 + 8 + i, k0 + 12 + i, blocks ascending: one fp32 fma chain per output in an order that
//                 depends on K alone.  The bias is one fp32 add behind the chain; relu is fmaxf(v, 0); its backward keeps dA where
//                 the saved activation is > 0.  An activation [K][16] sits in LDS as [K / 4][16][4], zeros past the width.
//   loss          every thread adds the fp64 squares of the fp32 residuals it holds (tiles ascending, four columns each), the 512
//                 sums meet in a halving tree: one fp64 partial per tile.
// ae_update (launch B).  One workgroup of 256 threads per (weight tensor, 16 x 16 output tile), plus one that finishes the losses.
//   dW[n][k] = sum_r dz[r][n] a[r][k] over the rows of the views that feed the tensor, x rows then y rows: wave w takes the 4-row
//   blocks w, w + 4, ... of a view (one MFMA per block, rows past the view's end as zeros), the four waves' sums are added in wave
//   order.  db[n] (the tiles with column-tile index 0): lane (n, g) of wave w adds dz[4 blk + g][n] over the same blocks, the 16
//   partial sums are added in the order 4 w + g.  The thread that owns an element applies opt_update (umlh_common.h) to W, m and v
//   in place: every element has exactly one owner, nothing is split over K and nothing is reduced afterwards.  The last workgroup
//   adds the tiles' loss partials (thread t: a contiguous run in tile order, then a halving tree), divides by rows_v * D in fp64,
//   rounds once, and forms loss = alpha_x loss_x + alpha_y loss_y as two fp32 products and one add (no contraction).
// No float atomics, no workgroup waits on another; grids and summation orders are functions of the shapes alone: results are bitwise
// reproducible across calls, streams and CU counts.  A row's activations depend on the parameters and the row alone.
//
// ae_rows and ae_update are the instantiations ae_rows_k<false> and ae_update_k<false> of the kernel templates below.
// Grouped forms: ae_rows_grouped = ae_rows_k<true>, ae_update_grouped = ae_update_k<true> and ae_loss_grouped
//   run several independent runs (members) in one launch each.  A workgroup finds its member from blockIdx.x and a prefix array of
//   first workgroups, copies the member's descriptor from a device table that stays constant for the whole call, and then runs the
//   very statements the single-run instantiation runs: per member the results are bit for bit those of the single-run launches.
//   Members share nothing that is written: each has its own scratch region (ae_group_plan).  No atomics, no waits.
#include "umlh_common.h"
#include "umlh_launch.h"
#include "umlh_stage.h"
#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int AE_ROWS = 16;               // rows of one launch-A workgroup (the N of the MFMA)
constexpr int AE_THREADS = 512;
constexpr int AE_WAVES = AE_THREADS / 64;
constexpr int AE_PB = 4;                  // k blocks whose weight loads go out before the first MFMA of the batch
constexpr int AE_UPD_THREADS = 256;
constexpr int AE_UPD_WAVES = AE_UPD_THREADS / 64;
constexpr int AE_UPD_PB = 8;              // row blocks whose loads go out before the first MFMA of the batch
constexpr int AE_N_ACT = 6;               // a0 .. a5, and dz1 .. dz6

struct AeView {
    const float* table;          // [*, ld] fp32
    const int* idx;              // [rows] row ids into table (NULL: rows 0 .. rows - 1)
    long long ld;
    int rows;
    const float* w_in; const float* b_in; const float* w_out; const float* b_out;
    float* act[AE_N_ACT];        // a0 .. a5 in scratch (NULL: not kept)
    float* dz[AE_N_ACT];         // dz1 .. dz6 in scratch
    float* rec;                  // optional [rows][D]
    float* emb;                  // optional [rows][L]
    double* partial;             // [tiles] fp64 sums of squared residuals (NULL: no loss, and no decoder unless rec is asked for)
    float scale;                 // alpha_v * 2 / (rows_v * D)
    int backward;
};

struct AeRowArgs {
    AeView v[2];
    const float* we0; const float* be0; const float* we2; const float* be2;
    const float* wd0; const float* bd0; const float* wd2; const float* bd2;
    int D, C, L;
    int tiles_x;                 // workgroups [0, tiles_x) are the x view's
};

struct AeLoss {
    const double* partial[2];
    int tiles[2];
    int rows[2];
    int D;
    float alpha[2];
    int mode_xy;                 // 0: loss = loss_x
    float* out;                  // [n_out]: loss_x, loss_y (, loss)
    int n_out;
};

struct AeTensor {
    float* w; float* mw; float* vw;       // [N][K]
    float* b; float* mb; float* vb;       // [N]
    const float* dz[2];                   // [rows_v][N] per feeding view (rows 0: the view does not feed it)
    const float* a[2];                    // [rows_v][K]
    int rows[2];
    int N, K;
    int blk0, kt;                         // first workgroup, column tiles
};

struct AeUpdArgs {
    AeTensor t[8];
    int count, tiles;
    OptArgs o;
    AeLoss loss;
};

__host__ __device__ __forceinline__ int ae_pad16(int v) { return (v + 15) & ~15; }
__device__ __forceinline__ int ae_at(int c, int r) { return ((c >> 2) * AE_ROWS + r) * 4 + (c & 3); }

// element (output column c, reduction index k) of a product's weight operand: W[c][k], or W[k][c] of a backward product
template <bool TR>
__device__ __forceinline__ f32x4 ae_load_w(const float* __restrict__ W, int N, int K, int col, int k, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (TR) {
        if (k + 0 < K) v.x = W[(size_t)(k + 0) * N + col];
        if (k + 1 < K) v.y = W[(size_t)(k + 1) * N + col];
        if (k + 2 < K) v.z = W[(size_t)(k + 2) * N + col];
        if (k + 3 < K) v.w = W[(size_t)(k + 3) * N + col];
    } else {
        const float* p = W + (size_t)col * K + k;
        if (vec) {                                                  // K % 4 == 0 and a 16-byte aligned base: all four or none
            if (k < K) v = *reinterpret_cast<const f32x4*>(p);
        } else {
            if (k + 0 < K) v.x = p[0];
            if (k + 1 < K) v.y = p[1];
            if (k + 2 < K) v.z = p[2];
            if (k + 3 < K) v.w = p[3];
        }
    }
    return v;
}

// dst[N][16] = epi(column, W . act, row): all waves, any N and K.  epi returns what the next product reads; columns >= N of the
// last tile are written as zeros.  Ends with a workgroup barrier.
template <bool TR, class Epi>
__device__ __forceinline__ void ae_linear(const float* __restrict__ W, int N, int K, const float* act, float* dst, Epi epi) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
    const int nt = (N + 15) >> 4, nkb = (K + 15) >> 4;
    const bool vec = !TR && (K & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    for (int t = wave; t < nt; t += AE_WAVES) {
        int col = t * 16 + m;
        if (col > N - 1) col = N - 1;                                   // a column past N: its result is dropped
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < nkb; kb += AE_PB) {
            f32x4 a[AE_PB];
#pragma unroll
            for (int j = 0; j < AE_PB; ++j) a[j] = ae_load_w<TR>(W, N, K, col, kb + j < nkb ? (kb + j) * 16 + 4 * g : K, vec);
#pragma unroll
            for (int j = 0; j < AE_PB; ++j) {
                if (kb + j < nkb) {                                      // wave-uniform
                    const f32x4 b = *reinterpret_cast<const f32x4*>(act + (((kb + j) * 4 + g) * AE_ROWS + m) * 4);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].x, b.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].y, b.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].z, b.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].w, b.w, acc, 0, 0, 0);
                }
            }
        }
        // the accumulators are read right behind the last MFMA of the chain (the note in umlh_kernels_micro.hip)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 7" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        const int c = t * 16 + 4 * g;                                   // the lane holds columns c .. c + 3 of row m
        f32x4 v;
        v.x = c + 0 < N ? epi(c + 0, acc.x, m) : 0.f;
        v.y = c + 1 < N ? epi(c + 1, acc.y, m) : 0.f;
        v.z = c + 2 < N ? epi(c + 2, acc.z, m) : 0.f;
        v.w = c + 3 < N ? epi(c + 3, acc.w, m) : 0.f;
        *reinterpret_cast<f32x4*>(dst + ((t * 4 + g) * AE_ROWS + m) * 4) = v;
    }
    __syncthreads();
}

// The member of workgroup wg of a grouped launch: the largest m with first[m] <= wg.  first[i] = the first workgroup of member i
// (strictly ascending: every member has a workgroup; first[0] = 0), first[n] = the grid, INT_MAX from there to entry
// UMLH_AE_MAX_GROUP.  A uniform binary search: six dependent scalar loads within one 256-byte block.
__device__ __forceinline__ int ae_member(const int* __restrict__ first, int wg) {
    static_assert(UMLH_AE_MAX_GROUP == 64, "the search below walks 64 entries");
    int m = 0;
#pragma unroll
    for (int step = UMLH_AE_MAX_GROUP / 2; step >= 1; step >>= 1)
        if (wg >= first[m + step]) m += step;
    return m;
}

// Launch A, the one statement of every product of the rows path, in two instantiations.
//   GROUPED = false (ae_rows): a is the run's descriptor, workgroup blockIdx.x is one of its (view, 16-row tile) pairs; tab, first,
//     n_members and step are not read.
//   GROUPED = true (ae_rows_grouped): a arrives unset.  The workgroup finds its member m in first, copies from tab[m] (a device
//     table that stays as it is for the whole call) the fields the body reads into a, its own view as view 0 of a one-view run,
//     and forms what depends on the step from step.  From there on it is the same code on the same values.  The copy into locals
//     matters: a descriptor read through a pointer would be loaded again behind every memory clobber of ae_linear.
// The body is kept in the kernel and not in a __device__ function taking the descriptor by reference: across such a boundary the
// compiler reads both views' fields up front (69 -> 106 SGPRs and 72 spilled in ae_rows; profiles/gaussian_group_resources.txt).
template <bool GROUPED>
__global__ __launch_bounds__(AE_THREADS) void ae_rows_k(AeRowArgs a, const AeRowArgs* __restrict__ tab, const int* __restrict__ first,
                                                        int n_members, int step) {
    extern __shared__ __attribute__((aligned(16))) float ae_lds[];
    int wg = (int)blockIdx.x;
    if constexpr (GROUPED) {
        const int m = ae_member(first, wg);
        const AeRowArgs& g = tab[m];
        const int local = wg - first[m], tx = g.tiles_x, gv = local >= tx ? 1 : 0;
        a.v[0] = g.v[gv];
        if (a.v[0].idx) a.v[0].idx += (size_t)step * (size_t)a.v[0].rows;   // the step takes idx[step * batch ..)
        a.tiles_x = INT_MAX;                                            // every workgroup is view 0's
        a.we0 = g.we0; a.be0 = g.be0; a.we2 = g.we2; a.be2 = g.be2;
        a.wd0 = g.wd0; a.bd0 = g.bd0; a.wd2 = g.wd2; a.bd2 = g.bd2;
        a.D = g.D; a.C = g.C; a.L = g.L;
        wg = local - (gv ? tx : 0);
        __builtin_assume(wg < INT_MAX);                                 // so that the view index below is the constant 0
    }
    const int D = a.D, C = a.C, L = a.L;
    const int vi = wg >= a.tiles_x ? 1 : 0;
    const AeView& V = a.v[vi];
    const int tile = wg - (vi ? a.tiles_x : 0);
    const int row0 = tile * AE_ROWS, n = V.rows, tid = threadIdx.x;
    const int maxw = ae_pad16(D > C ? (D > L ? D : L) : (C > L ? C : L));
    float* X = ae_lds;
    float* Y = X + maxw * AE_ROWS;
    double* red = reinterpret_cast<double*>(Y + maxw * AE_ROWS);

    // a0: the tile's rows of the table, zeros past D and past the view's last row
    for (int i = tid; i < AE_ROWS * D; i += AE_THREADS) {
        const int r = i / D, c = i - r * D, row = row0 + r;
        float v = 0.f;
        if (row < n) {
            const long long rid = V.idx ? (long long)V.idx[row] : (long long)row;
            v = V.table[rid * V.ld + c];
            if (V.act[0]) V.act[0][(size_t)row * D + c] = v;
        }
        X[ae_at(c, r)] = v;
    }
    for (int i = tid; i < (ae_pad16(D) - D) * AE_ROWS; i += AE_THREADS) X[ae_at(D + (i >> 4), i & 15)] = 0.f;
    __syncthreads();

    // what a forward product leaves in scratch: act j [rows][w]
    auto keep = [&](float* base, int w, int c, int r, float v) {
        if (base && row0 + r < n) base[(size_t)(row0 + r) * w + c] = v;
    };
    {
        const float* b = V.b_in;
        float* o = V.act[1];
        ae_linear<false>(V.w_in, C, D, X, Y, [&](int c, float v, int r) { v += b[c]; keep(o, C, c, r, v); return v; });
    }
    {
        const float* b = a.be0;
        float* o = V.act[2];
        ae_linear<false>(a.we0, L, C, Y, X, [&](int c, float v, int r) { v = fmaxf(v + b[c], 0.f); keep(o, L, c, r, v); return v; });
    }
    {
        const float* b = a.be2;
        float* o = V.act[3];
        float* e = V.emb;
        ae_linear<false>(a.we2, L, L, X, Y, [&](int c, float v, int r) { v += b[c]; keep(o, L, c, r, v); keep(e, L, c, r, v); return v; });
    }
    if (!V.partial && !V.rec) return;                                   // the embedding alone was asked for (uniform)
    {
        const float* b = a.bd0;
        float* o = V.act[4];
        ae_linear<false>(a.wd0, L, L, Y, X, [&](int c, float v, int r) { v = fmaxf(v + b[c], 0.f); keep(o, L, c, r, v); return v; });
    }
    {
        const float* b = a.bd2;
        float* o = V.act[5];
        ae_linear<false>(a.wd2, C, L, X, Y, [&](int c, float v, int r) { v += b[c]; keep(o, C, c, r, v); return v; });
    }
    double lsum = 0.0;
    {
        const float* b = V.b_out;
        float* rec = V.rec;
        float* o = V.dz[5];
        const float scale = V.scale;
        ae_linear<false>(V.w_out, D, C, Y, X, [&](int c, float v, int r) {
            v += b[c];
            float dz = 0.f;
            if (row0 + r < n) {
                const long long rid = V.idx ? (long long)V.idx[row0 + r] : (long long)(row0 + r);
                const float res = v - V.table[rid * V.ld + c];
                lsum += (double)res * (double)res;
                dz = scale * res;
                if (rec) rec[(size_t)(row0 + r) * D + c] = v;
                if (o) o[(size_t)(row0 + r) * D + c] = dz;
            }
            return dz;
        });
    }
    if (V.partial) {
        const double s = block_reduce<AE_THREADS>(lsum, red, OpSum());
        if (tid == 0) V.partial[tile] = s;
    }
    if (!V.backward) return;
    // backward: X holds dz6
    {
        float* o = V.dz[4];
        ae_linear<true>(V.w_out, C, D, X, Y, [&](int c, float v, int r) { keep(o, C, c, r, v); return v; });          // dz5
    }
    {
        float* o = V.dz[3];
        const float* gate = V.act[4];
        ae_linear<true>(a.wd2, L, C, Y, X, [&](int c, float v, int r) {                                              // dz4
            v = (row0 + r < n && gate[(size_t)(row0 + r) * L + c] > 0.f) ? v : 0.f;
            keep(o, L, c, r, v);
            return v;
        });
    }
    {
        float* o = V.dz[2];
        ae_linear<true>(a.wd0, L, L, X, Y, [&](int c, float v, int r) { keep(o, L, c, r, v); return v; });           // dz3
    }
    {
        float* o = V.dz[1];
        const float* gate = V.act[2];
        ae_linear<true>(a.we2, L, L, Y, X, [&](int c, float v, int r) {                                              // dz2
            v = (row0 + r < n && gate[(size_t)(row0 + r) * L + c] > 0.f) ? v : 0.f;
            keep(o, L, c, r, v);
            return v;
        });
    }
    {
        float* o = V.dz[0];
        ae_linear<true>(a.we0, C, L, X, Y, [&](int c, float v, int r) { keep(o, C, c, r, v); return v; });           // dz1
    }
}

// the step's losses from the tiles' partials; 256 threads, red[256]
__device__ __forceinline__ void ae_loss_body(const AeLoss& l, double* red) {
    const int tid = threadIdx.x;
    float lv[2] = {0.f, 0.f};
    for (int v = 0; v < 2; ++v) {
        if (l.rows[v] == 0 || l.partial[v] == nullptr) continue;                       // uniform
        const int per = (l.tiles[v] + AE_UPD_THREADS - 1) / AE_UPD_THREADS;
        const int lo = tid * per, hi = lo + per < l.tiles[v] ? lo + per : l.tiles[v];
        double s = 0.0;
        for (int i = lo; i < hi; ++i) s += l.partial[v][i];
        s = block_reduce<AE_UPD_THREADS>(s, red, OpSum());
        lv[v] = (float)(s / ((double)l.rows[v] * (double)l.D));
    }
    if (tid == 0) {
        l.out[0] = lv[0];
        l.out[1] = lv[1];
        if (l.n_out > 2) l.out[2] = l.mode_xy ? __fadd_rn(__fmul_rn(l.alpha[0], lv[0]), __fmul_rn(l.alpha[1], lv[1])) : lv[0];
    }
}

__global__ __launch_bounds__(AE_UPD_THREADS) void ae_loss(const AeLoss l) {
    __shared__ double red[AE_UPD_THREADS];
    ae_loss_body(l, red);
}

// Launch B, the one statement of the update path, in two instantiations (as ae_rows_k).
//   GROUPED = false (ae_update): a is the run's descriptor; workgroup blockIdx.x is one of its weight tiles or its loss workgroup.
//   GROUPED = true (ae_update_grouped): a arrives unset.  Member m's workgroups are its weight tiles and then its loss workgroup;
//     the workgroup copies its own tensor from tab[m] into a as the only tensor, the member's optimizer constants of the step from
//     opt ([n_steps][n_members], formed on the host), and the loss descriptor with out moved to the step's three floats.
template <bool GROUPED>
__global__ __launch_bounds__(AE_UPD_THREADS) void ae_update_k(AeUpdArgs a, const AeUpdArgs* __restrict__ tab, const int* __restrict__ first,
                                                              const OptArgs* __restrict__ opt, int n_members, int step) {
    __shared__ double red[AE_UPD_THREADS];
    __shared__ float part[AE_UPD_WAVES][256];
    __shared__ float bpart[16][16];
    int b = blockIdx.x;
    if constexpr (GROUPED) {
        const int m = ae_member(first, b);
        const AeUpdArgs& g = tab[m];
        b -= first[m];
        int gi = 0;
        for (int i = 1; i < g.count; ++i)
            if (b >= g.t[i].blk0) gi = i;
        a.t[0] = g.t[gi];                                               // unused by the loss workgroup
        a.count = 1;
        a.tiles = g.tiles;
        a.o = opt[(size_t)step * (size_t)n_members + m];
        a.loss = g.loss;
        a.loss.out += (size_t)3 * (size_t)step;
    }
    const int tid = threadIdx.x;
    if (b >= a.tiles) {
        ae_loss_body(a.loss, red);
        return;
    }
    int ti = 0;
    for (int i = 1; i < a.count; ++i)
        if (b >= a.t[i].blk0) ti = i;
    const AeTensor& T = a.t[ti];
    const int tile = b - T.blk0, n0 = (tile / T.kt) * 16, k0 = (tile % T.kt) * 16, N = T.N, K = T.K;
    const int wave = tid >> 6, lane = tid & 63, m = lane & 15, g = lane >> 4;
    const bool n_ok = n0 + m < N, k_ok = k0 + m < K;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float bs = 0.f;
    for (int v = 0; v < 2; ++v) {
        const int rows = T.rows[v];
        if (rows == 0) continue;                                         // uniform
        const float* __restrict__ dz = T.dz[v] + n0 + m;
        const float* __restrict__ av = T.a[v] + k0 + m;
        const int nblk = (rows + 3) >> 2;
        for (int blk = wave; blk < nblk; blk += AE_UPD_WAVES * AE_UPD_PB) {
            float x[AE_UPD_PB], y[AE_UPD_PB];
#pragma unroll
            for (int j = 0; j < AE_UPD_PB; ++j) {
                const int r = (blk + j * AE_UPD_WAVES) * 4 + g;              // r >= rows also covers blocks past nblk
                x[j] = (r < rows && n_ok) ? dz[(size_t)r * N] : 0.f;
                y[j] = (r < rows && k_ok) ? av[(size_t)r * K] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < AE_UPD_PB; ++j) {
                if (blk + j * AE_UPD_WAVES < nblk) {                         // wave-uniform
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j], y[j], acc, 0, 0, 0);
                    bs += x[j];
                }
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 7" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // the lane holds dW[n0 + 4 g + i][k0 + m], i = 0 .. 3
    part[wave][(4 * g + 0) * 16 + m] = acc.x;
    part[wave][(4 * g + 1) * 16 + m] = acc.y;
    part[wave][(4 * g + 2) * 16 + m] = acc.z;
    part[wave][(4 * g + 3) * 16 + m] = acc.w;
    bpart[wave * 4 + g][m] = bs;
    __syncthreads();
    const bool adam = a.o.kind != UMLH_OPT_SGD;
    {
        const int nn = n0 + (tid >> 4), kk = k0 + (tid & 15);
        if (nn < N && kk < K) {
            const float gr = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
            const size_t i = (size_t)nn * K + kk;
            float p = T.w[i], mm = T.mw[i], vv = adam ? T.vw[i] : 0.f;
            opt_update(a.o, gr, p, mm, vv);
            T.w[i] = p;
            T.mw[i] = mm;
            if (adam) T.vw[i] = vv;
        }
    }
    if (k0 == 0 && tid < 16 && n0 + tid < N) {
        float gr = bpart[0][tid];
        for (int j = 1; j < 16; ++j) gr += bpart[j][tid];
        const int i = n0 + tid;
        float p = T.b[i], mm = T.mb[i], vv = adam ? T.vb[i] : 0.f;
        opt_update(a.o, gr, p, mm, vv);
        T.b[i] = p;
        T.mb[i] = mm;
        if (adam) T.vb[i] = vv;
    }
}

// the losses of a grouped evaluation forward: one workgroup per member (none asked for: nothing to do)
__global__ __launch_bounds__(AE_UPD_THREADS) void ae_loss_grouped(const AeLoss* __restrict__ tab) {
    __shared__ double red[AE_UPD_THREADS];
    const AeLoss l = tab[blockIdx.x];
    if (l.out == nullptr) return;                                        // uniform
    ae_loss_body(l, red);
}

inline size_t ae_lds_bytes(int D, int C, int L) {
    const size_t maxw = (size_t)ae_pad16(std::max(D, std::max(C, L)));
    return 2 * maxw * AE_ROWS * sizeof(float) + AE_THREADS * sizeof(double);
}

// The one scratch plan of both entry points: per view the tiles' fp64 loss partials, and for a training step a0 .. a5 and
// dz1 .. dz6 of every row.  Offsets in bytes, every region on a 256-byte boundary.
struct AePlan {
    long long partial[2];
    long long act[2][AE_N_ACT];
    long long dz[2][AE_N_ACT];
    long long bytes;
};

inline AePlan ae_plan(int D, int C, int L, int rows_x, int rows_y, int train) {
    AePlan p;
    ScratchLayout lay;
    const int rows[2] = {rows_x, rows_y};
    const int aw[AE_N_ACT] = {D, C, L, L, L, C}, zw[AE_N_ACT] = {C, L, L, L, C, D};
    for (int v = 0; v < 2; ++v) {
        p.partial[v] = lay.take((long long)((rows[v] + AE_ROWS - 1) / AE_ROWS) * 8);
        for (int j = 0; j < AE_N_ACT; ++j) {
            p.act[v][j] = train ? lay.take((long long)rows[v] * aw[j] * 4) : -1;
            p.dz[v][j] = train ? lay.take((long long)rows[v] * zw[j] * 4) : -1;
        }
    }
    p.bytes = lay.end > 0 ? lay.end : 256;
    return p;
}

// The scratch plan of a grouped call, built on ae_plan.  In front the tables that one upload per call fills: the members' launch-A
// descriptors, their launch-B descriptors (training) or loss descriptors (evaluation), the two prefix arrays of first workgroups
// and (training) the [n_steps][n] optimizer constants.  Behind them one private ae_plan region per member: no member's workgroups
// read or write another's.  n_steps > 0: a training group; n_steps == 0: an evaluation group.
struct AeGroupPlan {
    long long rows, upd, first_a, first_b, opt;
    long long head;                                   // bytes of the uploaded tables, from offset 0
    long long member[UMLH_AE_MAX_GROUP];
    long long bytes;
};

AeGroupPlan ae_group_plan(int n, int n_steps, const umlh_ae_cfg_t* const* cfg, const int* rows_x, const int* rows_y) {
    AeGroupPlan p = {};
    ScratchLayout lay;
    const int train = n_steps > 0;
    p.rows = lay.take((long long)n * (long long)sizeof(AeRowArgs));
    p.upd = lay.take((long long)n * (long long)(train ? sizeof(AeUpdArgs) : sizeof(AeLoss)));
    p.first_a = lay.take((long long)(UMLH_AE_MAX_GROUP + 1) * (long long)sizeof(int));
    p.first_b = lay.take((long long)(UMLH_AE_MAX_GROUP + 1) * (long long)sizeof(int));
    p.opt = lay.take((long long)n_steps * n * (long long)sizeof(OptArgs));
    p.head = lay.end;
    for (int i = 0; i < n; ++i)
        p.member[i] = lay.take(ae_plan(cfg[i]->dim_obs, cfg[i]->dim_common, cfg[i]->dim_latent, rows_x[i], rows_y[i], train).bytes);
    p.bytes = lay.end;
    return p;
}

void ae_fill_rows(AeRowArgs& r, const umlh_ae_cfg_t* cfg, const float* const* P) {
    r.D = cfg->dim_obs; r.C = cfg->dim_common; r.L = cfg->dim_latent;
    r.v[0].w_in = P[0]; r.v[0].b_in = P[1]; r.v[1].w_in = P[2]; r.v[1].b_in = P[3];
    r.we0 = P[4]; r.be0 = P[5]; r.we2 = P[6]; r.be2 = P[7]; r.wd0 = P[8]; r.bd0 = P[9]; r.wd2 = P[10]; r.bd2 = P[11];
    r.v[0].w_out = P[12]; r.v[0].b_out = P[13]; r.v[1].w_out = P[14]; r.v[1].b_out = P[15];
}

// The descriptors of one evaluation forward on its scratch region: launch A's (r) and the loss launch's (l; l.out NULL: no losses).
void ae_build_forward(AeRowArgs& r, AeLoss& l, const umlh_ae_cfg_t* cfg, const float* const* P, const float* x, long long ldx,
                      const int* idx_x, int n_x, const float* y, long long ldy, const int* idx_y, int n_y, float* losses, float* rec_x,
                      float* rec_y, float* emb_x, float* emb_y, void* scratch) {
    const AePlan p = ae_plan(cfg->dim_obs, cfg->dim_common, cfg->dim_latent, n_x, n_y, 0);
    ae_fill_rows(r, cfg, P);
    const float* tab[2] = {x, y};
    const long long ld[2] = {ldx, ldy};
    const int* idx[2] = {idx_x, idx_y};
    const int rows[2] = {n_x, n_y};
    float* rec[2] = {rec_x, rec_y};
    float* emb[2] = {emb_x, emb_y};
    for (int v = 0; v < 2; ++v) {
        AeView& V = r.v[v];
        V.table = tab[v]; V.idx = idx[v]; V.ld = ld[v]; V.rows = rows[v]; V.rec = rec[v]; V.emb = emb[v];
        V.partial = losses ? at<double>(scratch, p.partial[v]) : nullptr;
        V.scale = 0.f; V.backward = 0;
        l.partial[v] = V.partial; l.tiles[v] = (rows[v] + AE_ROWS - 1) / AE_ROWS; l.rows[v] = rows[v];
    }
    r.tiles_x = l.tiles[0];
    l.D = cfg->dim_obs; l.out = losses; l.n_out = 2;
}

// The descriptors of one training step of one run on its scratch region: launch A's (r) and launch B's (u, all but the optimizer
// constants u.o).  idx_x / idx_y and losses are the step's own.
void ae_build_step(AeRowArgs& r, AeUpdArgs& u, const umlh_ae_cfg_t* cfg, float* const* P, float* const* M, float* const* V, const float* x,
                   long long ldx, const int* idx_x, int batch_x, const float* y, long long ldy, const int* idx_y, int batch_y,
                   int backward_y, float alpha_x, float alpha_y, float* losses, void* scratch) {
    const int D = cfg->dim_obs, C = cfg->dim_common, L = cfg->dim_latent;
    const AePlan p = ae_plan(D, C, L, batch_x, batch_y, 1);
    ae_fill_rows(r, cfg, P);
    const float* tab[2] = {x, y};
    const long long ld[2] = {ldx, ldy};
    const int* idx[2] = {idx_x, idx_y};
    const int rows[2] = {batch_x, batch_y};
    const float alpha[2] = {alpha_x, alpha_y};
    const int back[2] = {batch_x > 0, batch_y > 0 && backward_y};
    for (int v = 0; v < 2; ++v) {
        AeView& W = r.v[v];
        W.table = tab[v]; W.idx = idx[v]; W.ld = ld[v]; W.rows = rows[v]; W.rec = nullptr; W.emb = nullptr;
        W.partial = at<double>(scratch, p.partial[v]);
        W.backward = back[v];
        W.scale = rows[v] > 0 ? (float)((double)alpha[v] * 2.0 / ((double)rows[v] * (double)D)) : 0.f;
        for (int j = 0; j < AE_N_ACT; ++j) {
            W.act[j] = back[v] ? at<float>(scratch, p.act[v][j]) : nullptr;
            W.dz[j] = back[v] ? at<float>(scratch, p.dz[v][j]) : nullptr;
        }
        u.loss.partial[v] = W.partial; u.loss.tiles[v] = (rows[v] + AE_ROWS - 1) / AE_ROWS; u.loss.rows[v] = rows[v];
        u.loss.alpha[v] = alpha[v];
    }
    r.tiles_x = u.loss.tiles[0];
    u.loss.D = D; u.loss.mode_xy = backward_y ? 1 : 0; u.loss.out = losses; u.loss.n_out = 3;
    // tensor k of the state_dict order, the dz / a blocks that form its gradient, the views that feed it (-1: both)
    struct Feed { int k, dz, a, N, K, view; };
    const Feed feeds[8] = {{0, 0, 0, C, D, 0}, {2, 0, 0, C, D, 1}, {4, 1, 1, L, C, -1}, {6, 2, 2, L, L, -1},
                           {8, 3, 3, L, L, -1}, {10, 4, 4, C, L, -1}, {12, 5, 5, D, C, 0}, {14, 5, 5, D, C, 1}};
    int blk = 0;
    for (const Feed& f : feeds) {
        if (f.view >= 0 && !back[f.view]) continue;                      // a view without a backward: its heads are not touched
        if (!back[0] && !back[1]) continue;
        AeTensor& T = u.t[u.count++];
        T.w = P[f.k]; T.mw = M[f.k]; T.vw = V ? V[f.k] : nullptr;
        T.b = P[f.k + 1]; T.mb = M[f.k + 1]; T.vb = V ? V[f.k + 1] : nullptr;
        for (int v = 0; v < 2; ++v) {
            const bool on = back[v] && (f.view < 0 || f.view == v);
            T.rows[v] = on ? rows[v] : 0;
            T.dz[v] = on ? r.v[v].dz[f.dz] : nullptr;
            T.a[v] = on ? r.v[v].act[f.a] : nullptr;
        }
        T.N = f.N; T.K = f.K; T.kt = (f.K + 15) / 16; T.blk0 = blk;
        blk += ((f.N + 15) / 16) * T.kt;
    }
    u.tiles = blk;
}

inline int ae_tiles(const AeRowArgs& r) { return r.tiles_x + (r.v[1].rows + AE_ROWS - 1) / AE_ROWS; }

int ae_launch_rows(const AeRowArgs& r, hipStream_t st) {
    if (int e = raise_lds_limit<&ae_rows_k<false>>((int)ae_lds_bytes(UMLH_AE_MAX_OBS, UMLH_AE_MAX_COMMON, UMLH_AE_MAX_LATENT))) return e;
    hipLaunchKernelGGL(ae_rows_k<false>, dim3((unsigned)ae_tiles(r)), dim3(AE_THREADS), ae_lds_bytes(r.D, r.C, r.L), st, r, nullptr, nullptr, 0, 0);
    return (int)hipGetLastError();
}

// Pinned staging of the grouped calls' tables (umlh_stage.h): the source of the asynchronous upload outlives it, and a call waits
// on the host only for a copy that is two calls old.
StageRings g_ae_stage;

// first[i] = first workgroup of member i; first[n] = the grid; INT_MAX from there on
void ae_fill_first(int* first, const int* counts, int n) {
    int at = 0;
    for (int i = 0; i <= UMLH_AE_MAX_GROUP; ++i) {
        first[i] = i <= n ? at : INT_MAX;
        if (i < n) at += counts[i];
    }
}

int ae_launch_rows_grouped(const AeRowArgs* tab, const int* first, int n, int grid, size_t lds, int s, hipStream_t st) {
    if (int e = raise_lds_limit<&ae_rows_k<true>>((int)ae_lds_bytes(UMLH_AE_MAX_OBS, UMLH_AE_MAX_COMMON, UMLH_AE_MAX_LATENT))) return e;
    hipLaunchKernelGGL(ae_rows_k<true>, dim3((unsigned)grid), dim3(AE_THREADS), lds, st, AeRowArgs{}, tab, first, n, s);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" unsigned long long umlh_ae_plan_bytes(const umlh_ae_cfg_t* cfg, int rows_x, int rows_y, int train) {
    return (unsigned long long)ae_plan(cfg->dim_obs, cfg->dim_common, cfg->dim_latent, rows_x, rows_y, train).bytes;
}

extern "C" int umlh_ae_launch_forward(const umlh_ae_cfg_t* cfg, const float* const* P, const float* x, long long ldx, const int* idx_x,
                                      int n_x, const float* y, long long ldy, const int* idx_y, int n_y, float* losses, float* rec_x,
                                      float* rec_y, float* emb_x, float* emb_y, void* scratch, hipStream_t st) {
    AeRowArgs r = {};
    AeLoss l = {};
    ae_build_forward(r, l, cfg, P, x, ldx, idx_x, n_x, y, ldy, idx_y, n_y, losses, rec_x, rec_y, emb_x, emb_y, scratch);
    if (int e = ae_launch_rows(r, st)) return e;
    if (losses) hipLaunchKernelGGL(ae_loss, dim3(1), dim3(AE_UPD_THREADS), 0, st, l);
    return (int)hipGetLastError();
}

// one training step: launch A, launch B.  idx_x / idx_y and losses are the step's own.  part: 0 = the step; 1 = launch A alone,
// 2 = launch B alone on the scratch an earlier whole step left (umlh_ae_bench_steps only: not a training step).
extern "C" int umlh_ae_launch_step(const umlh_ae_cfg_t* cfg, float* const* P, float* const* M, float* const* V, const float* x,
                                   long long ldx, const int* idx_x, int batch_x, const float* y, long long ldy, const int* idx_y,
                                   int batch_y, int backward_y, float alpha_x, float alpha_y, const OptArgs* o, float* losses,
                                   void* scratch, int part, hipStream_t st) {
    AeRowArgs r = {};
    AeUpdArgs u = {};
    ae_build_step(r, u, cfg, P, M, V, x, ldx, idx_x, batch_x, y, ldy, idx_y, batch_y, backward_y, alpha_x, alpha_y, losses, scratch);
    u.o = *o;
    if (part != 2)
        if (int e = ae_launch_rows(r, st)) return e;
    if (part != 1) hipLaunchKernelGGL(ae_update_k<false>, dim3((unsigned)(u.tiles + 1)), dim3(AE_UPD_THREADS), 0, st, u, nullptr, nullptr, nullptr, 0, 0);
    return (int)hipGetLastError();
}

extern "C" unsigned long long umlh_ae_group_plan_bytes(const umlh_ae_group_item_t* items, int n, int n_steps) {
    const umlh_ae_cfg_t* cfg[UMLH_AE_MAX_GROUP];
    int rx[UMLH_AE_MAX_GROUP], ry[UMLH_AE_MAX_GROUP];
    for (int i = 0; i < n; ++i) { cfg[i] = &items[i].cfg; rx[i] = items[i].batch_x; ry[i] = items[i].batch_y; }
    return (unsigned long long)ae_group_plan(n, n_steps, cfg, rx, ry).bytes;
}

extern "C" unsigned long long umlh_ae_eval_group_plan_bytes(const umlh_ae_eval_item_t* items, int n) {
    const umlh_ae_cfg_t* cfg[UMLH_AE_MAX_GROUP];
    int rx[UMLH_AE_MAX_GROUP], ry[UMLH_AE_MAX_GROUP];
    for (int i = 0; i < n; ++i) { cfg[i] = &items[i].cfg; rx[i] = items[i].n_x; ry[i] = items[i].n_y; }
    return (unsigned long long)ae_group_plan(n, 0, cfg, rx, ry).bytes;
}

// n_steps training steps of n runs: one upload of the tables, then launch A and launch B of the whole group per step.  opt: HOST
// [n_steps][n] optimizer constants.  V of a member under sgd has been replaced by NULL by the caller.
extern "C" int umlh_ae_launch_group(const umlh_ae_group_item_t* items, int n, int n_steps, const OptArgs* opt, void* scratch,
                                    hipStream_t st) {
    const umlh_ae_cfg_t* cfg[UMLH_AE_MAX_GROUP];
    int rx[UMLH_AE_MAX_GROUP], ry[UMLH_AE_MAX_GROUP];
    for (int i = 0; i < n; ++i) { cfg[i] = &items[i].cfg; rx[i] = items[i].batch_x; ry[i] = items[i].batch_y; }
    const AeGroupPlan p = ae_group_plan(n, n_steps, cfg, rx, ry);
    int grid_a = 0, grid_b = 0;
    size_t lds = 0;
    const int e = g_ae_stage.upload(scratch, (size_t)p.head, st, [&](unsigned char* h) {
        AeRowArgs* R = at<AeRowArgs>(h, p.rows);
        AeUpdArgs* U = at<AeUpdArgs>(h, p.upd);
        int ca[UMLH_AE_MAX_GROUP], cb[UMLH_AE_MAX_GROUP];
        for (int i = 0; i < n; ++i) {
            const umlh_ae_group_item_t& it = items[i];
            R[i] = AeRowArgs{};
            U[i] = AeUpdArgs{};
            ae_build_step(R[i], U[i], &it.cfg, it.P, it.M, it.optimizer != UMLH_OPT_SGD ? it.V : nullptr, it.x, it.ldx, it.idx_x, it.batch_x,
                          it.y, it.ldy, it.idx_y, it.batch_y, it.backward_y, it.alpha_x, it.alpha_y, it.losses, at<char>(scratch, p.member[i]));
            ca[i] = ae_tiles(R[i]);
            cb[i] = U[i].tiles + 1;
            grid_a += ca[i];
            grid_b += cb[i];
            lds = std::max(lds, ae_lds_bytes(R[i].D, R[i].C, R[i].L));
        }
        ae_fill_first(at<int>(h, p.first_a), ca, n);
        ae_fill_first(at<int>(h, p.first_b), cb, n);
        memcpy(h + p.opt, opt, (size_t)n_steps * n * sizeof(OptArgs));
    });
    if (e) return e;
    for (int s = 0; s < n_steps; ++s) {
        if (int e2 = ae_launch_rows_grouped(at<AeRowArgs>(scratch, p.rows), at<int>(scratch, p.first_a), n, grid_a, lds, s, st)) return e2;
        hipLaunchKernelGGL(ae_update_k<true>, dim3((unsigned)grid_b), dim3(AE_UPD_THREADS), 0, st, AeUpdArgs{}, at<AeUpdArgs>(scratch, p.upd),
                           at<int>(scratch, p.first_b), at<OptArgs>(scratch, p.opt), n, s);
        if (int e2 = (int)hipGetLastError()) return e2;
    }
    return 0;
}

// the evaluation forward of n runs: one upload, launch A of the whole group, one loss workgroup per member
extern "C" int umlh_ae_launch_forward_group(const umlh_ae_eval_item_t* items, int n, void* scratch, hipStream_t st) {
    const umlh_ae_cfg_t* cfg[UMLH_AE_MAX_GROUP];
    int rx[UMLH_AE_MAX_GROUP], ry[UMLH_AE_MAX_GROUP];
    for (int i = 0; i < n; ++i) { cfg[i] = &items[i].cfg; rx[i] = items[i].n_x; ry[i] = items[i].n_y; }
    const AeGroupPlan p = ae_group_plan(n, 0, cfg, rx, ry);
    int grid_a = 0;
    size_t lds = 0;
    bool any_loss = false;
    const int e = g_ae_stage.upload(scratch, (size_t)p.head, st, [&](unsigned char* h) {
        AeRowArgs* R = at<AeRowArgs>(h, p.rows);
        AeLoss* Ls = at<AeLoss>(h, p.upd);
        int ca[UMLH_AE_MAX_GROUP];
        for (int i = 0; i < n; ++i) {
            const umlh_ae_eval_item_t& it = items[i];
            R[i] = AeRowArgs{};
            Ls[i] = AeLoss{};
            ae_build_forward(R[i], Ls[i], &it.cfg, it.P, it.x, it.ldx, it.idx_x, it.n_x, it.y, it.ldy, it.idx_y, it.n_y, it.losses,
                             it.n_x ? it.rec_x : nullptr, it.n_y ? it.rec_y : nullptr, it.n_x ? it.emb_x : nullptr,
                             it.n_y ? it.emb_y : nullptr, at<char>(scratch, p.member[i]));
            ca[i] = ae_tiles(R[i]);
            grid_a += ca[i];
            lds = std::max(lds, ae_lds_bytes(R[i].D, R[i].C, R[i].L));
            any_loss = any_loss || it.losses != nullptr;
        }
        ae_fill_first(at<int>(h, p.first_a), ca, n);
        ae_fill_first(at<int>(h, p.first_b), ca, 0);
    });
    if (e) return e;
    if (int e2 = ae_launch_rows_grouped(at<AeRowArgs>(scratch, p.rows), at<int>(scratch, p.first_a), n, grid_a, lds, 0, st)) return e2;
    if (any_loss) hipLaunchKernelGGL(ae_loss_grouped, dim3((unsigned)n), dim3(AE_UPD_THREADS), 0, st, at<AeLoss>(scratch, p.upd));
    return (int)hipGetLastError();
}

