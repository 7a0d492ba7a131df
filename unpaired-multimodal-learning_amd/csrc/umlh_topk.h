// The streaming top-k neighbour core shared by the alignment k-NN (knn_tiles / knn_merge, umlh_kernels_align.hip), the
// k-NN probe (kp_tiles / kp_merge / kp_refine, umlh_kernels_knn.hip) and the class report (ev_tiles / ev_merge / ev_refine,
// umlh_kernels_evalreport.hip), the 32 x 64 Gram k loop that rbf_tiles (umlh_kernels_align_ext.hip) runs as well, and the
// scratch plan and launch sequence of the three users.  For the .hip files only; the kernels stay where they are launched.
//
// A workgroup takes a strip of 32 query rows and a chunk of 256-column tiles of the train rows, scores every (row, column)
// pair on v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma chain) and keeps, per row, the `width` best columns under the strict
// total order (score desc, index asc): one partial list per chunk, merged pairwise afterwards.  The result is bitwise
// independent of `splits`: chunks start on tile boundaries, every score is the same fma chain wherever it is computed, and
// the kept lists are exact top-`width` under the strict order.  Nothing forms a rows x columns array.
//
// List entries that no column has filled are SENTINELS: negative indices -1 - e at score -inf, compared as unsigned so that
// they sort behind every real index at an equal score (and, among themselves, the larger e first).  A sentinel is never an
// address; a caller that publishes indices says what a negative one becomes.
#pragma once
#include "umlh_common.h"
#include "umlh_launch.h"

constexpr int TK_ROWS = 32;              // query rows of a workgroup's strip
constexpr int TK_COLS = 256;             // train rows (columns) of a tile: 4 waves x 64
constexpr int TK_LD = TK_COLS + 1;       // score tile row stride (floats): the filter's reads are conflict-free
constexpr int TK_KMAX = 32;              // largest list width
constexpr int TK_KLD = TK_KMAX + 1;      // list row stride
constexpr int TK_TARGET_WG = 512;        // auto splits: about two workgroups per CU of the 256
constexpr int TK_MAX_SPLITS = 1024;      // (grid y)

// Column chunks asked of a launch (or of several that share one grid) of `strips` 32-row strips in all: `splits` as asked for,
// or (0 = auto) as many as bring the grid to TK_TARGET_WG workgroups.
inline int topk_splits_for_strips(long long strips, int splits) {
    long long s = splits > 0 ? splits : (strips > 0 ? (TK_TARGET_WG + strips - 1) / strips : 1);
    return (int)(s > TK_MAX_SPLITS ? TK_MAX_SPLITS : (s < 1 ? 1 : s));
}

// Column chunks of a launch over n_query x n_train: `splits` as asked for (0 = auto), at most one per tile.
inline int topk_splits(long long n_query, long long n_train, int splits) {
    const long long ntiles = (n_train + TK_COLS - 1) / TK_COLS, strips = (n_query + TK_ROWS - 1) / TK_ROWS;
    const long long s = topk_splits_for_strips(strips, splits);
    return (int)(s > ntiles ? ntiles : s);
}

// Scratch of a launch: `front_bytes` of the caller's own, the chunks' partial lists (scores, then indices: [splits][nq][kc]
// each) and, for a two-stage user, the merged candidates [nq][kc], kc = min(k + margin, nt).  A user without stage 2 passes
// margin 0 (its k < nt: kc = k) and needs `cand` bytes: its scratch ends where the candidates would start.
struct TopkPlan { int kc, splits, ntiles; long long part_s, part_i, cand, total; };

inline TopkPlan topk_plan(long long nq, long long nt, int k, int margin, int splits, long long front_bytes) {
    TopkPlan p;
    p.kc = (int)(k + margin < nt ? k + margin : nt);
    p.splits = topk_splits(nq, nt, splits);
    p.ntiles = (int)((nt + TK_COLS - 1) / TK_COLS);
    const long long list = (long long)p.splits * nq * p.kc * 4;
    ScratchLayout lay;
    lay.take(front_bytes);
    p.part_s = lay.take(list), p.part_i = lay.take(list);
    p.cand = lay.take(nq * p.kc * 4), p.total = lay.end;
    return p;
}

// load4<true> may be used: whole float4s in every row, every row on a 16-byte boundary.
inline bool topk_vec_ok(int d, int ldq, int ldt, const float* q, const float* t) {
    return (d % 4 == 0) && (ldq % 4 == 0) && (ldt % 4 == 0) && ((((uintptr_t)q | (uintptr_t)t) & 15) == 0);
}

// Stage 1: the tiles kernel, in its vector or its scalar form, on the strip x splits grid.
template <class... A, class... B>
inline void topk_launch_tiles(void (*vec)(A...), void (*scalar)(A...), bool vec_ok, long long nq, int splits, hipStream_t st, B... args) {
    const dim3 grid((unsigned)((nq + TK_ROWS - 1) / TK_ROWS), (unsigned)splits);
    hipLaunchKernelGGL(vec_ok ? vec : scalar, grid, dim3(256), 0, st, args...);
}

// The merge of a plan's lists into its candidates (thread per row), then stage 2 on them (wave per row) with its own arguments.
template <class... A, class... B>
inline void topk_launch_rerank(void (*merge)(const float*, const int*, int, int, int, int*), void (*refine)(A...), const TopkPlan& p,
                               long long nq, void* scratch, hipStream_t st, B... refine_args) {
    hipLaunchKernelGGL(merge, dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, st, at<float>(scratch, p.part_s), at<int>(scratch, p.part_i),
                       (int)nq, p.kc, p.splits, at<int>(scratch, p.cand));
    hipLaunchKernelGGL(refine, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, refine_args...);
}

__device__ __forceinline__ bool topk_better(float s, int j, float ts, int tj) {
    return s > ts || (s == ts && (unsigned)j < (unsigned)tj);
}

// x[row][k .. k+3], zero outside [0, n) x [0, d)
template <bool VEC>
__device__ __forceinline__ f32x4v load4(const float* __restrict__ x, long long row, long long n, int k, int d, int ldx) {
    f32x4v v = {0.f, 0.f, 0.f, 0.f};
    if (row < n) {
        const float* p = x + row * (long long)ldx + k;
        if (VEC) {
            if (k < d) v = *reinterpret_cast<const f32x4v*>(p);
        } else {
            if (k < d) v[0] = p[0];
            if (k + 1 < d) v[1] = p[1];
            if (k + 2 < d) v[2] = p[2];
            if (k + 3 < d) v[3] = p[3];
        }
    }
    return v;
}

// The 32 x 64 block of inner products of row ra (the strip row c32 of this lane) with rows rb0 / rb1 (the wave's columns
// c32 / 32 + c32), two 32x32 accumulators.  load_a(row, k) / load_b(row, k) give x[row][k .. k+3], zero past the matrix.  The k
// loop runs in blocks of 8: lane half h supplies k = 8kb + 4h + s to MFMA step s, for A and B alike, so every product is the
// same fixed permutation of its fma chain.
template <class LA, class LB>
__device__ __forceinline__ void gram_32x64(const LA& load_a, const LB& load_b, int d, long long ra, long long rb0, long long rb1, int h,
                                           f32x16& acc0, f32x16& acc1) {
    const int nk = (d + 7) / 8;
    f32x4v a = load_a(ra, 4 * h), b0 = load_b(rb0, 4 * h), b1 = load_b(rb1, 4 * h);
    for (int kb = 0; kb < nk; ++kb) {
        const int kn = (kb + 1) * 8 + 4 * h;         // next block (zero past d: no access)
        const f32x4v an = load_a(ra, kn), b0n = load_b(rb0, kn), b1n = load_b(rb1, kn);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b0[s], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b1[s], acc1, 0, 0, 0);
        }
        a = an; b0 = b0n; b1 = b1n;
    }
}

// What a policy P of topk_tiles starts from: query rows qx [nq, ldq], train rows tx [nt, ldt], d columns each, lists of `width`
// <= TK_KMAX entries.  P adds
//   static constexpr bool EXCLUDE_SELF      column j is left out of global row j's list
//   float col_term(long long j) const       a per-column value, loaded once per tile (j may lie past nt)
//   float score(float acc, float t)         the ranked score from acc = q_i . t_j and the column's term (static, or const when
//                                           it needs a value of the launch, as the sign of the class report's scale)
struct TopkOperands {
    const float* __restrict__ qx;
    const float* __restrict__ tx;
    int nq, ldq, nt, ldt, d, width;
};

// One workgroup (256 threads): query rows [r0, r0 + 32) x the train tiles [t0, t1) of chunk blockIdx.y.  Wave w computes the
// 32 x 64 product block of columns w*64.. of a tile (gram_32x64).  Epilogue per tile: scores -> LDS; each (row, 32-column part)
// thread keeps the candidates that beat the row's current width-th entry (on a chunk's first tile also not worse than the
// width-th best of the 32 group-of-8 maxima of the tile, a valid lower bound; the maxima of empty groups are sentinels of
// their own, behind the lists', and only ever act as that bound); then the list is rebuilt from the old list plus the
// survivors by rank counting, which is exact and independent of the order the survivors were appended in.  A NaN score beats
// nothing and never enters a list.  The chunk's list goes to part_s / part_i [splits][nq][width].
template <bool VEC, class P>
__device__ __forceinline__ void topk_tiles(const P& p, int ntiles, int splits, float* __restrict__ part_s, int* __restrict__ part_i) {
    __shared__ float tile[TK_ROWS * TK_LD];
    __shared__ float ls[2][TK_ROWS * TK_KLD];
    __shared__ int li[2][TK_ROWS * TK_KLD];
    __shared__ unsigned char surv[TK_ROWS * TK_COLS];
    __shared__ int cnt[TK_ROWS];
    __shared__ float gms[TK_ROWS * TK_KLD];          // first tile: group maxima, then the tile bound in column 0
    __shared__ int gmi[TK_ROWS * TK_KLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c32 = lane & 31;
    const int r0 = blockIdx.x * TK_ROWS, split = blockIdx.y, nq = p.nq, nt = p.nt, width = p.width;
    const int nrow = nq - r0;                        // strip rows inside the matrix (> 0; may pass 32)
    const int t0 = (int)((long long)split * ntiles / splits), t1 = (int)((long long)(split + 1) * ntiles / splits);
    for (int e = tid; e < TK_ROWS * TK_KLD; e += 256) {
        ls[0][e] = -INFINITY;
        li[0][e] = -1 - (e % TK_KLD);                // distinct sentinels: ranks stay unique
    }
    if (tid < TK_ROWS) cnt[tid] = 0;
    int cur = 0;
    const auto load_q = [&](long long row, int k) { return load4<VEC>(p.qx, row, nq, k, p.d, p.ldq); };
    const auto load_t = [&](long long row, int k) { return load4<VEC>(p.tx, row, nt, k, p.d, p.ldt); };
    for (int t = t0; t < t1; ++t) {
        const long long cb = (long long)t * TK_COLS;       // < nt: every tile holds a column, so the casts below are exact
        const int jb = (int)cb, ncol = nt - jb < TK_COLS ? nt - jb : TK_COLS;      // tile column c < ncol is train row jb + c
        const long long ra = (long long)r0 + c32, rb0 = cb + wave * 64 + c32, rb1 = rb0 + 32;
        const float n0 = p.col_term(rb0), n1 = p.col_term(rb1);
        f32x16 acc0 = {}, acc1 = {};
        gram_32x64(load_q, load_t, p.d, ra, rb0, rb1, h, acc0, acc1);
#pragma unroll
        for (int q = 0; q < 16; ++q) {               // acc[q]: row 8(q/4) + 4h + q%4, column c32 (the last rebuild ended on a barrier)
            const int i = 8 * (q >> 2) + 4 * h + (q & 3);
            tile[i * TK_LD + wave * 64 + c32] = p.score(acc0[q], n0);
            tile[i * TK_LD + wave * 64 + 32 + c32] = p.score(acc1[q], n1);
        }
        __syncthreads();
        const int fr = tid & 31, part = tid >> 5;     // filter mapping: row fr, columns part*32 ..
        const int self = (int)((long long)r0 + fr - cb);     // the tile column of global row r0 + fr, if it has one
        const float* cls = ls[cur];
        const int* cli = li[cur];
        float bs = -INFINITY;                        // tile bound (first tile of the chunk only)
        int bj = -1;
        if (t == t0) {
            for (int g = 0; g < 4; ++g) {
                float ms = -INFINITY;
                int mj = -2 - TK_KMAX - (part * 4 + g);
                for (int m = 0; m < 8; ++m) {
                    const int c = part * 32 + g * 8 + m;
                    const float s = tile[fr * TK_LD + c];
                    if (c < ncol && !(P::EXCLUDE_SELF && c == self) && topk_better(s, jb + c, ms, mj)) { ms = s; mj = jb + c; }
                }
                gms[fr * TK_KLD + part * 4 + g] = ms;
                gmi[fr * TK_KLD + part * 4 + g] = mj;
            }
            __syncthreads();
            const int rr = tid >> 3, sub = tid & 7;
            float ws = 0.f;
            int wj = 0, hit = 0;
            for (int m = sub; m < 32; m += 8) {      // rank of each group maximum among the 32
                const float s = gms[rr * TK_KLD + m];
                const int j = gmi[rr * TK_KLD + m];
                int rank = 0;
                for (int q = 0; q < 32; ++q) rank += topk_better(gms[rr * TK_KLD + q], gmi[rr * TK_KLD + q], s, j);
                if (rank == width - 1) { ws = s; wj = j; hit = 1; }
            }
            __syncthreads();
            if (hit) { gms[rr * TK_KLD] = ws; gmi[rr * TK_KLD] = wj; }
            __syncthreads();
            bs = gms[fr * TK_KLD];
            bj = gmi[fr * TK_KLD];
        }
        if (fr < nrow) {
            const float ts = cls[fr * TK_KLD + width - 1];
            const int tj = cli[fr * TK_KLD + width - 1];
            for (int m = 0; m < 32; ++m) {
                const int c = part * 32 + m;
                if (c >= ncol) break;
                const int j = jb + c;
                const float s = tile[fr * TK_LD + c];
                if (!(P::EXCLUDE_SELF && c == self) && topk_better(s, j, ts, tj) && !topk_better(bs, bj, s, j)) {
                    const int sp = atomicAdd(&cnt[fr], 1);           // sp < 256: a tile has 256 columns
                    surv[fr * TK_COLS + sp] = (unsigned char)c;
                }
            }
        }
        __syncthreads();
        {   // rebuild: row rr's candidates are its `width` list entries and its survivors; rank < width goes to position rank
            const int rr = tid >> 3, sub = tid & 7, m_all = width + cnt[rr];
            float* nls = ls[cur ^ 1];
            int* nli = li[cur ^ 1];
            auto cand = [&](int m, float& s, int& j) {
                if (m < width) { s = cls[rr * TK_KLD + m]; j = cli[rr * TK_KLD + m]; }
                else { const int c = surv[rr * TK_COLS + m - width]; s = tile[rr * TK_LD + c]; j = jb + c; }
            };
            for (int m = sub; m < m_all; m += 8) {
                float s;
                int j;
                cand(m, s, j);
                int rank = 0;
                for (int q = 0; q < m_all; ++q) {
                    float s2;
                    int j2;
                    cand(q, s2, j2);
                    rank += topk_better(s2, j2, s, j);
                }
                if (rank < width) { nls[rr * TK_KLD + rank] = s; nli[rr * TK_KLD + rank] = j; }
            }
            __syncthreads();
            if (tid < TK_ROWS) cnt[tid] = 0;
            cur ^= 1;
        }
    }
    for (int e = tid; e < TK_ROWS * width; e += 256) {
        const int r = e / width, q = e - r * width;
        if (r < nrow) {
            const long long o = ((long long)split * nq + r0 + r) * width + q;
            part_s[o] = ls[cur][r * TK_KLD + q];
            part_i[o] = li[cur][r * TK_KLD + q];
        }
    }
}

// Thread per query row (64 per workgroup): the chunks' sorted lists merged pairwise in chunk order (exact under the strict
// order), then write(o, score, j) for every entry o = row * width + q of the merged list; j < 0 is a sentinel.
template <class W>
__device__ __forceinline__ void topk_merge(const float* __restrict__ part_s, const int* __restrict__ part_i, int nq, int width,
                                           int splits, const W& write) {
    __shared__ float bs[2][64 * TK_KLD];
    __shared__ int bi[2][64 * TK_KLD];
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x * 64 + tid;
    if (row >= nq) return;
    float* cs = &bs[0][tid * TK_KLD];
    int* ci = &bi[0][tid * TK_KLD];
    float* ns = &bs[1][tid * TK_KLD];
    int* ni = &bi[1][tid * TK_KLD];
    for (int q = 0; q < width; ++q) { cs[q] = part_s[row * width + q]; ci[q] = part_i[row * width + q]; }
    for (int s = 1; s < splits; ++s) {
        const float* ps = part_s + ((long long)s * nq + row) * width;
        const int* pi = part_i + ((long long)s * nq + row) * width;
        int ia = 0, ib = 0;
        for (int q = 0; q < width; ++q) {            // ia + ib = q < width: both stay in range
            const float sa = cs[ia], sb = ps[ib];
            const int ja = ci[ia], jb = pi[ib];
            if (topk_better(sa, ja, sb, jb)) { ns[q] = sa; ni[q] = ja; ++ia; }
            else { ns[q] = sb; ni[q] = jb; ++ib; }
        }
        float* ts = cs; cs = ns; ns = ts;
        int* ti = ci; ci = ni; ni = ti;
    }
    for (int q = 0; q < width; ++q) write(row * width + q, cs[q], ci[q]);
}

// The write of a two-stage user's merge kernel: candidates int32 [nq, kc], sentinels as they are.
struct TopkCandidates { int* __restrict__ cand; __device__ void operator()(long long o, float, int j) const { cand[o] = j; } };

// Stage 2 of a two-stage user: a row's merged candidates scored again in double from the fp32 operands and re-ranked; the first
// k -> out_idx / out_val [nq, k] (out_val may be NULL).  A policy R starts from TopkOperands (width = kc) and adds
//   static constexpr bool DESCENDING                 the larger value ranks first (else the smaller); equal values by index asc
//   static double acc(float q, float t, double s)    one element of the row sum
//   double finish(double s, int j) const             the ranked value, from the row sum and the column
//   static float publish(double v)                   what out_val gets
//   static int open_slot(int lane)                   what out_idx gets at a position that no candidate fills (out_val: NaN)
// One wave per row (4 per workgroup).  Lane l adds k = l, l + 64, ... ascending, then the xor tree of wave_sum_f64 (every lane ends
// with the same bits).  Only a VALID candidate, 0 <= j < nt, is scored: a sentinel is never an address.  The v-th valid candidate
// parks in lane v, which is also its place c in the list: a merged list carries its sentinels last (they sit at -inf behind every
// real index, topk_better).  A lane ranks its candidate among the valid ones with NaN last (NaN and the worst infinity share one
// key; the index settles equal keys); rank r < k writes position r.  Positions [valid, k) -- none unless scores were NaN -- are
// open slots.  No LDS, no barrier.
template <class R>
__device__ __forceinline__ void topk_refine(const R& r, int k, const int* __restrict__ cand, int* __restrict__ out_idx,
                                            float* __restrict__ out_val) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kc = r.width;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= r.nq) return;                         // whole waves leave
    const float* q = r.qx + row * (long long)r.ldq;
    double myv = 0.0;
    int myj = -1, valid = 0;
    for (int c = 0; c < kc; ++c) {
        const int j = cand[row * kc + c];            // wave-uniform
        if (j < 0 || j >= r.nt) continue;
        const float* t = r.tx + (long long)j * r.ldt;
        double s = 0.0;
        for (int kk = lane; kk < r.d; kk += 64) s = R::acc(q[kk], t[kk], s);
        const double v = r.finish(wave_sum_f64(s), j);
        if (lane == valid) { myv = v; myj = j; }
        ++valid;
    }
    const auto first = [](double a, double b) { return R::DESCENDING ? a > b : a < b; };
    const double worst = R::DESCENDING ? -(double)INFINITY : (double)INFINITY, key = first(myv, worst) ? myv : worst;
    int rank = 0;
    for (int c = 0; c < kc; ++c) {                   // every lane takes part in the shuffles
        const double v2 = __shfl(myv, c), key2 = first(v2, worst) ? v2 : worst;
        const int j2 = __shfl(myj, c);
        rank += j2 >= 0 && (first(key2, key) || (key2 == key && j2 < myj));
    }
    if (myj >= 0 && rank < k) {
        out_idx[row * k + rank] = myj;
        if (out_val) out_val[row * k + rank] = R::publish(myv);
    }
    if (lane >= valid && lane < k) {
        out_idx[row * k + lane] = R::open_slot(lane);
        if (out_val) out_val[row * k + lane] = __builtin_nanf("");
    }
}
