// k-nearest-neighbour probe (MultiBench/train.py:99-100: KNeighborsClassifier() -- Euclidean metric, uniform weights) for gfx950.
//
//   kp_norms     |t|^2 of every train row: one fp32 fma chain per row, k ascending
//   kp_tiles     stage 1: fused tile q_i . t_j on v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma chain), the candidate score
//                2 q.t - |t|^2 (the negated |t|^2 - 2 q.t; |q|^2 is constant per row) and a streaming per-row top-kc under the
//                strict order (score desc, index asc); one partial list per column chunk.  The scheme of knn_tiles
//                (umlh_kernels_align.hip) for two matrices and without the self exclusion.
//   kp_merge     merges the chunks' lists of a query -> candidates int32 [n_query, kc]
//   kp_refine    stage 2: sum_k (q_k - t_k)^2 in double from the fp32 inputs for the kc candidates of a query (one wave per
//                query: lane l adds k = l, l + 64, ... ascending, then a fixed xor tree), re-ranked by (value asc, index asc);
//                the first k -> idx, sqrt -> dist
//   kp_vote      the most frequent label among labels[idx[i, :k]], count ties to the smallest label value; integer count of
//                pred == y
//
// Nothing here forms an n_query x n_train array and no reduction uses a float atomic.  The result is bitwise independent of
// `splits`: column chunks start on 256-column tile boundaries, every score is the same fma chain wherever it is computed, and
// the kept lists are exact top-kc under a strict total order.
//
// List entries that no train row has filled are SENTINELS: negative indices -1 - e, compared as unsigned so that they sort
// behind every real index at an equal score.  A sentinel is never used as an address: kp_refine and kp_vote test
// 0 <= j < n_train before every gather, and kp_refine fills the positions that have no valid candidate (a query row of NaNs,
// whose comparisons are all false) with the in-range index of the position itself and a NaN distance.
#include "umlh_common.h"
#include "umlh_launch.h"
#include <climits>

namespace {

constexpr int KP_ROWS = 32;              // query rows of a workgroup's strip
constexpr int KP_COLS = 256;             // train rows of a tile: 4 waves x 64
constexpr int KP_LD = KP_COLS + 1;       // score tile row stride (floats): the filter's reads are conflict-free
constexpr int KP_KMAX = 32;              // list width: kc = min(k + 8, n_train) <= 32
constexpr int KP_KLD = KP_KMAX + 1;      // list row stride
constexpr int KP_MARGIN = 8;             // candidates kept beyond k
constexpr int KP_TARGET_WG = 512;        // auto splits: about two workgroups per CU of the 256
constexpr int KP_MAX_SPLITS = 1024;      // (grid y)

__device__ __forceinline__ bool kp_better(float s, int j, float ts, int tj) {
    return s > ts || (s == ts && (unsigned)j < (unsigned)tj);
}

// x[row][k .. k+3], zero outside [0, n) x [0, d)
template <bool VEC>
__device__ __forceinline__ f32x4v kp_load4(const float* __restrict__ x, long long row, long long n, int k, int d, int ldx) {
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

__global__ __launch_bounds__(256) void kp_norms(const float* __restrict__ t, long long n, int d, int ld, float* __restrict__ tn) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const float* p = t + row * (long long)ld;
    float s = 0.f;
    for (int k = 0; k < d; ++k) s = fmaf(p[k], p[k], s);
    tn[row] = s;
}

// One workgroup: query rows [r0, r0 + 32) x the train tiles [t0, t1) of chunk blockIdx.y.  Wave w computes the 32 x 64 product
// block of columns w*64.. of a tile with two 32x32 accumulators.  The k loop runs in blocks of 8: lane half h supplies
// k = 8kb + 4h + s to MFMA step s, for A (the query rows) and B (the train rows) alike, so every product is the same fixed
// permutation of its fma chain.  Epilogue per tile: scores -> LDS; each (row, 32-column part) thread keeps the candidates that
// beat the row's current kc-th entry (on a chunk's first tile also not worse than the kc-th best of the 32 group-of-8 maxima of
// the tile, a valid lower bound); then the list is rebuilt from the old list plus the survivors by rank counting, which is
// exact and independent of the order the survivors were appended in.  A NaN score beats nothing and never enters a list.
template <bool VEC>
__global__ __launch_bounds__(256) void kp_tiles(const float* __restrict__ qx, int nq, int ldq, const float* __restrict__ tx, int nt,
                                                int ldt, const float* __restrict__ tn, int d, int kc, int ntiles, int splits,
                                                float* __restrict__ part_s, int* __restrict__ part_i) {
    __shared__ float tile[KP_ROWS * KP_LD];
    __shared__ float ls[2][KP_ROWS * KP_KLD];
    __shared__ int li[2][KP_ROWS * KP_KLD];
    __shared__ unsigned char surv[KP_ROWS * KP_COLS];
    __shared__ int cnt[KP_ROWS];
    __shared__ float gms[KP_ROWS * KP_KLD];          // first tile: group maxima, then the tile bound in column 0
    __shared__ int gmi[KP_ROWS * KP_KLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c32 = lane & 31;
    const int r0 = blockIdx.x * KP_ROWS, split = blockIdx.y;
    const int t0 = (int)((long long)split * ntiles / splits), t1 = (int)((long long)(split + 1) * ntiles / splits);
    for (int e = tid; e < KP_ROWS * KP_KLD; e += 256) {
        ls[0][e] = -INFINITY;
        li[0][e] = -1 - (e % KP_KLD);                // distinct sentinels: ranks stay unique
    }
    if (tid < KP_ROWS) cnt[tid] = 0;
    int cur = 0;
    const int nk = (d + 7) / 8;
    for (int t = t0; t < t1; ++t) {
        const long long cb = (long long)t * KP_COLS;
        const long long ra = (long long)r0 + c32, rb0 = cb + wave * 64 + c32, rb1 = rb0 + 32;
        const float n0 = rb0 < nt ? tn[rb0] : 0.f, n1 = rb1 < nt ? tn[rb1] : 0.f;
        f32x16 acc0 = {}, acc1 = {};
        f32x4v a = kp_load4<VEC>(qx, ra, nq, 4 * h, d, ldq), b0 = kp_load4<VEC>(tx, rb0, nt, 4 * h, d, ldt),
               b1 = kp_load4<VEC>(tx, rb1, nt, 4 * h, d, ldt);
        for (int kb = 0; kb < nk; ++kb) {
            const int kn = (kb + 1) * 8 + 4 * h;     // next block (zero past d: no access)
            const f32x4v an = kp_load4<VEC>(qx, ra, nq, kn, d, ldq), b0n = kp_load4<VEC>(tx, rb0, nt, kn, d, ldt),
                         b1n = kp_load4<VEC>(tx, rb1, nt, kn, d, ldt);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b0[s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b1[s], acc1, 0, 0, 0);
            }
            a = an; b0 = b0n; b1 = b1n;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {               // acc[q]: row 8(q/4) + 4h + q%4, column c32 (the last rebuild ended on a barrier)
            const int i = 8 * (q >> 2) + 4 * h + (q & 3);
            tile[i * KP_LD + wave * 64 + c32] = fmaf(2.f, acc0[q], -n0);       // 2 q.t exact, one rounding
            tile[i * KP_LD + wave * 64 + 32 + c32] = fmaf(2.f, acc1[q], -n1);
        }
        __syncthreads();
        const int fr = tid & 31, part = tid >> 5;
        const long long gi = (long long)r0 + fr;      // filter mapping: row fr, columns part*32 ..
        const float* cls = ls[cur];
        const int* cli = li[cur];
        float bs = -INFINITY;                        // tile bound (first tile of the chunk only)
        int bj = -1;
        if (t == t0) {
            for (int g = 0; g < 4; ++g) {
                float ms = -INFINITY;
                int mj = -2 - KP_KMAX - (part * 4 + g);
                for (int m = 0; m < 8; ++m) {
                    const int c = part * 32 + g * 8 + m;
                    const float s = tile[fr * KP_LD + c];
                    if (cb + c < nt && kp_better(s, (int)(cb + c), ms, mj)) { ms = s; mj = (int)(cb + c); }
                }
                gms[fr * KP_KLD + part * 4 + g] = ms;
                gmi[fr * KP_KLD + part * 4 + g] = mj;
            }
            __syncthreads();
            const int rr = tid >> 3, sub = tid & 7;
            float ws = 0.f;
            int wj = 0, hit = 0;
            for (int m = sub; m < 32; m += 8) {      // rank of each group maximum among the 32
                const float s = gms[rr * KP_KLD + m];
                const int j = gmi[rr * KP_KLD + m];
                int rank = 0;
                for (int q = 0; q < 32; ++q) rank += kp_better(gms[rr * KP_KLD + q], gmi[rr * KP_KLD + q], s, j);
                if (rank == kc - 1) { ws = s; wj = j; hit = 1; }
            }
            __syncthreads();
            if (hit) { gms[rr * KP_KLD] = ws; gmi[rr * KP_KLD] = wj; }
            __syncthreads();
            bs = gms[fr * KP_KLD];
            bj = gmi[fr * KP_KLD];
        }
        if (gi < nq) {
            const float ts = cls[fr * KP_KLD + kc - 1];
            const int tj = cli[fr * KP_KLD + kc - 1];
            for (int m = 0; m < 32; ++m) {
                const int c = part * 32 + m;
                if (cb + c >= nt) break;
                const int j = (int)(cb + c);
                const float s = tile[fr * KP_LD + c];
                if (kp_better(s, j, ts, tj) && !kp_better(bs, bj, s, j)) {
                    const int p = atomicAdd(&cnt[fr], 1);            // p < 256: a tile has 256 columns
                    surv[fr * KP_COLS + p] = (unsigned char)c;
                }
            }
        }
        __syncthreads();
        {   // rebuild: row rr's candidates are its kc list entries and its survivors; rank < kc goes to position rank
            const int rr = tid >> 3, sub = tid & 7, m_all = kc + cnt[rr];
            float* nls = ls[cur ^ 1];
            int* nli = li[cur ^ 1];
            auto cand = [&](int m, float& s, int& j) {
                if (m < kc) { s = cls[rr * KP_KLD + m]; j = cli[rr * KP_KLD + m]; }
                else { const int c = surv[rr * KP_COLS + m - kc]; s = tile[rr * KP_LD + c]; j = (int)(cb + c); }
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
                    rank += kp_better(s2, j2, s, j);
                }
                if (rank < kc) { nls[rr * KP_KLD + rank] = s; nli[rr * KP_KLD + rank] = j; }
            }
            __syncthreads();
            if (tid < KP_ROWS) cnt[tid] = 0;
            cur ^= 1;
        }
    }
    for (int e = tid; e < KP_ROWS * kc; e += 256) {
        const int r = e / kc, q = e - r * kc;
        if ((long long)r0 + r < nq) {
            const long long o = ((long long)split * nq + r0 + r) * kc + q;
            part_s[o] = ls[cur][r * KP_KLD + q];
            part_i[o] = li[cur][r * KP_KLD + q];
        }
    }
}

// Thread per query: the chunks' sorted lists merged pairwise in chunk order (exact under the strict order).
__global__ __launch_bounds__(64) void kp_merge(const float* __restrict__ part_s, const int* __restrict__ part_i, int nq, int kc,
                                               int splits, int* __restrict__ cand) {
    __shared__ float bs[2][64 * KP_KLD];
    __shared__ int bi[2][64 * KP_KLD];
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x * 64 + tid;
    if (row >= nq) return;
    float* cs = &bs[0][tid * KP_KLD];
    int* ci = &bi[0][tid * KP_KLD];
    float* ns = &bs[1][tid * KP_KLD];
    int* ni = &bi[1][tid * KP_KLD];
    for (int q = 0; q < kc; ++q) { cs[q] = part_s[row * kc + q]; ci[q] = part_i[row * kc + q]; }
    for (int s = 1; s < splits; ++s) {
        const float* ps = part_s + ((long long)s * nq + row) * kc;
        const int* pi = part_i + ((long long)s * nq + row) * kc;
        int ia = 0, ib = 0;
        for (int q = 0; q < kc; ++q) {               // ia + ib = q < kc: both stay in range
            const float sa = cs[ia], sb = ps[ib];
            const int ja = ci[ia], jb = pi[ib];
            if (kp_better(sa, ja, sb, jb)) { ns[q] = sa; ni[q] = ja; ++ia; }
            else { ns[q] = sb; ni[q] = jb; ++ib; }
        }
        float* ts = cs; cs = ns; ns = ts;
        int* ti = ci; ci = ni; ni = ti;
    }
    for (int q = 0; q < kc; ++q) cand[row * kc + q] = ci[q];
}

// One wave per query (4 per workgroup).  Candidate c's squared distance: lane l sums (q_k - t_k)^2 over k = l, l + 64, ... in
// double, then the xor tree 32, 16, .., 1 (every lane ends with the same bits); lane c keeps it.  Lane c < kc then ranks its
// candidate among the VALID candidates (0 <= j < nt) by (value, index) with NaN ordered as +inf; rank r < k writes position r.
// Positions [valid, k) -- there are none unless the row's scores were NaN -- get the index of the position (k <= nt) and a
// NaN distance.  No LDS, no barrier.
__global__ __launch_bounds__(256) void kp_refine(const float* __restrict__ qx, int nq, int ldq, const float* __restrict__ tx, int nt,
                                                 int ldt, int d, int k, int kc, const int* __restrict__ cand, int* __restrict__ idx,
                                                 float* __restrict__ dist) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= nq) return;                           // whole waves leave
    const float* q = qx + row * (long long)ldq;
    double myv = 0.0;
    int myj = -1, valid = 0;
    for (int c = 0; c < kc; ++c) {
        const int j = cand[row * kc + c];            // wave-uniform
        if (j < 0 || j >= nt) continue;              // a sentinel is never an address
        const float* t = tx + (long long)j * ldt;
        double s = 0.0;
        for (int kk = lane; kk < d; kk += 64) {
            const double df = (double)q[kk] - (double)t[kk];
            s = fma(df, df, s);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == c) { myv = s; myj = j; }
        ++valid;
    }
    const double inf = (double)INFINITY, key = myv < inf ? myv : inf;
    int rank = 0;
    for (int c = 0; c < kc; ++c) {                   // every lane takes part in the shuffles
        const double v2 = __shfl(myv, c), key2 = v2 < inf ? v2 : inf;
        const int j2 = __shfl(myj, c);
        rank += j2 >= 0 && (key2 < key || (key2 == key && j2 < myj));
    }
    if (myj >= 0 && rank < k) {
        idx[row * k + rank] = myj;
        if (dist) dist[row * k + rank] = (float)sqrt(myv);
    }
    if (lane >= valid && lane < k) {
        idx[row * k + lane] = lane;
        if (dist) dist[row * k + lane] = __builtin_nanf("");
    }
}

// Thread per query.  The winner has the largest count; among equal counts the smallest label value (sklearn: argmax over the
// sorted classes_).  An index outside [0, nt) casts no vote (umlh_knn_search never writes one); a row with no vote predicts -1.
__global__ __launch_bounds__(256) void kp_vote(const int* __restrict__ idx, int nq, int k, const int* __restrict__ labels, int nt,
                                               const int* __restrict__ y, int* __restrict__ pred, int* __restrict__ votes,
                                               unsigned long long* __restrict__ correct) {
    __shared__ int red[256];
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x * 256 + tid;
    int hit = 0;
    if (row < nq) {
        int lab[24];
#pragma unroll
        for (int p = 0; p < 24; ++p) {
            lab[p] = -1;
            if (p < k) {
                const int j = idx[row * k + p];
                if (j >= 0 && j < nt) lab[p] = labels[j];
            }
        }
        int best = -1, best_n = 0;
#pragma unroll
        for (int p = 0; p < 24; ++p) {
            int c = 0;
#pragma unroll
            for (int q = 0; q < 24; ++q) c += (lab[q] == lab[p]);
            if (lab[p] >= 0 && (c > best_n || (c == best_n && lab[p] < best))) { best = lab[p]; best_n = c; }
        }
        if (pred) pred[row] = best;
        if (votes) votes[row] = best_n;
        if (y) hit = (y[row] == best);
    }
    if (correct) {
        red[tid] = hit;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0 && red[0]) atomicAdd(correct, (unsigned long long)red[0]);      // integer: exact in any order
    }
}

inline long long kp_align_up(long long x) { return (x + 255) / 256 * 256; }

struct KpPlan { int kc, splits, ntiles; long long norms, part_s, part_i, cand, total; };

KpPlan kp_plan(long long nt, long long nq, int k, int splits) {
    KpPlan p;
    p.kc = (int)(k + KP_MARGIN < nt ? k + KP_MARGIN : nt);
    const long long ntiles = (nt + KP_COLS - 1) / KP_COLS, strips = (nq + KP_ROWS - 1) / KP_ROWS;
    long long s = splits > 0 ? splits : (KP_TARGET_WG + strips - 1) / strips;
    if (s > KP_MAX_SPLITS) s = KP_MAX_SPLITS;
    p.splits = (int)(s < 1 ? 1 : (s > ntiles ? ntiles : s));
    p.ntiles = (int)ntiles;
    const long long list = kp_align_up((long long)p.splits * nq * p.kc * 4);
    p.norms = 0;
    p.part_s = kp_align_up(nt * 4);
    p.part_i = p.part_s + list;
    p.cand = p.part_i + list;
    p.total = p.cand + kp_align_up(nq * p.kc * 4);
    return p;
}

}  // namespace

// ---- plan and launchers (validation is the caller's: umlh_api.cpp) ----
extern "C" {

unsigned long long umlh_knn_bytes(long long nt, long long nq, int k, int splits) {
    return (unsigned long long)kp_plan(nt, nq, k, splits).total;
}

int umlh_knn_launch_search(const float* train, long long nt, int ldt, const float* query, long long nq, int ldq, int d, int k,
                           int splits, int* idx, float* dist, void* scratch, hipStream_t st) {
    const KpPlan p = kp_plan(nt, nq, k, splits);
    float* tn = (float*)((char*)scratch + p.norms);
    float* ps = (float*)((char*)scratch + p.part_s);
    int* pi = (int*)((char*)scratch + p.part_i);
    int* cand = (int*)((char*)scratch + p.cand);
    hipLaunchKernelGGL(kp_norms, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, train, nt, d, ldt, tn);
    const dim3 grid((unsigned)((nq + KP_ROWS - 1) / KP_ROWS), (unsigned)p.splits);
    const bool vec = (d % 4 == 0) && (ldt % 4 == 0) && (ldq % 4 == 0) && ((((uintptr_t)train | (uintptr_t)query) & 15) == 0);
    if (vec)
        hipLaunchKernelGGL(kp_tiles<true>, grid, dim3(256), 0, st, query, (int)nq, ldq, train, (int)nt, ldt, tn, d, p.kc, p.ntiles,
                           p.splits, ps, pi);
    else
        hipLaunchKernelGGL(kp_tiles<false>, grid, dim3(256), 0, st, query, (int)nq, ldq, train, (int)nt, ldt, tn, d, p.kc, p.ntiles,
                           p.splits, ps, pi);
    hipLaunchKernelGGL(kp_merge, dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, st, ps, pi, (int)nq, p.kc, p.splits, cand);
    hipLaunchKernelGGL(kp_refine, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, query, (int)nq, ldq, train, (int)nt, ldt, d, k,
                       p.kc, cand, idx, dist);
    return (int)hipGetLastError();
}

int umlh_knn_launch_vote(const int* idx, long long nq, int k, const int* labels, long long nt, const int* y, int* pred, int* votes,
                         long long* correct, hipStream_t st) {
    if (correct) {
        const hipError_t e = hipMemsetAsync(correct, 0, 8, st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kp_vote, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, idx, (int)nq, k, labels, (int)nt, y, pred, votes,
                       (unsigned long long*)correct);
    return (int)hipGetLastError();
}

}  // extern "C"
