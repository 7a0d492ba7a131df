// k-nearest-neighbour probe (MultiBench/train.py:99-100: KNeighborsClassifier() -- Euclidean metric, uniform weights) for gfx950.
//
//   kp_norms     |t|^2 of every train row: one fp32 fma chain per row, k ascending
//   kp_tiles     stage 1: fused tile q_i . t_j on v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma chain), the candidate score
//                2 q.t - |t|^2 (the negated |t|^2 - 2 q.t; |q|^2 is constant per row) and a streaming per-row top-kc under the
//                strict order (score desc, index asc); one partial list per column chunk.  The body is topk_tiles of
//                umlh_topk.h, which knn_tiles (umlh_kernels_align.hip) runs as well: here on two matrices, with the score
//                epilogue above and without the self exclusion.
//   kp_merge     merges the chunks' lists of a query (topk_merge) -> candidates int32 [n_query, kc]
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
#include "umlh_topk.h"

namespace {

constexpr int KP_MARGIN = 8;             // candidates kept beyond k: kc = min(k + 8, n_train) <= TK_KMAX

__global__ __launch_bounds__(256) void kp_norms(const float* __restrict__ t, long long n, int d, int ld, float* __restrict__ tn) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const float* p = t + row * (long long)ld;
    float s = 0.f;
    for (int k = 0; k < d; ++k) s = fmaf(p[k], p[k], s);
    tn[row] = s;
}

// Query rows against train rows: the candidate score 2 q.t - |t|^2 (2 q.t exact, one rounding), nothing excluded.
struct KpPair : TopkOperands {
    const float* __restrict__ tn;
    static constexpr bool EXCLUDE_SELF = false;
    __device__ float col_term(long long j) const { return j < nt ? tn[j] : 0.f; }
    __device__ static float score(float acc, float t2) { return fmaf(2.f, acc, -t2); }
};

// Stage 1 (topk_tiles, umlh_topk.h): query rows [32 blockIdx.x, +32) x the train tiles of chunk blockIdx.y -> one partial list.
template <bool VEC>
__global__ __launch_bounds__(256) void kp_tiles(const float* __restrict__ qx, int nq, int ldq, const float* __restrict__ tx, int nt,
                                                int ldt, const float* __restrict__ tn, int d, int kc, int ntiles, int splits,
                                                float* __restrict__ part_s, int* __restrict__ part_i) {
    topk_tiles<VEC>(KpPair{{qx, tx, nq, ldq, nt, ldt, d, kc}, tn}, ntiles, splits, part_s, part_i);
}

// topk_merge -> candidates int32 [n_query, kc], sentinels as they are.
__global__ __launch_bounds__(64) void kp_merge(const float* __restrict__ part_s, const int* __restrict__ part_i, int nq, int kc,
                                               int splits, int* __restrict__ cand) {
    topk_merge(part_s, part_i, nq, kc, splits, [=](long long o, float, int j) { cand[o] = j; });
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
        s = wave_sum_f64(s);
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
        hit = block_reduce<256>(hit, red, OpSum());
        if (tid == 0 && hit) atomicAdd(correct, (unsigned long long)hit);            // integer: exact in any order
    }
}

struct KpPlan { int kc, splits, ntiles; long long norms, part_s, part_i, cand, total; };

KpPlan kp_plan(long long nt, long long nq, int k, int splits) {
    KpPlan p;
    p.kc = (int)(k + KP_MARGIN < nt ? k + KP_MARGIN : nt);
    p.splits = topk_splits(nq, nt, splits);
    p.ntiles = (int)((nt + TK_COLS - 1) / TK_COLS);
    const long long list = align_up((long long)p.splits * nq * p.kc * 4);
    p.norms = 0;
    p.part_s = align_up(nt * 4);
    p.part_i = p.part_s + list;
    p.cand = p.part_i + list;
    p.total = p.cand + align_up(nq * p.kc * 4);
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
    float* tn = at<float>(scratch, p.norms);
    float* ps = at<float>(scratch, p.part_s);
    int* pi = at<int>(scratch, p.part_i);
    int* cand = at<int>(scratch, p.cand);
    hipLaunchKernelGGL(kp_norms, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, train, nt, d, ldt, tn);
    const dim3 grid((unsigned)((nq + TK_ROWS - 1) / TK_ROWS), (unsigned)p.splits);
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
