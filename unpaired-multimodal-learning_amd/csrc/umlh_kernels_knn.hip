// k-nearest-neighbour probe (MultiBench/train.py:99-100: KNeighborsClassifier() -- Euclidean metric, uniform weights) for gfx950.
//
//   kp_norms     |t|^2 of every train row: one fp32 fma chain per row, k ascending
//   kp_tiles     stage 1: fused tile q_i . t_j on v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma chain), the candidate score
//                2 q.t - |t|^2 (the negated |t|^2 - 2 q.t; |q|^2 is constant per row) and a streaming per-row top-kc under the
//                strict order (score desc, index asc); one partial list per column chunk.  The body is topk_tiles of
//                umlh_topk.h, which knn_tiles (umlh_kernels_align.hip) runs as well: here on two matrices, with the score
//                epilogue above and without the self exclusion.
//   kp_merge     merges the chunks' lists of a query (topk_merge) -> candidates int32 [n_query, kc]
//   kp_refine    stage 2: sum_k (q_k - t_k)^2 in double from the fp32 inputs for the kc candidates of a query, re-ranked by
//                (value asc, index asc); the first k -> idx, sqrt -> dist.  The body is topk_refine of umlh_topk.h, which
//                ev_refine (umlh_kernels_evalreport.hip) runs as well.
//   kp_vote      the most frequent label among labels[idx[i, :k]], count ties to the smallest label value; integer count of
//                pred == y
//
// Nothing here forms an n_query x n_train array and no reduction uses a float atomic.  The result is bitwise independent of
// `splits`: column chunks start on 256-column tile boundaries, every score is the same fma chain wherever it is computed, and
// the kept lists are exact top-kc under a strict total order.
//
// List entries that no train row has filled are SENTINELS (umlh_topk.h): negative indices.  A sentinel is never used as an
// address: kp_refine and kp_vote test 0 <= j < n_train before every gather, and kp_refine fills the positions that have no
// valid candidate (a query row of NaNs, whose comparisons are all false; NaN train rows when n_train < k + their count) with
// the in-range index of the position itself and a NaN distance.
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
    topk_merge(part_s, part_i, nq, kc, splits, TopkCandidates{cand});
}

// A candidate's squared distance sum_k (q_k - t_k)^2, the smaller first; sqrt -> dist.  A position without a candidate gets its
// own index (k <= n_train: in range).
struct KpDistance : TopkOperands {
    static constexpr bool DESCENDING = false;
    __device__ static double acc(float q, float t, double s) { const double df = (double)q - (double)t; return fma(df, df, s); }
    __device__ static double finish(double s, int) { return s; }
    __device__ static float publish(double v) { return (float)sqrt(v); }
    __device__ static int open_slot(int lane) { return lane; }
};

// Stage 2 (topk_refine, umlh_topk.h): one wave per query (4 per workgroup) re-ranks its kc candidates -> idx, dist [n_query, k].
__global__ __launch_bounds__(256) void kp_refine(const float* __restrict__ qx, int nq, int ldq, const float* __restrict__ tx, int nt,
                                                 int ldt, int d, int k, int kc, const int* __restrict__ cand, int* __restrict__ idx,
                                                 float* __restrict__ dist) {
    topk_refine(KpDistance{{qx, tx, nq, ldq, nt, ldt, d, kc}}, k, cand, idx, dist);
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

// |t|^2 [n_train] in front of the lists and candidates
TopkPlan kp_plan(long long nt, long long nq, int k, int splits) { return topk_plan(nq, nt, k, KP_MARGIN, splits, nt * 4); }

}  // namespace

// ---- plan and launchers (validation is the caller's: umlh_ops.cpp) ----
extern "C" {

unsigned long long umlh_knn_bytes(long long nt, long long nq, int k, int splits) {
    return (unsigned long long)kp_plan(nt, nq, k, splits).total;
}

int umlh_knn_launch_search(const float* train, long long nt, int ldt, const float* query, long long nq, int ldq, int d, int k,
                           int splits, int* idx, float* dist, void* scratch, hipStream_t st) {
    const TopkPlan p = kp_plan(nt, nq, k, splits);
    float* tn = at<float>(scratch, 0);
    hipLaunchKernelGGL(kp_norms, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, train, nt, d, ldt, tn);
    topk_launch_tiles(kp_tiles<true>, kp_tiles<false>, topk_vec_ok(d, ldq, ldt, query, train), nq, p.splits, st, query, (int)nq, ldq,
                      train, (int)nt, ldt, tn, d, p.kc, p.ntiles, p.splits, at<float>(scratch, p.part_s), at<int>(scratch, p.part_i));
    topk_launch_rerank(kp_merge, kp_refine, p, nq, scratch, st, query, (int)nq, ldq, train, (int)nt, ldt, d, k, p.kc,
                       at<int>(scratch, p.cand), idx, dist);
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
