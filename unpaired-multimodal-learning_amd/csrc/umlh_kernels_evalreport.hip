// Class-wise validation report (the `val_classwise` slot of finetune.train()) for gfx950.
//
//   ev_tiles     stage 1: fused tile x_i . w_j on v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma chain), the candidate score
//                sgn * (x.w_j + b_j) with sgn = sign(scale) in {-1, 0, +1} read from the device scalar (both factors exact: the
//                order is that of the scaled logits whatever the sign; a zero scale ties every class, which the index settles)
//                and a streaming per-row top-kc under the strict order (score desc, index asc); one partial list per column
//                chunk.  The body is topk_tiles of umlh_topk.h, which knn_tiles (umlh_kernels_align.hip) and kp_tiles
//                (umlh_kernels_knn.hip) run as well: here the train rows are the head's weight rows, nothing is excluded.
//   ev_merge     merges the chunks' lists of a row (topk_merge) -> candidates int32 [n, kc]
//   ev_refine    stage 2: z = (double)scale * (sum_k (double)x_k (double)w_jk + (double)b_j) for the kc candidates of a row,
//                re-ranked by (z desc, class index asc); the first k -> cls, z rounded once to fp32 -> logit.  The body is
//                topk_refine of umlh_topk.h, which kp_refine (umlh_kernels_knn.hip) runs as well.
//   ev_classwise per-class support / top-1 hits / top-k hits / confusion counts from cls and the labels: 64-bit integer
//                atomics only, one per distinct (label, prediction) pair of a wave; the outputs are ADDED into
//
// Nothing here forms an n x C array and no reduction uses a float atomic.  The top-k result is bitwise independent of `splits`:
// column chunks start on 256-column tile boundaries, every score is the same fma chain wherever it is computed, and the kept
// lists are exact top-kc under a strict total order.
//
// List entries that no class has filled are SENTINELS (umlh_topk.h): negative indices.  A sentinel is never used as an address: ev_refine
// tests 0 <= j < C before every gather and fills the positions that have no valid candidate (a row of NaNs, whose comparisons
// are all false) with class -1 and a NaN logit; ev_classwise treats a class outside [0, C) as "no prediction".
#include "umlh_common.h"
#include "umlh_launch.h"
#include "umlh_topk.h"

namespace {

constexpr int EV_MARGIN = 8;             // candidates kept beyond k: kc = min(k + 8, C) <= TK_KMAX

// Feature rows against head weight rows: the candidate score sgn * (x.w_j + b_j), nothing excluded.
struct EvPair : TopkOperands {
    const float* __restrict__ bias;      // [nt] or NULL
    float sgn;
    static constexpr bool EXCLUDE_SELF = false;
    __device__ float col_term(long long j) const { return bias && j < nt ? bias[j] : 0.f; }
    __device__ float score(float acc, float b) const { return sgn * (acc + b); }
};

// Stage 1 (topk_tiles, umlh_topk.h): rows [32 blockIdx.x, +32) x the class tiles of chunk blockIdx.y -> one partial list.
template <bool VEC>
__global__ __launch_bounds__(256) void ev_tiles(const float* __restrict__ x, int n, int ldx, const float* __restrict__ w, int C, int ldw,
                                                const float* __restrict__ bias, const float* __restrict__ scale, int d, int kc,
                                                int ntiles, int splits, float* __restrict__ part_s, int* __restrict__ part_i) {
    const float sc = scale ? *scale : 1.f;
    const float sgn = sc > 0.f ? 1.f : (sc < 0.f ? -1.f : 0.f);
    topk_tiles<VEC>(EvPair{{x, w, n, ldx, C, ldw, d, kc}, bias, sgn}, ntiles, splits, part_s, part_i);
}

// topk_merge -> candidates int32 [n, kc], sentinels as they are.
__global__ __launch_bounds__(64) void ev_merge(const float* __restrict__ part_s, const int* __restrict__ part_i, int n, int kc,
                                               int splits, int* __restrict__ cand) {
    topk_merge(part_s, part_i, n, kc, splits, TopkCandidates{cand});
}

// A candidate's logit z = scale * (sum_k x_k w_jk + b_j), the larger first; z rounded once to fp32 -> logit.  A position without
// a candidate gets class -1.
struct EvLogit : TopkOperands {
    const float* __restrict__ bias;      // [nt] or NULL
    double sc;
    static constexpr bool DESCENDING = true;
    __device__ static double acc(float x, float w, double s) { return fma((double)x, (double)w, s); }
    __device__ double finish(double s, int j) const { return sc * (s + (bias ? (double)bias[j] : 0.0)); }
    __device__ static float publish(double z) { return (float)z; }
    __device__ static int open_slot(int) { return -1; }
};

// Stage 2 (topk_refine, umlh_topk.h): one wave per row (4 per workgroup) re-ranks its kc candidates -> cls, logit [n, k].
__global__ __launch_bounds__(256) void ev_refine(const float* __restrict__ x, int n, int ldx, const float* __restrict__ w, int C, int ldw,
                                                 const float* __restrict__ bias, const float* __restrict__ scale, int d, int k, int kc,
                                                 const int* __restrict__ cand, int* __restrict__ cls, float* __restrict__ logit) {
    topk_refine(EvLogit{{x, w, n, ldx, C, ldw, d, kc}, bias, scale ? (double)*scale : 1.0}, k, cand, cls, logit);
}

__device__ __forceinline__ void add_i64(long long* p, int v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// Thread per row.  A row whose label lies outside [0, C) counts in misc[0] alone.  The others are grouped inside their wave
// by (label, prediction) -- prediction = cls[i, 0], or -1 when that lies outside [0, C) -- and the first lane of a group adds the
// group's counts: one atomic per output and group, so a table of one class costs one atomic per wave and counter, not one per
// row.  A group without a prediction counts in support and misc[1] alone.  Integer sums: the result does not depend on the order.
__global__ __launch_bounds__(256) void ev_classwise(const int* __restrict__ cls, long long n, int k, const long long* __restrict__ labels,
                                                    long long C, long long* __restrict__ support, long long* __restrict__ hit1,
                                                    long long* __restrict__ hitk, long long* __restrict__ confusion,
                                                    long long* __restrict__ misc) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    long long lab = -1;
    int pred = -1, among = 0;
    bool valid = false, ignored = false;
    if (row < n) {
        lab = labels[row];
        valid = lab >= 0 && lab < C;
        ignored = !valid;
        if (valid) {
            const int* cr = cls + row * k;
            const int p = cr[0];
            pred = p >= 0 && p < C ? p : -1;
            for (int q = 0; q < k; ++q) among |= (cr[q] == lab);
        }
    }
    const unsigned long long ign = __ballot(ignored);
    if (ign && lane == __ffsll((long long)ign) - 1) add_i64(&misc[0], __popcll(ign));
    unsigned long long todo = __ballot(valid);
    while (todo) {                                   // wave-uniform: every lane sees the same mask
        const int leader = __ffsll((long long)todo) - 1;
        const long long gl = __shfl(lab, leader);
        const int gp = __shfl(pred, leader);
        const bool mine = valid && lab == gl && pred == gp;
        const unsigned long long grp = __ballot(mine), grpk = __ballot(mine && among);
        if (lane == leader) {
            const int cnt = __popcll(grp), cntk = __popcll(grpk);
            add_i64(&support[gl], cnt);
            if (gp < 0) add_i64(&misc[1], cnt);
            else {
                if (gp == gl) add_i64(&hit1[gl], cnt);
                if (cntk) add_i64(&hitk[gl], cntk);
                if (confusion) add_i64(&confusion[gl * C + gp], cnt);
            }
        }
        todo &= ~grp;
    }
}

}  // namespace

// ---- plan and launchers (validation is the caller's: umlh_ops.cpp) ----
extern "C" {

unsigned long long umlh_evalreport_bytes(long long n, long long C, int k, int splits) {
    return (unsigned long long)topk_plan(n, C, k, EV_MARGIN, splits, 0).total;
}

int umlh_evalreport_launch_topk(const float* x, long long n, int ldx, const float* w, long long C, int ldw, int d, const float* bias,
                                const float* scale, int k, int splits, int* cls, float* logit, void* scratch, hipStream_t st) {
    const TopkPlan p = topk_plan(n, C, k, EV_MARGIN, splits, 0);
    topk_launch_tiles(ev_tiles<true>, ev_tiles<false>, topk_vec_ok(d, ldx, ldw, x, w), n, p.splits, st, x, (int)n, ldx, w, (int)C, ldw,
                      bias, scale, d, p.kc, p.ntiles, p.splits, at<float>(scratch, p.part_s), at<int>(scratch, p.part_i));
    topk_launch_rerank(ev_merge, ev_refine, p, n, scratch, st, x, (int)n, ldx, w, (int)C, ldw, bias, scale, d, k, p.kc,
                       at<int>(scratch, p.cand), cls, logit);
    return (int)hipGetLastError();
}

int umlh_evalreport_launch_classwise(const int* cls, long long n, int k, const long long* labels, long long C, long long* support,
                                     long long* hit1, long long* hitk, long long* confusion, long long* misc, hipStream_t st) {
    hipLaunchKernelGGL(ev_classwise, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cls, n, k, labels, C, support, hit1, hitk,
                       confusion, misc);
    return (int)hipGetLastError();
}

}  // extern "C"
