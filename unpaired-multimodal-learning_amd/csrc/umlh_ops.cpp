// The stateless entry points of include/umlh.h, in the header's section order: each one checks its arguments and calls one
// launcher (a few chain two or three).  None takes a umlh_handle_t (those are in umlh_api.cpp).  Every check precedes the
// first HIP call, so a refused call has touched neither the device nor the stream.  No allocation, no synchronisation (one
// exception, said where it is: the host-side tables of umlh_ae_train_steps_grouped).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "umlh_host.h"
#include "umlh_launch.h"

// ---- the vocabulary of checks ----
// Row counts and int32 strides: n < 2^31 wherever a kernel indexes rows with an int; n <= 2^30 in the alignment metrics, whose
// int32 indices need room for the tile and sentinel arithmetic.
static const int64_t ROWS_END = (int64_t)1 << 31;         // exclusive
static const int64_t ALIGN_MAX_ROWS = (int64_t)1 << 30;   // inclusive
// the longest neighbour / class list of the streaming top-k users with a vote or a report behind them (k-NN probe, class-wise report)
static const int LIST_MAX_K = 24;

// int64_t is `long` here and the launchers take `long long`: same size, distinct types
static_assert(sizeof(long long) == sizeof(int64_t), "the launchers' long long is the ABI's int64_t");
static inline const long long* ll(const int64_t* p) { return reinterpret_cast<const long long*>(p); }
static inline long long* ll(int64_t* p) { return reinterpret_cast<long long*>(p); }

// The one scratch check: the size, then (align != 0) the alignment of the base.  Every region of every scratch layout starts
// on a 256-byte boundary from the base (align_up, umlh_launch.h), so the base decides the alignment of every slab.
// The policy records what each entry point has always checked; it is not derived from the layouts, and the entry points keep it:
//   8 bytes  umlh_probe_fit (fp64 solver state), umlh_row_abs_quantile (fp64 partials), umlh_abs_kth (u64 histogram),
//            umlh_knn_accuracy (int64 partials), umlh_seq_column_standardize and umlh_tab_standardize (fp64 partials);
//   4 bytes  umlh_knn_search, umlh_eval_topk (float scores and int indices of the top-k core, nothing wider);
//   none     everything else.  Of these umlh_align_knn (float / int) and umlh_class_index (int counts) need 4 bytes and
//            umlh_seq_mse_backward takes a float*; the others carve fp64 or int64 slabs (Gram and column sums, partial sums,
//            eigen-solver work) and rely on the caller's allocator: the Python side passes blocks of torch's caching
//            allocator, which are aligned far beyond 8 bytes.
// Two wordings of the size line exist and tests pin both: SCRATCH_BYTES_EQ is the one of the report and outlier sections.
static const char SCRATCH_OF[] = "%s: scratch of %llu bytes, %llu needed";
static const char SCRATCH_BYTES_EQ[] = "%s: scratch_bytes=%llu, %llu needed";
static int check_scratch(const char* who, const void* scratch, uint64_t scratch_bytes, uint64_t need, unsigned align,
                         const char* size_fmt = SCRATCH_OF) {
    if (scratch_bytes < need) return fail(UMLH_E_INVALID, size_fmt, who, (unsigned long long)scratch_bytes, (unsigned long long)need);
    if (align && (reinterpret_cast<uintptr_t>(scratch) & (align - 1)) != 0)
        return fail(UMLH_E_INVALID, "%s: scratch must be %u-byte aligned", who, align);
    return UMLH_OK;
}

// two nested strides cover `outer` x `inner` rows of d floats without overlap in one of the two nestings
static bool strides_ok(int64_t outer, int64_t inner, int32_t d, int64_t so, int64_t si) {
    if (si < d || (outer > 1 && so < d)) return false;
    if (outer <= 1 || inner <= 1) return true;
    return so >= (inner - 1) * si + d || si >= (outer - 1) * so + d;
}

// the stride checks of one [b, t_len, d] view; 0 = fine
static int check_strides(const char* who, const char* ldb_name, const char* ldt_name, int32_t b, int32_t t_len, int32_t d, int64_t ldb,
                         int64_t ldt) {
    if (ldt < d) return fail(UMLH_E_INVALID, "%s: %s=%lld < d=%d", who, ldt_name, (long long)ldt, d);
    if (ldb < d) return fail(UMLH_E_INVALID, "%s: %s=%lld < d=%d", who, ldb_name, (long long)ldb, d);
    if (!strides_ok(b, t_len, d, ldb, ldt))
        return fail(UMLH_E_INVALID, "%s: %s=%lld %s=%lld overlap for b=%d t_len=%d d=%d", who, ldb_name, (long long)ldb, ldt_name,
                    (long long)ldt, b, t_len, d);
    return UMLH_OK;
}

// the list length and the row count of the alignment entry points that take topk >= 1; 0 = fine.  who = NULL: no message (a
// size query)
static int check_align_lists(const char* who, int32_t topk, int64_t n) {
    if (topk < 1 || topk > 32) return who ? fail(UMLH_E_INVALID, "%s: topk=%d outside 1..32", who, topk) : UMLH_E_INVALID;
    if (n <= topk || n > ALIGN_MAX_ROWS)
        return who ? fail(UMLH_E_INVALID, "%s: n=%lld rows for topk=%d (need topk < n <= 2^30)", who, (long long)n, topk) : UMLH_E_INVALID;
    return UMLH_OK;
}

// the list length of the k-NN probe and the class-wise report; 0 = fine
static int check_list_k(const char* who, int32_t k) {
    if (k < 1 || k > LIST_MAX_K) return fail(UMLH_E_INVALID, "%s: k=%d outside 1..%d", who, k, LIST_MAX_K);
    return UMLH_OK;
}

// ---- bf16 shadow of a feature table ----
int umlh_to_bf16(const float* src, void* dst, int64_t n, void* stream) {
    if (!src || !dst || n < 0) return fail(UMLH_E_INVALID, "umlh_to_bf16: bad arguments");
    HIPCHK(umlh_launch_to_bf16(src, dst, n, (hipStream_t)stream), "to_bf16");
    return UMLH_OK;
}

// ---- MultiBench critics: next-step MSE decoder, InfoNCE (kernels: umlh_kernels_seq.hip) ----
int umlh_seq_mse_forward(const float* z, const float* w, const float* bias, const float* x, const int64_t* lengths, int32_t B,
                         int32_t T, int32_t Z, int32_t D, float* recon, float* dres, float* row_partial, float* loss_cnt,
                         void* stream) {
    if (!z || !w || !bias || !x || !dres || !row_partial || !loss_cnt) return fail(UMLH_E_INVALID, "umlh_seq_mse_forward: null buffer");
    if (B < 1 || T < 1 || Z < 1 || D < 1 || Z > 8192) return fail(UMLH_E_INVALID, "umlh_seq_mse_forward: bad shape B=%d T=%d Z=%d D=%d", B, T, Z, D);
    HIPCHK(umlh_seq_launch_fwd(z, w, bias, x, lengths, B, T, Z, D, recon, dres, row_partial, loss_cnt, (hipStream_t)stream), "seq fwd");
    return UMLH_OK;
}

// the decoder gradient dW [D,Z] over R = B*T rows: splits_for(D, Z, R) slabs and row_chunk(R) rows per db partial, the encoder layers' rule
uint64_t umlh_seq_mse_backward_scratch_floats(int32_t B, int32_t T, int32_t Z, int32_t D) {
    if (B < 1 || T < 1 || Z < 1 || D < 1) return 0;
    const int R = B * T, chunk = row_chunk(R);
    return (uint64_t)splits_for(D, Z, R) * D * Z + (uint64_t)((R + chunk - 1) / chunk) * D + 64;
}

int umlh_seq_mse_backward(const float* z, const float* w, const float* dres, const float* loss_cnt, const float* grad_out,
                          int32_t B, int32_t T, int32_t Z, int32_t D, float* dz, float* dw, float* db, float* scratch, void* stream) {
    if (!z || !w || !dres || !loss_cnt || !grad_out || !dz || !dw || !db) return fail(UMLH_E_INVALID, "umlh_seq_mse_backward: null buffer");
    if (B < 1 || T < 1 || Z < 1 || D < 1 || D > 8192) return fail(UMLH_E_INVALID, "umlh_seq_mse_backward: bad shape");
    hipStream_t st = (hipStream_t)stream;
    const int R = B * T, sp = splits_for(D, Z, R);
    if (!scratch || sp == 1) {
        // without slab memory a planned split becomes a chain of launches over the same row chunks (umlh_seq_launch_bwd)
        const int dw_chunk = sp > 1 ? (int)round_up((R + sp - 1) / sp, KT) : 0;
        HIPCHK(umlh_seq_launch_bwd(z, w, dres, loss_cnt, grad_out, B, T, Z, D, dz, dw, db, 1, dw_chunk, st), "seq bwd");
        return UMLH_OK;
    }
    // dz as before; dW[d][k] = s * sum_r dres[r][d] z[r][k] as split-K slabs, db[d] = s * sum_r dres[r][d] as row-chunk partials,
    // both summed and scaled (s = 2 * grad_out / denominator, device-side) by one multi-reduce
    HIPCHK(umlh_seq_launch_bwd(z, w, dres, loss_cnt, grad_out, B, T, Z, D, dz, dw, db, 0, 0, st), "seq bwd (dz)");
    const int chunk = row_chunk(R), nr = (R + chunk - 1) / chunk;
    float* slabs = scratch;
    float* part = scratch + (size_t)sp * D * Z;
    int ns = 1;
    RC(umlh_gemm_f32_epi(dres, z, nullptr, D, Z, R, D, Z, 1, 1, nullptr, sp, slabs, 1, &ns, st));
    HIPCHK(umlh_enc_launch_colsum_partial(dres, R, D, chunk, part, st), "seq bwd (db partials)");
    MultiReduceArgs red;
    memset(&red, 0, sizeof(red));
    red.d[0] = ReduceDesc{slabs, dw, (long long)D * Z, (long long)D * Z, ns, 0};
    red.d[1] = ReduceDesc{part, db, (long long)D, (long long)D, nr, 0};
    red.count = 2;
    red.s_num = grad_out; red.s_den = loss_cnt + 1; red.s_mul = 2.f;
    HIPCHK(umlh_enc_launch_multi_reduce(&red, st), "seq bwd (reduce)");
    return UMLH_OK;
}

// SequenceInfoNCELoss (MultiBench/models.py:145-175) over n valid rows
int umlh_infonce_forward(const float* pred, const float* target, int32_t n, int32_t D, float temperature, float* pred_hat,
                         float* target_hat, float* pred_norm, float* probs, float* row_loss, float* loss, void* stream) {
    if (!pred || !target || !pred_hat || !target_hat || !pred_norm || !probs || !row_loss || !loss)
        return fail(UMLH_E_INVALID, "umlh_infonce_forward: null buffer");
    if (n < 1 || D < 1 || !(temperature > 0.f)) return fail(UMLH_E_INVALID, "umlh_infonce_forward: bad shape (n=%d D=%d)", n, D);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(umlh_seq_launch_l2norm(pred, n, D, pred_hat, pred_norm, st), "infonce l2norm(pred)");
    HIPCHK(umlh_seq_launch_l2norm(target, n, D, target_hat, row_loss, st), "infonce l2norm(target)");   // (row_loss: scratch for the unused norms)
    int ns = 1;
    RC(umlh_gemm_f32_epi(pred_hat, target_hat, probs, n, n, D, D, D, 0, 0, nullptr, 1, nullptr, 0, &ns, st));
    HIPCHK(umlh_seq_launch_nce_rows(probs, n, 1.f / temperature, row_loss, loss, st), "infonce rows");
    return UMLH_OK;
}

int umlh_infonce_backward(const float* pred_hat, const float* target_hat, const float* pred_norm, const float* probs,
                          const float* grad_out, int32_t n, int32_t D, float temperature, float* dhat, float* dpred, void* stream) {
    if (!pred_hat || !target_hat || !pred_norm || !probs || !grad_out || !dhat || !dpred)
        return fail(UMLH_E_INVALID, "umlh_infonce_backward: null buffer");
    if (n < 1 || D < 1 || !(temperature > 0.f)) return fail(UMLH_E_INVALID, "umlh_infonce_backward: bad shape");
    hipStream_t st = (hipStream_t)stream;
    int ns = 1;
    RC(umlh_gemm_f32_epi(probs, target_hat, dhat, n, D, n, n, D, 0, 1, nullptr, 1, nullptr, 0, &ns, st));   // dhat = (softmax - I) target_hat
    HIPCHK(umlh_seq_launch_l2norm_bwd(dhat, pred_hat, pred_norm, grad_out, 1.f / ((float)n * temperature), n, D, dpred, st), "infonce l2norm bwd");
    return UMLH_OK;
}

// ---- MultiBench shared encoder ops (kernels: umlh_kernels_enc.hip, GEMMs: gemm_f32) ----
int umlh_gemm_f32(const float* A, const float* B, float* out, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb,
                  int32_t ldo, int32_t ta, int32_t tb, const int64_t* a_rows, const int64_t* k_rows, float alpha,
                  int32_t splits, float* slabs, void* stream) {
    if (!A || !B || !out || M < 0 || N < 0 || K < 1 || (ta && a_rows) || (!tb && k_rows) || splits < 1 || (splits > 1 && !slabs))
        return fail(UMLH_E_INVALID, "umlh_gemm_f32: bad arguments");
    if ((ta == 1 && tb == 0) || ta < 0 || ta > 1 || tb < 0 || tb > 1)
        return fail(UMLH_E_INVALID, "umlh_gemm_f32: (ta, tb) = (%d, %d) unsupported (supported: (0,0), (0,1), (1,1))", ta, tb);
    if (lda < (ta ? M : K) || ldb < (tb ? N : K) || ldo < N)
        return fail(UMLH_E_INVALID, "umlh_gemm_f32: strides shorter than a row (lda=%d ldb=%d ldo=%d for M=%d N=%d K=%d ta=%d tb=%d)",
                    lda, ldb, ldo, M, N, K, ta, tb);
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.B = B; g.a_rows = a_rows; g.k_rows = k_rows;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldo = ldo;
    g.alpha = alpha; g.k_switch = K; g.k_valid1 = K;
    // dense operands and a short K range per workgroup: the latency-oriented kernel (see gemm_enc)
    const bool dense = !a_rows && !k_rows && (K + splits - 1) / splits <= 512;
    auto launch = dense ? umlh_f32_launch_gemm_enc : umlh_f32_launch_gemm;
    if (splits == 1) {
        g.out = out; g.k_chunk = K; g.slab_stride = 0;
        HIPCHK(launch(&g, ta, tb, 1, (hipStream_t)stream), "gemm_f32");
        return UMLH_OK;
    }
    const int chunk = (int)round_up((K + splits - 1) / splits, KT);
    const int ns = (K + chunk - 1) / chunk;
    g.out = slabs; g.k_chunk = chunk; g.slab_stride = (long long)M * ldo;
    HIPCHK(launch(&g, ta, tb, ns, (hipStream_t)stream), "gemm_f32 (split-K)");
    HIPCHK(umlh_enc_launch_reduce_slabs(slabs, ns, g.slab_stride, M, N, ldo, nullptr, out, (hipStream_t)stream), "split-K reduce");
    return UMLH_OK;
}

int umlh_gemm_f32_epi(const float* A, const float* B, float* out, int M, int N, int K, int lda, int ldb, int ta, int tb,
                      const Epilogue* epi, int splits, float* slabs, int defer, int* ns_out, hipStream_t stream) {
    if (!A || !B || M < 1 || N < 1 || K < 1 || splits < 1 || ((defer || splits > 1) && !slabs) || (!defer && !out))
        return fail(UMLH_E_INVALID, "gemm_f32 (epilogue): bad arguments");
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.B = B; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldo = N;
    g.alpha = 1.f; g.k_switch = K; g.k_valid1 = K;
    const int chunk = splits == 1 ? K : (int)round_up((K + splits - 1) / splits, KT);
    const int ns = (K + chunk - 1) / chunk;
    g.k_chunk = chunk;
    g.slab_stride = (long long)M * N;
    if (ns_out) *ns_out = ns;
    if (!defer && ns == 1) {
        g.out = out;
        if (epi) g.epi = *epi;
        HIPCHK(umlh_f32_launch_gemm_enc(&g, ta, tb, 1, stream), "gemm_enc (epilogue)");
        return UMLH_OK;
    }
    g.out = slabs;
    HIPCHK(umlh_f32_launch_gemm_enc(&g, ta, tb, ns, stream), "gemm_enc (slabs)");
    if (defer) return UMLH_OK;
    HIPCHK(umlh_enc_launch_reduce_slabs(slabs, ns, g.slab_stride, M, N, N, epi, out, stream), "split-K reduce (epilogue)");
    return UMLH_OK;
}

int umlh_bias_act(float* y, const float* bias, int64_t M, int32_t N, int32_t relu, void* stream) {
    if (!y || M < 0 || N < 1) return fail(UMLH_E_INVALID, "umlh_bias_act: bad arguments");
    HIPCHK(umlh_enc_launch_bias_act(y, bias, M, N, relu, (hipStream_t)stream), "bias_act");
    return UMLH_OK;
}

int umlh_relu_backward(const float* y, float* dy, int64_t n, void* stream) {
    if (!y || !dy || n < 0) return fail(UMLH_E_INVALID, "umlh_relu_backward: bad arguments");
    HIPCHK(umlh_enc_launch_relu_bwd(y, dy, n, (hipStream_t)stream), "relu_bwd");
    return UMLH_OK;
}

int umlh_dropout(float* x, int64_t n, float p, uint64_t seed, void* stream) {
    if (!x || n < 0 || !(p >= 0.f && p < 1.f)) return fail(UMLH_E_INVALID, "umlh_dropout: bad arguments");
    HIPCHK(umlh_enc_launch_dropout(x, n, p, seed, (hipStream_t)stream), "dropout");
    return UMLH_OK;
}

int umlh_add_inplace(float* y, const float* x, int64_t n, void* stream) {
    if (!y || !x || n < 0) return fail(UMLH_E_INVALID, "umlh_add_inplace: bad arguments");
    HIPCHK(umlh_enc_launch_add_inplace(y, x, n, (hipStream_t)stream), "add_inplace");
    return UMLH_OK;
}

int umlh_colsum(const float* x, int32_t M, int32_t N, float* out, void* stream) {
    if (!x || !out || M < 0 || N < 1) return fail(UMLH_E_INVALID, "umlh_colsum: bad arguments");
    HIPCHK(umlh_enc_launch_colsum(x, M, N, out, (hipStream_t)stream), "colsum");
    return UMLH_OK;
}

int umlh_add_layernorm_forward(const float* x, const float* r, const float* gamma, const float* beta, int32_t M, int32_t N,
                               float eps, float* s, float* y, float* mean, float* rstd, void* stream) {
    if (!x || !gamma || !beta || !s || !y || !mean || !rstd || M < 0 || N < 1)
        return fail(UMLH_E_INVALID, "umlh_add_layernorm_forward: bad arguments");
    HIPCHK(umlh_enc_launch_add_layernorm(x, r, gamma, beta, M, N, eps, s, y, mean, rstd, (hipStream_t)stream), "add_layernorm");
    return UMLH_OK;
}

int umlh_layernorm_backward(const float* dy, const float* s, const float* gamma, const float* mean, const float* rstd,
                            int32_t M, int32_t N, float* ds, float* dgamma, float* dbeta, void* stream) {
    if (!dy || !s || !gamma || !mean || !rstd || !ds || !dgamma || !dbeta || M < 0 || N < 1)
        return fail(UMLH_E_INVALID, "umlh_layernorm_backward: bad arguments");
    HIPCHK(umlh_enc_launch_layernorm_bwd(dy, s, gamma, mean, rstd, M, N, ds, dgamma, dbeta, (hipStream_t)stream), "layernorm_bwd");
    return UMLH_OK;
}

int umlh_add_positions(float* x, const float* pos, int32_t T, int32_t B, int32_t Z, void* stream) {
    if (!x || !pos || T < 1 || B < 1 || Z < 1) return fail(UMLH_E_INVALID, "umlh_add_positions: bad arguments");
    HIPCHK(umlh_enc_launch_add_pos(x, pos, T, B, Z, (hipStream_t)stream), "add_pos");
    return UMLH_OK;
}

int umlh_positions_backward(const float* dx, int32_t T, int32_t B, int32_t Z, float* dpos, void* stream) {
    if (!dx || !dpos || T < 1 || B < 1 || Z < 1) return fail(UMLH_E_INVALID, "umlh_positions_backward: bad arguments");
    HIPCHK(umlh_enc_launch_pos_grad(dx, T, B, Z, dpos, (hipStream_t)stream), "pos_grad");
    return UMLH_OK;
}

int umlh_gather_rows(const float* x, const int64_t* idx, int32_t n, int32_t Z, float* out, int32_t scatter, void* stream) {
    if (!x || !idx || !out || n < 0 || Z < 1) return fail(UMLH_E_INVALID, "umlh_gather_rows: bad arguments");
    HIPCHK(umlh_enc_launch_gather_rows(x, idx, n, Z, out, scatter, (hipStream_t)stream), "gather_rows");
    return UMLH_OK;
}

int umlh_attention_forward(const float* qkv, const int64_t* lengths, int32_t T, int32_t B, int32_t Z, int32_t H, float p,
                           uint64_t seed, float* ctx, float* lse, void* stream) {
    if (!qkv || !ctx || !lse || B < 1 || !(p >= 0.f && p < 1.f)) return fail(UMLH_E_INVALID, "umlh_attention_forward: bad arguments");
    if (T < 1 || T > 128 || H < 1 || Z % H != 0 || Z / H > 64)
        return fail(UMLH_E_INVALID, "umlh_attention_forward: T=%d Z=%d H=%d outside the kernel's envelope (T <= 128, Z/H <= 64)", T, Z, H);
    HIPCHK(umlh_enc_launch_attention_fwd(qkv, lengths, T, B, Z, H, p, seed, nullptr, ctx, lse, (hipStream_t)stream), "attention_fwd");
    return UMLH_OK;
}

int umlh_attention_backward(const float* qkv, const int64_t* lengths, const float* lse, const float* dctx, int32_t T, int32_t B,
                            int32_t Z, int32_t H, float p, uint64_t seed, float* dqkv, void* stream) {
    if (!qkv || !lse || !dctx || !dqkv || B < 1 || !(p >= 0.f && p < 1.f))
        return fail(UMLH_E_INVALID, "umlh_attention_backward: bad arguments");
    if (T < 1 || T > 128 || H < 1 || Z % H != 0 || Z / H > 64)
        return fail(UMLH_E_INVALID, "umlh_attention_backward: T=%d Z=%d H=%d outside the kernel's envelope", T, Z, H);
    HIPCHK(umlh_enc_launch_attention_bwd(qkv, lengths, lse, dctx, T, B, Z, H, p, seed, nullptr, dqkv, (hipStream_t)stream), "attention_bwd");
    return UMLH_OK;
}

// ---- permutation, standalone optimizer (kernels: umlh_kernels_f32.hip) ----
int umlh_random_permutation(int64_t n, uint64_t seed, int64_t* out, void* stream) {
    if (n < 0 || (n > 0 && !out)) return fail(UMLH_E_INVALID, "umlh_random_permutation: bad arguments");
    HIPCHK(umlh_launch_feistel_perm(n, seed, ll(out), (hipStream_t)stream), "feistel perm");
    return UMLH_OK;
}

// the spans of one modality of umlh_index_block; 0 = fine, *total = ids they write
static int check_index_spans(const char* who, const char* side, const umlh_index_span_t* spans, int32_t n_spans, const int64_t* out,
                             int64_t* total) {
    *total = 0;
    if (n_spans < 0 || (n_spans > 0 && !spans)) return fail(UMLH_E_INVALID, "%s: %s: %d spans without a span array", who, side, n_spans);
    for (int i = 0; i < n_spans; ++i) {
        const umlh_index_span_t& s = spans[i];
        if (s.kind < UMLH_SPAN_FEISTEL || s.kind > UMLH_SPAN_IOTA) return fail(UMLH_E_INVALID, "%s: %s span %d: unknown kind %d", who, side, i, s.kind);
        if (s.n < 0 || s.start < 0 || s.count < 0 || s.start > s.n || s.count > s.n - s.start)
            return fail(UMLH_E_INVALID, "%s: %s span %d: start=%lld count=%lld outside an order of n=%lld rows", who, side, i,
                        (long long)s.start, (long long)s.count, (long long)s.n);
        if (s.kind == UMLH_SPAN_FEISTEL && s.n > ((int64_t)1 << 62))
            return fail(UMLH_E_INVALID, "%s: %s span %d: n=%lld rows (a Feistel order holds at most 2^62)", who, side, i, (long long)s.n);
        if (s.kind == UMLH_SPAN_TABLE && s.count > 0 && !s.order) return fail(UMLH_E_INVALID, "%s: %s span %d: a TABLE span needs its order", who, side, i);
        *total += s.count;
        if (*total >= ROWS_END) return fail(UMLH_E_INVALID, "%s: %s: more than 2^31 - 1 ids in one block", who, side);
    }
    if (*total > 0 && !out) return fail(UMLH_E_INVALID, "%s: %s: %lld ids and no destination", who, side, (long long)*total);
    return UMLH_OK;
}

int umlh_index_block(const umlh_index_span_t* img_spans, int32_t n_img_spans, int64_t* img_out, const umlh_index_span_t* txt_spans,
                     int32_t n_txt_spans, int64_t* txt_out, void* stream) {
    const char* who = "umlh_index_block";
    int64_t total_img = 0, total_txt = 0;
    RC(check_index_spans(who, "image", img_spans, n_img_spans, img_out, &total_img));
    RC(check_index_spans(who, "text", txt_spans, n_txt_spans, txt_out, &total_txt));
    // descriptors travel by value, UMLH_INDEX_SPANS_MAX per launch: image spans first, then text, each modality back to back
    IndexBlockArgs a;
    memset(&a, 0, sizeof(a));
    const umlh_index_span_t* side[2] = {img_spans, txt_spans};
    const int32_t n_side[2] = {n_img_spans, n_txt_spans};
    int64_t* dst_side[2] = {img_out, txt_out};
    for (int m = 0; m < 2; ++m) {
        long long* dst = ll(dst_side[m]);
        for (int i = 0; i < n_side[m]; ++i) {
            const umlh_index_span_t& s = side[m][i];
            if (s.count == 0) continue;
            a.s[a.count++] = IndexSpanDesc{ll(s.order), dst, s.n, s.seed, s.start, s.count, s.kind, 0, 0, 0};
            dst += s.count;
            if (a.count == UMLH_INDEX_SPANS_MAX) {
                HIPCHK(umlh_launch_index_block(&a, (hipStream_t)stream), who);
                a.count = 0;
            }
        }
    }
    if (a.count > 0) HIPCHK(umlh_launch_index_block(&a, (hipStream_t)stream), who);
    return UMLH_OK;
}

// the step's optimizer constants from loose hyper-parameters
static OptArgs standalone_opt(int32_t optimizer, double lr, int64_t step, double beta1, double beta2, double eps, double momentum,
                              double weight_decay) {
    umlh_config_t c;
    memset(&c, 0, sizeof(c));
    c.optimizer = optimizer; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps; c.momentum = momentum; c.weight_decay = weight_decay;
    umlh_hyper_t hy;
    memset(&hy, 0, sizeof(hy));
    hy.lr = lr; hy.step = step;
    return make_opt(c, hy);
}

int umlh_optimizer_step(int32_t optimizer, float* param, const float* grad, float* m, float* v, int64_t n, double lr,
                        int64_t step, double beta1, double beta2, double eps, double momentum, double weight_decay,
                        void* stream) {
    if (optimizer < UMLH_OPT_SGD || optimizer > UMLH_OPT_ADAMW)
        return fail(UMLH_E_INVALID, "umlh_optimizer_step: unknown optimizer %d", optimizer);
    if (!param || !grad || !m || (optimizer != UMLH_OPT_SGD && !v) || n < 0)
        return fail(UMLH_E_INVALID, "umlh_optimizer_step: null buffer");
    const OptArgs o = standalone_opt(optimizer, lr, step, beta1, beta2, eps, momentum, weight_decay);
    // reduce_update picks its float4 path from n alone and moves 16 bytes per access.  A base that is not 16-byte aligned (a view
    // at an odd element offset; a block of torch's allocator never is) takes the element-wise kernel of the multi-tensor entry.
    const uintptr_t bases = reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(m) |
                            (optimizer != UMLH_OPT_SGD ? reinterpret_cast<uintptr_t>(v) : 0);
    if (bases & 15) {
        float* const pp[1] = {param};
        const float* const gg[1] = {grad};
        float* const mm[1] = {m};
        float* const vv[1] = {v};
        const long long cnt = n;
        HIPCHK(umlh_launch_multi_opt(1, pp, gg, mm, vv, &cnt, &o, (hipStream_t)stream), "optimizer step (unaligned base)");
        return UMLH_OK;
    }
    HIPCHK(umlh_launch_reduce_update(1, grad, 1, n, n, nullptr, param, m, v, &o, 0, 0, (hipStream_t)stream),
           "optimizer step");
    return UMLH_OK;
}

int umlh_optimizer_step_multi(int32_t optimizer, int32_t n_tensors, float* const* params, const float* const* grads, float* const* m,
                              float* const* v, const int64_t* n, double lr, int64_t step, double beta1, double beta2, double eps,
                              double momentum, double weight_decay, void* stream) {
    if (optimizer < UMLH_OPT_SGD || optimizer > UMLH_OPT_ADAMW) return fail(UMLH_E_INVALID, "umlh_optimizer_step_multi: unknown optimizer %d", optimizer);
    if (n_tensors < 0 || (n_tensors > 0 && (!params || !grads || !m || !n || (optimizer != UMLH_OPT_SGD && !v))))
        return fail(UMLH_E_INVALID, "umlh_optimizer_step_multi: null argument");
    const OptArgs o = standalone_opt(optimizer, lr, step, beta1, beta2, eps, momentum, weight_decay);
    for (int t0 = 0; t0 < n_tensors; t0 += UMLH_MULTI_OPT_MAX) {
        const int k = n_tensors - t0 < UMLH_MULTI_OPT_MAX ? n_tensors - t0 : UMLH_MULTI_OPT_MAX;
        long long cnt[UMLH_MULTI_OPT_MAX];
        for (int i = 0; i < k; ++i) {
            if (!params[t0 + i] || !grads[t0 + i] || !m[t0 + i] || n[t0 + i] < 0 || (optimizer != UMLH_OPT_SGD && !v[t0 + i]))
                return fail(UMLH_E_INVALID, "umlh_optimizer_step_multi: tensor %d has a null buffer", t0 + i);
            cnt[i] = n[t0 + i];
        }
        HIPCHK(umlh_launch_multi_opt(k, params + t0, grads + t0, m + t0, v ? v + t0 : nullptr, cnt, &o, (hipStream_t)stream), "optimizer step (multi)");
    }
    return UMLH_OK;
}

// ---- alignment metrics (kernels: umlh_kernels_align.hip) ----
uint64_t umlh_align_scratch_bytes(int64_t n, int32_t d_a, int32_t d_b, int32_t topk, int32_t splits) {
    if (n < 1 || n > ALIGN_MAX_ROWS || d_a < 1 || d_b < 1 || topk < 0 || topk > 32 || (topk > 0 && topk >= n) || splits < 0) return 0;
    uint64_t b = umlh_align_cka_bytes(n, d_a, d_b, splits);
    const uint64_t m = umlh_align_mutual_bytes(n);
    if (m > b) b = m;
    if (topk > 0) {
        const uint64_t k = umlh_align_knn_bytes(n, topk, splits);
        if (k > b) b = k;
    }
    return b;
}

int umlh_align_knn(const float* x, int64_t n, int32_t d, int32_t ldx, int32_t topk, int32_t splits, int32_t* knn,
                   float* scores, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_align_knn";
    if (!x || !knn || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (x, knn and scratch are required)", who);
    RC(check_align_lists(who, topk, n));
    if (d < 1 || ldx < d) return fail(UMLH_E_INVALID, "%s: d=%d ldx=%d (need 1 <= d <= ldx)", who, d, ldx);
    if (splits < 0) return fail(UMLH_E_INVALID, "%s: splits=%d < 0", who, splits);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_align_knn_bytes(n, topk, splits), 0));
    HIPCHK(umlh_align_launch_knn(x, n, d, ldx, topk, splits, knn, scores, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_align_mutual_knn(const int32_t* knn_a, const int32_t* knn_b, int64_t n, int32_t topk, double* out, void* scratch,
                          uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_align_mutual_knn";
    if (!knn_a || !knn_b || !out || !scratch)
        return fail(UMLH_E_INVALID, "%s: null pointer (knn_a, knn_b, out and scratch are required)", who);
    RC(check_align_lists(who, topk, n));
    RC(check_scratch(who, scratch, scratch_bytes, umlh_align_mutual_bytes(n), 0));
    HIPCHK(umlh_align_launch_mutual(knn_a, knn_b, n, topk, out, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// the shape checks of one feature pair, shared by the CKA forms and the members of umlh_align_pairs (who: the function, or the
// function and the member; NULL: no message, a size query); 0 = fine
static int check_pair_shape(const char* who, int32_t lda, int32_t d_a, int32_t ldb, int32_t d_b, int64_t n, int32_t unbiased, int32_t splits) {
    if (d_a < 1 || d_b < 1 || lda < d_a || ldb < d_b)
        return who ? fail(UMLH_E_INVALID, "%s: d_a=%d lda=%d d_b=%d ldb=%d (need 1 <= d <= ld)", who, d_a, lda, d_b, ldb) : UMLH_E_INVALID;
    if (n < 1 || n > ALIGN_MAX_ROWS)
        return who ? fail(UMLH_E_INVALID, "%s: n=%lld rows (need 1 <= n <= 2^30)", who, (long long)n) : UMLH_E_INVALID;
    if (unbiased && n < 4)
        return who ? fail(UMLH_E_INVALID, "%s: n=%lld rows, the unbiased HSIC divides by n - 3 (need n >= 4)", who, (long long)n)
                   : UMLH_E_INVALID;
    if (splits < 0) return who ? fail(UMLH_E_INVALID, "%s: splits=%d < 0", who, splits) : UMLH_E_INVALID;
    return UMLH_OK;
}

// the shared checks of the feature-space CKA forms; 0 = fine
static int check_cka(const char* who, const float* a, int32_t lda, int32_t d_a, const float* b, int32_t ldb, int32_t d_b, int64_t n,
                     int32_t unbiased, int32_t splits, const double* out4, const void* scratch) {
    if (!a || !b || !out4 || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (a, b, out4 and scratch are required)", who);
    return check_pair_shape(who, lda, d_a, ldb, d_b, n, unbiased, splits);
}

int umlh_align_cka(const float* a, int32_t lda, int32_t d_a, const float* b, int32_t ldb, int32_t d_b, int64_t n,
                   int32_t splits, double* out4, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_align_cka";
    RC(check_cka(who, a, lda, d_a, b, ldb, d_b, n, 0, splits, out4, scratch));
    RC(check_scratch(who, scratch, scratch_bytes, umlh_align_cka_bytes(n, d_a, d_b, splits), 0));
    HIPCHK(umlh_align_launch_cka(a, lda, d_a, b, ldb, d_b, n, splits, out4, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- grouped form: many pairs in one fixed train of launches ----
// what one member is held to: the pair's shape as umlh_align_cka holds it, the list length as umlh_align_knn does.  who = NULL:
// the size query, which runs the same shape checks without a message and does not look at the pointers
static int check_align_member(const char* who, const umlh_align_pair_t& it, int32_t splits) {
    if (who && (!it.a || !it.b || !it.out5))
        return fail(UMLH_E_INVALID, "%s: null pointer (%s is required)", who, !it.a ? "a" : !it.b ? "b" : "out5");
    if (!it.cka && !it.topk) return who ? fail(UMLH_E_INVALID, "%s: cka=0 and topk=0 ask for nothing", who) : UMLH_E_INVALID;
    RC(check_pair_shape(who, it.lda, it.d_a, it.ldb, it.d_b, it.n, 0, splits));
    if (it.topk != 0) RC(check_align_lists(who, it.topk, it.n));
    return UMLH_OK;
}

static int check_align_group_count(const char* who, const void* items, int32_t n_items, int32_t splits) {
    if (!items) return who ? fail(UMLH_E_INVALID, "%s: items is NULL", who) : UMLH_E_INVALID;
    if (n_items < 1 || n_items > UMLH_ALIGN_MAX_PAIRS)
        return who ? fail(UMLH_E_INVALID, "%s: n_items=%d outside 1..%d", who, n_items, UMLH_ALIGN_MAX_PAIRS) : UMLH_E_INVALID;
    if (splits < 0) return who ? fail(UMLH_E_INVALID, "%s: splits=%d < 0", who, splits) : UMLH_E_INVALID;
    return UMLH_OK;
}

// no output pointer occurs twice among the members: every member's workgroups write while the others' run
static int check_align_group_unique(const char* who, const umlh_align_pair_t* items, int32_t n_items) {
    static const char* const NAMES[5] = {"out5", "knn_a", "knn_b", "scores_a", "scores_b"};
    struct Ref { const void* p; int member, field; };
    std::vector<Ref> refs;
    refs.reserve((size_t)n_items * 5);
    for (int i = 0; i < n_items; ++i) {
        const void* out[5] = {items[i].out5, items[i].knn_a, items[i].knn_b, items[i].scores_a, items[i].scores_b};
        for (int k = 0; k < 5; ++k)
            if (out[k] && (k == 0 || items[i].topk != 0)) refs.push_back({out[k], i, k});
    }
    std::sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) {
        return a.p != b.p ? std::less<const void*>()(a.p, b.p) : a.member != b.member ? a.member < b.member : a.field < b.field;
    });
    for (size_t i = 1; i < refs.size(); ++i)
        if (refs[i].p == refs[i - 1].p)
            return fail(UMLH_E_INVALID, "%s: member %d: %s is also member %d's %s (members may not share output buffers)", who,
                        refs[i].member, NAMES[refs[i].field], refs[i - 1].member, NAMES[refs[i - 1].field]);
    return UMLH_OK;
}

uint64_t umlh_align_pairs_scratch(const umlh_align_pair_t* items, int32_t n_items, int32_t splits) {
    if (check_align_group_count(nullptr, items, n_items, splits)) return 0;
    for (int i = 0; i < n_items; ++i)
        if (check_align_member(nullptr, items[i], splits)) return 0;
    return umlh_align_pairs_bytes(items, n_items, splits);
}

int umlh_align_pairs(const umlh_align_pair_t* items, int32_t n_items, int32_t splits, void* scratch, uint64_t scratch_bytes,
                     void* stream) {
    const char* who = "umlh_align_pairs";
    RC(check_align_group_count(who, items, n_items, splits));
    char member[64];
    for (int i = 0; i < n_items; ++i) {
        snprintf(member, sizeof(member), "%s: member %d", who, i);
        RC(check_align_member(member, items[i], splits));
    }
    RC(check_align_group_unique(who, items, n_items));
    if (!scratch) return fail(UMLH_E_INVALID, "%s: scratch is NULL", who);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_align_pairs_bytes(items, n_items, splits), 8));
    HIPCHK(umlh_align_launch_pairs(items, n_items, splits, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- the other alignment metrics (kernels: umlh_kernels_align_ext.hip) ----
static bool align_topk_ok(int64_t n, int32_t topk, int32_t lo) { return topk >= lo && topk <= 32 && topk < n && n <= ALIGN_MAX_ROWS; }

uint64_t umlh_align_ext_scratch_bytes(int32_t kind, int64_t n, int32_t d_a, int32_t d_b, int32_t topk, int32_t splits) {
    if (n < 1 || n > ALIGN_MAX_ROWS) return 0;
    switch (kind) {
    case UMLH_ALIGN_CKA_UNBIASED:
        return (n < 4 || d_a < 1 || d_b < 1 || splits < 0) ? 0 : umlh_align_ext_cka_unbiased_bytes(n, d_a, d_b, splits);
    case UMLH_ALIGN_CKA_RBF:
        return (d_a < 1 || d_b < 1 || splits < 0) ? 0 : umlh_align_ext_rbf_bytes(n, d_a, d_b, splits);
    case UMLH_ALIGN_CKNNA:
        return (n < 4 || !align_topk_ok(n, topk, 2)) ? 0 : umlh_align_ext_cknna_bytes(n);
    case UMLH_ALIGN_LIST_STATS:
        return !align_topk_ok(n, topk, 1) ? 0 : umlh_align_ext_list_bytes(n);
    }
    return 0;
}

int umlh_align_cka_unbiased(const float* a, int32_t lda, int32_t d_a, const float* b, int32_t ldb, int32_t d_b, int64_t n,
                            int32_t splits, double* out4, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_align_cka_unbiased";
    RC(check_cka(who, a, lda, d_a, b, ldb, d_b, n, 1, splits, out4, scratch));
    RC(check_scratch(who, scratch, scratch_bytes, umlh_align_ext_cka_unbiased_bytes(n, d_a, d_b, splits), 0));
    HIPCHK(umlh_align_ext_launch_cka_unbiased(a, lda, d_a, b, ldb, d_b, n, splits, out4, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_align_cka_rbf(const float* a, int32_t lda, int32_t d_a, const float* b, int32_t ldb, int32_t d_b, int64_t n, double sigma,
                       int32_t unbiased, int32_t splits, double* out4, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_align_cka_rbf";
    RC(check_cka(who, a, lda, d_a, b, ldb, d_b, n, unbiased, splits, out4, scratch));
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(UMLH_E_INVALID, "%s: sigma=%g (need a finite sigma > 0)", who, sigma);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_align_ext_rbf_bytes(n, d_a, d_b, splits), 0));
    HIPCHK(umlh_align_ext_launch_rbf(a, lda, d_a, b, ldb, d_b, n, sigma, unbiased ? 1 : 0, splits, out4, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_align_cknna(const int32_t* knn_a, const float* scores_a, const int32_t* knn_b, const float* scores_b, int64_t n, int32_t topk,
                     double* out4, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_align_cknna";
    if (!knn_a || !scores_a || !knn_b || !scores_b || !out4 || !scratch)
        return fail(UMLH_E_INVALID, "%s: null pointer (both lists, both scores, out4 and scratch are required)", who);
    if (topk < 2) return fail(UMLH_E_INVALID, "%s: CKNNA requires topk >= 2 (topk=%d)", who, topk);
    if (topk > 32) return fail(UMLH_E_INVALID, "%s: topk=%d outside 2..32", who, topk);
    if (n <= topk || n < 4 || n > ALIGN_MAX_ROWS)
        return fail(UMLH_E_INVALID, "%s: n=%lld rows for topk=%d (need topk < n, 4 <= n <= 2^30)", who, (long long)n, topk);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_align_ext_cknna_bytes(n), 0));
    HIPCHK(umlh_align_ext_launch_cknna(knn_a, scores_a, knn_b, scores_b, n, topk, out4, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_align_list_stats(const int32_t* knn_a, const int32_t* knn_b, int64_t n, int32_t topk, int32_t* rows, double* out3,
                          void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_align_list_stats";
    if (!knn_a || !knn_b || !out3 || !scratch)
        return fail(UMLH_E_INVALID, "%s: null pointer (knn_a, knn_b, out3 and scratch are required)", who);
    RC(check_align_lists(who, topk, n));
    RC(check_scratch(who, scratch, scratch_bytes, umlh_align_ext_list_bytes(n), 0));
    HIPCHK(umlh_align_ext_launch_list_stats(knn_a, knn_b, n, topk, rows, out3, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- linear probes (kernels: umlh_kernels_probe.hip) ----
static const int PROBE_MAX_D = 1024, PROBE_MAX_ITER = 1000;
static bool probe_shape_ok(int64_t n, int32_t d, int32_t ldx, int64_t n_min = 2) {
    return n >= n_min && n < ROWS_END && d >= 1 && d <= PROBE_MAX_D && ldx >= d;
}

int umlh_masked_mean(const float* z, int32_t b, int32_t t_len, int32_t zdim, int64_t ldb, int64_t ldt, const int64_t* lengths,
                     float* out, int32_t ldo, void* stream) {
    if (!z || !out) return fail(UMLH_E_INVALID, "umlh_masked_mean: null pointer (z and out are required)");
    if (b < 1 || t_len < 1 || zdim < 1) return fail(UMLH_E_INVALID, "umlh_masked_mean: b=%d t_len=%d zdim=%d (need all >= 1)", b, t_len, zdim);
    if (ldb < zdim || ldt < zdim || ldo < zdim)
        return fail(UMLH_E_INVALID, "umlh_masked_mean: ldb=%lld ldt=%lld ldo=%d (need every stride >= zdim=%d)", (long long)ldb, (long long)ldt, ldo, zdim);
    HIPCHK(umlh_probe_launch_masked_mean(z, b, t_len, zdim, ldb, ldt, ll(lengths), out, ldo, (hipStream_t)stream), "umlh_masked_mean");
    return UMLH_OK;
}

uint64_t umlh_probe_scratch_bytes(int64_t n, int32_t d, int32_t max_iter) {
    if (!probe_shape_ok(n, d, d) || max_iter < 0 || max_iter > PROBE_MAX_ITER) return 0;
    return max_iter == 0 ? umlh_probe_stats_bytes(d) : umlh_probe_fit_bytes(n, d, max_iter);
}

int umlh_probe_column_stats(const float* x, int64_t n, int32_t d, int32_t ldx, double* stats, void* scratch, uint64_t scratch_bytes,
                            void* stream) {
    const char* who = "umlh_probe_column_stats";
    if (!x || !stats || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (x, stats and scratch are required)", who);
    if (!probe_shape_ok(n, d, ldx))
        return fail(UMLH_E_INVALID, "%s: n=%lld d=%d ldx=%d (need 2 <= n < 2^31, 1 <= d <= 1024, ldx >= d)", who, (long long)n, d, ldx);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_probe_stats_bytes(d), 0));
    HIPCHK(umlh_probe_launch_stats(x, n, d, ldx, stats, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_probe_fit(const float* x, int64_t n, int32_t d, int32_t ldx, const int32_t* y, const double* stats, int32_t kind, double c,
                   int32_t max_iter, double gtol, double* coef, umlh_probe_record_t* record, double* objectives, void* scratch,
                   uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_probe_fit";
    if (!x || !y || !coef || !record || !scratch)
        return fail(UMLH_E_INVALID, "%s: null pointer (x, y, coef, record and scratch are required)", who);
    if (!probe_shape_ok(n, d, ldx))
        return fail(UMLH_E_INVALID, "%s: n=%lld d=%d ldx=%d (need 2 <= n < 2^31, 1 <= d <= 1024, ldx >= d)", who, (long long)n, d, ldx);
    if (kind != UMLH_PROBE_LBFGS && kind != UMLH_PROBE_LIBLINEAR) return fail(UMLH_E_INVALID, "%s: kind=%d (0 = lbfgs, 1 = liblinear objective)", who, kind);
    if (!(c > 0.0) || !(c < 1e300)) return fail(UMLH_E_INVALID, "%s: c=%g (need a finite c > 0)", who, c);
    if (max_iter < 1 || max_iter > PROBE_MAX_ITER) return fail(UMLH_E_INVALID, "%s: max_iter=%d outside 1..%d", who, max_iter, PROBE_MAX_ITER);
    if (!(gtol >= 0.0)) return fail(UMLH_E_INVALID, "%s: gtol=%g (need gtol >= 0)", who, gtol);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_probe_fit_bytes(n, d, max_iter), 8));
    HIPCHK(umlh_probe_launch_fit(x, n, d, ldx, y, stats, kind, c, max_iter, gtol, coef, record, objectives, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_probe_score(const float* x, int64_t n, int32_t d, int32_t ldx, const double* stats, const double* coef, const int32_t* y,
                     int64_t* correct, float* decision, void* stream) {
    if (!x || !coef) return fail(UMLH_E_INVALID, "umlh_probe_score: null pointer (x and coef are required)");
    if (!correct && !decision) return fail(UMLH_E_INVALID, "umlh_probe_score: nothing to compute (correct and decision are both NULL)");
    if (correct && !y) return fail(UMLH_E_INVALID, "umlh_probe_score: correct needs the labels y");
    if (!probe_shape_ok(n, d, ldx, 1))
        return fail(UMLH_E_INVALID, "umlh_probe_score: n=%lld d=%d ldx=%d (need 1 <= n < 2^31, 1 <= d <= 1024, ldx >= d)", (long long)n, d, ldx);
    HIPCHK(umlh_probe_launch_score(x, n, d, ldx, stats, coef, y, ll(correct), decision, (hipStream_t)stream), "umlh_probe_score");
    return UMLH_OK;
}

// ---- multinomial logistic probe (kernels: umlh_kernels_softmax_probe.hip) ----
static const int SOFTMAX_MAX_D = 2048, SOFTMAX_MAX_CLASSES = 4096, SOFTMAX_MAX_HISTORY = 32;
static bool softmax_shape_ok(int64_t n, int32_t d, int32_t n_class) {
    return n >= 2 && d >= 1 && d <= SOFTMAX_MAX_D && n_class >= 2 && n_class <= SOFTMAX_MAX_CLASSES && n < ROWS_END && n * n_class < ROWS_END;
}

// the checks the evaluation and the fit share; 0 = fine
static int check_softmax(const char* who, const float* x, int64_t n, int32_t d, int32_t ldx, const int32_t* y, int32_t n_class, double c,
                         const float* coef, int32_t ldc, const void* scratch) {
    if (!x || !y || !coef || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (x, y, coef and scratch are required)", who);
    if (!softmax_shape_ok(n, d, n_class))
        return fail(UMLH_E_INVALID, "%s: n=%lld d=%d n_class=%d (need 2 <= n, 1 <= d <= 2048, 2 <= n_class <= 4096, n * n_class < 2^31)", who,
                    (long long)n, d, n_class);
    if (ldx < d) return fail(UMLH_E_INVALID, "%s: ldx=%d < d=%d", who, ldx, d);
    if (ldc < d + 1) return fail(UMLH_E_INVALID, "%s: ldc=%d < d + 1 = %d", who, ldc, d + 1);
    if (!(c > 0.0) || !(c < 1e300)) return fail(UMLH_E_INVALID, "%s: c=%g (need a finite c > 0)", who, c);
    return UMLH_OK;
}

uint64_t umlh_softmax_probe_scratch_bytes(int64_t n, int32_t d, int32_t n_class, int32_t max_iter, int32_t history) {
    if (!softmax_shape_ok(n, d, n_class) || max_iter < 0 || max_iter > PROBE_MAX_ITER) return 0;
    if (max_iter == 0) return umlh_softmax_probe_bytes(n, d, n_class, 0, 1);
    if (history < 1 || history > SOFTMAX_MAX_HISTORY) return 0;
    return umlh_softmax_probe_bytes(n, d, n_class, 1, history);
}

int umlh_softmax_probe_eval(const float* x, int64_t n, int32_t d, int32_t ldx, const int32_t* y, const double* stats, int32_t n_class,
                            double c, const float* coef, int32_t ldc, double* objective, float* grad, int32_t ldg, double* max_grad,
                            void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_softmax_probe_eval";
    RC(check_softmax(who, x, n, d, ldx, y, n_class, c, coef, ldc, scratch));
    if (!objective && !grad && !max_grad) return fail(UMLH_E_INVALID, "%s: nothing to compute (objective, grad and max_grad are all NULL)", who);
    if (grad && ldg < d + 1) return fail(UMLH_E_INVALID, "%s: ldg=%d < d + 1 = %d", who, ldg, d + 1);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_softmax_probe_bytes(n, d, n_class, 0, 1), 8));
    HIPCHK(umlh_softmax_probe_launch_eval(x, n, d, ldx, y, stats, n_class, c, const_cast<float*>(coef), ldc, objective, grad, ldg, max_grad,
                                          scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_softmax_probe_fit(const float* x, int64_t n, int32_t d, int32_t ldx, const int32_t* y, const double* stats, int32_t n_class,
                           double c, int32_t max_iter, int32_t history, double gtol, int32_t init, float* coef, int32_t ldc,
                           umlh_probe_record_t* record, double* objectives, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_softmax_probe_fit";
    RC(check_softmax(who, x, n, d, ldx, y, n_class, c, coef, ldc, scratch));
    if (!record) return fail(UMLH_E_INVALID, "%s: null pointer (record is required)", who);
    if (max_iter < 1 || max_iter > PROBE_MAX_ITER) return fail(UMLH_E_INVALID, "%s: max_iter=%d outside 1..%d", who, max_iter, PROBE_MAX_ITER);
    if (history < 1 || history > SOFTMAX_MAX_HISTORY) return fail(UMLH_E_INVALID, "%s: history=%d outside 1..%d", who, history, SOFTMAX_MAX_HISTORY);
    if (!(gtol >= 0.0)) return fail(UMLH_E_INVALID, "%s: gtol=%g (need gtol >= 0)", who, gtol);
    if (init != 0 && init != 1) return fail(UMLH_E_INVALID, "%s: init=%d (0 = start from zero, 1 = start from coef)", who, init);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_softmax_probe_bytes(n, d, n_class, 1, history), 8));
    HIPCHK(umlh_softmax_probe_launch_fit(x, n, d, ldx, y, stats, n_class, c, max_iter, history, gtol, init, coef, ldc, record, objectives,
                                         scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_softmax_probe_fold(const float* coef, int32_t ldc, int32_t n_class, int32_t d, const double* stats, float* w, int32_t ldw,
                            float* bias, void* stream) {
    const char* who = "umlh_softmax_probe_fold";
    if (!coef || !w || !bias) return fail(UMLH_E_INVALID, "%s: null pointer (coef, w and bias are required)", who);
    if (n_class < 1 || n_class > SOFTMAX_MAX_CLASSES || d < 1 || d > SOFTMAX_MAX_D)
        return fail(UMLH_E_INVALID, "%s: n_class=%d d=%d (need 1 <= n_class <= 4096, 1 <= d <= 2048)", who, n_class, d);
    if (ldc < d + 1) return fail(UMLH_E_INVALID, "%s: ldc=%d < d + 1 = %d", who, ldc, d + 1);
    if (ldw < d) return fail(UMLH_E_INVALID, "%s: ldw=%d < d=%d", who, ldw, d);
    HIPCHK(umlh_softmax_probe_launch_fold(coef, ldc, n_class, d, stats, w, ldw, bias, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- k-nearest-neighbour probe (kernels: umlh_kernels_knn.hip) ----
static bool knn_shape_ok(int64_t n_train, int64_t n_query, int32_t k) {
    return k >= 1 && k <= LIST_MAX_K && n_train >= k && n_train < ROWS_END && n_query >= 1 && n_query < ROWS_END;
}

uint64_t umlh_knn_scratch_bytes(int64_t n_train, int64_t n_query, int32_t d, int32_t k, int32_t splits) {
    if (!knn_shape_ok(n_train, n_query, k) || d < 1 || splits < 0) return 0;
    return umlh_knn_bytes(n_train, n_query, k, splits);
}

int umlh_knn_search(const float* train, int64_t n_train, int32_t ld_train, const float* query, int64_t n_query, int32_t ld_query,
                    int32_t d, int32_t k, int32_t splits, int32_t* idx, float* dist, void* scratch, uint64_t scratch_bytes,
                    void* stream) {
    const char* who = "umlh_knn_search";
    if (!train || !query || !idx || !scratch)
        return fail(UMLH_E_INVALID, "%s: null pointer (train, query, idx and scratch are required)", who);
    RC(check_list_k(who, k));
    if (!knn_shape_ok(n_train, n_query, k))
        return fail(UMLH_E_INVALID, "%s: n_train=%lld n_query=%lld for k=%d (need k <= n_train < 2^31, 1 <= n_query < 2^31)", who,
                    (long long)n_train, (long long)n_query, k);
    if (d < 1 || ld_train < d || ld_query < d)
        return fail(UMLH_E_INVALID, "%s: d=%d ld_train=%d ld_query=%d (need 1 <= d <= ld)", who, d, ld_train, ld_query);
    if (splits < 0) return fail(UMLH_E_INVALID, "%s: splits=%d < 0", who, splits);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_knn_bytes(n_train, n_query, k, splits), 4));
    HIPCHK(umlh_knn_launch_search(train, n_train, ld_train, query, n_query, ld_query, d, k, splits, idx, dist, scratch,
                                  (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_knn_vote(const int32_t* idx, int64_t n_query, int32_t k, const int32_t* train_labels, int64_t n_train, const int32_t* y,
                  int32_t* pred, int32_t* votes, int64_t* correct, void* stream) {
    const char* who = "umlh_knn_vote";
    if (!idx || !train_labels) return fail(UMLH_E_INVALID, "%s: null pointer (idx and train_labels are required)", who);
    if (!pred && !votes && !correct) return fail(UMLH_E_INVALID, "%s: nothing to compute (pred, votes and correct are all NULL)", who);
    if (correct && !y) return fail(UMLH_E_INVALID, "%s: correct needs the labels y", who);
    RC(check_list_k(who, k));
    if (n_train < 1 || n_train >= ROWS_END || n_query < 1 || n_query >= ROWS_END)
        return fail(UMLH_E_INVALID, "%s: n_train=%lld n_query=%lld (need 1 <= n < 2^31)", who, (long long)n_train, (long long)n_query);
    HIPCHK(umlh_knn_launch_vote(idx, n_query, k, train_labels, n_train, y, pred, votes, ll(correct), (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- singular values and effective rank (kernels: umlh_kernels_spectral.hip) ----
static const int SPECTRAL_MAX_D = 512, SPECTRAL_MAX_BATCH = 65535;

static bool spectral_shape_ok(int64_t batch, int64_t n, int32_t d) {
    return batch >= 1 && batch <= SPECTRAL_MAX_BATCH && n >= 1 && n < ROWS_END && batch * n < ROWS_END && d >= 1 && d <= SPECTRAL_MAX_D;
}

uint64_t umlh_spectral_scratch_bytes(int32_t batch, int64_t n, int32_t d) {
    return spectral_shape_ok(batch, n, d) ? umlh_spectral_bytes(batch, n, d) : 0;
}

// the shared checks of the two dense forms; 0 = fine
static int check_spectral(const char* who, const float* a, int32_t batch, int64_t n, int32_t d, int64_t ld_batch, int64_t ld_row,
                          const void* out, const void* scratch, uint64_t scratch_bytes) {
    if (!a || !out || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (the input, the output and scratch are required)", who);
    if (d < 1 || d > SPECTRAL_MAX_D) return fail(UMLH_E_INVALID, "%s: d=%d outside 1..%d", who, d, SPECTRAL_MAX_D);
    if (!spectral_shape_ok(batch, n, d))
        return fail(UMLH_E_INVALID, "%s: batch=%d n=%lld (need 1 <= batch <= %d, n >= 1, batch * n < 2^31)", who, batch, (long long)n,
                    SPECTRAL_MAX_BATCH);
    if (ld_row < d) return fail(UMLH_E_INVALID, "%s: ld_row=%lld < d=%d", who, (long long)ld_row, d);
    if (!strides_ok(batch, n, d, ld_batch, ld_row))
        return fail(UMLH_E_INVALID, "%s: ld_batch=%lld ld_row=%lld overlap for batch=%d n=%lld d=%d", who, (long long)ld_batch,
                    (long long)ld_row, batch, (long long)n, d);
    return check_scratch(who, scratch, scratch_bytes, umlh_spectral_bytes(batch, n, d), 0);
}

int umlh_svdvals(const float* a, int32_t batch, int64_t n, int32_t d, int64_t ld_batch, int64_t ld_row, double* sv, void* scratch,
                 uint64_t scratch_bytes, void* stream) {
    RC(check_spectral("umlh_svdvals", a, batch, n, d, ld_batch, ld_row, sv, scratch, scratch_bytes));
    HIPCHK(umlh_spectral_launch(a, batch, n, (int)n, ld_batch, 0, ld_row, nullptr, 0, d, 0.0, nullptr, nullptr, sv,
                                (int)(n < d ? n : d), scratch, (hipStream_t)stream), "umlh_svdvals");
    return UMLH_OK;
}

int umlh_effective_rank(const float* a, int32_t batch, int64_t n, int32_t d, int64_t ld_batch, int64_t ld_row, double eps, double* erank,
                        double* sv_or_null, void* scratch, uint64_t scratch_bytes, void* stream) {
    RC(check_spectral("umlh_effective_rank", a, batch, n, d, ld_batch, ld_row, erank, scratch, scratch_bytes));
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(UMLH_E_INVALID, "umlh_effective_rank: eps=%g (need a finite eps >= 0)", eps);
    HIPCHK(umlh_spectral_launch(a, batch, n, (int)n, ld_batch, 0, ld_row, nullptr, 0, d, eps, erank, nullptr, sv_or_null,
                                (int)(n < d ? n : d), scratch, (hipStream_t)stream), "umlh_effective_rank");
    return UMLH_OK;
}

int umlh_effective_rank_seq(const float* z, int32_t b, int32_t t_len, int32_t d, int64_t ldb, int64_t ldt, const int64_t* lengths,
                            int32_t drop_last, double eps, double* out2, double* sv_or_null, void* scratch, uint64_t scratch_bytes,
                            void* stream) {
    const char* who = "umlh_effective_rank_seq";
    if (!z || !out2 || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (z, out2 and scratch are required)", who);
    if (d < 1 || d > SPECTRAL_MAX_D) return fail(UMLH_E_INVALID, "%s: d=%d outside 1..%d", who, d, SPECTRAL_MAX_D);
    if (b < 1 || t_len < 1 || !spectral_shape_ok(1, (int64_t)b * t_len, d))
        return fail(UMLH_E_INVALID, "%s: b=%d t_len=%d (need b >= 1, t_len >= 1, b * t_len < 2^31)", who, b, t_len);
    if (ldt < d || ldb < d) return fail(UMLH_E_INVALID, "%s: ldb=%lld ldt=%lld shorter than d=%d", who, (long long)ldb, (long long)ldt, d);
    if (!strides_ok(b, t_len, d, ldb, ldt))
        return fail(UMLH_E_INVALID, "%s: ldb=%lld ldt=%lld overlap for b=%d t_len=%d d=%d", who, (long long)ldb, (long long)ldt, b, t_len, d);
    if (drop_last < 0) return fail(UMLH_E_INVALID, "%s: drop_last=%d < 0", who, drop_last);
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(UMLH_E_INVALID, "%s: eps=%g (need a finite eps >= 0)", who, eps);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_spectral_bytes(1, (int64_t)b * t_len, d), 0));
    HIPCHK(umlh_spectral_launch(z, 1, (int64_t)b * t_len, t_len, 0, ldb, ldt, ll(lengths), drop_last, d, eps, out2, out2 + 1, sv_or_null,
                                d, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- principal subspaces and SVCCA (kernels: umlh_kernels_spectral.hip) ----
static const int SUBSPACE_MAX_Q = 64;

// d_b = 0: the single-matrix op.  The row stride is an int in the column-statistics kernels, hence ld < 2^31.
static bool subspace_shape_ok(int64_t n, int32_t d_a, int32_t d_b, int32_t q) {
    if (n < 2 || n >= ROWS_END || d_a < 1 || d_a > SPECTRAL_MAX_D || d_b < 0 || d_b > SPECTRAL_MAX_D) return false;
    const int64_t lim = std::min<int64_t>(std::min<int64_t>(n, d_a), std::min<int64_t>(d_b ? d_b : d_a, SUBSPACE_MAX_Q));
    return q >= 1 && q <= lim;
}

uint64_t umlh_subspace_scratch_bytes(int64_t n, int32_t d_a, int32_t d_b, int32_t q) {
    return subspace_shape_ok(n, d_a, d_b, q) ? umlh_subspace_bytes(n, d_a, d_b, q) : 0;
}

// the checks of one view; 0 = fine
static int check_view(const char* who, const char* name, int32_t d, int64_t ld) {
    if (d < 1 || d > SPECTRAL_MAX_D) return fail(UMLH_E_INVALID, "%s: d_%s=%d outside 1..%d", who, name, d, SPECTRAL_MAX_D);
    if (ld < d || ld >= ROWS_END)
        return fail(UMLH_E_INVALID, "%s: ld_%s=%lld (need d_%s=%d <= ld < 2^31)", who, name, (long long)ld, name, d);
    return UMLH_OK;
}

int umlh_principal_subspace(const float* a, int64_t n, int32_t d, int64_t ld_row, int32_t q, int32_t standardize, double* evals,
                            double* evecs, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_principal_subspace";
    if (!a || !evals || !evecs || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (a, evals, evecs and scratch are required)", who);
    if (n < 2 || n >= ROWS_END) return fail(UMLH_E_INVALID, "%s: n=%lld (need 2 <= n < 2^31)", who, (long long)n);
    RC(check_view(who, "a", d, ld_row));
    if (!subspace_shape_ok(n, d, 0, q))
        return fail(UMLH_E_INVALID, "%s: q=%d outside 1..min(n, d, %d) for n=%lld d=%d", who, q, SUBSPACE_MAX_Q, (long long)n, d);
    if (standardize != 0 && standardize != 1) return fail(UMLH_E_INVALID, "%s: standardize=%d (need 0 or 1)", who, standardize);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_subspace_bytes(n, d, 0, q), 0));
    HIPCHK(umlh_subspace_launch(a, n, d, ld_row, q, standardize, evals, evecs, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_svcca(const float* a, const float* b, int64_t n, int32_t d_a, int32_t d_b, int64_t ld_a, int64_t ld_b, int32_t q, double* out,
               double* rho_or_null, double* evals_or_null, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_svcca";
    if (!a || !b || !out || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (a, b, out and scratch are required)", who);
    if (n < 2 || n >= ROWS_END) return fail(UMLH_E_INVALID, "%s: n=%lld (need 2 <= n < 2^31)", who, (long long)n);
    RC(check_view(who, "a", d_a, ld_a));
    RC(check_view(who, "b", d_b, ld_b));
    if (!subspace_shape_ok(n, d_a, d_b, q))
        return fail(UMLH_E_INVALID, "%s: q=%d outside 1..min(n, d_a, d_b, %d) for n=%lld d_a=%d d_b=%d", who, q, SUBSPACE_MAX_Q,
                    (long long)n, d_a, d_b);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_subspace_bytes(n, d_a, d_b, q), 0));
    HIPCHK(umlh_svcca_launch(a, b, n, d_a, d_b, ld_a, ld_b, q, out, rho_or_null, evals_or_null, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- embedding capture (kernels: umlh_kernels_capture.hip) ----
static const int SEQ_MAX_B = 65535;   // sequences of one [b, t_len, d] view: a grid dimension of the capture and step-statistics kernels

int umlh_seq_compact(const float* z, int32_t b, int32_t t_len, int32_t d, int64_t ldb, int64_t ldt, const int64_t* lengths,
                     int32_t drop_last, float* out, int64_t ldo, int64_t out_rows, int64_t* rows_total, void* stream) {
    const char* who = "umlh_seq_compact";
    if (!z || !out) return fail(UMLH_E_INVALID, "%s: null pointer (z and out are required)", who);
    if (!rows_total) return fail(UMLH_E_INVALID, "%s: rows_total is NULL (the row count is always written)", who);
    if (d < 1) return fail(UMLH_E_INVALID, "%s: d=%d < 1", who, d);
    if (b < 1 || b > SEQ_MAX_B) return fail(UMLH_E_INVALID, "%s: b=%d outside 1..%d", who, b, SEQ_MAX_B);
    if (t_len < 1) return fail(UMLH_E_INVALID, "%s: t_len=%d < 1", who, t_len);
    RC(check_strides(who, "ldb", "ldt", b, t_len, d, ldb, ldt));
    if (drop_last < 0) return fail(UMLH_E_INVALID, "%s: drop_last=%d < 0", who, drop_last);
    if (ldo < d) return fail(UMLH_E_INVALID, "%s: ldo=%lld < d=%d", who, (long long)ldo, d);
    if (out_rows < 0) return fail(UMLH_E_INVALID, "%s: out_rows=%lld < 0", who, (long long)out_rows);
    HIPCHK(umlh_capture_launch_compact(z, b, t_len, d, ldb, ldt, ll(lengths), drop_last, out, ldo, out_rows, ll(rows_total),
                                       (hipStream_t)stream), who);
    return UMLH_OK;
}

uint64_t umlh_paired_cosine_scratch_bytes(int64_t n, int32_t d) {
    return n >= 1 && d >= 1 ? umlh_capture_cosine_bytes(n) : 0;
}

int umlh_paired_cosine(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t n, int32_t d, double eps, double* out2,
                       float* rows_or_null, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_paired_cosine";
    if (!a || !b || !out2 || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (a, b, out2 and scratch are required)", who);
    if (n < 1) return fail(UMLH_E_INVALID, "%s: n=%lld rows (need n >= 1)", who, (long long)n);
    if (d < 1) return fail(UMLH_E_INVALID, "%s: d=%d < 1", who, d);
    if (lda < d) return fail(UMLH_E_INVALID, "%s: lda=%lld < d=%d", who, (long long)lda, d);
    if (ldb < d) return fail(UMLH_E_INVALID, "%s: ldb=%lld < d=%d", who, (long long)ldb, d);
    if (!(eps >= 0.0)) return fail(UMLH_E_INVALID, "%s: eps=%g (need eps >= 0)", who, eps);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_capture_cosine_bytes(n), 0));
    HIPCHK(umlh_capture_launch_cosine(a, lda, b, ldb, n, d, eps, out2, rows_or_null, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- per-step logged statistics (kernels: umlh_kernels_stepstats.hip) ----
static bool step_stats_shape_ok(int32_t b, int32_t t_len, int32_t d) {
    return b >= 1 && b <= SEQ_MAX_B && t_len >= 1 && d >= 1 && umlh_stepstats_partials(b, t_len, d) >= 0;
}

uint64_t umlh_seq_step_stats_scratch_bytes(int32_t b, int32_t t_len, int32_t d) {
    return step_stats_shape_ok(b, t_len, d) ? umlh_stepstats_bytes(b, t_len, d) : 0;
}

int umlh_seq_step_stats(const float* x, int64_t ldb, int64_t ldt, const float* recon_or_null, int64_t ldb_r, int64_t ldt_r, int32_t b,
                        int32_t t_len, int32_t d, const int64_t* lengths, double* out4, void* scratch, uint64_t scratch_bytes,
                        void* stream) {
    const char* who = "umlh_seq_step_stats";
    if (!x || !out4 || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (x, out4 and scratch are required)", who);
    if (d < 1) return fail(UMLH_E_INVALID, "%s: d=%d < 1", who, d);
    if (b < 1 || b > SEQ_MAX_B) return fail(UMLH_E_INVALID, "%s: b=%d outside 1..%d", who, b, SEQ_MAX_B);
    if (t_len < 1) return fail(UMLH_E_INVALID, "%s: t_len=%d < 1", who, t_len);
    if (!step_stats_shape_ok(b, t_len, d))
        return fail(UMLH_E_INVALID, "%s: b=%d t_len=%d d=%d too large (need b * ceil((t_len - 1) / 64) * ceil(d / 1024) <= 2^22)", who, b,
                    t_len, d);
    RC(check_strides(who, "ldb", "ldt", b, t_len, d, ldb, ldt));
    if (recon_or_null) RC(check_strides(who, "ldb_r", "ldt_r", b, t_len, d, ldb_r, ldt_r));
    RC(check_scratch(who, scratch, scratch_bytes, umlh_stepstats_bytes(b, t_len, d), 0));
    HIPCHK(umlh_stepstats_launch(x, ldb, ldt, recon_or_null, ldb_r, ldt_r, b, t_len, d, ll(lengths), out4, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- rollout and spectra (kernels: umlh_kernels_rollout.hip) ----
int umlh_rollout(const umlh_rollout_cfg_t* cfg, const float* const* P, const float* conv_w_or_null, const float* pos0_or_null,
                 const float* w_in, const float* b_in, const float* w_out, const float* b_out, const float* x0, int64_t ldx, int64_t n,
                 float* out, int64_t ldb, int64_t ldt, void* stream) {
    const char* who = "umlh_rollout";
    if (!cfg) return fail(UMLH_E_INVALID, "%s: cfg is NULL", who);
    if (!w_in || !b_in || !w_out || !b_out || !x0 || !out)
        return fail(UMLH_E_INVALID, "%s: null pointer (w_in, b_in, w_out, b_out, x0 and out are required)", who);
    if (cfg->Z < 1 || cfg->Z > 512) return fail(UMLH_E_INVALID, "%s: Z=%d outside the envelope 1..512", who, cfg->Z);
    if (cfg->d_ff < 1 || cfg->d_ff > 2048) return fail(UMLH_E_INVALID, "%s: d_ff=%d outside the envelope 1..2048", who, cfg->d_ff);
    if (cfg->D < 1 || cfg->D > 1024) return fail(UMLH_E_INVALID, "%s: D=%d outside the envelope 1..1024", who, cfg->D);
    if (cfg->n_layers < 0 || cfg->n_layers > UMLH_ROLLOUT_MAX_LAYERS)
        return fail(UMLH_E_INVALID, "%s: n_layers=%d outside 0..%d", who, cfg->n_layers, UMLH_ROLLOUT_MAX_LAYERS);
    if (cfg->steps < 0 || cfg->steps > 4096) return fail(UMLH_E_INVALID, "%s: steps=%d outside 0..4096", who, cfg->steps);
    if (!(cfg->eps >= 0.0f)) return fail(UMLH_E_INVALID, "%s: eps=%g (need eps >= 0)", who, (double)cfg->eps);
    if (n < 1 || n > ((int64_t)1 << 20)) return fail(UMLH_E_INVALID, "%s: n=%lld rows (need 1 <= n <= 2^20)", who, (long long)n);
    if (cfg->n_layers > 0 && !P) return fail(UMLH_E_INVALID, "%s: P is NULL with n_layers=%d", who, cfg->n_layers);
    for (int i = 0; i < 12 * cfg->n_layers; ++i)
        if (!P[i]) return fail(UMLH_E_INVALID, "%s: P[%d] is NULL (12 tensors per layer)", who, i);
    if (ldx < cfg->D) return fail(UMLH_E_INVALID, "%s: ldx=%lld < D=%d", who, (long long)ldx, cfg->D);
    if (ldt < cfg->D) return fail(UMLH_E_INVALID, "%s: ldt=%lld < D=%d", who, (long long)ldt, cfg->D);
    if (ldb < (int64_t)cfg->steps * ldt + cfg->D)
        return fail(UMLH_E_INVALID, "%s: ldb=%lld < steps*ldt + D = %lld (rows of out would overlap)", who, (long long)ldb,
                    (long long)((int64_t)cfg->steps * ldt + cfg->D));
    if (umlh_rollout_lds_bytes(cfg->Z, cfg->d_ff, cfg->D) > UMLH_ROLLOUT_MAX_LDS)
        return fail(UMLH_E_INVALID, "%s: Z=%d D=%d outside the envelope (LDS)", who, cfg->Z, cfg->D);
    HIPCHK(umlh_rollout_launch(cfg, P, conv_w_or_null, pos0_or_null, w_in, b_in, w_out, b_out, x0, ldx, n, out, ldb, ldt,
                               (hipStream_t)stream), who);
    return UMLH_OK;
}

static bool spectrum_shape_ok(int32_t b, int32_t t_len, int32_t d) {
    return b >= 1 && b <= (1 << 20) && t_len >= 1 && t_len <= UMLH_SPECTRUM_MAX_T && d >= 1 && umlh_spectrum_partials(b, t_len, d) >= 0;
}

uint64_t umlh_seq_spectrum_scratch_bytes(int32_t b, int32_t t_len, int32_t d) {
    return spectrum_shape_ok(b, t_len, d) ? umlh_spectrum_bytes(b, t_len, d) : 0;
}

int umlh_seq_spectrum(const float* x, int64_t ldb, int64_t ldt, int32_t b, int32_t t_len, int32_t d, double* out, void* scratch,
                      uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_seq_spectrum";
    if (!x || !out || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (x, out and scratch are required)", who);
    if (d < 1) return fail(UMLH_E_INVALID, "%s: d=%d < 1", who, d);
    if (b < 1 || b > (1 << 20)) return fail(UMLH_E_INVALID, "%s: b=%d outside 1..2^20", who, b);
    if (t_len < 1 || t_len > UMLH_SPECTRUM_MAX_T) return fail(UMLH_E_INVALID, "%s: t_len=%d outside 1..%d", who, t_len, UMLH_SPECTRUM_MAX_T);
    if (!spectrum_shape_ok(b, t_len, d))
        return fail(UMLH_E_INVALID, "%s: b=%d d=%d too large (need ceil(b / 16) * ceil(d / 16) <= 2^20)", who, b, d);
    RC(check_strides(who, "ldb", "ldt", b, t_len, d, ldb, ldt));
    RC(check_scratch(who, scratch, scratch_bytes, umlh_spectrum_bytes(b, t_len, d), 0));
    HIPCHK(umlh_spectrum_launch(x, ldb, ldt, b, t_len, d, out, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- class index and class statistics (kernels: umlh_kernels_classstats.hip) ----
static bool class_index_shape_ok(int64_t n, int32_t n_class) { return n >= 1 && n < ROWS_END && n_class >= 1; }

uint64_t umlh_class_index_scratch_bytes(int64_t n, int32_t n_class) {
    return class_index_shape_ok(n, n_class) ? umlh_classindex_bytes(n, n_class) : 0;
}

int umlh_class_index(const int64_t* labels, int64_t n, int32_t n_class, int32_t* order, int64_t* offsets, void* scratch,
                     uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_class_index";
    if (!labels) return fail(UMLH_E_INVALID, "%s: labels is NULL", who);
    if (!order) return fail(UMLH_E_INVALID, "%s: order is NULL", who);
    if (!offsets) return fail(UMLH_E_INVALID, "%s: offsets is NULL", who);
    if (!scratch) return fail(UMLH_E_INVALID, "%s: scratch is NULL", who);
    if (n < 1 || n >= ROWS_END) return fail(UMLH_E_INVALID, "%s: n=%lld rows (need 1 <= n < 2^31)", who, (long long)n);
    if (n_class < 1) return fail(UMLH_E_INVALID, "%s: n_class=%d < 1", who, n_class);
    const uint64_t need = umlh_classindex_bytes(n, n_class);
    if (need == 0)
        return fail(UMLH_E_INVALID, "%s: n=%lld with n_class=%d needs more than 2^28 block counts (ceil(n / 256) * n_class)", who,
                    (long long)n, n_class);
    RC(check_scratch(who, scratch, scratch_bytes, need, 0));
    HIPCHK(umlh_classindex_launch(ll(labels), n, n_class, order, ll(offsets), scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

uint64_t umlh_class_stats_scratch_bytes(int64_t n, int32_t d, int32_t n_class) {
    return class_index_shape_ok(n, n_class) && d >= 1 ? umlh_classstats_bytes(n, d, n_class) : 0;
}

int umlh_class_stats(const float* feats, int64_t ld, int64_t n, int32_t d, const int32_t* order, const int64_t* offsets, int32_t n_class,
                     float* means, int64_t ld_means, double* dist, double* out2, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_class_stats";
    if (!feats) return fail(UMLH_E_INVALID, "%s: feats is NULL", who);
    if (!order) return fail(UMLH_E_INVALID, "%s: order is NULL", who);
    if (!offsets) return fail(UMLH_E_INVALID, "%s: offsets is NULL", who);
    if (!means) return fail(UMLH_E_INVALID, "%s: means is NULL", who);
    if (!dist) return fail(UMLH_E_INVALID, "%s: dist is NULL", who);
    if (!out2) return fail(UMLH_E_INVALID, "%s: out2 is NULL", who);
    if (!scratch) return fail(UMLH_E_INVALID, "%s: scratch is NULL", who);
    if (n < 1 || n >= ROWS_END) return fail(UMLH_E_INVALID, "%s: n=%lld rows (need 1 <= n < 2^31)", who, (long long)n);
    if (d < 1) return fail(UMLH_E_INVALID, "%s: d=%d < 1", who, d);
    if (n_class < 1) return fail(UMLH_E_INVALID, "%s: n_class=%d < 1", who, n_class);
    if (ld < d) return fail(UMLH_E_INVALID, "%s: ld=%lld < d=%d", who, (long long)ld, d);
    if (ld_means < d) return fail(UMLH_E_INVALID, "%s: ld_means=%lld < d=%d", who, (long long)ld_means, d);
    const uintptr_t f0 = reinterpret_cast<uintptr_t>(feats), f1 = f0 + ((uint64_t)(n - 1) * (uint64_t)ld + (uint64_t)d) * sizeof(float);
    const uintptr_t m0 = reinterpret_cast<uintptr_t>(means), m1 = m0 + ((uint64_t)(n_class - 1) * (uint64_t)ld_means + (uint64_t)d) * sizeof(float);
    if (m0 < f1 && f0 < m1) return fail(UMLH_E_INVALID, "%s: means overlaps feats", who);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_classstats_bytes(n, d, n_class), 0));
    HIPCHK(umlh_classstats_launch(feats, ld, n, d, order, ll(offsets), n_class, means, ld_means, dist, out2, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- class-wise validation report (kernels: umlh_kernels_evalreport.hip) ----
static bool eval_topk_shape_ok(int64_t n, int64_t n_class, int32_t k) {
    return k >= 1 && k <= LIST_MAX_K && n_class >= k && n_class < ROWS_END && n >= 1 && n < ROWS_END;
}

uint64_t umlh_eval_topk_scratch_bytes(int64_t n, int64_t n_class, int32_t d, int32_t k, int32_t splits) {
    if (!eval_topk_shape_ok(n, n_class, k) || d < 1 || splits < 0) return 0;
    return umlh_evalreport_bytes(n, n_class, k, splits);
}

int umlh_eval_topk(const float* x, int64_t n, int32_t ldx, const float* w, int64_t n_class, int32_t ldw, int32_t d,
                   const float* bias_or_null, const float* scale_dev_or_null, int32_t k, int32_t splits, int32_t* cls,
                   float* logit_or_null, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_eval_topk";
    if (!x || !w || !cls || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (x, w, cls and scratch are required)", who);
    RC(check_list_k(who, k));
    if (!eval_topk_shape_ok(n, n_class, k))
        return fail(UMLH_E_INVALID, "%s: n=%lld n_class=%lld for k=%d (need 1 <= n < 2^31, k <= n_class < 2^31)", who, (long long)n,
                    (long long)n_class, k);
    if (d < 1 || ldx < d || ldw < d) return fail(UMLH_E_INVALID, "%s: d=%d ldx=%d ldw=%d (need 1 <= d <= ld)", who, d, ldx, ldw);
    if (splits < 0) return fail(UMLH_E_INVALID, "%s: splits=%d < 0", who, splits);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_evalreport_bytes(n, n_class, k, splits), 4, SCRATCH_BYTES_EQ));
    HIPCHK(umlh_evalreport_launch_topk(x, n, ldx, w, n_class, ldw, d, bias_or_null, scale_dev_or_null, k, splits, cls, logit_or_null,
                                       scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_eval_classwise(const int32_t* cls, int64_t n, int32_t k, const int64_t* labels, int64_t n_class, int64_t* support,
                        int64_t* hit1, int64_t* hitk, int64_t* confusion_or_null, int64_t* misc2, void* stream) {
    const char* who = "umlh_eval_classwise";
    if (!cls || !labels || !support || !hit1 || !hitk || !misc2)
        return fail(UMLH_E_INVALID, "%s: null pointer (cls, labels, support, hit1, hitk and misc2 are required)", who);
    RC(check_list_k(who, k));
    if (n < 1 || n >= ROWS_END || n_class < 1 || n_class >= ROWS_END)
        return fail(UMLH_E_INVALID, "%s: n=%lld n_class=%lld (need 1 <= n < 2^31, 1 <= n_class < 2^31)", who, (long long)n,
                    (long long)n_class);
    HIPCHK(umlh_evalreport_launch_classwise(cls, n, k, ll(labels), n_class, ll(support), ll(hit1), ll(hitk), ll(confusion_or_null),
                                            ll(misc2), (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- outlier clamp and feature preparation (kernels: umlh_kernels_outlier.hip) ----
static bool outlier_shape_ok(int64_t n, int64_t d) {
    return n >= 1 && d >= 1 && d < ROWS_END && n < (1LL << 40) && n * d < (1LL << 40);      // n, d < 2^40, 2^31: no overflow
}

uint64_t umlh_outlier_scratch_bytes(int32_t kind, int64_t n, int64_t d) {
    if (!outlier_shape_ok(n, d)) return 0;
    if (kind == UMLH_OUTLIER_ROW_QUANTILE) return umlh_outlier_quantile_bytes(n);
    if (kind == UMLH_OUTLIER_ABS_KTH) return umlh_outlier_kth_bytes();
    if (kind == UMLH_OUTLIER_KNN_ACCURACY) return n < ROWS_END ? umlh_outlier_accuracy_bytes(n) : 0;
    return 0;
}

static int outlier_check(const char* who, int64_t n, int64_t d, int64_t ld) {
    if (!outlier_shape_ok(n, d))
        return fail(UMLH_E_INVALID, "%s: n=%lld d=%lld (need n >= 1, 1 <= d < 2^31, n * d < 2^40)", who, (long long)n, (long long)d);
    if (ld < d) return fail(UMLH_E_INVALID, "%s: row stride %lld < d=%lld", who, (long long)ld, (long long)d);
    return UMLH_OK;
}

int umlh_row_abs_quantile(const float* x, int64_t n, int64_t d, int64_t ld, double q, float* lo_val, float* hi_val, float* quant,
                          double* mean64, float* q_val, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_row_abs_quantile";
    if (!x || !quant || !q_val || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (x, quant, q_val and scratch are required)", who);
    RC(outlier_check(who, n, d, ld));
    if (!(q >= 0.0 && q < 1.0)) return fail(UMLH_E_INVALID, "%s: q=%g outside [0, 1)", who, q);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_outlier_quantile_bytes(n), 8, SCRATCH_BYTES_EQ));
    const double pos = q * (double)(d - 1);
    int64_t lo = (int64_t)std::floor(pos);
    if (lo > d - 1) lo = d - 1;
    const int64_t hi = lo + 1 < d ? lo + 1 : d - 1;
    HIPCHK(umlh_outlier_launch_quantile(x, n, (int)d, ld, (int)lo, (int)hi, pos - (double)lo, lo_val, hi_val, quant, mean64, q_val,
                                        scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_abs_kth(const float* x, int64_t n, int64_t d, int64_t ld, int64_t k, float* out, void* scratch, uint64_t scratch_bytes,
                 void* stream) {
    const char* who = "umlh_abs_kth";
    if (!x || !out || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (x, out and scratch are required)", who);
    RC(outlier_check(who, n, d, ld));
    if (k < 0 || k >= n * d) return fail(UMLH_E_INVALID, "%s: k=%lld outside 0..n*d-1 = %lld", who, (long long)k, (long long)(n * d - 1));
    RC(check_scratch(who, scratch, scratch_bytes, umlh_outlier_kth_bytes(), 8, SCRATCH_BYTES_EQ));
    HIPCHK(umlh_outlier_launch_kth(x, n, d, ld, k, out, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_clamp_rows(const float* x, int64_t n, int64_t d, int64_t ldx, const float* q_val, int32_t normalize, float* out,
                    int64_t ldo, void* stream) {
    const char* who = "umlh_clamp_rows";
    if (!x || !q_val || !out) return fail(UMLH_E_INVALID, "%s: null pointer (x, q_val and out are required)", who);
    RC(outlier_check(who, n, d, ldx));
    if (ldo < d) return fail(UMLH_E_INVALID, "%s: output row stride %lld < d=%lld", who, (long long)ldo, (long long)d);
    if (out == x && ldo != ldx)
        return fail(UMLH_E_INVALID, "%s: in place needs ldo == ldx (ldo=%lld ldx=%lld)", who, (long long)ldo, (long long)ldx);
    HIPCHK(umlh_outlier_launch_clamp(x, n, (int)d, ldx, q_val, normalize != 0, out, ldo, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_knn_accuracy(const int32_t* knn, int64_t n, int64_t m, int64_t ld, double* out, void* scratch, uint64_t scratch_bytes,
                      void* stream) {
    const char* who = "umlh_knn_accuracy";
    if (!knn || !out || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (knn, out and scratch are required)", who);
    if (!outlier_shape_ok(n, m) || n >= ROWS_END)
        return fail(UMLH_E_INVALID, "%s: n=%lld m=%lld (need 1 <= n < 2^31, 1 <= m < 2^31, n * m < 2^40)", who, (long long)n, (long long)m);
    if (ld != 0 && ld < m) return fail(UMLH_E_INVALID, "%s: row stride %lld (need 0 or >= m=%lld)", who, (long long)ld, (long long)m);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_outlier_accuracy_bytes(n), 8, SCRATCH_BYTES_EQ));
    HIPCHK(umlh_outlier_launch_accuracy(knn, n, m, ld, out, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- device loader of the affect datasets (kernels: umlh_kernels_seqload.hip) ----
static const int64_t SEQ_BLOCK_END = (int64_t)1 << 31;    // exclusive: t_len * d words of one sample are indexed with an int
static const int SEQ_MAX_BATCH = 65535, SEQ_MAX_COLS = 1 << 20;

// the shape of one [n, t_len, d] table; 0 = fine
static int check_seq_table(const char* who, int64_t n, int32_t t_len, int32_t d) {
    if (n < 1 || n >= ROWS_END) return fail(UMLH_E_INVALID, "%s: n=%lld samples (need 1 <= n < 2^31)", who, (long long)n);
    if (t_len < 1) return fail(UMLH_E_INVALID, "%s: t_len=%d < 1", who, t_len);
    if (d < 1 || d > SEQ_MAX_COLS) return fail(UMLH_E_INVALID, "%s: d=%d outside 1..%d", who, d, SEQ_MAX_COLS);
    if ((int64_t)t_len * d >= SEQ_BLOCK_END)
        return fail(UMLH_E_INVALID, "%s: t_len=%d d=%d (need t_len * d < 2^31 words per sample)", who, t_len, d);
    return UMLH_OK;
}

int umlh_seq_first_nonzero(const float* x, int64_t n, int32_t t_len, int32_t d, int32_t* start, void* stream) {
    const char* who = "umlh_seq_first_nonzero";
    if (!x || !start) return fail(UMLH_E_INVALID, "%s: null pointer (x and start are required)", who);
    RC(check_seq_table(who, n, t_len, d));
    HIPCHK(umlh_seqload_launch_first_row(x, n, t_len, d, start, (hipStream_t)stream), who);
    return UMLH_OK;
}

static bool colnorm_shape_ok(int64_t rows, int32_t d) { return rows >= 1 && rows < ((int64_t)1 << 40) && d >= 1 && d <= SEQ_MAX_COLS; }

uint64_t umlh_seq_column_standardize_scratch(int64_t rows, int32_t d) {
    return colnorm_shape_ok(rows, d) ? umlh_seqload_colnorm_bytes(rows, d) : 0;
}

int umlh_seq_column_standardize(const float* x, int64_t rows, int32_t d, int64_t ldx, float* out, int64_t ldo, double* stats,
                                void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_seq_column_standardize";
    if (!x || !out || !stats || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (x, out, stats and scratch are required)", who);
    if (!colnorm_shape_ok(rows, d))
        return fail(UMLH_E_INVALID, "%s: rows=%lld d=%d (need 1 <= rows < 2^40, 1 <= d <= %d)", who, (long long)rows, d, SEQ_MAX_COLS);
    if (ldx < d) return fail(UMLH_E_INVALID, "%s: ldx=%lld < d=%d", who, (long long)ldx, d);
    if (ldo < d) return fail(UMLH_E_INVALID, "%s: ldo=%lld < d=%d", who, (long long)ldo, d);
    if (out == x && ldo != ldx)
        return fail(UMLH_E_INVALID, "%s: in place needs ldo == ldx (ldo=%lld ldx=%lld)", who, (long long)ldo, (long long)ldx);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_seqload_colnorm_bytes(rows, d), 8));
    HIPCHK(umlh_seqload_launch_colnorm(x, rows, d, ldx, out, ldo, stats, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_seq_standardize(float* x, int64_t n, int32_t t_len, int32_t d, const int32_t* start, void* stream) {
    const char* who = "umlh_seq_standardize";
    if (!x || !start) return fail(UMLH_E_INVALID, "%s: null pointer (x and start are required)", who);
    RC(check_seq_table(who, n, t_len, d));
    HIPCHK(umlh_seqload_launch_znorm(x, n, t_len, d, start, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_seq_gather_pad(const float* const* srcs, const int32_t* dims, int32_t n_src, int64_t n, int32_t t_len, const int32_t* start,
                        const int64_t* ids, int32_t b, int32_t t_out, float* const* outs, int64_t* lengths, void* stream) {
    const char* who = "umlh_seq_gather_pad";
    if (!srcs || !dims || !outs || !start || !ids || !lengths)
        return fail(UMLH_E_INVALID, "%s: null pointer (srcs, dims, outs, start, ids and lengths are required)", who);
    if (n_src < 1 || n_src > UMLH_SEQ_GATHER_MAX_SOURCES)
        return fail(UMLH_E_INVALID, "%s: n_src=%d outside 1..%d", who, n_src, UMLH_SEQ_GATHER_MAX_SOURCES);
    if (b < 1 || b > SEQ_MAX_BATCH) return fail(UMLH_E_INVALID, "%s: b=%d outside 1..%d", who, b, SEQ_MAX_BATCH);
    if (t_out < 1) return fail(UMLH_E_INVALID, "%s: t_out=%d < 1", who, t_out);
    int used = 0;
    for (int m = 0; m < n_src; ++m) {
        if (!srcs[m]) continue;
        ++used;
        if (!outs[m]) return fail(UMLH_E_INVALID, "%s: source %d has no destination", who, m);
        RC(check_seq_table(who, n, t_len, dims[m]));
        if ((int64_t)t_out * dims[m] >= SEQ_BLOCK_END)
            return fail(UMLH_E_INVALID, "%s: t_out=%d d=%d of source %d (need t_out * d < 2^31 words per block)", who, t_out, dims[m], m);
    }
    if (!used) return fail(UMLH_E_INVALID, "%s: every source is NULL", who);
    HIPCHK(umlh_seqload_launch_gather_pad(srcs, dims, n_src, n, t_len, start, ll(ids), b, t_out, outs, ll(lengths), (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- robustness test sets: time-series noise on a table of the loader (after the loader's section here: it shares its checks) ----
int umlh_seq_perturb(const float* src, int64_t n, int32_t t_len, int32_t d, int32_t unit_rows, const double* eps, const uint8_t* keep,
                     float elem_p, uint64_t seed, float* dst, int32_t* start_out, void* stream) {
    const char* who = "umlh_seq_perturb";
    if (!src || !dst) return fail(UMLH_E_INVALID, "%s: null pointer (src and dst are required)", who);
    RC(check_seq_table(who, n, t_len, d));
    if (unit_rows != t_len && unit_rows != 1)
        return fail(UMLH_E_INVALID, "%s: unit_rows=%d (need t_len=%d, one draw per sample, or 1, one per time step)", who, unit_rows, t_len);
    if (!(elem_p >= 0.f && elem_p <= 1.f)) return fail(UMLH_E_INVALID, "%s: elem_p=%g outside [0, 1]", who, (double)elem_p);
    const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t bytes = (uintptr_t)n * (uintptr_t)t_len * (uintptr_t)d * sizeof(float);
    if (a != b && a < b + bytes && b < a + bytes)
        return fail(UMLH_E_INVALID, "%s: dst overlaps src partially (in place needs dst == src)", who);
    HIPCHK(umlh_seqload_launch_perturb(src, n, t_len, d, unit_rows == 1 && t_len != 1, eps, keep, elem_p, seed, dst, start_out,
                                       (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- MIMIC loader: standardisation of a cleaned table, tabular noise, row gather (kernels: umlh_kernels_tabular.hip; after the
// loader's section here, as the robustness section above: it shares its checks) ----
// bytes [a, a + na) and [b, b + nb) share at least one byte
static bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

uint64_t umlh_tab_standardize_scratch(int64_t rows, int32_t d) {
    return colnorm_shape_ok(rows, d) ? umlh_seqload_colnorm_bytes(rows, d) : 0;
}

int umlh_tab_standardize(const void* x, int32_t x_is_f64, int64_t rows, int32_t d, int64_t ldx, float* out, int64_t ldo, double* stats,
                         void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_tab_standardize";
    if (!x || !out || !stats || !scratch) return fail(UMLH_E_INVALID, "%s: null pointer (x, out, stats and scratch are required)", who);
    if (x_is_f64 != 0 && x_is_f64 != 1) return fail(UMLH_E_INVALID, "%s: x_is_f64=%d (0: a float source, 1: a double source)", who, x_is_f64);
    if (!colnorm_shape_ok(rows, d))
        return fail(UMLH_E_INVALID, "%s: rows=%lld d=%d (need 1 <= rows < 2^40, 1 <= d <= %d)", who, (long long)rows, d, SEQ_MAX_COLS);
    if (ldx < d) return fail(UMLH_E_INVALID, "%s: ldx=%lld < d=%d", who, (long long)ldx, d);
    if (ldo < d) return fail(UMLH_E_INVALID, "%s: ldo=%lld < d=%d", who, (long long)ldo, d);
    if (x_is_f64) {
        if (ranges_overlap(x, ((uint64_t)(rows - 1) * ldx + d) * sizeof(double), out, ((uint64_t)(rows - 1) * ldo + d) * sizeof(float)))
            return fail(UMLH_E_INVALID, "%s: out aliases the double source x (in place needs a float source)", who);
    } else if (out == x) {
        if (ldo != ldx) return fail(UMLH_E_INVALID, "%s: in place needs ldo == ldx (ldo=%lld ldx=%lld)", who, (long long)ldo, (long long)ldx);
    } else if (ranges_overlap(x, ((uint64_t)(rows - 1) * ldx + d) * sizeof(float), out, ((uint64_t)(rows - 1) * ldo + d) * sizeof(float))) {
        return fail(UMLH_E_INVALID, "%s: out overlaps x partially (in place needs out == x and ldo == ldx)", who);
    }
    RC(check_scratch(who, scratch, scratch_bytes, umlh_seqload_colnorm_bytes(rows, d), 8));
    HIPCHK(umlh_tab_launch_standardize(x, x_is_f64, rows, d, ldx, out, ldo, stats, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_tab_perturb(const float* src, int64_t n, int32_t d, int64_t lds, const uint8_t* drop, const uint8_t* carry, float p_drop,
                     float p_carry, uint64_t seed, float* dst, int64_t ldd, void* stream) {
    const char* who = "umlh_tab_perturb";
    if (!src || !dst) return fail(UMLH_E_INVALID, "%s: null pointer (src and dst are required)", who);
    if (n < 1 || n >= ROWS_END) return fail(UMLH_E_INVALID, "%s: n=%lld rows (need 1 <= n < 2^31)", who, (long long)n);
    if (d < 1 || d > SEQ_MAX_COLS) return fail(UMLH_E_INVALID, "%s: d=%d outside 1..%d", who, d, SEQ_MAX_COLS);
    if (lds < d) return fail(UMLH_E_INVALID, "%s: lds=%lld < d=%d", who, (long long)lds, d);
    if (ldd < d) return fail(UMLH_E_INVALID, "%s: ldd=%lld < d=%d", who, (long long)ldd, d);
    if (!(p_drop >= 0.f && p_drop <= 1.f)) return fail(UMLH_E_INVALID, "%s: p_drop=%g outside [0, 1]", who, (double)p_drop);
    if (!(p_carry >= 0.f && p_carry <= 1.f)) return fail(UMLH_E_INVALID, "%s: p_carry=%g outside [0, 1]", who, (double)p_carry);
    if (src == dst ? lds != ldd
                   : ranges_overlap(src, ((uint64_t)(n - 1) * lds + d) * sizeof(float), dst, ((uint64_t)(n - 1) * ldd + d) * sizeof(float)))
        return fail(UMLH_E_INVALID, "%s: dst overlaps src partially (in place needs dst == src and ldd == lds)", who);
    HIPCHK(umlh_tab_launch_perturb(src, n, d, lds, drop, carry, p_drop, p_carry, seed, dst, ldd, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_rows_gather(const float* const* srcs, const int32_t* widths, int32_t n_src, int64_t n, const int64_t* ids, int32_t b,
                     float* const* outs, void* stream) {
    const char* who = "umlh_rows_gather";
    if (!srcs || !widths || !outs || !ids) return fail(UMLH_E_INVALID, "%s: null pointer (srcs, widths, outs and ids are required)", who);
    if (n_src < 1 || n_src > UMLH_SEQ_GATHER_MAX_SOURCES)
        return fail(UMLH_E_INVALID, "%s: n_src=%d outside 1..%d", who, n_src, UMLH_SEQ_GATHER_MAX_SOURCES);
    if (n < 1 || n >= ROWS_END) return fail(UMLH_E_INVALID, "%s: n=%lld rows (need 1 <= n < 2^31)", who, (long long)n);
    if (b < 1 || b > SEQ_MAX_BATCH) return fail(UMLH_E_INVALID, "%s: b=%d outside 1..%d", who, b, SEQ_MAX_BATCH);
    int used = 0;
    for (int m = 0; m < n_src; ++m) {
        if (!srcs[m]) continue;
        ++used;
        if (!outs[m]) return fail(UMLH_E_INVALID, "%s: source %d has no destination", who, m);
        if (widths[m] < 1) return fail(UMLH_E_INVALID, "%s: widths[%d]=%d (need 1 <= width < 2^31)", who, m, widths[m]);
    }
    if (!used) return fail(UMLH_E_INVALID, "%s: every source is NULL", who);
    HIPCHK(umlh_tab_launch_gather(srcs, widths, n_src, n, ll(ids), b, outs, (hipStream_t)stream), who);
    return UMLH_OK;
}

// ---- the Gaussian toy's autoencoder (kernels: umlh_kernels_gauss.hip) ----
// the dimensions and the rows of both views against the envelope; 0 = fine.  who == NULL: silent (the size query)
static int check_ae_shape(const char* who, const umlh_ae_cfg_t* cfg, int32_t rows_x, int32_t rows_y, int32_t max_rows, const char* rx,
                          const char* ry) {
#define AE_FAIL(...) return who ? fail(UMLH_E_INVALID, __VA_ARGS__) : UMLH_E_INVALID
    if (!cfg) AE_FAIL("%s: cfg is NULL", who);
    if (cfg->dim_obs < 1 || cfg->dim_obs > UMLH_AE_MAX_OBS) AE_FAIL("%s: dim_obs=%d outside 1..%d", who, cfg->dim_obs, UMLH_AE_MAX_OBS);
    if (cfg->dim_common < 1 || cfg->dim_common > UMLH_AE_MAX_COMMON)
        AE_FAIL("%s: dim_common=%d outside 1..%d", who, cfg->dim_common, UMLH_AE_MAX_COMMON);
    if (cfg->dim_latent < 1 || cfg->dim_latent > UMLH_AE_MAX_LATENT)
        AE_FAIL("%s: dim_latent=%d outside 1..%d", who, cfg->dim_latent, UMLH_AE_MAX_LATENT);
    if (rows_x < 0 || rows_x > max_rows) AE_FAIL("%s: %s=%d outside 0..%d", who, rx, rows_x, max_rows);
    if (rows_y < 0 || rows_y > max_rows) AE_FAIL("%s: %s=%d outside 0..%d", who, ry, rows_y, max_rows);
    if (rows_x == 0 && rows_y == 0) AE_FAIL("%s: %s=0 and %s=0 (both views absent)", who, rx, ry);
#undef AE_FAIL
    return UMLH_OK;
}

static int check_ae_tensors(const char* who, const char* name, const float* const* t) {
    if (!t) return fail(UMLH_E_INVALID, "%s: %s is NULL (an array of 16 device pointers)", who, name);
    for (int i = 0; i < 16; ++i)
        if (!t[i]) return fail(UMLH_E_INVALID, "%s: %s[%d] is NULL", who, name, i);
    return UMLH_OK;
}

static int check_ae_table(const char* who, const char* name, const char* ldname, const float* table, int64_t ld, int32_t rows, int32_t d) {
    if (rows == 0) return UMLH_OK;
    if (!table) return fail(UMLH_E_INVALID, "%s: %s is NULL with %d rows asked for", who, name, rows);
    if (ld < d) return fail(UMLH_E_INVALID, "%s: %s=%lld < dim_obs=%d", who, ldname, (long long)ld, d);
    return UMLH_OK;
}

// the argument checks one run shares between the single-run entry points and the members of the grouped ones (who: the function,
// or the function and the member)
static int check_ae_forward_args(const char* who, const umlh_ae_cfg_t* cfg, const float* const* P, const float* x, int64_t ldx, int32_t n_x,
                                 const float* y, int64_t ldy, int32_t n_y) {
    RC(check_ae_shape(who, cfg, n_x, n_y, UMLH_AE_MAX_EVAL_ROWS, "n_x", "n_y"));
    RC(check_ae_tensors(who, "P", P));
    RC(check_ae_table(who, "x", "ldx", x, ldx, n_x, cfg->dim_obs));
    RC(check_ae_table(who, "y", "ldy", y, ldy, n_y, cfg->dim_obs));
    return UMLH_OK;
}

static int check_ae_train_args(const char* who, const umlh_ae_cfg_t* cfg, float* const* P, float* const* M, float* const* V, const float* x,
                               int64_t ldx, int32_t batch_x, const float* y, int64_t ldy, int32_t batch_y, int32_t n_steps,
                               int32_t backward_y, int32_t optimizer, const float* losses) {
    RC(check_ae_shape(who, cfg, batch_x, batch_y, UMLH_AE_MAX_BATCH, "batch_x", "batch_y"));
    if (n_steps < 1 || n_steps > UMLH_AE_MAX_BATCH) return fail(UMLH_E_INVALID, "%s: n_steps=%d outside 1..%d", who, n_steps, UMLH_AE_MAX_BATCH);
    if (backward_y != 0 && backward_y != 1) return fail(UMLH_E_INVALID, "%s: backward_y=%d (0: mode 'x', 1: mode 'xy')", who, backward_y);
    if (optimizer < UMLH_OPT_SGD || optimizer > UMLH_OPT_ADAMW) return fail(UMLH_E_INVALID, "%s: unknown optimizer %d", who, optimizer);
    RC(check_ae_tensors(who, "P", P));
    RC(check_ae_tensors(who, "M", M));
    if (optimizer != UMLH_OPT_SGD) RC(check_ae_tensors(who, "V", V));
    RC(check_ae_table(who, "x", "ldx", x, ldx, batch_x, cfg->dim_obs));
    RC(check_ae_table(who, "y", "ldy", y, ldy, batch_y, cfg->dim_obs));
    if (!losses) return fail(UMLH_E_INVALID, "%s: losses is NULL", who);
    return UMLH_OK;
}

uint64_t umlh_ae_scratch(const umlh_ae_cfg_t* cfg, int32_t rows_x, int32_t rows_y, int32_t train) {
    if (train != 0 && train != 1) return 0;
    if (check_ae_shape(nullptr, cfg, rows_x, rows_y, train ? UMLH_AE_MAX_BATCH : UMLH_AE_MAX_EVAL_ROWS, "", "")) return 0;
    return umlh_ae_plan_bytes(cfg, rows_x, rows_y, train);
}

int umlh_ae_forward(const umlh_ae_cfg_t* cfg, const float* const* P, const float* x, int64_t ldx, const int32_t* idx_x, int32_t n_x,
                    const float* y, int64_t ldy, const int32_t* idx_y, int32_t n_y, float* losses, float* rec_x, float* rec_y,
                    float* emb_x, float* emb_y, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_ae_forward";
    RC(check_ae_forward_args(who, cfg, P, x, ldx, n_x, y, ldy, n_y));
    if (!scratch) return fail(UMLH_E_INVALID, "%s: scratch is NULL", who);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_ae_plan_bytes(cfg, n_x, n_y, 0), 8));
    HIPCHK(umlh_ae_launch_forward(cfg, P, x, ldx, idx_x, n_x, y, ldy, idx_y, n_y, losses, n_x ? rec_x : nullptr, n_y ? rec_y : nullptr,
                                  n_x ? emb_x : nullptr, n_y ? emb_y : nullptr, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// part: 0 = whole steps (umlh_ae_train_steps); 1 / 2 = one launch of every step (umlh_ae_bench_steps)
static int ae_steps(const char* who, int part, const umlh_ae_cfg_t* cfg, float* const* P, float* const* M, float* const* V, const float* x,
                    int64_t ldx, const int32_t* idx_x, int32_t batch_x, const float* y, int64_t ldy, const int32_t* idx_y, int32_t batch_y,
                    int32_t n_steps, int32_t backward_y, float alpha_x, float alpha_y, int32_t optimizer, double lr, int64_t first_step,
                    double beta1, double beta2, double eps, double momentum, double weight_decay, float* losses, void* scratch,
                    uint64_t scratch_bytes, void* stream) {
    if (part < 0 || part > 2) return fail(UMLH_E_INVALID, "%s: part=%d outside 0..2", who, part);
    RC(check_ae_train_args(who, cfg, P, M, V, x, ldx, batch_x, y, ldy, batch_y, n_steps, backward_y, optimizer, losses));
    if (!scratch) return fail(UMLH_E_INVALID, "%s: scratch is NULL", who);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_ae_plan_bytes(cfg, batch_x, batch_y, 1), 8));
    for (int s = 0; s < n_steps; ++s) {
        const OptArgs o = standalone_opt(optimizer, lr, first_step + s, beta1, beta2, eps, momentum, weight_decay);
        HIPCHK(umlh_ae_launch_step(cfg, P, M, optimizer != UMLH_OPT_SGD ? V : nullptr, x, ldx, idx_x ? idx_x + (size_t)s * batch_x : nullptr,
                                   batch_x, y, ldy, idx_y ? idx_y + (size_t)s * batch_y : nullptr, batch_y, backward_y, alpha_x, alpha_y,
                                   &o, losses + (size_t)3 * s, scratch, part, (hipStream_t)stream), who);
    }
    return UMLH_OK;
}

int umlh_ae_train_steps(const umlh_ae_cfg_t* cfg, float* const* P, float* const* M, float* const* V, const float* x, int64_t ldx,
                        const int32_t* idx_x, int32_t batch_x, const float* y, int64_t ldy, const int32_t* idx_y, int32_t batch_y,
                        int32_t n_steps, int32_t backward_y, float alpha_x, float alpha_y, int32_t optimizer, double lr,
                        int64_t first_step, double beta1, double beta2, double eps, double momentum, double weight_decay,
                        float* losses, void* scratch, uint64_t scratch_bytes, void* stream) {
    return ae_steps("umlh_ae_train_steps", 0, cfg, P, M, V, x, ldx, idx_x, batch_x, y, ldy, idx_y, batch_y, n_steps, backward_y, alpha_x,
                    alpha_y, optimizer, lr, first_step, beta1, beta2, eps, momentum, weight_decay, losses, scratch, scratch_bytes, stream);
}

// ---- grouped forms: several runs in one launch pair per step ----
static int check_ae_group_count(const char* who, const void* items, int32_t n_items) {
    if (!items) return who ? fail(UMLH_E_INVALID, "%s: items is NULL", who) : UMLH_E_INVALID;
    if (n_items < 1 || n_items > UMLH_AE_MAX_GROUP)
        return who ? fail(UMLH_E_INVALID, "%s: n_items=%d outside 1..%d", who, n_items, UMLH_AE_MAX_GROUP) : UMLH_E_INVALID;
    return UMLH_OK;
}

// no device pointer occurs twice among the members' P / M / V (V of an sgd member is not looked at): every member's workgroups
// update its tensors in place while the others' run
static int check_ae_group_unique(const char* who, const umlh_ae_group_item_t* items, int32_t n_items) {
    struct Ref { const float* p; int member, set, index; };
    std::vector<Ref> refs;
    refs.reserve((size_t)n_items * 48);
    for (int i = 0; i < n_items; ++i) {
        float* const* sets[3] = {items[i].P, items[i].M, items[i].optimizer != UMLH_OPT_SGD ? items[i].V : nullptr};
        for (int k = 0; k < 3; ++k)
            for (int j = 0; sets[k] && j < 16; ++j) refs.push_back({sets[k][j], i, k, j});
    }
    std::sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) {
        return a.p != b.p ? std::less<const float*>()(a.p, b.p) : a.member != b.member ? a.member < b.member
               : a.set != b.set ? a.set < b.set : a.index < b.index;
    });
    for (size_t i = 1; i < refs.size(); ++i)
        if (refs[i].p == refs[i - 1].p)
            return fail(UMLH_E_INVALID, "%s: member %d: %c[%d] is also member %d's %c[%d] (members may not share parameter or moment tensors)",
                        who, refs[i].member, "PMV"[refs[i].set], refs[i].index, refs[i - 1].member, "PMV"[refs[i - 1].set], refs[i - 1].index);
    return UMLH_OK;
}

uint64_t umlh_ae_group_scratch(const umlh_ae_group_item_t* items, int32_t n_items, int32_t n_steps) {
    if (check_ae_group_count(nullptr, items, n_items)) return 0;
    if (n_steps < 1 || n_steps > UMLH_AE_MAX_BATCH) return 0;
    for (int i = 0; i < n_items; ++i)
        if (check_ae_shape(nullptr, &items[i].cfg, items[i].batch_x, items[i].batch_y, UMLH_AE_MAX_BATCH, "", "")) return 0;
    return umlh_ae_group_plan_bytes(items, n_items, n_steps);
}

uint64_t umlh_ae_eval_group_scratch(const umlh_ae_eval_item_t* items, int32_t n_items) {
    if (check_ae_group_count(nullptr, items, n_items)) return 0;
    for (int i = 0; i < n_items; ++i)
        if (check_ae_shape(nullptr, &items[i].cfg, items[i].n_x, items[i].n_y, UMLH_AE_MAX_EVAL_ROWS, "", "")) return 0;
    return umlh_ae_eval_group_plan_bytes(items, n_items);
}

// The one entry point of this file that allocates on the host: the [n_steps][n_items] optimizer constants are formed here, step by
// step as ae_steps forms them, and handed to the launcher, which stages them with the descriptors for one upload.
int umlh_ae_train_steps_grouped(const umlh_ae_group_item_t* items, int32_t n_items, int32_t n_steps, void* scratch, uint64_t scratch_bytes,
                                void* stream) {
    const char* who = "umlh_ae_train_steps_grouped";
    RC(check_ae_group_count(who, items, n_items));
    char member[64];
    for (int i = 0; i < n_items; ++i) {
        const umlh_ae_group_item_t& it = items[i];
        snprintf(member, sizeof(member), "%s: member %d", who, i);
        RC(check_ae_train_args(member, &it.cfg, it.P, it.M, it.V, it.x, it.ldx, it.batch_x, it.y, it.ldy, it.batch_y, n_steps, it.backward_y,
                               it.optimizer, it.losses));
    }
    RC(check_ae_group_unique(who, items, n_items));
    if (!scratch) return fail(UMLH_E_INVALID, "%s: scratch is NULL", who);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_ae_group_plan_bytes(items, n_items, n_steps), 8));
    std::vector<OptArgs> opt((size_t)n_steps * n_items);
    for (int s = 0; s < n_steps; ++s)
        for (int i = 0; i < n_items; ++i) {
            const umlh_ae_group_item_t& it = items[i];
            opt[(size_t)s * n_items + i] = standalone_opt(it.optimizer, it.lr, it.first_step + s, it.beta1, it.beta2, it.eps, it.momentum,
                                                          it.weight_decay);
        }
    HIPCHK(umlh_ae_launch_group(items, n_items, n_steps, opt.data(), scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

int umlh_ae_forward_grouped(const umlh_ae_eval_item_t* items, int32_t n_items, void* scratch, uint64_t scratch_bytes, void* stream) {
    const char* who = "umlh_ae_forward_grouped";
    RC(check_ae_group_count(who, items, n_items));
    char member[64];
    for (int i = 0; i < n_items; ++i) {
        const umlh_ae_eval_item_t& it = items[i];
        snprintf(member, sizeof(member), "%s: member %d", who, i);
        RC(check_ae_forward_args(member, &it.cfg, it.P, it.x, it.ldx, it.n_x, it.y, it.ldy, it.n_y));
    }
    if (!scratch) return fail(UMLH_E_INVALID, "%s: scratch is NULL", who);
    RC(check_scratch(who, scratch, scratch_bytes, umlh_ae_eval_group_plan_bytes(items, n_items), 8));
    HIPCHK(umlh_ae_launch_forward_group(items, n_items, scratch, (hipStream_t)stream), who);
    return UMLH_OK;
}

// benchmark only (umlh_launch.h): one launch of every step
extern "C" int umlh_ae_bench_steps(const umlh_ae_cfg_t* cfg, float* const* P, float* const* M, float* const* V, const float* x, long long ldx,
                                   const int* idx_x, int batch_x, const float* y, long long ldy, const int* idx_y, int batch_y, int n_steps,
                                   int backward_y, float alpha_x, float alpha_y, int optimizer, double lr, long long first_step,
                                   double beta1, double beta2, double eps, double momentum, double weight_decay, float* losses,
                                   void* scratch, unsigned long long scratch_bytes, int part, void* stream) {
    return ae_steps("umlh_ae_bench_steps", part, cfg, P, M, V, x, ldx, idx_x, batch_x, y, ldy, idx_y, batch_y, n_steps, backward_y, alpha_x,
                    alpha_y, optimizer, lr, first_step, beta1, beta2, eps, momentum, weight_decay, losses, scratch, scratch_bytes, stream);
}
