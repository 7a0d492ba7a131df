// Internal launch interface: every extern "C" function that a .hip file defines for the host code (kernel launchers and their
// *_config / *_bytes / *_tasks / *_supported helpers), declared exactly once.  Every file that defines one and every file that
// calls one includes this header, so a prototype that drifts from its definition is a compile error (the names are
// extern "C": a drifted prototype would still link).  Not part of the C ABI (include/umlh.h).
#pragma once
#include <atomic>
#include "umlh_common.h"
#include "umlh_micro.h"

// Scratch layouts of the metric launchers: every region starts on a 256-byte boundary; region `off` of a scratch block as T*.
inline long long align_up(long long x) { return (x + 255) / 256 * 256; }
template <class T>
inline T* at(void* scratch, long long off) { return reinterpret_cast<T*>(static_cast<char*>(scratch) + off); }
constexpr int UMLH_COLSTAT_CHUNKS = 256;       // most row chunks of the fp64 column statistics of the device loaders
struct ScratchLayout {                 // regions of one scratch block, each on a 256-byte boundary
    long long end;
    explicit ScratchLayout(long long start = 0) : end(start) {}      // start: a multiple of 256
    long long take(long long bytes) { const long long at = end; end += align_up(bytes); return at; }
};

// Raises Kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) to `bytes`, once per device: the attribute is per
// device, and bit d of the mask (one mask per kernel instantiation) says it is set on device d.  Returns 0 or the HIP error of
// hipGetDevice / hipFuncSetAttribute.  Called right before the launch it serves: a stream capture cannot set attributes, so a
// launcher's first call on a device must come outside one.
template <auto Kernel>
__attribute__((visibility("hidden"))) int raise_lds_limit(int bytes) {
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (!((done.load(std::memory_order_acquire) >> (dev & 63)) & 1ULL)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return (int)e;
        done.fetch_or(1ULL << (dev & 63), std::memory_order_release);
    }
    return 0;
}

extern "C" {
// ---- umlh_kernels_f32.hip: fp32 head step, generic fp32 GEMMs, optimizer / finalize kernels ----
int umlh_launch_w_shadow32(const float* w, float* dst, int C, int K, int cpad, hipStream_t stream);
int umlh_f32_fwd_config(int C, int* ctw, int* wc);
int umlh_f32_launch_fwd(const FwdArgs* a, int ctw, int wc, int grid, hipStream_t stream);
int umlh_f32_launch_gemm(const GemmArgs* g, int ta, int tb, int splits, hipStream_t stream);
int umlh_f32_launch_gemm_enc(const GemmArgs* g, int ta, int tb, int splits, hipStream_t stream);
int umlh_launch_reduce_update(int mode, const float* slabs, int n_slabs, long long slab_stride, long long n, float* grad_out,
                              float* p, float* m, float* v, const OptArgs* o, long long frozen_lo, long long frozen_hi,
                              hipStream_t stream);
int umlh_launch_multi_opt(int n, float* const* p, const float* const* g, float* const* m, float* const* v, const long long* cnt,
                          const OptArgs* o, hipStream_t stream);
int umlh_launch_head_step(const HeadFuse* hf, const DiagArgs* dg, float* shadow32, hipStream_t stream);
int umlh_launch_feistel_perm(long long n, unsigned long long seed, long long* out, hipStream_t stream);
int umlh_launch_index_block(IndexBlockArgs* a, hipStream_t stream);
int umlh_launch_finalize(const FinalizeArgs* f, hipStream_t stream);
int umlh_launch_zero_shot(const float* feats, const int64_t* labels, long long n, int d, int C, float* w, hipStream_t stream);
// ---- umlh_kernels_bf16.hip: bf16 head step ----
int umlh_launch_to_bf16(const float* src, void* dst, long long n, hipStream_t stream);
int umlh_launch_iota(long long* dst, long long n, hipStream_t stream);
int umlh_launch_w_shadow(const float* w, void* dst, int C, int K, int cpad, hipStream_t stream);
int umlh_bf16_fwd_ts(int wc, int stw);
int umlh_bf16_launch_fwd_q(const FwdArgsB* a, int nq, int tiles, hipStream_t stream);
int umlh_bf16_launch_fwd(const FwdArgsB* a, int ctw, int wc, int stw, int grid, hipStream_t stream);
int umlh_bf16_launch_transpose_shadow(const float* src, int R, int Cc, int ldd, void* dst, int mode, hipStream_t stream);
int umlh_bf16_step_tasks(int nfwd, int M, int N, int splits, long long n_head, int with_head);
int umlh_bf16_launch_step(const FwdArgsB* a, int ctw, int wc, int nfwd, const DwArgsB* g, int splits, unsigned* claim,
                          unsigned long long* done, unsigned* status, unsigned epoch, int ts, int total_cols,
                          const HeadFuse* hf, unsigned long long* timeline, int cus, int lazy, hipStream_t stream);
int umlh_bf16_launch_dw(const DwArgsB* g, int splits, int am, int om, hipStream_t stream);
// ---- umlh_kernels_micro.hip: micro-step path ----
int umlh_micro_chunking(int d, int* nch, int* cw);
int umlh_micro_bf16_supported(int nch, int cw);
int umlh_micro_launch(int nch, int cw, int bf16, const UmlhMicroHead* heads, int n_heads, int n_steps, int grid,
                      hipStream_t st);
// ---- umlh_p2p.hip: direct peer-to-peer all-reduce (its public entry points are in umlh.h) ----
int umlh_p2p_launch(void* const* regions, int n_ranks, int rank, float* msg, long long n, long long n_max, unsigned epoch,
                    hipStream_t st);
int umlh_p2p_status_offset(long long n_max, int n_ranks, unsigned long long* off);
// ---- umlh_kernels_seq.hip: sequence decoder MSE / InfoNCE ----
int umlh_seq_launch_fwd(const float* z, const float* w, const float* b, const float* x, const int64_t* lengths, int B, int T,
                        int Z, int D, float* recon, float* dres, float* row_partial, float* loss_cnt, hipStream_t st);
int umlh_seq_launch_bwd(const float* z, const float* w, const float* dres, const float* loss_cnt, const float* grad_out, int B,
                        int T, int Z, int D, float* dz, float* dw, float* db, int with_params, int dw_chunk, hipStream_t st);
int umlh_seq_launch_l2norm(const float* x, int n, int D, float* y, float* norm, hipStream_t st);
int umlh_seq_launch_nce_rows(float* dots, int n, float inv_temp, float* row_loss, float* loss, hipStream_t st);
int umlh_seq_launch_l2norm_bwd(const float* dy, const float* y, const float* norm, const float* grad_out, float scale, int n,
                               int D, float* dx, hipStream_t st);
// ---- umlh_kernels_enc.hip: MultiBench encoder layers ----
int umlh_enc_launch_bias_act(float* y, const float* b, long long M, int N, int relu, hipStream_t st);
int umlh_enc_launch_relu_bwd(const float* y, float* dy, long long n, hipStream_t st);
int umlh_enc_launch_dropout(float* x, long long n, float p, unsigned long long seed, hipStream_t st);
int umlh_enc_launch_add_inplace(float* y, const float* x, long long n, hipStream_t st);
int umlh_enc_launch_colsum(const float* x, int M, int N, float* out, hipStream_t st);
int umlh_enc_launch_add_layernorm(const float* x, const float* r, const float* gamma, const float* beta, int M, int N,
                                  float eps, float* s_out, float* y, float* mean, float* rstd, hipStream_t st);
int umlh_enc_launch_layernorm_bwd(const float* dy, const float* s, const float* gamma, const float* mean, const float* rstd,
                                  int M, int N, float* ds, float* dgamma, float* dbeta, hipStream_t st);
// out[m*ldo + n] (m < M, n < N) = epilogue(sum of ns slabs) (slab s at slabs + s*stride, same row stride ldo); columns [N, ldo)
// untouched.  e may be NULL (none); an epilogue indexes dense [M, N] buffers: hipErrorInvalidValue for one at ldo != N
int umlh_enc_launch_reduce_slabs(const float* slabs, int ns, long long stride, int M, int N, int ldo, const Epilogue* e, float* out,
                                 hipStream_t st);
int umlh_enc_launch_add_layernorm_fused(const float* x, int ns, long long stride, const Epilogue* e, const float* gamma,
                                        const float* beta, int M, int N, float eps, float* s_out, float* y, float* mean,
                                        float* rstd, hipStream_t st);
int umlh_enc_launch_layernorm_bwd_rows_fused(const float* dy, int ns, long long stride, const float* add, float* dy_out,
                                             const float* s, const float* gamma, const float* mean, const float* rstd, int M,
                                             int N, float* ds, float* dsd, float p, unsigned long long seed,
                                             const unsigned long long* seed_ptr, hipStream_t st);
int umlh_enc_launch_colsum_partial(const float* x, int M, int N, int chunk, float* part, hipStream_t st);
int umlh_enc_launch_ln_cols_partial(const float* dy, const float* s, const float* mean, const float* rstd, const float* dsd,
                                    int M, int N, int chunk, float* part_g, float* part_b, float* part_d, hipStream_t st);
int umlh_enc_launch_multi_reduce(MultiReduceArgs* a, hipStream_t st);
int umlh_enc_launch_set_u64(unsigned long long* dst, unsigned long long v, hipStream_t st);
float umlh_enc_drop_inv_keep(float p);
unsigned umlh_enc_drop_thresh(float p);
int umlh_enc_launch_add_pos(float* x, const float* pos, int T, int B, int Z, hipStream_t st);
int umlh_enc_launch_pos_grad(const float* dx, int T, int B, int Z, float* dpos, hipStream_t st);
int umlh_enc_launch_gather_rows(const float* x, const int64_t* idx, int n, int Z, float* out, int scatter, hipStream_t st);
int umlh_enc_launch_attention_fwd(const float* qkv, const int64_t* lengths, int T, int B, int Z, int H, float p,
                                  unsigned long long seed, const unsigned long long* seed_ptr, float* ctx, float* lse,
                                  hipStream_t st);
int umlh_enc_launch_attention_bwd(const float* qkv, const int64_t* lengths, const float* lse, const float* dctx, int T, int B,
                                  int Z, int H, float p, unsigned long long seed, const unsigned long long* seed_ptr,
                                  float* dqkv, hipStream_t st);
// ---- umlh_kernels_align.hip: alignment metrics ----
int umlh_align_knn_splits(long long n, int splits);
unsigned long long umlh_align_knn_bytes(long long n, int topk, int splits);
unsigned long long umlh_align_mutual_bytes(long long n);
unsigned long long umlh_align_cka_bytes(long long n, int da, int db, int splits);
int umlh_align_launch_knn(const float* x, long long n, int d, int ldx, int topk, int splits, int* knn, float* scores,
                          void* scratch, hipStream_t st);
int umlh_align_launch_mutual(const int* ka, const int* kb, long long n, int topk, double* out, void* scratch, hipStream_t st);
int umlh_align_launch_cka(const float* a, int lda, int da, const float* b, int ldb, int db, long long n, int splits,
                          double* out4, void* scratch, hipStream_t st);
int umlh_align_cka_sum_chunks(long long n);
long long umlh_align_cka_tile_sq_offset(long long n, int da, int db, int splits);
int umlh_align_launch_colsum(const float* a, int lda, int da, const float* b, int ldb, int db, long long n, double* partial,
                             hipStream_t st);
int umlh_align_launch_cka_products(const float* a, int lda, int da, const float* b, int ldb, int db, long long n, int splits,
                                   void* scratch, hipStream_t st);
// grouped form: n pairs in one fixed train of launches (the plan is that of the size query)
unsigned long long umlh_align_pairs_bytes(const umlh_align_pair_t* items, int n, int splits);
int umlh_align_launch_pairs(const umlh_align_pair_t* items, int n, int splits, void* scratch, hipStream_t st);
// ---- umlh_kernels_align_ext.hip: unbiased / RBF CKA, CKNNA, k-NN list statistics ----
unsigned long long umlh_align_ext_cka_unbiased_bytes(long long n, int da, int db, int splits);
unsigned long long umlh_align_ext_rbf_bytes(long long n, int da, int db, int splits);
unsigned long long umlh_align_ext_cknna_bytes(long long n);
unsigned long long umlh_align_ext_list_bytes(long long n);
int umlh_align_ext_launch_cka_unbiased(const float* a, int lda, int da, const float* b, int ldb, int db, long long n, int splits,
                                       double* out4, void* scratch, hipStream_t st);
int umlh_align_ext_launch_rbf(const float* a, int lda, int da, const float* b, int ldb, int db, long long n, double sigma,
                              int unbiased, int splits, double* out4, void* scratch, hipStream_t st);
int umlh_align_ext_launch_cknna(const int* ka, const float* sa, const int* kb, const float* sb, long long n, int topk, double* out4,
                                void* scratch, hipStream_t st);
int umlh_align_ext_launch_list_stats(const int* ka, const int* kb, long long n, int topk, int* rows, double* out3, void* scratch,
                                     hipStream_t st);
// ---- umlh_kernels_probe.hip: linear probes ----
unsigned long long umlh_probe_fit_bytes(long long n, int d, int max_iter);
unsigned long long umlh_probe_stats_bytes(int d);
int umlh_probe_launch_masked_mean(const float* z, int B, int T, int Z, long long ldb, long long ldt, const long long* lengths,
                                  float* out, int ldo, hipStream_t st);
int umlh_probe_launch_stats(const float* x, long long n, int d, int ldx, double* stats, void* scratch, hipStream_t st);
// the first pass of umlh_probe_launch_stats alone: mean[d], same scratch
int umlh_probe_launch_means(const float* x, long long n, int d, int ldx, double* mean, void* scratch, hipStream_t st);
int umlh_probe_launch_fit(const float* x, long long n, int d, int ldx, const int* y, const double* stats, int kind, double c,
                          int max_iter, double gtol, double* coef, umlh_probe_record_t* rec, double* objectives, void* scratch,
                          hipStream_t st);
int umlh_probe_launch_score(const float* x, long long n, int d, int ldx, const double* stats, const double* coef, const int* y,
                            long long* correct, float* decision, hipStream_t st);
// ---- umlh_kernels_softmax_probe.hip: multinomial logistic probe ----
unsigned long long umlh_softmax_probe_bytes(long long n, int d, int n_class, int fit, int history);     // fit = 0: the evaluation
int umlh_softmax_probe_launch_eval(const float* x, long long n, int d, int ldx, const int* y, const double* stats, int n_class, double c,
                                   float* coef, int ldc, double* objective, float* grad, int ldg, double* max_grad, void* scratch,
                                   hipStream_t st);
int umlh_softmax_probe_launch_fit(const float* x, long long n, int d, int ldx, const int* y, const double* stats, int n_class, double c,
                                  int max_iter, int history, double gtol, int init, float* coef, int ldc, umlh_probe_record_t* rec,
                                  double* objectives, void* scratch, hipStream_t st);
int umlh_softmax_probe_launch_fold(const float* coef, int ldc, int n_class, int d, const double* stats, float* w, int ldw, float* bias,
                                   hipStream_t st);
// ---- umlh_kernels_knn.hip: k-nearest-neighbour probe ----
unsigned long long umlh_knn_bytes(long long nt, long long nq, int k, int splits);
int umlh_knn_launch_search(const float* train, long long nt, int ldt, const float* query, long long nq, int ldq, int d, int k,
                           int splits, int* idx, float* dist, void* scratch, hipStream_t st);
int umlh_knn_launch_vote(const int* idx, long long nq, int k, const int* labels, long long nt, const int* y, int* pred, int* votes,
                         long long* correct, hipStream_t st);
// ---- umlh_kernels_spectral.hip: fp64 Gram, symmetric eigenvalues, singular values and effective rank ----
int umlh_spectral_chunks(int batch, long long n);
unsigned long long umlh_spectral_bytes(int batch, long long n, int d);
int umlh_spectral_launch(const float* a, int batch, long long rows, int period, long long sm, long long so, long long si,
                         const long long* lengths, int drop_last, int d, double eps, double* erank, double* rows_out, double* sv,
                         int sv_ld, void* scratch, hipStream_t st);
// top-q eigenpairs of a feature Gram and SVCCA; d_b = 0 in umlh_subspace_bytes: the single-matrix op
unsigned long long umlh_subspace_bytes(long long n, int da, int db, int q);
int umlh_subspace_launch(const float* a, long long n, int d, long long ld, int q, int standardize, double* evals, double* evecs,
                         void* scratch, hipStream_t st);
int umlh_svcca_launch(const float* a, const float* b, long long n, int da, int db, long long lda, long long ldb, int q, double* out,
                      double* rho, double* evals, void* scratch, hipStream_t st);
// ---- umlh_kernels_capture.hip: ragged row compaction, mean paired cosine ----
unsigned long long umlh_capture_cosine_bytes(long long n);
int umlh_capture_launch_compact(const float* z, int B, int T, int d, long long ldb, long long ldt, const long long* lengths,
                                int drop_last, float* out, long long ldo, long long out_rows, long long* rows_total, hipStream_t st);
int umlh_capture_launch_cosine(const float* a, long long lda, const float* b, long long ldb, long long n, int d, double eps,
                               double* out2, float* rows, void* scratch, hipStream_t st);
// ---- umlh_kernels_classstats.hip: stable counting sort of rows by label, per-class mean rows and in-class distances ----
unsigned long long umlh_classindex_bytes(long long n, int n_class);      // 0: the block-by-class count table would pass 1 GiB
int umlh_classindex_launch(const long long* labels, long long n, int n_class, int* order, long long* offsets, void* scratch,
                           hipStream_t st);
unsigned long long umlh_classstats_bytes(long long n, int d, int n_class);
int umlh_classstats_launch(const float* feats, long long ld, long long n, int d, const int* order, const long long* offsets,
                           int n_class, float* means, long long ld_means, double* dist, double* out2, void* scratch, hipStream_t st);
// ---- umlh_kernels_evalreport.hip: top-k classes per row, class-wise counters ----
unsigned long long umlh_evalreport_bytes(long long n, long long C, int k, int splits);
int umlh_evalreport_launch_topk(const float* x, long long n, int ldx, const float* w, long long C, int ldw, int d, const float* bias,
                                const float* scale, int k, int splits, int* cls, float* logit, void* scratch, hipStream_t st);
int umlh_evalreport_launch_classwise(const int* cls, long long n, int k, const long long* labels, long long C, long long* support,
                                     long long* hit1, long long* hitk, long long* confusion, long long* misc, hipStream_t st);
// ---- umlh_kernels_stepstats.hip: per-step logged statistics (trivial next-frame error, masked reconstruction error) ----
long long umlh_stepstats_partials(int B, int T, int d);       // partial sums of one call; -1: more than the final kernel takes
unsigned long long umlh_stepstats_bytes(int B, int T, int d);
int umlh_stepstats_launch(const float* x, long long ldb, long long ldt, const float* recon, long long ldb_r, long long ldt_r, int B, int T,
                          int d, const long long* lengths, double* out4, void* scratch, hipStream_t st);
// ---- umlh_kernels_rollout.hip: one-launch rollout, spectral-bias spectra ----
unsigned long long umlh_rollout_lds_bytes(int Z, int dff, int D);
int umlh_rollout_launch(const umlh_rollout_cfg_t* cfg, const float* const* P, const float* conv_w, const float* pos0, const float* w_in,
                        const float* b_in, const float* w_out, const float* b_out, const float* x0, long long ldx, long long n, float* out,
                        long long ldb, long long ldt, hipStream_t st);
long long umlh_spectrum_partials(int B, int T, int d);        // partial vectors of one call; -1: more than the final kernel takes
unsigned long long umlh_spectrum_bytes(int B, int T, int d);
int umlh_spectrum_launch(const float* x, long long ldb, long long ldt, int B, int T, int d, double* out, void* scratch, hipStream_t st);
// ---- umlh_kernels_outlier.hip: row quantile and global k-th of |x|, clamp (+ row normalisation), k-NN accuracy ----
unsigned long long umlh_outlier_quantile_bytes(long long n);
unsigned long long umlh_outlier_kth_bytes(void);
unsigned long long umlh_outlier_accuracy_bytes(long long n);
int umlh_outlier_launch_quantile(const float* x, long long n, int d, long long ld, int lo, int hi, double frac, float* lo_val,
                                 float* hi_val, float* quant, double* mean64, float* q_val, void* scratch, hipStream_t st);
int umlh_outlier_launch_kth(const float* x, long long n, long long d, long long ld, long long k, float* out, void* scratch,
                            hipStream_t st);
int umlh_outlier_launch_clamp(const float* x, long long n, int d, long long ldx, const float* q_val, int normalize, float* out,
                              long long ldo, hipStream_t st);
int umlh_outlier_launch_accuracy(const int* knn, long long n, long long m, long long ld, double* out, void* scratch, hipStream_t st);
// ---- umlh_kernels_seqload.hip: device loader of the affect datasets (first nonzero row, two standardisations, batch gather-pad) ----
unsigned long long umlh_seqload_colnorm_bytes(long long rows, int d);
// the final kernel of the column statistics: the `chunks` partials of every column in chunk order -> stats[c] = mean (pass 0),
// stats[d + c] = population std (pass 1).  Shared with umlh_kernels_tabular.hip, whose plan is the same min(rows,
// UMLH_COLSTAT_CHUNKS) row chunks in one region of doubles
int umlh_seqload_launch_stats_final(const double* partial, long long rows, int d, int chunks, int pass, double* stats, hipStream_t st);
int umlh_seqload_launch_first_row(const float* x, long long n, int T, int D, int* start, hipStream_t st);
int umlh_seqload_launch_colnorm(const float* x, long long rows, int d, long long ldx, float* out, long long ldo, double* stats,
                                void* scratch, hipStream_t st);
int umlh_seqload_launch_znorm(float* x, long long n, int T, int d, const int* start, hipStream_t st);
// srcs, dims, outs: host arrays of n_src entries; a NULL source is skipped
int umlh_seqload_launch_gather_pad(const float* const* srcs, const int* dims, int n_src, long long n, int T, const int* start,
                                   const long long* ids, int B, int t_out, float* const* outs, long long* lengths, hipStream_t st);
// per_step: the unit of one eps / keep draw is a row (else a sample); eps, keep and start_out may be NULL; dst may be src
int umlh_seqload_launch_perturb(const float* src, long long n, int T, int D, int per_step, const double* eps, const unsigned char* keep,
                                float elem_p, unsigned long long seed, float* dst, int* start_out, hipStream_t st);
// ---- umlh_kernels_tabular.hip: MIMIC loader (standardisation of a cleaned float / double table, tabular noise, row gather) ----
// scratch: umlh_seqload_colnorm_bytes(rows, d)
int umlh_tab_launch_standardize(const void* x, int x_is_f64, long long rows, int d, long long ldx, float* out, long long ldo,
                                double* stats, void* scratch, hipStream_t st);
// drop [n, d] and carry [n, d - 1] may be NULL: then p_drop / p_carry of the counter streams seed / seed + 1; dst may be src
int umlh_tab_launch_perturb(const float* src, long long n, int d, long long lds, const unsigned char* drop, const unsigned char* carry,
                            float p_drop, float p_carry, unsigned long long seed, float* dst, long long ldd, hipStream_t st);
// srcs, widths, outs: host arrays of n_src entries; a NULL source is skipped
int umlh_tab_launch_gather(const float* const* srcs, const int* widths, int n_src, long long n, const long long* ids, int B,
                           float* const* outs, hipStream_t st);
// ---- umlh_kernels_gauss.hip: the Gaussian toy's autoencoder (forward; one training step = launch A + launch B) ----
unsigned long long umlh_ae_plan_bytes(const umlh_ae_cfg_t* cfg, int rows_x, int rows_y, int train);
int umlh_ae_launch_forward(const umlh_ae_cfg_t* cfg, const float* const* P, const float* x, long long ldx, const int* idx_x, int n_x,
                           const float* y, long long ldy, const int* idx_y, int n_y, float* losses, float* rec_x, float* rec_y,
                           float* emb_x, float* emb_y, void* scratch, hipStream_t st);
int umlh_ae_launch_step(const umlh_ae_cfg_t* cfg, float* const* P, float* const* M, float* const* V, const float* x, long long ldx,
                        const int* idx_x, int batch_x, const float* y, long long ldy, const int* idx_y, int batch_y, int backward_y,
                        float alpha_x, float alpha_y, const OptArgs* o, float* losses, void* scratch, int part, hipStream_t st);
// grouped forms: n members in one launch pair per step.  opt: HOST [n_steps][n] optimizer constants, member i of step s at s * n + i
unsigned long long umlh_ae_group_plan_bytes(const umlh_ae_group_item_t* items, int n, int n_steps);
unsigned long long umlh_ae_eval_group_plan_bytes(const umlh_ae_eval_item_t* items, int n);
int umlh_ae_launch_group(const umlh_ae_group_item_t* items, int n, int n_steps, const OptArgs* opt, void* scratch, hipStream_t st);
int umlh_ae_launch_forward_group(const umlh_ae_eval_item_t* items, int n, void* scratch, hipStream_t st);
// ---- umlh_ops.cpp, for scripts/bench_gaussian.py alone ----
// umlh_ae_train_steps with its checks, launching only a part of every step: part 1 = launch A alone, 2 = launch B alone on the
// scratch an earlier whole step left, 0 = whole steps.  NOT a training call (with part 1 the weights never change, with part 2
// they move along a stale gradient) and not part of the C ABI: it exists so that the two launches can be timed apart, and nothing
// in the environment can make umlh_ae_train_steps do this.
int umlh_ae_bench_steps(const umlh_ae_cfg_t* cfg, float* const* P, float* const* M, float* const* V, const float* x, long long ldx,
                        const int* idx_x, int batch_x, const float* y, long long ldy, const int* idx_y, int batch_y, int n_steps,
                        int backward_y, float alpha_x, float alpha_y, int optimizer, double lr, long long first_step, double beta1,
                        double beta2, double eps, double momentum, double weight_decay, float* losses, void* scratch,
                        unsigned long long scratch_bytes, int part, void* stream);

// ---- umlh_api.cpp, for umlh_encoder.cpp ----
// out[M,N] (ldo == N) = epilogue(A B^T) with the operand layouts of umlh_gemm_f32.  `splits` K-slabs go to `slabs`
// ([ns][M*N], ns returned in *ns_out).  defer != 0: the raw slabs (ns >= 1) are left for the consumer, `out` and `epi` unused;
// else one slab applies `epi` in the GEMM, more launch the slab reduction with `epi`.
int umlh_gemm_f32_epi(const float* A, const float* B, float* out, int M, int N, int K, int lda, int ldb, int ta, int tb,
                      const Epilogue* epi, int splits, float* slabs, int defer, int* ns_out, hipStream_t stream);
}
