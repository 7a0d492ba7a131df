/*
 * umlh.h -- C ABI of the MI355X-native UML head fine-tune hot path.
 *
 * The reference (OEmiliatanO/Unpaired-Multimodal-Learning) has no FFI / plugin
 * boundary: the hot path sits behind a Python duck-typed contract between
 * vision_language/finetune.py:train() and the model / optimizer / scheduler /
 * loader objects it is handed.  This header is the
 * boundary a maintainer binds underneath that contract (ctypes stub in
 * INTEGRATION.md).  Each entry point cites the reference lines it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *   - plain C types only; every pointer marked "device" is HIP device memory
 *     owned by the caller (torch allocates it); the library never allocates,
 *     frees or synchronises, so every call is graph-capturable (on a capturing stream the bf16 step takes its
 *     launch-per-kernel form: the one-launch step tags its in-launch hand-offs with a per-launch argument; the
 *     single-launch micro path and the opt-in 2-D forward use such tags too and are not meant for capture).
 *   - every function returns 0 on success or a negative UMLH_E_* code;
 *     umlh_last_error() returns a thread-local message for the last failure.
 *   - all work is enqueued on the hipStream_t passed as `void* stream`
 *     (asynchronous w.r.t. the host); a handle is not thread-safe.
 *   - features are row-major fp32 [rows, dim]; labels are int64 (torch.long);
 *     optional `index` (int64) gathers rows from a device-resident table, which
 *     replaces the DataLoader collate of finetune.py:33-39,165-172.
 *
 * Environment switches read by the library (tuning / analysis; defaults are the measured-fastest settings; the table
 * tests/_switches.py names the line that reads each one, and a test holds it and this list to the source).
 * Read when a handle is created or its workspace is sized (umlh_create, umlh_workspace_bytes): a process may create
 * handles under different settings.
 *   UMLH_BF16_FUSE=2|1|0 bf16 mode, linear head: the whole step as one launch (step_bf16, default) | forward + dW as one
 *                        launch (fwd_dw_bf16) + the update kernel | three launches
 *   UMLH_BF16_FWD2D=1    bf16 mode: the 2-D forward (128-row tiles x 256-class groups, in-launch softmax merge); slower at cfg2
 *   UMLH_BF16_STW=2      bf16 mode: two sample tiles per wave of the 1-D forward
 *   UMLH_MICRO=0         never take the single-launch micro step
 *   UMLH_STEP_GRID=n     bf16 mode: the one-launch step on n workgroups instead of one per compute unit
 *   UMLH_STEP_LAZY=1     bf16 mode: every fourth workgroup of the one-launch step leaves its home tiles to whoever needs them
 *   UMLH_FORCE_DP=1      take the data-parallel split step (grad -> all-reduce -> update) with one rank
 *   UMLH_DBG_FWD / UMLH_DBG_DW / UMLH_DBG_STEP   in-kernel stamps (scripts/fwd_stamps.py, dw_stamps.py, step_timeline.py)
 * Those below are read once per process, at the first call that needs them: another value takes a fresh process.
 *   UMLH_WT=0            plain instead of write-through (sc1) stores for what a kernel hands to the next launch
 *   UMLH_F32_X3=0        fp32 mode: products on the fp32 MFMA instead of three-way bf16 splits on the bf16 MFMA
 *   UMLH_F32_FWD=1       fp32 forward stages W through LDS chunk by chunk instead of streaming its fragment-major shadow
 *   UMLH_F32_DW=0        fp32 dW through the generic GEMM instead of dw_f32
 *   UMLH_F32_TM=1|2      fp32 GEMM: force the 64 x 64 | 128 x 128 tile (tuning runs)
 *   UMLH_ENC_GRAPH=0     encoder plans: no HIP-graph replay
 *   UMLH_ENC_SPLIT_WGS=n encoder GEMMs: split K until about n workgroups are in flight (default 768)
 *   UMLH_DBG_MICRO       in-kernel stamps of the micro step (scripts/micro_stamps.py)
 *   UMLH_DBG_GEMM_STAMPS / UMLH_DBG_GEMM_CALL   analysis builds only, read at every gemm_enc launch: address of a stamp
 *                        buffer and the index of the launch to stamp
 */
#ifndef UMLH_H
#define UMLH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UMLH_OK              0
#define UMLH_E_INVALID      -1   /* bad argument / unsupported shape            */
#define UMLH_E_UNBOUND      -2   /* umlh_bind() not called / workspace too small */
#define UMLH_E_HIP          -3   /* a HIP runtime call failed                   */
#define UMLH_E_NOGPU        -4   /* no gfx950 device visible                    */

/* engine/optimizer/optim.py:6,15-31 AVAI_OPTIMS */
#define UMLH_OPT_SGD   0   /* torch.optim.SGD(momentum=0.9, nesterov=False)  optim.py:34-48 */
#define UMLH_OPT_ADAM  1   /* torch.optim.Adam(betas=(0.9,0.999))            optim.py:50-59 */
#define UMLH_OPT_ADAMW 2   /* torch.optim.AdamW(betas=(0.9,0.999))           optim.py:61-71 */

#define UMLH_PREC_FP32 0   /* fp32 operands, fp32 results: the parity mode (logits / loss 1e-4).  The fused step forms its products
                            * from three-way bf16 splits of both operands on the bf16 MFMA (six exact piece products per product, fp32
                            * accumulation; what is dropped is 2^-24 of a product rms, 2^-20 worst case: as accurate against float64 as the fp32 MFMA chain) -- or, with UMLH_F32_X3=0 in the environment, on
                            * the f32-input MFMA as in ABI <= 3.  umlh_logits, umlh_project and umlh_gemm_f32 use the same x3 form on the
                            * 128x128 gemm_f32 tile (chosen once its grid reaches 768 workgroups, split-K slabs counted) and in dw_f32x3;
                            * smaller grids and the dense encoder GEMMs use the f32-input MFMA.  Both forms meet the same accuracy
                            * criterion against float64 (tests/_gemm_ref.py).  So a row's logits can differ in the last bits with the
                            * batch size.  An infinite operand on an x3 path gives NaN, not +-inf (its mid piece is inf - inf): a
                            * non-finite input still never gives a finite output, and NaN stays NaN. */
#define UMLH_PREC_BF16 1   /* bf16 operands, fp32 accumulate: the throughput mode         */

typedef struct umlh_handle_s* umlh_handle_t;

/* Shape + optimizer of one head.  Mirrors the constructor arguments of
 * engine/models/head.py:39-70 (UML) / :101-125 (UMLClip) and of
 * engine/optimizer/optim.py:15 build_optimizer. */
typedef struct {
    int32_t d_img;          /* image feature dim (vision_model.num_features)                 */
    int32_t d_shared;       /* head input dim (text_indim if has_proj else d_img)            */
    int32_t num_classes;    /* C, 1..1024                                                    */
    int32_t has_proj;       /* 1: img_proj Linear(d_img -> d_shared, bias=False) head.py:64-66 */
    int32_t learnable_temp; /* 1: img_scale / txt_scale are parameters        head.py:69-70 */
    int32_t optimizer;      /* UMLH_OPT_*                                                    */
    int32_t precision;      /* UMLH_PREC_*                                                   */
    int32_t max_rows_img;   /* per-step row capacity, image modality                         */
    int32_t max_rows_txt;   /* per-step row capacity, text modality                          */
    double  beta1, beta2, eps, momentum, weight_decay;  /* python floats of optim.py:9,12 */
} umlh_config_t;

/* Caller-owned device state (torch tensors): parameters in reference
 * parameters() order img_proj.weight, head.weight, img_scale, txt_scale, and the
 * optimizer state torch.optim keeps for each (exp_avg / momentum_buffer, exp_avg_sq). */
typedef struct {
    float* w_head;  float* m_head;  float* v_head;     /* [C, d_shared]                    */
    float* w_proj;  float* m_proj;  float* v_proj;     /* [d_shared, d_img] or NULL        */
    float* scales;  float* m_scales; float* v_scales;  /* [2] = {img_scale, txt_scale}     */
    void*    workspace;                                /* >= umlh_workspace_bytes(cfg)     */
    uint64_t workspace_bytes;
} umlh_buffers_t;

/* One modality's rows for one step: what fetch_next() + .to(device) deliver in
 * finetune.py:164-174, as (table, index) instead of a collated copy. */
typedef struct {
    const float*   feats;       /* device [table_rows, dim] fp32                           */
    const int64_t* labels;      /* device [table_rows]                                     */
    const int64_t* index;       /* device [rows] row ids into feats/labels, NULL = 0..rows-1 */
    int32_t        rows;        /* rows processed by THIS rank in this step (0 = absent)   */
    int32_t        global_rows; /* denominator of the CE mean: rows summed over all ranks  */
    const void*    feats_bf16;  /* device [table_rows, dim] bf16 copy of feats (umlh_to_bf16);
                                   required by train/grad/eval calls in UMLH_PREC_BF16 mode  */
} umlh_batch_t;

/* Per-step scalars: lr = scheduler value used by this optimizer.step()
 * (engine/optimizer/scheduler.py:58-81), step = 1-based count of optimizer steps
 * (Adam bias correction), alpha = text loss weight (finetune.py:188). */
typedef struct {
    double  lr;
    int64_t step;
    float   alpha;      /* weight of the text CE   (args.alpha)      finetune.py:188 */
    float   img_alpha;  /* weight of the image CE  (img_alpha = 1.0) finetune.py:160 */
    int32_t flags;      /* UMLH_F_* */
    int32_t reserved;
} umlh_hyper_t;
/* The caller guarantees that w_head has not been written by anyone but this handle since its
 * last umlh_apply_update / umlh_train_step: the bf16 weight shadow the update kernel produced
 * may be reused instead of rebuilt (bf16 mode only; default is to rebuild on every call). */
#define UMLH_F_WEIGHTS_UNCHANGED 1

/* Device float[UMLH_N_SCALARS] written by train/grad/eval calls. */
#define UMLH_S_LOSS_IMG   0   /* mean CE over image rows   finetune.py:186 */
#define UMLH_S_LOSS_TXT   1   /* mean CE over text rows    finetune.py:187 */
#define UMLH_S_ACC_IMG    2   /* top-1 accuracy, image     finetune.py:197 */
#define UMLH_S_ACC_TXT    3   /* top-1 accuracy, text      finetune.py:198 */
#define UMLH_S_GSCALE_IMG 4   /* d loss / d img_scale                      */
#define UMLH_S_GSCALE_TXT 5   /* d loss / d txt_scale                      */
#define UMLH_S_CORRECT    6   /* eval: number of correct rows (as float)   */
#define UMLH_S_LOSS_SUM   7   /* eval: sum of per-row CE                   */
/* Per-step gradient diagnostics (finetune.py:190-191,203-206,238): raw sums over all C*d elements
 * of the UNWEIGHTED per-modality head gradients g_img = dL_img/dW, g_txt = dL_txt/dW -- by-products
 * of the split-K slab reduction (image and text rows occupy separate slabs).  Written by
 * umlh_train_step(s) after umlh_enable_diagnostics(h, 1) (off by default: the accumulation costs
 * about 2.5 us per step at C*d = 512 000) when d_shared % 8 == 0; left untouched by umlh_eval_batch; in the
 * data-parallel split they are written by umlh_apply_update from the all-reduced per-modality gradients (the message
 * then carries g_img and g_txt separately); zero for a modality whose loss weight is 0.  The caller forms
 *   grad_direction_sim = DOT / sqrt(N2_IMG * N2_TXT),  img_grad_norm = sqrt(N2_IMG),
 *   txt_grad_norm = sqrt(N2_TXT),  grad_agreement_rate = AGREE / (C * d). */
#define UMLH_S_GRAD_DOT      8   /* sum g_img * g_txt                          */
#define UMLH_S_GRAD_N2_IMG   9   /* sum g_img^2                                */
#define UMLH_S_GRAD_N2_TXT   10  /* sum g_txt^2                                */
#define UMLH_S_GRAD_AGREE    11  /* #elements with sign(g_img) == sign(g_txt)  */
#define UMLH_N_CORE_SCALARS  8
#define UMLH_N_SCALARS    12

const char* umlh_last_error(void);
int  umlh_version(void);        /* ABI revision: 3 = round 2 (grouped / micro / data-parallel / encoder-plan / InfoNCE entry points); 4 = round 3 (umlh_step_status / umlh_step_launches, umlh_p2p_*); 5 = umlh_align_* (CKA, k-NN, mutual k-NN); 6 = umlh_masked_mean, umlh_probe_* (linear probes of MultiBench evaluate); 7 = umlh_align_cka_unbiased / _cka_rbf / _cknna / _list_stats; 8 = umlh_spectral_scratch_bytes, umlh_svdvals, umlh_effective_rank, umlh_effective_rank_seq; 9 = umlh_subspace_scratch_bytes, umlh_principal_subspace, umlh_svcca; 10 = umlh_seq_compact, umlh_paired_cosine_scratch_bytes, umlh_paired_cosine; 11 = umlh_seq_step_stats_scratch_bytes, umlh_seq_step_stats */

/* Bytes of workspace a handle with this config needs (0 on invalid config). */
uint64_t umlh_workspace_bytes(const umlh_config_t* cfg);

int  umlh_create(const umlh_config_t* cfg, umlh_handle_t* out);
int  umlh_destroy(umlh_handle_t h);
/* Attach parameter / optimizer-state / workspace buffers (state_dict round trips
 * stay on the torch side: finetune.py:249,274). */
int  umlh_bind(umlh_handle_t h, const umlh_buffers_t* bufs);

/* Per-step gradient diagnostics on/off (finetune.py:190-191,203-206: the reference computes them on
 * every step with two extra backward passes; here they ride on the slab reduction).  Off by default. */
int  umlh_enable_diagnostics(umlh_handle_t h, int32_t on);
/* Heads with bias (head.py:65,68 bias=True, run as packed rows [weight | bias | 0...]): the reference forms its
 * diagnostics over head.weight only (finetune.py:190-191), so only columns [0, cols) of every class row of w_head enter the
 * dot product, the norms and the sign-agreement count (cols = 0 or d_shared: all columns). */
int  umlh_set_diagnostic_columns(umlh_handle_t h, int32_t cols);

/* img_proj WITH bias (head.py:65 `bias=True`, run as a bias-free projection over rows [x | 1 | 0...]): row `row` of w_proj is the
 * constant row that copies the ones column into the projected rows (the head's own bias column needs it); the optimizer
 * leaves that row, and its moments, untouched.  row < 0 clears.  Needs d_img % 4 == 0. */
int  umlh_freeze_proj_row(umlh_handle_t h, int32_t row);

/* head.weight.data = get_zero_shot_weights(...)  head.py:22-37,96-98: per-class
 * mean of the text rows (rows of classes without text stay 0), rows L2-normalised. */
int  umlh_zero_shot_init(umlh_handle_t h, const float* text_feats, const int64_t* text_labels,
                         int64_t n_text, void* stream);

/* model(images, text_features) logits, unfused, for callers that want the
 * tensors (head.py:77-84 / :131-137).  modality 0 = image path (through img_proj
 * when has_proj, scaled by img_scale), 1 = text path (txt_scale).
 * logits_out: device [rows, C] fp32. */
int  umlh_logits(umlh_handle_t h, const umlh_batch_t* batch, int modality, float* logits_out, void* stream);

/* model.extract_features(images) for the projected head: out[rows, d_shared] =
 * img_proj(feats) (head.py:87-90).  Requires has_proj. */
int  umlh_project(umlh_handle_t h, const umlh_batch_t* batch, float* out, void* stream);

/* One whole training step (finetune.py:180-195 minus logging): fused
 * features x W^T * scale -> softmax-CE -> dZ, dW(+dW_proj, dscale), optimizer
 * update of every parameter.  Either batch may have rows == 0 (modality absent,
 * finetune.py:373-380).  scalars_out: device float[UMLH_N_SCALARS] or NULL. */
int  umlh_train_step(umlh_handle_t h, const umlh_batch_t* img, const umlh_batch_t* txt,
                     const umlh_hyper_t* hyper, float* scalars_out, void* stream);

/* Many consecutive training steps from device-resident tables with no host work in
 * between (the whole `for i in range(max_iters)` body of finetune.py:162-195 between two
 * evaluations).  Step k consumes index[offsets[k] .. offsets[k+1]) of each modality
 * (offsets: HOST int32[n_steps+1]; a modality with table == NULL is absent), uses
 * lr[k] (HOST double[n_steps]) and optimizer step number first_step + k, and writes its
 * scalars to scalars_out + k*UMLH_N_SCALARS (device, may be NULL). */
typedef struct {
    const float*   feats;       /* device [table_rows, dim] fp32                           */
    const void*    feats_bf16;  /* device bf16 shadow (UMLH_PREC_BF16) or NULL             */
    const int64_t* labels;      /* device [table_rows]                                     */
    const int64_t* index;       /* device int64: concatenated per-step row ids             */
    const int32_t* offsets;     /* HOST  int32 [n_steps + 1]                               */
} umlh_stream_t;
int  umlh_train_steps(umlh_handle_t h, const umlh_stream_t* img, const umlh_stream_t* txt, int32_t n_steps,
                      const double* lr, int64_t first_step, float alpha, float img_alpha,
                      float* scalars_out, void* stream);

/* Batch <= 64 linear heads (the reference's own operating point: batch 8 / 32 / 64, 12 800 iterations,
 * engine/optimizer/default.py:3-45): umlh_train_steps runs all n_steps inside ONE persistent launch when the head has
 * no img_proj, its width has a supported chunking (fp32: d in {16,32,48,64,80,96,128,256,384,512,640,768,1024}; bf16
 * operand mode: the multiples of 128 among them), diagnostics are off and every step has at most 4 sample tiles
 * (ceil(rows_img/16) + ceil(rows_txt/16) <= 4).  bf16 mode reads the fp32 tables and rounds operands at use (same
 * values as the bf16 shadows of the three-kernel path); for d <= 640 the step's rows stay in LDS as bf16.  The
 * class axis is cut into 16-class slices, one workgroup per slice owns its part of W / m / v for the whole call; the
 * slices of a head exchange their softmax statistics once per step (in-launch, bounded waits).  UMLH_MICRO=0 in the
 * environment disables the path.  A wait that gives up (another process starving the device of CUs) is reported
 * through umlh_micro_status (0 = ok); the head's state is then undefined.
 *
 * umlh_train_steps_grouped: the sweep of finetune.py:406-448 (HYPER_DICT grid x alpha x seeds: many independent heads over
 * the SAME feature tables) as grouped launches -- G heads [G, C, d] advance n_steps each inside the same persistent
 * launch(es), every head with its own index streams, lr table, optimizer state and scalar rows.  Results are bit-identical
 * to G separate umlh_train_steps calls.  Heads outside the micro envelope fall back to per-head stepping. */
typedef struct {
    umlh_handle_t handle;
    const umlh_stream_t* img;    /* NULL = modality absent */
    const umlh_stream_t* txt;
    const double* lr;            /* HOST double[n_steps] */
    int64_t first_step;
    float   alpha, img_alpha;
    float*  scalars_out;         /* device float[n_steps * UMLH_N_SCALARS] or NULL */
} umlh_group_item_t;
int  umlh_train_steps_grouped(const umlh_group_item_t* items, int32_t n_items, int32_t n_steps, void* stream);
int  umlh_micro_status(umlh_handle_t h, int32_t* status_out);
/* number of persistent micro-step launches this handle has taken part in (which path ran: tests, logging) */
int  umlh_micro_launches(umlh_handle_t h, int64_t* out);

/* The one-launch step of a linear bf16 head (forward, dW, update as claimed tasks of ONE launch: finetune.py:180-195 without a
 * kernel boundary).  Its in-launch waits are bounded (50 ms).  A wait that gives up (the device is being starved by another
 * tenant, or a fault) sets a device status word; the step that hit it and every later step of the handle apply NO update from
 * that point (a gradient that timed out is never stepped) and umlh_step_status returns, in status_out[0..3], {code (0 = ok),
 * first task of the range waited on, launch tag, phase}.  It synchronises with the device.  The host mirror raises UmlhError
 * whenever it reads the step scalars and finds the code set.  umlh_step_launches: one-launch steps taken by this handle. */
int  umlh_step_status(umlh_handle_t h, int32_t* status_out);

/* Direct peer-to-peer all-reduce of the gradient message (csrc/umlh_p2p.hip): reduce-scatter + all-gather over exchange regions
 * that every rank allocates in its own HBM (umlh_p2p_alloc of umlh_p2p_region_bytes(n_floats of umlh_grad_buffer, n_ranks)),
 * exports (umlh_p2p_export: a 64-byte hipIpcMemHandle_t to hand to the peers over the caller's store) and maps from its peers
 * (umlh_p2p_open).  umlh_p2p_attach makes it the handle's transport in place of RCCL / the callback (linear heads; the sums are
 * formed in rank order, bit-identical on every rank).  No reference call site exists (the reference is single-GPU); SURVEY 8(e)
 * asks for it because a ring is per-link bound on the xGMI mesh.  Its waits give up after 30 s (a peer that never arrives) and
 * report through umlh_step_status (code 2).  UNMEASURED on a multi-GPU node: RCCL remains the default transport. */
uint64_t umlh_p2p_region_bytes(int64_t n_max_floats, int32_t n_ranks);
int  umlh_p2p_alloc(uint64_t bytes, void** out);
int  umlh_p2p_free(void* p);
int  umlh_p2p_export(void* p, void* handle64);
int  umlh_p2p_open(const void* handle64, void** out);
int  umlh_p2p_close(void* p);
int  umlh_p2p_attach(umlh_handle_t h, void* const* regions, int32_t n_ranks, int32_t rank);
int  umlh_step_launches(umlh_handle_t h, int64_t* out);

/* Data-parallel split of the step: gradients only, laid out as ONE flat fp32
 * buffer [g_head | g_proj | g_scales(2) | scalars(UMLH_N_SCALARS)] inside the
 * workspace, already divided by batch->global_rows so a SUM all-reduce over ranks
 * yields the single-GPU gradient; then the update from that buffer.  With the gradient diagnostics enabled
 * (d_shared % 8 == 0) the head part is [g_img | g_txt]: the two per-modality gradients travel separately and
 * umlh_apply_update forms dot / norms / sign agreement from the all-reduced pair (pass the step's alpha / img_alpha in
 * its hyper), so the diagnostics of a data-parallel step are those of the global batch. */
/* Data-parallel transport.  With more than one rank attached, umlh_train_steps runs every step as
 *   gradients -> SUM all-reduce -> identical update,
 * all enqueued from C on the caller's stream (no host work per step): equal shards are assumed (every rank passes the same
 * row counts per step; the CE means divide by rows x n_ranks).  For a 2-layer head the head gradient's all-reduce runs on
 * a second stream beside the img_proj backward GEMMs.  The reference is single-process; there is no
 * reference call site.
 *   umlh_comm_unique_id / umlh_comm_init_rank: an RCCL communicator owned by the handle (librccl.so.1 is loaded at run
 *     time; rank 0 draws the 128-byte id and hands it to the others, e.g. by a torch.distributed broadcast);
 *   umlh_set_comm: attach an existing ncclComm_t instead;
 *   umlh_set_allreduce: a custom transport -- fn(ctx, device_buf, n_floats, stream) must SUM-all-reduce the buffer in
 *     place and be ordered with `stream` (tests plug gloo through a host callback; n_ranks == 1 makes umlh_train_steps take
 *     the split path alone, for pricing). */
#define UMLH_COMM_ID_BYTES 128
typedef int (*umlh_allreduce_fn)(void* ctx, float* device_buf, uint64_t n_floats, void* stream);
int  umlh_comm_unique_id(void* id_out /* UMLH_COMM_ID_BYTES */);
int  umlh_comm_init_rank(umlh_handle_t h, const void* id, int32_t n_ranks, int32_t rank);
int  umlh_set_comm(umlh_handle_t h, void* nccl_comm, int32_t n_ranks);
int  umlh_set_allreduce(umlh_handle_t h, umlh_allreduce_fn fn, void* ctx, int32_t n_ranks);

int  umlh_grad_step(umlh_handle_t h, const umlh_batch_t* img, const umlh_batch_t* txt,
                    const umlh_hyper_t* hyper, void* stream);
int  umlh_grad_buffer(umlh_handle_t h, float** device_ptr, uint64_t* n_floats);
/* Diagnostic builds only (UMLH_DBG_FWD=9): per-workgroup cycle stamps of the forward kernel,
 * a region of the workspace no other code reads. */
int  umlh_debug_buffer(umlh_handle_t h, void** device_ptr, uint64_t* n_bytes);
int  umlh_apply_update(umlh_handle_t h, const umlh_hyper_t* hyper, float* scalars_out, void* stream);

/* validate() inner loop for one batch (finetune.py:295-308): logits -> argmax ->
 * CE, nothing leaves the device.  Writes scalars_out[UMLH_S_CORRECT] (count) and
 * scalars_out[UMLH_S_LOSS_SUM] (sum of row losses); the caller forms the
 * per-batch means (finetune.py:311-312). */
int  umlh_eval_batch(umlh_handle_t h, const umlh_batch_t* batch, float* scalars_out, void* stream);

/* Whole-table evaluation: the same forward as umlh_eval_batch over up to max_rows_img rows, but the per-row
 * results are kept -- row_stats[2*r] = CE of row r, row_stats[2*r + 1] = 1 if its first arg-max is the label.
 * validate() (finetune.py:291-315) forms its per-batch mean losses from these for ANY batch size, so a
 * validation pass is one launch per 4096-row slab instead of one per batch. */
int  umlh_eval_rows(umlh_handle_t h, const umlh_batch_t* rows, float* row_stats, void* stream);

/* Per-phase device timing of umlh_train_step / umlh_grad_step with HIP events recorded
 * on the step's stream (bench.py's roofline leg; rocprofv3 --kernel-trace must agree).
 * Phases: 0 img_proj forward GEMM, 1 fused forward+CE, 2 dW_head GEMM, 3 img_proj
 * backward GEMMs, 4 slab reduce + optimizer + scalars.  enable creates the events,
 * read synchronises on the last one and returns milliseconds of the latest step. */
#define UMLH_N_PHASES 5
int  umlh_profile_enable(umlh_handle_t h, int enable);
int  umlh_profile_read(umlh_handle_t h, float* ms_out /* host float[UMLH_N_PHASES] */);

/* fp32 -> bf16 (round-to-nearest-even) copy of n elements: builds the bf16 shadow of a
 * device-resident feature table once, for UMLH_PREC_BF16 handles. */
int  umlh_to_bf16(const float* src, void* dst_bf16, int64_t n, void* stream);

/* MultiBench alternation step (MultiBench/train.py:354-399, models.py:194-243): per-modality
 * decoder Linear(z -> D) fused with the masked next-step MSE, forward and backward.
 *   recon[b,t,:] = W z[b,t,:] + bias;  loss = sum_{t<T-1, t+1<len_b} |recon[b,t]-x[b,t+1]|^2 / (D*#live + 1e-8)
 * (T == 1: plain reconstruction MSE, models.py:209-210; lengths == NULL: unmasked mean).
 * z [B,T,Z], w [D,Z], bias [D], x [B,T,D] fp32 device; lengths int64[B] device or NULL.
 * recon [B,T,D] optional; dres [B*T*D] and row_partial [B*T] scratch that the backward reads;
 * loss_cnt device float[2] = {loss, denominator}.  Backward: grad_out device scalar (d/d loss);
 * dz [B,T,Z], dw [D,Z], db [D]; scratch: umlh_seq_mse_backward_scratch_floats(B,T,Z,D) device floats for the split-K
 * slabs of dW and the row-chunk partials of db (NULL: db is one walk over all B*T rows per 64 columns, and dW, where the plan
 * splits the rows, a chain of launches over the same row chunks, each adding the sum so far).  lengths may hold any value:
 * below 2 no position of the sequence is live, above T it counts as T. */
int  umlh_seq_mse_forward(const float* z, const float* w, const float* bias, const float* x, const int64_t* lengths,
                          int32_t B, int32_t T, int32_t Z, int32_t D, float* recon, float* dres, float* row_partial,
                          float* loss_cnt, void* stream);
int  umlh_seq_mse_backward(const float* z, const float* w, const float* dres, const float* loss_cnt, const float* grad_out,
                           int32_t B, int32_t T, int32_t Z, int32_t D, float* dz, float* dw, float* db, float* scratch,
                           void* stream);
uint64_t umlh_seq_mse_backward_scratch_floats(int32_t B, int32_t T, int32_t Z, int32_t D);

/* SequenceInfoNCELoss (MultiBench/models.py:145-175), the contrastive alternative to the next-step MSE: over the n valid
 * (batch, time) rows, logits = normalize(pred) normalize(target)^T / temperature, labels = the diagonal, loss = mean CE.
 * pred / target [n, D] dense fp32 rows (the caller selects the valid rows, as the reference's boolean indexing does).
 * Forward leaves: pred_hat, target_hat [n, D] (unit rows), pred_norm [n], probs [n, n] = softmax(logits) - I, row_loss [n],
 * loss (device scalar).  Backward: grad_out device scalar; dhat [n, D] scratch; dpred [n, D] = d loss / d pred * grad_out.
 * (No gradient flows to the targets: they are the model's inputs.)
 * Rows of norm below 1e-12: a row is divided by max(|x|, 1e-12) and its gradient is (dy - y (y . dy)) / max(|x|, 1e-12) for
 * every row.  torch's F.normalize clamps with clamp_min, whose backward drops the projection term y (y . dy) of a clamped row; the
 * two agree for |x| = 0 (y = 0) and differ by |y|^2 = (|x| / 1e-12)^2 of the row's gradient for 0 < |x| < 1e-12. */
int  umlh_infonce_forward(const float* pred, const float* target, int32_t n, int32_t D, float temperature, float* pred_hat,
                          float* target_hat, float* pred_norm, float* probs, float* row_loss, float* loss, void* stream);
int  umlh_infonce_backward(const float* pred_hat, const float* target_hat, const float* pred_norm, const float* probs,
                           const float* grad_out, int32_t n, int32_t D, float temperature, float* dhat, float* dpred, void* stream);

/* ---- MultiBench shared encoder (MultiBench/models.py:39-127: Conv1d k=1 -> positions -> 5 x post-norm
 * nn.TransformerEncoderLayer(z, nhead, dim_feedforward=2048, relu, dropout) under a causal + key-padding
 * mask), forward and backward, fp32.  Token rows are m = t*B + b of a [T,B,*] activation (torch's
 * sequence-first layout).  The host mirror (multibench/encoder.py) strings these together exactly as
 * torch.nn.TransformerEncoderLayer.forward does; all pointers are device fp32 unless noted. ---- */

/* out[m][n] = alpha * sum_k A(m,k) B(n,k).  ta = 0: A[m*lda + k], rows optionally gathered by a_rows[m];
 * ta = 1: A[k*lda + m].  tb = 0: B[n*ldb + k];  tb = 1: B[k*ldb + n], rows optionally gathered by k_rows[k].
 * (ta,tb) in {(0,0),(0,1),(1,1)}: y = x W^T, dx = dy W, dW = dy^T x; other pairs and strides shorter than a row
 * (lda < (ta ? M : K), ldb < (tb ? N : K), ldo < N) are UMLH_E_INVALID.  Only the [M, N] window of out (row stride ldo)
 * is written.  Products: the fp32 MFMA, or the x3 form of UMLH_PREC_FP32 (three bf16 pieces per operand) on large grids
 * (the 128x128 tile at >= 768 workgroups, and the dW tile); both meet the same criterion against float64, and an
 * infinite operand on an x3 path yields NaN rather than +-inf.
 * splits > 1: split-K over `splits` slabs of M*ldo floats in `slabs` (caller scratch), summed into out in slab
 * order -- the encoder's GEMMs have few output tiles and a long K, so one tile per CU is latency-bound. */
int  umlh_gemm_f32(const float* A, const float* B, float* out, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb,
                   int32_t ldo, int32_t ta, int32_t tb, const int64_t* a_rows, const int64_t* k_rows, float alpha,
                   int32_t splits, float* slabs, void* stream);
/* y[m][n] = act(y[m][n] + bias[n]) in place (bias may be NULL; relu != 0: fmaxf(., 0) -- whatever is not > 0 becomes +0.0, a
 * NaN included, which torch.relu would keep) */
int  umlh_bias_act(float* y, const float* bias, int64_t M, int32_t N, int32_t relu, void* stream);
/* dy[i] = y[i] > 0 ? dy[i] : 0 in place */
int  umlh_relu_backward(const float* y, float* dy, int64_t n, void* stream);
/* x[i] = keep_i ? x[i] * (1.f/(1.f-p)) : 0 in place; keep_i is a pure function of (seed, i): the same call on the
 * gradient is the backward pass.  p == 0: no-op.  `seed` names a mask STREAM and i is the flat element index; every dropout of
 * the encoder draws from such a stream, so the mask of any of them is what this call leaves of a tensor of ones with the same p
 * and seed (tests/test_encoder_kernels_gpu.py builds its float64 references from exactly that). */
int  umlh_dropout(float* x, int64_t n, float p, uint64_t seed, void* stream);
/* y[i] += x[i]  (gradient fan-in of a residual branch) */
int  umlh_add_inplace(float* y, const float* x, int64_t n, void* stream);
/* out[n] = sum_m x[m][n]  (bias gradients) */
int  umlh_colsum(const float* x, int32_t M, int32_t N, float* out, void* stream);
/* s = x + r (r may be NULL); y = LayerNorm(s; gamma, beta, eps); mean/rstd [M] saved for the backward */
int  umlh_add_layernorm_forward(const float* x, const float* r, const float* gamma, const float* beta, int32_t M, int32_t N,
                                float eps, float* s, float* y, float* mean, float* rstd, void* stream);
/* ds [M,N] (gradient of both summands of s), dgamma [N], dbeta [N] */
int  umlh_layernorm_backward(const float* dy, const float* s, const float* gamma, const float* mean, const float* rstd,
                             int32_t M, int32_t N, float* ds, float* dgamma, float* dbeta, void* stream);
/* x[t,b,:] += pos[t,:]  /  dpos[t,:] = sum_b dx[t,b,:] */
int  umlh_add_positions(float* x, const float* pos, int32_t T, int32_t B, int32_t Z, void* stream);
int  umlh_positions_backward(const float* dx, int32_t T, int32_t B, int32_t Z, float* dpos, void* stream);
/* scatter == 0: out[j,:] = x[idx[j],:];  scatter != 0: out[idx[j],:] = x[j,:] (out pre-zeroed, idx unique) */
int  umlh_gather_rows(const float* x, const int64_t* idx, int32_t n, int32_t Z, float* out, int32_t scatter, void* stream);
/* Causal multi-head self-attention with key padding over packed in-projections qkv [T,B,3Z] (torch
 * MultiheadAttention layout), H heads; lengths int64[B] or NULL.  ctx [T,B,Z] (heads concatenated, before
 * out_proj), lse [B,H,T] saved for the backward.  p/seed: attention-probability dropout: the probability of (query t, key j) of batch b, head h is element
 * ((b*H + h)*T + t)*T + j of stream `seed`; it multiplies the NORMALISED probabilities (lse and the softmax denominator run
 * over all visible keys, kept or not); in the backward dv sums the dropped probabilities and dS is built from the undropped
 * ones.  Key j is visible to query t iff j <= t and j < lengths[b]; padded query rows are computed like any other; dk and dv
 * rows of padded keys are exactly 0.  T <= 128, Z/H <= 64. */
int  umlh_attention_forward(const float* qkv, const int64_t* lengths, int32_t T, int32_t B, int32_t Z, int32_t H, float p,
                            uint64_t seed, float* ctx, float* lse, void* stream);
int  umlh_attention_backward(const float* qkv, const int64_t* lengths, const float* lse, const float* dctx, int32_t T, int32_t B,
                             int32_t Z, int32_t H, float p, uint64_t seed, float* dqkv, void* stream);

/* One whole post-norm nn.TransformerEncoderLayer (MultiBench/models.py:57-60: d_model = Z, nhead = H, dim_feedforward = d_ff,
 * relu, dropout p, causal + key-padding mask), forward / backward, as ONE call each: the launch sequence the host mirror
 * used to drive op by op is enqueued from C (same kernels, same arithmetic, same dropout seeds: seed for the attention
 * probabilities (element index as in umlh_attention_forward), seed+1 / +2 / +3 for dropout1 / the FFN dropout / dropout2, each
 * indexed by the flat element m*N + n of its [M, N] activation: [M, Z], [M, d_ff], [M, Z]).
 *   params[12] = in_proj_weight [3Z,Z], in_proj_bias, out_proj.weight [Z,Z], out_proj.bias, linear1.weight [d_ff,Z],
 *                linear1.bias, linear2.weight [Z,d_ff], linear2.bias, norm1.weight, norm1.bias, norm2.weight, norm2.bias
 *   h_in / h_out [T*B, Z] token rows m = t*B + b;  saved: caller buffer of umlh_encoder_layer_saved_floats(cfg) floats that
 *   the backward of the same layer reads;  scratch: umlh_encoder_layer_scratch_floats(cfg) floats, reusable across layers.
 *   backward: dh_out = d loss / d h_out -> grads[12] (same order and shapes as params) and dh_in. */
typedef struct {
    int32_t T, B, Z, H, d_ff;
    float   p, eps;
    uint64_t seed;
    const uint64_t* seed_device;   /* optional device word added to `seed` by every kernel (NULL = none): lets a launch sequence
                                    * captured in a HIP graph draw fresh dropout masks at every replay */
} umlh_enc_layer_t;
uint64_t umlh_encoder_layer_saved_floats(const umlh_enc_layer_t* cfg);
uint64_t umlh_encoder_layer_scratch_floats(const umlh_enc_layer_t* cfg);
int  umlh_encoder_layer_forward(const umlh_enc_layer_t* cfg, const float* const* params, const float* h_in, const int64_t* lengths,
                                float* saved, float* scratch, float* h_out, void* stream);
int  umlh_encoder_layer_backward(const umlh_enc_layer_t* cfg, const float* const* params, const float* h_in, const int64_t* lengths,
                                 const float* saved, const float* dh_out, float* scratch, float* const* grads, float* dh_in,
                                 void* stream);

/* The whole stack of n_layers identical layers in one call each way.  P / G: 12 pointers per layer in the order above.
 * forward: layer li reads (li ? h + (li-1)*M*Z : h0) and writes h + li*M*Z (M = T*B) and saved + li*saved_floats; its dropout
 * streams start at cfg->seed + 7919*li.  backward: dh_out = gradient of the last layer's output, dh = two [M,Z] scratch
 * buffers, the gradient of h0 is left in dh0. */
int  umlh_encoder_stack_forward(const umlh_enc_layer_t* cfg, int32_t n_layers, const float* const* P, const float* h0,
                                const int64_t* lengths, float* saved, float* scratch, float* h, void* stream);
int  umlh_encoder_stack_backward(const umlh_enc_layer_t* cfg, int32_t n_layers, const float* const* P, const float* h0,
                                 const int64_t* lengths, const float* saved, const float* h, const float* dh_out, float* scratch,
                                 float* const* G, float* dh, float* dh0, void* stream);

/* Encoder plan: the layer stack bound to fixed buffers so that its launch sequences replay from HIP graphs (one graph launch per
 * forward / backward instead of 7 + 16 kernel launches per layer: at MOSEI sizes the alternation step is bound by the host's
 * launch rate).  The caller owns `workspace` (umlh_encoder_plan_floats(cfg, n_layers) device floats, alive as long as the plan)
 * and the parameter tensors P (12 per layer; their ADDRESSES are baked into the graphs -- make a new plan when they move).
 * Buffers inside the workspace (float offsets from umlh_encoder_plan_offsets):
 *   [0] h0 [T*B, Z]    input token rows, written by the caller before forward
 *   [1] lengths        int64[B] key-padding lengths (has_lengths != 0), written by the caller before forward
 *   [2] h_last [T*B,Z] output of the last layer
 *   [3] dh_out [T*B,Z] gradient of h_last, written by the caller before backward
 *   [4] dh0 [T*B, Z]   gradient of h0 after backward
 *   [5] grads          gradients of all parameters after backward, flat in P order
 * forward: seed = base of this pass's dropout streams (cfg->seed is ignored).  The first call of each direction runs the plain
 * launch sequence, the second captures it, later calls replay.  A plan serves ONE forward/backward pair at a time and one
 * stream at a time. */
typedef struct umlh_enc_plan_s* umlh_enc_plan_t;
uint64_t umlh_encoder_plan_floats(const umlh_enc_layer_t* cfg, int32_t n_layers);
int  umlh_encoder_plan_create(const umlh_enc_layer_t* cfg, int32_t n_layers, const float* const* P, int32_t has_lengths,
                              float* workspace, umlh_enc_plan_t* out);
int  umlh_encoder_plan_offsets(umlh_enc_plan_t plan, uint64_t offsets[6]);
int  umlh_encoder_plan_forward(umlh_enc_plan_t plan, uint64_t seed, void* stream);
int  umlh_encoder_plan_backward(umlh_enc_plan_t plan, void* stream);
void umlh_encoder_plan_destroy(umlh_enc_plan_t plan);

/* A pseudo-random permutation of 0..n-1 written as int64 (device), keyed by seed: 4-round Feistel
 * network + cycle walking, no sort.  Epoch shuffles for throughput runs; NOT the reference's
 * sampler order (that is reproduced host-side by the loader, finetune.py:370-371). */
int  umlh_random_permutation(int64_t n, uint64_t seed, int64_t* out, void* stream);

/* The row ids of a block of training steps, both modalities in one launch (index_block_kernel): each modality's ids are the
 * ids of its spans written back to back into its destination, which then serves as umlh_stream_t.index.  A span is `count`
 * consecutive positions start .. start+count-1 of one epoch order of n rows:
 *   UMLH_SPAN_FEISTEL  the order of umlh_random_permutation(n, seed): ids bit-identical to out[start .. start+count) of that
 *                      call, computed per element, the permutation is never written out;
 *   UMLH_SPAN_TABLE    order[start .. start+count) of a materialised device order of n int64 ids (a copy);
 *   UMLH_SPAN_IOTA     start .. start+count-1 (an unshuffled loader).
 * A modality without rows passes n_spans = 0.  Any number of spans: one launch carries 32 of them, more spans take more launches.
 * A span with count < 0, start < 0 or start + count > n, a FEISTEL span with n > 2^62, a TABLE span without order and a
 * destination missing for a positive total are UMLH_E_INVALID, checked for every span before the first launch.  Additive to
 * ABI v11: umlh_version() is unchanged, callers detect the feature by this symbol. */
#define UMLH_SPAN_FEISTEL 0
#define UMLH_SPAN_TABLE   1
#define UMLH_SPAN_IOTA    2
typedef struct {
    int32_t kind;            /* UMLH_SPAN_* */
    int32_t reserved;        /* 0 */
    int64_t n;               /* rows of the epoch order */
    uint64_t seed;           /* FEISTEL: the permutation's key */
    const int64_t* order;    /* TABLE: device, n ids; otherwise unused */
    int64_t start, count;
} umlh_index_span_t;
int  umlh_index_block(const umlh_index_span_t* img_spans, int32_t n_img_spans, int64_t* img_out,
                      const umlh_index_span_t* txt_spans, int32_t n_txt_spans, int64_t* txt_out, void* stream);

/* Standalone optimizer.step() for one parameter tensor from a caller-computed
 * gradient (engine/optimizer/optim.py:34-71; torch.optim single-tensor recurrences):
 * the same update kernel the fused step applies.  v may be NULL for SGD and is not touched by it; step < 1 counts as
 * step 1.  That kernel moves 16 bytes per access: when param, grad, m or (Adam / AdamW) v is not 16-byte aligned the call
 * runs the element-wise kernel of umlh_optimizer_step_multi instead, which needs 4-byte alignment only. */
int  umlh_optimizer_step(int32_t optimizer, float* param, const float* grad, float* m, float* v, int64_t n,
                         double lr, int64_t step, double beta1, double beta2, double eps, double momentum,
                         double weight_decay, void* stream);
/* The same update for MANY parameter tensors in one launch per 48 tensors (optimizer.step() over all 70 tensors of the
 * MultiBench model, MultiBench/main.py:122): host arrays of n_tensors device pointers / element counts; v may be NULL for SGD. */
int  umlh_optimizer_step_multi(int32_t optimizer, int32_t n_tensors, float* const* params, const float* const* grads,
                               float* const* m, float* const* v, const int64_t* n, double lr, int64_t step, double beta1,
                               double beta2, double eps, double momentum, double weight_decay, void* stream);

/* ---- representation-alignment metrics (vision_language/metrics.py; the same in MultiBench/metrics.py and
 * Gaussian_experiment/metrics.py).  Features are row-major fp32 [n, d] with row stride ld >= d.  No N x N array is
 * formed; results are bitwise reproducible for a given `splits` (0 = auto) and no reduction uses float atomics.
 * Every argument check happens before any HIP call.  `scratch` is caller device memory of at least
 * umlh_align_scratch_bytes(...) bytes with the same arguments; results are device memory written on `stream`. */

/* Scratch bytes for umlh_align_knn (topk >= 1; topk = 0: none), umlh_align_mutual_knn and umlh_align_cka with these
 * arguments: O(n*topk*splits + tiles + d^2), no n^2 term.  0 on invalid arguments (n < 1, d_a or d_b < 1, topk outside
 * 0..32, topk >= n, splits < 0). */
uint64_t umlh_align_scratch_bytes(int64_t n, int32_t d_a, int32_t d_b, int32_t topk, int32_t splits);
/* compute_nearest_neighbors(feats, topk) (metrics.py:272-285): per row i the topk columns j != i with the largest raw
 * inner product x_i . x_j (not cosine), ordered by (score desc, index asc) -- exact ties go to the smaller index; the
 * reference excludes self by writing -1e8 on the diagonal, here self is skipped.  knn int32 [n, topk]; scores fp32
 * [n, topk] or NULL.  Products on the f32 MFMA (a k-ordered fp32 fma chain); the result is bitwise independent of
 * `splits` (column chunks of the fused Gram + top-k pass).  1 <= topk <= 32, topk < n. */
int  umlh_align_knn(const float* x, int64_t n, int32_t d, int32_t ldx, int32_t topk, int32_t splits, int32_t* knn,
                    float* scores, void* scratch, uint64_t scratch_bytes, void* stream);
/* AlignmentMetrics.mutual_knn given both neighbour lists (metrics.py:55-84): mean over rows of
 * |knn_a(i) n knn_b(i)| / topk; the counts are summed as integers, the mean is formed once in double -> out[0]. */
int  umlh_align_mutual_knn(const int32_t* knn_a, const int32_t* knn_b, int64_t n, int32_t topk, double* out, void* scratch,
                           uint64_t scratch_bytes, void* stream);
/* AlignmentMetrics.cka(a, b, kernel_metric='ip', unbiased=False) (metrics.py:96-119 with hsic_biased :252-255) in
 * feature space: trace(K H L H) = ||Ac^T Bc||_F^2 with Ac, Bc the column-centred features (centred on load).
 * out4 = {hsic_kl / (sqrt(hsic_kk * hsic_ll) + 1e-6), hsic_kl, hsic_kk, hsic_ll} in double; no 1/(n-1)^2 factor. */
int  umlh_align_cka(const float* a, int32_t lda, int32_t d_a, const float* b, int32_t ldb, int32_t d_b, int64_t n,
                    int32_t splits, double* out4, void* scratch, uint64_t scratch_bytes, void* stream);

/* The other metrics of AlignmentMetrics, with a scratch query of their own (umlh_align_scratch_bytes keeps its values). */
#define UMLH_ALIGN_CKA_UNBIASED 0
#define UMLH_ALIGN_CKA_RBF      1
#define UMLH_ALIGN_CKNNA        2
#define UMLH_ALIGN_LIST_STATS   3

/* Scratch bytes of the entry point `kind` (above) with these arguments: O(n*splits + tiles + d^2), no n^2 term.  The CKA
 * kinds ignore topk, the list kinds ignore d_a, d_b and splits.  0 on invalid arguments (unknown kind, n < 1, n < 4 for the
 * unbiased CKA, d < 1, splits < 0, topk outside 1..32 (CKNNA: 2..32) or topk >= n). */
uint64_t umlh_align_ext_scratch_bytes(int32_t kind, int64_t n, int32_t d_a, int32_t d_b, int32_t topk, int32_t splits);
/* AlignmentMetrics.unbiased_cka(a, b) = cka(kernel_metric='ip', unbiased=True) (metrics.py:96-125 with hsic_unbiased
 * :230-249) in feature space.  hsic_unbiased of a linear kernel is invariant under a translation of the features, so the
 * features are centred on load as in umlh_align_cka; with centred rows x_i, y_i and m = n:
 * sum K~ . L~ = ||Ac^T Bc||_F^2 - sum_i |x_i|^2 |y_i|^2, (K~ 1)_i = x_i . (sum_j x_j) - |x_i|^2 (the column sums are those of
 * the rounded centred values), 1^T K~ L~ 1 = (K~ 1) . (L~ 1).  out4 = {hsic_kl / (sqrt(hsic_kk * hsic_ll) + 1e-6), hsic_kl,
 * hsic_kk, hsic_ll} in double.  n >= 4 (the m - 3 divisor). */
int  umlh_align_cka_unbiased(const float* a, int32_t lda, int32_t d_a, const float* b, int32_t ldb, int32_t d_b, int64_t n,
                             int32_t splits, double* out4, void* scratch, uint64_t scratch_bytes, void* stream);
/* AlignmentMetrics.cka(a, b, kernel_metric='rbf', rbf_sigma=sigma, unbiased=...) (metrics.py:103-119): K_ij =
 * exp(-|a_i - a_j|^2 / (2 sigma^2)), L likewise from b; the n x n pairs are streamed in 32 x 256 tiles (Gram tiles of the
 * column-centred rows on the f32 MFMA, squared distances clamped at 0, full-accuracy fp32 exp; the diagonal is exactly 1 for
 * the biased form and left out of the unbiased one) and reduced to sum K.L, K.K, L.L and the row sums K1, L1 in double.
 * biased (hsic_biased :252-255): trace(K H L H) = sum K.L - (2/n) K1.L1 + (1^T K 1)(1^T L 1)/n^2; unbiased: :230-249, n >= 4.
 * out4 as above.  sigma > 0 and finite. */
int  umlh_align_cka_rbf(const float* a, int32_t lda, int32_t d_a, const float* b, int32_t ldb, int32_t d_b, int64_t n,
                        double sigma, int32_t unbiased, int32_t splits, double* out4, void* scratch, uint64_t scratch_bytes,
                        void* stream);
/* AlignmentMetrics.cknna(a, b, topk, distance_agnostic=False, unbiased=True) (metrics.py:180-227) from the neighbour lists
 * and scores of umlh_align_knn on a and on b (self excluded there: the reference's -inf diagonal).  With S(i) = knn_a(i) n
 * knn_b(i), M_ij = K_ij [j in S(i)], P_ij = L_ij [j in S(i)]: sim_kl = hsic_unbiased(M, P) (:230-249; M and P are not
 * symmetric: the first term is sum_ij M_ij P_ji), sim_kk with S = knn_a and M = P, sim_ll likewise on b.
 * out4 = {sim_kl / (sqrt(sim_kk * sim_ll) + 1e-6), sim_kl, sim_kk, sim_ll} in double; a negative product under the root gives
 * NaN as in the reference.  2 <= topk <= 32 ("CKNNA requires topk >= 2", :184-185), topk < n, n >= 4. */
int  umlh_align_cknna(const int32_t* knn_a, const float* scores_a, const int32_t* knn_b, const float* scores_b, int64_t n,
                      int32_t topk, double* out4, void* scratch, uint64_t scratch_bytes, void* stream);
/* cycle_knn (metrics.py:39-51, :258-269), lcs_knn (:88-92, :288-308) and edit_distance_knn (:164-176) given both neighbour
 * lists int32 [n, topk].  Per row: hit = i is among knn_a[knn_b[i, p], q]; the length of the longest common subsequence of
 * knn_a[i, :] and knn_b[i, :]; their Levenshtein distance with unit costs.  rows: int32 [n, 3] = {hit, lcs, distance} or NULL.
 * out3 = {mean hit, mean LCS length (not divided by topk, as the reference returns it), 1 - mean distance / topk} in double
 * from integer sums.  1 <= topk <= 32, topk < n. */
int  umlh_align_list_stats(const int32_t* knn_a, const int32_t* knn_b, int64_t n, int32_t topk, int32_t* rows, double* out3,
                           void* scratch, uint64_t scratch_bytes, void* stream);

/* Grouped form: the CKA and / or the mutual k-NN of up to UMLH_ALIGN_MAX_PAIRS feature pairs (members) in one fixed train of
 * launches, for callers that measure many small pairs at once (every evaluation of a sweep, the pairs of an embedding capture).
 *   bit identity    with the same `splits`, every word a member's outputs receive is the word the single-pair entry points
 *                   write: out5[0..3] is the out4 of umlh_align_cka, out5[4] the output of umlh_align_mutual_knn on the lists of
 *                   umlh_align_knn on a and on b, and the lists and scores, where asked for, are umlh_align_knn's.
 *   independence    members may differ in every field, and a member's results do not depend on which other members are in the
 *                   group or on their order.
 *   chunk counts    a CKA's bits depend on its row-chunk count, so every member uses the row chunks umlh_align_cka picks for
 *                   (n, d_a, d_b, splits).  k-NN bits do not depend on the column-chunk count: with splits = 0 it follows from the
 *                   32-row strips of ALL views of the group (the rule of the single call on their sum, at most one chunk per
 *                   256-column tile of the member), so a group of many small members runs one chunk per view.  splits > 0 is
 *                   taken as given for both metrics.  One exception, which the single calls share among themselves: a list that
 *                   no column fills (a row of NaN scores) holds one run of sentinels per merged chunk, so ITS words are those of
 *                   the single call made with the same chunk count; they are >= n at a score of -inf for every count.
 *   launches        at most ten, whatever n_items is: column sums, cross products, tile squares and the final of the CKAs; the
 *                   k-NN tiles (one launch per load form: rows of whole aligned float4s, and the rest), one merge; the mutual
 *                   count and its final.  Both views of every member share the tiles and merge launches.  A stage that no
 *                   member asks for is not launched.
 *   pointers        members may share inputs.  An output pointer (out5, knn_*, scores_*) that occurs twice among the members
 *                   is UMLH_E_INVALID.
 *   checks          every check precedes the first HIP call; the message names the function, `member i` and the argument.
 *                   n_items outside 1..UMLH_ALIGN_MAX_PAIRS, a member with cka == 0 and topk == 0, and a NULL or short scratch
 *                   are UMLH_E_INVALID; otherwise a member is held to the checks of umlh_align_cka / umlh_align_knn.
 *   descriptors     the members' descriptors reach the device in one asynchronous upload per call into the head of `scratch`,
 *                   from pinned staging that is reused behind events.  The call does not synchronise the host; `items` may be
 *                   freed when it returns.
 * Additive to ABI v11: umlh_version() is unchanged, callers detect the feature by this symbol. */
#define UMLH_ALIGN_MAX_PAIRS 64
typedef struct {                      /* one pair: the arguments of umlh_align_cka / _knn / _mutual_knn */
    const float* a; int32_t lda, d_a;
    const float* b; int32_t ldb, d_b;
    int64_t n;
    int32_t cka;                      /* 0: out5[0..3] are left untouched */
    int32_t topk;                     /* 0: no lists, out5[4] is left untouched; else 1..32, < n */
    double* out5;                     /* {cka, hsic_kl, hsic_kk, hsic_ll, mutual_knn} */
    int32_t* knn_a; int32_t* knn_b;   /* [n, topk], or NULL: the lists live in scratch */
    float* scores_a; float* scores_b; /* [n, topk] or NULL */
} umlh_align_pair_t;
/* Scratch bytes of umlh_align_pairs with these arguments (a multiple of 256: the descriptor tables, then per member its CKA
 * region, its two views' list slabs, the lists where knn_* is NULL, the mutual partials).  With splits > 0, and for one member
 * at splits = 0, this is at least the sum of the members' umlh_align_scratch_bytes, and it grows with every member added.  With
 * splits = 0 a larger group may need LESS than its members' single calls together, and adding a member may shrink it: the k-NN
 * slabs follow the group's chunk count, which falls as the group grows (six pairs of n = 2000, topk 10, d 10 + 10: about 0.85 MB,
 * against 1.28 MB for one single call).  0 on invalid arguments (items NULL,
 * n_items outside 1..64, splits < 0, a member outside the single-pair envelope or one that asks for nothing). */
uint64_t umlh_align_pairs_scratch(const umlh_align_pair_t* items, int32_t n_items, int32_t splits);
int  umlh_align_pairs(const umlh_align_pair_t* items, int32_t n_items, int32_t splits, void* scratch, uint64_t scratch_bytes,
                      void* stream);

/* ---- linear probes of the MultiBench evaluate() (MultiBench/train.py:31-91,93-240): masked mean pooling, StandardScaler
 * statistics, an L2-regularised BINARY logistic regression fitted on the device, and its score.  Features are row-major fp32
 * [n, d] with row stride ld >= d, labels int32 0/1.  Every argument check happens before any HIP call; everything runs on
 * `stream`; outputs are device memory; results are bitwise reproducible (fixed-order double reductions, no float atomics). */

#define UMLH_PROBE_LBFGS      0   /* LogisticRegression(max_iter=200): sum_i log(1 + exp(-t_i (w.x_i + b))) + |w|^2 / (2C) */
#define UMLH_PROBE_LIBLINEAR  1   /* ... solver='liblinear': the intercept is penalised too, (|w|^2 + b^2) / (2C)          */

/* What a fit leaves behind (device memory, 24 bytes). */
typedef struct {
    int32_t iterations;   /* accepted Newton steps                                                                       */
    int32_t converged;    /* 0: iteration budget spent, or the inputs made the gradient NaN; 1: max|gradient| <= gtol;
                           * 2: the precision floor of the objective: the last accepted step gained less than 1e-11 |f|
                           *    (Newton's next gain is the square of that), or the predicted gain fell below 8 ulp of f,
                           *    or no step length gave a representable decrease with less than 1e-10 |f| predicted      */
    double  max_grad;     /* max |gradient| of the objective at the returned coefficients                                */
    double  objective;    /* the objective there                                                                         */
} umlh_probe_record_t;

/* out[b, :] = sum_{t < L_b} z[b, t, :] / L_b with L_b = min(max(lengths[b], 0), t_len) (train.py:120-125); lengths = NULL:
 * the plain mean over t_len (evaluate_raw_data's x.mean(axis=1)).  z[b, t, c] is read at z[b*ldb + t*ldt + c] (floats; any
 * strides >= zdim, so a [T, B, Z] block is pooled in place), out[b, c] written at out[b*ldo + c].  L_b = 0 gives NaN like
 * the reference's 0/0.  One fp32 chain per element, t ascending. */
int  umlh_masked_mean(const float* z, int32_t b, int32_t t_len, int32_t zdim, int64_t ldb, int64_t ldt, const int64_t* lengths,
                      float* out, int32_t ldo, void* stream);
/* Scratch bytes for umlh_probe_fit (max_iter >= 1) or umlh_probe_column_stats (max_iter = 0) at these sizes: 20 n bytes of
 * O(n) vectors + O(d^2) tiles, no n x d term.  0 on invalid arguments (n < 2 or >= 2^31, d outside 1..1024, max_iter
 * outside 0..1000). */
uint64_t umlh_probe_scratch_bytes(int64_t n, int32_t d, int32_t max_iter);
/* StandardScaler().fit(x): stats[0..d) = column means, stats[d..2d) = population standard deviations (ddof = 0), a value
 * below 10 * DBL_EPSILON replaced by 1 as sklearn does.  Two passes in double, fixed order. */
int  umlh_probe_column_stats(const float* x, int64_t n, int32_t d, int32_t ldx, double* stats, void* scratch,
                             uint64_t scratch_bytes, void* stream);
/* Fits the optimum of the `kind` objective with x~ = [x, 1], t = 2y - 1 and inverse regularisation c by a damped Newton
 * iteration from w = 0: the gradient X~^T (p - y) + R w and the objective are summed in double in a fixed order, the
 * Hessian X~^T diag(p (1 - p)) X~ + R comes off the fp32 MFMA and only shapes the step, and a step is accepted only with
 * sufficient decrease of the objective (step lengths 1, 1/2, ..., 2^-11).  stats (NULL or the 2d doubles of
 * umlh_probe_column_stats) standardises x on load; the coefficients then live in the standardised space, as sklearn's
 * pipeline keeps them.  coef[0..d) = w, coef[d] = intercept (device doubles, also the iterate while the fit runs).
 * The call enqueues a fixed train of launches for max_iter iterations and returns; once the device-side test fires the
 * remaining launches return at once.  objectives: NULL or max_iter + 1 doubles, objective after k accepted steps (NaN
 * beyond the last).  Each fit in flight needs its own scratch, coef and record.  1 <= d <= 1024, 2 <= n < 2^31. */
int  umlh_probe_fit(const float* x, int64_t n, int32_t d, int32_t ldx, const int32_t* y, const double* stats, int32_t kind,
                    double c, int32_t max_iter, double gtol, double* coef, umlh_probe_record_t* record, double* objectives,
                    void* scratch, uint64_t scratch_bytes, void* stream);
/* decision_i = coef . x~_i (fp32 products on the MFMA, standardised on load when stats is given); prediction 1 iff
 * decision > 0.  decision: NULL or n floats.  correct: NULL or one int64 = #{i : prediction_i == y_i} (y required then). */
int  umlh_probe_score(const float* x, int64_t n, int32_t d, int32_t ldx, const double* stats, const double* coef,
                      const int32_t* y, int64_t* correct, float* decision, void* stream);

/* ---- multinomial (softmax) logistic probe: what LogisticRegression(max_iter=200) of the MultiBench probe factory
 * (MultiBench/train.py:96-99) fits on labels with more than two classes, and the L-BFGS linear probe of cached features (DESIGN
 * section 21).  Additive to ABI v11: umlh_version() is unchanged, callers detect the feature by these symbols.  Features are
 * row-major fp32 [n, d] with row stride ldx >= d, labels int32 in [0, n_class), coefficients fp32 coef[n_class, ldc] with
 * ldc >= d + 1 and the intercept in column d (columns past d are never touched).  The objective is sklearn's, as a sum:
 *   f(W) = sum_i (logsumexp_c z_ic - z_{i,y_i}) + (1 / (2 c)) sum_{class, j < d} W_cj^2,   z_ic = W_c . [x_i, 1]
 * (over-parameterised softmax, intercepts not penalised).  A row whose label lies outside [0, n_class) is never used as an
 * address and contributes nothing.  stats (NULL or the 2d doubles of umlh_probe_column_stats) standardises x on load,
 * (float)(((double)x - mean) * (1.0 / scale)); the coefficients then live in the standardised space.  Logits and the gradient
 * R^T x come off the project's fp32 GEMM (logits computed from the coefficients as partial products over chunks of at most 128
 * columns, added in double); the residuals R = softmax - onehot are fp32; the intercepts' gradient is the column sum of R in
 * double with its mean over the classes (0 up to the rounding of R) taken out; the objective, the slab sums of the gradient,
 * max|g| and every dot product of the solver are summed in double in a fixed order.  No float atomics: results are
 * bitwise reproducible across calls and streams, and do not depend on the alignment of x (16-byte or 4-byte loads).  Every
 * argument check happens before any HIP call and names the function and the argument; everything runs on `stream`; outputs are
 * device memory; the host reads nothing back.
 * Envelope: 2 <= n_class <= 4096, 1 <= d <= 2048, 2 <= n, n * n_class < 2^31, 0 <= max_iter <= 1000 (0: evaluation only, in
 * the scratch size), 1 <= history <= 32, finite c > 0; anything else is UMLH_E_INVALID.  scratch must be 8-byte aligned. */

/* Scratch bytes of umlh_softmax_probe_fit (max_iter >= 1) or umlh_softmax_probe_eval (max_iter = 0; history is ignored):
 * O(n * n_class + n * d + history * n_class * d).  0 on invalid arguments. */
uint64_t umlh_softmax_probe_scratch_bytes(int64_t n, int32_t d, int32_t n_class, int32_t max_iter, int32_t history);
/* f, its gradient and max|gradient| at the given coefficients.  objective, max_grad: one double each (either may be NULL);
 * grad: NULL or fp32 [n_class, ldg] with ldg >= d + 1 (columns 0 .. d of every row are written, nothing else). */
int  umlh_softmax_probe_eval(const float* x, int64_t n, int32_t d, int32_t ldx, const int32_t* y, const double* stats,
                             int32_t n_class, double c, const float* coef, int32_t ldc, double* objective, float* grad,
                             int32_t ldg, double* max_grad, void* scratch, uint64_t scratch_bytes, void* stream);
/* L-BFGS with `history` pairs from W = 0 (init = 0) or from what coef holds (init = 1), as a fixed train of launches for
 * max_iter iterations; once the device-side stop test fires every later launch (the GEMMs included) returns at once.  The
 * direction comes from the Gram matrix of [s_1.., y_1.., g] kept in double (two-loop recursion in coefficient space, H0 =
 * s.y / y.y, a pair with s.y <= 1e-12 |s||y| skipped, the first direction scaled by 1 / sum|g|); the line search evaluates the
 * objective at the step lengths 1, 1/2, .., 2^-11 (4 and 2 in front while there is no history) in one pass over Z and
 * Z_p = [x, 1] p^T and takes the largest with f(t) <= f + 1e-4 t g.p.  The logits are carried in double and advanced by
 * t Z_p; every decision that ends the fit is taken on logits recomputed from the coefficients, and record->objective and
 * record->max_grad are those of that fresh evaluation: bit for bit what umlh_softmax_probe_eval returns at the returned
 * coefficients.  record->converged: 1 = max|g| <= gtol; 2 = no step length gave sufficient decrease on fresh logits (the
 * precision floor); 0 = budget spent, or the objective or the gradient is NaN.  objectives: NULL or max_iter + 1 doubles,
 * [0] the objective at the start, [k] that value minus the decreases the line search accepted up to the k-th step
 * (non-increasing; what re-basing on fresh logits adds is kept out, so [iterations] and record->objective differ by the fp32
 * rounding of the logits), NaN beyond record->iterations.  Each fit in flight needs its own scratch, coef and record. */
int  umlh_softmax_probe_fit(const float* x, int64_t n, int32_t d, int32_t ldx, const int32_t* y, const double* stats,
                            int32_t n_class, double c, int32_t max_iter, int32_t history, double gtol, int32_t init, float* coef,
                            int32_t ldc, umlh_probe_record_t* record, double* objectives, void* scratch, uint64_t scratch_bytes,
                            void* stream);
/* The scaler folded into raw-feature weights: w[c, j] = W_cj / sigma_j (fp32 [n_class, ldw], ldw >= d), bias[c] = W_cd -
 * sum_j W_cj mu_j / sigma_j (fp32 [n_class]), formed in double and rounded once; stats = NULL: a plain copy.  umlh_eval_topk and
 * umlh_eval_classwise then score raw features. */
int  umlh_softmax_probe_fold(const float* coef, int32_t ldc, int32_t n_class, int32_t d, const double* stats, float* w, int32_t ldw,
                             float* bias, void* stream);

/* ---- k-nearest-neighbour probe: the 'knn' branch of the MultiBench make_classifier (MultiBench/train.py:99-100,
 * KNeighborsClassifier() = Euclidean metric, uniform weights).  Additive to ABI v11: umlh_version() is
 * unchanged, callers detect the feature by these symbols.  train is row-major fp32 [n_train, d] with row stride ld_train >= d,
 * query fp32 [n_query, d] with row stride ld_query >= d.  No n_query x n_train array is formed and no reduction uses a float
 * atomic.  Every argument check happens before any HIP call; everything runs on `stream`; outputs are device memory.
 * Envelope: 1 <= k <= 24, k <= n_train < 2^31, 1 <= n_query < 2^31, d >= 1, splits >= 0 (0 = auto); anything else is
 * UMLH_E_INVALID.
 *
 * Order rule: per query row the k train rows with the smallest Euclidean distance, ordered by (squared distance ascending,
 * train index ascending) -- exact ties go to the smaller index, the rule of umlh_align_knn.
 * Two stages.  (1) Candidates: the score |t|^2 - 2 q.t ascending (|q|^2 is constant per row) with q.t on the f32 MFMA (a
 * k-ordered fp32 fma chain) and |t|^2 one fp32 fma chain; the kc = min(k + 8, n_train) best under the strict order (score,
 * index) are kept by the 32-row strip / 256-column tile / column-chunk scheme of umlh_align_knn.  (2) The candidates' squared
 * distances are re-evaluated as sum_k (q_k - t_k)^2 in double from the fp32 inputs in a fixed order and re-ranked by (that
 * value, index); the first k are the answer and dist is the square root of the double value rounded to fp32.  Near-duplicate
 * points therefore carry no cancellation noise.  The result is bitwise independent of `splits` and reproducible across calls
 * and streams.
 * Index-range guarantee: every value written to idx lies in [0, n_train), whatever the data.  List slots that no train row
 * filled (n_train < k + 8; a query row of NaNs, whose comparisons are all false) are never used as addresses; output positions
 * they leave open get the position's own index and a NaN distance.  Results for rows that contain NaN / Inf are otherwise
 * unspecified; other rows are unaffected. */

/* Scratch bytes of the search with these arguments: O(n_query * kc * splits + n_train), no n_query * n_train term.  0 on
 * invalid arguments. */
uint64_t umlh_knn_scratch_bytes(int64_t n_train, int64_t n_query, int32_t d, int32_t k, int32_t splits);
/* idx int32 [n_query, k]; dist fp32 [n_query, k] or NULL; both dense. */
int  umlh_knn_search(const float* train, int64_t n_train, int32_t ld_train, const float* query, int64_t n_query, int32_t ld_query,
                     int32_t d, int32_t k, int32_t splits, int32_t* idx, float* dist, void* scratch, uint64_t scratch_bytes,
                     void* stream);
/* The uniform vote of KNeighborsClassifier.predict over idx int32 [n_query, k] (1 <= k <= 24): pred[i] = the label value with
 * the most occurrences among train_labels[idx[i, :]]; a count tie goes to the smallest label value (sklearn's argmax over the
 * sorted classes_).  train_labels int32 [n_train], any values >= 0: no class table is needed.  An idx value outside
 * [0, n_train) is not dereferenced and casts no vote.  Outputs, each optional but at least one required: pred int32 [n_query],
 * votes int32 [n_query] (the winner's count), correct (one int64 = #{pred == y}, integer sums; needs y int32 [n_query]). */
int  umlh_knn_vote(const int32_t* idx, int64_t n_query, int32_t k, const int32_t* train_labels, int64_t n_train, const int32_t* y,
                   int32_t* pred, int32_t* votes, int64_t* correct, void* stream);

/* ---- ABI v8: singular values and effective rank of fp32 feature matrices (MultiBench/utilis.py:27-36, the per-step
 * diagnostic of MultiBench/train.py:386-389).  sigma(A) = sqrt(eig(A^T A)): the d x d Gram is accumulated in fp64 from the
 * fp32 rows (their products are exact there), tridiagonalised by Householder reflections and its eigenvalues found by
 * bisection on Sturm counts with a fixed iteration count, all on the device.  Only the min(rows, d) largest eigenvalues are
 * used (an n x d matrix with n < d has n singular values; the other eigenvalues are rounding noise around zero), negative
 * ones are clamped to 0 before the root.  effective rank = exp(-sum p log(p + eps)), p = sigma / sum sigma, in fp64 in a fixed
 * order: zero valid rows give 1 (empty sums), an all-zero matrix gives NaN (0/0), as the reference's arithmetic does.
 * Rows are split into chunks = min(ceil(n / 256), max(1, 128 / batch)) per matrix; each chunk writes a d x d fp64 slab
 * and a second pass sums the slabs in chunk order: no float atomics, results are bitwise reproducible for given arguments.
 * Envelope: 1 <= d <= 512, 1 <= batch <= 65535, n >= 1, batch * n < 2^31; a[m, r, c] is read at a[m*ld_batch + r*ld_row + c]
 * with ld_row >= d and strides that do not make rows overlap.  Every argument check happens before any HIP call; `scratch`
 * is caller device memory of umlh_spectral_scratch_bytes(batch, n, d) bytes; results are device doubles written on `stream`. */

/* Scratch bytes: 8 d^2 (batch * chunks + batch) rounded up to 256-byte regions: O(chunks d^2 + batch d^2), no n x d term
 * (n enters through the chunk count only).  0 on invalid arguments.  The sequence form uses (1, b * t_len, d). */
uint64_t umlh_spectral_scratch_bytes(int32_t batch, int64_t n, int32_t d);
/* torch.linalg.svdvals(a) for a [batch, n, d]: sv[batch, min(n, d)], descending. */
int  umlh_svdvals(const float* a, int32_t batch, int64_t n, int32_t d, int64_t ld_batch, int64_t ld_row, double* sv, void* scratch,
                  uint64_t scratch_bytes, void* stream);
/* compute_effective_rank(a, eps) (utilis.py:27-36): erank[batch]; sv_or_null: NULL or [batch, min(n, d)] as umlh_svdvals. */
int  umlh_effective_rank(const float* a, int32_t batch, int64_t n, int32_t d, int64_t ld_batch, int64_t ld_row, double eps,
                         double* erank, double* sv_or_null, void* scratch, uint64_t scratch_bytes, void* stream);
/* The effective rank of the valid rows of a block of sequences pooled into ONE matrix (train.py:380-389 flattens the same
 * way): z[b, t, c] is read at z[b*ldb + t*ldt + c] (any non-overlapping strides >= d, so a [T, B, d] block or a column block
 * of a wider tensor is used in place); row (b, t) counts iff t < clamp(lengths[b], 0, t_len) - drop_last (lengths = NULL:
 * t_len everywhere).  Rows that do not count enter the Gram as zeros: no compaction, no host sync.  out2 = {effective rank,
 * number of valid rows}; sv_or_null: NULL or d doubles, the min(rows, d) singular values then zeros.  drop_last >= 0. */
int  umlh_effective_rank_seq(const float* z, int32_t b, int32_t t_len, int32_t d, int64_t ldb, int64_t ldt, const int64_t* lengths,
                             int32_t drop_last, double eps, double* out2, double* sv_or_null, void* scratch, uint64_t scratch_bytes,
                             void* stream);

/* ---- principal subspaces and SVCCA ----
 * The top-q eigenpairs of a feature Gram, on the machinery above: the tridiagonalisation keeps its reflectors, bisection
 * brackets the eigenvalues, inverse iteration on the tridiagonal (re-orthogonalised within clusters of close eigenvalues) gives
 * its eigenvectors and the reflectors are applied in reverse.  Each vector's largest-magnitude component is positive (the first
 * one on ties).  Standardised means the reference's per-column (x - mean) / (std + 1e-8) with the unbiased std
 * (MultiBench/metrics.py:132-135): column means in a first pass, the centred Gram Gc in a second, G = D Gc D with
 * D_j = 1 / (sqrt(Gc_jj / (n - 1)) + 1e-8); a constant column is an exactly zero row and column of G.
 * Envelope: 2 <= n < 2^31, 1 <= d <= 512, 1 <= q <= min(n, d_a, d_b, 64), d <= ld < 2^31.  Every argument check happens before
 * any HIP call; fixed iteration counts and summation orders: results are bitwise reproducible for given arguments. */

/* Scratch bytes of umlh_svcca, or of umlh_principal_subspace when d_b = 0 (then d_a = d): O(chunks max(d)^2), no n x d term.
 * 0 on invalid arguments. */
uint64_t umlh_subspace_scratch_bytes(int64_t n, int32_t d_a, int32_t d_b, int32_t q);
/* evals[q] (descending) and evecs[d, q] (row-major, orthonormal columns): the top-q eigenpairs of the standardised Gram
 * (standardize = 1) or of the plain a^T a (standardize = 0: sqrt(evals) are the first q values of umlh_svdvals). */
int  umlh_principal_subspace(const float* a, int64_t n, int32_t d, int64_t ld_row, int32_t q, int32_t standardize, double* evals,
                             double* evecs, void* scratch, uint64_t scratch_bytes, void* stream);
/* AlignmentMetrics.svcca(a, b, cca_dim = q) (metrics.py:129-160) in closed form: the mean of the canonical correlations rho
 * between the top-q left singular subspaces of the two standardised views, rho = sqrt(eig(M^T M)) clamped to [0, 1] with
 * M = L_a^(-1/2) V_a^T C V_b L_b^(-1/2), (L, V) the top-q eigenpairs of each standardised Gram and C the standardised
 * cross-Gram.  out[1]; rho_or_null: NULL or [q], descending; evals_or_null: NULL or [2, q].  Equals the reference's value when
 * sigma_q > sigma_(q+1) in both views; at a tie the subspace is not unique and the answer is deterministic but arbitrary.
 * NaN when lambda_q <= d 2^-53 lambda_1 in either view (numerical rank below q, an all-constant view included) or when an
 * input is not finite. */
int  umlh_svcca(const float* a, const float* b, int64_t n, int32_t d_a, int32_t d_b, int64_t ld_a, int64_t ld_b, int32_t q,
                double* out, double* rho_or_null, double* evals_or_null, void* scratch, uint64_t scratch_bytes, void* stream);

/* ---- ABI v10: the two device operations of the MultiBench embedding capture (MultiBench/train.py:300-347,456-512; DESIGN
 * section 14).  Every argument check happens before any HIP call; everything runs on `stream`; outputs are device memory;
 * no float atomics: results are bitwise reproducible for given arguments, independent of stream and of the device's CU count. */

/* Valid rows of a block of sequences, packed: z[b, t, c] is read at z[b*ldb + t*ldt + c]. Row (b, t) counts iff
 * t < clamp(lengths[b], 0, t_len) - drop_last (lengths = NULL: t_len everywhere) -- the predicate of umlh_effective_rank_seq.
 * It is written bit for bit to out[(sum_{b' < b} rows(b') + t) * ldo + c]. Rows whose index is >= out_rows are not written;
 * rows_total[0] (device int64, always written) is the number of valid rows, so a caller can detect a mismatch.
 * No scratch, no host sync.  1 <= b <= 65535, t_len >= 1, d >= 1, non-overlapping ldb, ldt >= d, ldo >= d, drop_last >= 0,
 * out_rows >= 0; out must not overlap z. */
int  umlh_seq_compact(const float* z, int32_t b, int32_t t_len, int32_t d, int64_t ldb, int64_t ldt, const int64_t* lengths,
                      int32_t drop_last, float* out, int64_t ldo, int64_t out_rows, int64_t* rows_total, void* stream);

uint64_t umlh_paired_cosine_scratch_bytes(int64_t n, int32_t d);   /* 0 on invalid arguments */
/* out2 = {mean_i cos_i, sum_i cos_i}, cos_i = (a_i / max(|a_i|, eps)) . (b_i / max(|b_i|, eps)): each norm is clamped on
 * its own, as torch's F.cosine_similarity does (not the product). Dot products and squared norms are accumulated in fp64
 * from the fp32 rows. rows_or_null: NULL or n floats, cos_i rounded to fp32. n >= 1, d >= 1, lda, ldb >= d, eps >= 0. */
int  umlh_paired_cosine(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t n, int32_t d, double eps,
                        double* out2, float* rows_or_null, void* scratch, uint64_t scratch_bytes, void* stream);

/* ---- ABI v11: the per-step logged statistics of the MultiBench training loop (MultiBench/train.py:403-426):
 * train/trivial_loss_* ("predict the next frame by copying this one") and train/recon_y_loss (the masked next-step MSE of the
 * reconstruction) of a block of padded sequences, in one pass.  x[b, t, c] is read at x[b*ldb + t*ldt + c], recon[b, t, c] at
 * recon[b*ldb_r + t*ldt_r + c] (floats).  With len_b = clamp(lengths[b], 0, t_len) (lengths = NULL: t_len everywhere) and every
 * sum over b, 0 <= t < t_len - 1 and all d columns:
 *   trivial_num = sum [t < len_b]     (x[b,t,c]     - x[b,t+1,c])^2,   trivial_cnt = d * #{(b,t): t < len_b}
 *   recon_num   = sum [t + 1 < len_b] (recon[b,t,c] - x[b,t+1,c])^2,   recon_cnt   = d * #{(b,t): t + 1 < len_b}
 *   out4 = {trivial_num / (trivial_cnt + 1e-8), trivial_cnt, recon_num / (recon_cnt + 1e-8), recon_cnt}   (device doubles)
 * The two masks differ ON PURPOSE, as in the reference: it weights the trivial loss by mask[:, :-1], so the pair
 * (len_b - 1, len_b), which reaches one row into the padding, counts; recon_y_loss uses mask[:, 1:], where that pair does not.
 * recon_or_null = NULL: slots 2 and 3 are 0.  t_len = 1: no pair exists, all four slots are 0 (the reference's trivial branch for
 * T = 1 gives 0 where it does not raise, its recon_y_loss 0 / 1e-8).
 * A pair its predicate excludes is skipped, not multiplied by zero: Inf or NaN in x rows t > len_b or in recon rows
 * t >= len_b - 1 does not reach the result.  The reference's 0 * Inf would make both values NaN there; its loaders pad with
 * zeros, where the two agree.
 * Differences, squares and sums are fp64 from the fp32 inputs, counts exact integers; no float atomics; the grid and every
 * summation order are functions of (b, t_len, d) alone, so results are bitwise reproducible across calls, streams and the two
 * load paths (16-byte loads when d, all strides and both base addresses are multiples of 16 bytes, 4-byte loads otherwise) and
 * do not depend on the CU count.  No sequential chain of additions is longer than 4096 terms: the error against exact arithmetic
 * is below (4096 + log2(partials) + 4) 2^-53 < 5e-13 relative.  Two launches (partial sums into scratch, a fixed-order final),
 * no host sync.  Every argument check happens before any HIP call.
 * Envelope: 1 <= b <= 65535, t_len >= 1, d >= 1, non-overlapping ldb, ldt >= d as umlh_effective_rank_seq allows (the same for
 * ldb_r, ldt_r when recon is given), and b * ceil((t_len - 1) / 64) * ceil(d / 1024) <= 2^22 partial sums. */
uint64_t umlh_seq_step_stats_scratch_bytes(int32_t b, int32_t t_len, int32_t d);   /* 0 on invalid arguments */
int  umlh_seq_step_stats(const float* x, int64_t ldb, int64_t ldt, const float* recon_or_null, int64_t ldb_r, int64_t ldt_r,
                         int32_t b, int32_t t_len, int32_t d, const int64_t* lengths, double* out4, void* scratch,
                         uint64_t scratch_bytes, void* stream);

/* ---- rollout and spectral-bias spectra of the MultiBench loop (MultiBench/train.py:245-292).  Additive to
 * ABI v11: umlh_version() is unchanged, callers detect the feature by these symbols.  Every argument check happens before any
 * HIP call; everything runs on `stream`; outputs are device memory; no float atomics, no workgroup waits on another one. */

#define UMLH_ROLLOUT_MAX_LAYERS 16
#define UMLH_ROLLOUT_MAX_LDS    (160 * 1024)
#define UMLH_SPECTRUM_MAX_T     1024

typedef struct {
    int32_t Z;          /* encoder width                                   1..512   */
    int32_t d_ff;       /* feed-forward width                              1..2048  */
    int32_t D;          /* modality width (in- and out-projection)         1..1024  */
    int32_t n_layers;   /* 0..UMLH_ROLLOUT_MAX_LAYERS                               */
    int32_t steps;      /* generated frames                                0..4096  */
    float   eps;        /* LayerNorm eps, >= 0                                      */
} umlh_rollout_cfg_t;

/* The reference's rollout() for one modality in one launch.  At T = 1 the causal softmax over a single key is exactly 1, so a
 * layer's attention is out_proj(v_proj(h)) and every row evolves on its own.  For row r, with the 12 tensors per layer in the
 * order of umlh_encoder_layer_forward (W_v, b_v = rows 2Z..3Z-1 of in_proj_weight / in_proj_bias):
 *   cur_0 = x0[r]                                                     x0[r, c] read at x0[r*ldx + c]
 *   for s = 1..steps:
 *     h = Wc (W_in cur_{s-1} + b_in) + pos0                           conv_w_or_null [Z, Z], pos0_or_null [Z]: absent when NULL
 *     per layer: a = W_o (W_v h + b_v) + b_o;  h = LN1(h + a);  f = W_2 relu(W_1 h + b_1) + b_2;  h = LN2(h + f)
 *     cur_s = W_out h + b_out
 *   out[r*ldb + s*ldt + c] = cur_s[c] for s = 0..steps (s = 0 is the seed itself, the reference's pred_x = [x]).
 * Post-norm, biased variance from the differences to the mean, rsqrt(var + eps); relu is fmaxf(v, 0) (NaN -> 0); no dropout:
 * the reference's rollout runs in eval mode.  Products on the fp32 MFMA, fp32 accumulation in one fma chain per output whose
 * order depends on the two lengths of the product alone (blocks of 16 k ascending; inside a block k = k0 + i, k0 + 4 + i,
 * k0 + 8 + i, k0 + 12 + i for i = 0..3; a product with fewer than 8 tiles of 16 outputs cuts its blocks into up to 8 contiguous
 * runs whose sums are added in run order).  A workgroup owns 16 rows and reads nothing another workgroup writes: a row's trajectory is
 * bitwise the same whatever n, its index in the batch, the stream and the CU count.
 * Envelope: 1 <= Z <= 512, 1 <= d_ff <= 2048, 1 <= D <= 1024, 0 <= n_layers <= 16, 0 <= steps <= 4096, 1 <= n <= 2^20,
 * ldx >= D, ldt >= D, ldb >= steps*ldt + D (rows of out do not overlap); out may alias x0 only as a whole: x0[r] being out[r, 0, :] itself.  Weights are dense row-major
 * ([out, in], as nn.Linear keeps them).  There is no fallback: a shape outside the envelope is UMLH_E_INVALID. */
int  umlh_rollout(const umlh_rollout_cfg_t* cfg, const float* const* P, const float* conv_w_or_null, const float* pos0_or_null,
                  const float* w_in, const float* b_in, const float* w_out, const float* b_out, const float* x0, int64_t ldx,
                  int64_t n, float* out, int64_t ldb, int64_t ldt, void* stream);

/* torch.abs(torch.fft.rfft(x, dim=1)).mean(dim=(0, 2)) of a [b, t_len, d] block read at x[b*ldb + t*ldt + c], T = t_len:
 *   out[k] = (1 / (b d)) sum_{b,c} | sum_t x[b,t,c] e^{-2 pi i k t / T} |    for k = 0..T/2      (T/2 + 1 device doubles)
 * A direct DFT: cos / sin(2 pi ((k t) mod T) / T) from an fp64 table built once per workgroup, products and sums in fp64 from
 * the fp32 inputs, t ascending.  Two launches (partial sums into scratch, a fixed-order final), no host sync, no lengths mask
 * (the reference has none).  The grid and every summation order are functions of (b, t_len, d) alone: results are bitwise
 * reproducible across calls and streams and do not depend on the CU count.  No sequential chain of additions is longer than
 * 4096 terms.  Envelope: 1 <= t_len <= 1024, d >= 1, 1 <= b <= 2^20, non-overlapping ldb, ldt >= d as umlh_seq_step_stats
 * allows, and ceil(b / 16) * ceil(d / 16) <= 2^20 partial vectors. */
uint64_t umlh_seq_spectrum_scratch_bytes(int32_t b, int32_t t_len, int32_t d);   /* 0 on invalid arguments */
int  umlh_seq_spectrum(const float* x, int64_t ldb, int64_t ldt, int32_t b, int32_t t_len, int32_t d, double* out, void* scratch,
                       uint64_t scratch_bytes, void* stream);

/* ---- class index and class statistics of the fine-tune loop's feature capture (vision_language/finetune.py:222-231; DESIGN
 * section 18).  Additive to ABI v11: umlh_version() is unchanged, callers detect the feature by these symbols.  Every argument
 * check happens before any HIP call and names the function and the argument; everything runs on `stream`; outputs are device
 * memory; no float atomics: results are bitwise reproducible across calls, streams and CU counts. */

/* A stable counting sort of the rows by label.  order (int32, room for n entries) lists the rows whose label lies in
 * [0, n_class), grouped by class in ascending class order and in ascending row order inside a class; offsets (int64,
 * n_class + 1 entries): class c is order[offsets[c] .. offsets[c + 1]), offsets[n_class] the number of listed rows.  A row with
 * any other label appears nowhere (the reference's `== label` never selects it); entries of order past offsets[n_class] are
 * not written.  Five enqueues (one memset, four launches over blocks of 256 rows), no host sync; meant to run once per run.
 * Envelope: 1 <= n < 2^31, n_class >= 1, ceil(n / 256) * n_class <= 2^28 (the block-by-class count table in scratch). */
uint64_t umlh_class_index_scratch_bytes(int64_t n, int32_t n_class);          /* 0 on invalid arguments */
int  umlh_class_index(const int64_t* labels, int64_t n, int32_t n_class, int32_t* order, int64_t* offsets,
                      void* scratch, uint64_t scratch_bytes, void* stream);

/* Per class c, with R_c the rows order[offsets[c] .. offsets[c + 1]) of feats (row i at feats[i*ld .. i*ld + d)):
 *   means[c*ld_means + j] = (float)(sum_{i in R_c} x_ij / |R_c|), the sum in fp64 over R_c in order's sequence (cut into chunks
 *                           of 256 rows, 4 interleaved partial sums per chunk, added in a fixed order), rounded once to fp32;
 *   dist[c]               = (1 / |R_c|) sum_{i in R_c} sqrt(sum_j (x_ij - means[c, j])^2) in fp64 against the fp32 mean that was
 *                           written: the differences are formed explicitly (two fp32 values subtract exactly in fp64), squared,
 *                           summed in fp64 and passed through an fp64 sqrt -- never |x|^2 - 2 x.m + |m|^2;
 *   out2                  = {sum_c dist[c] / n_class, number of empty classes}.
 * An empty class gives a NaN mean row and a NaN dist[c] (the mean of an empty slice), so out2[0] is NaN if any class is empty,
 * as np.mean of the reference's list is.  A non-finite value in a row reaches that row's class only.
 * The plan is not trusted: offsets is read through its running maximum clamped to [0, n] (disjoint ranges whatever it holds;
 * unchanged when it is a valid plan), and an entry of order outside [0, n) is skipped and does not count towards |R_c|.  order
 * must have room for n entries.  Nothing is written outside means[c, 0 .. d), dist[0 .. n_class) and out2[0 .. 2).
 * A class of any size works: one of at most 256 rows is read twice, back to back, by one workgroup; a longer one is spread
 * over one workgroup per 256 rows.  Both load paths (16-byte loads when d, ld, ld_means and both base addresses are multiples
 * of 16 bytes, 4-byte loads otherwise) add in the same order.  At most five launches, no host sync.
 * Envelope: 1 <= n < 2^31, d >= 1, n_class >= 1, ld >= d, ld_means >= d, means must not overlap feats. */
uint64_t umlh_class_stats_scratch_bytes(int64_t n, int32_t d, int32_t n_class);   /* 0 on invalid arguments */
int  umlh_class_stats(const float* feats, int64_t ld, int64_t n, int32_t d, const int32_t* order, const int64_t* offsets,
                      int32_t n_class, float* means, int64_t ld_means, double* dist, double* out2,
                      void* scratch, uint64_t scratch_bytes, void* stream);

/* ---- class-wise validation report: the top-k classes of every row and per-class counts of them (the `val_classwise` slot of
 * the fine-tune loop's result, vision_language/finetune.py:121, which the reference never fills).  Additive to
 * ABI v11: umlh_version() is unchanged, callers detect the feature by these symbols.  Handle-free: x is row-major fp32 [n, d]
 * with row stride ldx >= d (feature rows), w fp32 [n_class, d] with row stride ldw >= d (the head's weight rows; the packed
 * [weight | bias | pad] rows of a bias head are read in place with ldw > d), bias_or_null fp32 [n_class] dense,
 * scale_dev_or_null ONE fp32 in device memory (NULL = 1; it is never read on the host).  The logit of row i and class j is
 *   z_ij = scale * (x_i . w_j + b_j).
 * No n x n_class array is formed and no reduction uses a float atomic.  Every argument check happens before any HIP call and
 * names the function and the argument; everything runs on `stream`; outputs are device memory.
 * Envelope: 1 <= k <= 24, k <= n_class < 2^31, 1 <= n < 2^31, d >= 1, ldx >= d, ldw >= d, splits >= 0 (0 = auto); anything else
 * is UMLH_E_INVALID.
 *
 * Order rule: per row the k classes with the largest z, ordered by (z descending, class index ascending) -- exact ties go to
 * the smaller index, whatever the sign of scale (a negative scale ranks by the negated pre-scale value; a zero scale ties every
 * class and returns 0 .. k-1).
 * Two stages.  (1) Candidates: the score sign(scale) * (x.w_j + b_j) with x.w_j on the f32 MFMA (a k-ordered fp32 fma chain, one
 * fp32 addition of the bias); the kc = min(k + 8, n_class) best under the strict order (score descending, index ascending) are
 * kept by the 32-row strip / 256-column tile / column-chunk scheme of umlh_align_knn.  (2) The candidates are re-evaluated as
 * z = (double)scale * (sum_k (double)x_k (double)w_jk + (double)b_j) in a fixed order and re-ranked by (z, index); the first k
 * are the answer and logit is z rounded once to fp32.  The result is bitwise independent of `splits` and reproducible across
 * calls and streams.  Both load paths of stage 1 (16-byte loads when d, ldx, ldw are multiples of 4 and both base addresses of
 * 16 bytes; 4-byte loads otherwise) form the same fma chains.
 * Index-range guarantee: every value written to cls is -1 or lies in [0, n_class), whatever the data.  List slots that no class
 * filled (a row containing NaN, whose comparisons are all false; NaN weight rows leaving fewer than k classes) are never used
 * as addresses; the output positions they leave open get class -1 and a NaN logit.  Results for rows that contain Inf are
 * otherwise unspecified; other rows are unaffected. */

/* Scratch bytes of umlh_eval_topk with these arguments: O(n * kc * splits) with splits <= min(ceil(n_class / 256), 1024) and, in
 * auto mode, splits * n <= n + 16384: no n * n_class term.  0 on invalid arguments. */
uint64_t umlh_eval_topk_scratch_bytes(int64_t n, int64_t n_class, int32_t d, int32_t k, int32_t splits);
/* cls int32 [n, k]; logit_or_null fp32 [n, k] or NULL; both dense, every entry is written. */
int  umlh_eval_topk(const float* x, int64_t n, int32_t ldx, const float* w, int64_t n_class, int32_t ldw, int32_t d,
                    const float* bias_or_null, const float* scale_dev_or_null, int32_t k, int32_t splits,
                    int32_t* cls, float* logit_or_null, void* scratch, uint64_t scratch_bytes, void* stream);
/* Class-wise counts from cls int32 [n, k] (dense; what umlh_eval_topk wrote, or any list) and labels int64 [n].  Every output
 * is ADDED INTO (64-bit integer atomics: exact and reproducible in any order), so a table can be fed in slabs; the caller
 * zeroes the outputs before the first slab.  With pred_i = cls[i, 0], for every row i:
 *   label_i outside [0, n_class):  misc2[0] += 1, and the row counts nowhere else;
 *   otherwise  support[label_i] += 1, and
 *     pred_i outside [0, n_class) (the -1 of a NaN row; never used as an address):  misc2[1] += 1, nothing else;
 *     otherwise  hit1[label_i] += (pred_i == label_i),  hitk[label_i] += (label_i among cls[i, 0 .. k)),
 *                confusion[label_i * n_class + pred_i] += 1   (row = true class, column = predicted class).
 * support, hit1, hitk int64 [n_class]; confusion_or_null int64 [n_class, n_class] dense or NULL (off); misc2 int64 [2].
 * One launch, no scratch.  Envelope: 1 <= k <= 24, 1 <= n < 2^31, 1 <= n_class < 2^31. */
int  umlh_eval_classwise(const int32_t* cls, int64_t n, int32_t k, const int64_t* labels, int64_t n_class,
                         int64_t* support, int64_t* hit1, int64_t* hitk, int64_t* confusion_or_null, int64_t* misc2, void* stream);

/* ---- outlier clamp and feature preparation of the alignment metrics: the module-level remove_outliers and
 * compute_knn_accuracy of vision_language/metrics.py (the same in MultiBench/ and Gaussian_experiment/).
 * Additive to ABI v11: umlh_version() is unchanged, callers detect the feature by these symbols.  Features are row-major fp32
 * [n, d] with row stride ld >= d.  |x| is ordered by key = bits(x) & 0x7fffffff as an unsigned integer: the order of the
 * absolute values, -0.0 equal to +0.0, every NaN pattern above Inf (where torch.sort puts NaN).  Order statistics are found by
 * an MSB-first radix select (four 8-bit digits), never by a sort: they are exact, so every result below is bitwise
 * reproducible across calls and streams; counters are integers and no sum uses a float atomic.  Every argument check happens
 * before any HIP call; `scratch` is caller device memory of at least umlh_outlier_scratch_bytes(kind, n, d) bytes; everything
 * runs on `stream` and nothing is read back to the host.
 * Envelope: n >= 1, 1 <= d < 2^31, ld >= d, n * d < 2^40; anything else is UMLH_E_INVALID. */
#define UMLH_OUTLIER_ROW_QUANTILE 0
#define UMLH_OUTLIER_ABS_KTH      1
#define UMLH_OUTLIER_KNN_ACCURACY 2
/* Row widths at which umlh_row_abs_quantile and umlh_clamp_rows(normalize = 1) change kernels: up to WAVE_COLS columns a wave
 * works on a row (four rows per workgroup); up to LDS_COLS a workgroup reads its row from memory once and keeps it in LDS
 * (60 KiB: two workgroups per CU); a longer row is streamed once per pass. */
#define UMLH_ROW_QUANTILE_WAVE_COLS 1024
#define UMLH_ROW_QUANTILE_LDS_COLS  15360

/* Scratch bytes of the entry point `kind` (above); for UMLH_OUTLIER_KNN_ACCURACY d is the list width m.  0 on invalid
 * arguments (unknown kind, n < 1, d < 1, d >= 2^31, n * d >= 2^40; n >= 2^31 for the accuracy). */
uint64_t umlh_outlier_scratch_bytes(int32_t kind, int64_t n, int64_t d);
/* torch.quantile(feats.abs().flatten(start_dim=1), q, dim=1).mean() (metrics.py:336).  With s the ascending |x| of a row,
 * pos = q * (d - 1) in double, lo = floor(pos), hi = min(lo + 1, d - 1):
 *   lo_val[i] = s[lo], hi_val[i] = s[hi]                              (fp32 [n]; either may be NULL)
 *   quant[i]  = s[lo] + (s[hi] - s[lo]) * (pos - lo)                  formed in double, rounded once (fp32 [n], required)
 *   mean64[0] = sum_i quant[i] / n in double, in a fixed order        (may be NULL);   q_val[0] = (float)mean64 (required)
 * A row that holds a NaN gets quant = NaN (as torch.quantile) while its lo_val and hi_val follow the key order; mean64 and q_val
 * are then NaN.  0 <= q < 1 (q = 1 is the caller's identity case, metrics.py:328-329). */
int  umlh_row_abs_quantile(const float* x, int64_t n, int64_t d, int64_t ld, double q, float* lo_val, float* hi_val,
                           float* quant, double* mean64, float* q_val, void* scratch, uint64_t scratch_bytes, void* stream);
/* feats.view(-1).abs().sort().values[k] (metrics.py:333): the element of rank k (0-based, ascending) among all n * d values
 * of |x| -> out[0], one fp32 in device memory, bit-exact.  Four launches (one per digit); every workgroup adds its LDS counters
 * into 64-bit global counters and the one that takes the last ticket picks the digit: no workgroup waits for another.
 * 0 <= k < n * d. */
int  umlh_abs_kth(const float* x, int64_t n, int64_t d, int64_t ld, int64_t k, float* out, void* scratch,
                  uint64_t scratch_bytes, void* stream);
/* feats.clamp(-q_val, q_val) (metrics.py:341) with q_val ONE fp32 in device memory (never read on the host), torch.clamp's
 * tensor-bound semantics: a NaN element stays NaN, a NaN bound makes every element NaN, otherwise min(max(x, -q), q), so
 * +-Inf become +-q and -0.0 stays -0.0.  normalize != 0: the clamped row is then divided by max(|row|_2, 1e-12)
 * (F.normalize(dim=-1)) in the same launch; |row|^2 is summed in double in a fixed order, the division is one fp32 division.
 * out is row-major [n, d] with its own row stride ldo >= d; out == x (with ldo == ldx) works in place.  No scratch. */
int  umlh_clamp_rows(const float* x, int64_t n, int64_t d, int64_t ldx, const float* q_val, int32_t normalize, float* out,
                     int64_t ldo, void* stream);
/* compute_knn_accuracy(knn) (metrics.py:258-269): the share of rows i of the int32 list knn [n, m] that contain the value
 * i (m = topk, or topk^2 for the reference's knn_A[knn_B] of shape [n, k, k]).  Hits are summed as integers and the mean is
 * formed once in double -> out[0].  Row i starts at knn + i * ld, ld >= m; ld = 0 makes every row read the same m entries: the
 * share of the indices 0 .. n-1 found anywhere in ONE table of m entries, which is what the reference's expression evaluates to
 * for a 2-D list [n, k] (its comparison against arange(n).view(-1, 1, 1) broadcasts to [n, n, k]; m = n * k there).
 * 1 <= n < 2^31, 1 <= m < 2^31. */
int  umlh_knn_accuracy(const int32_t* knn, int64_t n, int64_t m, int64_t ld, double* out, void* scratch, uint64_t scratch_bytes,
                       void* stream);

/* ---- robustness test sets of the affect datasets: time-series noise on a table of the device loader below (the table layout
 * and its envelope are that section's; this one stands in front of it because the loader section is pinned as the last). ---- */
/* The time-series noise of the robustness test sets (MultiBench/robustness/timeseries_robust.py: white_noise, structured_drop,
 * random_drop) on one table, src -> dst, both [n, t_len, d].  Additive to ABI v11.
 * A unit shares one draw: unit_rows = t_len makes the unit a sample (what get_data.py:349-404 gets by handing whole tables to
 * the noise function), unit_rows = 1 a time step; anything else is UMLH_E_INVALID.  Unit u covers the rows u * unit_rows ... of
 * the flattened [n * t_len, d] table.  eps (double) and keep (uint8) are DEVICE arrays of n * t_len / unit_rows entries, drawn
 * on the host in the reference's order; either may be NULL (no noise / nothing dropped).  Per element x of unit u:
 *   keep[u] == 0          -> +0.0f, WRITTEN (an assignment as in the reference: NaN, Inf and negative values become +0.0)
 *   otherwise, with eps   -> (float)((double)x + eps[u]): one fp64 add, one rounding (eps[u] = 0.0 turns -0.0 into +0.0)
 *   otherwise, eps NULL   -> x, bit for bit
 * elem_p > 0 additionally writes +0.0f to element i (flat index in the table) when keep_elem(seed, i, thresh) of the project's
 * counter stream is false, thresh formed from elem_p as umlh_dropout forms it from p (elem_p = 1 drops every element); no
 * rescaling.  This is random_drop; it is NOT draw-compatible with numpy, where one host uniform is drawn per element.
 * elem_p = 0: off.  elem_p outside [0, 1] (NaN included) is UMLH_E_INVALID.
 * dst may be src (in place); a partial overlap is UMLH_E_INVALID.  start_out (optional, int32 [n]) receives
 * umlh_seq_first_nonzero of the RESULT, bit-equal to that function run on dst, from the same pass.  One launch, no scratch. */
int  umlh_seq_perturb(const float* src, int64_t n, int32_t t_len, int32_t d, int32_t unit_rows, const double* eps,
                      const uint8_t* keep, float elem_p, uint64_t seed, float* dst, int32_t* start_out, void* stream);

/* ---- MIMIC loader: table build, tabular noise and batches of MultiBench/datasets/mimic/get_data.py and
 * MultiBench/robustness/tabular_robust.py (kernels: umlh_kernels_tabular.hip).  Additive to ABI v11.  In
 * front of the affect loader's section for the same reason as the one above.  Every argument check happens before any HIP call
 * and names the function and the argument; everything runs on `stream`; no atomics on global memory: results are bitwise
 * reproducible across calls and streams. ---- */
/* get_data.py:38-51 in one call, on a [rows, d] matrix x (row r at x + r*ldx; float, or double with x_is_f64 = 1):
 *   v = x[r, c], or +0.0 where x[r, c] is NaN or +-Inf                   (X[isinf] = 0; X[isnan] = 0)
 *   stats[c] = mean_r v,  stats[d + c] = sqrt(mean_r (v - stats[c])^2)   (population std, as np.std; 2 d device doubles)
 *   out[r*ldo + c] = (float)((v - stats[c]) / stats[d + c])              (v in the source's precision: one fp64 subtraction,
 *                                                                         one fp64 division, one rounding)
 * The sums are those of umlh_seq_column_standardize: fp64, per row chunk and then in chunk order, on the same column-sum core
 * and the same plan -- on a float source without non-finite values stats and out equal that function's bit for bit.  A zero
 * std is NOT special-cased: 0 / 0 = NaN and v / 0 = +-Inf, as numpy gives.  out == x (with ldo == ldx) works in place for a
 * float source; any other overlap of out with a float x, and any overlap with a double x, is UMLH_E_INVALID.  x itself is
 * never written otherwise (the reference cleans its arrays in place).  Five launches, no host sync.  Envelope as umlh_seq_column_standardize: 1 <= rows < 2^40,
 * 1 <= d <= 2^20, ldx >= d, ldo >= d; scratch 8-byte aligned.  The size query does not end in _scratch_bytes (a closed family). */
uint64_t umlh_tab_standardize_scratch(int64_t rows, int32_t d);                  /* bytes; 0 on invalid arguments */
int  umlh_tab_standardize(const void* x, int32_t x_is_f64, int64_t rows, int32_t d, int64_t ldx, float* out, int64_t ldo,
                          double* stats, void* scratch, uint64_t scratch_bytes, void* stream);

/* add_tabular_noise (tabular_robust.py:7-52) on src [n, d] -> dst [n, d], fp32, row strides lds and ldd.  Per row i:
 *   1. drop:   v[j] = drop[i*d + j] ? +0.0f : src[i, j]      (an assignment: NaN, Inf and negative values become +0.0)
 *   2. carry:  out[0] = v[0];  out[j] = carry[i*(d-1) + j-1] ? out[j-1] : v[j]   for j >= 1
 * Step 2 is what the reference's swap_entry DOES.  Despite its name it swaps nothing: `data[i][j] = data[i][j-1]` copies the
 * already updated left neighbour to the right, and its second assignment `data[i][j-1] = data[i][j]` writes back the value it
 * has just read.  out[j] is therefore the dropped value of the last column <= j that does not carry: a prefix maximum over
 * column indices, not a serial chain.  Rows of at most 64 columns take a thread each; wider rows take a wave each with a scan
 * per 64-column chunk, the last result carried into the next chunk.  Everything else moves bit for bit (NaN payloads, -0.0).
 * drop ([n, d]) and carry ([n, d-1]) are DEVICE uint8 arrays drawn on the host in the reference's order (all of drop_entry's
 * uniforms, then all of swap_entry's); either may be NULL; with d = 1 carry is not read.  Counter-stream mode: with drop NULL
 * and p_drop > 0 element (i, j) drops when keep_elem(seed, i*d + j, thresh(p_drop)) of the project's counter stream is false,
 * thresh as umlh_dropout forms it (p = 1 takes every element); with carry NULL and p_carry > 0 column j >= 1 carries by the
 * same rule on seed + 1.  This mode is NOT draw-compatible with numpy.  A given mask wins over its p.  p outside [0, 1] (NaN
 * included) is UMLH_E_INVALID.  dst may be src with ldd == lds (in place); any other overlap is UMLH_E_INVALID.
 * Envelope: 1 <= n < 2^31, 1 <= d <= 2^20, lds >= d, ldd >= d.  One launch, no scratch. */
int  umlh_tab_perturb(const float* src, int64_t n, int32_t d, int64_t lds, const uint8_t* drop, const uint8_t* carry, float p_drop,
                      float p_carry, uint64_t seed, float* dst, int64_t ldd, void* stream);

/* One launch forms a batch from tables of different row widths (MIMIC: the static table, 5 words per sample, and the flattened
 * series, 24 * 12 = 288).  srcs, widths, outs are HOST arrays of n_src <= UMLH_SEQ_GATHER_MAX_SOURCES entries: source m is a
 * dense fp32 table [n, widths[m]], outs[m] a dense block [b, widths[m]]; a NULL source is skipped (its widths and outs
 * entries are not read), at least one must be given.  ids is int64 device memory [b]:
 *   outs[m][j, :] = srcs[m][ids[j], :], bit for bit;   a zero row for an id outside [0, n), which is never used as an address.
 * Repeated ids are fine.  Nothing is written outside the b * widths[m] words of a block.  Envelope: 1 <= b <= 65535,
 * 1 <= widths[m] < 2^31, 1 <= n < 2^31.  The step-path kernel of the MIMIC loader, as umlh_seq_gather_pad is the affect
 * loader's (that one needs one t_len for all its sources). */
int  umlh_rows_gather(const float* const* srcs, const int32_t* widths, int32_t n_src, int64_t n, const int64_t* ids, int32_t b,
                      float* const* outs, void* stream);

/* ---- the Gaussian toy's SharedAutoencoder (Gaussian_experiment/model.py:5-59, main.py:33-91): the forward of either or both
 * views as one call, and whole training steps (both views, forward, MSE, backward, optimizer update) as two launches each
 * (kernels: umlh_kernels_gauss.hip).  Additive to ABI v11: umlh_version() is unchanged, callers detect the
 * feature by these symbols.  The section sits in front of the affect loader's for the same reason as the one above.
 * Dimensions: dim_obs = D, dim_common = C, dim_latent = L.  P is a HOST array of 16 device pointers to dense row-major fp32
 * tensors in the model's state_dict order: in_head_x.{weight [C, D], bias [C]}, in_head_y, shared_encoder.0 [L, C],
 * shared_encoder.2 [L, L], shared_decoder.0 [L, L], shared_decoder.2 [C, L], out_head_x [D, C], out_head_y.  Per view v in
 * {x, y}, row r of that view:
 *   a0 = table_v[idx_v[r]]                       (row gather by int32 index; idx NULL = rows 0 .. n - 1; row i at table + i*ld)
 *   a1 = W_in_v a0 + b      a2 = relu(W_e0 a1 + b)     a3 = W_e2 a2 + b        (a3: the embedding, get_embeddings)
 *   a4 = relu(W_d0 a3 + b)  a5 = W_d2 a4 + b           rec = W_out_v a5 + b
 *   loss_v = mean over rows_v * D of (rec - a0)^2      (0 for an absent view)
 * Products: fp32 MFMA with fp32 accumulation, one fma chain per output in an order that depends on the reduction length alone
 * (blocks of 16 k ascending, MFMA i of a block takes k0 + i, k0 + 4 + i, k0 + 8 + i, k0 + 12 + i); the bias is one fp32 add behind
 * it; relu is fmaxf(v, 0), its backward keeps the gradient where the saved activation is > 0 (as umlh_relu_backward).  The loss
 * squares and sums are fp64 from the fp32 residuals, in a fixed order, rounded once to fp32.  A row's reconstruction and embedding
 * depend on the parameters and the row alone, not on its position or on the other rows.
 * Every argument check happens before any HIP call and names the function and the argument; everything runs on `stream`, no host
 * sync; no float atomics, no workgroup waits on another; grids and summation orders are functions of the shapes alone: results are
 * bitwise reproducible across calls, streams and CU counts.
 * Envelope: 1 <= D <= 1024, 1 <= C <= 512, 1 <= L <= 512, ld >= D; there is no fallback: anything else is UMLH_E_INVALID. */
#define UMLH_AE_MAX_OBS        1024
#define UMLH_AE_MAX_COMMON     512
#define UMLH_AE_MAX_LATENT     512
#define UMLH_AE_MAX_EVAL_ROWS  1048576   /* rows per view of one umlh_ae_forward                    */
#define UMLH_AE_MAX_BATCH      65536     /* rows per view and step, steps per umlh_ae_train_steps   */
typedef struct {
    int32_t dim_obs;        /* D */
    int32_t dim_common;     /* C */
    int32_t dim_latent;     /* L */
} umlh_ae_cfg_t;

/* Scratch bytes of umlh_ae_forward (train = 0: the tiles' loss partials; rows up to UMLH_AE_MAX_EVAL_ROWS) or of
 * umlh_ae_train_steps (train = 1: also a0 .. a5 and the six dZ blocks of every row, 2 D + 4 C + 6 L floats per row; rows up to
 * UMLH_AE_MAX_BATCH), computed from the one layout plan the launchers use; 0 on invalid arguments (both views absent included).
 * The fourth argument and the name are this header's: one plan serves both entry points, and the name does not end in
 * _scratch_bytes (a closed family, pinned value for value by a recorded file). */
uint64_t umlh_ae_scratch(const umlh_ae_cfg_t* cfg, int32_t rows_x, int32_t rows_y, int32_t train);

/* The evaluation forward over n_x rows of x and n_y rows of y (0 = view absent, its table is not read; at least one present).
 * Outputs, each optional (NULL): losses [2] = {loss_x, loss_y}; rec_x [n_x, D], rec_y [n_y, D]; emb_x [n_x, L], emb_y [n_y, L],
 * dense fp32 device memory.  A view whose loss and reconstruction are both unwanted stops behind its embedding.  One launch, one
 * more for the losses.  scratch: umlh_ae_scratch(cfg, n_x, n_y, 0), 8-byte aligned. */
int  umlh_ae_forward(const umlh_ae_cfg_t* cfg, const float* const* P, const float* x, int64_t ldx, const int32_t* idx_x, int32_t n_x,
                     const float* y, int64_t ldy, const int32_t* idx_y, int32_t n_y, float* losses, float* rec_x, float* rec_y,
                     float* emb_x, float* emb_y, void* scratch, uint64_t scratch_bytes, void* stream);

/* n_steps consecutive training steps, enqueued by a C loop: two launches per step whatever the dimensions, no host sync.  Step s
 * (0-based) takes the rows idx_x[s*batch_x .. (s+1)*batch_x) of x and idx_y[s*batch_y ..) of y: DEVICE int32 arrays of
 * n_steps * batch entries.  THE CALLER GUARANTEES that every index is a row of its table: an index is used as an address
 * unchecked.  A NULL index array means rows 0 .. batch - 1 in every step.  batch 0 = the view is absent (at least one present).
 * M and V are HOST arrays of 16 device pointers like P: the moments of the tensors (momentum_buffer / exp_avg, and exp_avg_sq).
 * P, M and V are updated IN PLACE, element by element, by the update of umlh_optimizer_step (sgd, adam, adamw) with the step
 * number first_step + s; under sgd V is neither read nor written and may be NULL.
 *   backward_y = 1 (the reference's mode 'xy'): dRec_v = alpha_v * 2 / (rows_v * D) * (rec - a0) with the factor formed in double
 *     and rounded once; loss = alpha_x * loss_x + alpha_y * loss_y as two fp32 products and one add, no contraction.
 *   backward_y = 0 (mode 'x', main.py:54-56): the y view runs forward only; loss_y is reported, loss = loss_x; in_head_y.*,
 *     out_head_y.* and their moments are not touched at all; the shared layers receive the x rows' gradient alone.
 * The gradient of a tensor is summed over the x rows, then the y rows: wave w of its tile's workgroup takes the 4-row blocks
 * w, w + 4, ... of a view in ascending order (one MFMA each) and the four wave sums are added in wave order; a bias gradient adds
 * the same blocks per lane and the 16 lane sums in a fixed order.  Every weight element is owned by one thread of one workgroup.
 * losses: [n_steps, 3] fp32 = loss_x, loss_y, loss of each step.  scratch: umlh_ae_scratch(cfg, batch_x, batch_y, 1), 8-byte
 * aligned, reused by every step.  Envelope: 0 <= batch <= 65536 per view, 1 <= n_steps <= 65536. */
int  umlh_ae_train_steps(const umlh_ae_cfg_t* cfg, float* const* P, float* const* M, float* const* V, const float* x, int64_t ldx,
                         const int32_t* idx_x, int32_t batch_x, const float* y, int64_t ldy, const int32_t* idx_y, int32_t batch_y,
                         int32_t n_steps, int32_t backward_y, float alpha_x, float alpha_y, int32_t optimizer, double lr,
                         int64_t first_step, double beta1, double beta2, double eps, double momentum, double weight_decay,
                         float* losses, void* scratch, uint64_t scratch_bytes, void* stream);

/* Grouped forms: up to UMLH_AE_MAX_GROUP independent runs (members) in one launch pair per step, for sweeps whose single runs
 * leave most of the device idle.  Additive to ABI v11.  A member is described by the arguments of the single-run entry point and
 * keeps their meaning field for field: the envelope, NULL index arrays, an absent view, V == NULL under sgd, backward_y = 0.
 * Members may differ in every field, cfg included; all take the same n_steps.
 *   BIT IDENTITY: after umlh_ae_train_steps_grouped every member's P, M, V and losses hold, bit for bit, what
 *   umlh_ae_train_steps with that member's arguments leaves; every output of umlh_ae_forward_grouped is bit for bit that of
 *   umlh_ae_forward.  A workgroup of a grouped launch finds its member and then runs the single-run kernel's own body.
 * Members may share feature tables and index arrays.  They may NOT share parameter or moment tensors: a device pointer that
 * occurs twice among all members' P / M / V (V of an sgd member is not looked at) is UMLH_E_INVALID.
 * Every check happens before the first HIP call; the message names the function, the member (`member i`) and the argument.
 * The members' descriptors and the optimizer constants of every step (formed on the host as by umlh_ae_train_steps) reach the
 * device in ONE asynchronous upload per call from pinned staging that is reused behind events: no upload per step and no host
 * synchronisation (a call waits only for the upload of the call before the previous one on the same device).  The device side
 * of these tables lives in the caller's scratch, in front of one private region per member: the size queries count both, which is
 * why the training query takes n_steps.  Launches per step: two, whatever n_items is.  scratch: 8-byte aligned. */
#define UMLH_AE_MAX_GROUP 64
typedef struct {                 /* one run of a training group: the arguments of umlh_ae_train_steps */
    umlh_ae_cfg_t cfg;
    float* const* P; float* const* M; float* const* V;     /* HOST arrays of 16 device pointers */
    const float* x; int64_t ldx; const int32_t* idx_x; int32_t batch_x;
    const float* y; int64_t ldy; const int32_t* idx_y; int32_t batch_y;
    int32_t backward_y; float alpha_x, alpha_y;
    int32_t optimizer; double lr; int64_t first_step; double beta1, beta2, eps, momentum, weight_decay;
    float* losses;               /* [n_steps, 3] */
} umlh_ae_group_item_t;
typedef struct {                 /* one run of an evaluation group: the arguments of umlh_ae_forward */
    umlh_ae_cfg_t cfg; const float* const* P;
    const float* x; int64_t ldx; const int32_t* idx_x; int32_t n_x;
    const float* y; int64_t ldy; const int32_t* idx_y; int32_t n_y;
    float* losses; float* rec_x; float* rec_y; float* emb_x; float* emb_y;
} umlh_ae_eval_item_t;
/* Scratch bytes of the grouped calls, from the one plan their launchers use: a multiple of 256; 0 on invalid arguments (items
 * NULL, n_items outside 1..UMLH_AE_MAX_GROUP, n_steps outside 1..UMLH_AE_MAX_BATCH, a member outside the single-run envelope). */
uint64_t umlh_ae_group_scratch(const umlh_ae_group_item_t* items, int32_t n_items, int32_t n_steps);
uint64_t umlh_ae_eval_group_scratch(const umlh_ae_eval_item_t* items, int32_t n_items);
int  umlh_ae_train_steps_grouped(const umlh_ae_group_item_t* items, int32_t n_items, int32_t n_steps,
                                 void* scratch, uint64_t scratch_bytes, void* stream);
int  umlh_ae_forward_grouped(const umlh_ae_eval_item_t* items, int32_t n_items,
                             void* scratch, uint64_t scratch_bytes, void* stream);

/* ---- device loader of the affect datasets (mosi, mosei, humor, sarcasm): what Affectdataset.__getitem__ and the _process_1
 * collate of MultiBench/datasets/affect/get_data.py:159-261,418-444 do per sample and per batch on the host, as three table-build
 * passes and one step-path kernel.  Additive to ABI v11: umlh_version() is unchanged, callers detect the
 * feature by these symbols.  A table is dense row-major fp32 [n, t_len, d] (sample, time, feature).  Every argument check
 * happens before any HIP call and names the function and the argument; everything runs on `stream`; outputs are device memory;
 * no atomics on global memory: results are bitwise reproducible across calls and streams.
 * Envelope of a table: 1 <= n < 2^31, t_len >= 1, 1 <= d <= 2^20, t_len * d < 2^31; anything else is UMLH_E_INVALID. */
#define UMLH_SEQ_GATHER_MAX_SOURCES 3

/* start[i] (int32 [n]) = the row of the first element of x[i] that compares != 0 -- a NaN counts, -0.0 does not, as
 * text.nonzero()[0][0] (get_data.py:209) -- and t_len when sample i has none (the reference drops or crashes on such a sample;
 * the caller drops it).  One launch. */
int  umlh_seq_first_nonzero(const float* x, int64_t n, int32_t t_len, int32_t d, int32_t* start, void* stream);

/* The reference's vision_norm (get_data.py:185-191) over the rows of a [rows, d] matrix (row r at x + r*ldx, rows = n * t_len
 * of a table, padding rows included):
 *   stats[c] = mean_r x[r, c],  stats[d + c] = sqrt(mean_r (x[r, c] - stats[c])^2)     (population std; 2 d device doubles)
 *   out[r*ldo + c] = (float)(((double)x[r, c] - stats[c]) / stats[d + c])
 * Sums in fp64 from the fp32 values, per row chunk and then in chunk order (the column-sum core of the probe's scaler
 * statistics); the second pass sums squared deviations from the mean the first one wrote.  A column with a zero std is NOT
 * special-cased: 0 / 0 = NaN and v / 0 = +-Inf, as numpy's expression gives.  out == x (with ldo == ldx) works in place.
 * Five launches, no host sync.  Envelope: 1 <= rows < 2^40, 1 <= d <= 2^20, ldx >= d, ldo >= d; scratch 8-byte aligned.
 * The size query does not end in _scratch_bytes: that family is closed (it is pinned value for value by a recorded file). */
uint64_t umlh_seq_column_standardize_scratch(int64_t rows, int32_t d);          /* bytes; 0 on invalid arguments */
int  umlh_seq_column_standardize(const float* x, int64_t rows, int32_t d, int64_t ldx, float* out, int64_t ldo, double* stats,
                                 void* scratch, uint64_t scratch_bytes, void* stream);

/* The reference's z_norm (get_data.py:223-226), in place: per sample i and column c over the rows t = s_i .. t_len - 1,
 * s_i = clamp(start[i], 0, t_len), L = t_len - s_i:
 *   mean = sum_t x / L and sd = sqrt(sum_t (x - mean)^2 / (L - 1)) in fp64 (t ascending, one chain each; the unbiased form),
 *   x[i, t, c] = nan_to_num((x[i, t, c] - (float)mean) / (float)sd) in fp32:  NaN -> 0, +Inf -> FLT_MAX, -Inf -> -FLT_MAX.
 * A constant column gives 0 / 0 and L = 1 gives sd = NaN: both become all 0.  Rows t < s_i are not touched.  One thread per
 * (sample, column): the result for a sample does not depend on n, on the grid or on the sample's position.  One launch. */
int  umlh_seq_standardize(float* x, int64_t n, int32_t t_len, int32_t d, const int32_t* start, void* stream);

/* One launch builds a batch in the _process_1 layout (get_data.py:418-444).  srcs, dims, outs are HOST arrays of n_src <= 3
 * entries: source m is a table [n, t_len, dims[m]], outs[m] a dense block [b, t_out, dims[m]]; a NULL source is skipped (its
 * dims and outs entries are not read), at least one must be given.  start (int32 [n]) and ids (int64 [b]) are device memory.
 * With s = clamp(start[ids[j]], 0, t_len) and len_j = min(t_len - s, t_out):
 *   outs[m][j, t, :] = srcs[m][ids[j], s + t, :] for t < len_j,   +0.0 for len_j <= t < t_out;      lengths[j] = len_j  (int64 [b])
 * t_out is the caller's (the host knows every length): the longest trimmed sequence of the batch reproduces pad_sequence; a
 * smaller one clips rows and lengths; a larger one pads further.  An id outside [0, n) gives a zero block and length 0 and is
 * never used as an address.  Repeated ids are fine.  Nothing is written outside the b * t_out * dims[m] words of a block and
 * lengths[0 .. b).  Envelope: every given source inside the table envelope above, 1 <= b <= 65535, t_out >= 1,
 * t_out * dims[m] < 2^31. */
int  umlh_seq_gather_pad(const float* const* srcs, const int32_t* dims, int32_t n_src, int64_t n, int32_t t_len,
                         const int32_t* start, const int64_t* ids, int32_t b, int32_t t_out, float* const* outs, int64_t* lengths,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UMLH_H */
