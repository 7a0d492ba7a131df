// Host side of the C ABI declared in include/umlh.h, the part that takes or builds a umlh_handle_t: argument checks, workspace
// partitioning, per-step launch sequences, the p2p / RCCL plumbing.  No allocation, no synchronisation.  (The stateless entry
// points are in umlh_ops.cpp, the encoder layers in umlh_encoder.cpp.)
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <new>

#include "umlh_host.h"
#include "umlh_launch.h"
#include "umlh_micro.h"
#include <mutex>

static thread_local char g_err[512] = "";
static int device_cus(int dev);

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

struct Layout {                 // workspace partition, in floats from the base
    long long dzt, h, dht, slabs_head, slabs_proj, partials, diag_part, grads, w16, iota, zeros, dbg, wpt16, wht16, xch, fuse_flags, w32s, total;
    long long ctl_tasks;        // one-launch step: task capacity of the control region at fuse_flags (step_ctl_at)
    int fwd_nq;                 // bf16 2-D forward (fwd_ce_bf16_q): class groups per row tile, 0 = the 1-D kernel
    long long mc_flags, mc_xchg, mc_tab, mc_desc;   // micro-step region (umlh_micro.h); mc_flags = 0: unsupported shape
    int mc_nwg, mc_nch, mc_cw;
    long long n_iota;
    int rcap_img, rcap_txt, ldz;     // padded row capacities
    int scap_head, scap_proj;        // split-K slab capacities
    long long n_head, n_proj;        // parameter counts
    int max_blocks;
};

static int split_cap(int M, int N) {
    long long tiles = (long long)((M + 127) / 128) * ((N + 127) / 128);
    long long want = 256 / tiles;
    if (want < 2) want = 2;           // image rows and text rows never share a slab (plan_splits)
    if (want > 64) want = 64;
    return (int)want;
}

// Modality-aligned split-K plan for dW_head: `r0` reduction rows of the image segment followed by `r1`
// of the text segment, at most `want` slabs of `chunk` rows (a multiple of `quantum`) each, every slab
// inside one modality.  Keeping the two partial sums in separate slabs makes the reference's
// per-modality gradients (finetune.py:190-191) by-products of the slab reduction.
struct SplitPlan { int chunk, n_img, n_txt; };
static SplitPlan plan_splits(int r0, int r1, int want, int quantum, int min_chunk) {
    SplitPlan sp = {min_chunk, 0, 0};
    const long long tot = (long long)r0 + r1;
    if (tot <= 0) return sp;
    int s0 = r0 > 0 ? (int)((want * (long long)r0 + tot / 2) / tot) : 0;
    if (r0 > 0 && s0 < 1) s0 = 1;
    if (r1 > 0 && s0 > want - 1) s0 = want - 1;
    int s1 = r1 > 0 ? want - s0 : 0;
    if (r1 > 0 && s1 < 1) s1 = 1;
    long long c0 = s0 > 0 ? (r0 + s0 - 1) / s0 : 0, c1 = s1 > 0 ? (r1 + s1 - 1) / s1 : 0;
    long long chunk = round_up(c0 > c1 ? c0 : c1, quantum);
    if (chunk < min_chunk) chunk = min_chunk;
    sp.chunk = (int)chunk;
    sp.n_img = (int)((r0 + chunk - 1) / chunk);
    sp.n_txt = (int)((r1 + chunk - 1) / chunk);
    return sp;
}

// ---- region descriptions: the size (in floats) and inner layout of every workspace region that more than one place has to
// know, each stated once.  make_layout sizes the regions with them; umlh_bind, the launches and the status / buffer queries
// find their words through them.  (The control words of the one-launch step: umlh_common.h; the micro-step regions: umlh_micro.h.) ----
// exchange granules (8 bytes) of the bf16 2-D forward
static long long xch_floats(const Layout& L) { return 2LL * (L.ldz / 128 + 2) * L.fwd_nq * 4 * 128; }
// gradient diagnostics: [head_step blocks][4] partial sums, then the ticket (diag_ticket)
static long long diag_part_floats(const Layout& L) { return 4 * ((L.n_head + 1023) / 1024 + 2); }
static const int DIAG_TICKET_FLOATS = 64;
// diagnostic stamps: [blocks][8 waves][8] u64
static long long dbg_floats(const Layout& L) { return (long long)L.max_blocks * 128; }
// gradient message [g_head | g_proj | g_scales(2) | scalars]; `diag`: the image and the text gradient of the head travel
// separately ([g_img | g_txt | ...], see dp_reduce_head).  The region holds the longer form.
static long long msg_head_floats(const Layout& L, bool diag) { return diag ? 2 * L.n_head : L.n_head; }
static long long msg_floats(const Layout& L, bool diag) { return msg_head_floats(L, diag) + L.n_proj + 2 + UMLH_N_SCALARS; }
static long long msg_cap_floats(const Layout& L) { return msg_floats(L, true); }

static bool make_layout(const umlh_config_t& c, Layout& L) {
    if (c.d_img < 1 || c.d_shared < 1 || c.num_classes < 1 || c.num_classes > 1024) return false;
    if (!c.has_proj && c.d_img != c.d_shared) return false;
    if (c.max_rows_img < 0 || c.max_rows_txt < 0 || c.max_rows_img + c.max_rows_txt < 1) return false;
    if (c.optimizer < UMLH_OPT_SGD || c.optimizer > UMLH_OPT_ADAMW) return false;
    if (c.precision != UMLH_PREC_FP32 && c.precision != UMLH_PREC_BF16) return false;
    // bf16 mode: the shared dim is the K of the fused forward (X tile staged in 128-wide K blocks); with img_proj the
    // image width is the K of H = X W_proj^T, whose row-major A operand is read in whole 64-wide chunks
    if (c.precision == UMLH_PREC_BF16 && (c.d_shared % 128 != 0 || (c.has_proj && c.d_img % 64 != 0))) return false;
    L.rcap_img = (int)round_up(c.max_rows_img, 256);
    L.rcap_txt = (int)round_up(c.max_rows_txt, 256);
    L.ldz = L.rcap_img + L.rcap_txt;
    L.n_head = (long long)c.num_classes * c.d_shared;
    L.n_proj = c.has_proj ? (long long)c.d_shared * c.d_img : 0;
    L.scap_head = split_cap(c.num_classes, c.d_shared);
    if (c.precision == UMLH_PREC_BF16 && L.scap_head < (L.ldz + 4095) / 4096 + 1) L.scap_head = (L.ldz + 4095) / 4096 + 1;
    L.scap_proj = c.has_proj ? split_cap(c.d_shared, c.d_img) : 0;
    if (c.has_proj && c.precision == UMLH_PREC_BF16 && L.scap_proj < (L.rcap_img + 4095) / 4096) L.scap_proj = (L.rcap_img + 4095) / 4096;
    L.max_blocks = L.ldz / 32 + 2;
    long long off = 0;
    auto take = [&](long long n) { long long o = off; off += round_up(n, 64); return o; };
    // fp32: dZ^T [C][ldz] floats.  bf16: [ldz/64][crows][64] shorts, crows = C rounded up to 128
    L.dzt = take(c.precision == UMLH_PREC_BF16 ? (round_up(c.num_classes, 128) * (long long)L.ldz + 1) / 2
                                               : (long long)c.num_classes * L.ldz);
    L.h = take(c.has_proj ? (long long)L.rcap_img * c.d_shared : 0);
    L.dht = take(c.has_proj ? (long long)c.d_shared * L.rcap_img : 0);
    L.slabs_head = take((long long)L.scap_head * L.n_head);
    L.slabs_proj = take((long long)L.scap_proj * L.n_proj);
    L.partials = take((long long)L.max_blocks * 4);
    L.diag_part = take(diag_part_floats(L) + DIAG_TICKET_FLOATS);
    L.grads = take(msg_cap_floats(L));
    L.w16 = take(c.precision == UMLH_PREC_BF16 ? 1024LL * c.d_shared / 2 : 0);   // bf16 chunk-major shadow of w_head (<= 1024 class rows)
    L.n_iota = L.rcap_img > L.rcap_txt ? L.rcap_img : L.rcap_txt;     // identity row ids: batch rows, classes, image-feature columns
    if (L.n_iota < 1024) L.n_iota = 1024;
    if (L.n_iota < c.d_img) L.n_iota = c.d_img;
    L.iota = take(c.precision == UMLH_PREC_BF16 ? 2LL * L.n_iota : 0);   // int64 0..n_iota-1
    L.zeros = take(64);
    L.dbg = take(dbg_floats(L));
    const bool bfp = c.precision == UMLH_PREC_BF16 && c.has_proj;
    L.wpt16 = take(bfp ? (L.n_proj + 1) / 2 : 0);         // bf16 W_proj^T [d_img][d_shared]
    L.wht16 = take(bfp ? 1024LL * round_up(c.d_shared, 128) / 2 : 0);   // bf16 W_head^T by class chunks [16][d_shared^128][64]
    // 2-D forward (128-row tiles x groups of 256 classes, cross-workgroup softmax merge; K resident in LDS): measured
    // slower than the 1-D kernel at cfg2 (umlh_kernels_bf16.hip) -> opt-in, UMLH_BF16_FWD2D=1, whenever the shape allows.
    L.fwd_nq = 0; L.xch = 0;
    if (c.precision == UMLH_PREC_BF16 && c.num_classes > 256 && c.d_shared % 256 == 0 && c.d_shared <= 512) {
        if (env_int("UMLH_BF16_FWD2D", 0) == 1) {
            L.fwd_nq = (c.num_classes + 255) / 256;
            L.xch = take(xch_floats(L));
        }
    }
    // fp32 mode: fragment-major fp32 shadow of w_head for the streamed forward (fwd_ce_f32 MODE 2): [K/16][cpad/32][64][8] floats
    L.w32s = 0;
    if (c.precision == UMLH_PREC_FP32 && c.d_shared % 32 == 0) {
        int ctw = 0, wc = 0;
        if (umlh_f32_fwd_config(c.num_classes, &ctw, &wc) > 0) L.w32s = take((long long)c.d_shared * 32 * ctw * wc * 3 / 2);   // (x3: three bf16 planes = 1.5x the fp32 shadow)
    }
    // one-launch step (step_bf16): the control words of every task it may have
    L.ctl_tasks = L.max_blocks + 4096 + L.n_head / 2048 + 8;
    L.fuse_flags = c.precision == UMLH_PREC_BF16 && !c.has_proj ? take(step_ctl_floats(L.ctl_tasks)) : 0;
    // micro-step path: linear head whose width has a supported chunking (bf16 operand mode: widths that are multiples of 128)
    L.mc_flags = L.mc_xchg = L.mc_tab = L.mc_desc = 0;
    L.mc_nwg = (c.num_classes + UMLH_MICRO_CS - 1) / UMLH_MICRO_CS;
    L.mc_nch = L.mc_cw = 0;
    if (!c.has_proj && umlh_micro_chunking(c.d_shared, &L.mc_nch, &L.mc_cw) &&
        (c.precision == UMLH_PREC_FP32 || umlh_micro_bf16_supported(L.mc_nch, L.mc_cw))) {
        L.mc_flags = take(sizeof(UmlhMicroFlags) / sizeof(float));
        L.mc_xchg = take(umlh_micro_xchg_floats(L.mc_nwg));                      // (directly behind the flags: bind zeroes both at once)
        L.mc_tab = take(sizeof(UmlhMicroTable) / sizeof(float));
        L.mc_desc = take((long long)UMLH_MICRO_MAX_HEADS * sizeof(UmlhMicroHead) / sizeof(float) + 16);
    }
    L.total = off;
    return true;
}

struct umlh_handle_s {
    umlh_config_t cfg;
    umlh_buffers_t buf;
    Layout L;
    bool bound;
    int ctw, wc, ts;            // fwd_ce tile configuration
    int stw;                    // bf16: 32-sample tiles per wave
    unsigned fwd_epoch;         // bf16 2-D forward: launch tag of the exchange granules
    unsigned fuse_epoch;        // single-launch forward + dW: launch tag of the forward blocks' granules
    int fuse;                   // forward and dW of a linear bf16 head as one launch (default; UMLH_BF16_FUSE=0: two launches)
    int dbg_step;               // UMLH_DBG_STEP=1: step_bf16 writes a per-task timeline into the debug buffer
    int step_lazy;              // UMLH_STEP_LAZY=1 (tests): see StepShape::lazy
    int step_grid;              // persistent workgroups of the one-launch step (CUs of the device; UMLH_STEP_GRID overrides)
    long long step_launches;    // one-launch steps taken (tests assert the path that ran)
    // state carried from umlh_grad_step to umlh_apply_update
    int last_rows_img, last_rows_txt;
    bool iota_ready;            // bf16: identity row-id table in the workspace initialised
    bool shadow_fresh;          // bf16: the W shadow was written by the previous step's update kernel
    bool diagnostics;           // umlh_enable_diagnostics
    int  diag_cols = 0;         // umlh_set_diagnostic_columns (0 = every column of w_head)
    int dbg_fwd, dbg_dw;        // timing-only ablation / cycle-stamp switches (UMLH_DBG_FWD / UMLH_DBG_DW), read once at create
    hipEvent_t ev[UMLH_N_PHASES + 1];   // phase boundaries, valid when profiling
    bool profiling;
    // micro-step path
    unsigned micro_epoch;       // last epoch published by this handle's workgroups (flags are zeroed at bind)
    unsigned char* stage;       // pinned host staging [2][stage_bytes] for the per-launch tables / descriptors (lazy)
    size_t stage_bytes;
    hipEvent_t stage_ev[2];     // copy-out of staging buffer i has completed
    int stage_next;
    int micro_off;              // UMLH_MICRO=0: never take the micro path
    long long micro_launches;   // persistent launches this handle took part in (tests assert the path that ran)
    // data-parallel stepping
    int frozen_proj_row;        // umlh_freeze_proj_row: row of w_proj the optimizer leaves alone (-1 = none)
    bool dp_diag;               // layout of the gradient message: [g_img | g_txt | g_proj | g_scales | scalars] instead of [g_head | ...]
    int n_ranks;                // > 1 (or dp_force): umlh_train_steps runs grad -> all-reduce -> update per step
    int dp_force;               // UMLH_FORCE_DP=1 / umlh_set_allreduce with one rank: take the split path also alone (pricing, tests)
    umlh_allreduce_fn ar_fn;    // custom transport (tests: gloo through a host callback), else RCCL through `comm`
    void* ar_ctx;
    void* p2p_region[8];        // umlh_p2p_attach: every rank's exchange region as mapped here (p2p_region[rank] = this rank's own)
    int p2p_on, p2p_rank;       // direct peer-to-peer all-reduce instead of RCCL / the callback
    unsigned p2p_epoch;
    void* comm;                 // ncclComm_t
    bool comm_owned;
    hipStream_t comm_stream;    // second stream: the head-gradient all-reduce of a 2-layer head runs beside the img_proj backward GEMMs
    hipEvent_t ev_head_ready, ev_head_done;
    int device;                 // HIP device the handle was created on: every launching entry point runs there
    int global_rows_img, global_rows_txt;   // global row counts of the last umlh_grad_step (gate the update on every rank alike)
};

// Every entry point that launches kernels for a handle makes the handle's device current for its duration
// (a process may drive several GPUs; the caller's current device is restored on return).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int want) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != want && hipSetDevice(want) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

static void dp_release(umlh_handle_t h);
static int grad_step_impl(umlh_handle_t h, const umlh_batch_t* img, const umlh_batch_t* txt, const umlh_hyper_t* hy, hipStream_t st,
                          bool comm);
static int apply_update_impl(umlh_handle_t h, const umlh_hyper_t* hy, float* scalars_out, hipStream_t st);

static inline void mark(umlh_handle_t h, int i, hipStream_t st) {
    if (h->profiling) (void)hipEventRecord(h->ev[i], st);
}

const char* umlh_last_error(void) { return g_err; }
int umlh_version(void) { return 11; }   // 3: round 2 (grouped / micro / data-parallel / encoder-plan / InfoNCE entry points, umlh_enc_layer_t.seed_device, umlh_seq_mse_backward scratch); 4: round 3 (umlh_step_status / _launches, umlh_p2p_*); 5: umlh_align_*; 6: umlh_masked_mean, umlh_probe_*; 7: umlh_align_cka_unbiased / _cka_rbf / _cknna / _list_stats; 8: umlh_spectral_scratch_bytes, umlh_svdvals, umlh_effective_rank, umlh_effective_rank_seq; 9: umlh_subspace_scratch_bytes, umlh_principal_subspace, umlh_svcca; 10: umlh_seq_compact, umlh_paired_cosine_scratch_bytes, umlh_paired_cosine; 11: umlh_seq_step_stats_scratch_bytes, umlh_seq_step_stats

int umlh_freeze_proj_row(umlh_handle_t h, int32_t row) {
    if (!h) return fail(UMLH_E_INVALID, "umlh_freeze_proj_row: null handle");
    if (row >= 0 && (!h->cfg.has_proj || row >= h->cfg.d_shared || h->cfg.d_img % 4 != 0))
        return fail(UMLH_E_INVALID, "umlh_freeze_proj_row: row %d of a [%d, %d] img_proj (needs img_proj and d_img %% 4 == 0)", row, h->cfg.d_shared, h->cfg.d_img);
    h->frozen_proj_row = row < 0 ? -1 : row;
    return UMLH_OK;
}

int umlh_set_diagnostic_columns(umlh_handle_t h, int32_t cols) {
    if (!h) return fail(UMLH_E_INVALID, "umlh_set_diagnostic_columns: null handle");
    if (cols < 0 || cols > h->cfg.d_shared) return fail(UMLH_E_INVALID, "umlh_set_diagnostic_columns: cols must be in [0, d_shared]");
    h->diag_cols = cols == h->cfg.d_shared ? 0 : cols;
    return UMLH_OK;
}

int umlh_enable_diagnostics(umlh_handle_t h, int32_t on) {
    if (!h) return fail(UMLH_E_INVALID, "umlh_enable_diagnostics: null handle");
    h->diagnostics = on != 0;
    return UMLH_OK;
}

uint64_t umlh_workspace_bytes(const umlh_config_t* cfg) {
    Layout L;
    if (!cfg || !make_layout(*cfg, L)) return 0;
    return (uint64_t)L.total * sizeof(float);
}

int umlh_create(const umlh_config_t* cfg, umlh_handle_t* out) {
    if (!cfg || !out) return fail(UMLH_E_INVALID, "umlh_create: null argument");
    Layout L;
    if (!make_layout(*cfg, L))
        return fail(UMLH_E_INVALID,
                    "umlh_create: unsupported config (d_img=%d d_shared=%d C=%d has_proj=%d opt=%d prec=%d rows=%d/%d)",
                    cfg->d_img, cfg->d_shared, cfg->num_classes, cfg->has_proj, cfg->optimizer, cfg->precision,
                    cfg->max_rows_img, cfg->max_rows_txt);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(UMLH_E_NOGPU, "umlh_create: no HIP device visible");
    umlh_handle_s* h = new (std::nothrow) umlh_handle_s();
    if (!h) return fail(UMLH_E_INVALID, "umlh_create: out of host memory");
    h->cfg = *cfg;
    h->L = L;
    h->bound = false;
    h->ts = umlh_f32_fwd_config(cfg->num_classes, &h->ctw, &h->wc);
    h->stw = 1;
    h->dbg_fwd = env_int("UMLH_DBG_FWD", 0);
    h->dbg_dw = env_int("UMLH_DBG_DW", 0);
    if (cfg->precision == UMLH_PREC_BF16) {
        // two 32-sample tiles per wave would halve the L2->CU stream of the head weight, but measured
        // slower on MI355X (51 vs 26 us at cfg2: half the CUs idle, VGPR-limited ring) -> opt-in only
        if (h->wc == 8 && h->ctw >= 2 && env_int("UMLH_BF16_STW", 1) == 2) h->stw = 2;
        h->ts = umlh_bf16_fwd_ts(h->wc, h->stw);
        if (L.fwd_nq) h->ts = 128;
    }
    h->fwd_epoch = 0;
    h->fuse_epoch = 0;
    h->dbg_step = env_int("UMLH_DBG_STEP", 0) == 1;
    h->step_grid = 0; h->step_launches = 0;
    h->step_lazy = env_int("UMLH_STEP_LAZY", 0) == 1;
    h->fuse = env_int("UMLH_BF16_FUSE", 2);   // 2 (default): the whole step as one launch; 1: forward + dW as one; 0: separate launches
    h->last_rows_img = h->last_rows_txt = 0;
    h->global_rows_img = h->global_rows_txt = 0;
    h->profiling = false;
    h->micro_epoch = 0;
    h->micro_launches = 0;
    h->frozen_proj_row = -1;
    h->dp_diag = false; h->n_ranks = 1; h->ar_fn = nullptr; h->ar_ctx = nullptr; h->comm = nullptr; h->comm_owned = false;
    h->comm_stream = nullptr;
    h->p2p_on = 0; h->p2p_rank = 0; h->p2p_epoch = 0; memset(h->p2p_region, 0, sizeof(h->p2p_region));
    h->dp_force = env_int("UMLH_FORCE_DP", 0) == 1;
    h->stage = nullptr; h->stage_bytes = 0; h->stage_next = 0;
    h->micro_off = env_int("UMLH_MICRO", 1) == 0;
    h->device = 0;
    (void)hipGetDevice(&h->device);
    const int grid_env = env_int("UMLH_STEP_GRID", 0);
    h->step_grid = grid_env > 0 ? grid_env : device_cus(h->device);   // fewer workgroups than tasks is always correct (tests: partial residency)
    memset(&h->buf, 0, sizeof(h->buf));
    *out = h;
    return UMLH_OK;
}

int umlh_profile_enable(umlh_handle_t h, int enable) {
    if (!h) return fail(UMLH_E_INVALID, "umlh_profile_enable: null handle");
    DeviceGuard dg_(h->device);
    if (enable && !h->profiling) {
        for (int i = 0; i <= UMLH_N_PHASES; ++i)
            if (hipEventCreate(&h->ev[i]) != hipSuccess) return fail(UMLH_E_HIP, "umlh_profile_enable: hipEventCreate failed");
        h->profiling = true;
    } else if (!enable && h->profiling) {
        for (int i = 0; i <= UMLH_N_PHASES; ++i) (void)hipEventDestroy(h->ev[i]);
        h->profiling = false;
    }
    return UMLH_OK;
}

int umlh_profile_read(umlh_handle_t h, float* ms_out) {
    if (!h || !ms_out) return fail(UMLH_E_INVALID, "umlh_profile_read: null argument");
    if (!h->profiling) return fail(UMLH_E_INVALID, "umlh_profile_read: profiling not enabled");
    DeviceGuard dg_(h->device);
    if (hipEventSynchronize(h->ev[UMLH_N_PHASES]) != hipSuccess) return fail(UMLH_E_HIP, "umlh_profile_read: sync failed");
    for (int i = 0; i < UMLH_N_PHASES; ++i)
        if (hipEventElapsedTime(&ms_out[i], h->ev[i], h->ev[i + 1]) != hipSuccess)
            return fail(UMLH_E_HIP, "umlh_profile_read: elapsed failed (run a step first)");
    return UMLH_OK;
}

int umlh_destroy(umlh_handle_t h) {
    if (h && h->profiling) umlh_profile_enable(h, 0);
    if (h) {
        DeviceGuard dg_(h->device);
        dp_release(h);
        if (h->comm_stream) {
            (void)hipStreamSynchronize(h->comm_stream);
            (void)hipEventDestroy(h->ev_head_ready); (void)hipEventDestroy(h->ev_head_done);
            (void)hipStreamDestroy(h->comm_stream);
        }
    }
    if (h && h->stage) {
        DeviceGuard dg_(h->device);
        (void)hipEventSynchronize(h->stage_ev[0]); (void)hipEventSynchronize(h->stage_ev[1]);
        (void)hipEventDestroy(h->stage_ev[0]); (void)hipEventDestroy(h->stage_ev[1]);
        (void)hipHostFree(h->stage);
    }
    delete h;
    return UMLH_OK;
}

static inline float* ws(umlh_handle_t h, long long off) { return static_cast<float*>(h->buf.workspace) + off; }
static inline int class_pad(const umlh_handle_s* h) { return 32 * h->ctw * h->wc; }   // class rows of the W shadows (whole 32-class tiles per wave)
// ticket of the gradient-diagnostics reduction, behind the [head_step blocks][4] partials (head_step_kernel leaves it at 0)
static inline unsigned* diag_ticket(umlh_handle_t h) {
    return reinterpret_cast<unsigned*>(ws(h, h->L.diag_part) + diag_part_floats(h->L));
}

// gradient message layout (see umlh_grad_step): head part, img_proj part, then g_scales(2) + scalars
static inline long long frozen_lo(const umlh_handle_s* h) { return h->frozen_proj_row < 0 ? 0 : (long long)h->frozen_proj_row * h->cfg.d_img; }
static inline long long frozen_hi(const umlh_handle_s* h) { return h->frozen_proj_row < 0 ? 0 : (long long)(h->frozen_proj_row + 1) * h->cfg.d_img; }
static inline long long msg_head_len(const umlh_handle_s* h) { return msg_head_floats(h->L, h->dp_diag); }
static inline long long msg_tail_off(const umlh_handle_s* h) { return msg_head_len(h) + h->L.n_proj; }
static inline long long msg_len(const umlh_handle_s* h) { return msg_floats(h->L, h->dp_diag); }
// the message form umlh_grad_step uses: per-modality head gradients when the diagnostics are on and head_step_kernel can form them
static inline bool split_diag(const umlh_handle_s* h) { return h->diagnostics && h->cfg.d_shared % 8 == 0; }
// the control words of the one-launch step / the micro path's status word
static inline StepCtl step_ctl(umlh_handle_t h) { return step_ctl_at(ws(h, h->L.fuse_flags), h->L.ctl_tasks); }
static inline unsigned* micro_status(umlh_handle_t h) { return &reinterpret_cast<UmlhMicroFlags*>(ws(h, h->L.mc_flags))->status; }

int umlh_bind(umlh_handle_t h, const umlh_buffers_t* b) {
    if (!h || !b) return fail(UMLH_E_INVALID, "umlh_bind: null argument");
    if (!b->w_head || !b->m_head || !b->workspace) return fail(UMLH_E_INVALID, "umlh_bind: w_head/m_head/workspace required");
    if (h->cfg.optimizer != UMLH_OPT_SGD && !b->v_head) return fail(UMLH_E_INVALID, "umlh_bind: v_head required for adam/adamw");
    if (h->cfg.has_proj && (!b->w_proj || !b->m_proj || (h->cfg.optimizer != UMLH_OPT_SGD && !b->v_proj)))
        return fail(UMLH_E_INVALID, "umlh_bind: img_proj buffers required when has_proj");
    if (!b->scales) return fail(UMLH_E_INVALID, "umlh_bind: scales[2] required");
    if (h->cfg.learnable_temp && (!b->m_scales || !b->v_scales))
        return fail(UMLH_E_INVALID, "umlh_bind: m_scales/v_scales required when learnable_temp");
    if (b->workspace_bytes < (uint64_t)h->L.total * sizeof(float))
        return fail(UMLH_E_UNBOUND, "umlh_bind: workspace too small (%llu < %llu bytes)",
                    (unsigned long long)b->workspace_bytes, (unsigned long long)h->L.total * sizeof(float));
    if ((reinterpret_cast<uintptr_t>(b->workspace) & 255) != 0) return fail(UMLH_E_INVALID, "umlh_bind: workspace must be 256-B aligned");
    h->buf = *b;
    h->bound = true;
    h->iota_ready = false;
    h->shadow_fresh = false;
    {
        DeviceGuard dg_(h->device);
        if (hipMemset(diag_ticket(h), 0, DIAG_TICKET_FLOATS * sizeof(float)) != hipSuccess) return fail(UMLH_E_HIP, "umlh_bind: clearing the diagnostics ticket failed");
    }
    if (h->L.fuse_flags) {        // done granules / claim words / status of the one-launch step: tag 0 = never written
        DeviceGuard dg_(h->device);
        if (hipMemset(ws(h, h->L.fuse_flags), 0, sizeof(float) * (size_t)step_ctl_floats(h->L.ctl_tasks)) != hipSuccess)
            return fail(UMLH_E_HIP, "umlh_bind: clearing the step control words failed");
        h->fuse_epoch = 0;
    }
    if (h->L.fwd_nq) {            // exchange granules of the 2-D forward: tag 0 = never written
        DeviceGuard dg_(h->device);
        if (hipMemset(ws(h, h->L.xch), 0, sizeof(float) * (size_t)xch_floats(h->L)) != hipSuccess)
            return fail(UMLH_E_HIP, "umlh_bind: clearing the forward exchange region failed");
        h->fwd_epoch = 0;
    }
    if (h->L.mc_flags) {          // epoch flags, status word and exchange records start from zero (bind time only)
        DeviceGuard dg_(h->device);
        const size_t n = sizeof(UmlhMicroFlags) + (size_t)umlh_micro_xchg_floats(h->L.mc_nwg) * sizeof(float);
        if (hipMemset(ws(h, h->L.mc_flags), 0, n) != hipSuccess) return fail(UMLH_E_HIP, "umlh_bind: clearing the micro-step region failed");
        h->micro_epoch = 0;
    }
    return UMLH_OK;
}

// forward blocks of the image segment: in bf16 mode the image columns of dZ^T are padded to whole
// 64-column chunks (every dW chunk then lies in one modality); the padding tile(s) run with all rows
// masked and write zeros
static inline int fwd_blocks_img(const umlh_handle_s* h, int rows) {
    int nb = (rows + h->ts - 1) / h->ts;
    if (h->cfg.precision == UMLH_PREC_BF16 && h->ts < 64 && nb > 0) {
        int per = 64 / h->ts;
        nb = (nb + per - 1) / per * per;
    }
    return nb;
}

static int check_batch(umlh_handle_t h, const umlh_batch_t* b, int cap, const char* who) {
    if (!b) return UMLH_OK;
    if (b->rows < 0 || b->rows > cap) return fail(UMLH_E_INVALID, "%s: rows=%d outside [0,%d]", who, b->rows, cap);
    if (b->rows > 0 && (!b->feats || !b->labels)) return fail(UMLH_E_INVALID, "%s: feats/labels null", who);
    if (b->rows > 0 && b->global_rows < b->rows) return fail(UMLH_E_INVALID, "%s: global_rows=%d < rows=%d", who, b->global_rows, b->rows);
    return UMLH_OK;
}

OptArgs make_opt(const umlh_config_t& c, const umlh_hyper_t& hy) {
    OptArgs o;
    memset(&o, 0, sizeof(o));
    o.plain = umlh_plain_stores();
    o.kind = c.optimizer;
    o.lr = (float)hy.lr;
    o.decay = (float)(1.0 - hy.lr * c.weight_decay);
    double t = (double)(hy.step < 1 ? 1 : hy.step);
    double bc1 = 1.0 - std::pow(c.beta1, t);
    double bc2 = 1.0 - std::pow(c.beta2, t);
    o.neg_step_size = (float)(-(hy.lr / bc1));
    o.bc2_sqrt = (float)std::sqrt(bc2);
    o.beta1 = (float)c.beta1;
    o.one_m_beta1 = (float)(1.0 - c.beta1);
    o.beta2 = (float)c.beta2;
    o.one_m_beta2 = (float)(1.0 - c.beta2);
    o.eps = (float)c.eps;
    o.momentum = (float)c.momentum;
    o.wd = (float)c.weight_decay;
    return o;
}

int umlh_zero_shot_init(umlh_handle_t h, const float* text_feats, const int64_t* text_labels, int64_t n_text,
                        void* stream) {
    if (!h || !h->bound) return fail(UMLH_E_UNBOUND, "umlh_zero_shot_init: handle not bound");
    if (!text_feats || !text_labels || n_text < 0) return fail(UMLH_E_INVALID, "umlh_zero_shot_init: bad arguments");
    DeviceGuard dg_(h->device);
    HIPCHK(umlh_launch_zero_shot(text_feats, text_labels, n_text, h->cfg.d_shared, h->cfg.num_classes,
                                 h->buf.w_head, (hipStream_t)stream), "zero_shot");
    return UMLH_OK;
}

// H = X_img[index] W_proj^T into the workspace (head.py:79)
static int launch_proj_forward(umlh_handle_t h, const umlh_batch_t* img, float* H, hipStream_t st) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = img->feats; g.a_rows = img->index; g.lda = h->cfg.d_img;
    g.B = h->buf.w_proj; g.ldb = h->cfg.d_img;
    g.out = H; g.ldo = h->cfg.d_shared;
    g.M = img->rows; g.N = h->cfg.d_shared; g.K = h->cfg.d_img;
    g.k_chunk = g.K; g.slab_stride = 0; g.alpha = 1.f;
    g.k_switch = INT_MAX; g.k_valid1 = g.K; g.k_valid2 = 0;
    return umlh_f32_launch_gemm(&g, 0, 0, 1, st);
}

int umlh_logits(umlh_handle_t h, const umlh_batch_t* b, int modality, float* out, void* stream) {
    if (!h || !h->bound) return fail(UMLH_E_UNBOUND, "umlh_logits: handle not bound");
    if (!b || !out || (modality != 0 && modality != 1)) return fail(UMLH_E_INVALID, "umlh_logits: bad arguments");
    DeviceGuard dg_(h->device);
    int rc = check_batch(h, b, modality == 0 ? h->L.rcap_img : h->L.rcap_txt, "umlh_logits");
    if (rc) return rc;
    if (b->rows == 0) return UMLH_OK;
    hipStream_t st = (hipStream_t)stream;
    const float* F = b->feats;
    const int64_t* idx = b->index;
    int ld = h->cfg.d_shared;
    if (modality == 0 && h->cfg.has_proj) {
        HIPCHK(launch_proj_forward(h, b, ws(h, h->L.h), st), "proj forward");
        F = ws(h, h->L.h);
        idx = nullptr;
    }
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = F; g.a_rows = idx; g.lda = ld;
    g.B = h->buf.w_head; g.ldb = h->cfg.d_shared;
    g.out = out; g.ldo = h->cfg.num_classes;
    g.M = b->rows; g.N = h->cfg.num_classes; g.K = h->cfg.d_shared;
    g.k_chunk = g.K; g.alpha = 1.f;
    g.k_switch = INT_MAX; g.k_valid1 = g.K;
    g.alpha_ptr = h->buf.scales + modality;             // device-resident logit scale
    HIPCHK(umlh_f32_launch_gemm(&g, 0, 0, 1, st), "logits gemm");
    return UMLH_OK;
}

int umlh_project(umlh_handle_t h, const umlh_batch_t* b, float* out, void* stream) {
    if (!h || !h->bound) return fail(UMLH_E_UNBOUND, "umlh_project: handle not bound");
    if (!b || !out) return fail(UMLH_E_INVALID, "umlh_project: null argument");
    if (!h->cfg.has_proj) return fail(UMLH_E_INVALID, "umlh_project: head has no img_proj");
    DeviceGuard dg_(h->device);
    int rc = check_batch(h, b, h->L.rcap_img, "umlh_project");
    if (rc) return rc;
    if (b->rows == 0) return UMLH_OK;
    HIPCHK(launch_proj_forward(h, b, out, (hipStream_t)stream), "proj forward");
    return UMLH_OK;
}

// One forward/backward: what it takes besides the handle and what it leaves behind, passed by reference through its stages.
// Filled by train_step_impl, grad_step_impl and the eval entry points; nothing of it outlives the call.
struct StepCall {
    // in
    const umlh_batch_t* img; const umlh_batch_t* txt; const umlh_hyper_t* hy;
    bool want_grad;                     // false: forward only (evaluation)
    hipStream_t st;
    const HeadFuse* head = nullptr;     // linear bf16 head: the update (or the slab sum into the gradient message) may ride in the one-launch step
    bool overlap = false;               // data-parallel 2-layer head: the head all-reduce starts behind dW_head (dp_after_head)
    float* row_stats = nullptr;         // per-row {CE, correct} output of the forward (umlh_eval_rows)
    // derived by forward_backward: rows, forward blocks and padded dZ^T columns of the image / text segment
    int ri, rt, nb0, nb1, r0p, r1p;
    // out
    int n_slabs_head = 0, n_slabs_proj = 0;   // split-K slabs the dW_head / dW_proj GEMMs wrote
    int n_slabs_img = 0;                // dW_head slabs that hold image rows (the rest hold text rows)
    bool head_done = false;             // `head` rode in the launch: nothing is left to reduce or update
};

static int dp_after_head(umlh_handle_t h, const StepCall& x);

static inline u16* ws16(umlh_handle_t h, long long off) { return reinterpret_cast<u16*>(ws(h, off)); }
static inline int64_t* ws_iota(umlh_handle_t h) { return reinterpret_cast<int64_t*>(ws(h, h->L.iota)); }
static inline unsigned long long* ws_stamps(umlh_handle_t h) { return reinterpret_cast<unsigned long long*>(ws(h, h->L.dbg)); }

// The two modalities' rows as the forward kernels see them (SegDesc / SegDescB).  `gathered`: the image features were
// already gathered by the projection (H, row r = batch row r); an absent modality keeps its zeroed descriptor.
template <class Seg, class T>
static void fill_segs(Seg* seg, umlh_handle_t h, const StepCall& x, const T* feats_img, bool gathered, const T* feats_txt) {
    if (x.ri > 0) {
        seg[0].feats = feats_img; seg[0].feat_index = gathered ? nullptr : x.img->index;
        seg[0].labels = x.img->labels; seg[0].label_index = x.img->index; seg[0].ld = h->cfg.d_shared; seg[0].rows = x.ri;
        seg[0].w_over_rows = x.hy->img_alpha / (float)x.img->global_rows;
    }
    seg[0].scale_ptr = h->buf.scales; seg[0].col0 = 0; seg[0].blk0 = 0;
    if (x.rt > 0) {
        seg[1].feats = feats_txt; seg[1].feat_index = x.txt->index;
        seg[1].labels = x.txt->labels; seg[1].label_index = x.txt->index; seg[1].ld = h->cfg.d_shared; seg[1].rows = x.rt;
        seg[1].w_over_rows = x.hy->alpha / (float)x.txt->global_rows;
    }
    seg[1].scale_ptr = h->buf.scales + 1; seg[1].col0 = x.r0p; seg[1].blk0 = x.nb0;
}

// ---- bf16 mode ----
// The GEMM loaders are branch-free: every pointer must be dereferenceable, also for an absent modality or a dense
// (index-less) batch -> identity row ids + a zero page from the workspace
static DwArgsB dw_base_args(umlh_handle_t h) {
    DwArgsB g;
    memset(&g, 0, sizeof(g));
    g.zeros = ws16(h, h->L.zeros); g.bcs = 64; g.a_rows = ws_iota(h); g.nsplit = g.nsplit1 = 1;
    g.dbg = h->dbg_dw;
    if (g.dbg >= 16) { g.dbg -= 16; g.stamps = ws_stamps(h); }   // +16: cycle stamps
    return g;
}

// H = X_img W_proj^T  (head.py:79): rows gathered by the batch index, bf16 row-major [r][d_shared] out.  W_proj^T is a
// per-step bf16 shadow of the fp32 master (6.5 MB at cfg3, against ~180 GFLOP of GEMMs per step).
static int bf16_proj_forward(umlh_handle_t h, const StepCall& x) {
    const umlh_config_t& c = h->cfg;
    u16* wpt16 = ws16(h, h->L.wpt16);
    HIPCHK(umlh_bf16_launch_transpose_shadow(h->buf.w_proj, c.d_shared, c.d_img, c.d_shared, wpt16, 0, x.st), "W_proj^T shadow");
    DwArgsB g = dw_base_args(h);
    g.A = static_cast<const u16*>(x.img->feats_bf16); g.lda = c.d_img; g.a_rows = x.img->index ? x.img->index : ws_iota(h);
    g.B = g.B2 = wpt16; g.k_rows = g.k_rows2 = ws_iota(h); g.ldb = g.ldb2 = c.d_shared;
    g.M = x.ri; g.N = c.d_shared; g.K = c.d_img;
    g.k_chunk = (int)round_up(c.d_img, 256); g.k_switch = c.d_img; g.k_valid1 = c.d_img; g.k_valid2 = 0;
    g.out16 = ws16(h, h->L.h); g.ldo = c.d_shared;
    if (g.k_chunk > 4096) return fail(UMLH_E_INVALID, "bf16 img_proj: d_img %d > 4096 unsupported", c.d_img);
    HIPCHK(umlh_bf16_launch_dw(&g, 1, 1, 1, x.st), "proj forward (bf16)");
    return UMLH_OK;
}

// Fills `fb` and launches the forward unless it is to ride in the one-launch step (`fused`, then bf16_dw_head launches it).
static int bf16_forward_ce(umlh_handle_t h, const StepCall& x, bool proj, FwdArgsB& fb, bool& fused) {
    const umlh_config_t& c = h->cfg;
    const Layout& L = h->L;
    const int nb = x.nb0 + x.nb1, crows = (int)round_up(c.num_classes, 128);
    memset(&fb, 0, sizeof(fb));
    fill_segs(fb.seg, h, x, x.ri > 0 ? (proj ? ws16(h, L.h) : static_cast<const u16*>(x.img->feats_bf16)) : nullptr, proj,
              x.rt > 0 ? static_cast<const u16*>(x.txt->feats_bf16) : nullptr);
    fb.W = ws16(h, L.w16); fb.C = c.num_classes; fb.K = c.d_shared;
    fb.dzt = x.want_grad ? ws16(h, L.dzt) : nullptr; fb.crows = crows;
    fb.partials = ws(h, L.partials);
    fb.dbg = h->dbg_fwd;
    fb.learn = c.learnable_temp;
    fb.row_stats = x.row_stats;
    fb.stamps = (fb.dbg == 9 || fb.dbg >= 20) ? ws_stamps(h) : nullptr;
    if (L.fwd_nq) {
        fb.xch = reinterpret_cast<unsigned long long*>(ws(h, L.xch));
        if (++h->fwd_epoch == 0) h->fwd_epoch = 1;
        fb.epoch = h->fwd_epoch;
        fb.wtiles = class_pad(h) / 32;
        fb.ntiles = nb;
        HIPCHK(umlh_bf16_launch_fwd_q(&fb, L.fwd_nq, nb, x.st), "fwd_ce_bf16_q");
    }
    // forward + dW as one launch (linear head, 1-D forward, write-through stores).  In profiling mode the interval
    // mark 1 -> 2 is then empty and mark 2 -> 3 holds the one launch.
    // (not while the stream is being captured into a HIP graph: the granules' epoch tag is a launch argument, a replay
    // would find the previous replay's tags and pass its gates early)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = h->fuse && hipStreamIsCapturing(x.st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
    // (the coherent loads address dZ^T and the slabs through 32-bit buffer offsets)
    const bool fits32 = (unsigned long long)((x.r0p + x.r1p + 63) / 64) * crows * 128ull < (1ull << 31) &&
                        (unsigned long long)L.scap_head * L.n_head * 4ull < (1ull << 31);
    fused = h->fuse && !capturing && fits32 && x.want_grad && !proj && !L.fwd_nq && h->stw == 1 && L.fuse_flags &&
            !umlh_plain_stores() && fb.dbg == 0 && h->dbg_dw == 0;
    if (!L.fwd_nq && !fused) HIPCHK(umlh_bf16_launch_fwd(&fb, h->ctw, h->wc, h->stw, nb, x.st), "fwd_ce_bf16");
    return UMLH_OK;
}

// dW_head = dZ^T [H or X_img ; X_txt] as split-K slabs; `fused`: together with the forward (and x.head) as ONE launch
static int bf16_dw_head(umlh_handle_t h, StepCall& x, bool proj, const FwdArgsB& fb, bool fused) {
    const umlh_config_t& c = h->cfg;
    const Layout& L = h->L;
    const umlh_batch_t* img = x.img; const umlh_batch_t* txt = x.txt;
    const int ri = x.ri, rt = x.rt, r0p = x.r0p, r1p = x.r1p, nb = x.nb0 + x.nb1;
    // chunk: multiples of 4 x 64 columns (4-stage pipeline), at most 4096 (row ids of a split live in LDS)
    SplitPlan sp = plan_splits(r0p, r1p, L.scap_head, 256, 256);
    if (sp.chunk > 4096) { sp.chunk = 4096; sp.n_img = (r0p + 4095) / 4096; sp.n_txt = (r1p + 4095) / 4096; }
    const int splits = sp.n_img + sp.n_txt;
    if (splits > L.scap_head)
        return fail(UMLH_E_INVALID, "bf16 dW: %d + %d reduction rows need more than %d split-K slabs", r0p, r1p, L.scap_head);
    const u16* any16 = ri > 0 ? static_cast<const u16*>(img->feats_bf16) : static_cast<const u16*>(txt->feats_bf16);
    int64_t* iota = ws_iota(h);
    DwArgsB g = dw_base_args(h);
    g.A = ws16(h, L.dzt); g.lda = (int)round_up(c.num_classes, 128);
    g.B = proj ? ws16(h, L.h) : (ri > 0 ? static_cast<const u16*>(img->feats_bf16) : any16);
    g.k_rows = (ri > 0 && img->index && !proj) ? img->index : iota; g.ldb = c.d_shared;
    g.B2 = rt > 0 ? static_cast<const u16*>(txt->feats_bf16) : any16;
    g.k_rows2 = (rt > 0 && txt->index) ? txt->index : iota; g.ldb2 = c.d_shared;
    g.out = ws(h, L.slabs_head); g.ldo = c.d_shared;
    g.M = c.num_classes; g.N = c.d_shared; g.K = r0p + r1p;
    g.k_chunk = sp.chunk; g.k_switch = r0p; g.k_valid1 = ri; g.k_valid2 = rt; g.slab_stride = L.n_head;
    g.nsplit = splits; g.nsplit1 = sp.n_img; x.n_slabs_img = sp.n_img;
    const bool with_head = fused && x.head && h->fuse >= 2;
    const int ntask = umlh_bf16_step_tasks(nb, g.M, g.N, splits, L.n_head, with_head);
    if (fused && ntask <= L.ctl_tasks) {
        // forward + dW (+ update + finalize) as ONE launch of persistent workgroups over claimed tasks (StepCtl)
        const StepCtl ctl = step_ctl(h);
        if (h->fuse_epoch > 0xFFFFFF00u) {            // tag wrap (2^32 launches): start the epoch-tagged words over (the status stays)
            HIPCHK((int)hipMemsetAsync(ctl.done, 0, step_ctl_tag_bytes(ctl), x.st), "step control words");
            h->fuse_epoch = 0;
        }
        ++h->fuse_epoch;
        HeadFuse hf;
        if (with_head) { hf = *x.head; hf.n_slabs = splits; hf.n_slabs_img = sp.n_img; }
        const bool timeline = h->dbg_step && 8LL * ntask <= dbg_floats(L);      // 4 u64 stamps per task
        HIPCHK(umlh_bf16_launch_step(&fb, h->ctw, h->wc, nb, &g, splits, ctl.claim, ctl.done, ctl.status, h->fuse_epoch, h->ts, nb * h->ts,
                                     with_head ? &hf : nullptr, timeline ? ws_stamps(h) : nullptr,
                                     h->step_grid, h->step_lazy, x.st), "step_bf16");
        x.head_done = with_head;
        h->step_launches++;
    } else {
        if (fused) HIPCHK(umlh_bf16_launch_fwd(&fb, h->ctw, h->wc, h->stw, nb, x.st), "fwd_ce_bf16");
        HIPCHK(umlh_bf16_launch_dw(&g, splits, 0, 0, x.st), "dw_bf16");
    }
    x.n_slabs_head = splits;
    return UMLH_OK;
}

// dH^T = W_head^T dZ^T (image columns), then dW_proj = dH^T X_img as split-K slabs
static int bf16_proj_backward(umlh_handle_t h, StepCall& x) {
    const umlh_config_t& c = h->cfg;
    const Layout& L = h->L;
    const int crows = (int)round_up(c.num_classes, 128), dsp = (int)round_up(c.d_shared, 128), r0p = x.r0p;
    int64_t* iota = ws_iota(h);
    // dH^T[n][r] = sum_c W_head[c][n] dZ^T[c][r]  (image columns), bf16 chunk-major [r/64][d_shared^128][64] out
    u16* wht16 = ws16(h, L.wht16);
    u16* dht16 = ws16(h, L.dht);
    HIPCHK(umlh_bf16_launch_transpose_shadow(h->buf.w_head, c.num_classes, c.d_shared, dsp, wht16, 1, x.st), "W_head^T shadow");
    const int kc = (int)round_up(c.num_classes, 64);
    DwArgsB g = dw_base_args(h);
    g.A = wht16; g.lda = dsp;
    g.B = g.B2 = ws16(h, L.dzt); g.k_rows = g.k_rows2 = iota; g.ldb = g.ldb2 = 64; g.bcs = crows * 64;
    g.M = c.d_shared; g.N = r0p; g.K = kc;
    g.k_chunk = (int)round_up(kc, 256); g.k_switch = kc; g.k_valid1 = c.num_classes; g.k_valid2 = 0;
    g.out16 = dht16; g.ldo = dsp;
    HIPCHK(umlh_bf16_launch_dw(&g, 1, 0, 2, x.st), "dH^T (bf16)");
    // dW_proj[n][k] = sum_r dH^T[n][r] X_img[r][k]
    SplitPlan sp = plan_splits(r0p, 0, L.scap_proj, 256, 256);
    if (sp.chunk > 4096) { sp.chunk = 4096; sp.n_img = (r0p + 4095) / 4096; }
    if (sp.n_img > L.scap_proj)
        return fail(UMLH_E_INVALID, "bf16 dW_proj: %d reduction rows need more than %d split-K slabs", r0p, L.scap_proj);
    DwArgsB p = dw_base_args(h);
    p.A = dht16; p.lda = dsp;
    p.B = p.B2 = static_cast<const u16*>(x.img->feats_bf16); p.k_rows = p.k_rows2 = x.img->index ? x.img->index : iota;
    p.ldb = p.ldb2 = c.d_img;
    p.M = c.d_shared; p.N = c.d_img; p.K = r0p;
    p.k_chunk = sp.chunk; p.k_switch = r0p; p.k_valid1 = x.ri; p.k_valid2 = 0;
    p.out = ws(h, L.slabs_proj); p.ldo = c.d_img; p.slab_stride = L.n_proj;
    p.nsplit = p.nsplit1 = sp.n_img;
    HIPCHK(umlh_bf16_launch_dw(&p, sp.n_img, 0, 0, x.st), "dW_proj (bf16)");
    x.n_slabs_proj = sp.n_img;
    return UMLH_OK;
}

static int forward_backward_bf16(umlh_handle_t h, StepCall& x) {
    const umlh_config_t& c = h->cfg;
    hipStream_t st = x.st;
    if ((x.ri > 0 && !x.img->feats_bf16) || (x.rt > 0 && !x.txt->feats_bf16))
        return fail(UMLH_E_INVALID, "bf16 mode: batch.feats_bf16 is required (umlh_to_bf16 of the feature table)");
    const bool proj = c.has_proj && x.ri > 0;
    mark(h, 0, st);
    if (!h->iota_ready) {                      // identity row ids + zero page of dw_base_args, once per bind
        HIPCHK(umlh_launch_iota(reinterpret_cast<long long*>(ws_iota(h)), h->L.n_iota, st), "iota");
        HIPCHK((int)hipMemsetAsync(ws(h, h->L.zeros), 0, 64 * sizeof(float), st), "zero page");
        h->iota_ready = true;
    }
    if (proj) RC(bf16_proj_forward(h, x));
    // bf16 shadow of the fp32 master weight: refreshed here unless the previous step of the same umlh_train_steps call just
    // wrote it from its update kernel (between calls the caller may have rewritten w_head: load_state_dict, zero-shot init)
    if (!h->shadow_fresh)
        HIPCHK(umlh_launch_w_shadow(h->buf.w_head, ws16(h, h->L.w16), c.num_classes, c.d_shared, class_pad(h), st), "w_shadow");
    h->shadow_fresh = false;
    mark(h, 1, st);
    FwdArgsB fb;
    bool fused = false;
    RC(bf16_forward_ce(h, x, proj, fb, fused));
    mark(h, 2, st);
    if (!x.want_grad) return UMLH_OK;
    RC(bf16_dw_head(h, x, proj, fb, fused));
    mark(h, 3, st);
    if (x.overlap) RC(dp_after_head(h, x));
    if (proj) RC(bf16_proj_backward(h, x));
    mark(h, 4, st);
    return UMLH_OK;
}

// ---- fp32 mode ----
static int f32_forward_ce(umlh_handle_t h, const StepCall& x) {
    const umlh_config_t& c = h->cfg;
    const Layout& L = h->L;
    FwdArgs fa;
    memset(&fa, 0, sizeof(fa));
    fill_segs(fa.seg, h, x, x.ri > 0 ? (c.has_proj ? ws(h, L.h) : x.img->feats) : nullptr, c.has_proj != 0,
              x.rt > 0 ? x.txt->feats : nullptr);
    fa.W = h->buf.w_head; fa.C = c.num_classes; fa.K = c.d_shared;
    fa.dzt = x.want_grad ? ws(h, L.dzt) : nullptr; fa.ldz = L.ldz;
    fa.partials = ws(h, L.partials);
    fa.row_stats = x.row_stats;
    fa.stamps = (h->dbg_fwd == 9 || h->dbg_fwd >= 20) ? ws_stamps(h) : nullptr;
    fa.dbg = h->dbg_fwd;
    fa.learn = c.learnable_temp;
    if (L.w32s) {
        // refreshed here unless the previous step of the same umlh_train_steps call (or the data-parallel update) just wrote
        // it from its update kernel (between calls the caller may have rewritten w_head)
        if (!h->shadow_fresh)
            HIPCHK(umlh_launch_w_shadow32(h->buf.w_head, ws(h, L.w32s), c.num_classes, c.d_shared, class_pad(h), x.st), "w_shadow32");
        h->shadow_fresh = false;
        fa.Ws = ws(h, L.w32s);
        fa.x3 = umlh_f32_x3();
    }
    HIPCHK(umlh_f32_launch_fwd(&fa, h->ctw, h->wc, x.nb0 + x.nb1, x.st), "fwd_ce");
    return UMLH_OK;
}

// dW_head[c][k] = sum_r dZ^T[c][r] F[r][k]  over image rows then text rows
static int f32_dw_head(umlh_handle_t h, StepCall& x) {
    const umlh_config_t& c = h->cfg;
    const Layout& L = h->L;
    const SplitPlan sp = plan_splits(x.r0p, x.r1p, L.scap_head, KT, 64);
    const int splits = sp.n_img + sp.n_txt;
    if (splits > L.scap_head)
        return fail(UMLH_E_INVALID, "dW: %d + %d reduction rows need more than %d split-K slabs", x.r0p, x.r1p, L.scap_head);
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = ws(h, L.dzt); g.lda = L.ldz;
    g.M = c.num_classes; g.N = c.d_shared; g.K = x.r0p + x.r1p;
    g.B = c.has_proj ? ws(h, L.h) : (x.img ? x.img->feats : nullptr);
    g.k_rows = c.has_proj ? nullptr : (x.img ? x.img->index : nullptr);
    g.ldb = c.d_shared;
    g.B2 = x.txt ? x.txt->feats : nullptr; g.k_rows2 = x.txt ? x.txt->index : nullptr; g.ldb2 = c.d_shared;
    g.k_switch = x.r0p; g.k_valid1 = x.ri; g.k_valid2 = x.rt;
    g.out = ws(h, L.slabs_head); g.ldo = c.d_shared;
    g.k_chunk = sp.chunk; g.slab_stride = L.n_head; g.alpha = 1.f; g.nsplit1 = sp.n_img; x.n_slabs_img = sp.n_img;
    HIPCHK(umlh_f32_launch_gemm(&g, 0, 1, splits, x.st), "dW_head gemm");
    x.n_slabs_head = splits;
    return UMLH_OK;
}

// dH^T = W_head^T dZ^T (image columns only), then dW_proj = dH^T X_img[index] as split-K slabs
static int f32_proj_backward(umlh_handle_t h, StepCall& x) {
    const umlh_config_t& c = h->cfg;
    const Layout& L = h->L;
    const int ri = x.ri;
    float* dht = ws(h, L.dht);
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = h->buf.w_head; g.lda = c.d_shared;            // A(m=n, k=c) = W[c][n]  (k-major)
    g.B = ws(h, L.dzt); g.ldb = L.ldz;                  // B(n=r, k=c) = dZ^T[c][r]
    g.M = c.d_shared; g.N = ri; g.K = c.num_classes;
    g.out = dht; g.ldo = L.rcap_img;
    g.k_chunk = g.K; g.alpha = 1.f;
    g.k_switch = INT_MAX; g.k_valid1 = g.K;
    HIPCHK(umlh_f32_launch_gemm(&g, 1, 1, 1, x.st), "dH gemm");
    int chunk = (int)round_up((ri + L.scap_proj - 1) / L.scap_proj, KT);
    if (chunk < 64) chunk = 64;
    const int splits = (ri + chunk - 1) / chunk;
    GemmArgs p;
    memset(&p, 0, sizeof(p));
    p.A = dht; p.lda = L.rcap_img;
    p.B = x.img->feats; p.k_rows = x.img->index; p.ldb = c.d_img;
    p.M = c.d_shared; p.N = c.d_img; p.K = ri;
    p.out = ws(h, L.slabs_proj); p.ldo = c.d_img;
    p.k_chunk = chunk; p.slab_stride = L.n_proj; p.alpha = 1.f;
    p.k_switch = INT_MAX; p.k_valid1 = ri;
    HIPCHK(umlh_f32_launch_gemm(&p, 0, 1, splits, x.st), "dW_proj gemm");
    x.n_slabs_proj = splits;
    return UMLH_OK;
}

static int forward_backward_f32(umlh_handle_t h, StepCall& x) {
    hipStream_t st = x.st;
    const bool proj = h->cfg.has_proj && x.ri > 0;
    mark(h, 0, st);
    if (proj) HIPCHK(launch_proj_forward(h, x.img, ws(h, h->L.h), st), "proj forward");
    mark(h, 1, st);
    RC(f32_forward_ce(h, x));
    mark(h, 2, st);
    if (!x.want_grad) return UMLH_OK;
    RC(f32_dw_head(h, x));
    mark(h, 3, st);
    if (x.overlap) RC(dp_after_head(h, x));
    if (proj) RC(f32_proj_backward(h, x));
    mark(h, 4, st);
    return UMLH_OK;
}

// Everything of a step up to (not including) the parameter update.
static int forward_backward(umlh_handle_t h, StepCall& x) {
    x.ri = x.img ? x.img->rows : 0;
    x.rt = x.txt ? x.txt->rows : 0;
    x.nb0 = fwd_blocks_img(h, x.ri);
    x.nb1 = (x.rt + h->ts - 1) / h->ts;
    x.r0p = x.nb0 * h->ts;
    x.r1p = x.nb1 * h->ts;
    return h->cfg.precision == UMLH_PREC_BF16 ? forward_backward_bf16(h, x) : forward_backward_f32(h, x);
}

static FinalizeArgs make_finalize(umlh_handle_t h, const umlh_batch_t* img, const umlh_batch_t* txt,
                                  const umlh_hyper_t* hy, bool from_partials, float* scalars_out, bool update) {
    const int ri = img ? img->rows : h->last_rows_img, rt = txt ? txt->rows : h->last_rows_txt;
    FinalizeArgs f;
    memset(&f, 0, sizeof(f));
    f.partials = from_partials ? ws(h, h->L.partials) : nullptr;
    f.nb0 = fwd_blocks_img(h, ri);
    f.nb1 = (rt + h->ts - 1) / h->ts;
    f.inv_rows0 = (img && img->rows > 0) ? 1.f / (float)img->global_rows : 0.f;
    f.inv_rows1 = (txt && txt->rows > 0) ? 1.f / (float)txt->global_rows : 0.f;
    f.w0 = hy ? hy->img_alpha : 1.f;
    f.w1 = hy ? hy->alpha : 1.f;
    f.tail = ws(h, h->L.grads) + msg_tail_off(h);
    f.scalars_out = scalars_out;
    f.scales = h->buf.scales; f.m_scales = h->buf.m_scales; f.v_scales = h->buf.v_scales;
    f.update_mask = 0;
    // a parameter is stepped iff its modality has rows on ANY rank (torch skips parameters without a gradient):
    // the data-parallel update must take the same decision on every rank, so it looks at the GLOBAL row counts
    const int gi = img ? img->global_rows : h->global_rows_img, gt = txt ? txt->global_rows : h->global_rows_txt;
    if (update && h->cfg.learnable_temp) f.update_mask = ((img ? ri : gi) > 0 ? 1 : 0) | ((txt ? rt : gt) > 0 ? 2 : 0);
    if (hy) f.opt = make_opt(h->cfg, *hy);
    return f;
}

static int check_step(umlh_handle_t h, const umlh_batch_t* img, const umlh_batch_t* txt, const umlh_hyper_t* hy,
                      const char* who, bool allow_empty_local = false) {
    if (!h || !h->bound) return fail(UMLH_E_UNBOUND, "%s: handle not bound", who);
    if (!hy) return fail(UMLH_E_INVALID, "%s: hyper is null", who);
    int rc = check_batch(h, img, h->cfg.max_rows_img, who);
    if (rc) return rc;
    rc = check_batch(h, txt, h->cfg.max_rows_txt, who);
    if (rc) return rc;
    // finetune.py:123 "At least one of the loaders should be provided"
    if ((img ? img->rows : 0) + (txt ? txt->rows : 0) == 0) {
        // data-parallel split: a rank may hold no row of a (small or unevenly sharded) global batch
        if (allow_empty_local && (img ? img->global_rows : 0) + (txt ? txt->global_rows : 0) > 0) return UMLH_OK;
        return fail(UMLH_E_INVALID, "%s: both modalities empty", who);
    }
    return UMLH_OK;
}

// The head reduce of a step, in the one form every launch of it takes (head_step_kernel through umlh_launch_head_step, or
// riding in the one-launch step of a linear bf16 head): `n_slabs` slabs of n_head floats at `slabs`, `stride` apart, are summed
// and the head is updated in place, or (grad_out != NULL, the data-parallel split step) the sum goes to grad_out with nothing
// updated.  The one-launch step fills in the slab counts itself.
static HeadFuse make_head_fuse(umlh_handle_t h, const OptArgs& o, const FinalizeArgs& f, const float* slabs, int n_slabs,
                               long long stride, float* grad_out) {
    HeadFuse hf;
    memset(&hf, 0, sizeof(hf));
    hf.slabs = slabs; hf.n_slabs = n_slabs; hf.slab_stride = stride; hf.C = h->cfg.num_classes; hf.K = h->cfg.d_shared;
    hf.cpad = class_pad(h); hf.o = o; hf.f = f;
    hf.grad_out = grad_out;
    if (!grad_out) {
        hf.p = h->buf.w_head; hf.m = h->buf.m_head; hf.v = h->buf.v_head;
        hf.shadow = h->cfg.precision == UMLH_PREC_BF16 ? ws16(h, h->L.w16) : nullptr;     // the next step's bf16 W shadow
    }
    return hf;
}
static inline bool head_fuse_shape(const umlh_handle_s* h) {
    return h->cfg.precision == UMLH_PREC_BF16 && !h->cfg.has_proj && h->cfg.d_shared % 8 == 0;
}

// head_step_kernel as a plain slab sum: no diagnostics, image slabs [0, n_slabs_img) summed before the text slabs
static DiagArgs diag_off(int n_slabs_img) {
    DiagArgs d;
    d.dst = nullptr; d.n_slabs_img = n_slabs_img; d.inv_w0 = d.inv_w1 = 0.f; d.part = nullptr; d.ticket = nullptr;
    return d;
}
// ... with the gradient diagnostics of the step written to `dst` (NULL: the plain slab sum)
static DiagArgs diag_live(umlh_handle_t h, const umlh_hyper_t* hy, float* dst, int n_slabs_img) {
    DiagArgs d = diag_off(n_slabs_img);
    if (!dst) return d;
    d.dst = dst;
    d.part = ws(h, h->L.diag_part);
    d.ticket = diag_ticket(h);
    d.cols = h->diag_cols;
    d.inv_w0 = hy->img_alpha != 0.f ? 1.f / hy->img_alpha : 0.f;
    d.inv_w1 = hy->alpha != 0.f ? 1.f / hy->alpha : 0.f;
    return d;
}

// Update the head from `n` slabs: the split-K slabs of dW_head (train_step_impl) or the one or two parts of the all-reduced
// gradient message (apply_update_impl).  `keep_shadow`: the W shadow the update kernel writes is the next forward's.
static int update_head(umlh_handle_t h, const float* slabs, int n, const OptArgs& o, const FinalizeArgs& f, const DiagArgs& dg,
                       bool keep_shadow, const char* what, hipStream_t st) {
    const HeadFuse hf = make_head_fuse(h, o, f, slabs, n, h->L.n_head, nullptr);
    if (hf.K % 8 == 0) {
        // one launch: slab sum + optimizer + next step's W shadow (bf16 / fp32 fragment-major) + scalars / logit scales
        float* shadow32 = h->L.w32s ? ws(h, h->L.w32s) : nullptr;
        HIPCHK(umlh_launch_head_step(&hf, &dg, shadow32, st), what);
        h->shadow_fresh = (hf.shadow || shadow32) && keep_shadow;
    } else {
        // (the two launches touch disjoint memory: the message tail, scalars and logit scales / the head weight and moments)
        HIPCHK(umlh_launch_finalize(&f, st), "finalize");
        HIPCHK(umlh_launch_reduce_update(1, slabs, n, hf.slab_stride, h->L.n_head, nullptr, hf.p, hf.m, hf.v, &o, 0, 0, st), "update head");
    }
    return UMLH_OK;
}

// Sum `n` head slabs (the first `n_img` hold image rows) into `out`, a head-sized part of the gradient message.  Image slabs
// and text slabs are summed separately, then added: the order of the fused step and of the one-launch gradient
// (step_update_task), so the message is bit-identical whichever launch form wrote it.
static int sum_head_slabs(umlh_handle_t h, const float* slabs, int n, int n_img, const OptArgs& o, const FinalizeArgs& f, float* out,
                          const char* what, hipStream_t st) {
    const HeadFuse hf = make_head_fuse(h, o, f, slabs, n, h->L.n_head, out);
    if (hf.K % 8 == 0) {
        const DiagArgs order = diag_off(n_img);
        HIPCHK(umlh_launch_head_step(&hf, &order, nullptr, st), what);
    } else {
        HIPCHK(umlh_launch_finalize(&f, st), "finalize");
        HIPCHK(umlh_launch_reduce_update(0, slabs, n, hf.slab_stride, h->L.n_head, out, nullptr, nullptr, nullptr, &o, 0, 0, st), what);
    }
    return UMLH_OK;
}

// Update img_proj from `n` slabs of n_proj floats (split-K slabs of dW_proj, or the all-reduced message part)
static int update_proj(umlh_handle_t h, const float* slabs, int n, const OptArgs& o, hipStream_t st) {
    HIPCHK(umlh_launch_reduce_update(1, slabs, n, h->L.n_proj, h->L.n_proj, nullptr, h->buf.w_proj, h->buf.m_proj, h->buf.v_proj, &o,
                                     frozen_lo(h), frozen_hi(h), st), "update proj");
    return UMLH_OK;
}

static int train_step_impl(umlh_handle_t h, const umlh_batch_t* img, const umlh_batch_t* txt, const umlh_hyper_t* hy,
                           float* scalars_out, hipStream_t st, bool keep_shadow) {
    // gradient diagnostics: written to the caller's scalar row (or the workspace tail) by the head-step launch
    h->dp_diag = false;
    float* tail = ws(h, h->L.grads) + msg_tail_off(h);
    float* diag_dst = h->diagnostics ? (scalars_out ? scalars_out : tail + 2) + UMLH_N_CORE_SCALARS : nullptr;
    OptArgs o = make_opt(h->cfg, *hy);
    FinalizeArgs f = make_finalize(h, img, txt, hy, true, scalars_out, true);
    // the update (and the step scalars) may ride in the forward + dW launch: linear bf16 head, no gradient diagnostics
    // (in profiling mode the interval mark 2 -> 3 then holds the whole step and the others are empty)
    StepCall x{img, txt, hy, true, st};
    HeadFuse hfuse;
    if (head_fuse_shape(h) && !diag_dst) { hfuse = make_head_fuse(h, o, f, ws(h, h->L.slabs_head), 0, h->L.n_head, nullptr); x.head = &hfuse; }
    RC(forward_backward(h, x));
    if (x.head_done) {
        h->shadow_fresh = keep_shadow;
        mark(h, 5, st);
        return UMLH_OK;
    }
    RC(update_head(h, ws(h, h->L.slabs_head), x.n_slabs_head, o, f, diag_live(h, hy, diag_dst, x.n_slabs_img), keep_shadow, "head step", st));
    if (x.n_slabs_proj > 0) RC(update_proj(h, ws(h, h->L.slabs_proj), x.n_slabs_proj, o, st));
    mark(h, 5, st);
    return UMLH_OK;
}


// --------------------------------------------------------------------------------------------------------------- //
// micro-step path (umlh_kernels_micro.hip): whole evaluation intervals of one or MANY heads in one persistent launch
// --------------------------------------------------------------------------------------------------------------- //
struct MicroItem {
    umlh_handle_t h;
    const umlh_stream_t* img; const umlh_stream_t* txt;
    const double* lr; int64_t first_step; float alpha, img_alpha; float* scalars_out;
};

static int device_cus(int dev) {
    static int cus[64];
    static std::once_flag once[64];
    const int d = dev & 63;
    std::call_once(once[d], [&] {
        hipDeviceProp_t p;
        cus[d] = hipGetDeviceProperties(&p, dev) == hipSuccess ? p.multiProcessorCount : 0;
    });
    return cus[d];
}

// Shape / row-count test of the micro path for `n_steps` steps of one head (no side effects).
static bool micro_eligible(umlh_handle_t h, const umlh_stream_t* img, const umlh_stream_t* txt, int n_steps) {
    if (!h->L.mc_flags || h->micro_off || h->diagnostics || h->profiling || n_steps < 1) return false;
    if (h->L.mc_nwg > device_cus(h->device) || h->L.mc_nwg > 64) return false;
    for (int k = 0; k < n_steps; ++k) {
        const int ri = img ? img->offsets[k + 1] - img->offsets[k] : 0, rt = txt ? txt->offsets[k + 1] - txt->offsets[k] : 0;
        if (ri < 0 || rt < 0 || ri + rt == 0) return false;
        if (ri > h->cfg.max_rows_img || rt > h->cfg.max_rows_txt) return false;
        if ((ri + 15) / 16 + (rt + 15) / 16 > UMLH_MICRO_MAX_ROWS / 16) return false;
    }
    return true;
}

static int micro_stage(umlh_handle_t h, unsigned char** out) {
    const size_t need = sizeof(UmlhMicroTable) + (size_t)UMLH_MICRO_MAX_HEADS * sizeof(UmlhMicroHead) + 64;
    if (!h->stage) {
        if (hipHostMalloc(reinterpret_cast<void**>(&h->stage), 2 * need, hipHostMallocDefault) != hipSuccess)
            return fail(UMLH_E_HIP, "micro step: pinned staging allocation failed");
        h->stage_bytes = need;
        for (int i = 0; i < 2; ++i)
            if (hipEventCreateWithFlags(&h->stage_ev[i], hipEventDisableTiming) != hipSuccess) return fail(UMLH_E_HIP, "micro step: event");
        (void)hipEventRecord(h->stage_ev[0], nullptr); (void)hipEventRecord(h->stage_ev[1], nullptr);
    }
    const int i = h->stage_next;
    h->stage_next ^= 1;
    if (hipEventSynchronize(h->stage_ev[i]) != hipSuccess) return fail(UMLH_E_HIP, "micro step: staging event");   // copy-out of its last use finished
    *out = h->stage + (size_t)i * h->stage_bytes;
    return i;
}

// Micro launches of one process on one device run one after the other, also when they are enqueued on different
// streams: two persistent grids that are each resident alone could otherwise strand each other's workgroups.
static std::mutex g_micro_mu;
static hipEvent_t g_micro_ev[64];
static bool g_micro_ev_ok[64];

// One launch: `n` heads x `n_steps` steps starting at step offset `k0` of every item's streams.
static int micro_launch_group(const MicroItem* it, int n, int k0, int n_steps, hipStream_t st) {
    umlh_handle_t h0 = it[0].h;
    unsigned char* stage0 = nullptr;
    const int sidx0 = micro_stage(h0, &stage0);
    if (sidx0 < 0) return sidx0;
    UmlhMicroHead* descs = reinterpret_cast<UmlhMicroHead*>(stage0 + sizeof(UmlhMicroTable));
    int grid = 0;
    for (int i = 0; i < n; ++i) {
        umlh_handle_t h = it[i].h;
        unsigned char* stg = stage0;
        int sidx = sidx0;
        if (i > 0) { sidx = micro_stage(h, &stg); if (sidx < 0) return sidx; }
        UmlhMicroTable* tab = reinterpret_cast<UmlhMicroTable*>(stg);
        for (int k = 0; k <= n_steps; ++k) {
            tab->offs[0][k] = it[i].img ? it[i].img->offsets[k0 + k] : 0;
            tab->offs[1][k] = it[i].txt ? it[i].txt->offsets[k0 + k] : 0;
        }
        for (int k = 0; k < n_steps; ++k) {
            umlh_hyper_t hy;
            memset(&hy, 0, sizeof(hy));
            hy.lr = it[i].lr[k0 + k]; hy.step = it[i].first_step + k0 + k;
            tab->opt[k] = make_opt(h->cfg, hy);
        }
        UmlhMicroTable* dtab = reinterpret_cast<UmlhMicroTable*>(ws(h, h->L.mc_tab));
        HIPCHK((int)hipMemcpyAsync(dtab, tab, sizeof(UmlhMicroTable), hipMemcpyHostToDevice, st), "micro step: table upload");
        if (i > 0) HIPCHK((int)hipEventRecord(h->stage_ev[sidx], st), "micro step: staging event");
        UmlhMicroHead& d = descs[i];
        memset(&d, 0, sizeof(d));
        const umlh_stream_t* s2[2] = {it[i].img, it[i].txt};
        for (int m = 0; m < 2; ++m) {
            if (!s2[m]) continue;
            d.feats[m] = s2[m]->feats; d.labels[m] = s2[m]->labels; d.index[m] = s2[m]->index; d.offs[m] = dtab->offs[m];
        }
        d.w = h->buf.w_head; d.m = h->buf.m_head; d.v = h->buf.v_head;
        d.scales = h->buf.scales; d.m_scales = h->buf.m_scales; d.v_scales = h->buf.v_scales;
        d.opt = dtab->opt;
        d.scalars_out = it[i].scalars_out ? it[i].scalars_out + (size_t)k0 * UMLH_N_SCALARS : nullptr;
        d.xchg = reinterpret_cast<unsigned long long*>(ws(h, h->L.mc_xchg));
        d.status = micro_status(h);
        static const bool dbg_micro = env_int("UMLH_DBG_MICRO", 0) == 1;
        d.stamps = (dbg_micro && dbg_floats(h->L) * sizeof(float) >= (size_t)h->L.mc_nwg * 96)
                       ? reinterpret_cast<unsigned long long*>(ws(h, h->L.dbg)) : nullptr;
        d.epoch0 = h->micro_epoch;
        h->micro_epoch += (unsigned)n_steps;
        h->micro_launches += 1;
        d.C = h->cfg.num_classes; d.d = h->cfg.d_shared; d.nwg = h->L.mc_nwg; d.wg0 = grid;
        d.learnable = h->cfg.learnable_temp; d.opt_kind = h->cfg.optimizer;
        d.w_img = it[i].img_alpha; d.w_txt = it[i].alpha;
        grid += d.nwg;
        h->shadow_fresh = false;
    }
    UmlhMicroHead* ddesc = reinterpret_cast<UmlhMicroHead*>(ws(h0, h0->L.mc_desc));
    HIPCHK((int)hipMemcpyAsync(ddesc, descs, sizeof(UmlhMicroHead) * (size_t)n, hipMemcpyHostToDevice, st), "micro step: descriptor upload");
    HIPCHK((int)hipEventRecord(h0->stage_ev[sidx0], st), "micro step: staging event");
    {
        std::lock_guard<std::mutex> lk(g_micro_mu);
        const int dv = h0->device & 63;
        if (!g_micro_ev_ok[dv]) {
            HIPCHK((int)hipEventCreateWithFlags(&g_micro_ev[dv], hipEventDisableTiming), "micro step: chain event");
            g_micro_ev_ok[dv] = true;
        } else {
            HIPCHK((int)hipStreamWaitEvent(st, g_micro_ev[dv], 0), "micro step: chain wait");
        }
        HIPCHK(umlh_micro_launch(h0->L.mc_nch, h0->L.mc_cw, h0->cfg.precision == UMLH_PREC_BF16, ddesc, n, n_steps, grid, st), "micro_steps_kernel");
        HIPCHK((int)hipEventRecord(g_micro_ev[dv], st), "micro step: chain record");
    }
    return UMLH_OK;
}

// All items: same number of steps; heads of one launch share the chunking (feature width) and fit the chip together.
static int micro_run(const MicroItem* it, int n_items, int n_steps, hipStream_t st) {
    const int cus = device_cus(it[0].h->device);
    for (int k0 = 0; k0 < n_steps; k0 += UMLH_MICRO_MAX_STEPS) {
        const int ns = n_steps - k0 < UMLH_MICRO_MAX_STEPS ? n_steps - k0 : UMLH_MICRO_MAX_STEPS;
        int a = 0;
        while (a < n_items) {
            int b = a, wgs = 0;
            while (b < n_items && b - a < UMLH_MICRO_MAX_HEADS && wgs + it[b].h->L.mc_nwg <= cus &&
                   it[b].h->cfg.d_shared == it[a].h->cfg.d_shared && it[b].h->cfg.precision == it[a].h->cfg.precision) {
                wgs += it[b].h->L.mc_nwg;
                ++b;
            }
            if (b == a) return fail(UMLH_E_INVALID, "micro step: head %d does not fit the device", a);
            int rc = micro_launch_group(it + a, b - a, k0, ns, st);
            if (rc) return rc;
            a = b;
        }
    }
    return UMLH_OK;
}

int umlh_micro_status(umlh_handle_t h, int32_t* status_out) {
    if (!h || !h->bound || !status_out) return fail(UMLH_E_INVALID, "umlh_micro_status: bad arguments");
    *status_out = 0;
    if (!h->L.mc_flags) return UMLH_OK;
    DeviceGuard dg_(h->device);
    unsigned v = 0;
    HIPCHK((int)hipMemcpy(&v, micro_status(h), sizeof(v), hipMemcpyDeviceToHost), "umlh_micro_status");
    *status_out = (int32_t)v;
    return UMLH_OK;
}

// status of the one-launch step's bounded waits: 0 = every wait of every step so far ended; else {code, first task of the range
// waited on, epoch, phase} of the FIRST wait that gave up (the step that hit it and all later ones applied no update)
int umlh_step_status(umlh_handle_t h, int32_t* status_out) {
    if (!h || !h->bound || !status_out) return fail(UMLH_E_INVALID, "umlh_step_status: bad arguments");
    status_out[0] = status_out[1] = status_out[2] = status_out[3] = 0;
    DeviceGuard dg_(h->device);
    if (h->L.fuse_flags) {
        HIPCHK((int)hipMemcpy(status_out, step_ctl(h).status, 4 * sizeof(int32_t), hipMemcpyDeviceToHost), "umlh_step_status");
    }
    if (status_out[0] == 0 && h->p2p_on) {       // the direct all-reduce's waits (30 s bound: a peer that never arrives)
        unsigned long long off = 0;
        if (umlh_p2p_status_offset(msg_cap_floats(h->L), h->n_ranks, &off) == 0) {
            unsigned v = 0;
            HIPCHK((int)hipMemcpy(&v, static_cast<unsigned char*>(h->p2p_region[h->p2p_rank]) + off, sizeof(v), hipMemcpyDeviceToHost), "umlh_step_status");
            if (v) { status_out[0] = 2; status_out[1] = (int32_t)(v >> 8); status_out[2] = (int32_t)h->p2p_epoch; status_out[3] = (int32_t)(v & 255u); }
        }
    }
    return UMLH_OK;
}

int umlh_step_launches(umlh_handle_t h, int64_t* out) {
    if (!h || !out) return fail(UMLH_E_INVALID, "umlh_step_launches: bad arguments");
    *out = h->step_launches;
    return UMLH_OK;
}

int umlh_micro_launches(umlh_handle_t h, int64_t* out) {
    if (!h || !out) return fail(UMLH_E_INVALID, "umlh_micro_launches: bad arguments");
    *out = h->micro_launches;
    return UMLH_OK;
}

static int check_streams(umlh_handle_t h, const umlh_stream_t* img, const umlh_stream_t* txt, int32_t n_steps, const double* lr,
                         const char* who) {
    if (!h || !h->bound) return fail(UMLH_E_UNBOUND, "%s: handle not bound", who);
    if (n_steps < 0 || !lr || (!img && !txt)) return fail(UMLH_E_INVALID, "%s: bad arguments", who);
    if ((img && (!img->offsets || !img->index)) || (txt && (!txt->offsets || !txt->index)))
        return fail(UMLH_E_INVALID, "%s: index/offsets required", who);
    return UMLH_OK;
}

int umlh_train_steps_grouped(const umlh_group_item_t* items, int32_t n_items, int32_t n_steps, void* stream) {
    if (!items || n_items < 1 || n_steps < 0) return fail(UMLH_E_INVALID, "umlh_train_steps_grouped: bad arguments");
    MicroItem* mi = new (std::nothrow) MicroItem[n_items];
    if (!mi) return fail(UMLH_E_INVALID, "umlh_train_steps_grouped: out of host memory");
    bool all_micro = true;
    int rc = UMLH_OK;
    for (int i = 0; i < n_items && !rc; ++i) {
        const umlh_group_item_t& g = items[i];
        rc = check_streams(g.handle, g.img, g.txt, n_steps, g.lr, "umlh_train_steps_grouped");
        if (rc) break;
        if (g.handle->device != items[0].handle->device) { rc = fail(UMLH_E_INVALID, "umlh_train_steps_grouped: heads on different devices"); break; }
        for (int j = 0; j < i; ++j)
            if (items[j].handle == g.handle) rc = fail(UMLH_E_INVALID, "umlh_train_steps_grouped: a handle appears twice");
        mi[i] = MicroItem{g.handle, g.img, g.txt, g.lr, g.first_step, g.alpha, g.img_alpha, g.scalars_out};
        all_micro = all_micro && micro_eligible(g.handle, g.img, g.txt, n_steps);
    }
    if (!rc && n_steps > 0) {
        DeviceGuard dg_(items[0].handle->device);
        if (all_micro) {
            rc = micro_run(mi, n_items, n_steps, (hipStream_t)stream);
        } else {          // shapes outside the micro kernel's envelope: the heads step one after the other on the general path
            for (int i = 0; i < n_items && !rc; ++i)
                rc = umlh_train_steps(items[i].handle, items[i].img, items[i].txt, n_steps, items[i].lr, items[i].first_step,
                                      items[i].alpha, items[i].img_alpha, items[i].scalars_out, stream);
        }
    }
    delete[] mi;
    return rc;
}

int umlh_train_step(umlh_handle_t h, const umlh_batch_t* img, const umlh_batch_t* txt, const umlh_hyper_t* hy,
                    float* scalars_out, void* stream) {
    int rc = check_step(h, img, txt, hy, "umlh_train_step");
    if (rc) return rc;
    DeviceGuard dg_(h->device);
    h->shadow_fresh = false;          // the caller may have rewritten w_head since the last call
    return train_step_impl(h, img, txt, hy, scalars_out, (hipStream_t)stream, false);
}

int umlh_train_steps(umlh_handle_t h, const umlh_stream_t* img, const umlh_stream_t* txt, int32_t n_steps,
                     const double* lr, int64_t first_step, float alpha, float img_alpha, float* scalars_out,
                     void* stream) {
    RC(check_streams(h, img, txt, n_steps, lr, "umlh_train_steps"));
    DeviceGuard dg_(h->device);
    const bool dp = h->n_ranks > 1 || h->dp_force;
    if (dp && h->n_ranks > 1 && !h->comm && !h->ar_fn && !h->p2p_on)
        return fail(UMLH_E_UNBOUND, "umlh_train_steps: %d ranks but no communicator", h->n_ranks);
    if (!dp && micro_eligible(h, img, txt, n_steps)) {       // batch <= 64 linear head: one persistent launch for all n_steps
        MicroItem it{h, img, txt, lr, first_step, alpha, img_alpha, scalars_out};
        return micro_run(&it, 1, n_steps, (hipStream_t)stream);
    }
    for (int k = 0; k < n_steps; ++k) {
        umlh_batch_t bi, bt;
        memset(&bi, 0, sizeof(bi));
        memset(&bt, 0, sizeof(bt));
        if (img) {
            bi.feats = img->feats; bi.feats_bf16 = img->feats_bf16; bi.labels = img->labels;
            bi.index = img->index + img->offsets[k];
            bi.rows = bi.global_rows = img->offsets[k + 1] - img->offsets[k];
        }
        if (txt) {
            bt.feats = txt->feats; bt.feats_bf16 = txt->feats_bf16; bt.labels = txt->labels;
            bt.index = txt->index + txt->offsets[k];
            bt.rows = bt.global_rows = txt->offsets[k + 1] - txt->offsets[k];
        }
        umlh_hyper_t hy;
        hy.lr = lr[k]; hy.step = first_step + k; hy.alpha = alpha; hy.img_alpha = img_alpha; hy.flags = 0; hy.reserved = 0;
        int rc = check_step(h, img ? &bi : nullptr, txt ? &bt : nullptr, &hy, "umlh_train_steps");
        if (rc) return rc;
        if (k == 0) h->shadow_fresh = false;
        float* so = scalars_out ? scalars_out + (size_t)k * UMLH_N_SCALARS : nullptr;
        if (dp) {
            // data parallel, equal shards: every rank brings the same row counts, the CE means divide by rows x ranks;
            // gradients -> SUM all-reduce (RCCL, enqueued on the same stream) -> identical update on every rank
            bi.global_rows = bi.rows * h->n_ranks;
            bt.global_rows = bt.rows * h->n_ranks;
            if (k > 0) hy.flags |= UMLH_F_WEIGHTS_UNCHANGED;      // the shadow of the weights this loop wrote is current
            rc = grad_step_impl(h, img ? &bi : nullptr, txt ? &bt : nullptr, &hy, (hipStream_t)stream, true);
            if (!rc) rc = apply_update_impl(h, &hy, so, (hipStream_t)stream);
        } else {
            rc = train_step_impl(h, img ? &bi : nullptr, txt ? &bt : nullptr, &hy, so, (hipStream_t)stream, k + 1 < n_steps);
        }
        if (rc) return rc;
    }
    h->shadow_fresh = false;
    return UMLH_OK;
}

// ---- RCCL, loaded at run time (the library has no link-time dependency on it; a process that imported torch already
// holds librccl.so.1 and gets that copy) ----
#include <dlfcn.h>
#include <rccl/rccl.h>
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclAllReduce) all_reduce = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
};
static RcclApi* rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) return;
        api.get_unique_id = reinterpret_cast<decltype(api.get_unique_id)>(dlsym(lib, "ncclGetUniqueId"));
        api.comm_init_rank = reinterpret_cast<decltype(api.comm_init_rank)>(dlsym(lib, "ncclCommInitRank"));
        api.all_reduce = reinterpret_cast<decltype(api.all_reduce)>(dlsym(lib, "ncclAllReduce"));
        api.comm_destroy = reinterpret_cast<decltype(api.comm_destroy)>(dlsym(lib, "ncclCommDestroy"));
        api.error_string = reinterpret_cast<decltype(api.error_string)>(dlsym(lib, "ncclGetErrorString"));
        if (api.get_unique_id && api.comm_init_rank && api.all_reduce && api.comm_destroy) api.lib = lib;
    });
    return api.lib ? &api : nullptr;
}

int umlh_comm_unique_id(void* id_out) {
    if (!id_out) return fail(UMLH_E_INVALID, "umlh_comm_unique_id: null argument");
    RcclApi* r = rccl_api();
    if (!r) return fail(UMLH_E_HIP, "umlh_comm_unique_id: librccl.so.1 could not be loaded");
    ncclUniqueId id;
    ncclResult_t e = r->get_unique_id(&id);
    if (e != ncclSuccess) return fail(UMLH_E_HIP, "ncclGetUniqueId: %s", r->error_string ? r->error_string(e) : "error");
    memcpy(id_out, &id, UMLH_COMM_ID_BYTES);
    return UMLH_OK;
}

static int dp_streams(umlh_handle_t h) {
    if (h->comm_stream) return UMLH_OK;
    HIPCHK((int)hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking), "data parallel: comm stream");
    HIPCHK((int)hipEventCreateWithFlags(&h->ev_head_ready, hipEventDisableTiming), "data parallel: event");
    HIPCHK((int)hipEventCreateWithFlags(&h->ev_head_done, hipEventDisableTiming), "data parallel: event");
    return UMLH_OK;
}

static void dp_release(umlh_handle_t h) {
    h->p2p_on = 0;
    if (h->comm && h->comm_owned) { RcclApi* r = rccl_api(); if (r) (void)r->comm_destroy(static_cast<ncclComm_t>(h->comm)); }
    h->comm = nullptr; h->comm_owned = false; h->ar_fn = nullptr; h->ar_ctx = nullptr; h->n_ranks = 1;
}

int umlh_comm_init_rank(umlh_handle_t h, const void* id, int32_t n_ranks, int32_t rank) {
    if (!h || !id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(UMLH_E_INVALID, "umlh_comm_init_rank: bad arguments");
    RcclApi* r = rccl_api();
    if (!r) return fail(UMLH_E_HIP, "umlh_comm_init_rank: librccl.so.1 could not be loaded");
    DeviceGuard dg_(h->device);
    dp_release(h);
    ncclUniqueId uid;
    memcpy(&uid, id, UMLH_COMM_ID_BYTES);
    ncclComm_t comm = nullptr;
    ncclResult_t e = r->comm_init_rank(&comm, n_ranks, uid, rank);
    if (e != ncclSuccess) return fail(UMLH_E_HIP, "ncclCommInitRank: %s", r->error_string ? r->error_string(e) : "error");
    h->comm = comm; h->comm_owned = true; h->n_ranks = n_ranks;
    return dp_streams(h);
}

int umlh_set_comm(umlh_handle_t h, void* nccl_comm, int32_t n_ranks) {
    if (!h || n_ranks < 1 || (!nccl_comm && n_ranks > 1)) return fail(UMLH_E_INVALID, "umlh_set_comm: bad arguments");
    if (nccl_comm && !rccl_api()) return fail(UMLH_E_HIP, "umlh_set_comm: librccl.so.1 could not be loaded");
    DeviceGuard dg_(h->device);
    dp_release(h);
    h->comm = nccl_comm; h->comm_owned = false; h->n_ranks = n_ranks;
    return nccl_comm ? dp_streams(h) : UMLH_OK;
}

// regions[q]: rank q's exchange region (umlh_p2p_region_bytes(umlh_grad_buffer floats, n_ranks) bytes from umlh_p2p_alloc on rank
// q, zero-filled) as mapped into THIS process: regions[rank] the local allocation, the others through umlh_p2p_open of the
// handles their owners exported.  The caller keeps the mappings alive until the handle is destroyed or another transport is set.
int umlh_p2p_attach(umlh_handle_t h, void* const* regions, int32_t n_ranks, int32_t rank) {
    if (!h || !regions || n_ranks < 1 || n_ranks > 8 || rank < 0 || rank >= n_ranks) return fail(UMLH_E_INVALID, "umlh_p2p_attach: bad arguments");
    if (h->cfg.has_proj) return fail(UMLH_E_INVALID, "umlh_p2p_attach: the 2-layer head overlaps two all-reduces per step on two streams; use RCCL there");
    for (int q = 0; q < n_ranks; ++q) if (!regions[q]) return fail(UMLH_E_INVALID, "umlh_p2p_attach: region %d is null", q);
    DeviceGuard dg_(h->device);
    dp_release(h);
    for (int q = 0; q < n_ranks; ++q) h->p2p_region[q] = regions[q];
    h->p2p_on = 1; h->p2p_rank = rank; h->p2p_epoch = 0; h->n_ranks = n_ranks;
    if (n_ranks == 1) h->dp_force = 1;
    return dp_streams(h);
}

int umlh_set_allreduce(umlh_handle_t h, umlh_allreduce_fn fn, void* ctx, int32_t n_ranks) {
    if (!h || n_ranks < 1 || (!fn && n_ranks > 1)) return fail(UMLH_E_INVALID, "umlh_set_allreduce: bad arguments");
    DeviceGuard dg_(h->device);
    dp_release(h);
    h->ar_fn = fn; h->ar_ctx = ctx; h->n_ranks = n_ranks;
    if (fn && n_ranks == 1) h->dp_force = 1;
    return fn ? dp_streams(h) : UMLH_OK;
}

// SUM all-reduce of `n` floats in place, enqueued on `st`
static int dp_allreduce(umlh_handle_t h, float* buf, long long n, hipStream_t st) {
    if (n <= 0) return UMLH_OK;
    if (h->p2p_on) {                 // direct reduce-scatter + all-gather over the peers' mapped regions (umlh_p2p.hip)
        if (++h->p2p_epoch == 0) h->p2p_epoch = 1;
        HIPCHK(umlh_p2p_launch(h->p2p_region, h->n_ranks, h->p2p_rank, buf, n, msg_cap_floats(h->L), h->p2p_epoch, st), "p2p all-reduce");
        return UMLH_OK;
    }
    if (h->ar_fn) {
        int rc = h->ar_fn(h->ar_ctx, buf, (uint64_t)n, st);
        return rc ? fail(UMLH_E_HIP, "data parallel: the all-reduce callback failed with code %d", rc) : UMLH_OK;
    }
    if (h->comm) {
        RcclApi* r = rccl_api();
        ncclResult_t e = r->all_reduce(buf, buf, (size_t)n, ncclFloat, ncclSum, static_cast<ncclComm_t>(h->comm), st);
        if (e != ncclSuccess) return fail(UMLH_E_HIP, "ncclAllReduce: %s", r->error_string ? r->error_string(e) : "error");
        return UMLH_OK;
    }
    return h->n_ranks > 1 ? fail(UMLH_E_UNBOUND, "data parallel: %d ranks but no communicator (umlh_comm_init_rank / umlh_set_comm / umlh_set_allreduce)", h->n_ranks)
                          : UMLH_OK;
}

// Sum the dW_head slabs into the gradient message: [g_head], or [g_img | g_txt] when the per-modality gradient
// diagnostics are on (finetune.py:190-191,203-206 need the GLOBAL per-modality gradients: dot products and norms are
// not linear in the ranks' partial sums, so the two sums travel separately and the update kernel forms the diagnostics
// from the all-reduced pair).
static int dp_reduce_head(umlh_handle_t h, const StepCall& x) {
    hipStream_t st = x.st;
    const int sh = x.n_slabs_head, si = x.n_slabs_img < sh ? x.n_slabs_img : sh;
    const OptArgs o = make_opt(h->cfg, *x.hy);
    const FinalizeArgs f = make_finalize(h, x.img, x.txt, x.hy, true, nullptr, false);
    const float* slabs = ws(h, h->L.slabs_head);
    float* grads = ws(h, h->L.grads);
    const long long nh = h->L.n_head;
    if (!h->dp_diag) return sum_head_slabs(h, slabs, sh, si, o, f, grads, "reduce head", st);
    FinalizeArgs f2 = f;
    f2.partials = nullptr;                               // the step scalars are formed once (first launch)
    if (si > 0) RC(sum_head_slabs(h, slabs, si, si, o, f, grads, "reduce head (image rows)", st));
    else HIPCHK((int)hipMemsetAsync(grads, 0, sizeof(float) * nh, st), "zero image gradient");
    if (sh - si > 0) RC(sum_head_slabs(h, slabs + (size_t)si * nh, sh - si, 0, o, si > 0 ? f2 : f, grads + nh, "reduce head (text rows)", st));
    else HIPCHK((int)hipMemsetAsync(grads + nh, 0, sizeof(float) * nh, st), "zero text gradient");
    return UMLH_OK;
}

// 2-layer head, data parallel: the head gradient is complete behind the dW_head GEMM; its all-reduce (12.8 MB at cfg3)
// runs on the second stream beside the img_proj backward GEMMs (dH^T, dW_proj) of the step's stream.
static int dp_after_head(umlh_handle_t h, const StepCall& x) {
    hipStream_t st = x.st;
    RC(dp_reduce_head(h, x));
    HIPCHK((int)hipEventRecord(h->ev_head_ready, st), "data parallel: event record");
    HIPCHK((int)hipStreamWaitEvent(h->comm_stream, h->ev_head_ready, 0), "data parallel: stream wait");
    RC(dp_allreduce(h, ws(h, h->L.grads), msg_head_len(h), h->comm_stream));
    HIPCHK((int)hipEventRecord(h->ev_head_done, h->comm_stream), "data parallel: event record");
    return UMLH_OK;
}

// Gradients of one step into the message buffer.  `comm`: also all-reduce it (the data-parallel multi-step loop); the
// head part then overlaps the img_proj backward when the head has one.
static int grad_step_impl(umlh_handle_t h, const umlh_batch_t* img, const umlh_batch_t* txt, const umlh_hyper_t* hy, hipStream_t st,
                          bool comm) {
    h->last_rows_img = img ? img->rows : 0;
    h->last_rows_txt = txt ? txt->rows : 0;
    h->global_rows_img = img ? img->global_rows : 0;
    h->global_rows_txt = txt ? txt->global_rows : 0;
    h->dp_diag = split_diag(h);
    float* grads = ws(h, h->L.grads);
    if (h->last_rows_img + h->last_rows_txt == 0) {       // no local row: this rank contributes zeros to the all-reduce
        HIPCHK((int)hipMemsetAsync(grads, 0, sizeof(float) * msg_len(h), st), "zero gradient buffer");
        return comm ? dp_allreduce(h, grads, msg_len(h), st) : UMLH_OK;
    }
    if (!(hy->flags & UMLH_F_WEIGHTS_UNCHANGED)) h->shadow_fresh = false;
    // (the gradient diagnostics of a split step are formed by umlh_apply_update)
    const bool overlap = comm && h->cfg.has_proj && h->comm_stream != nullptr && (img ? img->rows : 0) > 0;
    StepCall x{img, txt, hy, true, st};
    x.overlap = overlap;
    OptArgs o = make_opt(h->cfg, *hy);
    // linear bf16 head: the slab sum into the message (and the step scalars) rides in the forward + dW launch
    HeadFuse hfuse;
    if (head_fuse_shape(h) && !h->dp_diag && !overlap) {
        hfuse = make_head_fuse(h, o, make_finalize(h, img, txt, hy, true, nullptr, false), ws(h, h->L.slabs_head), 0, h->L.n_head, grads);
        x.head = &hfuse;
    }
    RC(forward_backward(h, x));
    if (!overlap && !x.head_done) RC(dp_reduce_head(h, x));
    const int sp = x.n_slabs_proj;
    if (h->cfg.has_proj) {
        float* gp = grads + msg_head_len(h);
        if (sp > 0)
            HIPCHK(umlh_launch_reduce_update(0, ws(h, h->L.slabs_proj), sp, h->L.n_proj, h->L.n_proj, gp, nullptr, nullptr, nullptr, &o, 0, 0, st),
                   "reduce proj");
        else
            HIPCHK((int)hipMemsetAsync(gp, 0, sizeof(float) * h->L.n_proj, st), "zero proj grad");
    }
    mark(h, 5, st);
    if (comm) {
        if (overlap) {                                    // head part is in flight on the second stream: the rest here, then join
            RC(dp_allreduce(h, grads + msg_head_len(h), msg_len(h) - msg_head_len(h), st));
            HIPCHK((int)hipStreamWaitEvent(st, h->ev_head_done, 0), "data parallel: stream wait");
        } else {
            RC(dp_allreduce(h, grads, msg_len(h), st));
        }
    }
    return UMLH_OK;
}

int umlh_grad_step(umlh_handle_t h, const umlh_batch_t* img, const umlh_batch_t* txt, const umlh_hyper_t* hy,
                   void* stream) {
    int rc = check_step(h, img, txt, hy, "umlh_grad_step", true);
    if (rc) return rc;
    DeviceGuard dg_(h->device);
    return grad_step_impl(h, img, txt, hy, (hipStream_t)stream, false);
}

int umlh_debug_buffer(umlh_handle_t h, void** device_ptr, uint64_t* n_bytes) {
    if (!h || !h->bound) return fail(UMLH_E_UNBOUND, "umlh_debug_buffer: handle not bound");
    if (device_ptr) *device_ptr = ws(h, h->L.dbg);
    if (n_bytes) *n_bytes = (uint64_t)dbg_floats(h->L) * sizeof(float);
    return UMLH_OK;
}

int umlh_grad_buffer(umlh_handle_t h, float** device_ptr, uint64_t* n_floats) {
    if (!h || !h->bound) return fail(UMLH_E_UNBOUND, "umlh_grad_buffer: handle not bound");
    if (device_ptr) *device_ptr = ws(h, h->L.grads);
    if (n_floats) *n_floats = (uint64_t)msg_floats(h->L, split_diag(h));         // the layout umlh_grad_step will use
    return UMLH_OK;
}

static int apply_update_impl(umlh_handle_t h, const umlh_hyper_t* hy, float* scalars_out, hipStream_t st) {
    OptArgs o = make_opt(h->cfg, *hy);
    float* grads = ws(h, h->L.grads);
    FinalizeArgs f = make_finalize(h, nullptr, nullptr, hy, false, scalars_out, true);
    // dp_diag: the two all-reduced per-modality gradients are the two "slabs" of the update kernel: it sums them, steps the
    // weights and accumulates dot / norms / sign agreement of the GLOBAL gradients (finetune.py:203-206).
    // (the shadow the update writes: the next umlh_grad_step may trust it, see umlh_grad_step)
    float* diag_dst = h->dp_diag ? (scalars_out ? scalars_out : f.tail + 2) + UMLH_N_CORE_SCALARS : nullptr;
    RC(update_head(h, grads, h->dp_diag ? 2 : 1, o, f, diag_live(h, hy, diag_dst, 1), true, "update head", st));
    if (h->cfg.has_proj && h->global_rows_img > 0) RC(update_proj(h, grads + msg_head_len(h), 1, o, st));
    return UMLH_OK;
}

int umlh_apply_update(umlh_handle_t h, const umlh_hyper_t* hy, float* scalars_out, void* stream) {
    if (!h || !h->bound) return fail(UMLH_E_UNBOUND, "umlh_apply_update: handle not bound");
    if (!hy) return fail(UMLH_E_INVALID, "umlh_apply_update: hyper is null");
    DeviceGuard dg_(h->device);
    return apply_update_impl(h, hy, scalars_out, (hipStream_t)stream);
}

// Forward only over one batch of image-side rows: the step scalars (umlh_eval_batch) or the per-row {CE, correct} (umlh_eval_rows)
static int eval_impl(umlh_handle_t h, const umlh_batch_t* b, float* scalars_out, float* row_stats, void* stream, const char* who) {
    if (!h || !h->bound) return fail(UMLH_E_UNBOUND, "%s: handle not bound", who);
    if (!b || (!scalars_out && !row_stats)) return fail(UMLH_E_INVALID, "%s: null argument", who);
    DeviceGuard dg_(h->device);
    RC(check_batch(h, b, h->cfg.max_rows_img, who));
    if (b->rows == 0) return fail(UMLH_E_INVALID, "%s: empty batch", who);
    hipStream_t st = (hipStream_t)stream;
    umlh_hyper_t hy;
    memset(&hy, 0, sizeof(hy));
    hy.lr = 0; hy.step = 1; hy.alpha = 1.f; hy.img_alpha = 1.f;
    h->shadow_fresh = false;
    StepCall x{b, nullptr, &hy, false, st};
    x.row_stats = row_stats;
    RC(forward_backward(h, x));
    if (!scalars_out) return UMLH_OK;
    FinalizeArgs f = make_finalize(h, b, nullptr, &hy, true, scalars_out, false);
    HIPCHK(umlh_launch_finalize(&f, st), "finalize");
    return UMLH_OK;
}

int umlh_eval_batch(umlh_handle_t h, const umlh_batch_t* b, float* scalars_out, void* stream) {
    return eval_impl(h, b, scalars_out, nullptr, stream, "umlh_eval_batch");
}

int umlh_eval_rows(umlh_handle_t h, const umlh_batch_t* b, float* row_stats, void* stream) {
    return eval_impl(h, b, nullptr, row_stats, stream, "umlh_eval_rows");
}
