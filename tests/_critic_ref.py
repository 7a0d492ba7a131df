"""The contract of the MultiBench critics of include/umlh.h (umlh_seq_mse_forward / _backward, umlh_infonce_forward / _backward)
restated in numpy, the plan of the decoder backward restated from csrc/umlh_host.h, the accuracy criteria the HIP kernels must
meet against the float64 evaluation, the case tables of tests/test_critic_kernels_gpu.py and a set of deliberately wrong variants
that the criteria must reject.  No GPU and no `umlh` import here.

seq_mse_ref and infonce_ref take `dtype`: float64 is the reference (MultiBench/models.py:129-175, 194-243), float32 is "an honest
fp32 implementation of the same formulas" and is what the composite bounds are calibrated on.  The fp32 evaluation restates the
kernels' arithmetic form only where csrc/umlh_kernels_seq.hip documents one: exp(x) is exp2 of the fp32-rounded x * log2(e)
(__expf), logits are dots * (1.f / temperature), lse = mx + log(s), row_loss = lse - diag, probs are exp(l - lse) - I (rebuilt
from lse, not e / s), and the gradient scale is 1.f / (n * temperature).

Criteria (none chosen in the GPU file, none set or changed by looking at a GPU result).
  * Single sums of products of a call's own inputs -- recon; dz, dw, db of the backward given the dres / loss_cnt / grad_out it is
    passed; dhat = probs . target_hat of the InfoNCE backward given arbitrary leaves -- meet _gemm_ref.CRIT_MAX / CRIT_RMS (2^-20
    max, 2^-23 rms) of |got - ref64| over the sum of the term magnitudes.  (Not dhat on a forward's own leaves: a row of
    softmax - I is one term near -1 followed by hundreds of small repeating ones, and the k-ordered fp32 chain the criterion is
    calibrated on reaches 2^-19 rms there at n = 257; tests/test_critic_ref_cpu.py emulates it.  The GPU test records that level.)
  * Ties to the kernel's own outputs are bit for bit: dres is float32(recon) - float32(x_target) on live positions and +0 on dead
    ones; loss_cnt[1] is D * #live (the + 1e-8 is absorbed in fp32 for every count >= 1; with no live position it is 1e-8);
    pred_hat / target_hat are x / norm as one IEEE fp32 division (the library is built without fast-math flags and hipcc's
    default is the correctly rounded fp32 division, so no ulp is allowed).
  * Sums of non-negative terms -- row_partial (the squares of the kernel's own dres), loss_cnt[0] (the kernel's own row partials
    over its own denominator) and the row norms -- are held relative to the float64 value at CRIT_MAX.
  * Composite outputs -- probs, row_loss, loss, dpred of InfoNCE; loss, dz, dw, db of the decoder taken end to end from the
    forward through the backward -- divide max|got - ref64| by max|ref64| of the output tensor (comp_err; an all-zero reference
    must be reproduced exactly).  The bound is 8 x the largest error of the fp32 evaluation over every case of the family and four
    data seeds, rounded up to a power of two; the factor covers contraction and summation orders numpy does not reproduce.  The
    sharp-softmax cases are a family of their own: at logits of +-100 one rounding of lse or of the diagonal logit is 2^-17
    absolute, a level the other cases must not inherit.  `leaves` is the InfoNCE backward on arbitrary leaves.  Measured on the
    CPU (log2 of the level -> log2 of the bound; tests/test_critic_ref_cpu.py re-measures them and allows 0.3 for another BLAS):

        family          output      level bound   |  family          output      level bound
        decoder         loss        -19.6   -16   |  infonce_sharp   probs       -10.8    -7
        decoder         dz          -20.4   -17   |  infonce_sharp   row_loss    -10.8    -7
        decoder         dw          -19.3   -16   |  infonce_sharp   loss         -9.3    -6
        decoder         db          -19.4   -16   |  infonce_sharp   dpred       -13.3   -10
        infonce         probs       -20.7   -17   |  leaves          dpred       -20.2   -17
        infonce         row_loss    -22.1   -19
        infonce         loss        -22.7   -19
        infonce         dpred       -19.8   -16

    The decoder's loss level is set by the smallest case (one live element: recon - x cancels to a few bits for two of the seeds),
    its dw / db levels by the 2112- and 4160-row sums; the sharp family's by rows whose loss is about 0.01 under logits of 100.

  * Exact values: n == 1 gives loss, probs and dpred exactly 0; no live position gives loss 0 and all three gradients exactly 0
    (not NaN); grad_out == 0 gives zeros.

Rows of norm below 1e-12.  The kernels divide by max(|x|, 1e-12) and the normalisation backward is c * (dy - y (y . dy)) / norm
for every row.  torch's F.normalize clamps with clamp_min, whose backward treats the denominator of a clamped row as the constant
1e-12 and so drops the projection term y (y . dy).  For |x| = 0 both agree (y = 0); for 0 < |x| < 1e-12 they differ by |y|^2 =
(|x| / 1e-12)^2 relative to the row's gradient.  infonce_ref returns both (dpred: the kernels' form, dpred_torch).
"""
import numpy as np

from _gemm_ref import CRIT_MAX, CRIT_RMS, gemm_err, meets_criterion, slab_count, spread_rows  # noqa: F401  (re-exported)
from _encoder_ref import bound_of, comp_err  # noqa: F401

F32, F64 = np.float32, np.float64
LOG2E = 1.4426950408889634
SPLIT_WGS = 768                  # csrc/umlh_host.h: splits_for's target when UMLH_ENC_SPLIT_WGS is unset (the tests never set it)
NORM_EPS = 1e-12
MSE_EPS = 1e-8
DATA_SEEDS = (0, 1, 2, 3)

DECODER_WRONG = ("target_t", "mask_t_lt_len", "denom_no_D", "t1_shifted", "len_not_clamped", "db_no_2")
INFONCE_WRONG = ("logits_transposed", "logits_times_temp", "targets_unnormalised", "no_mean", "no_projection")
WRONG_VARIANTS = DECODER_WRONG + INFONCE_WRONG


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------- #
# the plan of umlh_seq_mse_backward (csrc/umlh_host.h: splits_for, row_chunk; csrc/umlh_ops.cpp)
# ---------------------------------------------------------------------------------------------------------------------------- #
def splits_for(m, n, k):
    tiles = _cdiv(m, 64) * _cdiv(n, 64)
    if k < 128 or tiles >= SPLIT_WGS:
        return 1
    return max(1, min(_cdiv(SPLIT_WGS, tiles), k // 64, 32))


def row_chunk(M):
    return max(64, _cdiv(M, 64))


def plan(B, T, Z, D):
    """(sp, ns, chunk, nr): the planned splits of dW [D, Z] over the B*T rows, the slabs a split-K launch of sp actually produces,
    the rows per db chunk and the number of chunks."""
    R = B * T
    sp = splits_for(D, Z, R)
    chunk = row_chunk(R)
    return sp, slab_count(R, sp)[0], chunk, _cdiv(R, chunk)


def scratch_floats(B, T, Z, D):
    sp, _, _, nr = plan(B, T, Z, D)
    return sp * D * Z + nr * D + 64


# ---------------------------------------------------------------------------------------------------------------------------- #
# decoder Linear(z -> D) + masked next-step MSE
# ---------------------------------------------------------------------------------------------------------------------------- #
def live_mask(B, T, lengths, wrong=()):
    """bool[B, T]: position (b, t) enters the loss.  T == 1: every position; otherwise t < T - 1 and t + 1 < len_b."""
    if T == 1 and "t1_shifted" not in wrong:
        return np.ones((B, 1), bool)
    t = np.arange(T)[None, :]
    live = np.broadcast_to(t < T - 1, (B, T)).copy()
    if lengths is not None:
        ln = np.asarray(lengths, np.int64)[:, None]
        live &= (t < ln) if "mask_t_lt_len" in wrong else (t + 1 < ln)
    return live


def seq_mse_ref(z, w, b, x, lengths, grad_out, dtype=F64, wrong=()):
    """dict(recon [B,T,D], S_recon, live [B,T], dres [B,T,D], row_partial [B,T], loss, denominator, dz [B,T,Z], dw [D,Z], db [D])
    of the forward and of the backward on its own leaves.  T == 1: every position is live and the target is t; lengths None: the
    plain mean without the epsilon."""
    dt = dtype
    z, w, b, x = (np.asarray(a).astype(dt) for a in (z, w, b, x))
    B, T, Z = z.shape
    D = w.shape[0]
    live = live_mask(B, T, lengths, wrong)
    shift = T > 1 and "target_t" not in wrong
    xt = np.concatenate([x[:, 1:], x[:, -1:]], 1) if shift else x           # (the last position is never live when shifted)
    recon = (z.reshape(B * T, Z) @ w.T + b).astype(dt).reshape(B, T, D)
    dres = np.where(live[..., None], recon - xt, dt(0)).astype(dt)
    cnt = float(live.sum())
    if "len_not_clamped" in wrong and lengths is not None and T > 1:
        cnt = float(np.maximum(np.asarray(lengths, np.int64) - 1, 0).sum())
    cnt *= 1 if "denom_no_D" in wrong else D
    masked = lengths is not None and T > 1
    denom = dt(cnt) + dt(MSE_EPS) if masked or cnt == 0 else dt(cnt)
    row_partial = (dres * dres).sum(-1, dtype=dt)
    loss = dt(row_partial.sum(dtype=dt) / denom)
    s = dt(dt(2) * dt(grad_out) / denom)
    e2 = dres.reshape(B * T, D)
    dz = ((e2 @ w) * s).astype(dt).reshape(B, T, Z)
    dw = ((e2.T @ z.reshape(B * T, Z)) * s).astype(dt)
    db = (e2.sum(0, dtype=dt) * (s / dt(2) if "db_no_2" in wrong else s)).astype(dt)
    S_recon = np.abs(z.reshape(B * T, Z)) @ np.abs(w).T + np.abs(b)
    return dict(recon=recon, S_recon=S_recon.reshape(B, T, D), live=live, dres=dres, row_partial=row_partial, loss=loss,
                denominator=denom, dz=dz, dw=dw, db=db)


def seq_mse_backward_ref(z, w, dres, denominator, grad_out):
    """The backward as a function of its arguments, in float64: name -> (value, sum of term magnitudes) for dz, dw, db."""
    z, w, dres = (np.asarray(a, F64) for a in (z, w, dres))
    B, T, Z = z.shape
    D = w.shape[0]
    s = 2.0 * float(grad_out) / float(denominator)
    e, z2 = dres.reshape(B * T, D), z.reshape(B * T, Z)
    a = abs(s)
    return dict(dz=(s * (e @ w), a * (np.abs(e) @ np.abs(w))), dw=(s * (e.T @ z2), a * (np.abs(e).T @ np.abs(z2))),
                db=(s * e.sum(0), a * np.abs(e).sum(0)))


# ---------------------------------------------------------------------------------------------------------------------------- #
# SequenceInfoNCELoss
# ---------------------------------------------------------------------------------------------------------------------------- #
def _exp(x, dt):
    if dt == F64:
        return np.exp(x)
    return np.exp2((x * F32(LOG2E)).astype(F32)).astype(F32)


def _unit_rows(x, dt):
    with np.errstate(under="ignore"):
        nrm = np.maximum(np.sqrt((x * x).sum(-1, dtype=dt)), dt(NORM_EPS)).astype(dt)
    return (x / nrm[:, None]).astype(dt), nrm


def _normalize_bwd(dhat, y, nrm, c, dt, projection=True):
    """c * (dhat - y (y . dhat)) / nrm per row (c a scalar)."""
    cr = (dt(c) / nrm)[:, None]
    if not projection:
        return (cr * dhat).astype(dt)
    return (cr * (dhat - y * (y * dhat).sum(-1, keepdims=True, dtype=dt))).astype(dt)


def infonce_ref(pred, target, temperature, grad_out, dtype=F64, wrong=()):
    """dict(pred_hat, target_hat [n,D], pred_norm, target_norm [n], probs [n,n] = softmax - I, row_loss [n], loss, dhat [n,D],
    dpred [n,D] (the kernels' form for every row), dpred_torch (rows of norm below 1e-12 without the projection term))."""
    dt = dtype
    p, t = np.asarray(pred).astype(dt), np.asarray(target).astype(dt)
    n = p.shape[0]
    tau = F32(temperature)                                     # the entry points take a float
    ph, pn = _unit_rows(p, dt)
    th, tn = _unit_rows(t, dt)
    if "targets_unnormalised" in wrong:
        th = t
    dots = (ph @ th.T).astype(dt)
    if "logits_times_temp" in wrong:
        l = dots * dt(tau)
    else:
        l = (dots * (F32(1) / tau)).astype(dt) if dt == F32 else dots / dt(tau)
    if "logits_transposed" in wrong:
        l = l.T.copy()
    mx = l.max(-1, keepdims=True)
    ssum = _exp(l - mx, dt).sum(-1, dtype=dt)
    lse = (mx[:, 0] + np.log(ssum)).astype(dt)
    row_loss = (lse - np.diagonal(l)).astype(dt)
    probs = (_exp(l - lse[:, None], dt) - np.eye(n, dtype=dt)).astype(dt)
    mean = dt(1) if "no_mean" in wrong else dt(n)
    loss = dt(row_loss.sum(dtype=dt) / mean)
    dl = probs.T if "logits_transposed" in wrong else probs
    dhat = (dl @ th).astype(dt)
    if "logits_times_temp" in wrong:
        scale = dt(tau) / mean
    else:
        scale = F32(1) / (F32(mean) * tau) if dt == F32 else 1.0 / (float(mean) * float(tau))
    c = dt(dt(grad_out) * dt(scale))
    dpred = _normalize_bwd(dhat, ph, pn, c, dt, "no_projection" not in wrong)
    clamped = np.sqrt((p.astype(F64) ** 2).sum(-1)) < NORM_EPS
    dpred_torch = np.where(clamped[:, None], _normalize_bwd(dhat, ph, pn, c, dt, False), dpred)
    return dict(pred_hat=ph, target_hat=th, pred_norm=pn, target_norm=tn, probs=probs, row_loss=row_loss, loss=loss, dhat=dhat,
                dpred=dpred, dpred_torch=dpred_torch)


def infonce_backward_ref(pred_hat, target_hat, pred_norm, probs, grad_out, temperature, dtype=F64):
    """The backward as a function of its leaves: dict(dhat, S_dhat, dpred)."""
    dt = dtype
    ph, th, pn, pr = (np.asarray(a).astype(dt) for a in (pred_hat, target_hat, pred_norm, probs))
    n = ph.shape[0]
    tau = F32(temperature)
    dhat = (pr @ th).astype(dt)
    scale = F32(1) / (F32(n) * tau) if dt == F32 else 1.0 / (n * float(tau))
    return dict(dhat=dhat, S_dhat=np.abs(pr).astype(F64) @ np.abs(th).astype(F64),
                dpred=_normalize_bwd(dhat, ph, pn, dt(dt(grad_out) * dt(scale)), dt))


# ---------------------------------------------------------------------------------------------------------------------------- #
# case tables (tests/test_critic_kernels_gpu.py runs exactly these)
# ---------------------------------------------------------------------------------------------------------------------------- #
# id, (B, T, Z, D), the expected plan: sp, ns, chunk, nr
DECODER_CASES = [
    dict(id="a_sp1", B=3, T=9, Z=20, D=35, plan=(1, 1, 64, 1)),
    dict(id="b_t1", B=5, T=1, Z=8, D=6, plan=(1, 1, 64, 1)),
    dict(id="c_wide", B=2, T=4, Z=130, D=200, plan=(1, 1, 64, 1)),              # Z and D past the 128-thread loops
    dict(id="d_smallest", B=1, T=2, Z=1, D=1, plan=(1, 1, 64, 1)),
    dict(id="e_sp2", B=2, T=65, Z=40, D=35, plan=(2, 2, 64, 3)),                # 130 rows: 3 chunks, the last of 2 rows
    dict(id="f_sp3", B=4, T=50, Z=40, D=300, plan=(3, 3, 64, 4)),               # ragged 64-column tile in D
    dict(id="g_mosei", B=32, T=50, Z=40, D=35, plan=(25, 25, 64, 25)),          # the shape train() runs
    dict(id="h_cap32", B=33, T=64, Z=17, D=5, plan=(32, 27, 64, 33)),           # sp capped at 32, only 27 slabs produced
    dict(id="i_chunk65", B=65, T=64, Z=8, D=6, plan=(32, 29, 65, 64)),          # 65 rows per db chunk, 64 chunks
]
LENGTH_PATTERNS = ("none", "random", "edge", "dead")
GRAD_OUT = 3.0
ISOLATED_GRADS = (3.0, -0.5, 0.0)


def decoder_runs(c):
    """The lengths patterns a case runs under: all four at T > 1; at T == 1 with and without lengths."""
    return LENGTH_PATTERNS if c["T"] > 1 else ("none", "random")


def _rng(tag, data_seed):
    return np.random.default_rng([sum(ord(ch) for ch in tag) * 7919 + len(tag), int(data_seed)])


def build_lengths(c, pattern, data_seed=0):
    """int64[B] or None.  edge: T + 3, 0, T, -2, 1 in turn (then uniform in 1..T); dead: 1, 0, -2 in turn (no live position)."""
    B, T = c["B"], c["T"]
    rng = _rng(c["id"] + pattern, data_seed)
    if pattern == "none":
        return None
    if pattern == "random":
        return rng.integers(1, T + 1, B).astype(np.int64)
    if pattern == "edge":
        ln = rng.integers(1, T + 1, B).astype(np.int64)
        head = np.array([T + 3, 0, T, -2, 1], np.int64)[:B]
        ln[:head.size] = head
        return ln
    if pattern == "dead":
        return np.array([1, 0, -2], np.int64)[np.arange(B) % 3]
    raise KeyError(pattern)


def build_decoder(c, data_seed=0):
    """z [B,T,Z], w [D,Z] (N(0, 1/Z)), bias [D], x [B,T,D]: fp32."""
    rng = _rng(c["id"], data_seed)
    B, T, Z, D = c["B"], c["T"], c["Z"], c["D"]
    z, x = rng.standard_normal((B, T, Z)), rng.standard_normal((B, T, D))
    w, b = rng.standard_normal((D, Z)) / np.sqrt(Z), 0.1 * rng.standard_normal(D)
    return tuple(a.astype(F32) for a in (z, w, b, x))


def build_isolated(c, data_seed=0):
    """Hand-made leaves of the backward: dres [B,T,D] with row magnitudes over 10^+-3, a denominator that no forward produced."""
    rng = _rng(c["id"] + "isolated", data_seed)
    B, T, D = c["B"], c["T"], c["D"]
    return spread_rows(rng, B * T, D).reshape(B, T, D), F32(37.0 + B * T)


def decoder_eval(c, pattern, data_seed, dtype=F64, wrong=()):
    z, w, b, x = build_decoder(c, data_seed)
    r = seq_mse_ref(z, w, b, x, build_lengths(c, pattern, data_seed), GRAD_OUT, dtype, wrong)
    return {k: r[k] for k in ("loss", "dz", "dw", "db")}


# (n, D, temperature, kind)
INFONCE_CASES = [
    (1, 8, 0.07, "random"), (1, 1, 1.0, "random"), (2, 1, 1.0, "random"), (2, 300, 0.07, "random"), (3, 63, 0.07, "random"),
    (4, 64, 1.0, "random"), (5, 65, 0.07, "random"), (63, 300, 0.07, "random"), (64, 8, 1.0, "random"), (65, 64, 0.07, "random"),
    (257, 65, 0.07, "random"), (257, 1, 1.0, "random"),
    (257, 8, 0.01, "sharp"), (64, 1, 0.01, "sharp"), (5, 8, 0.01, "sharp"),
    (65, 63, 0.07, "zero_row"), (4, 8, 1.0, "zero_row"),
    (64, 300, 0.07, "tiny_row"), (5, 1, 0.07, "tiny_row"),
    (63, 64, 0.07, "duplicate_targets"), (3, 8, 1.0, "duplicate_targets"),
]
TINY_NORM = 1e-15


def infonce_id(c):
    return f"n{c[0]}_d{c[1]}_t{c[2]}_{c[3]}"


def infonce_family(c):
    return "infonce_sharp" if c[3] == "sharp" else "infonce"


def special_row(c):
    return c[0] // 2


def build_infonce(c, data_seed=0):
    """pred, target [n, D] fp32."""
    n, D, _, kind = c
    rng = _rng(infonce_id(c), data_seed)
    pred = rng.standard_normal((n, D))
    target = pred + 0.01 * rng.standard_normal((n, D)) if kind == "sharp" else rng.standard_normal((n, D))
    if kind == "zero_row":
        pred[special_row(c)] = 0.0
    elif kind == "tiny_row":
        v = rng.standard_normal(D)
        pred[special_row(c)] = TINY_NORM * v / np.linalg.norm(v)
    elif kind == "duplicate_targets":
        target[1] = target[0]
        if n > 4:
            target[n - 1] = target[0]
    return pred.astype(F32), target.astype(F32)


def build_leaves(c, data_seed=0):
    """Arbitrary leaves of the InfoNCE backward (no forward produced them): pred_hat, target_hat [n,D], pred_norm [n] in 0.5 .. 2,
    probs [n,n] with row magnitudes over 10^+-3."""
    n, D = c[0], c[1]
    rng = _rng(infonce_id(c) + "leaves", data_seed)
    return (rng.standard_normal((n, D)).astype(F32), rng.standard_normal((n, D)).astype(F32), rng.uniform(0.5, 2.0, n).astype(F32),
            spread_rows(rng, n, n))


COMPOSITE = ("probs", "row_loss", "loss", "dpred")


def infonce_eval(c, data_seed, dtype=F64, wrong=()):
    pred, target = build_infonce(c, data_seed)
    r = infonce_ref(pred, target, c[2], GRAD_OUT, dtype, wrong)
    return {k: r[k] for k in COMPOSITE}


def leaves_eval(c, data_seed, dtype=F64):
    ph, th, pn, pr = build_leaves(c, data_seed)
    return dict(dpred=infonce_backward_ref(ph, th, pn, pr, GRAD_OUT, c[2], dtype)["dpred"])


# ---------------------------------------------------------------------------------------------------------------------------- #
# levels of the fp32 evaluation and the bounds derived from them
# ---------------------------------------------------------------------------------------------------------------------------- #
# log2 of the measured levels (rounded up to 0.1), the table of the module docstring
LEVELS_LOG2 = {
    "decoder": {"loss": -19.6, "dz": -20.4, "dw": -19.3, "db": -19.4},
    "infonce": {"probs": -20.7, "row_loss": -22.1, "loss": -22.7, "dpred": -19.8},
    "infonce_sharp": {"probs": -10.8, "row_loss": -10.8, "loss": -9.3, "dpred": -13.3},
    "leaves": {"dpred": -20.2},
}


def measure_levels():
    """family -> output -> largest comp_err of the fp32 evaluation against float64 over every case and four data seeds."""
    lv = {}

    def note(fam, got, ref):
        for k in ref:
            lv.setdefault(fam, {})[k] = max(lv.get(fam, {}).get(k, 0.0), comp_err(got[k], ref[k]))
    for ds in DATA_SEEDS:
        for c in DECODER_CASES:
            for pat in decoder_runs(c):
                note("decoder", decoder_eval(c, pat, ds, F32), decoder_eval(c, pat, ds))
        for c in INFONCE_CASES:
            note(infonce_family(c), infonce_eval(c, ds, F32), infonce_eval(c, ds))
            note("leaves", leaves_eval(c, ds, F32), leaves_eval(c, ds))
    return lv


BOUNDS = {fam: {k: bound_of(v) for k, v in d.items()} for fam, d in LEVELS_LOG2.items()}


def variant_excess(name):
    """The largest error / bound of the float64 wrong variant `name` against the float64 reference over the cases of its family
    (must be >= 8: the criterion rejects the variant)."""
    w, worst = (name,), 0.0
    if name in DECODER_WRONG:
        for c in DECODER_CASES:
            for pat in decoder_runs(c):
                got, ref = decoder_eval(c, pat, 0, F64, w), decoder_eval(c, pat, 0)
                worst = max([worst] + [comp_err(got[k], ref[k]) / BOUNDS["decoder"][k] for k in ref])
    elif name in INFONCE_WRONG:
        for c in INFONCE_CASES:
            got, ref = infonce_eval(c, 0, F64, w), infonce_eval(c, 0)
            worst = max([worst] + [comp_err(got[k], ref[k]) / BOUNDS[infonce_family(c)][k] for k in ref])
    else:
        raise KeyError(name)
    return worst
