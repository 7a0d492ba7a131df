"""The contract of the MultiBench encoder entry points of include/umlh.h (umlh_attention_*, umlh_add_layernorm_forward,
umlh_layernorm_backward, the small row / column ops, umlh_encoder_layer_* and umlh_encoder_stack_*) restated in numpy, the
accuracy criterion the HIP kernels must meet against its float64 evaluation, the case tables of tests/test_encoder_kernels_gpu.py
and a set of deliberately wrong variants that the criterion must reject.  No GPU and no `umlh` import here.

Every function takes `dtype`: float64 is the reference, float32 is "an honest fp32 implementation of the same formulas" and is
what the bounds are calibrated on.  The fp32 evaluation restates the kernels' arithmetic form only where the source documents
a form that limits accuracy:
  * exp(x) is exp2 of the fp32-rounded x * log2(e) (__expf in csrc/umlh_kernels_enc.hip);
  * the attention backward rebuilds the probabilities as exp(s - lse) from the saved fp32 lse and from scores formed as
    (q . k) * scale, while the forward forms (q * scale) . k (the comment above attention_bwd_kernel): at scores of +-30 the
    rounding of s and of lse is a relative error of about 2^-19 in every probability of the backward.
Both were written down before any GPU run; no bound below was set or changed by looking at a GPU result.

Criterion.  The error of an output is |got - ref64|.
  * Sum-like kernels (umlh_colsum, umlh_positions_backward, dgamma / dbeta of umlh_layernorm_backward) divide it by the sum of
    the magnitudes of the output's terms and must meet _gemm_ref.CRIT_MAX / CRIT_RMS (2^-20 / 2^-23) over the outputs.
  * Composite outputs divide the largest error by max|ref64| of the output tensor (dqkv is one tensor: at T = 1 its dq and dk
    thirds are identically zero in the reference).  An all-zero reference tensor must be reproduced exactly.  Their bound is
    8 x the largest error of the fp32 evaluation over every case of the family (p = 0 and the listed p) and four data seeds,
    rounded up to a power of two; the factor covers the summation orders the CPU does not reproduce (split-K slabs, wave
    reductions, 16 row groups).  Measured on the CPU (log2 of the level -> log2 of the bound; tests/test_encoder_ref_cpu.py
    re-measures them and allows 0.3 for another BLAS):

        family          output      level bound   |  family          output      level bound   |  family          output      level bound
        attention       ctx         -21.7   -18   |  layer           d_in_b      -20.1   -17   |  stack           d_in_w      -21.4   -18
        attention       lse         -23.2   -20   |  layer           d_out_w     -20.2   -17   |  stack           d_in_b      -21.5   -18
        attention       dqkv        -20.2   -17   |  layer           d_out_b     -20.9   -17   |  stack           d_out_w     -21.1   -18
        attention_sharp ctx         -21.6   -18   |  layer           d_w1        -21.1   -18   |  stack           d_out_b     -21.0   -18
        attention_sharp lse         -23.6   -20   |  layer           d_b1        -20.9   -17   |  stack           d_w1        -21.3   -18
        attention_sharp dqkv        -17.7   -14   |  layer           d_w2        -20.6   -17   |  stack           d_b1        -21.4   -18
        layernorm       y           -22.2   -19   |  layer           d_b2        -21.1   -18   |  stack           d_w2        -21.5   -18
        layernorm       mean        -20.0   -17   |  layer           d_g1        -20.2   -17   |  stack           d_b2        -22.2   -19
        layernorm       rstd        -22.5   -19   |  layer           d_be1       -19.9   -16   |  stack           d_g1        -21.1   -18
        layernorm       ds          -22.5   -19   |  layer           d_g2        -20.3   -17   |  stack           d_be1       -21.3   -18
        layer           h_out       -20.7   -17   |  layer           d_be2       -20.9   -17   |  stack           d_g2        -21.4   -18
        layer           dh_in       -20.6   -17   |  stack           h_out       -21.5   -18   |  stack           d_be2       -21.6   -18
        layer           d_in_w      -19.8   -16   |  stack           dh_in       -21.1   -18

Relu kinks.  A FFN unit whose pre-activation is within rounding of 0 can switch between two fp32 implementations, and the
gradients then differ by a discrete amount.  The layer and stack tables fix data seeds for which the float64 reference (with
the case's masks, at p = 0 and at the listed p) has no pre-activation with |pre| <= 2^-16 * (sum_k |x1_k w1_fk| + |b1_f|):
16 x the GEMM criterion's max, so no unit can flip unless an upstream error already breaks a bound.  The GPU assertions
therefore carry no "may differ" allowance.

Masks.  keep_mask() restates the counter hash of csrc/umlh_common.h: keep_elem so that the seeds can be searched and the levels
measured at p > 0 on the CPU.  The GPU tests take every mask from umlh_dropout on a tensor of ones and assert that it equals
keep_mask bit for bit, so the restatement cannot drift from the kernels unnoticed.
"""
import numpy as np

from _gemm_ref import CRIT_MAX, CRIT_RMS, gemm_err, spread_rows  # noqa: F401  (re-exported for the tests)

F32, F64 = np.float32, np.float64
LOG2E = 1.4426950408889634
KINK = 2.0 ** -16
STACK_SEED_STRIDE = 7919          # include/umlh.h: layer li draws from cfg->seed + 7919*li
EPS = 1e-5

WRONG_VARIANTS = ("mask_transposed", "l_kept_only", "dv_no_inv_keep", "dS_dropped", "streams_swapped", "layer1_uses_layer0_streams",
                  "pad_off_by_one", "ln_no_eps", "dgamma_no_rstd")


# ---------------------------------------------------------------------------------------------------------------------------- #
# dropout masks
# ---------------------------------------------------------------------------------------------------------------------------- #
def drop_thresh(p):
    p = float(F32(p))
    return 0 if p <= 0 else int(p * 4294967296.0)


def inv_keep(p, dtype=F64):
    """1 / (1 - float32(p)): in float64 for the reference, in fp32 arithmetic (the kernels' 1.f / (1.f - p)) for dtype float32."""
    if F32(p) <= 0:
        return dtype(1)
    return F32(1) / (F32(1) - F32(p)) if dtype == F32 else 1.0 / (1.0 - float(F32(p)))


def keep_mask(seed, n, p):
    """bool[n]: element i of stream `seed` is kept (csrc/umlh_common.h: keep_elem)."""
    th = drop_thresh(p)
    if th == 0:
        return np.ones(n, dtype=bool)
    with np.errstate(over="ignore"):
        x = np.uint64(seed % 2 ** 64) + np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(32)) >= np.uint64(th)


def layer_masks(cfg, seed, mask_fn=keep_mask):
    """The four masks of one layer call with dropout base `seed`; mask_fn(seed, n, p) -> bool[n] (the GPU tests pass a function
    that runs umlh_dropout on ones)."""
    T, B, Z, H, F, p = cfg["T"], cfg["B"], cfg["Z"], cfg["H"], cfg["d_ff"], cfg["p"]
    M = T * B
    return dict(att=mask_fn(seed, B * H * T * T, p).reshape(B, H, T, T), d1=mask_fn(seed + 1, M * Z, p).reshape(M, Z),
                ffn=mask_fn(seed + 2, M * F, p).reshape(M, F), d2=mask_fn(seed + 3, M * Z, p).reshape(M, Z))


# ---------------------------------------------------------------------------------------------------------------------------- #
# errors
# ---------------------------------------------------------------------------------------------------------------------------- #
def comp_err(got, ref):
    """max|got - ref| / max|ref| (an all-zero reference must be reproduced exactly; a non-finite got is an infinite error)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return np.inf
    d, s = float(np.abs(got - ref).max(initial=0.0)), float(np.abs(ref).max(initial=0.0))
    return d / s if s > 0 else (0.0 if d == 0 else np.inf)


def _exp(x, dt):
    if dt == F64:
        return np.exp(x)
    return np.exp2((x * F32(LOG2E)).astype(F32)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------- #
# attention
# ---------------------------------------------------------------------------------------------------------------------------- #
def visible(lengths, T, B, off=0):
    """bool[B, T, T]: key j is visible to query t iff j <= t and j < len_b (+ off: the off-by-one variant)."""
    ln = np.full(B, T, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64)
    j = np.arange(T)
    return (j[None, None, :] <= j[None, :, None]) & (j[None, None, :] < (ln[:, None, None] + off))


def attention_ref(qkv, lengths, T, B, Z, H, keep=None, inv_keep=1.0, dctx=None, dtype=F64, wrong=()):
    """ctx [T,B,Z], lse [B,H,T] (and dqkv [T,B,3Z] when dctx is given) of umlh_attention_forward / _backward.  keep: bool
    [B,H,T,T] (element ((b*H + h)*T + t)*T + j of the stream) or None; lse is over the undropped scores; dropout multiplies the
    normalised probabilities by keep * inv_keep."""
    dt, dh = dtype, Z // H
    x = np.asarray(qkv).astype(dt).reshape(T, B, 3, H, dh)
    q, k, v = (x[:, :, i].transpose(1, 2, 0, 3) for i in range(3))                  # [B,H,T,dh]
    scale = dt(1.0 / np.sqrt(dh))
    vis = visible(lengths, T, B, 1 if "pad_off_by_one" in wrong else 0)[:, None]     # [B,1,T,T]
    kT = k.transpose(0, 1, 3, 2)
    s = np.where(vis, np.matmul(q * scale, kT), dt(-np.inf))
    mx = s.max(-1, keepdims=True)
    e = np.where(vis, _exp(np.where(vis, s - mx, dt(0)), dt), dt(0))
    kp = np.ones((B, H, T, T), dt) if keep is None else np.asarray(keep).reshape(B, H, T, T).astype(dt)
    if "mask_transposed" in wrong:
        kp = kp.transpose(0, 1, 3, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = ((e * kp) if "l_kept_only" in wrong else e).sum(-1, keepdims=True)
        P = e / l
        ik = dt(inv_keep)
        ctx = np.matmul(P * kp * ik, v)
        lse = (mx + np.log(l))[..., 0].astype(dt)
    ctx = ctx.transpose(2, 0, 1, 3).reshape(T, B, Z)
    assert ctx.dtype == dt and lse.dtype == dt
    if dctx is None:
        return ctx, lse
    # backward: p = exp(s - lse) rebuilt from the saved lse, scores as (q . k) * scale
    dO = np.asarray(dctx).astype(dt).reshape(T, B, H, dh).transpose(1, 2, 0, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        sb = np.matmul(q, kT) * scale
        Pb = np.where(vis, _exp(np.where(vis, sb - lse[..., None], dt(0)), dt), dt(0))
        Pd = Pb * kp * ik
        dP = np.matmul(dO, v.transpose(0, 1, 3, 2)) * kp * ik
        D = (Pb * dP).sum(-1, keepdims=True)
        dS = (Pd if "dS_dropped" in wrong else Pb) * (dP - D) * scale
        dq, dk = np.matmul(dS, k), np.matmul(dS.transpose(0, 1, 3, 2), q)
        dv = np.matmul((Pb * kp if "dv_no_inv_keep" in wrong else Pd).transpose(0, 1, 3, 2), dO)
    dqkv = np.stack([dq, dk, dv], 0).transpose(3, 1, 0, 2, 4).reshape(T, B, 3 * Z)     # [3,B,H,T,dh] -> [T,B,3,H,dh]
    assert dqkv.dtype == dt
    return ctx, lse, dqkv


# ---------------------------------------------------------------------------------------------------------------------------- #
# LayerNorm and the small ops
# ---------------------------------------------------------------------------------------------------------------------------- #
def layernorm_ref(x, r, gamma, beta, eps=EPS, dtype=F64, wrong=()):
    """s = x + r (r may be None), y = LayerNorm(s) * gamma + beta, mean [M], rstd [M] (biased variance, two passes)."""
    dt = dtype
    s = np.asarray(x).astype(dt) + (0 if r is None else np.asarray(r).astype(dt))
    s = s.astype(dt)
    mean = s.mean(-1, dtype=dt)
    d = s - mean[:, None]
    var = (d * d).mean(-1, dtype=dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = (dt(1) / np.sqrt(var + (dt(0) if "ln_no_eps" in wrong else dt(F32(eps))))).astype(dt)
        y = d * rstd[:, None] * np.asarray(gamma).astype(dt) + np.asarray(beta).astype(dt)
    return s, y.astype(dt), mean, rstd


def layernorm_bwd_ref(dy, s, gamma, mean, rstd, dtype=F64, wrong=()):
    """ds [M,N], dgamma [N], dbeta [N], and the term-magnitude sums of dgamma and dbeta (the sum criterion's scale)."""
    dt = dtype
    dy, s, gamma = (np.asarray(a).astype(dt) for a in (dy, s, gamma))
    mean, rstd = np.asarray(mean).astype(dt)[:, None], np.asarray(rstd).astype(dt)[:, None]
    N = dy.shape[1]
    xh = (s - mean) * rstd
    g = gamma * dy
    a = g.sum(-1, keepdims=True, dtype=dt) / dt(N)
    b = (g * xh).sum(-1, keepdims=True, dtype=dt) / dt(N)
    ds = rstd * (g - a - xh * b)
    tg = dy * (s - mean) if "dgamma_no_rstd" in wrong else dy * xh
    return ds.astype(dt), tg.sum(0, dtype=dt), dy.sum(0, dtype=dt), np.abs(tg).sum(0), np.abs(dy).sum(0)


def colsum_ref(x):
    x = np.asarray(x, F64)
    return x.sum(0), np.abs(x).sum(0)


def positions_backward_ref(dx, T, B, Z):
    dx = np.asarray(dx, F64).reshape(T, B, Z)
    return dx.sum(1), np.abs(dx).sum(1)


def add_positions_ref(x, pos, T, B, Z):
    """fp32, one rounding per element: the kernel must be bit-equal."""
    return (np.asarray(x, F32).reshape(T, B, Z) + np.asarray(pos, F32).reshape(T, 1, Z)).astype(F32)


def gather_rows_ref(x, idx, n_out_rows, scatter):
    x, idx = np.asarray(x, F32), np.asarray(idx, np.int64)
    if not scatter:
        return x[idx]
    out = np.zeros((n_out_rows, x.shape[1]), F32)
    out[idx] = x
    return out


def bias_act_ref(y, bias, relu):
    """fp32 y + bias[n], then relu as the kernels' fmaxf(., 0): everything that is not > 0 (negatives, -0.0, NaN) becomes +0.0."""
    v = np.asarray(y, F32) + (F32(0) if bias is None else np.asarray(bias, F32)[None, :])
    v = v.astype(F32)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, v, F32(0)) if relu else v


def relu_backward_ref(y, dy):
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(y, F32) > 0, np.asarray(dy, F32), F32(0))


# ---------------------------------------------------------------------------------------------------------------------------- #
# one post-norm layer and the stack
# ---------------------------------------------------------------------------------------------------------------------------- #
PARAM_NAMES = ("in_w", "in_b", "out_w", "out_b", "w1", "b1", "w2", "b2", "g1", "be1", "g2", "be2")


def param_shapes(Z, F):
    return [(3 * Z, Z), (3 * Z,), (Z, Z), (Z,), (F, Z), (F,), (Z, F), (Z,), (Z,), (Z,), (Z,), (Z,)]


def layer_ref(cfg, params, h_in, lengths, masks=None, dh_out=None, dtype=F64, wrong=()):
    """The post-norm layer of include/umlh.h: x1 = norm1(h_in + drop1(attn(h_in))), h_out = norm2(x1 + drop2(linear2(dropf(relu(
    linear1(x1)))))).  cfg: dict(T, B, Z, H, d_ff, p, eps); params: the 12 tensors in header order; masks: dict(att, d1, ffn, d2)
    of bool arrays or None (nothing dropped).  Returns dict(h_out, x1, pre) and, with dh_out, grads (12 arrays) and dh_in."""
    dt = dtype
    T, B, Z, H, F = cfg["T"], cfg["B"], cfg["Z"], cfg["H"], cfg["d_ff"]
    M = T * B
    in_w, in_b, out_w, out_b, w1, b1, w2, b2, g1, be1, g2, be2 = (np.asarray(t).astype(dt) for t in params)
    ik = dt(inv_keep(cfg["p"], dt))
    one = lambda shape: np.ones(shape, dt)
    if masks is None:
        m_att, m1, mf, m2 = None, one((M, Z)), one((M, F)), one((M, Z))
    else:
        m_att, m1, mf, m2 = masks["att"], masks["d1"].astype(dt), masks["ffn"].astype(dt), masks["d2"].astype(dt)
    if "streams_swapped" in wrong:
        m1, m2 = m2, m1
    h = np.asarray(h_in).astype(dt).reshape(M, Z)
    qkv = h @ in_w.T + in_b
    att = attention_ref(qkv, lengths, T, B, Z, H, m_att, ik, None, dt, wrong)
    ctx = att[0].reshape(M, Z)
    a = ctx @ out_w.T + out_b
    s1, x1, mean1, rstd1 = layernorm_ref(h, a * m1 * ik, g1, be1, cfg["eps"], dt, wrong)
    pre = x1 @ w1.T + b1
    hid = np.maximum(pre, dt(0)) * mf * ik
    f = hid @ w2.T + b2
    s2, h_out, mean2, rstd2 = layernorm_ref(x1, f * m2 * ik, g2, be2, cfg["eps"], dt, wrong)
    out = dict(h_out=h_out, x1=x1, pre=pre)
    if dh_out is None:
        return out
    dy = np.asarray(dh_out).astype(dt).reshape(M, Z)
    ds2, dg2, dbe2 = layernorm_bwd_ref(dy, s2, g2, mean2, rstd2, dt, wrong)[:3]
    df = ds2 * m2 * ik
    db2, dw2 = df.sum(0, dtype=dt), df.T @ hid
    dpre = (df @ w2) * (pre > 0) * mf * ik
    dw1, db1 = dpre.T @ x1, dpre.sum(0, dtype=dt)
    dx1 = dpre @ w1 + ds2
    ds1, dg1, dbe1 = layernorm_bwd_ref(dx1, s1, g1, mean1, rstd1, dt, wrong)[:3]
    da = ds1 * m1 * ik
    dob, dow = da.sum(0, dtype=dt), da.T @ ctx
    dqkv = attention_ref(qkv, lengths, T, B, Z, H, m_att, ik, (da @ out_w).reshape(T, B, Z), dt, wrong)[2].reshape(M, 3 * Z)
    dinw, dinb = dqkv.T @ h, dqkv.sum(0, dtype=dt)
    out["dh_in"] = (dqkv @ in_w + ds1).astype(dt)
    out["grads"] = [g.astype(dt) for g in (dinw, dinb, dow, dob, dw1, db1, dw2, db2, dg1, dbe1, dg2, dbe2)]
    return out


def stack_ref(cfg, n_layers, params, h0, lengths, masks=None, dh_out=None, dtype=F64, wrong=()):
    """layer_ref chained: params 12 per layer, masks one dict per layer (or None).  Returns dict(h_out, layers: the per-layer
    forward dicts) and, with dh_out, grads (12 per layer) and dh_in."""
    if masks is not None and "layer1_uses_layer0_streams" in wrong:
        masks = [masks[0]] * n_layers
    h, fw = h0, []
    for li in range(n_layers):
        fw.append(layer_ref(cfg, params[12 * li:12 * li + 12], h, lengths, masks and masks[li], None, dtype, wrong))
        h = fw[-1]["h_out"]
    out = dict(h_out=h, layers=fw)
    if dh_out is None:
        return out
    g, grads = dh_out, [None] * (12 * n_layers)
    for li in reversed(range(n_layers)):
        r = layer_ref(cfg, params[12 * li:12 * li + 12], h0 if li == 0 else fw[li - 1]["h_out"], lengths, masks and masks[li], g,
                      dtype, wrong)
        grads[12 * li:12 * li + 12] = r["grads"]
        g = r["dh_in"]
    out["grads"], out["dh_in"] = grads, g
    return out


def kink_margin(fw, params):
    """min over the FFN units of |pre| / (sum_k |x1_k w1_fk| + |b1_f|) of a float64 layer forward."""
    w1, b1 = np.asarray(params[4], F64), np.asarray(params[5], F64)
    S = np.abs(fw["x1"]) @ np.abs(w1).T + np.abs(b1)
    return float((np.abs(fw["pre"]) / S).min())


# ---------------------------------------------------------------------------------------------------------------------------- #
# case tables (tests/test_encoder_kernels_gpu.py runs exactly these)
# ---------------------------------------------------------------------------------------------------------------------------- #
ELEMENT_COUNTS = (1, 255, 256, 257, 70001)
POS_SHAPES = ((1, 1, 1), (5, 3, 20), (128, 2, 33))
POS_GRAD_SHAPES = POS_SHAPES + ((50, 32, 40),)
COLSUM_M, COLSUM_N = (1, 15, 16, 17, 300), (1, 63, 64, 65, 130)
LN_M, LN_N = (1, 3, 4, 5, 135), (1, 20, 63, 64, 65, 300, 320)
# (M, N, row scale): the LN_M x LN_N grid at unit scale plus one case of small rows (variance 1e-4: eps = 1e-5 matters there)
LN_CASES = [(m, n, 1.0) for m in LN_M for n in LN_N] + [(5, 64, 1e-2)]

# id, T, B, Z, H, lengths, p, mask seed, scale of q and k
ATT_CASES = [
    dict(id="dh4_g16", T=7, B=3, Z=20, H=5, lengths=[7, 4, 1], p=0.1, seed=101, qk=1.0),
    dict(id="dh8_mosei", T=50, B=2, Z=40, H=5, lengths=[50, 23], p=0.1, seed=102, qk=1.0),
    dict(id="dh5_second_pass", T=65, B=2, Z=15, H=3, lengths=[65, 64], p=0.1, seed=103, qk=1.0),
    dict(id="dh33_one_group", T=9, B=2, Z=66, H=2, lengths=[9, 5], p=0.3, seed=104, qk=1.0),
    dict(id="envelope", T=128, B=1, Z=64, H=1, lengths=None, p=0.25, seed=105, qk=1.0),
    dict(id="t1", T=1, B=3, Z=6, H=2, lengths=None, p=0.5, seed=106, qk=1.0),
    dict(id="sharp", T=7, B=3, Z=20, H=5, lengths=[7, 4, 1], p=0.0, seed=107, qk=3.9),     # scores reach about +-30
]
MASK_PROBE = dict(id="mask_probe", T=33, B=2, Z=66, H=2, lengths=[33, 20], p=0.3, seed=108)

# `seeds`: data seeds whose float64 reference has no relu kink at p = 0 and at p (the GPU test uses the first, the level
# measurement all four); `seed`: base of the dropout streams
LAYER_CASES = [
    dict(id="dff2048_32slabs", T=7, B=3, Z=20, H=5, d_ff=2048, lengths=[7, 4, 1], p=0.1, eps=EPS, seed=201, seeds=(53, 66, 88, 114)),
    dict(id="m135_three_chunks", T=9, B=15, Z=130, H=5, d_ff=200, lengths=[9] + [i % 9 + 1 for i in range(14)], p=0.1, eps=EPS, seed=202,
         seeds=(15, 64, 163, 302)),
    dict(id="m300_five_chunks", T=50, B=6, Z=40, H=5, d_ff=96, lengths=None, p=0.3, eps=EPS, seed=203, seeds=(24, 40, 44, 100)),
]
STACK_CASE = dict(id="stack2", T=7, B=3, Z=20, H=5, d_ff=64, lengths=[7, 4, 1], p=0.1, eps=EPS, seed=301, n_layers=2, seeds=(0, 1, 2, 3))


# ---------------------------------------------------------------------------------------------------------------------------- #
# case data (deterministic in the case id and the data seed)
# ---------------------------------------------------------------------------------------------------------------------------- #
def _rng(tag, data_seed):
    return np.random.default_rng([sum(ord(ch) for ch in tag) * 7919 + len(tag), int(data_seed)])


def build_attention(c, data_seed=0):
    """(qkv [T,B,3Z], dctx [T,B,Z]) fp32; q and k scaled by c['qk']."""
    rng = _rng(c["id"], data_seed)
    T, B, Z = c["T"], c["B"], c["Z"]
    qkv = rng.standard_normal((T, B, 3 * Z))
    qkv[..., :2 * Z] *= c.get("qk", 1.0)
    return qkv.astype(F32), rng.standard_normal((T, B, Z)).astype(F32)


def build_layernorm(M, N, scale, data_seed=0):
    """x, r, gamma (0.5 .. 1.5 in magnitude, both signs), beta (|beta| >= 0.25), dy: fp32."""
    rng = _rng(f"ln_{M}_{N}_{scale}", data_seed)
    x = scale * (rng.standard_normal((M, N)) + 0.3)
    r = scale * rng.standard_normal((M, N))
    gamma = rng.uniform(0.5, 1.5, N) * rng.choice([-1.0, 1.0], N)
    beta = rng.uniform(0.25, 1.0, N) * rng.choice([-1.0, 1.0], N)
    return tuple(a.astype(F32) for a in (x, r, gamma, beta, rng.standard_normal((M, N))))


def build_layer(c, data_seed, n_layers=1):
    """(params: 12 per layer, h_in [M,Z], dh_out [M,Z]) fp32: weights N(0, 1/fan_in), biases 0.1 N(0,1), norm weights in
    0.5 .. 1.5, norm biases 0.3 N(0,1), unit-normal rows."""
    rng = _rng(c["id"], data_seed)
    Z, F, M = c["Z"], c["d_ff"], c["T"] * c["B"]
    params = []
    for _ in range(n_layers):
        for i, shp in enumerate(param_shapes(Z, F)):
            if i in (0, 2, 4, 6):
                t = rng.standard_normal(shp) / np.sqrt(shp[1])
            elif i in (8, 10):
                t = rng.uniform(0.5, 1.5, shp)
            else:
                t = (0.3 if i in (9, 11) else 0.1) * rng.standard_normal(shp)
            params.append(t.astype(F32))
    return params, rng.standard_normal((M, Z)).astype(F32), rng.standard_normal((M, Z)).astype(F32)


def stack_masks(c, p, mask_fn=keep_mask):
    return [layer_masks(dict(c, p=p), c["seed"] + STACK_SEED_STRIDE * li, mask_fn) for li in range(c["n_layers"])]


def layer_outputs(r, n_layers=1):
    """name -> array of a layer_ref / stack_ref result with gradients: h_out, dh_in and the 12 gradients (a stack's are
    concatenated over its layers: one bound per parameter kind)."""
    out = dict(h_out=r["h_out"], dh_in=r["dh_in"])
    for i, n in enumerate(PARAM_NAMES):
        out["d_" + n] = np.concatenate([r["grads"][12 * li + i].ravel() for li in range(n_layers)])
    return out


def runs_of(c):
    """The dropout rates a case runs at: 0 and the listed p."""
    return (0.0,) if c["p"] == 0 else (0.0, c["p"])


def layer_eval(c, p, data_seed, dtype=F64, wrong=(), mask_fn=keep_mask):
    """One run of a layer or stack case: (outputs by name, the per-layer forward dicts, params)."""
    n = c.get("n_layers", 1)
    params, h_in, dh_out = build_layer(c, data_seed, n)
    cfg = dict(c, p=p)
    if n == 1 and "n_layers" not in c:
        masks = layer_masks(cfg, c["seed"], mask_fn) if p > 0 else None
        r = layer_ref(cfg, params, h_in, c["lengths"], masks, dh_out, dtype, wrong)
        return layer_outputs(r), [r], params
    masks = stack_masks(c, p, mask_fn) if p > 0 else None
    r = stack_ref(cfg, n, params, h_in, c["lengths"], masks, dh_out, dtype, wrong)
    return layer_outputs(r, n), r["layers"], params


def case_kink_margin(c, data_seed):
    """The smallest |pre| / S over every FFN unit of every layer and both runs of a layer / stack case (float64)."""
    m = np.inf
    for p in runs_of(c):
        _, fws, params = layer_eval(c, p, data_seed)
        for li, fw in enumerate(fws):
            m = min(m, kink_margin(fw, params[12 * li:12 * li + 12]))
    return m


def attention_eval(c, p, data_seed, dtype=F64, wrong=(), mask_fn=keep_mask):
    qkv, dctx = build_attention(c, data_seed)
    T, B, Z, H = c["T"], c["B"], c["Z"], c["H"]
    keep = mask_fn(c["seed"], B * H * T * T, p).reshape(B, H, T, T) if p > 0 else None
    ctx, lse, dqkv = attention_ref(qkv, c["lengths"], T, B, Z, H, keep, inv_keep(p, dtype), dctx, dtype, wrong)
    return dict(ctx=ctx, lse=lse, dqkv=dqkv)


def att_family(c):
    """The sharp-softmax case is a family of its own: at scores of +-30 the backward's exp(s - lse) carries the rounding of s and
    lse (module docstring), a level the other cases must not inherit."""
    return "attention_sharp" if c["id"] == "sharp" else "attention"


def layernorm_eval(M, N, scale, with_r, data_seed, dtype=F64, wrong=()):
    """Forward, then the backward on the float64 forward's mean / rstd rounded to fp32 (the inputs the GPU test passes)."""
    x, r, gamma, beta, dy = build_layernorm(M, N, scale, data_seed)
    s, y, mean, rstd = layernorm_ref(x, r if with_r else None, gamma, beta, EPS, dtype, wrong)
    s64, _, mean64, rstd64 = layernorm_ref(x, r if with_r else None, gamma, beta, EPS, F64)
    with np.errstate(over="ignore"):
        s32, mean32, rstd32 = s64.astype(F32), mean64.astype(F32), rstd64.astype(F32)
    ds, dg, db, Sg, Sb = layernorm_bwd_ref(dy, s32, gamma, mean32, rstd32, dtype, wrong)
    return dict(y=y, mean=mean, rstd=rstd, ds=ds), dict(dgamma=(dg, Sg), dbeta=(db, Sb))


# ---------------------------------------------------------------------------------------------------------------------------- #
# levels of the fp32 evaluation and the bounds derived from them
# ---------------------------------------------------------------------------------------------------------------------------- #
DATA_SEEDS = (0, 1, 2, 3)

# log2 of the measured levels (rounded up to 0.1), the table of the module docstring
LEVELS_LOG2 = {
    "attention": {"ctx": -21.7, "lse": -23.2, "dqkv": -20.2},
    "attention_sharp": {"ctx": -21.6, "lse": -23.6, "dqkv": -17.7},
    "layernorm": {"y": -22.2, "mean": -20.0, "rstd": -22.5, "ds": -22.5},
    "layer": {"h_out": -20.7, "dh_in": -20.6, "d_in_w": -19.8, "d_in_b": -20.1, "d_out_w": -20.2, "d_out_b": -20.9,
        "d_w1": -21.1, "d_b1": -20.9, "d_w2": -20.6, "d_b2": -21.1, "d_g1": -20.2, "d_be1": -19.9, "d_g2": -20.3,
        "d_be2": -20.9},
    "stack": {"h_out": -21.5, "dh_in": -21.1, "d_in_w": -21.4, "d_in_b": -21.5, "d_out_w": -21.1, "d_out_b": -21.0,
        "d_w1": -21.3, "d_b1": -21.4, "d_w2": -21.5, "d_b2": -22.2, "d_g1": -21.1, "d_be1": -21.3, "d_g2": -21.4,
        "d_be2": -21.6},
}


def measure_levels():
    """family -> output -> largest comp_err of the fp32 evaluation against float64 over every case, both runs, four data seeds."""
    lv = {}

    def note(fam, got, ref):
        for k in ref:
            lv.setdefault(fam, {})[k] = max(lv.get(fam, {}).get(k, 0.0), comp_err(got[k], ref[k]))
    for c in ATT_CASES:
        for p in runs_of(c):
            for ds in DATA_SEEDS:
                note(att_family(c), attention_eval(c, p, ds, F32), attention_eval(c, p, ds))
    for M, N, scale in LN_CASES:
        for with_r in (False, True):
            for ds in DATA_SEEDS:
                note("layernorm", layernorm_eval(M, N, scale, with_r, ds, F32)[0], layernorm_eval(M, N, scale, with_r, ds)[0])
    for fam, cases in (("layer", LAYER_CASES), ("stack", [STACK_CASE])):
        for c in cases:
            for p in runs_of(c):
                for ds in c["seeds"]:
                    note(fam, layer_eval(c, p, ds, F32)[0], layer_eval(c, p, ds)[0])
    return lv


def bound_of(level_log2):
    """8 x the level, rounded up to a power of two."""
    return 2.0 ** int(np.ceil(level_log2 + 3.0 - 1e-9))


BOUNDS = {fam: {k: bound_of(v) for k, v in d.items()} for fam, d in LEVELS_LOG2.items()}


def variant_excess(name):
    """The largest error / bound of the float64 wrong variant `name` against the float64 reference, over the cases of its family
    (must be >= 8: the criterion rejects the variant).  Non-finite outputs of a variant (an all-dropped row under l_kept_only,
    N = 1 without eps) are left out: it has to break its bound through finite values."""
    w, worst = (name,), 0.0

    fin = lambda got, ref: np.where(np.isfinite(got), got, ref)     # (a variant has to break its bound through finite values)

    def note(fam, got, ref):
        nonlocal worst
        for k in ref:
            worst = max(worst, comp_err(fin(got[k], ref[k]), ref[k]) / BOUNDS[fam][k])
    if name in ("mask_transposed", "l_kept_only", "dv_no_inv_keep", "dS_dropped", "pad_off_by_one"):
        for c in ATT_CASES:
            for p in runs_of(c):
                note(att_family(c), attention_eval(c, p, 0, F64, w), attention_eval(c, p, 0))
    elif name == "streams_swapped":
        for c in LAYER_CASES:
            note("layer", layer_eval(c, c["p"], c["seeds"][0], F64, w)[0], layer_eval(c, c["p"], c["seeds"][0])[0])
    elif name == "layer1_uses_layer0_streams":
        c = STACK_CASE
        note("stack", layer_eval(c, c["p"], c["seeds"][0], F64, w)[0], layer_eval(c, c["p"], c["seeds"][0])[0])
    elif name in ("ln_no_eps", "dgamma_no_rstd"):
        for M, N, scale in LN_CASES:
            got, gsum = layernorm_eval(M, N, scale, True, 0, F64, w)
            ref, rsum = layernorm_eval(M, N, scale, True, 0)
            note("layernorm", got, ref)
            for k in rsum:
                worst = max(worst, gemm_err(fin(gsum[k][0], rsum[k][0]), rsum[k][0], rsum[k][1])[0] / CRIT_MAX)
    else:
        raise KeyError(name)
    return worst
