"""The contract of umlh_ae_forward and umlh_ae_train_steps (include/umlh.h) restated in numpy: the float64
statement of the SharedAutoencoder's forward and of one training step (gradients of all 16 tensors in both modes, then
_optstep_ref.opt_ref for the update), an honest fp32 restatement of the same formulas, the case table of
tests/test_gauss_kernels_gpu.py, the bounds calibrated on it and a set of deliberately wrong variants that the bounds must reject.
No GPU, no `umlh` import.

Model.  16 tensors in state_dict order (NAMES).  Per view v, row r:  a0 = table_v[idx_v[r]];  a1 = W_in_v a0 + b;
a2 = relu(W_e0 a1 + b);  a3 = W_e2 a2 + b (the embedding);  a4 = relu(W_d0 a3 + b);  a5 = W_d2 a4 + b;  rec = W_out_v a5 + b;
loss_v = mean over rows_v * D of (rec - a0)^2.  Mode 'xy': dRec_v = alpha_v * 2 / (rows_v * D) * (rec - a0),
loss = alpha_x loss_x + alpha_y loss_y.  Mode 'x': the y view has no backward, in_head_y / out_head_y receive nothing (None),
loss = loss_x.

fp32 restatement (dt = F32).  Every product is a sequential fp32 fma chain in the kernels' documented order: blocks of 16 k
ascending, inside a block k0 + 4 g + i for i = 0..3 (outer), g = 0..3 (inner); the bias one fp32 add behind it; relu masks from
the fp32 activations; the residual scaled by the fp32 factor; squares and sums of the loss in float64, rounded once.  A weight
gradient is four chains (wave w: the 4-row blocks w, w + 4, ... of x, then of y) added in wave order; a bias gradient 16 plain
fp32 sums (wave w, lane group g: rows 4 blk + g of those blocks) added in the order 4 w + g.

Error measures.  losses: |got - ref| / |ref|.  rec, emb and every gradient: max |got - ref| / max |ref| per tensor (a gradient
tensor that the reference leaves untouched must be absent or all zero).  Every bound is 8 x the largest error of the fp32
restatement against float64 over SEEDS x both modes (alpha = (1, 0.5)), rounded up to a power of two: case by case for the
tensors (LEVELS_LOG2 holds the 10 x 13 levels; a gradient's level ranges from 2^-24 at (1, 1, 1, 1, 1) to 2^-15 at
(17, 15, 4, 17, 1), where one relu unit of four with a small pre-activation carries a visible share of 18 rows' gradient, so one
bound for all cases would be set by that case), over the whole table for the three losses (one number per sample: LOSS_LEVELS_LOG2).
The largest level of each output over the table, log2 (tests/test_gauss_ref_cpu.py re-measures all of them):

        loss_x -22.2   loss_y -23.9   loss -22.2   rec -20.3   emb -20.5   out_head.weight -20.6   out_head.bias -21.9
        in_head, encoder, decoder (weight and bias): -15.0 at (17, 15, 4, 17, 1); -19.4 .. -24.3 elsewhere

    (in_head: in_head_x / in_head_y; encoder: shared_encoder.0 / .2; decoder: shared_decoder.0 / .2; out_head: out_head_x / _y.)
A gradient's error is NOT divided by the sum of the magnitudes of all the terms it expands into (the GEMM measure carried through
the chain): that sum grows with the widths (10^5 .. 10^10 times the gradient at the paper's widths and above) and a zero gradient
would pass there.

Relu kinks.  A unit whose pre-activation is within rounding of 0 can switch between two fp32 implementations and the gradients
then differ by a discrete amount.  build_case makes its data kink-free by construction: after the seeded draw, the bias of every
relu unit that has a row with |pre| <= 2^-16 * (sum_k |a_k w_k| + |b|) in the float64 forward is re-drawn from the same generator
(with a fourfold margin, for the indexed and the un-indexed rows) until none is left (random data would leave about eight such units in the L = 500 case, so seeds alone cannot be searched for).
The data is a function of (case, seed) alone; kink_margin returns the smallest ratio and the CPU test asserts it is > 2^-16 for
every case and seed, so no kink allowance is needed.
"""
import numpy as np

from _optstep_ref import opt_ref

F32, F64 = np.float32, np.float64
KINK = 2.0 ** -16
NAMES = ("in_head_x.weight", "in_head_x.bias", "in_head_y.weight", "in_head_y.bias", "shared_encoder.0.weight", "shared_encoder.0.bias",
         "shared_encoder.2.weight", "shared_encoder.2.bias", "shared_decoder.0.weight", "shared_decoder.0.bias",
         "shared_decoder.2.weight", "shared_decoder.2.bias", "out_head_x.weight", "out_head_x.bias", "out_head_y.weight",
         "out_head_y.bias")
GROUP = ("in_head", "in_head", "in_head", "in_head", "encoder", "encoder", "encoder", "encoder", "decoder", "decoder", "decoder",
         "decoder", "out_head", "out_head", "out_head", "out_head")
SEEDS = (0, 1, 2, 3)
ALPHA = (1.0, 0.5)
# (D, C, L, rows_x, rows_y): 16-row tile edges 1, 15, 16, 17, 33, 130; MFMA tile and k-block edges 1, 3, 4, 5, 15, 16, 17, 50, 100, 128, 257, 500
CASES = ((50, 128, 10, 130, 130), (1, 1, 1, 1, 1), (5, 17, 3, 15, 33), (16, 16, 16, 16, 16), (17, 15, 4, 17, 1), (100, 128, 100, 33, 16),
         (50, 257, 5, 16, 17), (50, 128, 500, 17, 15), (33, 64, 128, 130, 0), (33, 64, 128, 0, 130))


def case_id(c):
    return "D%d_C%d_L%d_x%d_y%d" % tuple(c)


def tensor_shapes(D, C, L):
    return [(C, D), (C,), (C, D), (C,), (L, C), (L,), (L, L), (L,), (L, L), (L,), (C, L), (C,), (D, C), (D,), (D, C), (D,)]


def group_key(k):
    return GROUP[k] + (".weight" if k % 2 == 0 else ".bias")


# ---------------------------------------------------------------------------------------------------------------------------- #
# products
# ---------------------------------------------------------------------------------------------------------------------------- #
def k_order(K):
    """The order in which a product of the row kernel adds its K terms."""
    out = []
    for k0 in range(0, K, 16):
        out += [k0 + 4 * g + i for i in range(4) for g in range(4) if k0 + 4 * g + i < K]
    return out


def _fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def mm(a, w, dt):
    """a [rows, K] . w [N, K]^T in float64, or as the fp32 fma chain of the kernels."""
    if dt == F64:
        return a @ w.T
    acc = np.zeros((a.shape[0], w.shape[0]), F32)
    for k in k_order(a.shape[1]):
        acc = _fma(a[:, k:k + 1], w[:, k][None, :], acc)
    return acc


def grad_w(dzs, acts, dt):
    """(dW [N, K], db [N]) over the views' rows: dzs / acts are lists of [rows_v, N] / [rows_v, K] blocks, x first."""
    N, K = dzs[0].shape[1], acts[0].shape[1]
    if dt == F64:
        return sum(dz.T @ a for dz, a in zip(dzs, acts)), sum(dz.sum(0) for dz in dzs)
    parts, bparts = [], []
    for w in range(4):
        acc = np.zeros((N, K), F32)
        bs = np.zeros((4, N), F32)
        for dz, a in zip(dzs, acts):
            rows = dz.shape[0]
            for blk in range(w, (rows + 3) // 4, 4):
                for g in range(4):
                    r = 4 * blk + g
                    if r < rows:
                        acc = _fma(dz[r][:, None], a[r][None, :], acc)
                        bs[g] = bs[g] + dz[r]
        parts.append(acc)
        bparts += [bs[g] for g in range(4)]
    dW = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    db = bparts[0]
    for p in bparts[1:]:
        db = db + p
    return dW, db


# ---------------------------------------------------------------------------------------------------------------------------- #
# the model
# ---------------------------------------------------------------------------------------------------------------------------- #
def view_forward(P, a0, v, dt=F64):
    """The activations of one view: dict a0 .. a5, rec, res, pre2, pre4 (the relu layers' pre-activations), S2, S4 (their
    term-magnitude sums, float64 only)."""
    P = [np.asarray(p, dt) for p in P]
    a0 = np.asarray(a0, dt)
    w_in, b_in, w_out, b_out = P[2 * v], P[2 * v + 1], P[12 + 2 * v], P[13 + 2 * v]
    f = {"a0": a0}
    f["a1"] = mm(a0, w_in, dt) + b_in
    f["pre2"] = mm(f["a1"], P[4], dt) + P[5]
    f["a2"] = np.maximum(f["pre2"], 0)
    f["a3"] = mm(f["a2"], P[6], dt) + P[7]
    f["pre4"] = mm(f["a3"], P[8], dt) + P[9]
    f["a4"] = np.maximum(f["pre4"], 0)
    f["a5"] = mm(f["a4"], P[10], dt) + P[11]
    f["rec"] = mm(f["a5"], w_out, dt) + b_out
    f["res"] = f["rec"] - a0
    if dt == F64:
        f["S2"] = np.abs(f["a1"]) @ np.abs(P[4]).T + np.abs(P[5])
        f["S4"] = np.abs(f["a3"]) @ np.abs(P[8]).T + np.abs(P[9])
    return f


def loss_of(res, dt):
    """mean of the squared residuals: float64, rounded once to fp32 in the fp32 restatement."""
    if res.size == 0:
        return dt(0.0)
    s = (res.astype(F64) ** 2).sum() / res.size
    return F32(s) if dt == F32 else s


def kink_margin(P, ax, ay):
    """The smallest |pre| / (sum_k |a_k w_k| + |b|) over both relu layers, both views and every row (float64)."""
    m = np.inf
    for v, a0 in enumerate((ax, ay)):
        if a0 is None or len(a0) == 0:
            continue
        f = view_forward(P, a0, v)
        for pre, S in ((f["pre2"], f["S2"]), (f["pre4"], f["S4"])):
            m = min(m, float((np.abs(pre) / S).min()))
    return m


def step_grads(P, ax, ay, mode="xy", alpha=ALPHA, dt=F64, wrong=()):
    """One step's forward and backward.  ax / ay: the gathered rows [rows_v, D] (None or 0 rows: view absent).  Returns a dict:
    losses (loss_x, loss_y, loss), grads [16] (None: the tensor is not touched), rec / emb per view."""
    D = np.asarray(P[0]).shape[1]
    views = [None if a is None or len(a) == 0 else np.asarray(a, dt) for a in (ax, ay)]
    fw = [None if a is None else view_forward(P, a, v, dt) for v, a in enumerate(views)]
    Pd = [np.asarray(p, dt) for p in P]
    lv = [dt(0.0) if f is None else loss_of(f["res"], dt) for f in fw]
    if "mean_over_rows" in wrong:
        lv = [l * D for l in lv]
    if mode == "xy":
        al = [dt(a) for a in alpha]
        loss = al[0] * lv[0] + al[1] * lv[1]
        loss = dt(loss)
    else:
        loss = lv[0]
    back = [fw[0] is not None, fw[1] is not None and (mode == "xy")]
    bw = [None, None]
    for v in range(2):
        if not back[v]:
            continue
        f = fw[v]
        rows = f["a0"].shape[0]
        a_v = alpha[v]
        if "alpha_y_on_x" in wrong:
            a_v = alpha[1]
        scale = a_v * 2.0 / (rows * (1 if "mean_over_rows" in wrong else D))
        scale = F32(scale) if dt == F32 else scale
        m4, m2 = f["a4"] > 0, f["a2"] > 0
        if "relu_mask_other" in wrong:
            m4, m2 = f["a2"] > 0, f["a4"] > 0
        z = {}
        z[6] = (scale * f["res"]).astype(dt)
        z[5] = mm(z[6], Pd[12 + 2 * v].T, dt)
        z[4] = np.where(m4, mm(z[5], Pd[10].T, dt), dt(0))
        z[3] = mm(z[4], Pd[8].T, dt)
        z[2] = np.where(m2, mm(z[3], Pd[6].T, dt), dt(0))
        z[1] = mm(z[2], Pd[4].T, dt)
        bw[v] = z
    grads = [None] * 16
    feeds = ((0, 1, "a0", 0), (2, 1, "a0", 1), (4, 2, "a1", -1), (6, 3, "a2", -1), (8, 4, "a3", -1), (10, 5, "a4", -1),
             (12, 6, "a5", 0), (14, 6, "a5", 1))
    for k, zi, an, view in feeds:
        vs = [v for v in range(2) if back[v] and (view < 0 or view == v)]
        if view < 0 and "no_y_in_shared" in wrong:
            vs = [v for v in vs if v == 0]
        if view < 0 and "x_twice" in wrong and back[0]:
            vs = [0, 0]
        if not vs:
            continue
        dzs, acts = [bw[v][zi] for v in vs], [fw[v][an] for v in vs]
        dW, db = grad_w(dzs, acts, dt)
        if "db_drop_tail" in wrong:
            db = sum(dz[:(dz.shape[0] // 16) * 16].sum(0) for dz in dzs)
        grads[k], grads[k + 1] = dW, db
    if mode == "x" and "in_head_y_stepped" in wrong and fw[1] is not None:
        # the y view's backward run although the mode has none: its in head receives a gradient
        g = step_grads(P, ax, ay, "xy", alpha, dt)
        grads[2], grads[3] = g["grads"][2], g["grads"][3]
    return dict(losses=(lv[0], lv[1], loss), grads=grads, rec=[None if f is None else f["rec"] for f in fw],
                emb=[None if f is None else f["a3"] for f in fw])


def apply_update(kind, P, grads, M, V, lr, step, wd=0.0, wrong=()):
    """(P, M, V) after the update, float64 lists; a tensor without a gradient stays as it is."""
    out = ([], [], [])
    for k in range(16):
        if grads[k] is None:
            p, m, v = (np.asarray(a, F64) for a in (P[k], M[k], V[k]))
        else:
            p, m, v = opt_ref(kind, P[k], grads[k], M[k], V[k], lr, step, wd=wd, wrong=wrong)
        for o, a in zip(out, (p, m, v)):
            o.append(a)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- #
# data
# ---------------------------------------------------------------------------------------------------------------------------- #
def build_case(case, seed):
    """fp32 parameters (nn.Linear's uniform(-1/sqrt(K), 1/sqrt(K))), two tables [rows + 5, D + 3] of standard normal rows (row
    stride ld = D + 3) and int32 row ids with repeats, kink-free by construction (module docstring)."""
    D, C, L, rx, ry = case
    rng = np.random.default_rng([sum(ord(ch) for ch in "gauss"), int(seed), D, C, L, rx, ry])
    fan =[D, D, D, D, C, C, L, L, L, L, L, L, C, C, C, C]
    P = [rng.uniform(-1.0, 1.0, shp).astype(F64) / np.sqrt(fan[k]) for k, shp in enumerate(tensor_shapes(D, C, L))]
    P = [p.astype(F32) for p in P]
    ld = D + 3
    tabs, idxs = [], []
    for rows in (rx, ry):
        n = rows + 5
        t = rng.standard_normal((n, ld)).astype(F32)
        idx = rng.integers(0, n, rows).astype(np.int32)
        if rows > 2:
            idx[1] = idx[0]                                             # a repeated row
        tabs.append(t)
        idxs.append(idx)
    c = dict(case=case, seed=seed, P=P, tables=tabs, idx=idxs, ld=ld, D=D, C=C, L=L, rows=(rx, ry))
    for _ in range(200):
        bad = [sorted(set(i) | set(u)) for i, u in zip(_kink_units(P, *gathered(c)), _kink_units(P, *gathered(c, False)))]
        if not any(len(b) for b in bad):
            return c
        for k, units in zip((5, 9), bad):
            for u in units:
                P[k][u] = F32(rng.uniform(-1.0, 1.0) / np.sqrt(fan[k]))
    raise RuntimeError(f"build_case{case} seed {seed}: relu units within the kink margin are left after 200 rounds of re-draws")


def _kink_units(P, ax, ay):
    bad = [set(), set()]
    for v, a0 in enumerate((ax, ay)):
        if a0 is None or len(a0) == 0:
            continue
        f = view_forward(P, a0, v)
        for j, (pre, S) in enumerate(((f["pre2"], f["S2"]), (f["pre4"], f["S4"]))):
            bad[j] |= set(np.nonzero((np.abs(pre) <= 4 * KINK * S).any(0))[0].tolist())
    return [sorted(b) for b in bad]


def gathered(c, indexed=True):
    """(ax, ay): the rows of each view [rows_v, D] fp32 (None for an absent view); indexed=False: rows 0 .. rows - 1."""
    out = []
    for v in range(2):
        rows = c["rows"][v]
        if rows == 0:
            out.append(None)
            continue
        ids = c["idx"][v] if indexed else np.arange(rows)
        out.append(c["tables"][v][ids][:, :c["D"]])
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------- #
# error measures, levels, bounds
# ---------------------------------------------------------------------------------------------------------------------------- #
OUTPUTS = ("loss_x", "loss_y", "loss", "rec", "emb") + tuple(sorted({group_key(k) for k in range(16)}))

# log2 of the measured levels per case, rounded up to 0.1; None: the fp32 restatement is exact there (an absent view's loss)
LEVELS_LOG2 = {
    (50, 128, 10, 130, 130): {"loss_x": -25.0, "loss_y": -24.4, "loss": -23.7, "rec": -20.7, "emb": -21.7, "decoder.bias": -21.2, "decoder.weight": -21.1, "encoder.bias": -21.6, "encoder.weight": -20.9, "in_head.bias": -21.6, "in_head.weight": -21.5, "out_head.bias": -22.3, "out_head.weight": -22.2},
    (1, 1, 1, 1, 1): {"loss_x": -22.2, "loss_y": -23.9, "loss": -22.2, "rec": -22.5, "emb": -24.1, "decoder.bias": -22.7, "decoder.weight": -22.6, "encoder.bias": -22.5, "encoder.weight": -21.9, "in_head.bias": -23.8, "in_head.weight": -23.7, "out_head.bias": -23.5, "out_head.weight": -23.4},
    (5, 17, 3, 15, 33): {"loss_x": -26.3, "loss_y": -23.9, "loss": -24.7, "rec": -21.9, "emb": -22.5, "decoder.bias": -19.9, "decoder.weight": -22.0, "encoder.bias": -19.3, "encoder.weight": -22.2, "in_head.bias": -22.4, "in_head.weight": -22.4, "out_head.bias": -22.8, "out_head.weight": -22.9},
    (16, 16, 16, 16, 16): {"loss_x": -24.0, "loss_y": -24.8, "loss": -24.0, "rec": -22.7, "emb": -22.6, "decoder.bias": -22.0, "decoder.weight": -21.9, "encoder.bias": -20.3, "encoder.weight": -21.5, "in_head.bias": -21.1, "in_head.weight": -22.1, "out_head.bias": -22.5, "out_head.weight": -22.9},
    (17, 15, 4, 17, 1): {"loss_x": -25.0, "loss_y": -24.1, "loss": -24.1, "rec": -22.7, "emb": -23.0, "decoder.bias": -15.0, "decoder.weight": -15.0, "encoder.bias": -15.0, "encoder.weight": -15.0, "in_head.bias": -15.0, "in_head.weight": -15.0, "out_head.bias": -22.4, "out_head.weight": -23.0},
    (100, 128, 100, 33, 16): {"loss_x": -25.3, "loss_y": -24.6, "loss": -23.8, "rec": -21.4, "emb": -21.1, "decoder.bias": -21.2, "decoder.weight": -20.4, "encoder.bias": -20.8, "encoder.weight": -20.6, "in_head.bias": -20.9, "in_head.weight": -21.1, "out_head.bias": -22.7, "out_head.weight": -21.6},
    (50, 257, 5, 16, 17): {"loss_x": -24.5, "loss_y": -24.0, "loss": -23.6, "rec": -20.3, "emb": -21.3, "decoder.bias": -20.7, "decoder.weight": -20.4, "encoder.bias": -21.2, "encoder.weight": -20.7, "in_head.bias": -20.9, "in_head.weight": -20.3, "out_head.bias": -22.4, "out_head.weight": -22.6},
    (50, 128, 500, 17, 15): {"loss_x": -24.4, "loss_y": -24.2, "loss": -24.3, "rec": -20.8, "emb": -20.5, "decoder.bias": -20.9, "decoder.weight": -20.6, "encoder.bias": -19.8, "encoder.weight": -20.2, "in_head.bias": -19.9, "in_head.weight": -20.3, "out_head.bias": -22.4, "out_head.weight": -20.6},
    (33, 64, 128, 130, 0): {"loss_x": -24.6, "loss_y": None, "loss": -24.6, "rec": -21.8, "emb": -21.5, "decoder.bias": -22.1, "decoder.weight": -22.0, "encoder.bias": -21.7, "encoder.weight": -21.6, "in_head.bias": -21.7, "in_head.weight": -21.7, "out_head.bias": -22.9, "out_head.weight": -22.3},
    (33, 64, 128, 0, 130): {"loss_x": None, "loss_y": -24.2, "loss": -24.2, "rec": -21.6, "emb": -21.0, "decoder.bias": -22.4, "decoder.weight": -21.5, "encoder.bias": -21.4, "encoder.weight": -21.6, "in_head.bias": -21.5, "in_head.weight": -21.6, "out_head.bias": -21.9, "out_head.weight": -22.3},
}


def bound_of(level_log2):
    """8 x the level, rounded up to a power of two; an exact output must stay exact."""
    return 0.0 if level_log2 is None else 2.0 ** int(np.ceil(level_log2 + 3 - 1e-9))


# A loss is ONE number per (case, seed, mode): eight samples say little about its level, so the three losses take their level over
# the whole table.  A tensor's error is already a maximum over its elements, and rec, emb and the gradients are bounded case by case.
LOSS_KEYS = ("loss_x", "loss_y", "loss")
LOSS_LEVELS_LOG2 = {k: max(d[k] for d in LEVELS_LOG2.values() if d[k] is not None) for k in LOSS_KEYS}
LOSS_BOUNDS = {k: bound_of(v) for k, v in LOSS_LEVELS_LOG2.items()}
BOUNDS = {c: {k: (0.0 if v is None else LOSS_BOUNDS[k]) if k in LOSS_KEYS else bound_of(v) for k, v in d.items()}
          for c, d in LEVELS_LOG2.items()}


def rel_err(got, ref):
    ref = float(ref)
    got = float(got)
    if not np.isfinite(got):
        return np.inf
    return abs(got - ref) / abs(ref) if ref != 0 else (0.0 if got == 0 else np.inf)


def tensor_err(got, ref):
    """max |got - ref| / max |ref|."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if not np.isfinite(got).all():
        return np.inf
    d, s = np.abs(got - ref).max(), np.abs(ref).max()
    return float(d / s) if s > 0 else (0.0 if d == 0 else np.inf)


def step_errors(got, ref):
    """output -> error of a step's results `got` against the float64 `ref` (both as step_grads returns them); a gradient that
    `ref` does not have (an untouched tensor) must be absent or all zero: any non-zero value is an infinite error."""
    e = {k: 0.0 for k in OUTPUTS}
    for j, k in enumerate(("loss_x", "loss_y", "loss")):
        e[k] = rel_err(got["losses"][j], ref["losses"][j])
    for v in range(2):
        if ref["rec"][v] is not None:
            e["rec"] = max(e["rec"], tensor_err(got["rec"][v], ref["rec"][v]))
            e["emb"] = max(e["emb"], tensor_err(got["emb"][v], ref["emb"][v]))
    for k in range(16):
        g, r = got["grads"][k], ref["grads"][k]
        if r is None:
            if g is not None and np.any(np.asarray(g) != 0):
                e[group_key(k)] = np.inf
            continue
        e[group_key(k)] = max(e[group_key(k)], np.inf if g is None else tensor_err(g, r))
    return e


MODES = (("xy", ALPHA), ("x", ALPHA))


def measure_levels(case, seeds=SEEDS):
    """output -> the largest error of the fp32 restatement against float64 over the seeds and both modes of one case."""
    lv = {k: 0.0 for k in OUTPUTS}
    for seed in seeds:
        c = build_case(case, seed)
        ax, ay = gathered(c)
        for mode, alpha in MODES:
            ref = step_grads(c["P"], ax, ay, mode, alpha)
            got = step_grads(c["P"], ax, ay, mode, alpha, dt=F32)
            for k, v in step_errors(got, ref).items():
                lv[k] = max(lv[k], v)
    return lv


WRONG_VARIANTS = ("no_y_in_shared", "x_twice", "mean_over_rows", "alpha_y_on_x", "relu_mask_other", "in_head_y_stepped", "db_drop_tail",
                  "gather_idx_x_for_y", "zero_gradient", "dropped_tile")
# rows that are no multiple of 16 in both views and masks that differ; the paper's widths; the largest L of the configs
VARIANT_CASES = ((5, 17, 3, 15, 33), (50, 128, 10, 130, 130), (50, 128, 500, 17, 15))
VARIANT_MODE = {"in_head_y_stepped": "x"}


def drop_last_tile(g):
    """g with the last 16 x 16 tile of a weight gradient (16 entries of a bias gradient) left at zero: a grid one workgroup short."""
    g = np.array(g, copy=True)
    if g.ndim == 2:
        g[16 * ((g.shape[0] - 1) // 16):, 16 * ((g.shape[1] - 1) // 16):] = 0
    else:
        g[16 * ((g.shape[0] - 1) // 16):] = 0
    return g


def variant_errors(name, case, seed=0):
    """output -> error / bound of the float64 wrong variant against the float64 reference."""
    c = build_case(case, seed)
    ax, ay = gathered(c)
    mode = VARIANT_MODE.get(name, "xy")
    ref = step_grads(c["P"], ax, ay, mode, ALPHA)
    if name == "gather_idx_x_for_y":
        ids = c["idx"][0][np.arange(c["rows"][1]) % c["rows"][0]] % len(c["tables"][1])
        got = step_grads(c["P"], ax, c["tables"][1][ids][:, :c["D"]], mode, ALPHA)
    elif name in ("zero_gradient", "dropped_tile"):
        got = dict(ref)
        got["grads"] = [None if g is None else (np.zeros_like(g) if name == "zero_gradient" else drop_last_tile(g)) for g in ref["grads"]]
    else:
        got = step_grads(c["P"], ax, ay, mode, ALPHA, wrong=(name,))
    return {k: (v / BOUNDS[case][k] if BOUNDS[case][k] > 0 else (0.0 if v == 0 else np.inf)) for k, v in step_errors(got, ref).items()}


def variant_excess(name, case, seed=0):
    """The largest error / bound of the wrong variant over the outputs (must be >= 8 on every case of VARIANT_CASES)."""
    return max(variant_errors(name, case, seed).values())
