"""ONE step of the single-launch micro path (csrc/umlh_kernels_micro.hip) restated in numpy: the float64 statement the device is
compared with, an honest fp32 restatement the bounds are calibrated on, deliberately wrong variants the bounds must reject, the
envelope of the path restated in Python, and the generators / case tables of tests/test_micro_kernels_gpu.py.  No GPU, no
`umlh` import.

The step (oracle/uml_oracle.py: step_grads, optimizer_step; include/umlh.h: umlh_train_steps, UMLH_S_*).  State
(W, m, v, scales, m_scales, v_scales); a modality with rows (gathered by row ids, duplicates allowed) is "present":

    raw = X W^T,  logits z = raw * scale[mod]
    loss[mod]  = mean over the modality's OWN rows of this step of CE(z, y)          (UMLH_S_LOSS_IMG / _TXT)
    acc[mod]   = first-arg-max hits / rows                                           (UMLH_S_ACC_IMG / _TXT)
    dscale[mod] = weight * mean(E_p[raw] - raw_y)                                    (UMLH_S_GSCALE_IMG / _TXT)
    dW = sum_mod (weight * scale / rows) (p - onehot)^T X,   weight = (img_alpha, alpha)
    UMLH_S_CORRECT = hits of both modalities, UMLH_S_LOSS_SUM = sum of the row losses of both modalities

The denominator is the per-modality row count of the step itself -- the kernel's `w / rows` -- not a global row count and not
the padded tile rows.  The update is tests/_optstep_ref.py: opt_ref applied to W with dW and, for learnable scales, to the scale
of every PRESENT modality with its dscale (an absent modality's scale and moments stay as they are).

bf16 operand mode (grad64(bf16=True)): X and W are rounded to bf16 at use in both products, dZ is rounded to bf16 in the dW
product; everything else is float64 on the fp32 master weights.

Arg-max.  grad64 asserts for every row that the gap between its largest logit and the largest logit of a class with a DIFFERENT
weight row is at least GAP = 2^-12 of scale * |w|max |x| (|.| the 2-norms).  An fp32 dot product of d <= 1024 terms is off by at
most d 2^-24 |w||x| = 2^-14 |w||x|, two of them and the multiplication by scale stay under 2^-12: no fp32 evaluation flips the
arg-max, and hit counts are compared exactly (scalar_errs: UMLH_S_CORRECT is the count; an accuracy is the count times the
rounded reciprocal of the row count, within 2^-22 of the quotient).  Classes with bit-identical weight rows have bit-identical logits in the kernel
(same operands, same order): the first index wins, in the reference as on the device.  The generators only emit rows that pass.

Error measures.
    gradient   |got - ref64| / S,  S_cj = sum_r |dZ64_rc| |x_rj|  (tests/_gemm_ref.py: gemm_err), max and rms
    W' m' v' scales  fp32 ulps of the larger magnitude before / after the step (tests/_optstep_ref.py: ulp_err);
               `scales` is the largest of scales / m_scales / v_scales
    loss, gscale     |got - ref| / max(1, |ref|), the largest over the scalars of the kind

Calibration.  grad32 + update32 are the step as an honest fp32 program would run it: both products as sequential fp32 fma chains
(_gemm_ref._chain, group 1; bf16 mode: operands through _rne_bf16, one rounding per 16 products), the softmax in fp32 over
16-class slices merged with the online rule, the row loss as log S + (max - z_y), the update as _optstep_ref.kernel_form(dtype=F32), separate and fused.  A level is
its largest error over CAL_SHAPES x four seeds; the bound is 8 x the level rounded up to a power of two (bound_of).  Two regimes:
`small` (scale 2, unit-norm rows and weights: the softmax barely amplifies the logit rounding) and `op` (scale 100, unit-norm
class prototypes as weights: the reference's operating point).  tests/test_micro_ref_cpu.py re-measures every level.

Measured on the CPU (level -> bound; gradient as log2, the others as printed):

    fp32 / small
        g_max          2^-19.71  ->  2^-16
        g_rms          2^-23.48  ->  2^-20
        loss             1.5e-07  ->  1.90735e-06
        gscale          4.07e-08  ->  4.76837e-07
        sgd.W               34.9  ->  512
        sgd.m               21.9  ->  256
        sgd.scales          7.09  ->  64
        adam.W              8.49  ->  128
        adam.m              6.12  ->  64
        adam.v              1.96  ->  16
        adam.scales         2.71  ->  32
        adamw.W             8.68  ->  128
        adamw.m             3.84  ->  32
        adamw.v             1.22  ->  16
        adamw.scales        2.39  ->  32
    fp32 / op
        g_max          2^ -8.39  ->  2^-5
        g_rms          2^-13.71  ->  2^-10
        loss            3.08e-06  ->  3.05176e-05
        gscale          5.06e-08  ->  4.76837e-07
        sgd.W           3.11e+03  ->  32768
        sgd.m           1.02e+03  ->  8192
        sgd.scales         0.856  ->  8
        adam.W               264  ->  4096
        adam.m               113  ->  1024
        adam.v              1.51  ->  16
        adam.scales         2.79  ->  32
        adamw.W              267  ->  4096
        adamw.m              113  ->  1024
        adamw.v             1.46  ->  16
        adamw.scales        2.92  ->  32
    bf16 / small
        g_max          2^-10.55  ->  2^-7
        g_rms          2^-17.30  ->  2^-14
        loss            2.24e-07  ->  1.90735e-06
        gscale          6.44e-09  ->  5.96046e-08
        sgd.W               55.4  ->  512
        sgd.m           1.56e+03  ->  16384
        sgd.scales          2.17  ->  32
        adam.W               306  ->  4096
        adam.m               187  ->  2048
        adam.v              18.9  ->  256
        adam.scales          1.2  ->  16
        adamw.W              307  ->  4096
        adamw.m              187  ->  2048
        adamw.v             1.24  ->  16
        adamw.scales       0.747  ->  8
    bf16 / op
        g_max          2^ -9.47  ->  2^-6
        g_rms          2^-16.22  ->  2^-13
        loss            3.19e-07  ->  3.8147e-06
        gscale          1.75e-08  ->  2.38419e-07
        sgd.W           1.06e+03  ->  16384
        sgd.m           2.13e+03  ->  32768
        sgd.scales         0.829  ->  8
        adam.W               234  ->  2048
        adam.m               213  ->  2048
        adam.v              1.26  ->  16
        adam.scales         3.06  ->  32
        adamw.W              235  ->  2048
        adamw.m              213  ->  2048
        adamw.v             1.28  ->  16
        adamw.scales       0.935  ->  8
"""
import functools

import numpy as np

from _gemm_ref import _chain, gemm_err
from _optstep_ref import F32, F64, bound_of, kernel_form, opt_ref, ulp_err
from test_x3_split_cpu import _rne_bf16

GAP = 2.0 ** -12
CS = 16                       # classes per workgroup (UMLH_MICRO_CS)
MAX_TILES, MAX_SLICES = 4, 64
# include/umlh.h: the widths of the micro path and their (NCH, CW) chunking (csrc/umlh_kernels_micro.hip: umlh_micro_chunking)
CHUNKING = {16: (1, 16), 32: (1, 32), 48: (3, 16), 64: (1, 64), 80: (5, 16), 96: (3, 32), 128: (1, 128), 256: (2, 128),
            384: (3, 128), 512: (4, 128), 640: (5, 128), 768: (6, 128), 1024: (8, 128)}
WIDTHS_F32 = tuple(CHUNKING)
WIDTHS_BF16 = tuple(d for d, (n, cw) in CHUNKING.items() if cw == 128)
S_LOSS_IMG, S_LOSS_TXT, S_ACC_IMG, S_ACC_TXT, S_GSCALE_IMG, S_GSCALE_TXT, S_CORRECT, S_LOSS_SUM = range(8)
OPT_WRONG = ("decay_after_update", "no_bc2", "step_off_by_one")


def _cdiv(a, b):
    return -(-a // b)


def chunking(d):
    """(NCH, CW) of a width, or None outside the table."""
    return CHUNKING.get(int(d))


def bf16_supported(d):
    c = chunking(d)
    return c is not None and c[1] == 128


def eligible(d, C, ri, rt, bf16=False):
    """The envelope of the micro path for one step: width in the table (bf16: the 128-wide chunkings), at most 4 sample tiles,
    at most 64 class slices, at least one row."""
    if chunking(d) is None or (bf16 and not bf16_supported(d)):
        return False
    return ri >= 0 and rt >= 0 and ri + rt > 0 and _cdiv(ri, 16) + _cdiv(rt, 16) <= MAX_TILES and _cdiv(C, CS) <= MAX_SLICES


def bf(a):
    """Round to bf16 (nearest even), as float64."""
    return _rne_bf16(np.ascontiguousarray(a, dtype=F32)).astype(F64)


def make_state(W, m=None, v=None, scales=(1.0, 1.0), m_scales=(0.0, 0.0), v_scales=(0.0, 0.0)):
    W = np.ascontiguousarray(W, F32)
    z = np.zeros_like(W)
    return dict(W=W, m=z.copy() if m is None else np.ascontiguousarray(m, F32), v=z.copy() if v is None else np.ascontiguousarray(v, F32),
                scales=np.asarray(scales, F32), m_scales=np.asarray(m_scales, F32), v_scales=np.asarray(v_scales, F32))


def _present(mods):
    return [mods[k] is not None and len(mods[k][1]) > 0 for k in (0, 1)]


# ---------------------------------------------------------------------------------------------------------------------------- #
# float64
# ---------------------------------------------------------------------------------------------------------------------------- #
def gaps_ok(W, X, scale):
    """Per row of X: the top logit leads the best class with a different weight row by >= GAP * |scale| |w|max |x|."""
    W, X = np.asarray(W, F64), np.asarray(X, F64)
    _, first = np.unique(W, axis=0, return_index=True)
    if first.size < 2:
        return np.ones(X.shape[0], bool)
    z = float(scale) * (X @ W[np.sort(first)].T)
    top = np.partition(z, -2, axis=1)[:, -2:]
    lim = GAP * abs(float(scale)) * np.sqrt((W * W).sum(1)).max() * np.sqrt((X * X).sum(1))
    return (top[:, 1] - top[:, 0]) >= lim


def grad64(st, mods, weights, bf16=False, check_gap=True):
    """Forward, scalars and gradient of one step in float64.  mods = [(X [r, d], y [r]) or None] for image, text;
    weights = (img_alpha, alpha).  Returns dW, its normaliser S, the eight scalars and the two d loss / d scale."""
    W = st["W"].astype(F64)
    Wq = bf(W) if bf16 else W
    dW, S, sc = np.zeros_like(W), np.zeros_like(W), np.zeros(8)
    for mod, pres in enumerate(_present(mods)):
        if not pres:
            continue
        X, y = np.asarray(mods[mod][0], F64), np.asarray(mods[mod][1], np.int64)
        Xq = bf(X) if bf16 else X
        r, s = len(y), float(st["scales"][mod])
        assert not check_gap or gaps_ok(Wq, Xq, s).all(), "a row's arg-max is not safe against fp32 rounding"
        raw = Xq @ Wq.T
        z = raw * s
        mx = z.max(1)
        e = np.exp(z - mx[:, None])
        se = e.sum(1)
        p = e / se[:, None]
        ar = np.arange(r)
        ce = np.log(se) + (mx - z[ar, y])
        onehot = np.zeros_like(p)
        onehot[ar, y] = 1.0
        dz = (weights[mod] * s / r) * (p - onehot)
        dzq = bf(dz) if bf16 else dz
        dW += dzq.T @ Xq
        S += np.abs(dzq).T @ np.abs(Xq)
        hits = float((z.argmax(1) == y).sum())
        sc[S_LOSS_IMG + mod], sc[S_ACC_IMG + mod] = ce.mean(), hits / r
        sc[S_GSCALE_IMG + mod] = weights[mod] * ((p * raw).sum(1) - raw[ar, y]).mean()
        sc[S_CORRECT] += hits
        sc[S_LOSS_SUM] += ce.sum()
    return dict(dW=dW, S=S, scalars=sc, present=_present(mods))


def _update(fn, st, g, kind, learn, wrong=(), chunk=None):
    """fn(p, g, m, v) -> (p, m, v) applied to W and, when learnable, to the scales of the present modalities."""
    out = {k: np.asarray(a, F64).copy() for k, a in st.items()}
    W, m, v = fn(st["W"], g["dW"], st["m"], st["v"])
    if "moments_chunk_shift" in wrong:                       # chunk c's moments land in chunk c - 1's columns
        nch, cw = chunk
        ms, vs = np.asarray(st["m"], F64).copy(), np.asarray(st["v"], F64).copy()
        for c in range(1, nch):
            ms[:, (c - 1) * cw:c * cw] = np.asarray(m)[:, c * cw:(c + 1) * cw]
            if v is not None:
                vs[:, (c - 1) * cw:c * cw] = np.asarray(v)[:, c * cw:(c + 1) * cw]
        m, v = ms, (vs if v is not None else None)
    out["W"], out["m"] = np.asarray(W, F64), np.asarray(m, F64)
    if v is not None:
        out["v"] = np.asarray(v, F64)
    if learn:
        for mod in (0, 1):
            if not (g["present"][mod] or "scale_absent" in wrong):
                continue
            gs = g["scalars"][S_GSCALE_IMG + mod] if g["present"][mod] else 0.0
            p, m1, v1 = fn(st["scales"][mod:mod + 1], np.asarray([gs]), st["m_scales"][mod:mod + 1], st["v_scales"][mod:mod + 1])
            out["scales"][mod], out["m_scales"][mod] = p[0], m1[0]
            if v1 is not None:
                out["v_scales"][mod] = v1[0]
    return out


def update64(st, g, kind, lr, step, wd=0.0, learn=False, momentum=0.9, wrong=(), chunk=None):
    """The state after the optimizer step (opt_ref), float64.  SGD leaves v and v_scales alone."""
    ow = tuple(w for w in wrong if w in OPT_WRONG)
    fn = lambda p, gr, m, v: opt_ref(kind, p, gr, m, v, lr, step, momentum=momentum, wd=wd, wrong=ow)
    return _update(fn, st, g, kind, learn, wrong, chunk)


def step64(st, mods, weights, kind, lr, step, wd=0.0, learn=False, momentum=0.9, bf16=False):
    """(gradient record, state after the step): everything the device writes for one step."""
    g = grad64(st, mods, weights, bf16=bf16)
    return g, update64(st, g, kind, lr, step, wd, learn, momentum)


# ---------------------------------------------------------------------------------------------------------------------------- #
# fp32 restatement, with the wrong variants
# ---------------------------------------------------------------------------------------------------------------------------- #
WRONG_VARIANTS = ("dw_rows60_63", "fwd_last_kstep", "mean_over_padded", "padding_valid", "txt_img_alpha", "merge_no_rescale",
                  "merge_tie_high", "label_first_slice", "dscale_no_rawy", "scale_absent", "serw_wrong_factor",
                  "decay_after_update", "no_bc2", "step_off_by_one", "moments_chunk_shift", "stale_chunk")
# not a wrong step but a careless one, and what the kernels did before this campaign: the row loss as (log S + max) - z_y.  On the
# exact shapes (logits in the thousands) it misses their 1e-5 tolerance; tests/test_micro_ref_cpu.py shows it.
LOSS_MAX_FIRST = "loss_max_first"


def _f(x):
    return np.asarray(x, F64).astype(F32)


def grad32(st, mods, weights, bf16=False, wrong=(), stale=None):
    """grad64's outputs as an fp32 program forms them (module docstring).  Rows sit in the kernel's slot layout (image tiles,
    then text tiles, 16 slots each, padding slots with zero dZ).  `wrong`: names of WRONG_VARIANTS; `stale`: the feature rows of
    another step, used by the variant `stale_chunk` for the second chunk of the dW product."""
    W = np.ascontiguousarray(st["W"], F32)
    C, d = W.shape
    nwg = _cdiv(C, CS)
    Cp = nwg * CS
    nch, cw = chunking(d) or (1, d)
    group = 16 if bf16 else 1
    q = (lambda a: _rne_bf16(np.ascontiguousarray(a, F32))) if bf16 else (lambda a: np.ascontiguousarray(a, F32))
    pres = _present(mods)
    rows = [len(mods[k][1]) if pres[k] else 0 for k in (0, 1)]
    tiles = [_cdiv(r, 16) for r in rows]
    nslot = 16 * (tiles[0] + tiles[1])
    dz_slots, x_slots = np.zeros((nslot, C), F32), np.zeros((nslot, d), F32)
    sc, hits_all, loss_all = np.zeros(8, F32), F32(0), F32(0)
    NEG = F32(-np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for mod in (0, 1):
            if not pres[mod]:
                continue
            X, y = np.ascontiguousarray(mods[mod][0], F32), np.asarray(mods[mod][1], np.int64)
            Xd = X if stale is None else np.ascontiguousarray(stale[mod], F32)
            r = den = rows[mod]
            if "padding_valid" in wrong and r % 16:          # the first padding slot re-reads the last row and counts
                X, Xd, y, r = np.vstack([X, X[-1:]]), np.vstack([Xd, Xd[-1:]]), np.append(y, y[-1]), r + 1
            if "mean_over_padded" in wrong:
                den = 16 * tiles[mod]
            wmod = F32(weights[0] if (mod == 1 and "txt_img_alpha" in wrong) else weights[mod])
            s = F32(st["scales"][mod])
            raw = _chain([q(X)], [q(W)], ((0, 0),), group)
            if "fwd_last_kstep" in wrong:                    # classes 4g + 3 without the last MFMA's four k
                ks = d - 16 + np.array([3, 7, 11, 15])
                raw[:, 3::4] = _f(raw[:, 3::4].astype(F64) - X[:, ks].astype(F64) @ W[3::4, ks].astype(F64).T)
            z = np.full((r, Cp), NEG, F32)
            z[:, :C] = raw * s
            rawp = np.zeros((r, Cp), F32)
            rawp[:, :C] = raw
            z3, raw3 = z.reshape(r, nwg, CS), rawp.reshape(r, nwg, CS)
            ar = np.arange(r)
            mloc = z3.max(2)
            e = np.exp(z3 - mloc[:, :, None]).astype(F32)
            sloc = e.sum(2, dtype=F32)
            serw = (e * raw3).sum(2, dtype=F32)
            amloc = z3.argmax(2) + CS * np.arange(nwg)[None, :]
            RY = raw[ar, y].copy()
            if "label_first_slice" in wrong:
                RY = np.where(y < CS, RY, F32(0))
            M, Ssum, SR, AM = np.full(r, NEG, F32), np.zeros(r, F32), np.zeros(r, F32), np.full(r, 2 ** 31 - 1, np.int64)
            for w in range(nwg):
                m_, s_, sr_, am_ = mloc[:, w], sloc[:, w], serw[:, w], amloc[:, w]
                Mn = np.maximum(M, m_)
                fo = np.where(M == NEG, F32(0), np.exp(M - Mn)).astype(F32)
                fn = np.exp(m_ - Mn).astype(F32)
                Ssum = (Ssum + s_ * fn) if "merge_no_rescale" in wrong else (Ssum * fo + s_ * fn)
                SR = (SR * fn + sr_ * fo) if "serw_wrong_factor" in wrong else (SR * fo + sr_ * fn)
                take = (m_ >= M) if "merge_tie_high" in wrong else ((m_ > M) | ((m_ == M) & (am_ < AM)))
                AM = np.where(take, am_, AM)
                M = Mn
            f = (np.exp(mloc - M[:, None]).astype(F32) * (F32(1) / Ssum)[:, None]).astype(F32)
            p = (e * f[:, :, None]).astype(F32).reshape(r, Cp)[:, :C]
            onehot = np.zeros((r, C), F32)
            onehot[ar, y] = 1
            coef = F32(F32(wmod / F32(den)) * s)
            dz = ((p - onehot) * coef).astype(F32)
            if "loss_max_first" in wrong:                    # (log S + M) - z_y: rounds at the ulp of the largest logit
                vl = ((np.log(Ssum).astype(F32) + M) - RY * s).astype(F32)
            else:
                vl = (np.log(Ssum).astype(F32) + (M - RY * s).astype(F32)).astype(F32)
            vg = (SR / Ssum).astype(F32) if "dscale_no_rawy" in wrong else ((SR / Ssum).astype(F32) - RY).astype(F32)
            hits = F32((AM == y).sum())
            hits_all += hits
            loss_all += vl.sum(dtype=F32)
            inv = F32(1) / F32(den)
            sc[S_LOSS_IMG + mod], sc[S_ACC_IMG + mod] = vl.sum(dtype=F32) * inv, hits * inv
            sc[S_GSCALE_IMG + mod] = vg.sum(dtype=F32) * wmod * inv
            s0 = 16 * tiles[0] if mod == 1 else 0
            r = min(r, 16 * tiles[mod])
            dz_slots[s0:s0 + r], x_slots[s0:s0 + r] = dz[:r], X[:r]
            if "stale_chunk" in wrong:
                c = min(1, nch - 1)
                x_slots[s0:s0 + r, c * cw:(c + 1) * cw] = Xd[:r, c * cw:(c + 1) * cw]
    sc[S_CORRECT] = hits_all
    sc[S_LOSS_SUM] = loss_all
    if "dw_rows60_63" in wrong:
        dz_slots[60:64, 3::4] = 0
    dW = _chain([q(dz_slots.T)], [q(x_slots.T)], ((0, 0),), group)
    return dict(dW=dW.astype(F64), scalars=sc.astype(F64), present=pres)


def update32(st, g, kind, lr, step, wd=0.0, learn=False, momentum=0.9, fused=False, wrong=(), chunk=None):
    """kernel_form in fp32 (separate or fused); an optimizer variant of OPT_WRONG runs opt_ref(wrong=...) on the fp32 gradient."""
    if any(w in OPT_WRONG for w in wrong):
        return update64(st, g, kind, lr, step, wd, learn, momentum, wrong, chunk)
    fn = lambda p, gr, m, v: kernel_form(kind, p, gr, m, v, lr, step, momentum=momentum, wd=wd, dtype=F32, fused=fused)
    return _update(fn, st, g, kind, learn, wrong, chunk)


# ---------------------------------------------------------------------------------------------------------------------------- #
# error measures
# ---------------------------------------------------------------------------------------------------------------------------- #
def grad_err(got_dW, ref):
    """(max, rms) of |got - dW64| / S.  Elements whose S lies below the fp32 normal range (a softmax tail of exp(-128) and
    less) cannot be resolved by an fp32 result at all: there the output must itself be below 2^-126 and is left out of the ratio."""
    got, tiny = np.asarray(got_dW, F64), ref["S"] < 2.0 ** -126
    if tiny.any() and not np.abs(got[tiny]).max() < 2.0 ** -126:
        return np.inf, np.inf
    if tiny.all():
        return 0.0, 0.0
    return gemm_err(got[~tiny], ref["dW"][~tiny], ref["S"][~tiny])


def scalar_errs(got, ref, learn):
    """loss / gscale: |got - ref| / max(1, |ref|).  acc: 0 when the hit counts are exact, else inf -- UMLH_S_CORRECT must be the
    count itself, and an accuracy must lie within 2^-22 relative of hits / rows (the kernel multiplies the count by the rounded
    reciprocal of the row count: two roundings of at most 2^-24 relative each), which pins the count since rows <= 64."""
    got, want = np.asarray(got[:8], F64), ref["scalars"]
    rel = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    acc = [S_ACC_IMG, S_ACC_TXT]
    ok = got[S_CORRECT] == want[S_CORRECT] and np.all(np.abs(got[acc] - want[acc]) <= 2.0 ** -22 * want[acc])
    out = {"loss": float(rel[[S_LOSS_IMG, S_LOSS_TXT, S_LOSS_SUM]].max()), "acc": 0.0 if ok else np.inf}
    if learn:
        out["gscale"] = float(rel[[S_GSCALE_IMG, S_GSCALE_TXT]].max())
    return out


def state_errs(got, ref, before, kind, learn):
    """W / m / v (/ scales) in ulps; under SGD v and v_scales must be bit-identical to `before` and are not measured."""
    out = {k: ulp_err(got[k], ref[k], before[k]) for k in (("W", "m") if kind == "sgd" else ("W", "m", "v"))}
    if learn:
        names = ("scales", "m_scales") if kind == "sgd" else ("scales", "m_scales", "v_scales")
        out["scales"] = max(ulp_err(got[k], ref[k], before[k]) for k in names)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- #
# generators
# ---------------------------------------------------------------------------------------------------------------------------- #
REGIMES = {"small": 2.0, "op": 100.0}


def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def make_tables(d, C, regime, seed=0, n_img=100, n_txt=90, tie=False, last_slice=False):
    """Feature tables, labels and weights of a case (read-only; shared by the tests).  `small`: unit-norm random rows and
    weights, scale 2.  `op`: weights are unit-norm class prototypes (zero-shot-like), a row is its class prototype at cosine
    ~0.12 plus unit noise, scale 100.  Rows whose arg-max is not safe (gaps_ok, for the fp32 AND the bf16-rounded operands) are
    drawn again.  tie: classes a < b of different slices get bit-identical weight rows and some rows of both labels that they
    win.  last_slice: half of the labels fall into the last (partial) class slice."""
    rng = np.random.default_rng([d, C, int(seed), 0 if regime == "small" else 1, int(tie), int(last_slice)])
    scale = REGIMES[regime]
    P = _unit(rng.standard_normal((C, d)))
    W = P.astype(F32)
    a = b = None
    if tie:
        assert C > CS
        a, b = int(rng.integers(0, CS)), int(rng.integers(CS * ((C - 1) // CS), C))
        W[b] = W[a]
    Wb = bf(W)

    def rows(n):
        y = rng.integers(0, C, n)
        if last_slice:
            y[::2] = rng.integers(CS * ((C - 1) // CS), C, len(y[::2]))
        if tie:
            y[1::5], y[2::5] = a, b
        draw = lambda yy: _unit((0.12 * P[yy] if regime == "op" else 0.0) + _unit(rng.standard_normal((len(yy), d)))).astype(F32)
        x = draw(y)
        if tie:                                              # rows of the tied labels are won by the tied pair
            t = (y == a) | (y == b)
            x[t] = _unit(P[a][None, :] + 0.5 * _unit(rng.standard_normal((int(t.sum()), d)))).astype(F32)
        for _ in range(200):
            bad = ~(gaps_ok(W, x, scale) & gaps_ok(Wb, bf(x), scale))
            if not bad.any():
                return x, y.astype(np.int64)
            if tie:
                t = bad & ((y == a) | (y == b))
                x[t] = _unit(P[a][None, :] + 0.5 * _unit(rng.standard_normal((int(t.sum()), d)))).astype(F32)
                bad &= ~t
            x[bad] = draw(y[bad])
        raise AssertionError("no safe rows found")
    xi, yi = rows(n_img)
    xt, yt = rows(n_txt)
    for arr in (xi, yi, xt, yt, W):
        arr.setflags(write=False)
    return dict(xi=xi, yi=yi, xt=xt, yt=yt, W=W, scale=scale, tie=(a, b))


def draw_ids(rng, n_table, r):
    """r row ids with duplicates (the first id is repeated whenever there is room)."""
    ids = rng.integers(0, n_table, r)
    if r >= 3:
        ids[r // 2] = ids[0]
    return ids.astype(np.int64)


def step_mods(tab, ids_i, ids_t):
    return [None if ids_i is None or len(ids_i) == 0 else (tab["xi"][ids_i], tab["yi"][ids_i]),
            None if ids_t is None or len(ids_t) == 0 else (tab["xt"][ids_t], tab["yt"][ids_t])]


def live_state(tab, g, seed, scales=None):
    """A well conditioned live optimizer state for the gradient g (float64 dW): |m| in 0.5 .. 1 of max(|g|, rms g) with either
    sign and v in 1 .. 4 of max(g^2, rms^2).  v >= g^2 keeps |d update / d g| <= lr / sqrt(v): the step does not amplify the
    rounding of the gradient, and no element of m is small against the gradient's own error."""
    rng = np.random.default_rng([int(seed), 77])
    gm = np.maximum(np.abs(g), np.sqrt((g * g).mean()) + 1e-30)
    m = rng.choice([-1.0, 1.0], g.shape) * gm * rng.uniform(0.5, 1.0, g.shape)
    v = gm * gm * rng.uniform(1.0, 4.0, g.shape)
    s = tab["scale"]
    return make_state(tab["W"], m, v, scales=scales or (s, 0.75 * s), m_scales=(0.02, -0.03), v_scales=(0.004, 0.006))


def live_case(tab, mods, seed, bf16=False):
    """live_state for the gradient the step itself will form (at the live state's scales)."""
    s = tab["scale"]
    return live_state(tab, grad64(make_state(tab["W"], scales=(s, 0.75 * s)), mods, WEIGHTS, bf16=bf16)["dW"], seed)


ALPHA, IMG_ALPHA = 0.7, 1.0
WEIGHTS = (IMG_ALPHA, ALPHA)
# the optimizer cases: lr and decay of tests/_optstep_ref.py (at the reference's own lr 1e-3 / wd 0.01 a decay applied after the
# update differs by lr * wd * update, under one ulp of a unit-norm weight: no accuracy test could tell)
LR = 1e-2
KIND_WD = {"sgd": 0.1, "adam": 0.1, "adamw": 0.1}
OPT_STEPS = (1, 2, 1000)

# ---------------------------------------------------------------------------------------------------------------------------- #
# calibration
# ---------------------------------------------------------------------------------------------------------------------------- #
CAL_SEEDS = (0, 1, 2, 3)
# (d, C, rows_img, rows_txt): every chunk width, register / memory moments, one and 63 class slices, ragged and single rows
CAL_SHAPES = ((48, 37, 32, 32), (48, 37, 17, 30), (256, 37, 32, 32), (1024, 37, 17, 30), (128, 2, 8, 8), (768, 1000, 32, 32),
              (640, 100, 64, 0), (512, 17, 1, 1))


def _merge(dst, src):
    for k, v in src.items():
        dst[k] = max(dst.get(k, 0.0), v)


def measure_levels(mode, regime, shapes=CAL_SHAPES, seeds=CAL_SEEDS):
    """measure -> level of step32 against step64: g_max, g_rms, loss, gscale and, per optimizer kind, `kind.W` ... in ulps."""
    bf16 = mode == "bf16"
    lv = {}
    for d, C, ri, rt in shapes:
        if bf16 and not bf16_supported(d):
            continue
        for seed in seeds:
            tab = make_tables(d, C, regime, seed, 100, 90, False, False)
            rng = np.random.default_rng([seed, d, C])
            mods = step_mods(tab, draw_ids(rng, 100, ri), draw_ids(rng, 90, rt))
            st0 = make_state(tab["W"], scales=(tab["scale"], 0.75 * tab["scale"]))
            ref = grad64(st0, mods, WEIGHTS, bf16=bf16)
            got = grad32(st0, mods, WEIGHTS, bf16=bf16)
            mx, rms = grad_err(got["dW"], ref)
            _merge(lv, {"g_max": mx, "g_rms": rms})
            _merge(lv, {k: v for k, v in scalar_errs(got["scalars"], ref, True).items() if k != "acc"})
            assert scalar_errs(got["scalars"], ref, True)["acc"] == 0.0
            st = live_state(tab, ref["dW"], seed)
            for kind in ("sgd", "adam", "adamw"):
                for step in OPT_STEPS:
                    want = update64(st, ref, kind, LR, step, KIND_WD[kind], True)
                    for fused in (False, True):
                        have = update32(st, got, kind, LR, step, KIND_WD[kind], True, fused=fused)
                        _merge(lv, {f"{kind}.{k}": v for k, v in state_errs(have, want, st, kind, True).items()})
    return lv


# measured levels (rounded up in the last printed digit): the table of the module docstring
LEVELS = {
    ('fp32', 'small'): {
        "g_max": 1.17e-06, "g_rms": 8.56e-08, "loss": 1.5e-07, "gscale": 4.07e-08, "sgd.W": 34.9, "sgd.m": 21.9,
        "sgd.scales": 7.09, "adam.W": 8.49, "adam.m": 6.12, "adam.v": 1.96, "adam.scales": 2.71, "adamw.W": 8.68,
        "adamw.m": 3.84, "adamw.v": 1.22, "adamw.scales": 2.39,
    },
    ('fp32', 'op'): {
        "g_max": 0.00298, "g_rms": 7.46e-05, "loss": 3.08e-06, "gscale": 5.06e-08, "sgd.W": 3.11e+03, "sgd.m": 1.02e+03,
        "sgd.scales": 0.856, "adam.W": 264, "adam.m": 113, "adam.v": 1.51, "adam.scales": 2.79, "adamw.W": 267,
        "adamw.m": 113, "adamw.v": 1.46, "adamw.scales": 2.92,
    },
    ('bf16', 'small'): {
        "g_max": 0.000665, "g_rms": 6.2e-06, "loss": 2.24e-07, "gscale": 6.44e-09, "sgd.W": 55.4, "sgd.m": 1.56e+03,
        "sgd.scales": 2.17, "adam.W": 306, "adam.m": 187, "adam.v": 18.9, "adam.scales": 1.2, "adamw.W": 307,
        "adamw.m": 187, "adamw.v": 1.24, "adamw.scales": 0.747,
    },
    ('bf16', 'op'): {
        "g_max": 0.00141, "g_rms": 1.31e-05, "loss": 3.19e-07, "gscale": 1.75e-08, "sgd.W": 1.06e+03, "sgd.m": 2.13e+03,
        "sgd.scales": 0.829, "adam.W": 234, "adam.m": 213, "adam.v": 1.26, "adam.scales": 3.06, "adamw.W": 235,
        "adamw.m": 213, "adamw.v": 1.28, "adamw.scales": 0.935,
    },
}


def bound(mode, regime, key):
    return bound_of(LEVELS[(mode, regime)][key])


# ---------------------------------------------------------------------------------------------------------------------------- #
# case tables (tests/test_micro_kernels_gpu.py runs exactly these; tests/test_micro_ref_cpu.py turns the wrong variants on them)
# ---------------------------------------------------------------------------------------------------------------------------- #
N_IMG, N_TXT = 100, 90                                     # table rows
PROBE_ROWS = ((32, 32), (17, 30))                          # all 64 slots live; two ragged 2-tile modalities
PROBE_C = 37                                               # three class slices, the last one partial
PATTERNS = ((64, 0), (0, 64), (1, 1), (8, 8), (16, 48), (48, 16), (1, 48), (33, 16), (20, 30))
PATTERN_WIDTHS = ((48, "fp32"), (640, "fp32"), (1024, "fp32"), (640, "bf16"))
CLASS_SWEEP = (2, 16, 17, 100, 1000, 1024)
CLASS_WIDTHS = (128, 768)
OPT_WIDTHS = (80, 512, 768, 1024)                          # moments in registers / v in memory / m and v in memory
OPT_WIDTHS_BF16 = (640, 512, 768, 1024)                    # (80 has no bf16 kernel: the largest resident-rows ring instead)
OPT_KINDS = ("sgd", "adam", "adamw")


def tables(d, C, regime, seed=0, tie=False, last_slice=False):
    return make_tables(d, C, regime, seed, N_IMG, N_TXT, tie, last_slice)


def build_case(d, C, ri, rt, regime, seed=0, tie=False, last_slice=False):
    """(tables, image row ids or None, text row ids or None) of a one-step case."""
    tab = make_tables(d, C, regime, seed, N_IMG, N_TXT, tie, last_slice)
    rng = np.random.default_rng([int(seed), d, C, ri, rt])
    return tab, (draw_ids(rng, N_IMG, ri) if ri else None), (draw_ids(rng, N_TXT, rt) if rt else None)


def probe_state(tab):
    """Zero moments, both scales at the regime's value: under SGD with momentum 0 and no decay m' is the gradient itself."""
    return make_state(tab["W"], scales=(tab["scale"], tab["scale"]))


def excess(errs, mode, regime, prefix=""):
    """The largest error / bound over the measures of `errs` (`acc` has the bound 0: any miss is infinite)."""
    worst = 0.0
    for k, e in errs.items():
        if k == "acc":
            worst = max(worst, e)
        else:
            worst = max(worst, e / bound(mode, regime, prefix + k))
    return worst


def variant_excess(name, d, C, ri, rt, regime, kind=None, step=1, learn=True, tie=False, seed=0):
    """error / bound of step32 with the wrong variant `name` against step64 at one case: the probe's measures (kind None) or
    the state after a real optimizer step from a live state."""
    tab, ii, ti = build_case(d, C, ri, rt, regime, seed, tie=tie)
    mods = step_mods(tab, ii, ti)
    stale = None
    if name == "stale_chunk":                               # the rows of another step: every id moved on by one
        stale = [None if i is None else x[(i + 1) % len(x)] for i, x in ((ii, tab["xi"]), (ti, tab["xt"]))]
    st0 = probe_state(tab)
    ref = grad64(st0, mods, WEIGHTS)
    got = grad32(st0, mods, WEIGHTS, wrong=(name,), stale=stale)
    mx, rms = grad_err(got["dW"], ref)
    errs = dict(g_max=mx, g_rms=rms, **scalar_errs(got["scalars"], ref, learn))
    worst = excess(errs, "fp32", regime)
    if kind is not None:
        st = live_state(tab, ref["dW"], seed)
        ref = grad64(st, mods, WEIGHTS)
        got = grad32(st, mods, WEIGHTS, wrong=(name,), stale=stale)
        want = update64(st, ref, kind, LR, step, KIND_WD[kind], learn)
        have = update32(st, got, kind, LR, step, KIND_WD[kind], learn, wrong=(name,), chunk=chunking(d))
        worst = max(worst, excess(state_errs(have, want, st, kind, learn), "fp32", regime, kind + "."))
    return worst


# variant -> the GPU cases it is turned on (any one of them must break a bound by 8 x)
VARIANT_CASES = {
    "dw_rows60_63": [dict(d=256, C=PROBE_C, ri=32, rt=32, regime=r) for r in REGIMES],
    "fwd_last_kstep": [dict(d=256, C=PROBE_C, ri=32, rt=32, regime=r) for r in REGIMES],
    "mean_over_padded": [dict(d=256, C=PROBE_C, ri=17, rt=30, regime=r) for r in REGIMES],
    "padding_valid": [dict(d=256, C=PROBE_C, ri=17, rt=30, regime=r) for r in REGIMES],
    "txt_img_alpha": [dict(d=48, C=PROBE_C, ri=32, rt=32, regime=r) for r in REGIMES],
    "merge_no_rescale": [dict(d=128, C=100, ri=32, rt=32, regime=r) for r in REGIMES],
    "merge_tie_high": [dict(d=128, C=100, ri=32, rt=32, regime=r, tie=True) for r in REGIMES],
    "label_first_slice": [dict(d=128, C=100, ri=32, rt=32, regime=r) for r in REGIMES],
    "dscale_no_rawy": [dict(d=80, C=PROBE_C, ri=17, rt=30, regime=r, kind="adamw") for r in REGIMES],
    "scale_absent": [dict(d=80, C=PROBE_C, ri=0, rt=64, regime=r, kind="adam") for r in REGIMES],
    "serw_wrong_factor": [dict(d=128, C=100, ri=32, rt=32, regime=r) for r in REGIMES],
    "decay_after_update": [dict(d=80, C=PROBE_C, ri=17, rt=30, regime=r, kind="adamw", step=s) for r in REGIMES for s in OPT_STEPS],
    "no_bc2": [dict(d=512, C=PROBE_C, ri=17, rt=30, regime=r, kind="adam") for r in REGIMES],
    "step_off_by_one": [dict(d=512, C=PROBE_C, ri=17, rt=30, regime=r, kind="adamw") for r in REGIMES],
    "moments_chunk_shift": [dict(d=768, C=PROBE_C, ri=17, rt=30, regime=r, kind="adamw") for r in REGIMES],
    "stale_chunk": [dict(d=256, C=PROBE_C, ri=32, rt=32, regime=r) for r in REGIMES],
}

# ---------------------------------------------------------------------------------------------------------------------------- #
# bf16 operand mode bit for bit: the construction of tests/_bf16_exact_ref.py on the micro step's own denominators
# ---------------------------------------------------------------------------------------------------------------------------- #
EXACT_PATTERNS = ((32, 32), (8, 8), (1, 1), (64, 0), (16, 32))
EXACT_C = 100                                              # seven class slices, the last one of four classes
EXACT_LIVE = ((16, 16), (2, 96), (64, 16))                 # (live classes, live_from): from the second slice on / the last slice only


def exact_shapes():
    """Every bf16 width x every row pattern, the live sets rotating so that each width and each pattern meets all three;
    one negative scale; one 63-slice head whose live classes sit in its last slice."""
    import _bf16_exact_ref as X
    out = []
    for i, d in enumerate(WIDTHS_BF16):
        for j, (ri, rt) in enumerate(EXACT_PATTERNS):
            live, lf = EXACT_LIVE[(i + j) % 3]
            out.append(X.single(d, EXACT_C, live, ri, rt, live_from=lf, own_rows=True, cap=64, tab_i=N_IMG, tab_t=N_TXT,
                                scale=-64.0 if (d, j) == (384, 0) else 64.0))
    out.append(X.single(256, 1000, 2, 32, 32, live_from=992, own_rows=True, cap=64, tab_i=N_IMG, tab_t=N_TXT))
    return out
