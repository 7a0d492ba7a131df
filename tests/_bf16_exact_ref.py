"""Operands for which the whole bf16 head step is EXACT, and its float64 reference  --  TEST INFRASTRUCTURE ONLY.

The bf16 step rounds features, W_head, W_proj, H, dZ and dH to bf16 and accumulates in fp32, so against float64 it normally
carries 2^-9 per rounded element.  The operands built here make every one of those roundings the identity and every fp32
accumulation exact, so the float64 result cast to fp32 is the ONLY correct answer and the device is compared with it bit for
bit (tests/test_bf16_exact_gpu.py); tests/test_bf16_exact_cpu.py runs the construction for every shape and shows that the
criterion notices one-row defects.

Construction (G = 2^15 global rows, scale = +-64, img_alpha = 1, alpha = 1/2, so coef = weight * scale / G is a power of two):
  * a live set of C' classes: all live rows of W_head agree on every column a feature row can be non-zero in; dead rows are
    the same with -+2 in column 0 (the sign opposite to scale's); every feature row has a 1 in column 0.  The live logits of a
    row are then bit-identical (same operands, same order) and every dead logit lies 128 below, -184 in log2 units, where exp2
    is 0 in fp32.  So p = 1/C' on live classes and exactly 0 on dead ones, and the true dZ values coef/C', coef(1/C' - 1), 0 and
    -coef are bf16 numbers for C' <= 256.  The device's own rcp / exp2 / fma may be an fp32 ulp off; its rounding of dZ to bf16
    lands back on the exact value, since a representable value is half a bf16 ulp away from any tie.  (C' = 512 is out:
    511/512 needs 9 significant bits and sits exactly on a tie.)
  * operands are small integers, so every sum the device forms (logits, H, dH, dW_head, dW_proj) is a sum of integer multiples
    of one power-of-two quantum q with sum|terms|/q < 2^24: every partial sum, in any order, tile shape or split-K plan, is
    exact in fp32.
None of this is trusted: ``reference`` asserts every representability condition it relies on.

Scalar definitions (oracle/uml_oracle.py step_grads, include/umlh.h umlh_batch_t / UMLH_S_*): loss = weighted CE "mean" whose
denominator is ``global_rows``, i.e. sum of the row losses / G, unweighted in the scalars; accuracy = first-arg-max hits / G;
dZ = weight * scale * (softmax - onehot) / G; dW_head = dZ_i^T F_i + dZ_t^T X_t; dH = dZ_i W_head; dW_proj = dH^T X_i;
plain SGD: W - lr * g.

``own_rows`` (the single-launch micro step, tests/test_micro_kernels_gpu.py): the denominator of each modality is its OWN row
count of the step in place of G -- the micro kernel's ``w / rows`` -- and must be a power of two (1 .. 64), so that
weight * scale / rows stays one; C' = 16 joins the live counts there (1/16 and 15/16 are bf16 numbers).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

G = 1 << 15                       # global_rows of every RowBatch
IMG_ALPHA, ALPHA = 1.0, 0.5
LR = 2.0 ** -3
LIVE_COUNTS = (2, 8, 32, 64, 128, 256)
LIMIT = float(1 << 24)


@dataclass(frozen=True)
class Shape:
    d_img: int
    d: int                        # d_shared (= d_img for the single-layer head)
    C: int
    live: int                     # C'
    ri: int
    rt: int
    two_layer: bool = False
    scale: float = 64.0
    cap: int = 512                # row capacity of the image side (text: 512)
    tab_i: int = 400              # rows of the tables the batches are gathered from
    tab_t: int = 350
    live_from: int = 0            # classes below are all dead
    dense: bool = False           # index=None: rows 0..rows-1 of the tables
    own_rows: bool = False        # denominators: each modality's own row count (a power of two), not G

    @property
    def id(self) -> str:
        s = f"{self.d_img}-{self.d}" if self.two_layer else f"{self.d}"
        return f"{s}-{self.C}-{self.live}-{self.ri}-{self.rt}" + ("-neg" if self.scale < 0 else "") + ("-dense" if self.dense else "") + (f"-own{self.live_from}" if self.own_rows else "")

    def den(self, mod: str) -> int:
        """The denominator of a modality's mean ('img' / 'txt')."""
        return (self.ri if mod == "img" else self.rt) if self.own_rows else G


def single(d, C, live, ri, rt, **kw) -> Shape:
    return Shape(d, d, C, live, ri, rt, **kw)


def double(d_img, d_sh, C, live, ri, rt, **kw) -> Shape:
    return Shape(d_img, d_sh, C, live, ri, rt, two_layer=True, **kw)


# The smallest shapes that still cross every tile boundary of the bf16 kernels: 32-row forward tiles, 64-row k-chunks, 256-row
# slabs, 128-class tiles, 128-column d tiles.
SINGLE_SHAPES = [
    single(128, 64, 64, 300, 257),
    single(128, 2, 2, 1, 1),
    single(256, 37, 32, 65, 0),
    single(384, 200, 64, 33, 1, live_from=128),          # the first arg-max comes from the second 128-class tile
    single(1024, 1000, 128, 0, 63),
    single(512, 1000, 256, 255, 257, scale=-64.0),
    single(512, 1000, 256, 4096, 333, cap=4096, tab_i=5000, tab_t=600),   # several split-K slabs and a short last one
]
DENSE_SHAPES = [single(128, 64, 64, 300, 257, dense=True), single(512, 1000, 256, 255, 257, scale=-64.0, dense=True)]
DOUBLE_SHAPES = [
    double(64, 128, 10, 8, 70, 33),
    double(192, 256, 200, 64, 257, 0),
    double(1024, 384, 1000, 256, 300, 257),
    double(128, 1024, 1000, 128, 1, 63),
]
UPDATE_SHAPES = [SINGLE_SHAPES[0], SINGLE_SHAPES[3], SINGLE_SHAPES[5], DOUBLE_SHAPES[0]]
ALL_SHAPES = SINGLE_SHAPES + DENSE_SHAPES + DOUBLE_SHAPES


@dataclass
class Case:
    shape: Shape
    live: np.ndarray              # sorted class ids
    xi: np.ndarray                # image table [tab_i, d_img] fp32
    yi: np.ndarray                # its labels
    ii: Optional[np.ndarray]      # gathered row ids (duplicates included) or None
    xt: np.ndarray                # text table [tab_t, d] fp32
    yt: np.ndarray
    ti: Optional[np.ndarray]
    w_head: np.ndarray            # [C, d] fp32
    w_proj: Optional[np.ndarray]  # [d, d_img] fp32


@dataclass
class Ref:
    g_head: np.ndarray            # fp32: the float64 gradient, exactly
    g_proj: Optional[np.ndarray]
    loss_img: float               # float64
    loss_txt: float
    acc_img: np.float32
    acc_txt: np.float32
    w_head_new: np.ndarray        # W - LR * g, fp32, exact
    w_proj_new: Optional[np.ndarray]


def bf16_round(a) -> np.ndarray:
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def assert_bf16_exact(name: str, a64: np.ndarray) -> None:
    """``a64`` (float64) is a bf16 number element for element: what the device rounds to bf16 it leaves unchanged."""
    a32 = a64.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a64), f"{name}: not even fp32 numbers"
    assert np.array_equal(bf16_round(a32), a32), f"{name}: a bf16 rounding would change it"


def assert_f32_exact(name: str, a64: np.ndarray) -> np.ndarray:
    a32 = a64.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a64), f"{name}: does not survive the fp32 round trip"
    return a32


def assert_exact_sum(name: str, a: np.ndarray, b: np.ndarray, q: float) -> None:
    """Every term of the contraction a @ b is an integer multiple of q and sum|terms|/q < 2^24 for every output element:
    all its partial sums, in any order, are fp32 numbers."""
    terms = np.abs(a) @ np.abs(b)
    assert terms.size == 0 or terms.max() / q < LIMIT, f"{name}: sum|terms|/q = {terms.max() / q:.3g} >= 2^24"


def _ints(rng, lo, hi, shape) -> np.ndarray:
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def _live_set(rng, s: Shape) -> np.ndarray:
    cand = np.arange(s.live_from, s.C)
    if s.live == s.C:
        return np.arange(s.C)
    chosen = []
    if s.C > 256 and not s.own_rows:   # every 32-class slice (one wave's classes of the widest forward) holds a live class
        chosen = [int(rng.integers(lo, min(lo + 32, s.C))) for lo in range(0, s.C, 32)]
    rest = np.setdiff1d(cand, chosen)
    chosen = np.concatenate([np.asarray(chosen, dtype=np.int64), rng.choice(rest, s.live - len(chosen), replace=False)])
    return np.sort(chosen)


def _labels(rng, s: Shape, live: np.ndarray, n: int) -> np.ndarray:
    """About a quarter on the lowest live class (the only label the full tie counts as correct), the other live labels
    uniform; about 10 % dead labels when there are dead classes."""
    y = rng.choice(live, n)
    y[rng.random(n) < 0.25] = live[0]
    dead = np.setdiff1d(np.arange(s.C), live)
    if dead.size:
        pick = rng.random(n) < 0.1
        y[pick] = rng.choice(dead, int(pick.sum()))
    return y.astype(np.int64)


def make_case(s: Shape, seed: Optional[int] = None) -> Case:
    if s.own_rows and any(r & (r - 1) or r > 64 for r in (s.ri, s.rt)):
        raise ValueError("own_rows: row counts must be powers of two up to 64 (or 0)")
    if s.live not in LIVE_COUNTS + ((16,) if s.own_rows else ()):
        raise ValueError(f"C' = {s.live}: the dZ values coef/C' and coef(1/C' - 1) are bf16 numbers only for C' in {LIVE_COUNTS} "
                         "(at 512, 511/512 is a rounding tie)")
    if s.live > s.C - s.live_from or abs(s.scale) != 64.0:
        raise ValueError("bad shape")
    rng = np.random.default_rng(seed if seed is not None else 7 * s.d_img + 3 * s.d + s.C + s.ri + s.rt)
    live = _live_set(rng, s)
    dead_shift = -2.0 if s.scale > 0 else 2.0
    is_live = np.zeros(s.C, dtype=bool)
    is_live[live] = True
    h = s.d // 2 if s.two_layer else s.d                     # the columns the features can see
    v = _ints(rng, -1, 1, h)
    w = np.zeros((s.C, s.d), dtype=np.float32)
    w[:, :h] = v
    w[~is_live, 0] += dead_shift
    w_proj = None
    if s.two_layer:
        # columns >= h: live entries in {-1, 0, 1} whose sum over the live rows is even and at most 16 in magnitude
        for n in range(h, s.d):
            m = 2 * int(rng.integers(0, s.live // 2 + 1))                       # non-zeros (even, as the sum is)
            top = min(16, m)
            sgn_sum = 2 * int(rng.integers(-(top // 2), top // 2 + 1))
            col = np.zeros(s.live, dtype=np.float32)
            col[:(m + sgn_sum) // 2] = 1.0
            col[(m + sgn_sum) // 2:m] = -1.0
            w[live, n] = rng.permutation(col)
        w[np.ix_(~is_live, np.arange(h, s.d))] = _ints(rng, -1, 1, (int((~is_live).sum()), s.d - h))
        w_proj = np.zeros((s.d, s.d_img), dtype=np.float32)
        w_proj[0, 0] = 1.0
        chunks = s.d_img // 64
        for n in range(1, h):                                                   # <= 16 entries +-1 over all 64-wide k-chunks
            for c in range(chunks):
                cnt = 16 // chunks + (1 if c < 16 % chunks else 0)
                cols = rng.choice(np.arange(max(64 * c, 1), 64 * c + 64), cnt, replace=False)
                w_proj[n, cols] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), cnt)
        xi = _ints(rng, -3, 3, (s.tab_i, s.d_img))
    else:
        xi = _ints(rng, -7, 7, (s.tab_i, s.d_img))
    xi[:, 0] = 1.0
    xt = _ints(rng, -7, 7, (s.tab_t, s.d))
    xt[:, 0] = 1.0
    xt[:, h:] = 0.0
    yi, yt = _labels(rng, s, live, s.tab_i), _labels(rng, s, live, s.tab_t)
    ii = ti = None
    if not s.dense:
        ii, ti = rng.integers(0, s.tab_i, s.ri), rng.integers(0, s.tab_t, s.rt)         # with duplicates
    assert s.ri <= s.tab_i and s.rt <= s.tab_t
    return Case(s, live, xi, yi, ii, xt, yt, ti, w, w_proj)


MUTATIONS = ("drop_last_row", "padded_row_dz", "swap_across_seam", "shift_k_chunk", "dh_rounded_twice", "argmax_second_live")


def _segment(case: Case, F: np.ndarray, y: np.ndarray, weight: float, mutation, den: int = G):
    """Forward + CE of one modality's rows F [r, d] (float64): (dZ [r, C], sum of row losses, first-arg-max hits)."""
    s = case.shape
    W = case.w_head.astype(np.float64)
    r = F.shape[0]
    assert_bf16_exact("forward features", F)
    assert np.all(F[:, 0] == 1.0)
    assert_exact_sum("logits", F, W.T, 1.0)
    z = s.scale * (F @ W.T)
    is_live = np.zeros(s.C, dtype=bool)
    is_live[case.live] = True
    zl = z[:, is_live]
    assert np.all(zl == zl[:, :1]), "live logits of a row differ"
    if (~is_live).any():
        assert np.all(z[:, ~is_live] <= zl[:, :1] - 100.0), "a dead logit is less than 100 below the live ones"
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    se = e.sum(axis=1, keepdims=True)
    ce = np.log(se)[:, 0] + (m[:, 0] - z[np.arange(r), y])                       # (the difference of two logits is exact)
    assert np.allclose(ce, np.log(s.live) + np.where(is_live[y], 0.0, 128.0), rtol=0, atol=1e-12)
    p = np.where(is_live, 1.0 / s.live, 0.0)[None, :].repeat(r, axis=0)       # the softmax, exactly ...
    assert np.abs(e / se - p).max(initial=0.0) < 1e-15                            # ... as float64 confirms
    coef = weight * s.scale / den
    onehot = np.zeros_like(p)
    onehot[np.arange(r), y] = 1.0
    dz = coef * (p - onehot)
    assert_bf16_exact("dZ", dz)
    pred = z.argmax(axis=1)                                                       # first maximal index
    if mutation == "argmax_second_live":
        pred = np.where(pred == case.live[0], case.live[1], pred)
    return dz, float(ce.sum()), int((pred == y).sum())


def reference(case: Case, mutation: Optional[str] = None) -> Ref:
    """The step in float64, every exactness condition asserted.  ``mutation``: one of MUTATIONS, the defect a kernel could
    have, applied to the reference's own inputs (tests/test_bf16_exact_cpu.py)."""
    assert mutation is None or mutation in MUTATIONS
    s = case.shape
    f64 = np.float64
    ids_i = (np.arange(s.ri) if case.ii is None else case.ii[:s.ri]).copy()
    ids_t = (np.arange(s.rt) if case.ti is None else case.ti[:s.rt]).copy()
    if mutation == "drop_last_row":
        if len(ids_i):
            ids_i = ids_i[:-1]
        else:
            ids_t = ids_t[:-1]
    if mutation == "swap_across_seam":
        a, b = int(ids_i[-1]), int(ids_t[0])
        ids_i[-1], ids_t[0] = b % s.tab_i, a % s.tab_t
    W = case.w_head.astype(f64)
    assert_bf16_exact("W_head", W)
    assert np.abs(W).max() < 4
    q = ALPHA * abs(s.scale) / max(s.den("img"), s.den("txt")) / s.live   # the quantum of every gradient term (image terms: 2q;
                                                              # own_rows: both coefficients are power-of-two multiples of it)
    g_head = np.zeros((s.C, s.d), dtype=f64)
    terms_head = np.zeros((s.C, s.d), dtype=f64)
    g_proj = None
    out = {}
    for mod, ids, tab, lab, weight in (("img", ids_i, case.xi, case.yi, IMG_ALPHA), ("txt", ids_t, case.xt, case.yt, ALPHA)):
        out[mod] = (0.0, 0)
        if len(ids) == 0:
            continue
        X = tab[ids].astype(f64)
        y = lab[ids]
        assert_bf16_exact(f"{mod} features", X)
        F = X
        if mod == "img" and s.two_layer:
            Wp = case.w_proj.astype(f64)
            assert_bf16_exact("W_proj", Wp)
            h = s.d // 2
            assert not Wp[h:].any() and Wp[0, 0] == 1 and np.abs(Wp[0]).sum() == 1 and not Wp[1:, 0].any()
            assert np.abs(Wp).sum(axis=1).max() <= 16
            assert_exact_sum("H", X, Wp.T, 1.0)
            F = X @ Wp.T
            assert_bf16_exact("H", F)
            assert np.abs(F).max() <= 48 and np.all(F == np.round(F))
        dz, ce_sum, hits = _segment(case, F, y, weight, mutation, s.den(mod))
        out[mod] = (ce_sum, hits)
        Fdw = F
        if mutation == "shift_k_chunk" and mod == "img":         # the second 64-row chunk of the dW operand one row late
            Fdw = F.copy()
            Fdw[64:128] = F[65:129]
        assert_exact_sum(f"dW_head ({mod})", dz.T, Fdw, q)
        terms_head += np.abs(dz.T) @ np.abs(Fdw)
        g_head += dz.T @ Fdw
        if mutation == "padded_row_dz" and mod == "img":         # the row behind the last one, as if it were no padding
            pad = np.where(np.isin(np.arange(s.C), case.live), weight * s.scale / s.den(mod) / s.live, 0.0)
            nxt = tab[(int(ids[-1]) + 1) % tab.shape[0]].astype(f64)
            g_head += np.outer(pad, nxt @ case.w_proj.astype(f64).T if s.two_layer else nxt)
        if mod == "img" and s.two_layer:
            assert_exact_sum("dH", dz, W, q)
            dh = dz @ W
            if mutation == "dh_rounded_twice":                   # half a bf16 ulp added, then rounded to bf16 again
                ulp = np.where(dh != 0, 2.0 ** (np.frexp(dh)[1] - 8.0), 0.0)      # |dh| in [2^(e-1), 2^e): 8 significant bits
                dh = bf16_round(dh + 0.5 * ulp).astype(f64)
            assert_bf16_exact("dH", dh)
            assert_exact_sum("dW_proj", dh.T, X, q)
            g_proj = dh.T @ X
    assert terms_head.max() / q < LIMIT, "dW_head: image and text slabs together"
    g_head32 = assert_f32_exact("dW_head", g_head)
    w_new = assert_f32_exact("W_head - lr g", W - LR * g_head)
    g_proj32 = wp_new = None
    if s.two_layer:
        if g_proj is None:
            g_proj = np.zeros((s.d, s.d_img), dtype=f64)
        g_proj32 = assert_f32_exact("dW_proj", g_proj)
        wp_new = assert_f32_exact("W_proj - lr g", case.w_proj.astype(f64) - LR * g_proj)
    acc = [assert_f32_exact("accuracy", np.asarray(out[m][1] / max(s.den(m), 1), dtype=f64)) for m in ("img", "txt")]
    return Ref(g_head32, g_proj32, out["img"][0] / max(s.den("img"), 1), out["txt"][0] / max(s.den("txt"), 1), np.float32(acc[0]),
               np.float32(acc[1]), w_new, wp_new)


@functools.lru_cache(maxsize=None)
def case_and_reference(s: Shape):
    """(Case, Ref) of a shape, built once and shared by every test that runs it; treat both as read-only."""
    case = make_case(s)
    return case, reference(case)


def mismatches(got: np.ndarray, want: np.ndarray, limit: int = 6):
    """Bit-equality of two fp32 arrays over ALL elements: (count, first few (row, column, got.hex(), want.hex()))."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return len(bad), [(int(r), int(c), float(got[r, c]).hex(), float(want[r, c]).hex()) for r, c in bad[:limit]]
