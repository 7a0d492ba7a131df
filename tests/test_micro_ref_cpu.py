"""CPU: tests/_micro_ref.py, the float64 statement of one micro step and the bounds tests/test_micro_kernels_gpu.py applies.
(a) The statement is pinned: it agrees with oracle/uml_oracle.py (step_grads + optimizer_step) and with torch float64 autograd
(F.cross_entropy, torch.optim single-tensor forms) to 1e-12; (b) every level of the calibration table is re-measured and lies
under its bound by the stated 8 x; (c) each wrong variant, turned on in the fp32 restatement at a GPU case, breaks a bound by
8 x or more; (d) the exact bf16 construction meets its representability conditions at every exact shape; (e) the envelope
restated in Python is the library's and the header's."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bf16_exact_ref as X
import _micro_ref as R
from conftest import ROOT
from oracle import uml_oracle as O

PIN_CASES = [
    # d, C, rows_img, rows_txt, kind, learnable, step
    (48, 37, 17, 30, "adamw", True, 1),
    (128, 100, 32, 32, "adam", True, 1000),
    (80, 37, 64, 0, "sgd", True, 2),
    (256, 17, 0, 64, "adamw", True, 2),
    (16, 2, 1, 1, "sgd", False, 1),
    (96, 37, 20, 30, "adam", False, 2),
]


def _pin_inputs(d, C, ri, rt, kind, learn, step):
    tab, ii, ti = R.build_case(d, C, ri, rt, "small")
    mods = R.step_mods(tab, ii, ti)
    g0 = R.grad64(R.probe_state(tab), mods, R.WEIGHTS)
    st = R.live_state(tab, g0["dW"], 1)
    return mods, st


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


@pytest.mark.parametrize("d,C,ri,rt,kind,learn,step", PIN_CASES)
def test_reference_agrees_with_the_oracle(d, C, ri, rt, kind, learn, step):
    mods, st = _pin_inputs(d, C, ri, rt, kind, learn, step)
    wd = R.KIND_WD[kind]
    g, new = R.step64(st, mods, R.WEIGHTS, kind, R.LR, step, wd, learn)
    hs = O.HeadState(st["W"].astype(np.float64), None, float(st["scales"][0]), float(st["scales"][1]), learn)
    xs = [None if m is None else m[0].astype(np.float64) for m in mods]
    ys = [None if m is None else m[1] for m in mods]
    so = O.step_grads(hs, xs[0], ys[0], xs[1], ys[1], R.ALPHA, R.IMG_ALPHA)
    assert _rel(g["dW"], so.grads["w_head"]) < 1e-12
    for mod, (loss, acc, name) in enumerate(((so.loss_img, so.acc_img, "img_scale"), (so.loss_txt, so.acc_txt, "txt_scale"))):
        if not g["present"][mod]:
            assert g["scalars"][mod] == 0 and name not in so.grads
            continue
        assert abs(g["scalars"][R.S_LOSS_IMG + mod] - loss) <= 1e-12 * max(1.0, abs(loss))
        assert g["scalars"][R.S_ACC_IMG + mod] == acc
        if learn:
            assert abs(g["scalars"][R.S_GSCALE_IMG + mod] - float(so.grads[name])) <= 1e-12 * max(1.0, abs(float(so.grads[name])))
    opt = O.OptState(kind, wd, step - 1)
    names = {"w_head": ("W", "m", "v", None), "img_scale": ("scales", "m_scales", "v_scales", 0), "txt_scale": ("scales", "m_scales", "v_scales", 1)}
    for n in hs.param_names():
        _, km, kv, i = names[n]
        opt.m[n] = np.asarray(st[km] if i is None else st[km][i], np.float64)
        opt.v[n] = np.asarray(st[kv] if i is None else st[kv][i], np.float64)
    O.optimizer_step(hs, so.grads, opt, R.LR)
    assert _rel(new["W"], hs.w_head) < 1e-12 and _rel(new["m"], opt.m["w_head"]) < 1e-12
    if kind != "sgd":
        assert _rel(new["v"], opt.v["w_head"]) < 1e-12
    else:
        assert np.array_equal(new["v"], st["v"].astype(np.float64)) and np.array_equal(new["v_scales"], st["v_scales"].astype(np.float64))
    assert _rel(new["scales"], [hs.img_scale, hs.txt_scale]) < 1e-12
    for mod, n in enumerate(("img_scale", "txt_scale")):
        if learn and g["present"][mod]:
            assert abs(new["m_scales"][mod] - float(opt.m[n])) <= 1e-12 * abs(float(opt.m[n]))
        else:                                              # fixed scales, or a modality without rows: nothing moves
            assert all(new[k][mod] == np.float64(st[k][mod]) for k in ("scales", "m_scales", "v_scales"))


@pytest.mark.parametrize("d,C,ri,rt,kind,learn,step", PIN_CASES)
def test_reference_agrees_with_torch_autograd(d, C, ri, rt, kind, learn, step):
    mods, st = _pin_inputs(d, C, ri, rt, kind, learn, step)
    wd = R.KIND_WD[kind]
    g, new = R.step64(st, mods, R.WEIGHTS, kind, R.LR, step, wd, learn)
    T = lambda a: torch.tensor(np.asarray(a, np.float64))
    W = T(st["W"]).requires_grad_()
    sc = [T(st["scales"][k]).requires_grad_(learn) for k in (0, 1)]
    loss = 0.0
    for mod, w in enumerate(R.WEIGHTS):
        if g["present"][mod]:
            ce = F.cross_entropy((T(mods[mod][0]) @ W.T) * sc[mod], torch.as_tensor(mods[mod][1]))
            assert abs(float(ce.detach()) - g["scalars"][R.S_LOSS_IMG + mod]) <= 1e-12 * max(1.0, float(ce.detach()))
            loss = loss + w * ce
    params = [W] + (sc if learn else [])
    if kind == "sgd":
        opt = torch.optim.SGD(params, lr=R.LR, momentum=0.9, weight_decay=wd, foreach=False)
    else:
        opt = (torch.optim.Adam if kind == "adam" else torch.optim.AdamW)(params, lr=R.LR, weight_decay=wd, foreach=False)
    moments = [(st["m"], st["v"])] + [(st["m_scales"][k], st["v_scales"][k]) for k in (0, 1)]
    for p, (m, v) in zip(params, moments):
        if kind == "sgd":
            opt.state[p] = {"momentum_buffer": T(m).clone()}
        else:
            opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": T(m).clone(), "exp_avg_sq": T(v).clone()}
    loss.backward()
    assert _rel(g["dW"], W.grad.numpy()) < 1e-12
    for mod in (0, 1):
        if learn and g["present"][mod]:
            assert abs(g["scalars"][R.S_GSCALE_IMG + mod] - float(sc[mod].grad)) <= 1e-12 * max(1.0, abs(float(sc[mod].grad)))
        else:
            assert sc[mod].grad is None
    opt.step()
    assert _rel(new["W"], W.detach().numpy()) < 1e-12
    key = "momentum_buffer" if kind == "sgd" else "exp_avg"
    assert _rel(new["m"], opt.state[W][key].numpy()) < 1e-12
    if kind != "sgd":
        assert _rel(new["v"], opt.state[W]["exp_avg_sq"].numpy()) < 1e-12
    assert _rel(new["scales"], [float(sc[0].detach()), float(sc[1].detach())]) < 1e-12
    for mod in (0, 1):
        if learn and g["present"][mod]:
            assert abs(new["m_scales"][mod] - float(opt.state[sc[mod]][key])) <= 1e-12 * abs(float(opt.state[sc[mod]][key]))
            if kind != "sgd":
                assert abs(new["v_scales"][mod] - float(opt.state[sc[mod]]["exp_avg_sq"])) <= 1e-12 * float(opt.state[sc[mod]]["exp_avg_sq"])


def test_bf16_statement_rounds_the_operands_and_nothing_else():
    """On operands that are bf16 numbers already the bf16 statement differs from the fp32 one only through dZ's rounding in
    the dW product: the same scalars, and a gradient within 2^-9 of every term."""
    tab, ii, ti = R.build_case(128, 37, 17, 30, "small")
    tabq = dict(tab, xi=R.bf(tab["xi"]).astype(np.float32), xt=R.bf(tab["xt"]).astype(np.float32), W=R.bf(tab["W"]).astype(np.float32))
    mods, st = R.step_mods(tabq, ii, ti), R.probe_state(tabq)
    a, b = R.grad64(st, mods, R.WEIGHTS, bf16=False), R.grad64(st, mods, R.WEIGHTS, bf16=True)
    assert np.array_equal(a["scalars"], b["scalars"])                         # the forward saw the same numbers
    mx, _ = R.grad_err(b["dW"], a)
    assert 0 < mx <= 2.0 ** -9                                                # dZ rounded to 8 significant bits: 2^-9 of every term


@pytest.mark.parametrize("mode,regime", [(m, r) for m in ("fp32", "bf16") for r in R.REGIMES])
def test_levels_lie_under_their_bounds(mode, regime):
    lv = R.measure_levels(mode, regime)
    table = R.LEVELS[(mode, regime)]
    assert set(lv) == set(table)
    for k, v in lv.items():
        print(f"{mode:5s} {regime:6s} {k:14s} level {v:10.4g}  table {table[k]:10.4g}  bound {R.bound(mode, regime, k):10.4g}")
        assert v <= table[k] * (1 + 1e-9), (k, v, table[k])                   # the table is the measurement, rounded up
        assert 8.0 * v <= R.bound(mode, regime, k), (k, v)


@pytest.mark.parametrize("name", R.WRONG_VARIANTS)
def test_wrong_variants_break_a_bound(name):
    worst = [R.variant_excess(name, **c) for c in R.VARIANT_CASES[name]]
    print(f"{name}: error / bound per case {['%.3g' % w for w in worst]}")
    assert max(worst) >= 8.0


def test_the_unmodified_restatement_meets_every_bound_at_the_variant_cases():
    """The control of the test above: with no variant switched on, the same cases stay under their bounds."""
    seen = set()
    for cases in R.VARIANT_CASES.values():
        for c in cases:
            key = tuple(sorted(c.items()))
            if key not in seen:
                seen.add(key)
                assert R.variant_excess("none", **c) <= 1.0, c


@pytest.mark.parametrize("shape", R.exact_shapes(), ids=lambda s: s.id)
def test_exact_construction_holds_on_the_micro_denominators(shape):
    case, ref = X.case_and_reference(shape)              # (every representability condition is asserted inside)
    s = shape
    assert len(case.live) == s.live and case.live.min() >= s.live_from
    assert R.eligible(s.d, s.C, s.ri, s.rt, bf16=True)
    assert np.abs(ref.g_head).max() > 0 and X.mismatches(ref.w_head_new, case.w_head)[0] > 0
    for rows, acc in ((s.ri, ref.acc_img), (s.rt, ref.acc_txt)):
        assert float(acc) * max(rows, 1) == round(float(acc) * max(rows, 1)) <= rows


def test_exact_shapes_cover_every_width_pattern_and_live_set():
    shapes = R.exact_shapes()
    assert {s.d for s in shapes} == set(R.WIDTHS_BF16)
    assert {(s.ri, s.rt) for s in shapes} >= set(R.EXACT_PATTERNS)
    for d in R.WIDTHS_BF16:
        assert {(s.live, s.live_from) for s in shapes if s.d == d} >= set(R.EXACT_LIVE)
    for p in R.EXACT_PATTERNS:
        assert {(s.live, s.live_from) for s in shapes if (s.ri, s.rt) == p and s.C == R.EXACT_C} >= set(R.EXACT_LIVE)
    assert sum(s.scale < 0 for s in shapes) == 1
    assert any(s.live_from // 16 == 1 for s in shapes) and any(s.live_from // 16 == (s.C - 1) // 16 for s in shapes)


# ---- the envelope ----
def test_envelope_matches_the_header():
    text = open(os.path.join(ROOT, "include", "umlh.h")).read()
    m = re.search(r"fp32: d in \{([0-9,\s]+)\}", text)
    assert m, "the header no longer lists the widths of the micro path"
    assert tuple(int(v) for v in m.group(1).split(",")) == R.WIDTHS_F32
    assert "the multiples of 128 among them" in re.sub(r"\s*\*\s*", " ", text)
    assert R.WIDTHS_BF16 == tuple(d for d in R.WIDTHS_F32 if d % 128 == 0) and len(R.WIDTHS_F32) == 13 and len(R.WIDTHS_BF16) == 7
    assert "ceil(rows_img/16) + ceil(rows_txt/16) <= 4" in text
    # chunks: the widest power-of-two chunk <= 128 dividing d, at most 8 of them and never 7
    for d, (nch, cw) in R.CHUNKING.items():
        assert nch * cw == d and cw in (16, 32, 64, 128) and (cw == 128 or d % (2 * cw)) and nch in (1, 2, 3, 4, 5, 6, 8)
    for ri, rt, ok in ((32, 32, True), (17, 30, True), (17, 47, False), (49, 15, False), (64, 0, True), (0, 64, True), (0, 0, False),
                       (1, 48, True), (33, 16, True), (16, 48, True)):
        assert R.eligible(128, 37, ri, rt) == ok, (ri, rt)
    assert R.eligible(128, 1024, 8, 8) and not R.eligible(128, 1025, 8, 8)
    assert not R.eligible(192, 37, 8, 8) and R.eligible(96, 37, 8, 8) and not R.eligible(96, 37, 8, 8, bf16=True)


def test_envelope_matches_the_library():
    import umlh
    umlh.build_library()
    lib = umlh.load_library()
    for d in range(1, 1101):
        nch, cw = C.c_int(-1), C.c_int(-1)
        ok = lib.umlh_micro_chunking(C.c_int(d), C.byref(nch), C.byref(cw))
        assert bool(ok) == (R.chunking(d) is not None), d
        if ok:
            assert (nch.value, cw.value) == R.chunking(d), d
            assert bool(lib.umlh_micro_bf16_supported(nch, cw)) == R.bf16_supported(d), d
    for nch in range(0, 10):
        for cw in (16, 32, 64, 128, 256):
            want = cw == 128 and nch * cw in R.CHUNKING
            assert bool(lib.umlh_micro_bf16_supported(C.c_int(nch), C.c_int(cw))) == want, (nch, cw)


def test_row_loss_must_subtract_the_label_logit_before_adding_the_log():
    """(log S + max) - z_y rounds at the ulp of the largest logit -- 2^-12 for logits in the thousands, as on the exact
    shapes -- and misses their 1e-5 tolerance at small row counts; log S + (max - z_y), what the kernels compute, keeps it."""
    worst = {(): 0.0, (R.LOSS_MAX_FIRST,): 0.0}
    for s in R.exact_shapes():
        if (s.ri, s.rt) not in ((1, 1), (8, 8)):
            continue
        case, ref = X.case_and_reference(s)
        tab = dict(xi=case.xi, yi=case.yi, xt=case.xt, yt=case.yt)
        st = R.make_state(case.w_head, scales=(s.scale, s.scale))
        mods = R.step_mods(tab, case.ii, case.ti)
        for wrong in worst:
            sc = R.grad32(st, mods, (X.IMG_ALPHA, X.ALPHA), bf16=True, wrong=wrong)["scalars"]
            for k, want in ((R.S_LOSS_IMG, ref.loss_img), (R.S_LOSS_TXT, ref.loss_txt)):
                worst[wrong] = max(worst[wrong], abs(sc[k] - want) / max(1.0, abs(want)))
    print(f"loss error on the exact shapes: {worst[()]:.2e}; with (log S + max) - z_y: {worst[(R.LOSS_MAX_FIRST,)]:.2e}")
    assert worst[()] <= 1e-5 < worst[(R.LOSS_MAX_FIRST,)]
