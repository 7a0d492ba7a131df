"""CPU: the float64 reference of the standalone optimizer entry points (tests/_optstep_ref.py) is itself pinned -- against
oracle/uml_oracle.py: optimizer_step and torch.optim in float64 over five steps -- and the criterion it carries is shown to be
calibrated (the levels of the module docstring re-measured) and to discriminate (every deliberately wrong variant breaks the bound
by 8x or more).  No GPU, no `umlh` import."""
import re

import numpy as np
import pytest
import torch

import _optstep_ref as O
from oracle import uml_oracle as UO

F32, F64 = np.float32, np.float64


def _five_steps(kind, wd, seed=0):
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal((6, 5))
    grads = [rng.standard_normal((6, 5)) * 10.0 ** rng.uniform(-2, 1) for _ in range(5)]
    return p0, grads


@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("wd", O.WDS)
def test_opt_ref_equals_the_oracle_and_torch_over_five_steps(kind, wd):
    p0, grads = _five_steps(kind, wd)
    # opt_ref, fresh state
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    # the oracle (float64 state)
    st, ost = UO.HeadState(p0.copy()), UO.OptState(kind, wd)
    assert (UO.ADAM_BETAS, UO.ADAM_EPS, UO.SGD_MOMENTUM) == (O.BETAS, O.EPS, O.MOMENTUM)
    # torch.optim (float64)
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    topt = {"sgd": lambda: torch.optim.SGD([tp], lr=O.LR, momentum=O.MOMENTUM, weight_decay=wd),
            "adam": lambda: torch.optim.Adam([tp], lr=O.LR, betas=O.BETAS, eps=O.EPS, weight_decay=wd),
            "adamw": lambda: torch.optim.AdamW([tp], lr=O.LR, betas=O.BETAS, eps=O.EPS, weight_decay=wd)}[kind]()
    for k, g in enumerate(grads):
        p, m, v = O.opt_ref(kind, p, g, m, v, O.LR, k + 1, wd=wd)
        UO.optimizer_step(st, {"w_head": g}, ost, O.LR)
        tp.grad = torch.from_numpy(g.copy())
        topt.step()
        for other in (st.w_head, tp.detach().numpy()):
            assert np.abs(p - other).max() <= 1e-13 * max(1.0, np.abs(p).max()), (kind, wd, k)
    assert np.abs(m - ost.m["w_head"]).max() <= 1e-13 * np.abs(m).max()
    if kind != "sgd":
        assert np.abs(v - ost.v["w_head"]).max() <= 1e-13 * np.abs(v).max()


@pytest.mark.parametrize("kind", O.KINDS)
def test_kernel_form_in_float64_is_the_reference_up_to_its_fp32_constants(kind):
    data = O.build_data(O.N_LEVEL, 0)
    for wd, step in O.settings():
        got = O.kernel_form(kind, *data, O.LR, step, wd=wd)
        for o, e in O.errors_against_ref(kind, got, data, wd, step).items():
            assert e <= O.LEVELS_ULP[kind][o], (kind, wd, step, o, e)       # the constants' roundings alone stay inside the level
    # step < 1 is step 1, in both references
    for a, b in zip(O.kernel_form(kind, *data, O.LR, 0, wd=0.1), O.kernel_form(kind, *data, O.LR, 1, wd=0.1)):
        assert np.array_equal(a, b)
    for a, b in zip(O.opt_ref(kind, *data, O.LR, -3, wd=0.1), O.opt_ref(kind, *data, O.LR, 1, wd=0.1)):
        assert np.array_equal(a, b)
    if kind == "sgd":
        assert O.opt_ref(kind, data[0], data[1], data[2], None, O.LR, 1)[2] is None
        assert np.array_equal(O.opt_ref(kind, *data, O.LR, 1)[2], data[3].astype(F64))      # v is left alone


def test_the_data_reaches_the_regimes_the_criterion_names():
    p, g, m, v = O.build_data(O.N_LEVEL, 0)
    assert np.log10(np.abs(p).max() / np.abs(p).min()) > 5.5 and np.log10(np.abs(g[np.abs(g) > 1e-4]).max() / np.abs(g[np.abs(g) > 1e-4]).min()) > 5.5
    small = np.abs(g) < 1e-7
    assert small.sum() >= O.N_LEVEL // 8 and (np.sqrt(v[small]) < 10 * O.EPS).all()       # eps decides the step there
    assert (m != 0).all() and (v > 0).all() and (p < 0).any() and (g < 0).any()


def test_levels_of_the_docstring_are_remeasured_and_under_their_bounds():
    lv = O.measure_levels()
    rows = {(r[1], r[2]): (float(r[3]), int(r[4])) for r in re.finditer(r"(sgd|adam|adamw) +([pmv]) +(\d+\.\d+) +(\d+)", O.__doc__)}
    assert set(rows) == {(k, o) for k in O.KINDS for o in O.outputs_of(k)}
    for kind, d in lv.items():
        for o, e in d.items():
            rec = O.LEVELS_ULP[kind][o]
            assert e <= rec * 1.01 and e >= rec * 0.5, (kind, o, e, rec)
            assert 8 * rec <= O.BOUNDS[kind][o] < 16 * rec
            assert rows[kind, o] == (rec, int(O.BOUNDS[kind][o])), (kind, o, rows[kind, o])


@pytest.mark.parametrize("name", O.WRONG_VARIANTS)
def test_every_wrong_variant_breaks_the_bound_by_8x(name):
    assert O.variant_excess(name) >= 8.0, name


def test_case_tables():
    assert O.SINGLE_N == (0, 1, 3, 4, 5, 1023, 1024, 1025, 4099)
    lists = O.multi_lists()
    assert [lists[k] for k in ("one_empty", "one", "empty_between", "empty_first", "empty_last", "block_edges")] == \
        [[0], [1], [1024, 0, 5], [0, 5], [5, 0], [1025, 1023, 1]]
    for k in (48, 49, 70, 97):
        n = lists[f"tensors_{k}"]
        assert len(n) == k and min(n) == 0 and max(n) <= 3000 and n[0] == 0 and sum(1 for x in n if x) > k // 2
        assert n[-1] == (3000 if k == 49 else 0)              # (49: the second launch is one full tensor)
        if k > O.MULTI_MAX:
            assert n[O.MULTI_MAX - 1] == 0 and n[O.MULTI_MAX] == 3000
    # (t, e) -> p is exact and injective over the tables
    seen = np.concatenate([O.encode_p(t, 3000) for t in range(97)])
    assert np.unique(seen).size == seen.size
    assert np.array_equal(O.encode_p(96, 3000).astype(F64), 97 + np.arange(3000) / 4096.0)


def test_bf16_specials_cover_ties_and_non_finite_values():
    bits = O.bf16_specials()
    lo, kept = bits & 0xFFFF, (bits >> 16) & 1
    finite = ((bits >> 23) & 0xFF) != 0xFF
    for k in (0, 1):
        for s in (0, 1):
            assert ((lo == 0x8000) & (kept == k) & ((bits >> 31) == s) & finite).any()      # a tie, kept bit even / odd, each sign
    x = bits.view(F32)
    assert np.isinf(x).sum() == 2 and np.isnan(x).sum() >= 8 and (bits == 0x80000000).any() and (bits == 0).any()
    assert ((x != 0) & (np.abs(x) < np.finfo(F32).tiny)).sum() >= 6 and (bits == 0x7F7FFFFF).any()
    # torch's conversion is round-to-nearest-even on exactly these: the GPU test's reference
    t = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    tie = (lo == 0x8000) & finite
    up = ((bits[tie] >> 16) + kept[tie]).astype(np.uint16)
    assert np.array_equal(t[tie], up)
    assert t[bits == 0x7F7FFFFF][0] == 0x7F80 and t[bits == 0xFF7FFFFF][0] == 0xFF80      # the largest float rounds to inf
    for n in O.BF16_N:
        assert O.build_bf16_input(n).size == n
