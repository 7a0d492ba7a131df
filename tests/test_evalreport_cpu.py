"""No-GPU checks of the class-wise validation report: the float64 restatement tests/_evalreport_ref.py against torch CPU float64;
six deliberately wrong restatements are told apart on the case tables; the sharpness constant and the non-sharp cap hold from
the reference side alone; the entry points exist at ABI v11, size their scratch without an n x n_class term and reject every
envelope violation before any HIP call; finetune.train has the switch, off by default."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

import _evalreport_ref as R

E_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_case_table_covers_the_grid():
    cs = R.CASES
    assert {c["n"] for c in cs} == set(R.NS) and {c["d"] for c in cs} == set(R.DS) and {c["k"] for c in cs} == set(R.KS)
    assert {c["scale"] for c in cs} == set(R.SCALES) and {c["bias"] for c in cs} == {False, True}
    for k in R.KS:
        assert {c["C"] for c in cs if c["k"] == k} == {k, k + 8, k + 9, 255, 256, 257, 513}
    assert {(c["d"], c["layout"]) for c in cs} == {(d, lay) for d in R.DS for lay in R.LAYOUTS}
    assert all(c["k"] <= c["C"] for c in cs)
    # both signs of the scale meet a bias, and meet a C beyond the candidate margin
    assert {(c["scale"], c["bias"]) for c in cs} == {(s, b) for s in R.SCALES for b in (False, True)}
    assert {c["scale"] for c in cs if c["C"] > c["k"] + R.MARGIN} == set(R.SCALES)


def test_restatement_against_torch_float64():
    for case in R.CASES:
        x, w, b = R.case_data(case)
        z = R.logits64(x, w, b, case["scale"])
        tz = torch.from_numpy(x).double() @ torch.from_numpy(w).double().T
        if b is not None:
            tz = tz + torch.from_numpy(b).double()
        if case["scale"] is not None:
            tz = case["scale"] * tz
        # two float64 evaluations in different summation orders: each within d 2^-53 of sum_k |x_k w_jk| <= the magnitude
        tol = 2 * (case["d"] + 2) * 2.0 ** -53 * R.magnitude(x, w, b).max() * abs(case["scale"] or 1.0)
        np.testing.assert_allclose(z, tz.numpy(), rtol=0, atol=tol, err_msg=case["name"])
        cls, val = R.topk(x, w, b, case["scale"], case["k"])
        assert len(np.unique(z)) == z.size, case["name"]                      # random data: no ties, torch.topk is unambiguous
        tv, ti = torch.topk(torch.from_numpy(z), case["k"], dim=1)
        assert np.array_equal(cls, ti.numpy()) and np.array_equal(val, tv.numpy()), case["name"]
        y = R.labels_for(case["n"], case["C"], case["seed"])
        rep = R.report(cls, y, case["C"], confusion=True)
        ty, tp, Cn = torch.from_numpy(y), torch.from_numpy(cls[:, 0]), case["C"]
        ok = (ty >= 0) & (ty < Cn)
        assert np.array_equal(rep["support"], torch.bincount(ty[ok], minlength=Cn).numpy())
        assert np.array_equal(rep["hit1"], torch.bincount(ty[ok & (tp == ty)], minlength=Cn).numpy())
        assert np.array_equal(rep["hitk"], torch.bincount(ty[ok & (torch.from_numpy(cls) == ty[:, None]).any(1)], minlength=Cn).numpy())
        assert np.array_equal(rep["confusion"], torch.bincount(ty[ok] * Cn + tp[ok], minlength=Cn * Cn).reshape(Cn, Cn).numpy())
        assert rep["misc"].tolist() == [int((~ok).sum()), 0]
        assert rep["confusion"].sum() == case["n"] - rep["misc"].sum() and np.array_equal(np.diag(rep["confusion"]), rep["hit1"])


def test_nan_rows_and_open_slots_of_the_restatement():
    rng = np.random.default_rng(3)
    x, w = rng.standard_normal((4, 6)).astype(np.float32), rng.standard_normal((20, 6)).astype(np.float32)
    x[1, 0] = np.nan
    cls, val = R.topk(x, w, None, None, 5)
    assert (cls[1] == -1).all() and np.isnan(val[1]).all() and (cls[[0, 2, 3]] >= 0).all()
    rep = R.report(cls, cls[:, 0].clip(0), len(w))                       # every row labelled with its own best class (row 1: class 0)
    assert rep["misc"].tolist() == [0, 1] and rep["support"].sum() == 4 and rep["hit1"].sum() == rep["hitk"].sum() == 3
    w[7] = np.nan                                                        # a NaN weight row is a class that is never listed
    w2 = w[:6]
    w2[2] = np.nan
    cls, val = R.topk(x[[0]], w2, None, None, 6)
    assert sorted(cls[0, :5]) == [0, 1, 3, 4, 5] and cls[0, 5] == -1 and np.isnan(val[0, 5])


@pytest.mark.parametrize("variant", R.TOPK_VARIANTS + R.REPORT_VARIANTS)
def test_wrong_variants_are_told_apart(variant):
    caught = 0
    if variant == "tie_larger_index":                                   # ties are certain only on integer-valued data
        for name, (x, w, b, scale, k) in R.integer_cases().items():
            caught += not np.array_equal(R.topk(x, w, b, scale, k)[0], R.topk(x, w, b, scale, k, variant)[0])
        assert caught == len(R.integer_cases())
        return
    for case in R.CASES:
        x, w, b = R.case_data(case)
        cls, _ = R.topk(x, w, b, case["scale"], case["k"])
        if variant in R.TOPK_VARIANTS:
            differs = not np.array_equal(cls, R.topk(x, w, b, case["scale"], case["k"], variant)[0])
            if variant == "bias_dropped" and case["bias"] and case["C"] > case["k"]:
                assert differs, case["name"]
            if variant == "scale_sign_ignored" and case["scale"] is not None and case["scale"] < 0 and case["C"] > 1:
                assert differs, case["name"]
        else:
            y = R.labels_for(case["n"], case["C"], case["seed"])
            good, bad = R.report(cls, y, case["C"], True), R.report(cls, y, case["C"], True, variant)
            differs = any(not np.array_equal(good[key], bad[key]) for key in good)
            if variant == "bad_labels_counted" and case["n"] >= 4:
                assert differs, case["name"]
        caught += differs
    assert caught >= 1, variant
    if variant in ("confusion_transposed", "hitk_short"):               # every case with rows enough to show it
        assert caught >= len(R.CASES) // 3, (variant, caught)


def test_sharpness_constant_and_cap():
    worst = 0.0
    for case in R.CASES:
        x, w, b = R.case_data(case)
        err = R.stage1_error(x, w, b)
        blunt = int((~R.sharp(x, w, b, case["k"], case["scale"])).sum())
        print(f"{case['name']} n={case['n']} C={case['C']} d={case['d']} k={case['k']}: fp32 stage-1 error "
              f"2^{math.log2(err) if err > 0 else -math.inf:.2f} of the magnitude, non-sharp {blunt} of {case['n']}")
        assert blunt <= R.CAP * case["n"], case["name"]
        worst = max(worst, err)
    print(f"largest 2^{math.log2(worst):.2f}")
    assert 2.0 ** math.ceil(math.log2(8 * worst)) == R.TAU
    x, w, b = R.case_data(R.CASES[0])
    assert R.sharp(x, w[:9], None, 1).all()                                      # C <= kc: every row is sharp


def test_symbols_exist_and_the_version_stays(lib):
    import umlh
    from umlh import _lib
    assert lib.umlh_version() == 11
    for name in ("umlh_eval_topk_scratch_bytes", "umlh_eval_topk", "umlh_eval_classwise"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert umlh.topk_classes is umlh.report.topk_classes and umlh.class_report is umlh.report.class_report
    assert "umlh_kernels_evalreport.hip" in _lib.SOURCES


def test_scratch_query(lib):
    q = lib.umlh_eval_topk_scratch_bytes
    for args in ((100, 10, 8, 0, 0), (100, 30, 8, 25, 0), (100, 4, 8, 5, 0), (100, 10, 0, 5, 0), (100, 10, 8, 5, -1), (0, 10, 8, 5, 0),
                 (1 << 31, 10, 8, 5, 0), (100, 1 << 31, 8, 5, 0), (100, 0, 8, 5, 0), (-1, 10, 8, 5, 0)):
        assert q(*args) == 0, args
    assert q(1, 5, 1, 5, 0) > 0                                                   # n_class == k
    assert q(64, 4096, 8, 5, 1) < q(64, 4096, 8, 5, 2) < q(64, 4096, 8, 5, 4)     # grows with splits
    assert q(64, 4096, 8, 5, 16) == q(64, 4096, 8, 5, 1000)                       # (at most one chunk per 256-column tile)
    # linear in n: the lists (kc <= 32 entries of two words per chunk and row) and the candidates, nothing else
    for splits in (1, 8):
        a, b2 = q(50000, 1000, 512, 24, splits), q(100000, 1000, 512, 24, splits)
        assert 0 < a < b2 <= 2 * a + 3 * 256, (splits, a, b2)
        assert b2 <= 100000 * 32 * 4 * (2 * splits + 1) + 3 * 256
    # auto mode: splits * n <= n + 32 * 512, so still linear in n, and no n * n_class term -- the class count enters through the
    # number of chunks alone, which the tile count caps: a thousand times the classes never costs more than the chunk cap allows
    for n in (1, 2500, 50000, 10 ** 6):
        small, large = q(n, 1000, 512, 5, 0), q(n, 10 ** 6, 512, 5, 0)
        assert 0 < small <= large <= (n + 32 * 512 + 32) * 13 * 4 * 2 + n * 13 * 4 + 3 * 256, (n, small, large)
    n = 10 ** 6
    assert q(n, n, 1024, 24, 0) <= n * 32 * 4 * 3 + 3 * 256                      # a million rows by a million classes: 384 MB, not 4 TB
    assert q(2 * n, n, 1024, 24, 0) <= 2 * q(n, n, 1024, 24, 0) and q(n, 2 * n, 1024, 24, 0) <= 2 * q(n, n, 1024, 24, 0)


def test_envelope_violations_are_invalid_before_any_hip_call(lib):
    fake = C.c_void_p(256)                                   # never dereferenced: every check comes first
    big = 1 << 40

    def topk(n=10, ldx=8, nc=100, ldw=8, d=8, k=5, splits=0, x=fake, w=fake, cls=fake, scratch=fake, nbytes=big):
        return lib.umlh_eval_topk(x, n, ldx, w, nc, ldw, d, None, None, k, splits, cls, None, scratch, nbytes, None)

    for kw, arg in ((dict(k=0), b"k="), (dict(k=25), b"k="), (dict(k=5, nc=4), b"n_class="), (dict(d=0), b"d="), (dict(ldx=7), b"ldx="),
                    (dict(ldw=7), b"ldw="), (dict(splits=-1), b"splits="), (dict(n=0), b"n="), (dict(n=1 << 31), b"n="),
                    (dict(nc=1 << 31), b"n_class="), (dict(x=None), b"x"), (dict(w=None), b"w"), (dict(cls=None), b"cls"),
                    (dict(scratch=None), b"scratch"), (dict(nbytes=16), b"scratch_bytes="),
                    (dict(scratch=C.c_void_p(258)), b"scratch")):
        assert topk(**kw) == E_INVALID, kw
        msg = lib.umlh_last_error()
        assert b"umlh_eval_topk" in msg and arg in msg, (kw, msg)

    def classwise(n=10, k=5, nc=100, cls=fake, labels=fake, support=fake, hit1=fake, hitk=fake, misc=fake):
        return lib.umlh_eval_classwise(cls, n, k, labels, nc, support, hit1, hitk, None, misc, None)

    for kw, arg in ((dict(k=0), b"k="), (dict(k=25), b"k="), (dict(n=0), b"n="), (dict(n=1 << 31), b"n="), (dict(nc=0), b"n_class="),
                    (dict(nc=1 << 31), b"n_class="), (dict(cls=None), b"cls"), (dict(labels=None), b"labels"),
                    (dict(support=None), b"support"), (dict(hit1=None), b"hit1"), (dict(hitk=None), b"hitk"), (dict(misc=None), b"misc2")):
        assert classwise(**kw) == E_INVALID, kw
        msg = lib.umlh_last_error()
        assert b"umlh_eval_classwise" in msg and arg in msg, (kw, msg)


def test_python_surface():
    import finetune as ft
    from engine.models.head import UML, UMLClip
    p = inspect.signature(ft.train).parameters["classwise"]
    assert p.default is False
    sig = inspect.signature(ft.validate_classwise)
    assert sig.parameters["topk"].default == 5 and sig.parameters["confusion"].default is False
    assert ft._classwise_kwargs(False) is None and ft._classwise_kwargs(None) is None
    assert ft._classwise_kwargs(True) == {} and ft._classwise_kwargs({"topk": 3}) == {"topk": 3}
    for cls in (UML, UMLClip):
        assert inspect.signature(cls.predict_topk).parameters["k"].default == 5
