"""CPU checks of the outlier clamp: the float64 statement of tests/_outlier_ref.py reproduces the reference's recorded results
(tests/golden/outliers.npz, written by scripts/make_golden_outliers.py), its bounds table is what this test measures, every
wrong variant misses a bound by 8 x, and the Python wrappers, the prototype table and the library carry the new names."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _outlier_ref as R
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("umlh_outlier_scratch_bytes", "umlh_row_abs_quantile", "umlh_abs_kth", "umlh_clamp_rows", "umlh_knn_accuracy")


@pytest.fixture(scope="module")
def gold():
    return load_golden("outliers")


def cases(g, exact=None):
    for name in g["cases"]:
        ex = int(g[f"{name}/exact"])
        if exact is None or ex == int(exact):
            yield str(name), g[f"{name}/x"], float(g[f"{name}/q"]), ex


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def test_fixture_covers_the_issue_cases(gold):
    names = [c[0] for c in cases(gold)]
    assert len(names) == 26 and {float(gold[f"{n}/q"]) for n in names} == {0.5, 0.95, 0.999}
    assert any(gold[f"{n}/x"].ndim == 3 for n in names)
    for what in ("nan_", "inf_", "negzero_", "heavy_", "gauss_"):
        assert any(n.startswith(what) for n in names), what
    assert gold["knn2"].ndim == 2 and gold["knn3"].ndim == 3


def test_exact_bound_and_clamp_are_bit_equal(gold):
    for name, x, q, _ in cases(gold, exact=1):
        mine = R.abs_kth(x, R.exact_index(q, x.size))
        assert np.array_equal(bits(mine), bits(gold[f"{name}/q_val"])), name
        assert np.array_equal(bits(R.remove_outliers(x, q, True)), bits(gold[f"{name}/out"])), name


def test_clamp_at_the_recorded_bound_is_bit_equal(gold):
    """-0.0, +-Inf, NaN elements and a NaN or zero bound: the statement's clamp is the reference's, bit for bit."""
    for name, x, q, _ in cases(gold):
        assert np.array_equal(bits(R.clamp(x, gold[f"{name}/q_val"])), bits(gold[f"{name}/out"])), name
    out = gold["negzero_6x9_q50_rows/out"]
    assert np.signbit(out[0, :4]).all() and (out[0, :4] == 0).all()          # -0.0 stays -0.0
    assert np.isnan(gold["nan_5x16_q50_rows/out"]).all()                     # NaN bound: everything NaN
    x, out = gold["nan_5x16_q50_exact/x"], gold["nan_5x16_q50_exact/out"]
    assert np.array_equal(np.isnan(out), np.isnan(x)) and np.isnan(x).sum() == 1
    x, out, qv = (gold[f"inf_5x16_q95_exact/{k}"] for k in ("x", "out", "q_val"))
    assert out[1, 3] == qv and out[4, 0] == -qv and np.isfinite(qv)


def measured(gold):
    wq = wv = wn = 0.0
    for name, x, q, ex in cases(gold):
        out = gold[f"{name}/out"]
        if not ex:
            r = R.row_quantile(x, q)
            wq = max(wq, R.rel_diff(gold[f"{name}/rowq"], r["quant"]))
            wv = max(wv, R.rel_diff(gold[f"{name}/q_val"], r["q_val"]))
        if np.isfinite(out).all():
            wn = max(wn, R.max_rel(R.normalize32(out), R.normalize64(out)))
    return wq, wv, wn


def test_bounds_table_is_what_the_golden_cases_measure(gold):
    wq, wv, wn = measured(gold)
    print(f"worst relative difference: quant {wq:.3e} (2^{math.log2(wq):.1f}), q_val {wv:.3e} (2^{math.log2(wv):.1f}), "
          f"fp32 normalise {wn:.3e} (2^{math.log2(wn):.1f})")
    assert R.QUANT_BOUND == R.pow2_ceil(8 * wq)
    assert R.QVAL_BOUND == R.pow2_ceil(8 * wv)
    assert R.NORM_BOUND == R.pow2_ceil(8 * wn)
    doc = R.__doc__
    for v, b in ((wq, R.QUANT_BOUND), (wv, R.QVAL_BOUND), (wn, R.NORM_BOUND)):
        assert f"2^{math.log2(v):.1f} ({v:.2e})" in doc and f"= 2^{int(math.log2(b))}" in doc


def test_statement_reproduces_the_reference_within_the_bounds(gold):
    for name, x, q, _ in cases(gold, exact=0):
        r = R.row_quantile(x, q)
        assert R.rel_diff(gold[f"{name}/rowq"], r["quant"]) <= R.QUANT_BOUND, name
        assert R.rel_diff(gold[f"{name}/q_val"], r["q_val"]) <= R.QVAL_BOUND, name
        out, ref = R.remove_outliers(x, q), gold[f"{name}/out"]
        qv = float(gold[f"{name}/q_val"])
        if np.isfinite(qv):          # only the elements AT the bound may differ, by the bound's own difference
            fin = np.isfinite(ref)
            assert np.array_equal(np.isnan(out), np.isnan(ref)), name
            assert np.abs(out[fin].astype(np.float64) - ref[fin]).max(initial=0.0) <= R.QVAL_BOUND * abs(qv), name
        else:
            assert np.array_equal(bits(out), bits(ref)), name


def test_order_statistics_are_the_sorted_values(gold):
    x = gold["gauss_17x257_q50_rows/x"]
    r = R.row_quantile(x, 0.5)
    assert R.positions(0.5, 257) == (128, 129, 0.0)
    assert np.array_equal(bits(r["quant"]), bits(r["lo_val"]))               # pos integral: the order statistic itself
    assert np.array_equal(r["lo_val"], np.sort(np.abs(x), axis=1)[:, 128])
    assert R.positions(0.999, 1) == (0, 0, 0.0) and R.positions(0.0, 9) == (0, 1, 0.0)


def test_knn_accuracy_statement(gold):
    assert abs(R.knn_accuracy(gold["knn3"]) - float(gold["acc3"])) < 1e-7
    assert R.knn_accuracy(gold["knn3"]) == R.knn_accuracy(gold["knn3"].reshape(30, 16))
    # a 2-D list: the reference's broadcast compares row i with the whole table, not with row i
    assert abs(R.knn_accuracy_reference(gold["knn2"]) - float(gold["acc2"])) < 1e-7
    assert abs(R.knn_accuracy(gold["knn2"]) - float(gold["acc2"])) > 0.5


def test_wrong_variants_miss_by_8x(gold):
    miss = {k: 0.0 for k in ("signed", "pos_qd", "nearest", "per_row", "exact_index", "normalize_first")}
    for name, x, q, ex in cases(gold):
        qv, out = gold[f"{name}/q_val"], gold[f"{name}/out"]
        if not (np.isfinite(x).all() and float(qv) > 0):
            continue
        rel = lambda v: abs(float(v) - float(qv)) / float(qv)
        if ex:
            miss["exact_index"] = max(miss["exact_index"], float((bits(R.wrong_exact_index(x, q)) != bits(qv)).any()))
        else:
            miss["signed"] = max(miss["signed"], rel(R.wrong_signed_quantile(x, q)) / R.QVAL_BOUND)
            miss["pos_qd"] = max(miss["pos_qd"], rel(R.wrong_pos_qd(x, q)) / R.QVAL_BOUND)
            miss["nearest"] = max(miss["nearest"], rel(R.wrong_nearest_rank(x, q)) / R.QVAL_BOUND)
            miss["per_row"] = max(miss["per_row"], np.abs(R.wrong_per_row_bound(x, q) - out).max() / float(qv) / R.QVAL_BOUND)
        ref = R.normalize64(out)
        miss["normalize_first"] = max(miss["normalize_first"], R.max_rel(R.wrong_normalize_first(x, q, ex), ref) / R.NORM_BOUND)
    assert miss.pop("exact_index") == 1.0               # the exact bound is bit-equal: any other bit pattern is a miss
    for k, v in miss.items():
        assert v >= 8.0, (k, v)


# ---- the Python wrappers' argument errors (raised before any GPU use) ----
def test_wrapper_argument_errors():
    import metrics
    import umlh
    A = umlh.align
    x = torch.randn(4, 6)
    for fn in (lambda: A.row_abs_quantile(x, 1.0), lambda: A.row_abs_quantile(x, -0.1), lambda: A.row_abs_quantile(x, float("nan")),
               lambda: A.row_abs_quantile(x[0], 0.5), lambda: A.row_abs_quantile(x.long(), 0.5),
               lambda: A.row_abs_quantile(torch.empty(0, 3), 0.5), lambda: A.abs_kth(x, 24), lambda: A.abs_kth(x, -1),
               lambda: A.remove_outliers(x, 1.5), lambda: A.remove_outliers(x, -0.01, exact=True),
               lambda: A.prepare_features(x, 2.0), lambda: A.prepare_features("x"),
               lambda: A.knn_accuracy(torch.zeros(3, 2)), lambda: A.knn_accuracy(torch.zeros(3, dtype=torch.int64)),
               lambda: A.knn_accuracy(torch.zeros(0, 2, dtype=torch.int64)), lambda: metrics.remove_outliers(x, 1.0001)):
        with pytest.raises(ValueError):
            fn()
    assert A.remove_outliers(x, 1) is x and A.remove_outliers(x, 1.0, exact=True) is x
    assert metrics.remove_outliers(x, 1) is x and metrics.remove_outliers(x, 1.0, max_threshold=3.0) is x
    assert (A.ROW_QUANTILE_WAVE_COLS, A.ROW_QUANTILE_LDS_COLS) == (1024, 15360)


def test_python_thresholds_are_the_headers():
    import umlh
    hdr = open(os.path.join(ROOT, "include", "umlh.h")).read()
    for name in ("ROW_QUANTILE_WAVE_COLS", "ROW_QUANTILE_LDS_COLS"):
        (v,) = re.findall(rf"#define UMLH_{name}\s+(\d+)", hdr)
        assert int(v) == getattr(umlh.align, name)
    for i, name in enumerate(("ROW_QUANTILE", "ABS_KTH", "KNN_ACCURACY")):
        (v,) = re.findall(rf"#define UMLH_OUTLIER_{name}\s+(\d+)", hdr)
        assert int(v) == i == getattr(umlh.align, f"KIND_{name}")


def test_prototype_table_has_the_new_names():
    from test_abi_cpu import header_prototypes, prototype_mismatches
    from umlh import _lib
    hdr = header_prototypes()
    for name in NEW_NAMES:
        assert name in hdr and name in _lib.PROTOTYPES, name
    assert hdr["umlh_row_abs_quantile"] == ("i32", ["pointer", "i64", "i64", "i64", "double"] + ["pointer"] * 6 + ["u64", "pointer"])
    assert prototype_mismatches({n: _lib.PROTOTYPES[n] for n in NEW_NAMES}) == sorted(
        f"{n}: declared in umlh.h, missing from the table" for n in hdr.keys() - set(NEW_NAMES))
    assert "umlh_kernels_outlier.hip" in _lib.SOURCES


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_library_exports_and_checks_before_any_hip_call(lib):
    """No GPU here: an entry point that reached a HIP call would return a HIP error, not UMLH_E_INVALID with its own message."""
    E_INVALID = -1
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
    q = lib.umlh_outlier_scratch_bytes
    assert q(0, 50000, 512) >= 8 * 13 and q(1, 7, 3) >= 4 * 256 * 8 and q(2, 10, 100) >= 8
    for bad in ((3, 4, 4), (-1, 4, 4), (0, 0, 4), (0, 4, 0), (1, 4, 1 << 31), (1, 1 << 20, 1 << 20), (2, 1 << 31, 2)):
        assert q(*bad) == 0, bad
    f = C.c_void_p(256)          # never dereferenced: the checks come first
    d = C.c_double
    calls = {
        "umlh_row_abs_quantile": [
            (None, 4, 4, 4, d(.5), None, None, f, None, f, f, 4096, None), (f, 0, 4, 4, d(.5), None, None, f, None, f, f, 4096, None),
            (f, 4, 0, 4, d(.5), None, None, f, None, f, f, 4096, None), (f, 4, 1 << 31, 1 << 31, d(.5), None, None, f, None, f, f, 4096, None),
            (f, 1 << 20, 1 << 20, 1 << 20, d(.5), None, None, f, None, f, f, 1 << 30, None),
            (f, 4, 4, 3, d(.5), None, None, f, None, f, f, 4096, None), (f, 4, 4, 4, d(1.0), None, None, f, None, f, f, 4096, None),
            (f, 4, 4, 4, d(-.1), None, None, f, None, f, f, 4096, None), (f, 4, 4, 4, d(float("nan")), None, None, f, None, f, f, 4096, None),
            (f, 4, 4, 4, d(.5), None, None, None, None, f, f, 4096, None), (f, 4, 4, 4, d(.5), None, None, f, None, None, f, 4096, None),
            (f, 4, 4, 4, d(.5), None, None, f, None, f, None, 4096, None), (f, 4, 4, 4, d(.5), None, None, f, None, f, f, 0, None),
            (f, 4, 4, 4, d(.5), None, None, f, None, f, C.c_void_p(260), 4096, None)],
        "umlh_abs_kth": [
            (None, 4, 4, 4, 0, f, f, 1 << 20, None), (f, 0, 4, 4, 0, f, f, 1 << 20, None), (f, 4, 4, 3, 0, f, f, 1 << 20, None),
            (f, 4, 4, 4, 16, f, f, 1 << 20, None), (f, 4, 4, 4, -1, f, f, 1 << 20, None), (f, 4, 4, 4, 0, None, f, 1 << 20, None),
            (f, 4, 4, 4, 0, f, None, 1 << 20, None), (f, 4, 4, 4, 0, f, f, 16, None), (f, 4, 4, 4, 0, f, C.c_void_p(260), 1 << 20, None)],
        "umlh_clamp_rows": [
            (None, 4, 4, 4, f, 0, f, 4, None), (f, 0, 4, 4, f, 0, f, 4, None), (f, 4, 0, 4, f, 0, f, 4, None), (f, 4, 4, 3, f, 0, f, 4, None),
            (f, 4, 4, 4, None, 0, f, 4, None), (f, 4, 4, 4, f, 0, None, 4, None), (f, 4, 4, 4, f, 1, f, 3, None),
            (f, 4, 4, 4, f, 0, f, 8, None)],          # in place with another stride
        "umlh_knn_accuracy": [
            (None, 4, 2, 2, f, f, 4096, None), (f, 0, 2, 2, f, f, 4096, None), (f, 4, 0, 0, f, f, 4096, None), (f, 4, 2, 1, f, f, 4096, None),
            (f, 1 << 31, 2, 2, f, f, 1 << 40, None), (f, 4, 2, 2, None, f, 4096, None), (f, 4, 2, 2, f, None, 4096, None),
            (f, 4, 2, 2, f, f, 0, None)],
    }
    for name, arglists in calls.items():
        for args in arglists:
            assert getattr(lib, name)(*args) == E_INVALID, (name, args)
            assert name.encode() in lib.umlh_last_error(), (name, args, lib.umlh_last_error())
