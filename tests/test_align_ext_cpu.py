"""The remaining alignment metrics without a GPU: the float64 restatement (tests/_align_ext_ref.py) against the reference's
recorded float64 values, the C ABI's argument checks (made before any HIP call), the scratch bound and the Python-level
errors."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _align_ext_ref as X
import _align_ref as R
from conftest import ROOT, load_golden

CASES = ("gauss", "offset", "wide", "ragged", "tiny", "toy")
NEW_SYMBOLS = ("umlh_align_ext_scratch_bytes", "umlh_align_cka_unbiased", "umlh_align_cka_rbf", "umlh_align_cknna",
               "umlh_align_list_stats")
K_UNBIASED, K_RBF, K_CKNNA, K_LIST = range(4)


@pytest.fixture(scope="module")
def gold():
    return load_golden("alignment")


@pytest.fixture(scope="module")
def ext():
    return load_golden("alignment_ext")


def test_golden_lists_every_case_and_no_inputs(ext):
    assert tuple(ext["cases"]) == CASES
    assert all(v.size <= 3 or k == "cases" for k, v in ext.items())          # recorded values only, no input arrays
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "alignment_ext.npz")) < 1 << 20


# The restatement works on centred features; the reference's float64 run on the raw ones carries its own cancellation
# (|mean| / spread ~ 50 on `offset`: about 2e-8 relative on the HSIC terms), so 1e-9 holds everywhere but there.
def _tol(case):
    return 1e-7 if case == "offset" else 1e-9


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference_unbiased_cka(gold, ext, case):
    c = X.unbiased_cka64(gold[f"{case}/a"], gold[f"{case}/b"])
    assert abs(c[0] - ext[f"{case}/ucka_ref64"]) <= _tol(case), (case, c[0], ext[f"{case}/ucka_ref64"])
    np.testing.assert_allclose(c[1:], ext[f"{case}/uhsic_ref64"], rtol=_tol(case) * 10)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference_rbf_cka(gold, ext, case):
    a, b = gold[f"{case}/a"], gold[f"{case}/b"]
    sigma = float(ext[f"{case}/rbf_raw_sigma"])
    assert abs(sigma - X.median_sigma(a, b)) <= 1e-12 * sigma
    for tag, xa, xb, s in (("norm", X.normalize_rows(a), X.normalize_rows(b), 1.0), ("raw", a, b, sigma)):
        for u, unbiased in (("b", False), ("u", True)):
            want = float(ext[f"{case}/rbf_{tag}_{u}_ref64"])
            dense = X.rbf_cka64(xa, xb, s, unbiased)
            assert abs(dense[0] - want) <= _tol(case), (case, tag, u, dense[0], want)
            blocked = X.rbf_cka64_blocked(xa, xb, s, unbiased, block=100)
            # each HSIC is a difference of float64 sums of N^2 kernel values <= 1: rounding of order 1e-16 N^2 per sum,
            # which the two summation orders do not share (on `offset` the normalised rows nearly coincide, K ~ 1)
            n = a.shape[0]
            atol = 1e-13 * n * n / (n * (n - 3) if unbiased else 1)
            np.testing.assert_allclose(blocked[1:], dense[1:], rtol=1e-10, atol=atol)
            assert abs(blocked[0] - dense[0]) <= 1e-7


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference_cknna_and_lists(gold, ext, case):
    a, b = gold[f"{case}/a"], gold[f"{case}/b"]
    if int(gold[f"{case}/undecidable"]) == 0:          # neighbour sets decided beyond fp32 noise for k in {1, 10, 32}
        for k in (10, 32):
            got = X.cknna64(a, b, k)[0]
            assert abs(got - float(ext[f"{case}/cknna_k{k}_ref64"])) <= 1e-9, (case, k, got)
    ka, sa = R.knn64(a, 10)
    kb, sb = R.knn64(b, 10)
    if R.list_decidable(sa, R.tau(a), 10).all() and R.list_decidable(sb, R.tau(b), 10).all():
        m = X.list_means(X.list_rows(ka, kb), 10)
        assert abs(m[0] - float(ext[f"{case}/cycle_k10_ref64"])) <= 1e-6       # the reference's means are fp32
        assert abs(m[1] - float(ext[f"{case}/lcs_k10_ref64"])) <= 1e-6
    else:
        assert case in ("offset", "toy")


def test_blocked_unbiased_linear_matches_dense(gold):
    a, b = gold["ragged/a"], gold["ragged/b"]
    np.testing.assert_allclose(X.unbiased_cka64_blocked(a, b, block=50), X.unbiased_cka64(a, b), rtol=1e-10)


def test_cknna_is_checked_on_at_least_five_cases(gold):
    assert sum(int(gold[f"{c}/undecidable"]) == 0 for c in CASES) >= 5


def test_the_reference_fp32_breaks_on_offset(ext):
    assert math.isnan(float(ext["offset/ucka_ref32"]))
    assert abs(float(ext["offset/rbf_norm_u_ref32"]) - float(ext["offset/rbf_norm_u_ref64"])) > 0.1


def test_masked_hsic_needs_the_transpose():
    g = np.random.default_rng(0)
    M, P = g.standard_normal((6, 6)), g.standard_normal((6, 6))
    Mt, Pt = M.copy(), P.copy()
    np.fill_diagonal(Mt, 0)
    np.fill_diagonal(Pt, 0)
    m = 6
    want = ((Mt * Pt.T).sum() + Mt.sum() * Pt.sum() / ((m - 1) * (m - 2)) - 2 * (Mt @ Pt).sum() / (m - 2)) / (m * (m - 3))
    assert abs(X.hsic_unbiased64(M, P) - want) <= 1e-12
    assert abs(X.hsic_unbiased64(M, P) - X.hsic_unbiased64(M, P.T)) > 1e-3


def test_list_dps_on_known_lists():
    assert X.lcs_length([1, 2, 3, 4], [1, 2, 3, 4]) == 4 and X.levenshtein([1, 2, 3, 4], [1, 2, 3, 4]) == 0
    assert X.lcs_length([1, 2, 3, 4], [4, 3, 2, 1]) == 1 and X.levenshtein([1, 2, 3, 4], [4, 3, 2, 1]) == 4
    assert X.lcs_length([1, 2, 3], [7, 8, 9]) == 0 and X.levenshtein([1, 2, 3], [7, 8, 9]) == 3
    assert X.lcs_length([1, 2, 3, 4], [2, 3, 4, 1]) == 3 and X.levenshtein([1, 2, 3, 4], [2, 3, 4, 1]) == 2
    assert X.levenshtein(list("kitten"), list("sitting")) == 3
    rows = X.list_rows(np.array([[1, 2], [2, 0], [0, 1]]), np.array([[2, 1], [0, 2], [1, 0]]))
    assert rows.tolist() == [[1, 1, 2], [1, 1, 2], [1, 1, 2]]
    assert X.list_means(rows, 2) == (1.0, 1.0, 0.0)


# ---- the C ABI: argument checks before any HIP call ----

@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_abi_revision_and_exports(lib):
    assert lib.umlh_version() >= 7
    hdr = open(os.path.join(ROOT, "include", "umlh.h")).read()
    declared = set(re.findall(r"\b(umlh_[a-z_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name


def _expect(lib, rc, who, what):
    msg = lib.umlh_last_error()
    assert rc == -1 and who in msg and what in msg, (rc, msg, what)


def test_cka_entry_points_validate_arguments(lib):
    f, big = C.c_void_p(64), 1 << 40                       # never dereferenced: every check comes first
    ub = lambda a, lda, da, b, ldb, db, n, splits=0, out=f, scratch=f, nbytes=big: lib.umlh_align_cka_unbiased(
        a, lda, da, b, ldb, db, n, splits, out, scratch, nbytes, None)
    rbf = lambda a, lda, da, b, ldb, db, n, sigma=1.0, unb=0, splits=0, out=f, scratch=f, nbytes=big: lib.umlh_align_cka_rbf(
        a, lda, da, b, ldb, db, n, sigma, unb, splits, out, scratch, nbytes, None)
    for fn, who in ((ub, b"umlh_align_cka_unbiased"), (rbf, b"umlh_align_cka_rbf")):
        _expect(lib, fn(None, 8, 8, f, 8, 8, 100), who, b"null")
        _expect(lib, fn(f, 8, 8, None, 8, 8, 100), who, b"null")
        _expect(lib, fn(f, 8, 8, f, 8, 8, 100, out=None), who, b"null")
        _expect(lib, fn(f, 8, 8, f, 8, 8, 100, scratch=None), who, b"null")
        _expect(lib, fn(f, 7, 8, f, 8, 8, 100), who, b"lda=7")
        _expect(lib, fn(f, 8, 8, f, 5, 6, 100), who, b"ldb=5")
        _expect(lib, fn(f, 8, 0, f, 8, 8, 100), who, b"d_a=0")
        _expect(lib, fn(f, 8, 8, f, 8, 8, 0), who, b"n=0")
        _expect(lib, fn(f, 8, 8, f, 8, 8, 100, splits=-1), who, b"splits=-1")
        _expect(lib, fn(f, 8, 8, f, 8, 8, 100, nbytes=8), who, b"scratch")
    _expect(lib, ub(f, 8, 8, f, 8, 8, 3), b"umlh_align_cka_unbiased", b"n=3")
    _expect(lib, rbf(f, 8, 8, f, 8, 8, 3, unb=1), b"umlh_align_cka_rbf", b"n=3")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _expect(lib, rbf(f, 8, 8, f, 8, 8, 100, sigma=bad), b"umlh_align_cka_rbf", b"sigma")


def test_list_entry_points_validate_arguments(lib):
    f, big = C.c_void_p(64), 1 << 40
    ck = lambda ka=f, sa=f, kb=f, sb=f, n=100, k=10, out=f, scratch=f, nbytes=big: lib.umlh_align_cknna(
        ka, sa, kb, sb, n, k, out, scratch, nbytes, None)
    who = b"umlh_align_cknna"
    for kw in ({"ka": None}, {"sa": None}, {"kb": None}, {"sb": None}, {"out": None}, {"scratch": None}):
        _expect(lib, ck(**kw), who, b"null")
    _expect(lib, ck(k=1), who, b"CKNNA requires topk >= 2")
    _expect(lib, ck(k=0), who, b"CKNNA requires topk >= 2")
    _expect(lib, ck(k=33), who, b"topk=33")
    _expect(lib, ck(n=10, k=10), who, b"n=10")
    _expect(lib, ck(n=3, k=2), who, b"n=3")
    _expect(lib, ck(nbytes=16), who, b"scratch")
    ls = lambda ka=f, kb=f, n=100, k=10, rows=None, out=f, scratch=f, nbytes=big: lib.umlh_align_list_stats(
        ka, kb, n, k, rows, out, scratch, nbytes, None)
    who = b"umlh_align_list_stats"
    for kw in ({"ka": None}, {"kb": None}, {"out": None}, {"scratch": None}):
        _expect(lib, ls(**kw), who, b"null")
    _expect(lib, ls(k=0), who, b"topk=0")
    _expect(lib, ls(k=33), who, b"topk=33")
    _expect(lib, ls(n=10, k=10), who, b"n=10")
    _expect(lib, ls(nbytes=0), who, b"scratch")


def test_ext_scratch_query(lib):
    sb = lib.umlh_align_ext_scratch_bytes
    n = 10 ** 6
    for kind, d_a, d_b, k in ((K_UNBIASED, 256, 256, 0), (K_RBF, 256, 256, 0), (K_RBF, 35, 300, 0), (K_CKNNA, 1, 1, 10),
                              (K_LIST, 1, 1, 10)):
        b1 = sb(kind, n, d_a, d_b, k, 0)
        assert 0 < b1 < 1 << 30, (kind, b1)
        assert sb(kind, 2 * n, d_a, d_b, k, 0) <= 2 * b1 + (1 << 20), kind          # no term grows with N^2
        for n_ in (2000, 50000, 123457):
            assert sb(kind, 2 * n_, d_a, d_b, k, 0) <= 2 * sb(kind, n_, d_a, d_b, k, 0) + (1 << 20), (kind, n_)
    # invalid arguments: 0
    assert sb(4, 100, 8, 8, 10, 0) == 0 and sb(-1, 100, 8, 8, 10, 0) == 0
    assert sb(K_UNBIASED, 3, 8, 8, 0, 0) == 0 and sb(K_UNBIASED, 100, 0, 8, 0, 0) == 0 and sb(K_UNBIASED, 100, 8, 8, 0, -1) == 0
    assert sb(K_RBF, 0, 8, 8, 0, 0) == 0 and sb(K_RBF, 100, 8, 0, 0, 0) == 0 and sb(K_RBF, 100, 8, 8, 0, -1) == 0
    assert sb(K_CKNNA, 100, 1, 1, 1, 0) == 0 and sb(K_CKNNA, 100, 1, 1, 33, 0) == 0 and sb(K_CKNNA, 10, 1, 1, 10, 0) == 0
    assert sb(K_LIST, 100, 1, 1, 0, 0) == 0 and sb(K_LIST, 100, 1, 1, 33, 0) == 0 and sb(K_LIST, 10, 1, 1, 10, 0) == 0
    # the existing query keeps its values (tests/test_align_cpu.py pins their growth)
    assert lib.umlh_align_scratch_bytes(100, 8, 8, 0, 0) > 0


def test_python_surface_validates_before_the_gpu(monkeypatch):
    import torch
    from umlh import align

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(align, "load_library", no_library)
    monkeypatch.setattr(align, "_device", no_library)
    a, b, c = torch.zeros(100, 8), torch.zeros(99, 8), torch.zeros(100, 5)
    for fn in (align.unbiased_cka, align.rbf_cka, lambda p, q: align.cknna(p, q, 10), lambda p, q: align.cycle_knn(p, q, 10),
               lambda p, q: align.lcs_knn(p, q, 10), lambda p, q: align.edit_distance_knn(p, q, 10)):
        with pytest.raises(ValueError, match="same N"):
            fn(a, b)
    with pytest.raises(ValueError, match="N=3"):
        align.unbiased_cka(a[:3], c[:3])
    with pytest.raises(ValueError, match="N=3"):
        align.rbf_cka(a[:3], c[:3], unbiased=True)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            align.rbf_cka(a, c, sigma=bad)
    with pytest.raises(ValueError, match="splits=-1"):
        align.rbf_cka(a, c, splits=-1)
    with pytest.raises(ValueError, match="topk >= 2"):
        align.cknna(a, c, 1)
    with pytest.raises(ValueError, match="topk=33"):
        align.cknna(a, c, 33)
    with pytest.raises(ValueError, match="topk=100"):
        align.lcs_knn(a, c, 100)
    with pytest.raises(ValueError, match="topk=0"):
        align.cycle_knn(a, c, 0)
    with pytest.raises(ValueError, match="neighbour lists"):
        align.list_stats(torch.zeros(10, 3, dtype=torch.int32), torch.zeros(10, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="topk=33"):
        align.list_stats(torch.zeros(100, 33, dtype=torch.int32), torch.zeros(100, 33, dtype=torch.int32))
    with pytest.raises(ValueError, match="Unrecognized metric: nope"):
        align.measure("nope", a, c)
    with pytest.raises(ValueError, match="Invalid kernel metric"):
        align.measure("cka", a, c, kernel_metric="poly")
    with pytest.raises(NotImplementedError, match="svcca"):
        align.measure("svcca", a, c)
    with pytest.raises(NotImplementedError, match="distance_agnostic"):
        align.measure("cknna", a, c, topk=10, distance_agnostic=True)
    with pytest.raises(NotImplementedError, match="unbiased=False"):
        align.measure("cknna", a, c, topk=10, unbiased=False)
    with pytest.raises(ValueError, match="topk >= 2"):
        align.measure("cknna", a, c, topk=1)


def test_metrics_module_points_at_measure():
    import metrics
    with pytest.raises(NotImplementedError, match="umlh.align.measure"):
        metrics.AlignmentMetrics.measure("cknna", None, None, topk=10)
