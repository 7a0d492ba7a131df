"""Alignment metrics without a GPU: the float64 restatement (tests/_align_ref.py) against the reference's recorded values,
the C ABI's argument checks (made before any HIP call) and the scratch bound."""
import ctypes as C

import numpy as np
import pytest

import _align_ref as R
from conftest import load_golden

CASES = ("gauss", "offset", "wide", "ragged", "tiny", "toy")


@pytest.fixture(scope="module")
def gold():
    return load_golden("alignment")


def test_golden_lists_every_case(gold):
    assert tuple(gold["cases"]) == CASES


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference_cka(gold, case):
    a, b = gold[f"{case}/a"], gold[f"{case}/b"]
    c64 = R.cka64(a, b)
    np.testing.assert_allclose(c64, gold[f"{case}/cka64"], rtol=1e-12, atol=0)
    if case == "offset":
        # recorded, not matched: the reference's fp32 trace(K H L H) cancels catastrophically on mean-50 columns
        assert abs(gold[f"{case}/ref_cka"] - c64[0]) > 1e-4
        assert abs(gold[f"{case}/ref_cka_multibench"] - c64[0]) < 1e-5
    else:
        assert abs(gold[f"{case}/ref_cka"] - c64[0]) <= 1e-6, (case, gold[f"{case}/ref_cka"], c64[0])
    # no 1/(N-1)^2 normalisation: the recorded HSIC terms are the plain traces (relative agreement, fp32 reference)
    if case != "offset":
        np.testing.assert_allclose(gold[f"{case}/ref_hsic"], c64[1:], rtol=2e-4)


def test_epsilon_term_moves_the_tiny_case(gold):
    a, b = gold["tiny/a"], gold["tiny/b"]
    c, kl, kk, ll = R.cka64(a, b)
    without = kl / np.sqrt(kk * ll)
    assert abs(without - c) > 1e-3          # the absolute 1e-6 is visible at std 1e-3
    assert abs(gold["tiny/ref_cka"] - c) <= 1e-6


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference_neighbours(gold, case):
    for v in ("a", "b"):
        x = gold[f"{case}/{v}"]
        idx, s = R.knn64(x, 10)
        t = R.tau(x)
        ok = R.list_decidable(s, t, 10)
        np.testing.assert_array_equal(idx[ok], gold[f"{case}/ref_knn_{v}"][ok])
        assert (idx[:, :10] != np.arange(x.shape[0])[:, None]).all()          # self excluded
        if case not in ("offset", "toy"):      # generated cases (the toy's 64 embeddings are fixed by the training replay)
            assert ok.mean() >= 0.99, (case, v, ok.mean())


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference_mutual_knn(gold, case):
    a, b = gold[f"{case}/a"], gold[f"{case}/b"]
    und = int(gold[f"{case}/undecidable"])
    for k in (1, 10, 32):
        ka, _ = R.knn64(a, k)
        kb, _ = R.knn64(b, k)
        m = R.mutual64(ka, kb)
        assert m == gold[f"{case}/mknn64_k{k}"]
        assert abs(m - gold[f"{case}/ref_mknn_k{k}"]) <= 1e-6 + und / a.shape[0], (case, k)


def test_restatement_tie_rule_is_score_desc_index_asc():
    x = np.array([[1, 0], [1, 0], [1, 0], [0, 1], [1, 0]], np.float32)
    idx, s = R.knn64(x, 3)
    assert idx[0].tolist() == [1, 2, 4]
    assert idx[3].tolist() == [0, 1, 2]            # all scores 0: smallest indices first
    assert s[3, :3].tolist() == [0.0, 0.0, 0.0]


def test_restatement_blocks_match_one_block():
    g = np.random.default_rng(3)
    x = g.integers(-2, 3, (300, 5)).astype(np.float32)
    i1, s1 = R.knn64(x, 7, block=64)
    i2, s2 = R.knn64(x, 7, block=4096)
    np.testing.assert_array_equal(i1, i2)
    np.testing.assert_array_equal(s1, s2)
    full = x.astype(np.float64) @ x.T.astype(np.float64)
    np.fill_diagonal(full, -np.inf)
    for r in (0, 17, 299):
        order = np.lexsort((np.arange(300), -full[r]))[:7]
        assert i1[r].tolist() == order.tolist()


# ---- the C ABI: argument checks before any HIP call ----

@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_abi_revision(lib):
    assert lib.umlh_version() >= 5


def test_knn_validates_arguments(lib):
    f = C.c_void_p(64)                       # never dereferenced: every check comes first
    knn = lambda x, n, d, ld, k, splits=0, out=f, scratch=f, nbytes=1 << 40: lib.umlh_align_knn(x, n, d, ld, k, splits, out, None, scratch, nbytes, None)
    for args, what in (((None, 100, 8, 8, 10), b"null"), ((f, 100, 8, 8, 10, 0, None), b"null"), ((f, 100, 8, 8, 10, 0, f, None), b"null"),
                       ((f, 100, 8, 8, 0), b"topk=0"), ((f, 100, 8, 8, 33), b"topk=33"), ((f, 10, 8, 8, 10), b"n=10"),
                       ((f, 100, 8, 7, 10), b"ldx=7"), ((f, 100, 0, 8, 10), b"d=0"), ((f, 100, 8, 8, 10, -1), b"splits=-1")):
        assert knn(*args) == -1, args
        msg = lib.umlh_last_error()
        assert b"umlh_align_knn" in msg and what in msg, (args, msg)
    assert knn(f, 100, 8, 8, 10, nbytes=16) == -1 and b"scratch" in lib.umlh_last_error()


def test_mutual_and_cka_validate_arguments(lib):
    f = C.c_void_p(64)
    mk = lib.umlh_align_mutual_knn
    for args, what in (((None, f, 100, 10, f, f, 1 << 40), b"null"), ((f, f, 100, 10, None, f, 1 << 40), b"null"),
                       ((f, f, 100, 0, f, f, 1 << 40), b"topk=0"), ((f, f, 100, 33, f, f, 1 << 40), b"topk=33"),
                       ((f, f, 10, 10, f, f, 1 << 40), b"n=10"), ((f, f, 100, 10, f, f, 0), b"scratch")):
        assert mk(*args, None) == -1, args
        msg = lib.umlh_last_error()
        assert b"umlh_align_mutual_knn" in msg and what in msg, (args, msg)
    ck = lambda a, lda, da, b, ldb, db, n, nbytes=1 << 40, out=f: lib.umlh_align_cka(a, lda, da, b, ldb, db, n, 0, out, f, nbytes, None)
    for args, what in (((None, 8, 8, f, 8, 8, 100), b"null"), ((f, 8, 8, None, 8, 8, 100), b"null"),
                       ((f, 8, 8, f, 8, 8, 100, 1 << 40, None), b"null"), ((f, 7, 8, f, 8, 8, 100), b"lda=7"),
                       ((f, 8, 8, f, 5, 6, 100), b"ldb=5"), ((f, 8, 0, f, 8, 8, 100), b"d_a=0"), ((f, 8, 8, f, 8, 8, 0), b"n=0"),
                       ((f, 8, 8, f, 8, 8, 100, 8), b"scratch")):
        assert ck(*args) == -1, args
        msg = lib.umlh_last_error()
        assert b"umlh_align_cka" in msg and what in msg, (args, msg)


def test_python_surface_validates_before_the_gpu():
    import torch
    from umlh import align
    a, b = torch.zeros(100, 8), torch.zeros(99, 8)
    with pytest.raises(ValueError, match="same N"):
        align.cka(a, b)
    with pytest.raises(ValueError, match="same N"):
        align.mutual_knn(a, b, 10)
    with pytest.raises(ValueError, match="topk=33"):
        align.knn(a, 33)
    with pytest.raises(ValueError, match="topk=0"):
        align.knn(a, 0)
    with pytest.raises(ValueError, match="topk=100"):
        align.knn(a, 100)


def test_metrics_module_names_and_errors():
    import metrics
    assert metrics.AlignmentMetrics.SUPPORTED_METRICS == ["cycle_knn", "mutual_knn", "lcs_knn", "cka", "unbiased_cka", "cknna",
                                                          "svcca", "edit_distance_knn"]
    with pytest.raises(ValueError, match="Unrecognized metric"):
        metrics.AlignmentMetrics.measure("knn_nope", None, None)
    for name in ("unbiased_cka", "cknna", "svcca", "cycle_knn", "lcs_knn", "edit_distance_knn"):
        with pytest.raises(NotImplementedError, match="supported"):
            metrics.AlignmentMetrics.measure(name, None, None, topk=10)
    with pytest.raises(NotImplementedError, match="rbf"):
        metrics.AlignmentMetrics.measure("cka", None, None, kernel_metric="rbf")
    with pytest.raises(NotImplementedError, match="unbiased"):
        metrics.AlignmentMetrics.measure("cka", None, None, unbiased=True)
    import finetune
    assert finetune.cka is metrics.cka and finetune.mknn is metrics.mknn


def test_scratch_has_no_quadratic_term(lib):
    sb = lib.umlh_align_scratch_bytes
    n = 10 ** 6
    b1 = sb(n, 256, 256, 10, 0)
    assert 0 < b1 < 1 << 30, b1
    assert sb(2 * n, 256, 256, 10, 0) <= 2 * b1 + (1 << 20)
    for n_ in (2000, 50000, 123457):
        assert sb(2 * n_, 35, 300, 10, 0) <= 2 * sb(n_, 35, 300, 10, 0) + (1 << 20)
    # invalid arguments: 0
    assert sb(100, 8, 8, 33, 0) == 0 and sb(10, 8, 8, 10, 0) == 0 and sb(100, 0, 8, 10, 0) == 0 and sb(100, 8, 8, 10, -1) == 0
    assert sb(100, 8, 8, 0, 0) > 0           # topk 0: CKA / mutual only
