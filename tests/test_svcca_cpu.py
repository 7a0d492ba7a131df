"""Principal subspaces / SVCCA without a GPU: the ABI revision and exports, the scratch query, the argument checks of the two
entry points (made before any HIP call), the Python-level errors, the float64 restatement against the golden, and the
condition on the golden's inputs: the reference's own values (five seeds, fp32 and fp64) lie within each case's bound of the
closed form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _svcca_ref as R
from conftest import ROOT, load_golden

NEW_SYMBOLS = ("umlh_subspace_scratch_bytes", "umlh_principal_subspace", "umlh_svcca")
CASES = ("mosei", "mid", "offset", "wide", "q1", "full", "same")
SHAPES = {"mosei": (257, 35, 300, 10), "mid": (400, 32, 48, 10), "offset": (500, 64, 64, 8), "wide": (40, 64, 48, 5),
          "q1": (300, 20, 24, 1), "full": (300, 6, 6, 6), "same": (300, 40, 40, 10)}


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


@pytest.fixture(scope="module")
def gold():
    return load_golden("svcca")


def test_abi_revision_and_exports(lib):
    from umlh import _lib
    assert lib.umlh_version() >= 9
    hdr = open(os.path.join(ROOT, "include", "umlh.h")).read()
    declared = set(re.findall(r"\b(umlh_[a-z_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name


def test_scratch_query(lib):
    sb = lib.umlh_subspace_scratch_bytes
    # invalid: n, d_a, d_b, q out of range; q above min(n, d_a, d_b, 64)
    for bad in ((1, 8, 8, 1), (0, 8, 8, 1), (-5, 8, 8, 1), (2 ** 31, 8, 8, 1), (100, 0, 8, 1), (100, 513, 8, 1), (100, 8, 513, 1),
                (100, 8, -1, 1), (100, 8, 8, 0), (100, 8, 8, 9), (100, 8, 4, 5), (5, 8, 8, 6), (100, 8, 0, 9), (100, 100, 100, 65),
                (100, 100, 0, 65), (100, 8, 8, -1)):
        assert sb(*bad) == 0, bad
    assert sb(2, 1, 1, 1) > 0 and sb(2 ** 31 - 1, 512, 512, 64) > 0 and sb(100, 8, 0, 8) > 0
    prev_pair = prev_single = 0
    for d in (1, 7, 64, 65, 300, 512):                      # monotone in d
        q = min(d, 10)
        pair, single = sb(5000, d, d, q), sb(5000, d, 0, q)
        assert pair > prev_pair and single > prev_single and single < pair, d
        prev_pair, prev_single = pair, single
    assert sb(5000, 35, 300, 10) > sb(5000, 35, 35, 10) and sb(5000, 300, 35, 10) > sb(5000, 35, 35, 10)
    # no n x d growth: past the chunk cap (128 chunks of 256 rows) the size does not move with n at all
    assert sb(10 ** 6, 300, 300, 10) == sb(10 ** 8, 300, 300, 10) == sb(128 * 256, 300, 300, 10)
    assert sb(10 ** 6, 300, 0, 10) == sb(10 ** 8, 300, 0, 10) == sb(128 * 256, 300, 0, 10)
    assert sb(10 ** 6, 300, 300, 10) < 64 * 8 * 300 * 300 * 129


def _expect(lib, rc, who, what):
    msg = lib.umlh_last_error()
    assert rc == -1 and who in msg and what in msg, (rc, msg, what)


def test_principal_subspace_validates_arguments(lib):
    f, big = C.c_void_p(64), 1 << 40                       # never dereferenced: every check comes first
    ps = lambda a=f, n=100, d=8, ld=8, q=3, std=1, evals=f, evecs=f, scratch=f, nbytes=big: lib.umlh_principal_subspace(
        a, n, d, ld, q, std, evals, evecs, scratch, nbytes, None)
    who = b"umlh_principal_subspace"
    for name in ("a", "evals", "evecs", "scratch"):
        _expect(lib, ps(**{name: None}), who, b"null")
    _expect(lib, ps(nbytes=lib.umlh_subspace_scratch_bytes(100, 8, 0, 3) - 1), who, b"scratch")
    _expect(lib, ps(nbytes=0), who, b"scratch")
    _expect(lib, ps(n=1), who, b"n=1")
    _expect(lib, ps(n=0), who, b"n=0")
    _expect(lib, ps(n=2 ** 31), who, b"2^31")
    _expect(lib, ps(d=0), who, b"d_a=0")
    _expect(lib, ps(d=513, ld=513), who, b"d_a=513")
    _expect(lib, ps(ld=7), who, b"ld_a=7")
    _expect(lib, ps(ld=2 ** 31), who, b"ld_a=2147483648")
    _expect(lib, ps(q=0), who, b"q=0")
    _expect(lib, ps(q=9), who, b"q=9")
    _expect(lib, ps(n=5, q=6), who, b"q=6")
    _expect(lib, ps(d=100, ld=100, q=65), who, b"q=65")
    _expect(lib, ps(std=2), who, b"standardize=2")
    assert ps(n=1, a=None) == -1


def test_svcca_validates_arguments(lib):
    f, big = C.c_void_p(64), 1 << 40
    sv = lambda a=f, b=f, n=100, d_a=8, d_b=12, ld_a=8, ld_b=12, q=3, out=f, rho=None, evals=None, scratch=f, nbytes=big: \
        lib.umlh_svcca(a, b, n, d_a, d_b, ld_a, ld_b, q, out, rho, evals, scratch, nbytes, None)
    who = b"umlh_svcca"
    for name in ("a", "b", "out", "scratch"):
        _expect(lib, sv(**{name: None}), who, b"null")
    _expect(lib, sv(nbytes=lib.umlh_subspace_scratch_bytes(100, 8, 12, 3) - 1), who, b"scratch")
    _expect(lib, sv(n=1), who, b"n=1")
    _expect(lib, sv(n=2 ** 31), who, b"2^31")
    _expect(lib, sv(d_a=0), who, b"d_a=0")
    _expect(lib, sv(d_b=0), who, b"d_b=0")
    _expect(lib, sv(d_a=513, ld_a=513), who, b"d_a=513")
    _expect(lib, sv(d_b=513, ld_b=513), who, b"d_b=513")
    _expect(lib, sv(ld_a=7), who, b"ld_a=7")
    _expect(lib, sv(ld_b=11), who, b"ld_b=11")
    _expect(lib, sv(q=0), who, b"q=0")
    _expect(lib, sv(q=9), who, b"q=9")                      # above d_a
    _expect(lib, sv(d_a=20, ld_a=20, q=13), who, b"q=13")   # above d_b
    _expect(lib, sv(n=2, q=3), who, b"q=3")                 # above n
    _expect(lib, sv(d_a=100, ld_a=100, d_b=100, ld_b=100, q=65), who, b"q=65")


def test_python_surface_validates_before_the_gpu(monkeypatch):
    import torch
    import umlh
    from umlh import align, spectral

    def no_library():
        raise AssertionError("the library was reached")
    for mod in (spectral, align):
        monkeypatch.setattr(mod, "load_library", no_library)
        monkeypatch.setattr(mod, "_device", no_library)
    assert umlh.principal_subspace is spectral.principal_subspace
    assert umlh.svcca is align.svcca and umlh.svcca_terms is align.svcca_terms
    ps = spectral.principal_subspace
    with pytest.raises(ValueError, match="2-D"):
        ps(torch.zeros(7), 1)
    with pytest.raises(ValueError, match="floating-point"):
        ps(torch.zeros(7, 3, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="d=513"):
        ps(torch.zeros(7, 513), 1)
    with pytest.raises(ValueError, match="n=1 "):
        ps(torch.zeros(1, 3), 1)
    with pytest.raises(ValueError, match="q=4"):
        ps(torch.zeros(7, 3), 4)
    with pytest.raises(ValueError, match="q=0"):
        ps(torch.zeros(7, 3), 0)
    with pytest.raises(ValueError, match="q=65"):
        ps(torch.zeros(100, 100), 65)
    with pytest.raises(ValueError, match="not an integer"):
        ps(torch.zeros(7, 3), 2.7)
    with pytest.raises(ValueError, match="not an integer"):
        align.svcca(torch.zeros(50, 20), torch.zeros(50, 20), 2.5)
    for fn in (align.svcca, align.svcca_terms):
        with pytest.raises(ValueError, match="same N"):
            fn(torch.zeros(7, 3), torch.zeros(8, 3))
        with pytest.raises(ValueError, match="same N"):
            fn(torch.zeros(7, 3), torch.zeros(7))
        with pytest.raises(ValueError, match="floating-point"):
            fn(torch.zeros(7, 3), torch.zeros(7, 3, dtype=torch.int64), 2)
        with pytest.raises(ValueError, match="d=513"):
            fn(torch.zeros(700, 513), torch.zeros(700, 20))
        with pytest.raises(ValueError, match="n=1 "):
            fn(torch.zeros(1, 3), torch.zeros(1, 3), 1)
        with pytest.raises(ValueError, match="q=10"):
            fn(torch.zeros(50, 20), torch.zeros(50, 9))     # the default cca_dim = 10 above d_b
        with pytest.raises(ValueError, match="q=65"):
            fn(torch.zeros(100, 100), torch.zeros(100, 100), 65)


def test_measure_still_refuses_svcca():
    import torch
    from umlh import align
    with pytest.raises(NotImplementedError, match="svcca"):
        align.measure("svcca", torch.zeros(20, 4), torch.zeros(20, 4))


def test_restatement_reproduces_the_golden(gold):
    assert tuple(gold["cases"]) == CASES
    for name in os.listdir(os.path.join(ROOT, "tests", "golden")):
        if name.startswith("svcca"):
            assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < 1 << 20, name
    for case in CASES:
        a, b, q = gold[f"{case}/a"], gold[f"{case}/b"], int(gold[f"{case}/q"])
        assert a.dtype == np.float32 and b.dtype == np.float32
        assert (a.shape[0], a.shape[1], b.shape[1], q) == SHAPES[case] and b.shape[0] == a.shape[0]
        rho = R.rho64(a, b, q)
        np.testing.assert_allclose(rho, gold[f"{case}/rho64"], rtol=0, atol=1e-13)
        assert abs(R.svcca64(a, b, q) - float(gold[f"{case}/closed64"])) <= 1e-13
        assert (np.diff(rho) <= 0).all() and rho.min() >= 0.0 and rho.max() <= 1.0
    assert (gold["offset/a"][:, 17] == np.float32(3.25)).all() and (gold["offset/b"][:, 40] == np.float32(-0.4375)).all()
    assert float(gold["same/closed64"]) > 1.0 - 1e-12


@pytest.mark.parametrize("case", CASES)
def test_reference_values_lie_within_the_bound_of_the_closed_form(gold, case):
    """A condition on the inputs, not on the code under test: where sigma_q is separated from sigma_(q+1) the reference's
    randomised SVD + CCA lands on the closed form, whatever the seed and the precision."""
    closed, bound = float(gold[f"{case}/closed64"]), float(gold[f"{case}/bound"])
    ref = np.concatenate([gold[f"{case}/ref32"], gold[f"{case}/ref64"]])
    assert ref.shape == (10,) and 0.0 < bound <= 1e-4
    err = np.abs(ref - closed)
    print(f"{case}: reference max |error| fp32 {err[:5].max():.3e} fp64 {err[5:].max():.3e} (bound {bound:.0e})")
    assert err.max() <= bound
    a, b, q = gold[f"{case}/a"], gold[f"{case}/b"], int(gold[f"{case}/q"])
    for x in (a, b):                                        # the planted gap that makes it so
        s = np.linalg.svd(R.standardise64(x), compute_uv=False)
        assert q == len(s) or s[q] / s[q - 1] <= 0.15, (case, s[q] / s[q - 1])


def test_restatement_eigenpairs_and_edge_cases():
    g = np.random.default_rng(5)
    a = g.standard_normal((50, 7)).astype(np.float32)
    a[:, 3] = 2.5                                           # a constant column is an exactly zero column after standardising
    x = R.standardise64(a)
    assert (x[:, 3] == 0.0).all() and abs(x[:, 0].std(ddof=1) - 1.0) < 1e-7
    G = R.gram64(a, True)
    lam, v, all_lam = R.top_eigh(G, 3)
    assert lam.shape == (3,) and v.shape == (7, 3) and all_lam.shape == (7,) and (np.diff(all_lam) <= 0).all()
    res, orth = R.eig_ratios(G, lam, v)
    assert res < 8 and orth < 8
    assert all(v[np.argmax(np.abs(v[:, k])), k] > 0 for k in range(3))
    np.testing.assert_allclose(np.sqrt(R.top_eigh(R.gram64(a, False), 3)[0]), np.linalg.svd(a.astype(np.float64), compute_uv=False)[:3],
                               rtol=1e-12)
    assert abs(R.svcca64(a, a, 3) - 1.0) < 1e-12
