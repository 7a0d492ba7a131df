"""Singular values / effective rank without a GPU: the ABI revision and exports, the scratch query, the argument checks of
the three entry points (made before any HIP call), the float64 restatement against the golden, and the Python-level errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _spectral_ref as R
from conftest import ROOT, load_golden

NEW_SYMBOLS = ("umlh_spectral_scratch_bytes", "umlh_svdvals", "umlh_effective_rank", "umlh_effective_rank_seq")


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_abi_revision_and_exports(lib):
    from umlh import _lib
    assert lib.umlh_version() >= 8
    hdr = open(os.path.join(ROOT, "include", "umlh.h")).read()
    declared = set(re.findall(r"\b(umlh_[a-z_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "umlh_kernels_spectral.hip" in _lib.SOURCES


def test_scratch_query(lib):
    from umlh import spectral
    sb = lib.umlh_spectral_scratch_bytes
    assert sb(1, 100, 0) == 0 and sb(1, 100, 513) == 0 and sb(0, 100, 8) == 0 and sb(1, 0, 8) == 0
    assert sb(1, 2 ** 31, 8) == 0 and sb(2, 2 ** 30, 8) == 0 and sb(-1, 100, 8) == 0 and sb(1, -5, 8) == 0
    assert sb(1, 2 ** 31 - 1, 8) > 0
    for batch, n, d in ((1, 10 ** 6, 300), (8, 1600, 300), (3, 120, 24), (1, 1, 1), (1, 45, 512), (200, 50, 35)):
        chunks = batch * spectral.chunk_count(batch, n)                   # slabs over the whole call
        got = sb(batch, n, d)
        assert 0 < got < 64 * d * d * 8 * (chunks + batch), (batch, n, d, got)
        assert got >= d * d * 8 * (chunks + batch)
    # no n x d growth: past the chunk cap the size does not move with n at all
    assert sb(1, 10 ** 6, 300) == sb(1, 10 ** 8, 300) == sb(1, 128 * 256, 300)
    assert spectral.chunk_count(1, 10 ** 6) == 128 and spectral.chunk_count(8, 1600) == 7 and spectral.chunk_count(500, 10 ** 4) == 1
    assert spectral.chunk_count(1, 1) == 1 and spectral.chunk_count(1, 257) == 2


def _expect(lib, rc, who, what):
    msg = lib.umlh_last_error()
    assert rc == -1 and who in msg and what in msg, (rc, msg, what)


def test_dense_entry_points_validate_arguments(lib):
    f, big = C.c_void_p(64), 1 << 40                       # never dereferenced: every check comes first
    sv = lambda a=f, batch=2, n=100, d=8, ldb=800, ldr=8, out=f, scratch=f, nbytes=big: lib.umlh_svdvals(
        a, batch, n, d, ldb, ldr, out, scratch, nbytes, None)
    er = lambda a=f, batch=2, n=100, d=8, ldb=800, ldr=8, eps=1e-6, out=f, scratch=f, nbytes=big: lib.umlh_effective_rank(
        a, batch, n, d, ldb, ldr, eps, out, None, scratch, nbytes, None)
    for fn, who in ((sv, b"umlh_svdvals"), (er, b"umlh_effective_rank")):
        _expect(lib, fn(a=None), who, b"null")
        _expect(lib, fn(out=None), who, b"null")
        _expect(lib, fn(scratch=None), who, b"null")
        _expect(lib, fn(nbytes=lib.umlh_spectral_scratch_bytes(2, 100, 8) - 1), who, b"scratch")
        _expect(lib, fn(nbytes=0), who, b"scratch")
        _expect(lib, fn(ldr=7), who, b"ld_row=7")
        _expect(lib, fn(d=0), who, b"d=0")
        _expect(lib, fn(d=513, ldr=513, ldb=51300), who, b"d=513")
        _expect(lib, fn(batch=0), who, b"batch=0")
        _expect(lib, fn(n=0), who, b"n=0")
        _expect(lib, fn(batch=2, n=2 ** 30, ldb=2 ** 33), who, b"batch=2")
        _expect(lib, fn(ldb=799), who, b"ld_batch=799")
    for bad in (-1.0, float("inf"), float("nan")):
        _expect(lib, er(eps=bad), b"umlh_effective_rank", b"eps")


def test_sequence_entry_point_validates_arguments(lib):
    f, big = C.c_void_p(64), 1 << 40
    sq = lambda z=f, b=5, t=9, d=24, ldb=216, ldt=24, lengths=None, drop=1, eps=1e-6, out=f, scratch=f, nbytes=big: \
        lib.umlh_effective_rank_seq(z, b, t, d, ldb, ldt, lengths, drop, eps, out, None, scratch, nbytes, None)
    who = b"umlh_effective_rank_seq"
    _expect(lib, sq(z=None), who, b"null")
    _expect(lib, sq(out=None), who, b"null")
    _expect(lib, sq(scratch=None), who, b"null")
    _expect(lib, sq(nbytes=lib.umlh_spectral_scratch_bytes(1, 45, 24) - 1), who, b"scratch")
    _expect(lib, sq(ldt=23), who, b"ldt=23")
    _expect(lib, sq(ldb=23, ldt=120), who, b"ldb=23")
    _expect(lib, sq(ldb=215), who, b"overlap")
    _expect(lib, sq(drop=-1), who, b"drop_last=-1")
    _expect(lib, sq(d=513, ldb=513 * 9, ldt=513), who, b"d=513")
    _expect(lib, sq(d=0), who, b"d=0")
    _expect(lib, sq(b=0), who, b"b=0")
    _expect(lib, sq(t=0), who, b"t_len=0")
    _expect(lib, sq(b=2 ** 16, t=2 ** 15, ldb=2 ** 15 * 24), who, b"2^31")
    _expect(lib, sq(eps=-1e-6), who, b"eps")


def test_restatement_reproduces_the_golden():
    g = load_golden("effective_rank")
    assert tuple(g["cases"]) == ("ragged", "wide", "batch3", "rank5")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "effective_rank.npz")) < 1 << 20
    for case in g["cases"]:
        a = g[f"{case}/a"]
        a3 = a if a.ndim == 3 else a[None]
        assert a.dtype == np.float32 and g[f"{case}/sv64"].shape == (a3.shape[0], min(a3.shape[1:]))
        np.testing.assert_allclose(R.svdvals64(a3), g[f"{case}/sv64"], rtol=0, atol=1e-13 * g[f"{case}/sv64"].max())
        np.testing.assert_allclose(R.erank64(a3), g[f"{case}/erank64"], rtol=1e-12)
        for b in range(a3.shape[0]):                   # the recorded errors of the reference are those of its recorded outputs
            e = R.errors(g[f"{case}/ref_sv"][b], g[f"{case}/ref_erank"][b], g[f"{case}/sv64"][b], g[f"{case}/erank64"][b])
            np.testing.assert_allclose(e, (g[f"{case}/ref_sv_err"][b], g[f"{case}/ref_erank_err"][b]), rtol=1e-9)
            assert 0 < e[0] < 1e-5 and e[1] < 1e-4
    assert np.linalg.matrix_rank(g["rank5/a"].astype(np.float64), tol=1e-4) == 5
    assert g["wide/a"].shape == (40, 64) and g["wide/sv64"].shape == (1, 40)


def test_row_predicate_and_edge_cases_of_the_restatement():
    z = np.arange(5 * 9 * 2, dtype=np.float64).reshape(5, 9, 2)
    lens = [9, 1, 4, 9, 2]
    assert R.valid_rows(z, lens, 0).shape[0] == 25 and R.valid_rows(z, lens, 1).shape[0] == 20
    assert R.valid_rows(z, None, 1).shape[0] == 40 and R.valid_rows(z, [20, -3, 0, 9, 9], 0).shape[0] == 27
    np.testing.assert_array_equal(R.valid_rows(z, lens, 1)[8], z[2, 0])
    assert R.erank_seq64(z, [1] * 5, 1) == (1.0, 0)
    assert np.isnan(R.erank64(np.zeros((4, 3))))
    assert abs(R.erank64(np.eye(4)) - np.exp(-np.log(0.25 + 1e-6))) < 1e-12


def test_utilis_exposes_the_reference_names():
    from multibench import utilis
    for name in ("set_seed", "cka", "mknn", "compute_effective_rank"):
        assert callable(getattr(utilis, name)), name
    import torch
    with pytest.raises(ValueError, match=r"\(B, N, D\)"):
        utilis.compute_effective_rank(torch.zeros(4, 3))


def test_python_surface_validates_before_the_gpu(monkeypatch):
    import torch
    import umlh
    from umlh import spectral

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(spectral, "load_library", no_library)
    monkeypatch.setattr(spectral, "_device", no_library)
    assert umlh.svdvals is spectral.svdvals and umlh.effective_rank is spectral.effective_rank
    assert umlh.effective_rank_seq is spectral.effective_rank_seq
    for fn in (spectral.svdvals, spectral.effective_rank):
        with pytest.raises(ValueError, match="2-D"):
            fn(torch.zeros(7))
        with pytest.raises(ValueError, match="floating-point"):
            fn(torch.zeros(7, 3, dtype=torch.int32))
        with pytest.raises(ValueError, match="d=513"):
            fn(torch.zeros(7, 513))
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(0, 3))
    with pytest.raises(ValueError, match="3-D"):
        spectral.effective_rank_seq(torch.zeros(7, 3))
    with pytest.raises(ValueError, match="floating-point"):
        spectral.effective_rank_seq(torch.zeros(2, 7, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="d=513"):
        spectral.effective_rank_seq(torch.zeros(2, 3, 513))
    with pytest.raises(ValueError, match="drop_last=-1"):
        spectral.effective_rank_seq(torch.zeros(2, 3, 4), drop_last=-1)
    with pytest.raises(ValueError, match="3 lengths for 2"):
        spectral.effective_rank_seq(torch.zeros(2, 3, 4), torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="eps"):
        spectral.effective_rank(torch.zeros(7, 3), eps=-1.0)


def test_train_keeps_its_signature_and_gains_the_switch():
    import inspect
    from multibench import train as mbt
    names = list(inspect.signature(mbt.train).parameters)
    assert names[-2:] == ["on_step", "effective_rank"]
    assert inspect.signature(mbt.train).parameters["effective_rank"].default is False
