"""GPU: unbiased / RBF CKA, CKNNA and the k-NN list statistics on the HIP kernels (umlh.align) against the reference's
recorded float64 values (tests/golden/alignment_ext.npz; inputs: the `alignment` fixture) and the float64 restatement
(tests/_align_ext_ref.py).  Tolerances are those of tests/test_align_gpu.py: 1e-5 absolute on a CKA value, rtol 1e-5 on the
HSIC terms."""
import math

import numpy as np
import pytest
import torch

import _align_ext_ref as X
import _align_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("gauss", "offset", "wide", "ragged", "tiny", "toy")


@pytest.fixture(scope="module")
def gold():
    return load_golden("alignment")


@pytest.fixture(scope="module")
def ext():
    return load_golden("alignment_ext")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _close_to_both(got, ref64, ref32, what):
    print(f"{what}: got {got!r} ref64 {ref64!r} ref32 {ref32!r} |got-ref64| {abs(got - ref64):.3e}")
    assert abs(got - ref64) <= 1e-5, (what, got, ref64)
    if math.isfinite(ref32):
        assert abs(got - ref32) <= 1e-5 + abs(ref32 - ref64), (what, got, ref32)


@pytest.mark.parametrize("case", CASES)
def test_golden_unbiased_cka(gold, ext, case):
    from umlh import align
    out = align.unbiased_cka_terms(dev(gold[f"{case}/a"]), dev(gold[f"{case}/b"])).cpu().numpy()
    ref32 = float(ext[f"{case}/ucka_ref32"])
    assert math.isfinite(ref32) == (case != "offset")            # the reference's own fp32 run returns NaN there
    print(case, "terms", out[1:], ext[f"{case}/uhsic_ref64"], "rel", np.abs(out[1:] / ext[f"{case}/uhsic_ref64"] - 1).max())
    _close_to_both(float(out[0]), float(ext[f"{case}/ucka_ref64"]), ref32, f"unbiased_cka[{case}]")
    np.testing.assert_allclose(out[1:], ext[f"{case}/uhsic_ref64"], rtol=1e-5)


@pytest.mark.parametrize("unbiased", [False, True])
@pytest.mark.parametrize("setting", ["norm", "raw"])
@pytest.mark.parametrize("case", CASES)
def test_golden_rbf_cka(gold, ext, case, setting, unbiased):
    from umlh import align
    a, b = gold[f"{case}/a"], gold[f"{case}/b"]
    if setting == "norm":                    # the reference's demo: rows L2-normalised in fp32, sigma = 1
        a, b, sigma = X.normalize_rows(a), X.normalize_rows(b), 1.0
    else:                                    # raw rows, sigma = the recorded mean median pairwise distance
        sigma = float(ext[f"{case}/rbf_raw_sigma"])
    got = float(align.rbf_cka(dev(a), dev(b), sigma, unbiased))
    want = float(ext[f"{case}/rbf_{setting}_{'u' if unbiased else 'b'}_ref64"])
    print(f"rbf_cka[{case},{setting},{unbiased}]: got {got!r} ref64 {want!r} diff {abs(got - want):.3e}")
    assert abs(got - want) <= 1e-5, (case, setting, unbiased, got, want)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("n,da,db", R.TILE_EDGES)
def test_tile_edge_unbiased_and_rbf_cka(n, da, db, strided):
    """The bounds of test_golden_unbiased_cka and test_golden_rbf_cka against float64 at the tile-edge shapes of
    tests/test_align_gpu.py, for every way the rows are chunked; sigma = the mean median pairwise distance."""
    from test_align_gpu import edge_views
    from umlh import align
    xa, xb = R.tile_edge_pair(n, da, db)
    a, b = edge_views(xa, xb, strided)
    u64, sigma = X.unbiased_cka64(xa, xb), X.median_sigma(xa, xb)
    r64 = {u: X.rbf_cka64(xa, xb, sigma, u) for u in (False, True)}
    for splits in (1, 3, 0):
        out = align.unbiased_cka_terms(a, b, splits=splits).cpu().numpy()
        print(f"unbiased_cka[{n},{da},{db},strided={strided},splits={splits}]: got {out!r} ref64 {u64!r}")
        assert abs(out[0] - u64[0]) <= 1e-5, (splits, out[0], u64[0])
        np.testing.assert_allclose(out[1:], u64[1:], rtol=1e-5)
        for u in (False, True):
            got = float(align.rbf_cka(a, b, sigma, u, splits=splits))
            print(f"rbf_cka[{n},{da},{db},strided={strided},unbiased={u},splits={splits}]: got {got!r} ref64 {r64[u][0]!r}")
            assert abs(got - r64[u][0]) <= 1e-5, (splits, u, got, r64[u][0])


@pytest.mark.parametrize("k", [10, 32])
def test_golden_cknna(gold, ext, k):
    from umlh import align
    checked = 0
    for case in CASES:
        if int(gold[f"{case}/undecidable"]) != 0:        # neighbour sets within fp32 noise of a tie: not decided
            continue
        got = float(align.cknna(dev(gold[f"{case}/a"]), dev(gold[f"{case}/b"]), k))
        _close_to_both(got, float(ext[f"{case}/cknna_k{k}_ref64"]), float(ext[f"{case}/cknna_k{k}_ref32"]), f"cknna[{case},k={k}]")
        checked += 1
    assert checked >= 5


@pytest.mark.parametrize("case", ["gauss", "wide", "ragged", "tiny", "toy"])
def test_list_statistics_against_restatement(gold, ext, case):
    from umlh import align
    a, b = gold[f"{case}/a"], gold[f"{case}/b"]
    ka, sa = R.knn64(a, 10)
    kb, sb = R.knn64(b, 10)
    ok = R.list_decidable(sa, R.tau(a), 10) & R.list_decidable(sb, R.tau(b), 10)
    want = X.list_rows(ka, kb)
    out, rows = align.list_stats(align.knn(dev(a), 10), align.knn(dev(b), 10), return_rows=True)
    rows, out = rows.cpu().numpy(), out.cpu().numpy()
    if case == "toy":                        # the toy's 64 embeddings are fixed by the training replay: decidable rows only
        assert ok.sum() >= 63
        np.testing.assert_array_equal(rows[ok], want[ok])
        return
    assert ok.all()
    np.testing.assert_array_equal(rows, want)
    np.testing.assert_allclose(out, X.list_means(want, 10), rtol=0, atol=1e-12)
    assert abs(out[0] - float(ext[f"{case}/cycle_k10_ref64"])) <= 1e-6
    assert abs(out[1] - float(ext[f"{case}/lcs_k10_ref64"])) <= 1e-6
    for fn, i in ((align.cycle_knn, 0), (align.lcs_knn, 1), (align.edit_distance_knn, 2)):
        assert float(fn(dev(a), dev(b), 10)) == out[i]


def _hand_lists(n, k, seed):
    """Row i's pair of k-lists by i % 5: identical, reversed, disjoint, rotated by one, two permutations of one pool."""
    g = np.random.default_rng(seed)
    ka, kb = np.empty((n, k), np.int32), np.empty((n, k), np.int32)
    h = n // 2
    for i in range(n):
        a = g.choice(n, k, replace=False)
        kind = i % 5
        if kind == 0:
            b = a.copy()
        elif kind == 1:
            b = a[::-1]
        elif kind == 2:                      # no common value (values repeat inside a list where n < 2k)
            a = (i + np.arange(k)) % h
            b = h + (i + np.arange(k)) % (n - h)
        elif kind == 3:
            b = np.roll(a, 1)
        else:
            b = g.permutation(a)
        ka[i], kb[i] = a, b
    return ka, kb


@pytest.mark.parametrize("k", [1, 2, 10, 32])
@pytest.mark.parametrize("n_kind", ["k+1", 257, 1000])
def test_list_stats_on_hand_made_lists(k, n_kind):
    from umlh import align
    n = k + 1 if n_kind == "k+1" else n_kind
    ka, kb = _hand_lists(n, k, 100 * k + n)
    want = X.list_rows(ka, kb)
    out, rows = align.list_stats(dev(ka), dev(kb), return_rows=True)
    np.testing.assert_array_equal(rows.cpu().numpy(), want)
    assert tuple(out.cpu().numpy()) == X.list_means(want, k)
    for kind, (lcs, dist) in ((0, (k, 0)), (2, (0, k))):                 # identical and disjoint lists: known values
        sel = np.arange(n) % 5 == kind
        assert (want[sel, 1] == lcs).all() and (want[sel, 2] == dist).all()


def test_determinism_and_splits():
    from umlh import align
    g = np.random.default_rng(11)
    z = g.standard_normal((3000, 6))
    a = dev((z @ g.standard_normal((6, 130)) + g.standard_normal((3000, 130))).astype(np.float32))
    b = dev((z @ g.standard_normal((6, 70)) + g.standard_normal((3000, 70))).astype(np.float32) + 20)
    for s in (0, 3):
        assert torch.equal(align.unbiased_cka_terms(a, b, s), align.unbiased_cka_terms(a, b, s))
        for u in (False, True):
            assert torch.equal(align.rbf_cka_terms(a, b, 15.0, u, s), align.rbf_cka_terms(a, b, 15.0, u, s))
        assert torch.equal(align.cknna_terms(a, b, 10, s), align.cknna_terms(a, b, 10, s))
    ka, kb = align.knn(a, 10), align.knn(b, 10)
    o1, r1 = align.list_stats(ka, kb, return_rows=True)
    o2, r2 = align.list_stats(ka, kb, return_rows=True)
    assert torch.equal(o1, o2) and torch.equal(r1, r2)
    # the lists do not depend on splits, so neither do CKNNA and the list statistics, bit for bit
    base = align.cknna_terms(a, b, 10, 1)
    assert torch.isfinite(base).all()
    for s in (2, 3, 7, 0):
        assert torch.equal(align.cknna_terms(a, b, 10, s), base), s
        assert torch.equal(align.list_stats(align.knn(a, 10, s), align.knn(b, 10, s)), o1), s
        assert torch.equal(align.lcs_knn(a, b, 10, s), o1[1])
    for u in (False, True):
        base = align.rbf_cka_terms(a, b, 15.0, u, 1).cpu().numpy()
        for s in (3, 0):
            np.testing.assert_allclose(align.rbf_cka_terms(a, b, 15.0, u, s).cpu().numpy(), base, rtol=1e-12, atol=0)


def test_no_quadratic_memory_and_float64_at_8191():
    from umlh import align
    n, d_a, d_b, sigma = 8191, 40, 24, 20.0
    g = np.random.default_rng(n)
    z = g.standard_normal((n, 8))
    xa = (z @ g.standard_normal((8, d_a)) + g.standard_normal((n, d_a))).astype(np.float32)
    xb = (z @ g.standard_normal((8, d_b)) + g.standard_normal((n, d_b))).astype(np.float32)
    a, b = dev(xa), dev(xb)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = {"rbf_b": align.rbf_cka(a, b, sigma, False), "rbf_u": align.rbf_cka(a, b, sigma, True),
           "lin_u": align.unbiased_cka(a, b), "cknna": align.cknna(a, b, 10)}
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 64 << 20           # one N x N fp32 array is 268 MB
    got = {k: float(v) for k, v in got.items()}
    assert math.isfinite(got["cknna"])
    sums = X.pair_sums64_blocked(xa, xb, sigma)
    want = {"rbf_b": X.cka64_from_sums(sums, False)[0], "rbf_u": X.cka64_from_sums(sums, True)[0],
            "lin_u": X.unbiased_cka64_blocked(xa, xb)[0]}
    for k, w in want.items():
        print(f"{k}: got {got[k]!r} float64 {w!r} diff {abs(got[k] - w):.3e}")
        assert abs(got[k] - w) <= 1e-5, (k, got[k], w)


def test_python_surface(gold):
    from umlh import align
    a, b = gold["gauss/a"], gold["gauss/b"]
    ta, tb = dev(a), dev(b)
    direct = {
        ("cycle_knn", (("topk", 10),)): align.cycle_knn(ta, tb, 10),
        ("mutual_knn", (("topk", 10),)): align.mutual_knn(ta, tb, 10),
        ("lcs_knn", (("topk", 10),)): align.lcs_knn(ta, tb, 10),
        ("edit_distance_knn", (("topk", 10),)): align.edit_distance_knn(ta, tb, 10),
        ("cka", ()): align.cka(ta, tb),
        ("cka", (("kernel_metric", "ip"),)): align.cka(ta, tb),
        ("cka", (("unbiased", True),)): align.unbiased_cka(ta, tb),
        ("cka", (("kernel_metric", "rbf"), ("rbf_sigma", 40.0))): align.rbf_cka(ta, tb, 40.0),
        ("cka", (("kernel_metric", "rbf"), ("rbf_sigma", 40.0), ("unbiased", True))): align.rbf_cka(ta, tb, 40.0, True),
        ("unbiased_cka", ()): align.unbiased_cka(ta, tb),
        ("unbiased_cka", (("kernel_metric", "rbf"), ("rbf_sigma", 40.0))): align.rbf_cka(ta, tb, 40.0, True),
        ("cknna", (("topk", 10),)): align.cknna(ta, tb, 10),
        ("cknna", (("topk", 10), ("distance_agnostic", False), ("unbiased", True))): align.cknna(ta, tb, 10),
    }
    for (name, kw), want in direct.items():
        got = align.measure(name, ta, tb, **dict(kw))
        assert isinstance(got, float) and got == float(want), (name, kw, got, float(want))
        assert want.dtype == torch.float64 and want.ndim == 0 and want.is_cuda
    u, r, c = float(align.unbiased_cka(ta, tb)), float(align.rbf_cka(ta, tb, 40.0)), float(align.cknna(ta, tb, 10))
    ca, cb = torch.from_numpy(a), torch.from_numpy(b)
    assert float(align.unbiased_cka(ca, cb)) == u                                   # CPU inputs go to the device
    assert float(align.rbf_cka(ca.double(), cb, 40.0)) == r                         # other float dtypes: upcast (exact here)
    assert float(align.cknna(ca, cb.double(), 10)) == c
    strided = torch.zeros(a.shape[0], 128, device=DEV)
    strided[:, :100] = ta
    assert float(align.unbiased_cka(strided[:, :100], tb)) == u                     # row stride passed as ld
    assert float(align.rbf_cka(strided[:, :100], tb, 40.0)) == r
    assert float(align.cknna(strided[:, :100], tb, 10)) == c
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        u_side, r_side, c_side = align.unbiased_cka(ta, tb), align.rbf_cka(ta, tb, 40.0), align.cknna(ta, tb, 10)
        l_side = align.lcs_knn(ta, tb, 10)
    side.synchronize()
    assert (float(u_side), float(r_side), float(c_side)) == (u, r, c) and float(l_side) == float(align.lcs_knn(ta, tb, 10))
    with pytest.raises(NotImplementedError):
        align.measure("svcca", ta, tb)
    with pytest.raises(NotImplementedError):
        align.measure("cknna", ta, tb, topk=10, distance_agnostic=True)
    with pytest.raises(NotImplementedError):
        align.measure("cknna", ta, tb, topk=10, unbiased=False)
    with pytest.raises(ValueError, match="topk >= 2"):
        align.cknna(ta, tb, topk=1)
    with pytest.raises(ValueError, match="Unrecognized metric"):
        align.measure("nope", ta, tb)
    assert align.measure("cka", ta, tb, kernel_metric="ip") == float(align.cka(ta, tb))
