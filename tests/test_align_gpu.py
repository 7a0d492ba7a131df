"""GPU: the alignment metrics on the HIP kernels (umlh.align, metrics.py, the Gaussian wiring) against the reference's
recorded values and the float64 restatement (tests/_align_ref.py)."""
import numpy as np
import pytest
import torch

import _align_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("gauss", "offset", "wide", "ragged", "tiny", "toy")


@pytest.fixture(scope="module")
def gold():
    return load_golden("alignment")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("case", CASES)
def test_golden_cka(gold, case):
    from umlh import align
    a, b = dev(gold[f"{case}/a"]), dev(gold[f"{case}/b"])
    out = align.cka_terms(a, b).cpu().numpy()
    c64, ref = gold[f"{case}/cka64"], float(gold[f"{case}/ref_cka"])
    assert abs(out[0] - c64[0]) <= 1e-5, (case, out[0], c64[0])
    assert abs(out[0] - ref) <= 1e-5 + abs(ref - c64[0]), (case, out[0], ref)
    np.testing.assert_allclose(out[1:], c64[1:], rtol=1e-5)


@pytest.mark.parametrize("case", CASES)
def test_golden_neighbours_and_mutual_knn(gold, case):
    from umlh import align
    und = int(gold[f"{case}/undecidable"])
    for v in ("a", "b"):
        x = gold[f"{case}/{v}"]
        _, s64 = R.knn64(x, 10)
        ok = R.list_decidable(s64, R.tau(x), 10)
        got = align.knn(dev(x), 10).cpu().numpy()
        np.testing.assert_array_equal(got[ok], gold[f"{case}/ref_knn_{v}"][ok])
        if case not in ("offset", "toy"):
            assert ok.mean() >= 0.99
    a, b = dev(gold[f"{case}/a"]), dev(gold[f"{case}/b"])
    n = a.shape[0]
    for k in (1, 10, 32):
        m = float(align.mutual_knn(a, b, k))
        assert abs(m - float(gold[f"{case}/ref_mknn_k{k}"])) <= 1e-6 + und / n, (case, k, m)
        assert abs(m - float(gold[f"{case}/mknn64_k{k}"])) <= 1e-12 + und / n, (case, k, m)


def edge_views(xa, xb, strided):
    """The pair on the device: dense, or as row-strided views whose padding columns hold NaN."""
    if not strided:
        return dev(xa), dev(xb)
    out = []
    for x, pad in ((xa, 3), (xb, 2)):
        w = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=DEV)
        w[:, :x.shape[1]] = dev(x)
        out.append(w[:, :x.shape[1]])
    return out


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("n,da,db", R.TILE_EDGES)
def test_tile_edge_cka(n, da, db, strided):
    """test_golden_cka's bounds against float64 at the tile-edge shapes, for every way the rows are chunked."""
    from umlh import align
    xa, xb = R.tile_edge_pair(n, da, db)
    a, b = edge_views(xa, xb, strided)
    c64 = R.cka64(xa, xb)
    for splits in (1, 3, 0):
        out = align.cka_terms(a, b, splits=splits).cpu().numpy()
        print(f"cka[{n},{da},{db},strided={strided},splits={splits}]: got {out!r} ref64 {c64!r}")
        assert abs(out[0] - c64[0]) <= 1e-5, (splits, out[0], c64[0])
        np.testing.assert_allclose(out[1:], c64[1:], rtol=1e-5)


def _tie_features(n, d, seed):
    g = np.random.default_rng(seed)
    return g.integers(-2, 3, (n, d)).astype(np.float32)   # every score an exact small integer: many ties


@pytest.mark.parametrize("n,d,k", [(300, 3, 10), (1000, 5, 32), (777, 2, 7), (64, 1, 5)])
def test_ties_follow_score_desc_index_asc_for_any_splits(n, d, k):
    from umlh import align
    x = _tie_features(n, d, n + d)
    full = x.astype(np.float64) @ x.T.astype(np.float64)
    np.fill_diagonal(full, -np.inf)
    want_i = np.stack([np.lexsort((np.arange(n), -full[r]))[:k] for r in range(n)])
    want_s = np.take_along_axis(full, want_i, 1).astype(np.float32)
    runs = [align.knn(dev(x), k, splits=s, return_scores=True) for s in (1, 2, 7, 0)]
    for i_, s_ in runs:
        np.testing.assert_array_equal(i_.cpu().numpy(), want_i)
        np.testing.assert_array_equal(s_.cpu().numpy(), want_s)


@pytest.mark.parametrize("n,d,k", [(255, 7, 1), (256, 1, 32), (257, 33, 24), (2048, 7, 32), (33, 3, 32), (6, 1, 5)])
def test_tile_boundary_and_width_edges_are_exact(n, d, k):
    """One column short of a tile, a whole tile, one column over, eight tiles; list widths 1, 24 and 32 (the widest), k = n - 1
    (every other row is a neighbour) and n below one strip.  Integer features: every fp32 score is exact."""
    from umlh import align
    x = _tie_features(n, d, n + d)
    full = x.astype(np.float64) @ x.T.astype(np.float64)
    np.fill_diagonal(full, -np.inf)
    want_i = np.stack([np.lexsort((np.arange(n), -full[r]))[:k] for r in range(n)])
    want_s = np.take_along_axis(full, want_i, 1).astype(np.float32)
    xd = dev(x)
    for splits in (1, 2, 3, 0):
        i_, s_ = align.knn(xd, k, splits=splits, return_scores=True)
        np.testing.assert_array_equal(i_.cpu().numpy(), want_i, err_msg=f"splits={splits}")
        np.testing.assert_array_equal(s_.cpu().numpy(), want_s, err_msg=f"splits={splits}")


def test_a_nan_row_fills_only_its_own_list():
    """A NaN score beats nothing: the NaN row's list stays unfilled (indices >= n at -inf), no row lists it, and a row whose
    clean list did not hold it keeps its bits."""
    from umlh import align
    n, d, k, bad = 300, 9, 5, 13
    x = np.random.default_rng(7).standard_normal((n, d)).astype(np.float32)
    xn = x.copy()
    xn[bad] = np.nan
    for splits in (1, 3):
        clean_i, clean_s = (t.cpu().numpy() for t in align.knn(dev(x), k, splits=splits, return_scores=True))
        i_, s_ = (t.cpu().numpy() for t in align.knn(dev(xn), k, splits=splits, return_scores=True))
        assert (i_[bad] >= n).all() and (s_[bad] == -np.inf).all(), (splits, i_[bad], s_[bad])
        others = np.arange(n) != bad
        assert not (i_[others] == bad).any(), splits
        free = others & ~(clean_i == bad).any(1)
        assert 0 < free.sum() < n - 1
        assert np.array_equal(i_[free], clean_i[free]) and np.array_equal(s_[free].view(np.int32), clean_s[free].view(np.int32)), splits


def test_split_independence_on_random_features():
    from umlh import align
    g = np.random.default_rng(5)
    x = dev(g.standard_normal((2000, 100)).astype(np.float32))
    base_i, base_s = align.knn(x, 10, splits=1, return_scores=True)
    for s in (2, 3, 7, 8, 0):
        i_, s_ = align.knn(x, 10, splits=s, return_scores=True)
        assert torch.equal(i_, base_i) and torch.equal(s_, base_s), s


@pytest.mark.parametrize("n,d", [(20000, 256), (50000, 35)])
def test_large_n_against_float64(n, d):
    from umlh import align
    g = np.random.default_rng(n + d)
    z = g.standard_normal((n, 8))
    xa = (z @ g.standard_normal((8, d)) + g.standard_normal((n, d))).astype(np.float32)
    xb = (z @ g.standard_normal((8, d)) + g.standard_normal((n, d))).astype(np.float32)
    a, b = dev(xa), dev(xb)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ka = align.knn(a, 10)
    kb = align.knn(b, 10)
    m = float(align.mutual_knn_lists(ka, kb))
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 256 << 20
    # float64 on a row subset (bounded CPU work): neighbour sets on every set-decidable row, per-row mutual counts on the
    # rows decidable in both views; the mean may differ from the subset's float64 value only through undecidable rows
    rows = np.random.default_rng(1).choice(n, 512, replace=False)
    sets, decs = [], []
    for x, kk in ((xa, ka), (xb, kb)):
        x64 = x.astype(np.float64)
        s = x64[rows] @ x64.T
        s[np.arange(len(rows)), rows] = -np.inf
        part = np.argpartition(-s, 11, axis=1)[:, :11]
        ps = np.take_along_axis(s, part, 1)
        o = np.lexsort((part, -ps), axis=1)
        ps, part = np.take_along_axis(ps, o, 1), np.take_along_axis(part, o, 1)
        nrm = np.sqrt(np.square(x64).sum(1))
        dec = (ps[:, 9] - ps[:, 10]) > R.TAU_SCALE * nrm[rows] * nrm.max()
        got = np.sort(kk.cpu().numpy()[rows], 1)
        np.testing.assert_array_equal(got[dec], np.sort(part[:, :10], 1)[dec])
        sets.append(part[:, :10])
        decs.append(dec)
    both = decs[0] & decs[1]
    assert both.mean() > 0.9
    ga, gb = ka.cpu().numpy()[rows], kb.cpu().numpy()[rows]
    hits_gpu = (ga[:, :, None] == gb[:, None, :]).any(-1).sum(1)
    hits_64 = (sets[0][:, :, None] == sets[1][:, None, :]).any(-1).sum(1)
    np.testing.assert_array_equal(hits_gpu[both], hits_64[both])
    full = (ka.cpu().numpy()[:, :, None] == kb.cpu().numpy()[:, None, :]).any(-1).sum()
    assert m == float(full) / (n * 10)


def test_every_entry_point_is_deterministic(gold):
    from umlh import align
    g = np.random.default_rng(11)
    a = dev(g.standard_normal((3000, 130)).astype(np.float32))
    b = dev(g.standard_normal((3000, 70)).astype(np.float32) + 20)
    i1, s1 = align.knn(a, 16, return_scores=True)
    i2, s2 = align.knn(a, 16, return_scores=True)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    assert torch.equal(align.cka_terms(a, b), align.cka_terms(a, b))
    assert torch.equal(align.cka_terms(a, b, splits=3), align.cka_terms(a, b, splits=3))
    assert torch.equal(align.mutual_knn(a, b, 10), align.mutual_knn(a, b, 10))


def test_python_surface(gold):
    import metrics
    from umlh import align
    a, b = gold["gauss/a"], gold["gauss/b"]
    ta, tb = dev(a), dev(b)
    c = metrics.AlignmentMetrics.measure("cka", ta, tb, kernel_metric="ip")
    m = metrics.AlignmentMetrics.measure("mutual_knn", ta, tb, topk=10)
    assert isinstance(c, float) and isinstance(m, float)
    assert c == float(align.cka(ta, tb)) and m == float(align.mutual_knn(ta, tb, 10))
    assert metrics.cka(torch.from_numpy(a), torch.from_numpy(b)) == c                  # CPU inputs go to the device
    assert metrics.mknn(torch.from_numpy(a).double(), torch.from_numpy(b)) == m        # other float dtypes: upcast (exact here)
    nn = metrics.compute_nearest_neighbors(ta, 10)
    assert nn.dtype == torch.int64 and nn.is_cuda and torch.equal(nn, align.knn(ta, 10).long())
    strided = torch.zeros(a.shape[0], 128, device=DEV)
    strided[:, :100] = ta
    assert float(align.cka(strided[:, :100], tb)) == c                              # row stride passed as ld
    with pytest.raises(ValueError):
        metrics.AlignmentMetrics.measure("nope", ta, tb)
    with pytest.raises(NotImplementedError):
        metrics.AlignmentMetrics.measure("cknna", ta, tb, topk=10)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c_side = align.cka(ta, tb)
        m_side = align.mutual_knn(ta, tb, 10)
    side.synchronize()
    assert float(c_side) == c and float(m_side) == m


def test_gaussian_alignment_logging_matches_float64():
    from gaussian.data import generate_data
    from gaussian.train import build_run, train_model_steps
    cfg = {"seed": 2, "num_samples": 2048, "dim_c": 10, "dim_x": 5, "dim_y": 5, "dim_obs": 50, "noise_std": 0.09,
           "attenuate_x": True, "attenuation": 0.05, "shared_latent_distribution_type": "gaussian"}
    d = generate_data(cfg)
    loader, model, opt = build_run(d, d, mode="xy", train_num_samples=1536, batch_size=128, seed=0, device=DEV)
    vx, vy = d["x"][1536:].to(DEV), d["y"][1536:].to(DEV)
    log = train_model_steps(model, loader, opt, 8, vx, vy, DEV, eval_every=2, alignment=True)
    assert len(log["val_cka"]) == len(log["val_mknn"]) == len(log["val_loss_x"]) == 4
    model.eval()
    with torch.no_grad():
        ex, ey = model.get_embeddings(vx, vy)
    ex, ey = ex.cpu().numpy(), ey.cpu().numpy()
    assert abs(log["val_cka"][-1] - R.cka64(ex, ey)[0]) <= 1e-5
    ia, sa = R.knn64(ex, 10)
    ib, sb = R.knn64(ey, 10)
    und = int((~(R.set_decidable(sa, R.tau(ex), 10) & R.set_decidable(sb, R.tau(ey), 10))).sum())
    assert abs(log["val_mknn"][-1] - R.mutual64(ia, ib)) <= 1e-12 + und / ex.shape[0]


def test_gaussian_replay_alignment_matches_reference(gold):
    from gaussian.train import build_run, train_model_steps
    g = load_golden("gaussian_toy")
    data = {"x": torch.from_numpy(g["data_x"]), "y": torch.from_numpy(g["data_y"])}
    loader, model, opt = build_run(data, data, mode="xy", train_num_samples=600, batch_size=128, seed=0, device=DEV)
    vx, vy = torch.from_numpy(g["val_x"]).to(DEV), torch.from_numpy(g["val_y"]).to(DEV)
    log = train_model_steps(model, loader, opt, 6, vx, vy, DEV, mode="xy", alpha_x=1.0, alpha_y=0.5, eval_every=6, alignment=True)
    assert len(log["val_cka"]) == 1
    assert abs(log["val_cka"][-1] - float(gold["toy/ref_cka"])) <= 1e-4
    # rows whose k-boundary gap is below the score change the 2e-4 embedding tolerance allows may flip: 1/64 each
    n, slack = 64, 0
    for v in ("a", "b"):
        x = gold[f"toy/{v}"].astype(np.float64)
        nrm = np.sqrt(np.square(x).sum(1))
        delta = 2 * 2e-4 * np.sqrt(x.shape[1]) * (nrm + nrm.max()) + R.tau(x)
        slack += int((gold[f"toy/set_gap_{v}_k10"] <= delta).sum())
    assert abs(log["val_mknn"][-1] - float(gold["toy/ref_mknn_k10"])) <= 1e-6 + slack / n


def test_cka_is_enqueued_on_the_current_stream():
    """The wrappers hand the kernels torch's CURRENT stream: issued under a side stream and read after synchronising only that
    stream, the result has the bits of the default-stream run."""
    from umlh import align
    g = torch.Generator().manual_seed(7)
    a, b = torch.randn(64, 8, generator=g).to(DEV), torch.randn(64, 8, generator=g).to(DEV)
    want = align.cka_terms(a, b).cpu()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got = align.cka_terms(a, b)
        side.synchronize()
        got = got.cpu()
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (got, want)
