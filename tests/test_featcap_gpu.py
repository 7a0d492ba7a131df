"""GPU: the class index and class statistics kernels against the float64 statements of tests/_featcap_ref.py, and
finetune.train() with capture_features_during_training=True against the reference's own runs (tests/golden/feature_capture.npz,
scripts/make_golden_featcap.py).  Every measured figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import _featcap_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _T(a, t=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, t).contiguous()


@pytest.fixture(scope="module")
def cases():
    """name -> (x, y, n_class, order, offsets, float64 means, rows): the references are computed once and shared."""
    out = {}
    for name, (x, y, c) in R.stats_cases().items():
        order, offsets = R.class_index(y, c)
        rows = R.class_rows(order, offsets, c, x.shape[0])
        out[name] = (x, y, c, order, offsets, R.class_means(x, rows), rows)
    return out


# ------------------------------------------------------------------------------------------ class_index
def _index_case(name):
    rng = np.random.default_rng(7)
    if name == "interleaved":
        return np.arange(1000) % 7, 7
    if name == "all_equal":
        return np.full(777, 2), 4
    if name == "out_of_range":
        y = rng.integers(-1, 6, 900)                         # -1 and n_class = 5 among the labels
        assert (y == -1).any() and (y == 5).any()
        return y, 5
    if name == "n1":
        return np.array([0]), 3
    if name == "n1_out_of_range":
        return np.array([3]), 3
    if name == "n70001_c3":
        return rng.integers(0, 3, 70001), 3
    if name == "n5000_c1000":
        return rng.choice(np.arange(0, 1000, 3), 5000), 1000  # two classes in three are empty
    raise KeyError(name)


@pytest.mark.parametrize("name", ["interleaved", "all_equal", "out_of_range", "n1", "n1_out_of_range", "n70001_c3", "n5000_c1000"])
def test_class_index_equals_the_stable_argsort(name):
    import umlh
    y, c = _index_case(name)
    order, offsets = umlh.class_index(_T(y, torch.int64), c)
    want_order, want_offsets = R.class_index(y, c)
    order, offsets = order.cpu().numpy(), offsets.cpu().numpy()
    m = int(want_offsets[-1])
    print(f"{name}: n {len(y)} classes {c} listed {m} empty classes {int((np.diff(want_offsets) == 0).sum())}")
    assert order.dtype == np.int32 and offsets.dtype == np.int64 and order.shape == (len(y),) and offsets.shape == (c + 1,)
    np.testing.assert_array_equal(offsets, want_offsets)
    np.testing.assert_array_equal(order[:m], want_order)


def test_class_index_writes_nothing_past_the_listed_rows():
    """A sentinel-filled ``order`` one entry longer than needed: the entries past offsets[n_class] keep the sentinel."""
    import umlh
    from umlh import _glue as glue
    from umlh._lib import check, load_library
    y, c = _index_case("out_of_range")
    n = len(y)
    labels = _T(y, torch.int64)
    order = torch.full((n + 1,), -77, dtype=torch.int32, device=DEV)
    offsets = torch.empty(c + 1, dtype=torch.int64, device=DEV)
    scratch, nbytes = glue.scratch("umlh_class_index_scratch_bytes", torch.device(DEV), n=n, n_class=c)
    check(load_library().umlh_class_index(labels.data_ptr(), n, c, order.data_ptr(), offsets.data_ptr(), scratch.data_ptr(), nbytes,
                                          glue.stream(torch.device(DEV))), "umlh_class_index")
    want_order, want_offsets = R.class_index(y, c)
    m = int(want_offsets[-1])
    got = order.cpu().numpy()
    assert m < n
    np.testing.assert_array_equal(got[:m], want_order)
    assert np.all(got[m:] == -77)
    again, _ = umlh.class_index(labels, c)
    np.testing.assert_array_equal(again.cpu().numpy()[:m], want_order)


# ------------------------------------------------------------------------------------------ class_stats
def _check_stats(name, x, c, order, offsets, m64, rows, means, dist, out2):
    """The three bounds of one case; ``means`` / ``dist`` / ``out2`` are the kernel's results as numpy arrays."""
    d = x.shape[1]
    empty = np.array([r.size == 0 for r in rows])
    finite = np.isfinite(m64)
    bound = R.means_bound(np.where(finite, m64, 0.0), np.where(np.isfinite(x), x, 0.0), rows)
    err = np.where(finite, np.abs(means.astype(np.float64) - np.where(finite, m64, 0.0)), 0.0)
    print(f"{name}: means max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f} (bound up to {bound.max():.3e})")
    assert np.all(np.isnan(means[empty])) and not np.isnan(means[~empty & np.isfinite(m64).all(axis=1)]).any()
    assert np.all(err <= bound)
    np.testing.assert_array_equal(means[~finite & ~empty[:, None]], m64[~finite & ~empty[:, None]].astype(np.float32))   # +-Inf / NaN columns
    want = R.class_dists(x, rows, means)                                        # float64, from the RETURNED fp32 means
    rel_bound = R.dist_rel_bound(d, rows)
    ok = ~np.isnan(want)
    rel = np.abs(dist[ok] - want[ok]) / np.where(want[ok] > 0, want[ok], 1.0)
    print(f"{name}: dist max rel err {rel.max() if rel.size else 0.0:.3e} bound {rel_bound[ok].min() if rel.size else 0.0:.3e}"
          f" (as a fraction of it: {np.max(rel / rel_bound[ok]) if rel.size else 0.0:.3f})")
    np.testing.assert_array_equal(np.isnan(dist), np.isnan(want))
    assert np.all(rel <= rel_bound[ok])
    want2 = R.out2(dist, rows)                                                  # from the returned dist[], over n_class terms
    print(f"{name}: out2 {out2} want {want2}")
    assert out2[1] == want2[1] == empty.sum()
    if np.isnan(want2[0]):
        assert np.isnan(out2[0])
    else:
        assert abs(out2[0] - want2[0]) <= (c + 4) * 2.0 ** -53 * abs(want2[0])
    return want


@pytest.mark.parametrize("name", sorted(R.stats_cases()))
def test_class_stats_against_float64(cases, name):
    import umlh
    x, y, c, order, offsets, m64, rows = cases[name]
    means, dist, out2 = umlh.class_stats(_T(x), _T(order, torch.int32), _T(offsets, torch.int64), c)
    assert means.dtype == torch.float32 and dist.dtype == torch.float64 and out2.dtype == torch.float64
    assert means.shape == (c, x.shape[1]) and dist.shape == (c,) and out2.shape == (2,) and means.is_cuda
    means, dist, out2 = means.cpu().numpy(), dist.cpu().numpy(), out2.cpu().numpy()
    _check_stats(name, x, c, order, offsets, m64, rows, means, dist, out2)
    if name == "one_row_class":
        assert rows[3].size == 1 and dist[3] == 0.0 and np.array_equal(means[3], x[rows[3][0]])
    if name == "empty_class":
        assert rows[2].size == 0 and np.isnan(means[2]).all() and np.isnan(dist[2]) and np.isnan(out2[0]) and out2[1] == 1
    if name == "one_class_5000_rows":
        assert rows[0].size == 5000
    # the index built on the device gives the same plan, hence the same bits
    o_dev, off_dev = umlh.class_index(_T(y, torch.int64), c)
    m2, d2, o2 = umlh.class_stats(_T(x), o_dev, off_dev, c)
    assert np.array_equal(m2.cpu().numpy(), means, equal_nan=True) and np.array_equal(d2.cpu().numpy(), dist, equal_nan=True)
    assert np.array_equal(o2.cpu().numpy(), out2, equal_nan=True)


def test_class_stats_strided_inputs_and_a_sentinel_means_buffer(cases):
    """ld > d (a column block of a wider matrix, which also takes the 4-byte load path), and ld_means > d in a NaN-sentinel
    buffer one row longer than needed: same bits as the dense call, nothing written outside means[:, :d]."""
    import umlh
    for name in ("d64", "d65", "one_class_5000_rows"):
        x, y, c, order, offsets, m64, rows = cases[name]
        n, d = x.shape
        dense = umlh.class_stats(_T(x), _T(order, torch.int32), _T(offsets, torch.int64), c)
        for pad_x, pad_m, shift in ((4, 8, 0), (3, 5, 1)):
            wide = torch.full((n, d + pad_x + shift), 1e30, dtype=torch.float32, device=DEV)
            wide[:, shift:shift + d] = _T(x)
            buf = torch.full((c + 1, d + pad_m), float("nan"), dtype=torch.float32, device=DEV)
            buf[:, d:] = -5.0
            buf[c] = -6.0
            means, dist, out2 = umlh.class_stats(wide[:, shift:shift + d], _T(order, torch.int32), _T(offsets, torch.int64), c,
                                                 means_out=buf[:c, :d])
            assert means.data_ptr() == buf.data_ptr()
            same = (torch.equal(buf[:c, :d], dense[0]), torch.equal(dist, dense[1]), torch.equal(out2, dense[2]))
            print(f"{name} ld {wide.stride(0)} ld_means {buf.stride(0)} offset {shift}: bit-equal to the dense call {same}")
            assert all(same)
            assert bool((buf[:c, d:] == -5.0).all()) and bool((buf[c] == -6.0).all())
            assert bool((wide[:, :shift] == 1e30).all()) and bool((wide[:, shift + d:] == 1e30).all())


def test_class_stats_inf_poisons_exactly_one_class(cases):
    import umlh
    x, y, c, order, offsets, m64, rows = cases["d65"]
    clean = umlh.class_stats(_T(x), _T(order, torch.int32), _T(offsets, torch.int64), c)
    bad = x.copy()
    victim = int(rows[4][1])
    bad[victim, 17] = np.inf
    means, dist, out2 = (t.cpu().numpy() for t in umlh.class_stats(_T(bad), _T(order, torch.int32), _T(offsets, torch.int64), c))
    cm, cd = clean[0].cpu().numpy(), clean[1].cpu().numpy()
    others = np.arange(c) != 4
    print(f"class 4: mean[17] {means[4, 17]} dist {dist[4]}; out2 {out2}")
    assert np.array_equal(means[others], cm[others]) and np.array_equal(dist[others], cd[others])
    assert means[4, 17] == np.inf and np.array_equal(np.delete(means[4], 17), np.delete(cm[4], 17))
    assert np.isnan(dist[4]) and np.isnan(out2[0]) and out2[1] == 0
    _check_stats("d65+inf", bad, c, order, offsets, R.class_means(bad, rows), rows, means, dist, out2)


def test_class_stats_bit_equal_across_calls_and_streams(cases):
    import umlh
    for name in ("d257", "1000x16_d32", "one_class_5000_rows"):
        x, y, c, order, offsets, m64, rows = cases[name]
        xt, ot, ft = _T(x), _T(order, torch.int32), _T(offsets, torch.int64)
        a = umlh.class_stats(xt, ot, ft, c)
        b = umlh.class_stats(xt, ot, ft, c)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            s = umlh.class_stats(xt, ot, ft, c)
        side.synchronize()
        for got in (b, s):
            assert all(torch.equal(p.view(torch.int32 if p.dtype == torch.float32 else torch.int64),
                                   q.view(torch.int32 if q.dtype == torch.float32 else torch.int64)) for p, q in zip(a, got)), name


def test_class_stats_ignores_the_bad_entries_of_a_stale_plan(cases):
    """``order`` holding n and -1, offsets reaching past n and going backwards: the call completes, those entries are ignored."""
    import umlh
    x, y, c, order, offsets, m64, rows = cases["d63"]
    n = x.shape[0]
    stale_order = order.copy()
    stale_order[[3, 40, 41]] = [n, -1, n + 5]
    assert len(stale_order) == n
    stale_offsets = offsets.copy()
    stale_offsets[2] = stale_offsets[1] - 3                   # goes backwards: class 1 is read as empty, class 2 starts at offsets[1]
    stale_offsets[-1] = n + 1000
    rows_s = R.class_rows(stale_order, stale_offsets, c, n)
    means, dist, out2 = (t.cpu().numpy() for t in umlh.class_stats(_T(x), _T(stale_order, torch.int32), _T(stale_offsets, torch.int64), c))
    print(f"stale plan: class sizes {[r.size for r in rows_s]} (valid plan {[r.size for r in rows]})")
    assert sum(r.size for r in rows_s) == n - 3 and rows_s[1].size == 0
    _check_stats("stale", x, c, stale_order, stale_offsets, R.class_means(x, rows_s), rows_s, means, dist, out2)


def test_bindings_accept_what_the_docstrings_say():
    import umlh
    x = torch.randn(30, 8, dtype=torch.float64)
    y = torch.arange(30, dtype=torch.int32) % 4                # CPU, int32 labels, fp64 features: converted
    order, offsets = umlh.class_index(y, 4)
    means, dist, out2 = umlh.class_stats(x, order, offsets, 4)
    want = torch.stack([x[y == k].mean(0) for k in range(4)]).float()
    assert torch.allclose(means.cpu(), want, atol=1e-6) and out2[1].item() == 0
    with pytest.raises(ValueError):
        umlh.class_index(torch.zeros(3), 2)
    with pytest.raises(ValueError):
        umlh.class_stats(x, order, offsets[:-1], 4)
    with pytest.raises(ValueError):
        umlh.class_stats(x, order, offsets, 4, means_out=torch.empty(4, 8))


# ------------------------------------------------------------------------------------------ end to end
class _Log:
    def __init__(self):
        self.rows = []

    def log(self, d):
        self.rows.append(d)


def _golden_run(g, tag, tmp, logger=None, capture=True, samples="golden", options=None, max_iters=None):
    """finetune.train() on the inputs of golden run ``tag`` under the golden's seed -> (out, model)."""
    import finetune as ft
    from engine.datasets.utils import FeatureLoader, FeatureTable, TextTensorDataset
    from engine.models.head import UML
    from engine.optimizer.optim import build_optimizer
    from engine.optimizer.scheduler import build_lr_scheduler
    from engine.tools.utils import set_random_seed
    d_img, d_txt, c, b, steps, eval_freq, lr, wd, alpha, shot, seed = g[f"{tag}::cfg"]
    d_img, d_txt, c, b, steps, eval_freq, shot, seed = map(int, (d_img, d_txt, c, b, steps, eval_freq, shot, seed))
    T = lambda k: torch.as_tensor(g[f"{tag}::{k}"])
    set_random_seed(seed)
    text_ds = TextTensorDataset(T("x_txt"), T("y_txt"), torch.zeros(len(g[f"{tag}::y_txt"]), dtype=torch.long))
    model = UML(d_img, d_txt, c, bias=False, learnable_temp=False)
    np.testing.assert_array_equal(model.head.weight.detach().numpy(), g[f"{tag}::w_head_init"])
    np.testing.assert_array_equal(model.img_proj.weight.detach().numpy(), g[f"{tag}::w_proj_init"])
    model.to(DEV)
    optimizer = build_optimizer(model.parameters(), "adamw", float(lr), float(wd))
    scheduler = build_lr_scheduler(optimizer, "cosine", 50, 1000, warmup_type="linear", warmup_lr=1e-5)
    il = FeatureLoader(FeatureTable(T("x_img"), T("y_img"), DEV), b, shuffle=True, kind="image")
    tl = FeatureLoader(FeatureTable(text_ds.input_tensor, text_ds.label_tensor, DEV), b, shuffle=True, kind="text")
    if str(g[f"{tag}::modality"]) == "image":
        tl = None
    vl = FeatureLoader(FeatureTable(T("x_val"), T("y_val"), DEV), b, shuffle=False)
    te = FeatureLoader(FeatureTable(T("x_test"), T("y_test"), DEV), b, shuffle=False)
    kw = {}
    if capture == "off":
        kw = dict(capture_features_during_training=False, features_pth=str(tmp))
    elif capture:
        kw = dict(capture_features_during_training=True, features_pth=str(tmp), capture_options=options,
                  capture_samples=(T("sample_x"), T("sample_y")) if samples == "golden" else samples)
    out = ft.train(model, il, tl, vl, te, optimizer, scheduler, device=DEV, max_iters=max_iters or steps, alpha=float(alpha),
                   eval_freq=eval_freq, patience=100, logger=logger, **kw)
    return out, model


def _knn_gaps(feats, k):
    """Per row the float64 gap between its k-th and (k+1)-th largest inner product with another row, relative to the largest."""
    f = np.asarray(feats, dtype=np.float64)
    s = f @ f.T
    np.fill_diagonal(s, -np.inf)
    top = -np.sort(-s, axis=1)
    return (top[:, k - 1] - top[:, k]) / np.abs(top[:, 0])


@pytest.mark.parametrize("tag", ["A", "B"])
def test_train_with_capture_matches_the_reference_run(tag, tmp_path):
    import umlh
    g = load_golden("feature_capture")
    lg = _Log()
    samples = "golden" if tag == "B" else None                # run A: take_capture_samples would take 16 shots; pass shot 5 below
    if tag == "A":
        import finetune as ft
        from engine.datasets.utils import FeatureLoader, FeatureTable
        table = FeatureTable(torch.as_tensor(g["A::x_img"]), torch.as_tensor(g["A::y_img"]), DEV)
        samples = ft.take_capture_samples(FeatureLoader(table, 16, kind="image"), shot=5)
        np.testing.assert_array_equal(samples[0].cpu().numpy(), g["A::sample_x"])
    out, model = _golden_run(g, tag, tmp_path, logger=lg, samples=samples)
    steps = [r for r in lg.rows if "train/image_loss" in r]
    n = int(g[f"{tag}::cfg"][4])
    assert len(steps) == n == out["train_scalars"].shape[0]
    ce = g[f"{tag}::train_ce"]
    sc = out["train_scalars"].numpy()
    if tag == "A":
        dl = np.abs(sc[:, umlh.S_LOSS_IMG] - ce).max()
    else:
        dl = max(np.abs(sc[:, umlh.S_LOSS_IMG] - ce[0::2]).max(), np.abs(sc[:, umlh.S_LOSS_TXT] - ce[1::2]).max())
    print(f"run {tag}: max |loss - reference| {dl:.2e}")
    assert dl <= 1e-4
    for k, r in enumerate(steps):
        got = (r["train/inclass_distance"], r["train/cka_score"], r["train/mknn_score"])
        want = (g[f"{tag}::inclass_distance"][k], g[f"{tag}::cka_score"][k], g[f"{tag}::mknn_score"][k])
        print(f"run {tag} step {k}: inclass {got[0]:.10g} (ref {want[0]:.10g}, rel {abs(got[0] - want[0]) / max(want[0], 1e-300):.2e}) "
              f"cka {got[1]:.9g} (ref {want[1]:.9g}) mknn {got[2]:.9g} (ref {want[2]:.9g})")
        np.testing.assert_array_equal(out["capture_scalars"][k].numpy(), np.asarray(got))
    for k, r in enumerate(steps):
        want = (g[f"{tag}::inclass_distance"][k], g[f"{tag}::cka_score"][k], g[f"{tag}::mknn_score"][k])
        assert abs(r["train/inclass_distance"] - want[0]) <= R.FP32_FORM_BOUND * want[0]
        if tag == "A":
            assert r["train/cka_score"] == 0 and r["train/mknn_score"] == 0
        else:
            assert abs(r["train/cka_score"] - want[1]) <= 1e-4
            rows = g["B::sample_x"].shape[0]
            assert round(r["train/mknn_score"] * rows * 10) == round(float(want[2]) * rows * 10)      # the same intersections
            assert abs(r["train/mknn_score"] - want[2]) <= 2.0 ** -22
    # the saved files: the reference's names, shapes and dtypes, contents within 1e-4
    names = [str(s) for s in g[f"{tag}::saved_files"]]
    assert sorted(f[:-4] for f in os.listdir(tmp_path) if f.endswith(".pth")) == sorted(names)
    for f in names:
        got, want = torch.load(os.path.join(tmp_path, f + ".pth")), g[f"{tag}::file::{f}"]
        assert isinstance(got, torch.Tensor) and got.device.type == "cpu" and tuple(got.shape) == want.shape, f
        assert str(got.dtype).replace("torch.", "") == str(want.dtype), (f, got.dtype, want.dtype)
        err = np.abs(got.numpy().astype(np.float64) - want).max()
        print(f"run {tag} {f}: shape {tuple(got.shape)} {got.dtype} max |diff| {err:.2e}")
        assert err <= 1e-4
    if tag == "B":
        # mutual k-NN can only be asserted exactly where every neighbour list is sharp in float64: the golden's are
        feats, text = g["B::file::all_iter_image_features"], g["B::file::all_iter_text_features"]
        gaps = np.concatenate([_knn_gaps(f, 10) for f in feats] + [_knn_gaps(text, 10)])
        print(f"run B: smallest relative gap between the 10th and 11th neighbour {gaps.min():.3e}")
        assert gaps.min() > 1e-4


def test_row_count_mismatch_gives_nan_scores_and_strict_raises(tmp_path, capsys):
    import feature_capture
    g = load_golden("feature_capture")
    # run B's text sample (12 rows) against run A's image sample (60 rows, 12 classes): CKA fits, mutual k-NN does not
    out, model = _golden_run(g, "B", tmp_path, logger=_Log(), samples=(torch.as_tensor(g["A::sample_x"]), torch.as_tensor(g["A::sample_y"])),
                             max_iters=2)
    printed = capsys.readouterr().out
    cap = out["capture_scalars"].numpy()
    print(cap)
    assert np.isnan(cap[:, 2]).all() and not np.isnan(cap[:, :2]).any() and (cap[:, 0] > 0.1).all()
    assert printed.count("disabled, logged as NaN") == 1 and "train/mknn_score" in printed
    with pytest.raises(ValueError, match="mknn_score"):
        _golden_run(g, "B", tmp_path, samples=(torch.as_tensor(g["A::sample_x"]), torch.as_tensor(g["A::sample_y"])), max_iters=1,
                    options={"strict": True})
    # 12 image rows against 12 text rows but 13 classes: CKA is the one that is off; 10 rows: mutual k-NN needs more than 10
    fc = feature_capture.FeatureCapture(model, torch.as_tensor(g["B::sample_x"]), torch.as_tensor(g["B::sample_y"]),
                                        torch.as_tensor(g["B::x_txt"]), 13)
    assert not fc.with_cka and fc.with_mknn
    fc = feature_capture.FeatureCapture(model, torch.as_tensor(g["B::sample_x"][:10]), torch.as_tensor(g["B::sample_y"][:10]),
                                        torch.as_tensor(g["B::x_txt"][:10]), 12)
    assert not fc.with_mknn
    vals = [float(v) for v in fc.step()]
    assert np.isnan(vals[0]) and np.isnan(vals[2])             # two of the 12 classes have no row: the reference's np.mean is NaN too


def test_flag_off_is_bit_equal_and_keep_features_false_writes_no_stack(tmp_path):
    g = load_golden("feature_capture")
    base, m0 = _golden_run(g, "B", tmp_path / "none", capture=False)                  # without the argument
    off, m1 = _golden_run(g, "B", tmp_path / "off", capture="off")                   # with it, False
    assert not os.path.exists(tmp_path / "none") and not os.path.exists(tmp_path / "off")
    assert torch.equal(base["train_scalars"], off["train_scalars"])
    assert all(torch.equal(base["model"][k], off["model"][k]) for k in base["model"])
    assert torch.equal(m0.head.weight, m1.head.weight) and torch.equal(m0.img_proj.weight, m1.img_proj.weight)
    assert "capture_scalars" not in off
    # keep_features=False: the four other files are written, the stack is not
    on, m2 = _golden_run(g, "B", tmp_path / "on", options={"keep_features": False})
    files = sorted(os.listdir(tmp_path / "on"))
    print(files)
    assert files == ["all_iter_image_labels.pth", "all_iter_image_raw_features.pth", "all_iter_text_features.pth", "all_iter_text_labels.pth"]
    assert on["capture_scalars"].shape == (6, 3) and not torch.isnan(on["capture_scalars"]).any()
