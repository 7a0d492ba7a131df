"""GPU: the linear probes on the HIP kernels (umlh.probe, multibench.train.evaluate) against the float64 restatement
(tests/_probe_ref.py) first and the values the reference recorded with sklearn second (tests/golden/probe_*.npz).

Every measured figure is printed before it is asserted (run with -s to see them; scripts/bench_probe.py writes the per-case
`delta` to profiles/probe_accuracy.txt)."""
import numpy as np
import pytest
import torch

import _probe_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROBE_CASES = ["mosi_a", "mosi_b", "mosei_a", "mosei_b", "humor_c"]
KIND = {R.LBFGS: "lbfgs", R.LIBLINEAR: "liblinear"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def coef(pr):
    return torch.cat([pr.coef_.reshape(-1), pr.intercept_]).cpu().numpy()


# ---- pooling ----
@pytest.mark.parametrize("B,T,Z", [(7, 13, 45), (32, 50, 40), (3, 1, 300), (5, 9, 64), (1, 17, 1)])
def test_masked_mean(B, T, Z):
    import umlh
    rng = np.random.default_rng(B * 1000 + T)
    z = (rng.standard_normal((B, T, Z)) * rng.uniform(0.1, 10, (B, 1, Z))).astype(np.float32)
    lens = rng.integers(1, T + 1, B)
    lens[0] = T
    lens[-1] = 1
    for L in (lens, None):
        got = umlh.masked_mean(dev(z), None if L is None else dev(L)).cpu().numpy()
        err, bound = np.abs(got - R.masked_mean(z, L)), R.masked_mean_bound(z, L)
        print(f"masked_mean B={B} T={T} Z={Z} lengths={'yes' if L is not None else 'None'}: max err/bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()
    # strided input (a [T, B, Z] block pooled in place, then a padded row stride) and a column block of a wider output
    ztb = dev(np.ascontiguousarray(z.transpose(1, 0, 2)))
    got = umlh.masked_mean(ztb.permute(1, 0, 2), dev(lens)).cpu().numpy()
    assert (np.abs(got - R.masked_mean(z, lens)) <= R.masked_mean_bound(z, lens)).all()
    wide = torch.full((B, T, Z + 5), 7.0, device=DEV)
    wide[:, :, :Z] = dev(z)
    out = torch.full((B, 2 * Z + 3), -1.0, device=DEV)
    ret = umlh.masked_mean(wide[:, :, :Z], dev(lens), out=out[:, Z:2 * Z])
    assert ret.data_ptr() == out[:, Z:2 * Z].data_ptr()
    o = out.cpu().numpy()
    assert (np.abs(o[:, Z:2 * Z] - R.masked_mean(z, lens)) <= R.masked_mean_bound(z, lens)).all()
    assert (o[:, :Z] == -1).all() and (o[:, 2 * Z:] == -1).all()
    # len = 0 -> NaN like the reference's 0/0; len > T counts as T; other rows untouched by either
    odd = lens.copy()
    odd[0] = T + 9
    if B > 1:
        odd[1] = 0
    got = umlh.masked_mean(dev(z), dev(odd)).cpu().numpy()
    want = R.masked_mean(z, odd)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and (B == 1 or np.isnan(got[1]).all())
    ok = ~np.isnan(want)
    assert (np.abs(got - want)[ok] <= R.masked_mean_bound(z, np.clip(odd, 1, T))[ok]).all()
    # other float dtypes are upcast, CPU tensors copied
    assert torch.equal(umlh.masked_mean(torch.from_numpy(z).double(), torch.from_numpy(lens)), umlh.masked_mean(dev(z), dev(lens)))


# ---- StandardScaler statistics ----
def test_column_stats():
    from umlh import probe
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((1284, 70)) * rng.uniform(1e-3, 50, 70) + rng.standard_normal(70) * 1000).astype(np.float32)
    x[:, 3] = 2.5
    x[:, 9] = -1000.25
    x[:, 11] = 0.0
    for xs in (dev(x), dev(np.concatenate([x, x], axis=1))[:, :70]):          # contiguous, then a row stride of 2 d
        st = probe.column_stats(xs).cpu().numpy()
        mean, sd = R.column_stats(x)
        rel_m = np.abs(st[0] - mean) / np.maximum(np.abs(mean), sd)
        rel_s = np.abs(st[1] - sd) / sd
        print(f"column_stats: max rel err mean {rel_m.max():.2e} std {rel_s.max():.2e}")
        assert rel_m.max() <= 1e-12 and rel_s.max() <= 1e-12
        assert st[1][3] == 1.0 and st[1][9] == 1.0 and st[1][11] == 1.0          # constant columns scale by 1
        assert st[0][3] == 2.5 and st[0][9] == -1000.25


@pytest.mark.parametrize("n,d,ldx", [(5, 65, 70), (257, 1, 1)])
def test_column_stats_edges(n, d, ldx):
    """test_column_stats's bound where the column-sum body has little to hold on to: fewer rows than row lanes times chunks
    with a second, one-column block of columns behind NaN padding; one column over more rows than chunks."""
    from umlh import probe
    rng = np.random.default_rng(100 * n + d)
    x = (rng.standard_normal((n, d)) * rng.uniform(1e-3, 50, d) + rng.standard_normal(d) * 1000).astype(np.float32)
    wide = torch.full((n, ldx), float("nan"), device=DEV)
    wide[:, :d] = dev(x)
    st = probe.column_stats(wide[:, :d]).cpu().numpy()
    mean, sd = R.column_stats(x)
    rel_m = np.abs(st[0] - mean) / np.maximum(np.abs(mean), sd)
    rel_s = np.abs(st[1] - sd) / sd
    print(f"column_stats[{n},{d},{ldx}]: max rel err mean {rel_m.max():.2e} std {rel_s.max():.2e}")
    assert rel_m.max() <= 1e-12 and rel_s.max() <= 1e-12


# ---- fit / predict / score on the recorded cases ----
@pytest.mark.parametrize("tag", PROBE_CASES)
def test_fit_reaches_the_optimum_closer_than_sklearn_did(tag):
    import umlh
    g = load_golden("probe_" + tag)
    kind = int(g["kind"])
    stats = (g["mean"], g["scale"]) if kind == R.LIBLINEAR else None
    w_star, delta_ref = g["w_star"], float(g["delta_ref"])
    pr = umlh.LogisticProbe(KIND[kind], keep_objectives=True).fit(dev(g["x_train"]), dev(g["y_train"]))
    w, rec = coef(pr), pr.record()
    obj = pr.objectives_.cpu().numpy()
    delta = np.abs(w - w_star).max()
    print(f"{tag}: record {rec} delta = max|w_gpu - w*| = {delta:.3e} (sklearn's own: {delta_ref:.3e}); objective steps "
          + " ".join(f"{v:.1e}" for v in -np.diff(obj)))
    assert rec["converged"] in (1, 2) and rec["n_iter"] == len(obj) - 1 and pr.n_iter_ == rec["n_iter"]
    assert np.all(np.diff(obj) <= 0) and np.isfinite(obj).all()
    assert obj[-1] == rec["objective"]
    xa = R._aug(R.standardise(g["x_train"], stats))
    assert abs(obj[-1] - R.objective(w, xa, g["y_train"].astype(np.float64), kind)) <= 1e-6 * obj[-1]
    assert delta <= delta_ref
    if stats is not None:
        st = pr.stats_.cpu().numpy()
        np.testing.assert_allclose(st[0], stats[0], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(st[1], stats[1], rtol=1e-12)
    for split in ("val", "test"):
        xh, yh = g["x_" + split], g["y_" + split]
        n, flips = len(yh), int(g["ref_flips_" + split])
        dec = pr.decision_function(dev(xh)).cpu().numpy()
        pred = pr.predict(dev(xh)).cpu().numpy()
        assert dec.dtype == np.float32 and pred.dtype == np.int64 and np.array_equal(pred, (dec > 0).astype(np.int64))
        d64 = R.decision(w_star, xh, stats)
        ok = R.decidable(w_star, xh, stats, w)
        und = int((~ok).sum())
        score = pr.score(dev(xh), dev(yh))
        s64, sref = R.score(w_star, xh, yh, stats), float(g["score_ref_" + split])
        print(f"  {split}: decidable {ok.mean():.4f} max|dec - dec64| {np.abs(dec - d64).max():.2e} score {score:.4f} "
              f"score64 {s64:.4f} sklearn {sref:.4f} (ref_flips {flips})")
        assert np.array_equal(pred[ok], (d64 > 0).astype(np.int64)[ok])
        assert ok.mean() >= 0.99
        assert isinstance(score, float) and score == float((pred == yh).sum()) / n
        assert abs(score - s64) <= und / n + 1e-12
        assert abs(score - sref) <= (flips + und) / n + 1e-12
        assert int(pr.correct(dev(xh), dev(yh))) == int((pred == yh).sum())


def tile_edge_problem(d, n=97, nh=200):
    """n training and nh held-out rows of d features off the origin, labels from a noisy linear rule; seeded by d.  With this
    seed base the float64 Newton iteration of _probe_ref.fit reaches max|gradient| <= 4e-12 in at most 9 steps for d = 31, 32,
    33, both kinds, with and without statistics: no fit ends at an iteration cap."""
    rng = np.random.default_rng(4400 + d)
    x = (rng.standard_normal((n + nh, d)) * rng.uniform(0.3, 2.0, d) + 0.5 * rng.standard_normal(d)).astype(np.float32)
    wt = rng.standard_normal(d) / np.sqrt(d)
    y = ((x - x.mean(0)) @ wt + 0.7 * rng.standard_normal(n + nh) > 0).astype(np.int64)
    return x[:n], y[:n], x[n:], y[n:]


@pytest.mark.parametrize("kind", [R.LBFGS, R.LIBLINEAR])
@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("d", [31, 32, 33])
def test_fit_and_score_at_tile_edges(monkeypatch, d, with_stats, kind):
    """The assertions of test_fit_reaches_the_optimum_closer_than_sklearn_did that need no recorded sklearn run, at N = 97 and
    D = d + 1 = 32, 33, 34 columns (one 32-column tile; the intercept alone in a second tile; two ragged tiles), against the
    float64 Newton optimum.  The statistics are switched independently of the solver kind: fit() standardises exactly when
    its kind is named 'liblinear', so the name is mapped to the solver under test."""
    import umlh
    from umlh import probe
    x, y, xh, yh = tile_edge_problem(d)
    stats = R.column_stats(x) if with_stats else None
    w_star, it, mg = R.fit(x, y, kind, stats=stats)
    assert mg <= 1e-10 and it < 200
    name = "liblinear" if with_stats else "lbfgs"
    monkeypatch.setitem(probe.KINDS, name, kind)
    pr = umlh.LogisticProbe(name, keep_objectives=True).fit(dev(x), dev(y))
    w, rec = coef(pr), pr.record()
    obj = pr.objectives_.cpu().numpy()
    print(f"d={d} stats={with_stats} {KIND[kind]}: record {rec} (float64 Newton: {it} iterations) "
          f"delta = max|w_gpu - w*| = {np.abs(w - w_star).max():.3e}")
    assert rec["converged"] in (1, 2) and rec["n_iter"] == len(obj) - 1 and pr.n_iter_ == rec["n_iter"]
    assert np.all(np.diff(obj) <= 0) and np.isfinite(obj).all()
    assert obj[-1] == rec["objective"]
    xa = R._aug(R.standardise(x, stats))
    assert abs(obj[-1] - R.objective(w, xa, y.astype(np.float64), kind)) <= 1e-6 * obj[-1]
    if with_stats:
        st = pr.stats_.cpu().numpy()
        np.testing.assert_allclose(st[0], stats[0], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(st[1], stats[1], rtol=1e-12)
    n = len(yh)
    dec = pr.decision_function(dev(xh)).cpu().numpy()
    pred = pr.predict(dev(xh)).cpu().numpy()
    d64 = R.decision(w_star, xh, stats)
    ok = R.decidable(w_star, xh, stats, w)
    score, s64 = pr.score(dev(xh), dev(yh)), R.score(w_star, xh, yh, stats)
    print(f"  held out: decidable {ok.mean():.4f} max|dec - dec64| {np.abs(dec - d64).max():.2e} score {score:.4f} score64 {s64:.4f}")
    assert np.array_equal(pred[ok], (d64 > 0).astype(np.int64)[ok])
    assert ok.mean() >= 0.99
    assert score == float((pred == yh).sum()) / n
    assert abs(score - s64) <= int((~ok).sum()) / n + 1e-12
    assert int(pr.correct(dev(xh), dev(yh))) == int((pred == yh).sum())


def test_fit_input_rules_and_errors():
    import umlh
    g = load_golden("probe_humor_c")
    x, y = g["x_train"], g["y_train"]
    base = umlh.LogisticProbe("lbfgs").fit(dev(x), dev(y))
    w = coef(base)
    padded = dev(np.concatenate([x, x + 1.0], axis=1))[:, :x.shape[1]]       # row stride 2 d, used in place
    assert np.array_equal(coef(umlh.LogisticProbe("lbfgs").fit(padded, dev(y))), w)
    assert np.array_equal(coef(umlh.LogisticProbe("lbfgs").fit(torch.from_numpy(x).double(), torch.from_numpy(y).float())), w)
    with pytest.raises(ValueError, match="only one class"):
        umlh.LogisticProbe("lbfgs").fit(dev(x), dev(np.ones_like(y)))
    with pytest.raises(ValueError):
        umlh.LogisticProbe("lbfgs").fit(dev(x), dev(y * 2))
    with pytest.raises(ValueError):
        umlh.LogisticProbe("lbfgs").fit(dev(x), dev(y[:-1]))
    with pytest.raises(ValueError):
        base.score(dev(x[:, :-1]), dev(y))
    # a budget too small to converge says so, and a gradient tolerance it can meet reports code 1
    short = umlh.LogisticProbe("lbfgs", max_iter=2).fit(dev(x), dev(y))
    assert short.converged_ == 0 and short.n_iter_ == 2
    loose = umlh.LogisticProbe("lbfgs", gtol=1.0).fit(dev(x), dev(y))
    assert loose.converged_ == 1 and loose.max_grad_ <= 1.0 and loose.n_iter_ < base.n_iter_


def test_fits_are_reproducible_and_independent():
    import umlh
    ga, gb = load_golden("probe_mosi_b"), load_golden("probe_humor_c")
    xa, ya, xb, yb = dev(ga["x_train"]), dev(ga["y_train"]), dev(gb["x_train"]), dev(gb["y_train"])

    def one(kind, x, y):
        pr = umlh.LogisticProbe(kind, keep_objectives=True).fit(x, y, check_classes=False)
        return pr

    def bits(pr):
        return coef(pr).tobytes() + pr.objectives_.cpu().numpy().tobytes() + bytes(str(pr.record()), "ascii")

    alone_a, alone_b = bits(one("liblinear", xa, ya)), bits(one("lbfgs", xb, yb))
    torch.cuda.synchronize()
    assert bits(one("liblinear", xa, ya)) == alone_a                          # twice the same data: bitwise equal
    pa, pb = one("liblinear", xa, ya), one("lbfgs", xb, yb)                   # back to back on one stream, nothing read between
    assert pa._keep[2].data_ptr() != pb._keep[2].data_ptr()                   # each with its own scratch
    assert bits(pa) == alone_a and bits(pb) == alone_b
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ps = one("lbfgs", xb, yb)
    side.synchronize()
    assert bits(ps) == alone_b


# ---- scale: no fixture, restatement only ----
@pytest.mark.parametrize("n,d,seed", [(16384, 300, 5), (4096, 600, 4)])
def test_fit_at_scale(n, d, seed):
    import umlh
    from umlh._lib import load_library
    rng = np.random.default_rng(seed)
    nh = 1000
    x = (rng.standard_normal((n + nh, d)) * rng.uniform(0.3, 2.0, d) + 0.2 * rng.standard_normal(d)).astype(np.float32)
    wt = rng.standard_normal(d) / np.sqrt(d)
    y = ((x - x.mean(0)) @ wt + 0.5 * rng.standard_normal(n + nh) > 0).astype(np.int64)
    w_star, it, mg = R.fit(x[:n], y[:n], R.LBFGS)
    assert mg <= 1e-10
    xt, yt, xh = dev(x[:n]), dev(y[:n]).to(torch.int32), dev(x[n:])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pr = umlh.LogisticProbe("lbfgs").fit(xt, yt, check_classes=False)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    budget = load_library().umlh_probe_scratch_bytes(n, d, pr.max_iter)
    w, rec = coef(pr), pr.record()
    delta = np.abs(w - w_star).max()
    ok = R.decidable(w_star, x[n:], None, w)
    pred = pr.predict(xh).cpu().numpy()
    print(f"N={n} d={d}: record {rec} (float64 Newton: {it} iterations) delta {delta:.3e} decidable {ok.mean():.4f} "
          f"extra memory {extra / 2**20:.1f} MiB, scratch {budget / 2**20:.1f} MiB")
    assert rec["converged"] in (1, 2)
    assert np.array_equal(pred[ok], (R.decision(w_star, x[n:]) > 0).astype(np.int64)[ok])
    assert ok.mean() >= 0.99
    assert extra <= budget + (4 << 20)
    assert abs(pr.score(xh, dev(y[n:])) - R.score(w_star, x[n:], y[n:])) <= (~ok).sum() / nh + 1e-12


# ---- end to end: multibench.train.evaluate / evaluate_raw_data / train ----
def _model(name):
    from multibench.models import Linear, Transformer, UML
    g = load_golden(name)
    z, dx, dy, B, T, pe, pl = (int(v) for v in g["cfg"])
    m = UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=5, conv1d=True, out_last=False,
                                                       pos_embd=bool(pe), pos_learnable=bool(pl), max_len=128),
            [Linear(z, dx), Linear(z, dy)], modality="xy")
    m.load_state_dict({k[4:]: torch.as_tensor(g[k]) for k in g.files if k.startswith("sd::")})
    return m.to(DEV)


def _config(g, freq=2):
    bs, cfg = int(g["batch_size"]), {"freq": freq}
    for t in ("train", "val", "test"):
        x, y, lx, ly, lab = (torch.from_numpy(g[f"{k}_{t}"]) for k in ("x", "y", "lx", "ly", "labels"))
        cfg[t] = [([x[s:s + bs], None, y[s:s + bs]], [lx[s:s + bs], None, ly[s:s + bs]], torch.arange(s, min(s + bs, len(x))),
                   lab[s:s + bs].reshape(-1, 1)) for s in range(0, len(x), bs)]
    return cfg


def _slack(w_star, w_ref, w_gpu, xh, stats, emb_tol):
    """Held-out samples the comparison cannot decide: the decidability margin of the module docstring, samples whose
    float64 decision value an `emb_tol` difference in every feature could flip, and sklearn's own flips."""
    d64 = R.decision(w_star, xh, stats)
    und = ~R.decidable(w_star, xh, stats, w_gpu)
    if emb_tol:
        scale = 1.0 if stats is None else stats[1]
        und |= np.abs(d64) <= emb_tol * np.abs(w_star[:-1] / scale).sum()
    flips = int(((R.decision(w_ref, xh, stats) > 0) != (d64 > 0)).sum())
    return int(und.sum()), flips


@pytest.mark.parametrize("tag", ["mosi", "humor"])
def test_evaluate_end_to_end(tag):
    from multibench.train import evaluate, evaluate_raw_data
    g = load_golden("probe_e2e_" + tag)
    ds = str(g["ds_name"])
    kind = R.LIBLINEAR if ds == "mosi" else R.LBFGS
    cfg = _config(g)
    model = _model(str(g["model"])).train()
    raw, _, raw_clfs = evaluate_raw_data(cfg, ds, return_probes=True)
    assert evaluate_raw_data(cfg, ds) == raw
    res, emb, clfs = evaluate(model, cfg, ds, device=DEV, return_embeddings=True)
    assert not model.training                                                   # evaluate leaves the model in eval mode, as the reference
    assert set(raw) == set(g["keys_raw"]) and set(res) == set(g["keys_eval"])
    assert evaluate(model, cfg, ds, device=DEV) == pytest.approx(res, nan_ok=True, abs=0)   # and is deterministic
    for k in res:
        ref = float(g["res::" + k])
        assert np.isnan(res[k]) == np.isnan(ref), k
        if "loss" in k:
            print(f"{tag} {k}: {res[k]:.6f} reference {ref:.6f}")
            assert abs(res[k] - ref) <= 1e-4
    # pooled embeddings against the reference's
    z = 20
    for t in ("train", "val", "test"):
        e = emb[t].cpu().numpy()
        dx, dy = np.abs(e[:, :z] - g["emb_x_" + t]).max(), np.abs(e[:, z:] - g["emb_y_" + t]).max()
        print(f"{tag} pooled {t}: max|emb - reference| x {dx:.2e} y {dy:.2e}")
        assert dx <= 2e-4 and dy <= 2e-4
    # probes: the float64 optimum on the reference's embeddings (raw: on the raw means), then the recorded sklearn score
    sets = {"": {t: (g["emb_x_" + t], g["emb_y_" + t]) for t in ("train", "val", "test")},
            "_raw": {t: (R.masked_mean(g["x_" + t]).astype(np.float32), R.masked_mean(g["y_" + t]).astype(np.float32))
                     for t in ("train", "val", "test")}}
    for suffix, feats in sets.items():
        got = raw if suffix else res
        for i, (name, pick) in enumerate((("x", lambda a: a[0]), ("y", lambda a: a[1]), ("xy", lambda a: np.concatenate(a, axis=1)))):
            xt = pick(feats["train"])
            stats = R.column_stats(xt) if kind == R.LIBLINEAR else None
            w_star, _, mg = R.fit(xt, g["y01_train"], kind, stats=stats)
            assert mg <= 1e-10
            w_ref = g[f"wref{suffix}_{name}"]
            w_gpu = coef(raw_clfs[i] if suffix else clfs[3 + i])
            for t in ("val", "test"):
                xh, yh = pick(feats[t]), g["y01_" + t]
                # embedding probes: the 2e-4 tests/test_multibench_gpu.py holds zx to; raw means: twice the fp32 chain bound
                # T 2^-24 sum|x| / T of a unit-variance feature over T = 9 steps, 1e-6
                und, flips = _slack(w_star, w_ref, w_gpu, xh, stats, 1e-6 if suffix else 2e-4)
                key = f"{t}/score_{name}{suffix}"
                s64, sref = R.score(w_star, xh, yh, stats), float(g["res::" + key])
                print(f"{tag} {key}: {got[key]:.4f} float64 {s64:.4f} reference {sref:.4f} (undecidable {und}, ref_flips {flips}, N {len(yh)})")
                assert abs(got[key] - s64) <= und / len(yh) + 1e-12
                assert abs(got[key] - sref) <= (flips + und) / len(yh) + 1e-12
    # modality separation: each split's probe is scored on its own training rows; the mean of three
    tol, want = 0.0, []
    for i, t in enumerate(("train", "val", "test")):
        both = np.concatenate([g["emb_x_" + t], g["emb_y_" + t]])
        which = np.concatenate([np.zeros(len(both) // 2, np.int64), np.ones(len(both) // 2, np.int64)])
        stats = R.column_stats(both) if kind == R.LIBLINEAR else None
        w_star, _, mg = R.fit(both, which, kind, stats=stats)
        und, flips = _slack(w_star, g["wref_sep_" + t], coef(clfs[i]), both, stats, 2e-4)
        want.append(R.score(w_star, both, which, stats))
        tol += (und + flips) / len(both) / 3
    ref = float(g["res::val/modality_separate"])
    print(f"{tag} val/modality_separate: {res['val/modality_separate']:.4f} float64 {np.mean(want):.4f} reference {ref:.4f} (slack {tol:.4f})")
    assert abs(res["val/modality_separate"] - np.mean(want)) <= tol + 1e-12
    assert abs(res["val/modality_separate"] - ref) <= tol + 1e-12


def test_train_evaluates_at_the_reference_batch_indices():
    from multibench.train import train
    g = load_golden("probe_e2e_humor")
    cfg = _config(g, freq=3)
    x, y, lx, ly = (torch.from_numpy(g[f"{k}_train"]) for k in ("x", "y", "lx", "ly"))
    loader = [([x[s:s + 16], None, y[s:s + 16]], [lx[s:s + 16], None, ly[s:s + 16]]) for s in range(0, 80, 16)]      # 5 batches
    torch.manual_seed(0)
    model = _model(str(g["model"]))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    plain = train(model, "xy", loader, loader, opt, num_epoch=1, step_k=-1, ds_name="humor", device=DEV)
    assert set(plain) == {"loss_x", "loss_y", "loss"} and len(plain["loss"]) == 5        # eval_config = {}: as before
    out = train(model, "xy", loader, loader, opt, num_epoch=2, step_k=-1, ds_name="humor", eval_config=cfg, device=DEV)
    assert model.training
    assert set(out) == {"loss_x", "loss_y", "loss", "raw", "eval"} and len(out["loss"]) == 10
    assert [(e, i) for e, i, _ in out["eval"]] == [(0, 0), (0, 3), (1, 0), (1, 3), (1, None)]
    assert set(out["raw"]) == set(g["keys_raw"])
    logged = {k for k in g["keys_eval"] if "private" not in k and "complete" not in k} | set(g["keys_raw"])
    for _, _, r in out["eval"]:
        assert set(r) == logged and all(np.isfinite(v) for v in r.values())
        assert all(0.0 <= r[k] <= 1.0 for k in r if "score" in k or "separate" in k)
    assert out["eval"][0][2]["val/loss_y"] != out["eval"][-1][2]["val/loss_y"]           # the model moved between evaluations
