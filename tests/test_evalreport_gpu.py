"""GPU: the class-wise validation report (umlh_eval_topk / umlh_eval_classwise, umlh.topk_classes / umlh.class_report,
model.predict_topk, finetune.validate_classwise, train(classwise=...)) against the float64 restatement tests/_evalreport_ref.py.

Random cases: the lists equal the restatement on every SHARP row (see _evalreport_ref.py), at most CAP of a case's rows may be
non-sharp, and the returned logits are the float64 values rounded once.  Integer-valued cases make every logit exact, so ties are
certain and the lists must equal the restatement on every row.  Shapes are the smallest at which the kernels can go wrong: the
32-row strip edges, the 256-column tile edges, C around the candidate margin, both load paths."""
import ctypes as C

import numpy as np
import pytest
import torch

import _evalreport_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_CLS, GUARD_LOGIT = -7777, -12345.5


def _place(a, layout):
    """fp32 device matrix of ``a``: dense, or with a row stride of d + 3 floats starting one float into its buffer (no 16-byte
    alignment of any row: the 4-byte load path)."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    if layout == "dense":
        return t
    rows, d = t.shape
    buf = torch.full((rows * (d + 3) + 1,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[1:].view(rows, d + 3)[:, :d]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.stride(0) == d + 3
    return view


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(a).to(DEV, dtype).contiguous()


def _raw_topk(x, w, b, scale, k, splits=0, stream=None, want_logit=True):
    """umlh_eval_topk through ctypes on device matrices used in place.  The outputs sit in buffers one row longer than needed,
    filled with guard values: -> (cls [n, k], logit [n, k], the two guard rows)."""
    import umlh
    from umlh import _glue as glue
    from umlh._lib import check, load_library
    lib = load_library()
    (n, d), nc = x.shape, w.shape[0]
    nbytes = lib.umlh_eval_topk_scratch_bytes(n, nc, d, k, splits)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    cls = torch.full((n + 1, k), GUARD_CLS, dtype=torch.int32, device=DEV)
    logit = torch.full((n + 1, k), GUARD_LOGIT, dtype=torch.float32, device=DEV)
    sc = None if scale is None else torch.tensor(float(scale), dtype=torch.float32, device=DEV)
    st = glue.stream(torch.device(DEV)) if stream is None else C.c_void_p(stream.cuda_stream)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())                          # the buffers above were filled there
    check(lib.umlh_eval_topk(x.data_ptr(), n, x.stride(0), w.data_ptr(), nc, w.stride(0), d, glue.ptr(b), glue.ptr(sc), k, splits,
                             cls.data_ptr(), logit.data_ptr() if want_logit else None, scratch.data_ptr(), nbytes, st), "umlh_eval_topk")
    (stream or torch.cuda.current_stream()).synchronize()
    return cls[:n].cpu().numpy(), logit[:n].cpu().numpy(), (cls[n].cpu().numpy(), logit[n].cpu().numpy())


def _logit_tolerance(z64, x, w, b, scale, d):
    """One rounding of the float64 value to fp32, plus the summation-order freedom of two float64 evaluations."""
    order = 2 * (d + 2) * 2.0 ** -53 * R.magnitude(x, w, b)[:, None] * abs(scale or 1.0)
    return 2.0 ** -24 * np.abs(z64) + order + 2.0 ** -149


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_topk_grid(case):
    import umlh
    x, w, b = R.case_data(case)
    k, scale = case["k"], case["scale"]
    want, z64 = R.topk(x, w, b, scale, k)
    sharp = R.sharp(x, w, b, k, scale)
    xd, wd, bd = _place(x, case["layout"]), _place(w, case["layout"]), _dev(b)
    got, logit, (g_cls, g_logit) = _raw_topk(xd, wd, bd, scale, k)
    blunt = int((~sharp).sum())
    wrong = int((got != want).any(1).sum())
    err = np.abs(logit.astype(np.float64) - z64)
    tol = _logit_tolerance(z64, x, w, b, scale, case["d"])
    same = got == want
    print(f"case {case['name']} n={case['n']} C={case['C']} d={case['d']} k={k} bias={case['bias']} scale={scale} {case['layout']}: "
          f"rows that differ {wrong} (non-sharp {blunt}), max logit error / tolerance {float((err / tol)[same].max()):.3f}")
    assert blunt <= R.CAP * case["n"]
    assert np.array_equal(got[sharp], want[sharp])
    assert ((got >= 0) & (got < case["C"])).all()                                # all of the output written, all in range
    assert (err[same] <= tol[same]).all()
    assert np.isfinite(logit).all()
    assert (g_cls == GUARD_CLS).all() and (g_logit == GUARD_LOGIT).all()         # nothing written behind the output
    # the Python surface is the same call
    sc = None if scale is None else torch.tensor(scale, dtype=torch.float32, device=DEV)
    pc, pl = umlh.topk_classes(xd, wd, bd, sc, k=k)
    assert pc.dtype == torch.int32 and pl.dtype == torch.float32 and tuple(pc.shape) == tuple(pl.shape) == (case["n"], k)
    assert np.array_equal(pc.cpu().numpy(), got) and np.array_equal(pl.cpu().numpy(), logit)
    # without the logits nothing else changes
    got2, logit2, _ = _raw_topk(xd, wd, bd, scale, k, want_logit=False)
    assert np.array_equal(got2, got) and (logit2 == GUARD_LOGIT).all()


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("name", sorted(R.integer_cases()))
def test_integer_valued_inputs_tie_exactly(name, layout):
    x, w, b, scale, k = R.integer_cases()[name]
    want, z64 = R.topk(x, w, b, scale, k)
    assert (np.diff(z64, axis=1) == 0).any()                                     # ties inside the lists, for certain
    got, logit, _ = _raw_topk(_place(x, layout), _place(w, layout), _dev(b), scale, k)
    assert np.array_equal(got, want)                                             # every row, no sharpness needed
    assert np.array_equal(logit, z64.astype(np.float32))
    if name == "all_equal_row":
        assert np.array_equal(got[3], np.arange(k)) and np.array_equal(got[40], np.arange(k))
    # the wrong statements differ from what the device returned
    assert not np.array_equal(got, R.topk(x, w, b, scale, k, "tie_larger_index")[0])
    if b is not None:
        assert not np.array_equal(got, R.topk(x, w, b, scale, k, "bias_dropped")[0])
    if scale is not None and scale < 0:
        assert not np.array_equal(got, R.topk(x, w, b, scale, k, "scale_sign_ignored")[0])


def test_zero_scale_ties_every_class():
    x, w, b, _, k = R.integer_cases()["duplicates"]
    got, logit, _ = _raw_topk(_dev(x), _dev(w), _dev(b), 0.0, k)
    assert np.array_equal(got, np.broadcast_to(np.arange(k), got.shape)) and (logit == 0).all()


def test_bit_equal_across_splits_calls_and_streams():
    rng = np.random.default_rng(21)
    n, nc, d, k = 70, 1300, 24, 5                                                # 6 column tiles, 3 strips
    ntiles = (nc + 255) // 256
    x, w = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nc, d)).astype(np.float32)
    w[700] = w[30]                                                               # a tie across two chunks
    b = rng.standard_normal(nc).astype(np.float32)
    xd, wd, bd = _dev(x), _dev(w), _dev(b)
    base = _raw_topk(xd, wd, bd, -2.5, k, splits=0)
    assert np.array_equal(base[0][R.sharp(x, w, b, k, -2.5)], R.topk(x, w, b, -2.5, k)[0][R.sharp(x, w, b, k, -2.5)])
    for splits in (1, 2, ntiles, ntiles + 5, 0):                                 # the last: a second call with the same arguments
        got = _raw_topk(xd, wd, bd, -2.5, k, splits=splits)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), splits
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    got = _raw_topk(xd, wd, bd, -2.5, k, splits=2, stream=side)
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])


def test_nan_row_gets_no_class_and_leaves_the_others_alone():
    rng = np.random.default_rng(22)
    n, nc, d, k = 40, 300, 9, 5
    x, w = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nc, d)).astype(np.float32)
    clean = _raw_topk(_dev(x), _dev(w), None, 100.0, k)
    x[7, 3] = np.nan
    x[33] = np.nan
    got, logit, (g_cls, g_logit) = _raw_topk(_dev(x), _dev(w), None, 100.0, k)
    for r in (7, 33):
        assert (got[r] == -1).all() and np.isnan(logit[r]).all()
    keep = np.setdiff1d(np.arange(n), [7, 33])
    assert np.array_equal(got[keep], clean[0][keep]) and np.array_equal(logit[keep], clean[1][keep])
    assert ((got[keep] >= 0) & (got[keep] < nc)).all()
    assert (g_cls == GUARD_CLS).all() and (g_logit == GUARD_LOGIT).all()
    # a NaN weight row is a class that is never listed; with k = C one slot stays open
    w6 = w[:6].copy()
    w6[2] = np.nan
    got, logit, _ = _raw_topk(_dev(x[:3]), _dev(w6), None, None, 6)
    want, _ = R.topk(x[:3], w6, None, None, 6)
    assert np.array_equal(got, want) and (got[:, 5] == -1).all() and np.isnan(logit[:, 5]).all()


# ---- class_report ----
def _lists(n, k, nc, seed, no_pred=()):
    rng = np.random.default_rng(seed)
    cls = np.stack([rng.permutation(nc)[:k] if nc >= k else rng.integers(0, nc, k) for _ in range(n)]).astype(np.int32)
    for r in no_pred:
        cls[r] = -1
    return cls


def _report(cls, y, nc, confusion=False, out=None):
    import umlh
    return umlh.class_report(torch.from_numpy(cls).to(DEV), torch.from_numpy(y).to(DEV), nc, confusion=confusion, out=out)


def _check_report(got, want):
    assert set(got) == set(want)
    for key in want:
        assert got[key].dtype == torch.int64 and np.array_equal(got[key].cpu().numpy(), want[key]), key


@pytest.mark.parametrize("n,k,nc", [(1, 1, 1), (300, 5, 37), (257, 1, 5), (1000, 24, 513), (256, 3, 3)])
def test_class_report_against_the_restatement(n, k, nc):
    cls = _lists(n, k, nc, seed=n + k, no_pred=(n // 2,) if n > 4 else ())
    y = R.labels_for(n, nc, seed=n, stray=False)
    y[: n // 3] = cls[: n // 3, 0].clip(0)                                       # a third of the rows are top-1 hits
    y[n // 3: n // 2] = cls[n // 3: n // 2, k - 1].clip(0)                       # some hit only at the last list position
    if n > 4:
        y[n - 1], y[n - 2] = -1, nc                                              # labels outside [0, C)
    want = R.report(cls, y, nc, confusion=True)
    got = _report(cls, y, nc, confusion=True)
    _check_report(got, want)
    ignored, no_pred = want["misc"]
    if n > 4:
        assert ignored >= 1 and no_pred >= 1
    assert int(got["confusion"].sum()) == n - ignored - no_pred
    assert torch.equal(torch.diagonal(got["confusion"]), got["hit1"])
    assert int(got["support"].sum()) == n - ignored
    if k == 1:
        assert torch.equal(got["hitk"], got["hit1"])
    else:
        assert int(got["hitk"].sum()) > int(got["hit1"].sum())
    _check_report(_report(cls, y, nc), R.report(cls, y, nc))                     # without the confusion matrix
    for variant in R.REPORT_VARIANTS:                                            # the wrong statements are not what the device counts
        bad = R.report(cls, y, nc, True, variant)
        if n >= 256 and not (variant == "hitk_short" and k == 1):
            assert any(not np.array_equal(got[key].cpu().numpy(), bad[key]) for key in bad), variant


def test_class_report_adds_into_its_outputs_and_takes_contention():
    n, k, nc = 1000, 5, 37
    cls, y = _lists(n, k, nc, seed=3, no_pred=(17, 900)), R.labels_for(n, nc, seed=4)
    whole = _report(cls, y, nc, confusion=True)
    parts = _report(cls[:333], y[:333], nc, confusion=True)
    again = _report(cls[333:], y[333:], nc, confusion=True, out=parts)
    assert again is parts
    for key in whole:
        assert torch.equal(whole[key], parts[key]), key
    with pytest.raises(ValueError):
        _report(cls, y, nc, confusion=False, out=parts)
    # every row of one class and one prediction: all atomics of a counter meet on one address
    n = 5000
    cls1 = np.full((n, 3), 2, np.int32)
    cls1[:, 1], cls1[:, 2] = 0, 1
    y1 = np.full(n, 2, np.int64)
    _check_report(_report(cls1, y1, 4, confusion=True), R.report(cls1, y1, 4, True))
    y1[:] = 1                                                                    # hits at the last position only
    got = _report(cls1, y1, 4, confusion=True)
    _check_report(got, R.report(cls1, y1, 4, True))
    assert got["hit1"].sum() == 0 and int(got["hitk"][1]) == n and int(got["confusion"][1, 2]) == n


# ---- model level ----
def _int_model(kind, d=16, nc=37, seed=0):
    """A head with small-integer weights (and projection, bias): every feature and logit is exact in fp32 and in fp64."""
    from engine.models.head import UML, UMLClip
    g = torch.Generator().manual_seed(seed)
    ri = lambda *shape, lo=-3, hi=4: torch.randint(lo, hi, shape, generator=g).float()
    if kind == "clip":
        model = UMLClip(d, nc, logit_scale_init=float(np.log(4.0)))
    else:
        model = UML(d, 24 if "proj" in kind else 0, nc, bias="bias" in kind, learnable_temp="temp" in kind)
    model.to(DEV)
    with torch.no_grad():
        model.head.weight.copy_(ri(*model.head.weight.shape))
        if model.head.bias is not None:
            model.head.bias.copy_(ri(nc, lo=-40, hi=41))
        if getattr(model, "img_proj", None) is not None:
            model.img_proj.weight.copy_(ri(*model.img_proj.weight.shape, lo=-1, hi=2))
            if model.img_proj.bias is not None:
                model.img_proj.bias.copy_(ri(model.img_proj.bias.shape[0], lo=-2, hi=3))
        if "temp" in kind:
            model.img_scale.data.fill_(-2.0 if "neg" in kind else 3.0)
    return model, ri


KINDS = ["plain", "proj", "bias", "proj_bias_temp", "temp_neg", "clip"]


@pytest.mark.parametrize("kind", KINDS)
def test_predict_topk_equals_the_restatement_on_the_models_features(kind):
    model, ri = _int_model(kind)
    x = ri(150, 16).to(DEV)
    cls, logits = model.predict_topk(x, k=5)
    feats = model.extract_features(x).float().cpu().numpy()
    bias = None if model.head.bias is None else model.head.bias.detach().cpu().numpy()
    scale = float(model._scales[0])
    want, z64 = R.topk(feats, model.head.weight.detach().cpu().numpy(), bias, scale, 5)
    assert abs(scale - {"temp_neg": -2.0, "proj_bias_temp": 3.0, "clip": 4.0}.get(kind, 1.0)) < 1e-6
    assert np.array_equal(cls.cpu().numpy(), want)
    if kind != "clip":                                                           # (an integer scale: the logits are exact too)
        assert np.array_equal(logits.cpu().numpy(), z64.astype(np.float32))
        zi, _ = model(x)                                                         # and they are the forward's logits
        assert np.array_equal(np.take_along_axis(zi.cpu().numpy(), want, 1), logits.cpu().numpy())


def _unique_best(model, x):
    """Rows of x whose best logit is unique, so that no comparison rests on the forward kernel's tie rule."""
    z, _ = model(x)
    top2 = torch.topk(z, 2, dim=1).values
    return x[top2[:, 0] > top2[:, 1]]


@pytest.mark.parametrize("kind", ["plain", "proj_bias_temp", "clip"])
def test_validate_classwise_agrees_with_validate(kind, monkeypatch):
    import finetune as ft
    from engine.datasets.utils import FeatureLoader, FeatureTable
    model, ri = _int_model(kind)
    nc = model.head.weight.shape[0]
    x = _unique_best(model, ri(260, 16).to(DEV))
    n = x.shape[0]
    assert n >= 150
    best = model(x)[0].argmax(1).cpu()
    y = torch.where(torch.arange(n) % 3 == 0, torch.randint(0, nc, (n,), generator=torch.Generator().manual_seed(1)), best)
    loader = FeatureLoader(FeatureTable(x.cpu(), y, DEV), 32, shuffle=False)
    monkeypatch.setattr(ft, "EVAL_SLAB", 64)                                     # several slabs into one set of counters
    _, val_acc = ft.validate(model, loader)
    rep = ft.validate_classwise(model, loader, topk=5, confusion=True)
    assert model.training
    assert 0.6 < val_acc < 0.8
    assert rep["top1_acc"] == val_acc                                            # exactly: integer logits, unique maxima
    assert int(rep["correct"].sum()) / n == val_acc
    assert rep["n"] == n and rep["ignored"] == 0 and rep["no_prediction"] == 0 and rep["topk"] == 5
    feats = model.extract_features(x).float().cpu().numpy()
    bias = None if model.head.bias is None else model.head.bias.detach().cpu().numpy()
    want_cls, _ = R.topk(feats, model.head.weight.detach().cpu().numpy(), bias, float(model._scales[0]), 5)
    want = R.report(want_cls, y.numpy(), nc, confusion=True)
    for key, name in (("support", "support"), ("correct", "hit1"), ("correct_topk", "hitk"), ("confusion", "confusion")):
        assert rep[key].dtype == torch.int64 and np.array_equal(rep[key].numpy(), want[name]), key
    seen = want["support"] > 0
    acc = np.where(seen, want["hit1"] / np.maximum(want["support"], 1), np.nan)
    acck = np.where(seen, want["hitk"] / np.maximum(want["support"], 1), np.nan)
    assert rep["acc"].dtype == torch.float64 and np.array_equal(rep["acc"].numpy(), acc, equal_nan=True)
    assert np.array_equal(rep["acc_topk"].numpy(), acck, equal_nan=True)
    assert abs(rep["mean_class_acc"] - acc[seen].mean()) < 1e-12 and abs(rep["mean_class_acc_topk"] - acck[seen].mean()) < 1e-12
    assert rep["topk_acc"] == want["hitk"].sum() / n and rep["topk_acc"] > rep["top1_acc"]
    # a loader that is not slab-evaluable goes batch by batch into the same counters; stray labels are ignored
    y2 = y.clone()
    y2[5], y2[6] = -1, nc
    shuffled = FeatureLoader(FeatureTable(x.cpu(), y2, DEV), 32, shuffle=True, generator=torch.Generator().manual_seed(2))
    rep2 = ft.validate_classwise(model, shuffled, topk=5)
    want2 = R.report(want_cls, y2.numpy(), nc)
    assert rep2["ignored"] == 2 and rep2["n"] == n and "confusion" not in rep2
    assert np.array_equal(rep2["support"].numpy(), want2["support"]) and np.array_equal(rep2["correct_topk"].numpy(), want2["hitk"])
    assert rep2["top1_acc"] == want2["hit1"].sum() / (n - 2)
    assert ft.validate_classwise(model, loader, topk=1000)["topk"] == 24          # clamped to the kernels' list length ...
    few, _ = _int_model("plain", nc=3)
    small = FeatureLoader(FeatureTable(x.cpu(), y % 3, DEV), 32, shuffle=False)
    assert ft.validate_classwise(few, small)["topk"] == 3                         # ... and to the number of classes


def _same_report(a, b):
    assert set(a) == set(b)
    for key in a:
        if torch.is_tensor(a[key]):
            assert np.array_equal(a[key].numpy(), b[key].numpy(), equal_nan=True), key
        else:
            assert a[key] == b[key] or (a[key] != a[key] and b[key] != b[key]), key


def _cfg1_run(classwise):
    import finetune as ft
    from engine.datasets.utils import FeatureLoader, FeatureTable, TextTensorDataset
    from engine.models.head import UMLClip
    from engine.optimizer.optim import build_optimizer
    from engine.optimizer.scheduler import build_lr_scheduler
    from engine.tools.utils import set_random_seed
    from oracle import fixtures_cfg1 as FX
    inp = {k: torch.from_numpy(v) for k, v in FX.cfg1_inputs().items()}
    set_random_seed(FX.SEED)
    text_ds = TextTensorDataset(inp["x_txt"], inp["y_txt"], torch.zeros(len(inp["y_txt"]), dtype=torch.long))
    model = UMLClip(FX.D, FX.C, logit_scale_init=FX.SCALE_LOG, bias=False)
    model.to(DEV)
    model.zero_shot_init(text_ds)
    optimizer = build_optimizer(model.parameters(), "adamw", FX.LR, FX.WD)
    scheduler = build_lr_scheduler(optimizer, "cosine", 50, 12800, warmup_type="linear", warmup_lr=1e-5)
    B = FX.BATCH
    image_loader = FeatureLoader(FeatureTable(inp["x_img"], inp["y_img"], DEV), B, shuffle=True, kind="image")
    text_loader = FeatureLoader(FeatureTable(text_ds.input_tensor, text_ds.label_tensor, DEV), B, shuffle=True, kind="text")
    val_loader = FeatureLoader(FeatureTable(inp["x_val"], inp["y_val"], DEV), B, shuffle=False)
    test_loader = FeatureLoader(FeatureTable(inp["x_test"], inp["y_test"], DEV), B, shuffle=False)
    kw = {} if classwise is None else {"classwise": classwise}
    out = ft.train(model, image_loader, text_loader, val_loader, test_loader, optimizer, scheduler, device=DEV,
                   max_iters=FX.MAX_ITERS, alpha=FX.ALPHA, eval_freq=FX.EVAL_FREQ, patience=FX.PATIENCE, **kw)
    return out, model, val_loader


def test_train_fills_val_classwise_and_changes_nothing_else():
    import finetune as ft
    from conftest import load_golden
    g = load_golden("train_cfg1")
    off, _, _ = _cfg1_run(None)
    on, model, val_loader = _cfg1_run({"topk": 5, "confusion": True})
    assert off["val_classwise"] is None
    assert on["iter"] == off["iter"] == int(g["best_iter"]) and on["val_acc"] == off["val_acc"] and on["val_loss"] == off["val_loss"]
    assert torch.equal(on["train_scalars"], off["train_scalars"]) and len(on["train_scalars"]) == int(g["n_steps"])
    assert set(on["model"]) == set(off["model"]) and all(torch.equal(on["model"][k], off["model"][k]) for k in on["model"])
    rep = on["val_classwise"]
    _same_report(rep, ft.validate_classwise(model, val_loader, topk=5, confusion=True))       # the model the run returns
    assert rep["n"] == 400 and rep["support"].tolist() == [4] * 100 and tuple(rep["confusion"].shape) == (100, 100)
    # 400 validation rows, fp32 forward against the fp64 refinement: the two top-1 figures differ by at most rows whose two best
    # logits lie within fp32 rounding of each other; none is expected here, one would be 1 / 400
    assert abs(rep["top1_acc"] - on["val_acc"]) <= 1 / 400 + 1e-12
    assert rep["top1_acc"] <= rep["topk_acc"] <= 1.0 and abs(rep["mean_class_acc"] - rep["top1_acc"]) < 1e-12   # balanced classes


def test_train_grouped_fills_the_flagged_run_only():
    import finetune as ft
    from engine.datasets.utils import FeatureLoader, FeatureTable
    from engine.models.head import UMLClip
    from engine.optimizer.optim import build_optimizer
    from engine.optimizer.scheduler import build_lr_scheduler
    g = torch.Generator().manual_seed(5)
    nc, d = 12, 64
    proto = torch.randn(nc, d, generator=g)

    def draw(n):
        y = torch.randint(0, nc, (n,), generator=g)
        return torch.nn.functional.normalize(proto[y] + 1.5 * torch.randn(n, d, generator=g), dim=1), y
    tables = {name: FeatureTable(*draw(n), DEV) for name, n in (("train", 120), ("text", 80), ("val", 90))}

    def runs(flags):
        out = []
        for k, flag in enumerate(flags):
            torch.manual_seed(7 + k)
            gen = torch.Generator()
            gen.manual_seed(7 + k)
            model = UMLClip(d, nc, logit_scale_init=4.60517).to(DEV)
            optimizer = build_optimizer(model.parameters(), "adamw", 1e-3, 0.01)
            scheduler = build_lr_scheduler(optimizer, "cosine", 10, 60, warmup_type="linear", warmup_lr=1e-5)
            r = dict(model=model, image_loader=FeatureLoader(tables["train"], 16, shuffle=True, kind="image", generator=gen),
                     text_loader=FeatureLoader(tables["text"], 16, shuffle=True, kind="text", generator=gen),
                     val_loader=FeatureLoader(tables["val"], 16, shuffle=False, generator=gen), test_loader=None,
                     optimizer=optimizer, scheduler=scheduler, max_iters=60, alpha=1.0, patience=5)
            if flag is not None:
                r["classwise"] = flag
            out.append(r)
        return out
    flagged = runs([{"topk": 3, "confusion": True}, None, True])
    outs = ft.train_grouped(flagged, device=DEV, eval_freq=20)
    plain = ft.train_grouped(runs([None, False, None]), device=DEV, eval_freq=20)
    assert outs[1]["val_classwise"] is None and all(p["val_classwise"] is None for p in plain)
    for a, b in zip(outs, plain):
        assert a["iter"] == b["iter"] and a["val_acc"] == b["val_acc"] and torch.equal(a["train_scalars"], b["train_scalars"])
        assert all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"])
    rep = outs[0]["val_classwise"]
    _same_report(rep, ft.validate_classwise(flagged[0]["model"], flagged[0]["val_loader"], topk=3, confusion=True))
    assert rep["n"] == 90 and rep["topk"] == 3 and int(rep["confusion"].sum()) == 90
    assert abs(rep["top1_acc"] - outs[0]["val_acc"]) <= 1 / 90 + 1e-12           # (at most one row of 90 within fp32 rounding of a tie)
    default = outs[2]["val_classwise"]                                           # classwise=True: the defaults of validate_classwise
    _same_report(default, ft.validate_classwise(flagged[2]["model"], flagged[2]["val_loader"]))
    assert default["topk"] == 5 and "confusion" not in default
