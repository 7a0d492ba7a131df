"""GPU: the multinomial logistic probe (umlh_softmax_probe_* through ctypes, umlh.SoftmaxProbe, multibench.train.evaluate with
``label_fn``, finetune.linear_probe) against the float64 statement of tests/_softmax_probe_ref.py and the fixtures
tests/golden/softmax_probe*.npz (sklearn's coefficients, the float64 optimum, TAU).

Bounds are derived, not tuned: the objective may differ from float64 by R.objective_allowance, a gradient entry by the fp32 GEMM
criterion of tests/_gemm_ref.py, a converged fit's float64 max|g| by gtol + R.grad_allowance.  Every measured figure is printed
before it is asserted (run with -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gemm_ref as GR
import _softmax_probe_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = list(R.CASES)
F32_SENTINEL = 0x7FBADBAD
F64_SENTINEL = 0x7FF8BADBADBADBAD


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f32_sentinels(*shape):
    return torch.full(shape, F32_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def f64_sentinels(n):
    return torch.full((n,), F64_SENTINEL, dtype=torch.int64, device=DEV).view(torch.float64)


def untouched(t):
    bits = t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    return bool((bits == (F32_SENTINEL if t.dtype == torch.float32 else F64_SENTINEL)).all())


@pytest.fixture(scope="module")
def golden():
    return load_golden("softmax_probe")


@pytest.fixture(scope="module")
def problems(golden):
    """case -> dict of the host arrays (x, y, stats, x~, optimum, sklearn's coefficients, tau) and the device operands (the
    features with the case's row stride); built once."""
    out = {}
    for name, c in R.CASES.items():
        x, y = R.make_case(name)
        stats = R.column_stats(x) if c["standardize"] else None
        xt = R.x_tilde(x, stats)
        wide = torch.full((c["n"], c["ldx"]), float("nan"), device=DEV)
        wide[:, :c["d"]] = dev(x)
        sk = np.concatenate([golden[f"{name}.sk_coef"], golden[f"{name}.sk_intercept"][:, None]], axis=1)
        out[name] = dict(c, x=x, y=y, stats=stats, xt=xt, opt=golden[f"{name}.opt"], sk=sk, tau=float(golden[f"{name}.tau"]),
                         xd=wide[:, :c["d"]], yd=dev(y), statsd=None if stats is None else dev(stats))
    return out


def sp_eval(xd, yd, W, K, c=1.0, statsd=None, ldc=None, want_grad=True):
    """umlh_softmax_probe_eval through ctypes into sentinel buffers: (objective, grad [K, D] or None, max_grad); asserts that
    all of the output was written and nothing behind it."""
    from umlh._lib import check, load_library
    lib = load_library()
    n, d = xd.shape
    D = d + 1
    ldc = ldc or D
    coef = f32_sentinels(K, ldc)
    coef[:, :D] = torch.as_tensor(W, dtype=torch.float32).to(DEV)
    nbytes = lib.umlh_softmax_probe_scratch_bytes(n, d, K, 0, 1)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ldg = D + 2
    grad = f32_sentinels(K + 1, ldg)
    scal = f64_sentinels(4)
    check(lib.umlh_softmax_probe_eval(xd.data_ptr(), n, d, xd.stride(0), yd.data_ptr(), None if statsd is None else statsd.data_ptr(), K, c,
                                      coef.data_ptr(), ldc, scal[0:].data_ptr(), grad.data_ptr() if want_grad else None, ldg,
                                      scal[2:].data_ptr(), scratch.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "umlh_softmax_probe_eval")
    torch.cuda.synchronize()
    assert untouched(scal[1::2]) and untouched(coef[:, D:])
    if want_grad:
        assert untouched(grad[K:]) and untouched(grad[:K, D:])
        assert not (grad[:K, :D].contiguous().view(torch.int32) == F32_SENTINEL).any()
    else:
        assert untouched(grad)
    return float(scal[0]), (grad[:K, :D].cpu().numpy() if want_grad else None), float(scal[2])


def sp_fit(xd, yd, K, c=1.0, statsd=None, max_iter=200, history=10, gtol=0.0, W0=None, stream=None):
    """umlh_softmax_probe_fit through ctypes into sentinel buffers: (W [K, D], record dict, objectives)."""
    from umlh._lib import check, load_library
    lib = load_library()
    n, d = xd.shape
    D, ldc = d + 1, d + 3
    coef = f32_sentinels(K + 1, ldc)
    if W0 is not None:
        coef[:K, :D] = torch.as_tensor(W0, dtype=torch.float32).to(DEV)
    nbytes = lib.umlh_softmax_probe_scratch_bytes(n, d, K, max_iter, history)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rec = torch.full((4,), F64_SENTINEL, dtype=torch.int64, device=DEV)
    obj = f64_sentinels(max_iter + 2)
    st = stream if stream is not None else torch.cuda.current_stream()
    st.wait_stream(torch.cuda.current_stream())                       # the buffers above were filled on the current stream
    check(lib.umlh_softmax_probe_fit(xd.data_ptr(), n, d, xd.stride(0), yd.data_ptr(), None if statsd is None else statsd.data_ptr(), K, c,
                                     max_iter, history, gtol, 0 if W0 is None else 1, coef.data_ptr(), ldc, rec.data_ptr(), obj.data_ptr(),
                                     scratch.data_ptr(), nbytes, C.c_void_p(st.cuda_stream)), "umlh_softmax_probe_fit")
    torch.cuda.synchronize()
    assert untouched(coef[K:]) and untouched(coef[:K, D:]) and untouched(obj[max_iter + 1:]) and int(rec[3]) == F64_SENTINEL
    raw = rec[:3].cpu().numpy().view(np.uint8)
    record = {"n_iter": int(raw[0:4].view("<i4")[0]), "converged": int(raw[4:8].view("<i4")[0]),
              "max_grad": float(raw[8:16].view("<f8")[0]), "objective": float(raw[16:24].view("<f8")[0])}
    return coef[:K, :D].cpu().numpy(), record, obj[:max_iter + 1].cpu().numpy()


def grad_error(W, p, got, c=1.0):
    """(max, rms) of the device gradient's error over the term-magnitude sums of R^T X~ (+ the ridge term's own magnitude)."""
    _, g64 = R.objective_grad(W, p["xt"], p["y"], c)
    xt = p["xt"].astype(np.float64)
    z = xt @ np.asarray(W, np.float64).T
    e = np.exp(z - z.max(1, keepdims=True))
    r = e / e.sum(1, keepdims=True)
    ok = (p["y"] >= 0) & (p["y"] < W.shape[0])
    r[np.arange(len(ok))[ok], p["y"][ok]] -= 1.0
    r[~ok] = 0.0
    S = np.abs(r).T @ np.abs(xt)
    S[:, :-1] += np.abs(np.asarray(W, np.float64)[:, :-1]) / c
    return GR.gemm_err(got, g64, S)


# ---- 1. evaluation against float64 ----
@pytest.mark.parametrize("name", CASES)
def test_eval_against_float64(problems, name):
    p = problems[name]
    K, D = p["K"], p["d"] + 1
    rng = np.random.default_rng(p["seed"])
    points = {"zero": np.zeros((K, D), np.float32), "optimum": p["opt"].astype(np.float32),
              "random": (rng.standard_normal((K, D)) * 0.5).astype(np.float32)}
    for tag, W in points.items():
        f, g, mg = sp_eval(p["xd"], p["yd"], W, K, statsd=p["statsd"], ldc=D + (3 if tag == "random" else 0))
        f64, g64 = R.objective_grad(W, p["xt"], p["y"], R.C_REG)
        allow = R.objective_allowance(W, p["xt"], p["y"], f64)
        err = grad_error(W, p, g)
        print(f"{name} at {tag}: f={f:.12g} |f - f64|={abs(f - f64):.3e} allowance={allow:.3e}  grad err/S max=2^{np.log2(max(err[0], 1e-300)):.1f} "
              f"rms=2^{np.log2(max(err[1], 1e-300)):.1f}  max|g|={mg:.6g} f64 {np.abs(g64).max():.6g}")
        assert abs(f - f64) <= allow
        assert GR.meets_criterion(err)
        assert abs(mg - np.abs(g64).max()) <= R.grad_allowance(W, p["xt"], p["y"]) + 2.0 ** -20 * np.abs(W).max() / R.C_REG
        assert mg >= np.abs(g).max() * (1 - 2.0 ** -23)             # max|g| is taken before the gradient is rounded to fp32


def test_eval_edges(problems):
    """Rows with out-of-range labels (skipped, no fault), logits of +-90, n_class = 2, objective only."""
    p = dict(problems["n257_d5_k3"])
    y2 = p["y"].copy()
    y2[::7] = -1
    y2[3::11] = 3
    y2[5] = 2 ** 30
    p["y"] = y2
    W = p["opt"].astype(np.float32)
    f, g, mg = sp_eval(p["xd"], dev(y2), W, 3)
    f64, g64 = R.objective_grad(W, p["xt"], y2, 1.0)
    print(f"out-of-range labels: |f - f64|={abs(f - f64):.3e} grad err={grad_error(W, p, g)}")
    assert abs(f - f64) <= R.objective_allowance(W, p["xt"], y2, f64) and GR.meets_criterion(grad_error(W, p, g))
    # logits of +-90 from the intercepts alone: f = 0 + 180 + 90 + 0 exactly representable terms
    x = torch.zeros((4, 1), device=DEV)
    W90 = np.array([[0.0, 90.0], [0.0, -90.0], [0.0, 0.0]], np.float32)
    f, g, mg = sp_eval(x, dev(np.array([0, 1, 2, 0], np.int32)), W90, 3)
    f64, g64 = R.objective_grad(W90, np.concatenate([np.zeros((4, 1)), np.ones((4, 1))], 1), np.array([0, 1, 2, 0]), 1.0)
    print(f"logits +-90: f={f!r} f64={f64!r} g={g.ravel()}")
    assert abs(f - f64) <= 2.0 ** -40 * f64 and np.isfinite(g).all() and np.abs(g - g64).max() <= 2.0 ** -20 * 4
    # two classes
    rng = np.random.default_rng(3)
    x2 = rng.standard_normal((130, 9)).astype(np.float32)
    yb = (rng.random(130) < 0.4).astype(np.int32)
    Wb = (rng.standard_normal((2, 10)) * 0.7).astype(np.float32)
    pb = dict(xt=R.x_tilde(x2), y=yb)
    f, g, mg = sp_eval(dev(x2), dev(yb), Wb, 2, c=0.5)
    f64, _ = R.objective_grad(Wb, pb["xt"], yb, 0.5)
    assert abs(f - f64) <= R.objective_allowance(Wb, pb["xt"], yb, f64) and GR.meets_criterion(grad_error(Wb, pb, g, c=0.5))
    f_only, none, mg_only = sp_eval(dev(x2), dev(yb), Wb, 2, c=0.5, want_grad=False)
    assert none is None and f_only == f and mg_only == mg


# ---- 2. the fit ----
@pytest.fixture(scope="module")
def fitted(problems):
    """case -> (SoftmaxProbe fitted at gtol = 1e-6 n with max_iter = 200, its coefficients [K, d + 1] on the host); fitted once."""
    import umlh
    out = {}
    for name, p in problems.items():
        pr = umlh.SoftmaxProbe(C=R.C_REG, max_iter=200, gtol=1e-6 * p["n"], standardize=p["standardize"], keep_objectives=True)
        pr.fit(p["xd"], p["yd"])
        out[name] = (pr, torch.cat([pr.coef_, pr.intercept_[:, None]], dim=1).cpu().numpy())
    return out


@pytest.mark.parametrize("name", CASES)
def test_fit_reaches_the_optimum(problems, fitted, name):
    p, (pr, W) = problems[name], fitted[name]
    rec, gtol = pr.record(), 1e-6 * p["n"]
    f64, g64 = R.objective_grad(W, p["xt"], p["y"], R.C_REG)
    f_sk = R.objective_grad(p["sk"], p["xt"], p["y"], R.C_REG, False)[0]
    f_opt = R.objective_grad(p["opt"], p["xt"], p["y"], R.C_REG, False)[0]
    E = R.grad_allowance(W, p["xt"], p["y"])
    obj = pr._objectives.cpu().numpy()
    sums = np.abs(W.astype(np.float64).sum(0))
    sum_tol = (rec["n_iter"] + 1) * 2.0 ** -23 * (p["K"] * np.abs(W).max() + np.abs(p["xt"]).sum(0).max())
    print(f"{name}: {rec} f64 gap to the optimum={(f64 - f_opt) / f_opt:.2e} (sklearn {(f_sk - f_opt) / f_opt:.2e}) f64 max|g|={np.abs(g64).max():.3e} "
          f"gtol={gtol:.3e} E={E:.2e} objectives[-1] - record={obj[rec['n_iter']] - rec['objective']:.2e} class sums max={sums.max():.2e} tol={sum_tol:.2e}")
    assert rec["converged"] == 1 and 1 <= rec["n_iter"] <= 200
    assert np.abs(g64).max() <= gtol + E
    assert f64 <= f_sk
    f, _, mg = sp_eval(p["xd"], p["yd"], W, p["K"], statsd=p["statsd"])
    assert (f, mg) == (rec["objective"], rec["max_grad"])                       # bit for bit
    assert (np.diff(obj[: rec["n_iter"] + 1]) <= 0).all() and np.isnan(obj[rec["n_iter"] + 1:]).all()
    assert torch.equal(pr.objectives_, pr._objectives[: rec["n_iter"] + 1])
    assert sums.max() <= sum_tol


# ---- 3. predictions ----
@pytest.mark.parametrize("name", CASES)
def test_predictions(problems, fitted, name):
    from umlh.report import class_report, topk_classes
    p, (pr, W) = problems[name], fitted[name]
    top, marg = R.margins(p["opt"], p["xt"])
    decidable = marg > p["tau"]
    xraw = p["xd"]
    pred = pr.predict(xraw).cpu().numpy()
    print(f"{name}: decidable {decidable.mean():.4f}, agreement on them {np.mean(pred[decidable] == top[decidable]):.4f}")
    assert decidable.mean() >= 0.95 and (pred[decidable] == top[decidable]).all()
    assert np.array_equal(pr.predict_topk(xraw, 2)[:, 0].cpu().numpy(), pred)
    cls, _ = topk_classes(xraw, pr.raw_weight_, pr.raw_bias_, k=1)
    hits = int(class_report(cls, p["yd"].to(torch.int64), p["K"])["hit1"].sum())
    assert pr.score(xraw, p["yd"]) == hits / p["n"] == float(np.mean(pred == p["y"]))
    assert int(pr.correct(xraw, p["yd"])) == hits and pr.correct(xraw, p["yd"]).device.type == "cuda"
    dec = pr.decision_function(xraw).cpu().numpy()
    z64 = p["xt"].astype(np.float64) @ W.astype(np.float64).T
    # the GEMM criterion on the raw-feature products, plus one rounding each of the standardised feature, the folded weight, the
    # bias and the bias addition (4 x 2^-24)
    s_raw = (np.abs(p["x"]).astype(np.float64) @ np.abs(pr.raw_weight_.cpu().numpy()).astype(np.float64).T + np.abs(pr.raw_bias_.cpu().numpy())).max()
    print(f"{name}: decision_function max err {np.abs(dec - z64).max():.3e} bound {(2.0 ** -20 + 2.0 ** -22) * s_raw:.3e}")
    assert dec.shape == (p["n"], p["K"]) and np.abs(dec - z64).max() <= (2.0 ** -20 + 2.0 ** -22) * s_raw
    # the fold against float64: 1 ulp per entry; predictions on raw features equal the standardised model's on decidable rows
    w, b = pr.raw_weight_.cpu().numpy(), pr.raw_bias_.cpu().numpy()
    d = p["d"]
    if p["stats"] is None:
        assert np.array_equal(w, W[:, :d]) and np.array_equal(b, W[:, d])
    else:
        w64 = W[:, :d].astype(np.float64) / p["stats"][d:]
        b64 = W[:, d].astype(np.float64) - (w64 * p["stats"][:d]).sum(1)
        ulp = lambda v: np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
        print(f"{name}: fold error in ulp: w {np.max(np.abs(w - w64) / ulp(w64)):.3f} b {np.max(np.abs(b - b64) / ulp(b64)):.3f}")
        assert (np.abs(w - w64) <= ulp(w64)).all() and (np.abs(b - b64) <= ulp(b64)).all()
        own = np.argmax(z64, axis=1)
        own_marg = np.sort(z64, axis=1)
        ok = (own_marg[:, -1] - own_marg[:, -2]) > p["tau"]
        assert (pred[ok] == own[ok]).all()


# ---- 4. determinism and control ----
def test_fit_is_reproducible_across_calls_streams_and_load_paths(problems):
    p = problems["n600_d33_k7_ld40"]
    gtol = 1e-6 * p["n"]
    W0, rec0, obj0 = sp_fit(p["xd"], p["yd"], p["K"], gtol=gtol)
    W1, rec1, obj1 = sp_fit(p["xd"], p["yd"], p["K"], gtol=gtol)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    W2, rec2, obj2 = sp_fit(p["xd"], p["yd"], p["K"], gtol=gtol, stream=side)
    # the 4-byte load path: an odd row stride, then a base one float past a 16-byte boundary
    odd = torch.full((p["n"], 41), float("nan"), device=DEV)
    odd[:, :33] = dev(p["x"])
    flat = torch.full((p["n"] * 40 + 1,), float("nan"), device=DEV)
    shifted = flat[1:].view(p["n"], 40)[:, :33]
    shifted.copy_(dev(p["x"]))
    assert p["xd"].data_ptr() % 16 == 0 and p["xd"].stride(0) % 4 == 0 and shifted.data_ptr() % 16 == 4
    W3, rec3, obj3 = sp_fit(odd[:, :33], p["yd"], p["K"], gtol=gtol)
    W4, rec4, obj4 = sp_fit(shifted, p["yd"], p["K"], gtol=gtol)
    for W, rec, obj in ((W1, rec1, obj1), (W2, rec2, obj2), (W3, rec3, obj3), (W4, rec4, obj4)):
        assert np.array_equal(W.view(np.int32), W0.view(np.int32)) and rec == rec0 and np.array_equal(obj, obj0, equal_nan=True)
    assert rec0["converged"] == 1


def test_fit_control(problems):
    p = problems["n600_d33_k7_ld40"]
    K, gtol = p["K"], 1e-6 * p["n"]
    # one iteration: exactly one accepted step
    W, rec, obj = sp_fit(p["xd"], p["yd"], K, max_iter=1, gtol=gtol)
    print(f"max_iter=1: {rec} objectives={obj}")
    assert rec["n_iter"] == 1 and rec["converged"] == 0 and obj[1] < obj[0] and obj[0] == pytest.approx(p["n"] * np.log(K), rel=1e-12)
    assert np.abs(W).max() > 0
    # a huge gtol stops at iteration 0 with W untouched (here: the start coefficients, bit for bit)
    rng = np.random.default_rng(9)
    Ws = (rng.standard_normal((K, p["d"] + 1)) * 0.1).astype(np.float32)
    W, rec, obj = sp_fit(p["xd"], p["yd"], K, gtol=1e30, W0=Ws)
    assert rec["n_iter"] == 0 and rec["converged"] == 1 and np.array_equal(W, Ws) and np.isnan(obj[1:]).all()
    W, rec, obj = sp_fit(p["xd"], p["yd"], K, gtol=1e30)
    assert rec["n_iter"] == 0 and rec["converged"] == 1 and (W == 0).all()
    # a warm start from the fitted coefficients stops at iteration 0
    Wf, recf, _ = sp_fit(p["xd"], p["yd"], K, gtol=gtol)
    W, rec, obj = sp_fit(p["xd"], p["yd"], K, gtol=gtol, W0=Wf)
    assert recf["converged"] == 1 and rec["n_iter"] == 0 and rec["converged"] == 1 and np.array_equal(W, Wf)
    assert (rec["objective"], rec["max_grad"]) == (recf["objective"], recf["max_grad"])
    # along C = 0.1 -> 1 a warm start takes no more iterations than a cold one and decides the same rows the same way
    W01, rec01, _ = sp_fit(p["xd"], p["yd"], K, c=0.1, gtol=gtol)
    Ww, recw, _ = sp_fit(p["xd"], p["yd"], K, c=1.0, gtol=gtol, W0=W01)
    print(f"C=0.1: {rec01}; C=1 warm: {recw}; C=1 cold: {recf}")
    assert rec01["converged"] == 1 and recw["converged"] == 1 and recw["n_iter"] <= recf["n_iter"]
    top, marg = R.margins(p["opt"], p["xt"])
    ok = marg > p["tau"]
    assert (R.margins(Ww, p["xt"])[0][ok] == top[ok]).all() and (R.margins(Wf, p["xt"])[0][ok] == top[ok]).all()
    # history = 1 and 32 reach the same optimum
    for h in (1, 32):
        Wh, rech, _ = sp_fit(p["xd"], p["yd"], K, gtol=gtol, history=h)
        _, g64 = R.objective_grad(Wh, p["xt"], p["y"], 1.0)
        print(f"history={h}: {rech}")
        assert rech["converged"] == 1 and np.abs(g64).max() <= gtol + R.grad_allowance(Wh, p["xt"], p["y"])


def test_fit_with_a_nan_row_ends_clean(problems):
    p = problems["n257_d5_k3"]
    x = p["x"].copy()
    x[17, 2] = np.nan
    W, rec, obj = sp_fit(dev(x), p["yd"], 3, gtol=1e-6 * p["n"], max_iter=20)          # sp_fit checks the sentinels around the outputs
    print(f"NaN row: {rec}")
    assert rec["converged"] == 0 and rec["n_iter"] == 0 and np.isnan(rec["max_grad"])
    f, g, mg = sp_eval(dev(x), p["yd"], np.zeros((3, 6), np.float32), 3)
    assert np.isnan(f) and np.isnan(mg)


def test_argument_errors(problems):
    from umlh._lib import load_library
    lib = load_library()
    p = problems["n257_d5_k3"]
    assert lib.umlh_softmax_probe_scratch_bytes(257, 5, 3, 10, 10) > lib.umlh_softmax_probe_scratch_bytes(257, 5, 3, 0, 0) > 0
    for bad in ((1, 5, 3, 10, 10), (257, 0, 3, 10, 10), (257, 2049, 3, 10, 10), (257, 5, 1, 10, 10), (257, 5, 4097, 10, 10),
                (2 ** 20, 5, 2048, 10, 10), (257, 5, 3, 1001, 10), (257, 5, 3, 10, 0), (257, 5, 3, 10, 33), (257, 5, 3, -1, 10)):
        assert lib.umlh_softmax_probe_scratch_bytes(*bad) == 0, bad
    coef = torch.zeros((3, 6), device=DEV)
    rec = torch.zeros(24, dtype=torch.uint8, device=DEV)
    nbytes = lib.umlh_softmax_probe_scratch_bytes(257, 5, 3, 5, 10)
    scratch = torch.empty(nbytes + 8, dtype=torch.uint8, device=DEV)
    good = dict(x=p["xd"].data_ptr(), n=257, d=5, ldx=5, y=p["yd"].data_ptr(), stats=None, n_class=3, c=1.0, max_iter=5, history=10, gtol=0.0,
                init=0, coef=coef.data_ptr(), ldc=6, record=rec.data_ptr(), objectives=None, scratch=scratch.data_ptr(), scratch_bytes=nbytes,
                stream=None)
    for change, word in ((dict(x=None), "null pointer"), (dict(ldx=4), "ldx"), (dict(ldc=5), "ldc"), (dict(c=0.0), "c="), (dict(max_iter=0), "max_iter"),
                         (dict(history=33), "history"), (dict(gtol=-1.0), "gtol"), (dict(init=2), "init"), (dict(record=None), "record"),
                         (dict(n_class=1), "n_class"), (dict(scratch_bytes=nbytes - 1), "needed"), (dict(scratch=scratch.data_ptr() + 4), "aligned")):
        rc = lib.umlh_softmax_probe_fit(*{**good, **change}.values())
        msg = lib.umlh_last_error().decode()
        assert rc != 0 and "umlh_softmax_probe_fit" in msg and word in msg, (change, msg)
    torch.cuda.synchronize()
    assert (coef == 0).all()


# ---- 5. Python layer and users ----
def test_softmax_probe_remaps_label_values():
    import umlh
    rng = np.random.default_rng(21)
    values = np.array([-3, 10, 11, 40])
    centers = rng.standard_normal((4, 6)) * 3
    idx = np.arange(400) % 4
    x = (centers[idx] + rng.standard_normal((400, 6))).astype(np.float32)
    pr = umlh.SoftmaxProbe().fit(dev(x), dev(values[idx]))
    assert pr.classes_.cpu().tolist() == values.tolist() and pr.coef_.shape == (4, 6) and pr.intercept_.shape == (4,)
    pred = pr.predict(dev(x)).cpu().numpy()
    assert set(np.unique(pred)) <= set(values.tolist()) and np.mean(pred == values[idx]) > 0.9
    assert pr.score(dev(x), dev(values[idx])) == float(np.mean(pred == values[idx]))
    assert pr.converged_ == 1 and pr.n_iter_ >= 1 and pr.max_grad_ <= 1e-4 * 400 and np.isfinite(pr.objective_)
    same = umlh.SoftmaxProbe().fit(dev(x), dev(idx), check_classes=False, n_classes=4)
    assert torch.equal(same.coef_, pr.coef_) and same.classes_.cpu().tolist() == [0, 1, 2, 3]
    warm = umlh.SoftmaxProbe().fit(dev(x), dev(values[idx]), coef_init=pr)
    assert warm.n_iter_ == 0 and torch.equal(warm.coef_, pr.coef_)
    with pytest.raises(ValueError, match="at least 2 classes"):
        umlh.SoftmaxProbe().fit(dev(x), dev(np.zeros(400, np.int64)))
    with pytest.raises(ValueError, match="coef_init"):
        umlh.SoftmaxProbe().fit(dev(x), dev(idx), coef_init=torch.zeros(3, 7))
    with pytest.raises(ValueError, match="labels for"):
        umlh.SoftmaxProbe().fit(dev(x), dev(idx[:-1]))
    assert isinstance(umlh.logistic_probe("lbfgs", 4), umlh.SoftmaxProbe) and isinstance(umlh.logistic_probe("lbfgs", 2), umlh.LogisticProbe)


def test_evaluate_with_label_fn():
    import umlh
    from multibench.train import evaluate, evaluate_raw_data
    from test_probe_gpu import _config, _model
    g = load_golden("probe_e2e_humor")
    ds, cfg = str(g["ds_name"]), _config(g)
    model = _model(str(g["model"]))
    three = lambda lab: np.arange(np.asarray(lab).size) % 3 * 5 - 5             # synthetic 3-class labels -5, 0, 5 by position
    res, emb, clfs = evaluate(model, cfg, ds, device=DEV, return_embeddings=True, label_fn=three)
    base = evaluate(model, cfg, ds, device=DEV)
    assert set(res) == set(base) == set(g["keys_eval"])
    assert [type(c).__name__ for c in clfs] == ["LogisticProbe"] * 3 + ["SoftmaxProbe"] * 3
    assert res["val/modality_separate"] == base["val/modality_separate"]
    z = emb["train"].shape[1] // 2
    lab = {t: dev(np.arange(emb[t].shape[0]) % 3) for t in emb}
    for name, cols in (("x", slice(0, z)), ("y", slice(z, 2 * z)), ("xy", slice(0, 2 * z))):
        own = umlh.SoftmaxProbe().fit(emb["train"][:, cols], lab["train"])
        for t in ("val", "test"):
            assert res[f"{t}/score_{name}"] == own.score(emb[t][:, cols], lab[t])
    raw = evaluate_raw_data(cfg, ds, label_fn=three)
    assert set(raw) == set(g["keys_raw"]) and all(0.0 <= v <= 1.0 for v in raw.values())
    # the default path is what it was: label_fn=None is the same call
    assert evaluate(model, cfg, ds, device=DEV, label_fn=None) == pytest.approx(base, nan_ok=True, abs=0)
    assert evaluate_raw_data(cfg, ds, label_fn=None) == evaluate_raw_data(cfg, ds)
    with pytest.raises(NotImplementedError):
        evaluate(model, cfg, "mimic", device=DEV)
    assert set(evaluate(model, cfg, "mimic", device=DEV, label_fn=three)) == set(base)


def test_linear_probe(problems):
    import finetune
    p = problems["n1600_d512_k100"]
    x, y = torch.from_numpy(p["x"]), torch.from_numpy(p["y"]).long()
    tr, va, te = slice(0, 960), slice(960, 1280), slice(1280, 1600)
    assert len(np.unique(p["y"][tr])) == 100
    out = finetune.linear_probe((x[tr], y[tr]), (x[va], y[va]), (x[te], y[te]), num_classes=100, classwise=True, device=DEV)
    print({k: out[k] for k in ("best_C", "val_acc", "test_acc", "per_C")}, [r["n_iter"] for r in out["records"]])
    accs = [r["val_acc"] for r in out["per_C"]]
    assert [r["C"] for r in out["per_C"]] == [0.01, 0.1, 1.0, 10.0, 100.0] and len(out["records"]) == 5
    best = int(np.argmax(accs))                                                  # (np.argmax takes the first of equals: the smaller C)
    assert out["best_C"] == out["per_C"][best]["C"] and out["val_acc"] == accs[best] and out["test_acc"] == out["per_C"][best]["test_acc"]
    assert out["test_acc"] == out["probe"].score(x[te].to(DEV), y[te].to(DEV)) and out["probe"].C == out["best_C"]
    assert out["classwise"]["top1_acc"] == out["test_acc"] and int(out["classwise"]["support"].sum()) == 320
