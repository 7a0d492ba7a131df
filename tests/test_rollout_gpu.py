"""GPU: the one-launch rollout (umlh.rollout_rows, multibench.train.rollout) and the spectra (umlh.seq_spectrum,
multibench.train.spectral_bias, train(rollout_spectra=True)).

Yardsticks.  Rollout: the float64 closed form of tests/_rollout_ref.py, per generated step max|got - ref| / max|ref| under the
bound of that module's criterion table (8 x what an fp32 numpy evaluation of the same formulas reaches), the seed row exact;
the reference's own outputs (tests/golden/rollout*.npz) under the fixture's bound.  Spectrum: numpy's float64 rfft at 1e-12 of
max_k out[k] -- the kernel's sums are fp64 chains of at most T + 16 + 16 + 4096 terms of about unit size, each rounding by 2^-53
(as for umlh_seq_step_stats), and the fp64 cos / sin table is good to a few 2^-53.  Outputs are written into NaN-sentinel
buffers one row longer than needed.  Every measured figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _rollout_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _run(p, x0, steps, pad_x=0, pad_out=0, x0_dev=None):
    """umlh.rollout_rows into a NaN buffer one row longer (and pad_out columns wider) than the result -> numpy [n, steps + 1, D]."""
    import umlh
    n, D = x0.shape
    if x0_dev is None:
        wide = torch.full((n, D + pad_x), float("nan"), device=DEV)
        wide[:, :D] = _dev(x0)
        x0_dev = wide[:, :D]
    buf = torch.full((n + 1, steps + 1, D + pad_out), float("nan"), device=DEV)
    out = buf[:n, :, :D]
    got = umlh.rollout_rows(x0_dev, _dev(p["w_in"]), _dev(p["b_in"]), _dev(p["conv"]), _dev(p["pos0"]),
                            [_dev(t) for layer in p["layers"] for t in layer], p["eps"], _dev(p["w_out"]), _dev(p["b_out"]), steps, out=out)
    assert got is out
    b = buf.cpu().numpy()
    assert np.isnan(b[n]).all() and np.isnan(b[:, :, D:]).all()                 # nothing written past the rows or the columns
    return b[:n, :, :D]


_REF = {}


def _case(name):
    """(params, x0, steps, float64 reference): computed once per case and shared."""
    if name not in _REF:
        p, x0, steps = R.make_case(name)
        _REF[name] = (p, x0, steps, R.rollout(p, x0, steps))
    return _REF[name]


STRIDED = {"z40_d35": (5, 3), "z300_d300": (4, 4), "z10_d5_long": (0, 1)}       # name -> (x0 row padding, out row padding)


@pytest.mark.parametrize("name", list(R.CASES))
def test_rollout_against_float64(name):
    p, x0, steps, ref = _case(name)
    pad_x, pad_out = STRIDED.get(name, (0, 0))
    got = _run(p, x0, steps, pad_x, pad_out)
    assert got.shape == ref.shape and np.array_equal(got[:, 0], x0)             # the seed row is a copy
    if steps:
        err = R.step_errors(got, ref)
        print(f"{name}: worst step error {err.max():.3e} at step {1 + int(err.argmax())}, step 1 {err[0]:.3e}, bound {R.BOUNDS[name]:.3e}")
        assert np.isfinite(got).all() and err.max() <= R.BOUNDS[name]


@pytest.mark.parametrize("name", ["z10_d5_long", "z300_d300", "z40_d371"])
def test_row_is_bitwise_independent_of_the_batch(name):
    p, x0, steps, _ = _case(name)
    full = _run(p, x0, steps)
    r = min(7, x0.shape[0] - 1)
    alone = _run(p, x0[r:r + 1], steps)
    assert np.array_equal(alone[0].view(np.int32), full[r].view(np.int32))
    last = _run(p, x0[-1:], steps)                                              # the only row of the last workgroup
    assert np.array_equal(last[0].view(np.int32), full[-1].view(np.int32))


def test_bitwise_equal_across_calls_and_streams():
    p, x0, steps, _ = _case("z40_d35")
    a = _run(p, x0, steps)
    b = _run(p, x0, steps)
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c = _run(p, x0, steps)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a.view(np.int32), c.view(np.int32))


# ---- the reference's own outputs, through multibench.train.rollout ----
@pytest.fixture(scope="module")
def golden():
    return load_golden("rollout")


def _golden_model(g, with_pos):
    from multibench.models import Linear, Transformer, UML
    z, dx, dy = 10, g["case1::x"].shape[2], g["case1::y"].shape[2]
    m = UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=int(g["n_layers"]), conv1d=True, out_last=False,
                                                       pos_embd=with_pos, pos_learnable=with_pos, max_len=128),
            [Linear(z, dx), Linear(z, dy)], modality="xy")
    m.load_state_dict({k[3:]: torch.as_tensor(g[k]) for k in g.files if k.startswith("w::") and (with_pos or "pos_embedding" not in k)})
    return m.to(DEV)


@pytest.mark.parametrize("tag,with_pos", [("case1", False), ("case2", True)])
def test_train_rollout_equals_the_reference(golden, tag, with_pos):
    from multibench.train import rollout
    m = _golden_model(golden, with_pos).train()
    x, y = _dev(golden[f"{tag}::x"]), _dev(golden[f"{tag}::y"])
    steps = int(golden[f"{tag}::steps"])
    px, py = rollout(m, x, y, steps=steps)
    assert not m.training                                                       # eval mode, and left there, as the reference does
    for name, seq, got in (("x", x, px), ("y", y, py)):
        want = golden[f"{tag}::pred_{name}"]
        T0 = seq.shape[1]
        got = got.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got[:, :T0], seq.cpu().numpy())
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{tag} {name}: against the reference {err:.3e} (bound {float(golden['bound']):.3e})")
        assert err <= float(golden["bound"])
    only_x, none_y = rollout(m, x, None, steps=steps)
    none_x, only_y = rollout(m, None, y, steps=steps)
    assert none_y is None and none_x is None and torch.equal(only_x, px) and torch.equal(only_y, py)


def test_train_rollout_against_the_step_by_step_modules(golden):
    """The same loop through the existing xproj_in / encoder / decoders modules at T = 1 (about 40 launches per step): both are
    fp32 evaluations within the fixture's bound of the float64 closed form, so they agree within the sum of the two bounds."""
    from multibench.train import rollout
    m = _golden_model(golden, True).eval()
    x = _dev(golden["case2::x"])
    steps = 8
    got, _ = rollout(m, x, None, steps=steps)
    with torch.no_grad():
        frames, cur = [x], x
        for _ in range(steps):
            cur = m.decoders[0](m.encoder(m.xproj_in(cur[:, -1, :].unsqueeze(1))))
            frames.append(cur)
        want = torch.cat(frames, dim=1)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"one launch against the module loop: {err:.3e} (2 x bound {2 * float(golden['bound']):.3e})")
    assert got.shape == want.shape and err <= 2 * float(golden["bound"])


def test_train_rollout_rejects_out_last_encoders(golden):
    from multibench.train import rollout
    m = _golden_model(golden, True)
    m.encoder.out_last = True
    with pytest.raises(ValueError, match="out_last"):
        rollout(m, _dev(golden["case2::x"]), None, steps=2)


# ---- spectrum ----
def _spectrum_check(x_dev, x_host):
    import umlh
    got = umlh.seq_spectrum(x_dev)
    want = R.spectrum(x_host)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == want.shape == (x_host.shape[1] // 2 + 1,)
    g = got.cpu().numpy()
    err = np.abs(g - want).max() / np.abs(want).max()
    print(f"spectrum {x_host.shape}: {err:.3e}")
    assert err <= 1e-12
    assert torch.equal(got, umlh.seq_spectrum(x_dev))                            # bitwise, call after call
    return got


@pytest.mark.parametrize("d", [1, 35, 300])
@pytest.mark.parametrize("T", [1, 2, 7, 50, 128])
def test_spectrum_against_numpy_float64(T, d):
    B = 33 if d == 35 else 5
    x = np.random.default_rng(1000 * T + d).standard_normal((B, T, d)).astype(np.float32)
    _spectrum_check(_dev(x), x)


def test_spectrum_reads_views_in_place():
    g = np.random.default_rng(3)
    wide = g.standard_normal((6, 9, 40)).astype(np.float32)
    _spectrum_check(_dev(wide)[:, :, 3:38], np.ascontiguousarray(wide[:, :, 3:38]))      # a column block of a wider tensor
    tb = g.standard_normal((9, 6, 35)).astype(np.float32)                                 # a [T, B, d] block
    _spectrum_check(_dev(tb).transpose(0, 1), np.ascontiguousarray(tb.transpose(1, 0, 2)))
    s = torch.cuda.Stream(device=DEV)
    x = _dev(wide)
    a = _spectrum_check(x, wide)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        b = _spectrum_check(x, wide)
    s.synchronize()
    assert torch.equal(a, b)


def test_spectral_bias_equals_the_reference_spectra(golden):
    from multibench.train import analyze_spectral_bias, spectral_bias
    for name in ("x", "y"):
        gt, pred = _dev(golden[f"spec::{name}_block"]), _dev(golden[f"case2::pred_{name}"])
        mg, mp = spectral_bias(gt, pred)
        for got, key in ((mg, f"spec::{name}_gt"), (mp, f"spec::{name}_pred")):
            want = golden[key]
            err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
            print(f"{key}: {err:.3e} (bound {float(golden['bound_spec']):.3e})")
            assert err <= float(golden["bound_spec"])
    import os
    cwd = os.getcwd()
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:                                   # the figure, if matplotlib is there, goes to cwd
        os.chdir(tmp)
        try:
            ag, ap = analyze_spectral_bias(gt, pred, 0.25, 3, modality_name="text", postfix="_t")
        finally:
            os.chdir(cwd)
    assert torch.equal(ag, mg) and torch.equal(ap, mp)


# ---- train(rollout_spectra=True) ----
class _ListLoader(list):
    """A list of batches in the reference's layout; deep-copied and re-iterated like a DataLoader."""


def _e2e_model(name):
    from multibench.models import Linear, Transformer, UML
    g = load_golden(name)
    z, dx, dy, B, T, pe, pl = (int(v) for v in g["cfg"])
    m = UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=5, conv1d=True, out_last=False,
                                                       pos_embd=bool(pe), pos_learnable=bool(pl), max_len=128),
            [Linear(z, dx), Linear(z, dy)], modality="xy")
    m.load_state_dict({k[4:]: torch.as_tensor(g[k]) for k in g.files if k.startswith("sd::")})
    return m.to(DEV)


def test_train_rollout_spectra():
    from multibench.train import rollout, spectral_bias, train
    g = load_golden("probe_e2e_humor")
    bs, cfg = int(g["batch_size"]), {"freq": 2}
    for t in ("train", "val", "test"):
        x, y, lx, ly, lab = (torch.from_numpy(g[f"{k}_{t}"]) for k in ("x", "y", "lx", "ly", "labels"))
        cfg[t] = [([x[s:s + bs], None, y[s:s + bs]], [lx[s:s + bs], None, ly[s:s + bs]], torch.arange(s, min(s + bs, len(x))),
                   lab[s:s + bs].reshape(-1, 1)) for s in range(0, len(x), bs)]
    x, y, lx, lab = (torch.from_numpy(g[f"{k}_train"]) for k in ("x", "y", "lx", "labels"))
    loader = _ListLoader(([x[s:s + 16], None, y[s:s + 16]], [lx[s:s + 16], None, lx[s:s + 16].roll(1)], torch.arange(s, s + 16),
                          lab[s:s + 16].reshape(-1, 1)) for s in range(0, 48, 16))
    res = {}
    for flag in (True, False):
        torch.manual_seed(0)
        model = _e2e_model(str(g["model"]))
        model.eval()
        model.train = lambda *a, **k: model                                      # stay in eval mode (dropout off): runs retrace each other
        res[flag] = train(model, "xy", loader, loader, torch.optim.SGD(model.parameters(), lr=0.0), num_epoch=1, step_k=-1,
                          ds_name="humor", eval_config=cfg, device=DEV, capture_embeddings_during_training=True, rollout_spectra=flag)
    on, off = res[True], res[False]
    for k in ("loss_x", "loss_y", "loss"):
        assert on[k] == off[k] and len(on[k]) == 3, k
    assert set(on) == set(off) | {"spectra"}
    assert [(e, i) for e, i, _ in on["spectra"]] == [(e, i) for e, i, _ in on["eval"] if i is not None] == [(0, 0), (0, 2)]
    xb, yb = loader[0][0][0].float().to(DEV), loader[0][0][2].float().to(DEV)    # the first batch of the fixed sample
    px, _ = rollout(model, xb[:, :1], None, steps=xb.shape[1] - 1)
    _, py = rollout(model, None, yb[:, :1], steps=yb.shape[1] - 1)
    want = dict(zip(("x_gt", "x_pred"), spectral_bias(xb, px)))
    want.update(zip(("y_gt", "y_pred"), spectral_bias(yb, py)))
    for _, _, sp in on["spectra"]:                                              # lr 0: the model never moved
        assert set(sp) == set(want)
        for k in want:
            assert sp[k] == want[k].cpu().tolist() and len(sp[k]) == (xb if k[0] == 'x' else yb).shape[1] // 2 + 1, k
