"""GPU: the fused training path of the Gaussian toy (gaussian.fused, gaussian.train.train_model_steps_fused) replays the
reference's own six steps from the golden file with the checks and tolerances of tests/test_gaussian_gpu.py, and tracks the
composed path (train_model_steps over the LinearFn / _DecoderNextStepMSE nodes) step for step from the same initial weights over
the same batches.  The first-step gradients of the golden file are covered by the sgd probe of tests/test_gauss_kernels_gpu.py."""
import numpy as np
import pytest
import torch

import _gauss_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_training_steps_replay_reference():
    from gaussian.train import build_run, train_model_steps_fused
    g = load_golden("gaussian_toy")
    data = {"x": torch.from_numpy(g["data_x"]), "y": torch.from_numpy(g["data_y"])}
    ds, gen, model, opt = build_run(data, data, mode="xy", train_num_samples=600, batch_size=128, seed=0, device=DEV, fused=True)
    for k, v in model.state_dict().items():                       # same init as the reference under make_reproducible(0)
        np.testing.assert_array_equal(v.cpu().numpy(), g["init/" + k])
    vx, vy = torch.from_numpy(g["val_x"]).to(DEV), torch.from_numpy(g["val_y"]).to(DEV)
    log = train_model_steps_fused(model, ds, opt, 6, vx, vy, DEV, batch_size=128, generator=gen, mode="xy", alpha_x=1.0, alpha_y=0.5,
                                  eval_every=6)
    np.testing.assert_allclose(log["loss_x"], g["loss_x"], rtol=2e-5)
    np.testing.assert_allclose(log["loss_y"], g["loss_y"], rtol=2e-5)
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), g["final/" + k], atol=2e-5, rtol=1e-4, err_msg=k)
    assert abs(log["val_loss_x"][-1] - float(g["val_loss_x"])) < 2e-5 * float(g["val_loss_x"])
    assert abs(log["val_loss_y"][-1] - float(g["val_loss_y"])) < 2e-5 * float(g["val_loss_y"])
    import umlh
    _, _, _, ex, ey = umlh.ae_forward([p.data for p in model.parameters()], vx, vy, losses=False, recon=False)
    np.testing.assert_allclose(ex.cpu().numpy(), g["emb_x"], atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(ey.cpu().numpy(), g["emb_y"], atol=2e-4, rtol=1e-4)
    assert opt.step_count == 6
    # the optimizer and the model are still the composed path's: a plain backward + optimizer.step() works on the same state
    before = [p.detach().clone() for p in model.parameters()]
    opt.zero_grad()
    lx, ly, _, _ = model(vx[:32], vy[:32])
    (lx + ly).backward()
    opt.step()
    torch.cuda.synchronize()
    assert opt.step_count == 7
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert all(torch.isfinite(p).all() for p in model.parameters())


def _data():
    from gaussian.data import generate_data
    cfg = {"seed": 1, "num_samples": 640, "dim_c": 10, "dim_x": 5, "dim_y": 5, "dim_obs": 50, "noise_std": 0.09,
           "attenuate_x": True, "attenuation": 0.05, "shared_latent_distribution_type": "gaussian"}
    return generate_data(cfg)


@pytest.mark.parametrize("mode,alpha_y", [("xy", 0.5), ("x", 1.0)])
def test_fused_loop_tracks_the_composed_loop(mode, alpha_y):
    from gaussian.train import build_run, train_model_steps, train_model_steps_fused
    d = _data()
    kw = dict(mode=mode, train_num_samples=512, batch_size=128, seed=0, lr=1e-3, device=DEV)
    vx, vy = d["x"][512:640].to(DEV), d["y"][512:640].to(DEV)
    loader, model_c, opt_c = build_run(d, d, **kw)
    log_c = train_model_steps(model_c, loader, opt_c, 12, vx, vy, DEV, mode=mode, alpha_x=1.0, alpha_y=alpha_y, eval_every=4, alignment=True)
    ds, gen, model_f, opt_f = build_run(d, d, fused=True, **kw)
    log_f = train_model_steps_fused(model_f, ds, opt_f, 12, vx, vy, DEV, batch_size=128, generator=gen, mode=mode, alpha_x=1.0,
                                    alpha_y=alpha_y, eval_every=4, alignment=True)
    assert list(log_f) == list(log_c)
    assert torch.equal(gen.get_state(), loader.generator.get_state())          # the generator ends where the loader's does
    assert {k: len(v) for k, v in log_f.items()} == {k: len(v) for k, v in log_c.items()}
    assert len(log_f["loss"]) == 12 and len(log_f["val_loss_x"]) == 3 and len(log_f["val_cka"]) == 3 and len(log_f["val_mknn"]) == 3
    # the losses of the two loops within the calibrated fp32 bound of each other (tests/_gauss_ref.py: LOSS_BOUNDS)
    worst = {}
    for k in ("loss_x", "loss_y", "loss", "val_loss_x", "val_loss_y"):
        worst[k] = max(abs(a - b) / abs(b) for a, b in zip(log_f[k], log_c[k]))
    print("\nGAUSS_FUSED_VS_COMPOSED", mode, {k: round(float(np.log2(v)), 2) if v > 0 else None for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= R.LOSS_BOUNDS["loss" if k == "loss" else k[-6:]], (k, v)
    assert all(np.isfinite(v) for v in log_f["val_cka"] + log_f["val_mknn"])
    if mode == "x":
        assert log_f["loss"] == log_f["loss_x"]
    assert opt_f.step_count == 12
    opt_f.zero_grad()
    lx, ly, _, _ = model_f(vx, vy)
    (lx + ly).backward()
    opt_f.step()
    torch.cuda.synchronize()
    assert opt_f.step_count == 13 and all(torch.isfinite(p).all() for p in model_f.parameters())
