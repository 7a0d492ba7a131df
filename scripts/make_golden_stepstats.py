#!/usr/bin/env python3
"""Golden vectors for the per-step logged statistics by RUNNING THE REFERENCE's MultiBench/train.py train() on the CPU.
Build machine only: needs the reference checkout (REFERENCE_ROOT, default ../reference next to the repo) and sklearn.  Writes
tests/golden/step_stats.npz (data only, allow_pickle=False, a few KB).

The reference's modules import as they are once the packages this machine lacks are stubbed (as in make_golden_probe.py);
``torch.Tensor.cuda`` is the identity while train() runs, ``wandb.log`` records what it is given, and a forward hook on the
reference UML keeps each TRAINING step's x, y, lengths and y_recon (the evaluations and the capture run the model in eval
mode and are not kept).  The reference loop reads the embedding capture's sample on every step (train.py:386), so it runs with
capture_embeddings_during_training=True and a small eval_config; the loaders are lists with a ``batch_size`` attribute.

Two runs, MSE critic and infoNCE_loss=True: 3 steps each, B 4, T 6, widths 5 and 7, zdim 10; lengths mix T, 2..T-1 and 1; rows
past a length are zero, as the reference loaders leave them.  ``bound`` = 8 x the largest relative difference between the
logged fp32 values and tests/_stepstats_ref.step_stats on the recorded tensors, rounded up to a power of two."""
import contextlib
import importlib.machinery
import io
import math
import os
import sys
import types
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _stepstats_ref as R   # noqa: E402
REF = os.path.join(os.environ.get("REFERENCE_ROOT", os.path.join(os.path.dirname(ROOT), "reference")), "MultiBench")
OUT = os.path.join(ROOT, "tests", "golden", "step_stats.npz")
LOGGED = []


def _stub(name, **attrs):
    if name in sys.modules:
        return
    try:
        __import__(name)
        return
    except Exception:
        pass
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__dict__.update(attrs)
    sys.modules[name] = m


class _Bar:
    def __init__(self, *a, **k):
        pass

    def update(self, *a):
        pass

    def set_postfix(self, *a, **k):
        pass

    def close(self):
        pass


_stub("torchvision", transforms=types.ModuleType("torchvision.transforms"))
_stub("torchvision.transforms")
_stub("wandb", log=None)
_stub("tqdm", tqdm=_Bar)
_stub("torchaudio", functional=types.ModuleType("torchaudio.functional"), __path__=[])
_stub("torchaudio.functional")
_stub("matplotlib", pyplot=types.ModuleType("matplotlib.pyplot"))
_stub("matplotlib.pyplot")
sys.path.insert(0, REF)
with contextlib.redirect_stdout(io.StringIO()):
    import models as RM       # noqa: E402
    import train as RT        # noqa: E402
RT.wandb = types.SimpleNamespace(log=lambda d, *a, **k: LOGGED.append(dict(d)))
RT.tqdm = _Bar

B, T, DX, DY, Z, STEPS = 4, 6, 5, 7, 10, 3
LENS_X = [[6, 3, 1, 5], [2, 6, 4, 1], [5, 1, 6, 2]]
LENS_Y = [[1, 6, 5, 3], [4, 2, 1, 6], [6, 5, 2, 1]]          # each batch a permutation of the x lengths: equal totals of valid rows


class Loader(list):
    batch_size = B


def padded(rng, lens, d):
    a = rng.standard_normal((len(lens), T, d)).astype(np.float32)
    for i, n in enumerate(lens):
        a[i, n:] = 0.0
    return torch.from_numpy(a)


def batches(rng, n_batches, lens_x, lens_y):
    out = Loader()
    for i in range(n_batches):
        lab = torch.tensor([1, -1, 1, -1]).roll(i).reshape(-1, 1)
        out.append(([padded(rng, lens_x[i % 3], DX), None, padded(rng, lens_y[i % 3], DY)],
                    [torch.tensor(lens_x[i % 3]), None, torch.tensor(lens_y[i % 3])], torch.arange(B * i, B * (i + 1)), lab))
    return out


def run(tag, info_nce, seed):
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = RM.UML(RM.Linear(DX, Z), RM.Linear(DY, Z),
                   RM.Transformer(Z, Z, nhead=5, num_layers=2, conv1d=True, out_last=False, pos_embd=True, pos_learnable=False, max_len=128),
                   [RM.Linear(Z, DX), RM.Linear(Z, DY)], modality="xy", infoNCE_loss=info_nce)
    loader = batches(rng, STEPS, LENS_X, LENS_Y)
    cfg = {"freq": STEPS, "train": batches(rng, 3, LENS_X, LENS_Y), "val": batches(rng, 2, LENS_X, LENS_Y),
           "test": batches(rng, 2, LENS_X, LENS_Y)}
    steps = []

    def keep(mod, args, kwargs, out):
        if mod.training:
            x, y, lx, ly = args
            steps.append((x.detach().clone(), y.detach().clone(), lx.clone(), ly.clone(), out["y_recon"].detach().clone()))
    hook = m.register_forward_hook(keep, with_kwargs=True)
    del LOGGED[:]
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            RT.train(m, "xy", loader, loader, torch.optim.Adam(m.parameters(), lr=1e-3), modalities=[0, 2], num_epoch=1, step_k=-1,
                     ds_name="humor", eval_config=cfg, capture_embeddings_during_training=True)
    finally:
        torch.Tensor.cuda = cuda
        hook.remove()
    logged = [d for d in LOGGED if "train/trivial_loss_x" in d]
    assert len(steps) == STEPS and len(logged) == STEPS, (len(steps), len(logged))
    rec, worst = {}, 0.0
    for j, k in enumerate(("x", "y", "lx", "ly", "y_recon")):
        rec[f"{tag}::{k}"] = np.stack([st[j].numpy() for st in steps])
    rec[f"{tag}::logged"] = np.array([[log[k] for k in R.LOGGED_KEYS] for log in logged], dtype=np.float64)      # [step, key]
    for s, ((x, y, lx, ly, yr), log) in enumerate(zip(steps, logged)):
        sx, sy = R.step_stats(x.numpy(), lx.numpy()), R.step_stats(y.numpy(), ly.numpy(), yr.numpy())
        for name, want, got in (("trivial_loss_x", log["train/trivial_loss_x"], sx[0]), ("trivial_loss_y", log["train/trivial_loss_y"], sy[0]),
                                ("recon_y_loss", log["train/recon_y_loss"], sy[2])):
            rel = abs(got - want) / abs(want)
            worst = max(worst, rel)
            print(f"  {tag} step {s} {name}: logged {want:.9g} float64 {got:.12g} rel {rel:.3e}")
        t32, r32 = R.reference_fp32(x.numpy(), lx.numpy())[0], R.reference_fp32(y.numpy(), ly.numpy(), yr.numpy())
        print(f"  {tag} step {s} fp32 numpy restatement: trivial_x {t32:.9g} trivial_y {r32[0]:.9g} recon_y {r32[1]:.9g}; "
              f"loss_y {log['train/loss_y']:.9g}")
    return rec, worst


if __name__ == "__main__":
    torch.set_num_threads(4)
    rec, worst = {}, 0.0
    for tag, nce, seed in (("mse", False, 21), ("nce", True, 22)):
        r, w = run(tag, nce, seed)
        rec.update(r)
        worst = max(worst, w)
    bound = 2.0 ** math.ceil(math.log2(8 * worst))
    print(f"largest relative difference {worst:.3e}; bound = {bound:.3e} = 2^{int(math.log2(bound))}")
    rec.update(bound=np.float64(bound))
    np.savez_compressed(OUT, **{k: np.asarray(v) for k, v in rec.items()})
    with np.load(OUT, allow_pickle=False) as z:
        assert set(z.files) == set(rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")
