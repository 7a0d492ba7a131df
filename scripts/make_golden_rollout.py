#!/usr/bin/env python3
"""Golden vectors for the rollout and the spectral-bias spectra by RUNNING THE REFERENCE's MultiBench/train.py rollout() and
analyze_spectral_bias() on the CPU.  Build machine only: needs the reference checkout (REFERENCE_ROOT, default ../reference next
to the repo).  Writes tests/golden/rollout.npz (seeds, outputs, spectra, bounds) and rollout.part1.npz / rollout.part2.npz (the
weights), data only, allow_pickle=False, every file under 1 MiB.

The reference's modules import as they are once the packages this machine lacks are stubbed (as in make_golden_stepstats.py).
analyze_spectral_bias returns nothing and only draws: ``plt`` is replaced by a recorder whose ``plot`` keeps its arguments,
which is the only way to the two magnitude vectors; ``os.makedirs`` is a no-op while it runs, so nothing is written.

One weight set: the reference UML with Z 10, nhead 5, 5 layers, widths 5 and 7, conv1d, learnable positions, every parameter
perturbed (no zero bias, no unit LayerNorm gain); the same state dict minus the table goes into a pos_embd=False model.
  case 1: B 4, T0 1, steps 5, no positions.     case 2: B 3, T0 3 (seed = last frame), steps 8, learnable positions.
The spectra are those of case 2: a random block of the rollout's shape as ground truth against the rollout, per modality.
``bound`` / ``bound_spec`` = 8 x the largest relative difference (max|a - b| / max|b|) between the reference's fp32 values and the
float64 restatement of tests/_rollout_ref.py, rounded up to a power of two."""
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
import _rollout_ref as R   # noqa: E402
REF = os.path.join(os.environ.get("REFERENCE_ROOT", os.path.join(os.path.dirname(ROOT), "reference")), "MultiBench")
OUT = os.path.join(ROOT, "tests", "golden", "rollout")


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

PLOTTED = []


class _Plot:
    """pyplot, recording: plot(freqs, magnitudes, ...) keeps the magnitudes; everything else is a no-op."""

    def plot(self, x, y, *a, **k):
        PLOTTED.append(np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y))

    def __getattr__(self, name):
        return lambda *a, **k: None


RT.plt = _Plot()
RT.os = types.SimpleNamespace(makedirs=lambda *a, **k: None)

Z, DX, DY, LAYERS = 10, 5, 7, 5


def model(pos):
    with contextlib.redirect_stdout(io.StringIO()):
        return RM.UML(RM.Linear(DX, Z), RM.Linear(DY, Z),
                      RM.Transformer(Z, Z, nhead=5, num_layers=LAYERS, conv1d=True, out_last=False, pos_embd=pos, pos_learnable=pos,
                                     max_len=128),
                      [RM.Linear(Z, DX), RM.Linear(Z, DY)], modality="xy")


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


if __name__ == "__main__":
    torch.set_num_threads(4)
    torch.manual_seed(31)
    rng = np.random.default_rng(31)
    m2 = model(True)
    with torch.no_grad():
        for name, t in m2.named_parameters():
            t.add_(torch.from_numpy((0.1 * rng.standard_normal(tuple(t.shape))).astype(np.float32)))
    sd = {k: v.detach().numpy().copy() for k, v in m2.state_dict().items() if v.dtype == torch.float32}
    m1 = model(False)
    m1.load_state_dict({k: v for k, v in m2.state_dict().items() if "pos_embedding" not in k})
    eps = float(m2.encoder.transformer.layers[0].norm1.eps)
    rec, worst, worst_spec = {"eps": np.float64(eps), "n_layers": np.int64(LAYERS)}, 0.0, 0.0
    for tag, m, with_pos, B, T0, steps in (("case1", m1, False, 4, 1, 5), ("case2", m2, True, 3, 3, 8)):
        x = torch.from_numpy(rng.standard_normal((B, T0, DX)).astype(np.float32))
        y = torch.from_numpy(rng.standard_normal((B, T0, DY)).astype(np.float32))
        px, py = RT.rollout(m, x, y, steps=steps)
        assert px.shape == (B, T0 + steps, DX) and py.shape == (B, T0 + steps, DY) and not m.training
        rec.update({f"{tag}::x": x.numpy(), f"{tag}::y": y.numpy(), f"{tag}::pred_x": px.numpy(), f"{tag}::pred_y": py.numpy(),
                    f"{tag}::steps": np.int64(steps)})
        for side, seq, pred in ((True, x, px), (False, y, py)):
            ref = R.rollout(R.params_from_state(sd, side, with_pos, LAYERS, eps), seq.numpy()[:, -1], steps)
            e = rel(pred.numpy()[:, T0 - 1:], ref)
            worst = max(worst, e)
            print(f"  {tag} {'x' if side else 'y'}: reference fp32 against the float64 closed form {e:.3e}")
        if tag == "case2":
            for side, pred, d in (("x", px, DX), ("y", py, DY)):
                gt = torch.from_numpy(rng.standard_normal((B, T0 + steps, d)).astype(np.float32))
                del PLOTTED[:]
                RT.analyze_spectral_bias(gt, pred, 0.5, 0, modality_name=side)
                assert len(PLOTTED) == 2 and PLOTTED[0].shape == ((T0 + steps) // 2 + 1,)
                rec.update({f"spec::{side}_block": gt.numpy(), f"spec::{side}_gt": PLOTTED[0], f"spec::{side}_pred": PLOTTED[1]})
                for got, blk in ((PLOTTED[0], gt.numpy()), (PLOTTED[1], pred.numpy())):
                    e = rel(got, R.spectrum(blk))
                    worst_spec = max(worst_spec, e)
                    print(f"  spectrum {side}: reference fp32 against numpy float64 {e:.3e}")
    bound = 2.0 ** math.ceil(math.log2(8 * worst))
    bound_spec = 2.0 ** math.ceil(math.log2(8 * worst_spec))
    print(f"rollout: largest relative difference {worst:.3e}; bound = 2^{int(math.log2(bound))}")
    print(f"spectra: largest relative difference {worst_spec:.3e}; bound_spec = 2^{int(math.log2(bound_spec))}")
    rec.update(bound=np.float64(bound), bound_spec=np.float64(bound_spec))
    keys = sorted(sd)
    parts = [rec, {f"w::{k}": sd[k] for k in keys if ".layers.0." in k or ".layers.1." in k or ".layers.2." in k},
             {f"w::{k}": sd[k] for k in keys if not (".layers.0." in k or ".layers.1." in k or ".layers.2." in k)}]
    for i, part in enumerate(parts):
        path = OUT + (".npz" if i == 0 else f".part{i}.npz")
        np.savez_compressed(path, **{k: np.asarray(v) for k, v in part.items()})
        with np.load(path, allow_pickle=False) as z:
            assert set(z.files) == set(part)
        assert os.path.getsize(path) < 1 << 20, path
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
