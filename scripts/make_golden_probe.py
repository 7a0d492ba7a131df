#!/usr/bin/env python3
"""Golden vectors for the linear probes by RUNNING THE REFERENCE's MultiBench/train.py (evaluate_raw_data and evaluate) and
models.py on the CPU.  Build machine only: needs the reference checkout (REFERENCE_ROOT, default ../reference next to the repo) and
sklearn.  Writes tests/golden/probe_*.npz (data only, allow_pickle=False, every file under 1 MiB).

The reference's modules import as they are once the packages this machine lacks are stubbed (torchvision, wandb, tqdm,
torchaudio, matplotlib: none is used by the two functions) and ``torch.Tensor.cuda`` is the identity while ``evaluate``
runs.  sklearn's estimators are observed, not replaced: recording subclasses of LogisticRegression and StandardScaler keep
the arrays they were fitted on and the fitted estimators, and ``np.random.permutation`` is wrapped to keep the row orders
``evaluate`` drew, so that its pooled embeddings can be read back unshuffled.

Probe cases: the features enter ``evaluate_raw_data`` as sequences of length 1 (their mean over time is the feature row),
so its x probe is sklearn fitted on exactly these rows; 'test' and 'val' are two held-out splits.  Seeds are kept only if the
conditions of tests/test_probe_*.py hold for the reference alone; what was found is printed."""
import contextlib
import importlib.machinery
import io
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
import _probe_ref as R   # noqa: E402
REF = os.path.join(os.environ.get("REFERENCE_ROOT", os.path.join(os.path.dirname(ROOT), "reference")), "MultiBench")
OUT = os.path.join(ROOT, "tests", "golden")


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


_stub("torchvision", transforms=types.ModuleType("torchvision.transforms"))
_stub("torchvision.transforms")
_stub("wandb", log=lambda *a, **k: None)
_stub("tqdm", tqdm=lambda *a, **k: None)
_stub("torchaudio", functional=types.ModuleType("torchaudio.functional"), __path__=[])
_stub("torchaudio.functional")
_stub("matplotlib", pyplot=types.ModuleType("matplotlib.pyplot"))
_stub("matplotlib.pyplot")
sys.path.insert(0, REF)
with contextlib.redirect_stdout(io.StringIO()):
    import models as RM       # noqa: E402
    import train as RT        # noqa: E402

FITS, SCALED, PERMS = [], [], []


class RecLR(RT.LogisticRegression):
    def fit(self, X, y, sample_weight=None):
        out = super().fit(X, y, sample_weight)
        FITS.append((self, np.array(X), np.array(y)))
        return out


class RecScaler(RT.StandardScaler):
    def fit(self, X, y=None, sample_weight=None):
        SCALED.append(np.array(X))
        return super().fit(X, y, sample_weight)


RT.LogisticRegression, RT.StandardScaler = RecLR, RecScaler


@contextlib.contextmanager
def observed():
    del FITS[:], SCALED[:], PERMS[:]
    cuda, perm = torch.Tensor.cuda, np.random.permutation

    def keep(n):
        PERMS.append(perm(n))
        return PERMS[-1]
    torch.Tensor.cuda = lambda self, *a, **k: self
    np.random.permutation = keep
    try:
        yield
    finally:
        torch.Tensor.cuda, np.random.permutation = cuda, perm


def batches(x, y, labels, lx=None, ly=None, bs=32):
    """The _process_1 batch layout evaluate reads: data_[0][0], data_[0][2], data_[1][0], data_[1][2], data_[3]."""
    out = []
    for s in range(0, len(x), bs):
        e = min(len(x), s + bs)
        tx = torch.from_numpy(x[s:e])
        ty = torch.from_numpy(y[s:e])
        llx = torch.from_numpy(lx[s:e]) if lx is not None else torch.full((e - s,), x.shape[1], dtype=torch.int64)
        lly = torch.from_numpy(ly[s:e]) if ly is not None else torch.full((e - s,), y.shape[1], dtype=torch.int64)
        out.append(([tx, None, ty], [llx, None, lly], torch.arange(s, e), torch.from_numpy(labels[s:e]).reshape(-1, 1)))
    return out


def raw_label(y01, ds_name, rng):
    """Regression-style targets whose mosi_label / sarcasm_label is y01."""
    if ds_name in ("mosi", "mosei"):
        mag = rng.uniform(0.2, 3.0, len(y01)).astype(np.float32)
        out = np.where(y01 == 1, mag, -mag).astype(np.float32)
        pos = np.flatnonzero(y01 == 1)
        out[pos[:2]] = [0.0, -0.0]                       # >= 0 counts as positive, and so does -0.0
        return out
    return np.where(y01 == 1, 1, -1).astype(np.int64)


def probe_case(tag, ds_name, n, d, nh, scale_hi, shift, const_col, noise, seed0):
    kind = R.LIBLINEAR if ds_name == "mosi" else R.LBFGS
    for seed in range(seed0, seed0 + 50):
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal((n + 2 * nh, d)) * rng.uniform(0.3, scale_hi, d) + shift * rng.standard_normal(d)).astype(np.float32)
        if const_col is not None:
            x[:, const_col] = 2.5
        wt = rng.standard_normal(d) / np.sqrt(d)
        y01 = (((x - x.mean(0)) / x.std(0).clip(1e-3)) @ wt + noise * rng.standard_normal(len(x)) > 0).astype(np.int64)
        lab = raw_label(y01, ds_name, rng)
        other = rng.standard_normal((len(x), 1, 2)).astype(np.float32)
        sl = {"train": slice(0, n), "val": slice(n, n + nh), "test": slice(n + nh, n + 2 * nh)}
        cfg = {k: batches(x[s][:, None, :], other[s], lab[s]) for k, s in sl.items()}
        with observed():
            res = RT.evaluate_raw_data(cfg, ds_name)
        clf, xfit, yfit = FITS[0]
        assert np.array_equal(yfit, y01[:n])
        stats = R.column_stats(x[:n]) if kind == R.LIBLINEAR else None
        if stats is not None:
            assert np.allclose(SCALED[0], x[:n]) and np.allclose(xfit, R.standardise(x[:n], stats), atol=1e-9)
        else:
            assert np.array_equal(xfit, x[:n])
        w_ref = np.concatenate([clf.coef_.reshape(-1), clf.intercept_.reshape(-1)])
        w_star, it, mg = R.fit(x[:n], y01[:n], kind, stats=stats)
        ok = mg <= 1e-10
        flips, rec = {}, {}
        for k in ("val", "test"):
            xh, yh = x[sl[k]], y01[sl[k]]
            p_ref = (R.decision(w_ref, xh, stats) > 0)
            p_opt = (R.decision(w_star, xh, stats) > 0)
            flips[k] = int((p_ref != p_opt).sum())
            sk = res[f"{k}/score_x_raw"]
            assert abs(sk - np.mean(p_ref == yh)) < 1e-12, (sk, np.mean(p_ref == yh))
            ok &= flips[k] <= 0.01 * nh and bool(R.decidable(w_star, xh, stats).all())
            rec[f"x_{k}"], rec[f"y_{k}"], rec[f"score_ref_{k}"], rec[f"ref_flips_{k}"] = xh, yh, sk, flips[k]
        dref = np.abs(w_ref - w_star).max()
        print(f"  {tag} seed {seed}: sklearn n_iter={int(np.max(clf.n_iter_))} max|w_ref-w*|={dref:.2e} newton it={it} max|g|={mg:.1e} "
              f"ref_flips={flips} scores={ {k: round(float(v), 4) for k, v in res.items() if 'score_x' in k} } -> {'kept' if ok else 'dropped'}")
        if not ok:
            continue
        rec.update(x_train=x[:n], y_train=y01[:n], labels_raw_train=lab[:n], kind=np.int64(kind), ds_name=np.array(ds_name),
                   w_ref=w_ref, w_star=w_star, n_iter_ref=np.int64(np.max(clf.n_iter_)), delta_ref=dref, seed=np.int64(seed))
        if stats is not None:
            rec.update(mean=stats[0], scale=stats[1])
        save(f"probe_{tag}", rec)
        return
    raise SystemExit(f"{tag}: no seed met the conditions")


def save(name, rec):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in rec.items()})
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(rec)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f"wrote {path} ({size / 1024:.0f} KiB)")


def e2e_case(tag, ds_name, seed, n=(128, 48, 48), bs=16, T=9):
    """evaluate / evaluate_raw_data of the reference on the model of tests/golden/mb_z20_nopos (its recorded state dict)."""
    with np.load(os.path.join(OUT, "mb_z20_nopos.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    p = os.path.join(OUT, "mb_z20_nopos.part1.npz")
    if os.path.exists(p):
        with np.load(p, allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files})
    zd, dx, dy = (int(v) for v in g["cfg"][:3])
    with contextlib.redirect_stdout(io.StringIO()):
        m = RM.UML(RM.Linear(dx, zd), RM.Linear(dy, zd),
                   RM.Transformer(zd, zd, nhead=5, num_layers=5, conv1d=True, out_last=False, pos_embd=False, pos_learnable=False,
                                  max_len=128), [RM.Linear(zd, dx), RM.Linear(zd, dy)], modality="xy")
    m.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd::")})
    rng = np.random.default_rng(seed)
    cfg, rec = {"freq": 2}, {}
    vx, vy = rng.standard_normal(dx), rng.standard_normal(dy)
    for k, nk in zip(("train", "val", "test"), n):
        x = rng.standard_normal((nk, T, dx)).astype(np.float32)
        y = rng.standard_normal((nk, T, dy)).astype(np.float32)
        lx = rng.integers(2, T + 1, nk)
        ly = rng.integers(2, T + 1, nk)
        lx[0], ly[0], lx[1], ly[1] = T, T, 1, 1
        s = x[:, :2].mean(1) @ vx / np.sqrt(dx) + y[:, :2].mean(1) @ vy / np.sqrt(dy) + 0.3 * rng.standard_normal(nk)
        y01 = (s > 0).astype(np.int64)
        lab = raw_label(y01, ds_name, rng)
        cfg[k] = batches(x, y, lab, lx, ly, bs)
        rec.update({f"x_{k}": x, f"y_{k}": y, f"lx_{k}": lx, f"ly_{k}": ly, f"labels_{k}": lab, f"y01_{k}": y01})
    coefs = lambda fits: [np.concatenate([f[0].coef_.reshape(-1), f[0].intercept_.reshape(-1)]) for f in fits]
    with observed():
        raw = RT.evaluate_raw_data(cfg, ds_name)
    for name, w in zip(("x", "y", "xy"), coefs(FITS)):             # sklearn's own solutions, to count its flips against the optimum
        rec["wref_raw_" + name] = w
    np.random.seed(seed)
    outs = []
    hook = m.register_forward_hook(lambda mod, args, out: outs.append(out))
    with observed():
        res = RT.evaluate(m.eval(), cfg, ds_name)
    hook.remove()
    first = 0
    for k in ("train", "val", "test"):                            # the token embeddings evaluate pooled, in batch order
        nb = len(cfg[k])
        rec[f"zx_{k}"] = torch.cat([o["zx"] for o in outs[first:first + nb]]).numpy()
        rec[f"zy_{k}"] = torch.cat([o["zy"] for o in outs[first:first + nb]]).numpy()
        first += nb
    for name, w in zip(("sep_train", "sep_val", "sep_test", "x", "y", "xy"), coefs(FITS)):
        rec["wref_" + name] = w
    fitted = list(SCALED) if ds_name == "mosi" else [f[1] for f in FITS]
    perms = list(PERMS)
    for i, k in enumerate(("train", "val", "test")):          # the modality-separation fits saw [x1; x2][perm]
        both = fitted[i][np.argsort(perms[i])]
        nk = both.shape[0] // 2
        rec[f"emb_x_{k}"], rec[f"emb_y_{k}"] = both[:nk], both[nk:]
    assert np.array_equal(fitted[3], rec["emb_x_train"]) and np.array_equal(fitted[4], rec["emb_y_train"])
    for k, v in {**raw, **res}.items():
        rec["res::" + k] = np.float64(v)
    rec.update(ds_name=np.array(ds_name), batch_size=np.int64(bs), model=np.array("mb_z20_nopos"),
               keys_raw=np.array(sorted(raw)), keys_eval=np.array(sorted(res)))
    print(f"  {tag}: " + " ".join(f"{k}={float(v):.4f}" for k, v in sorted({**raw, **res}.items()) if not np.isnan(float(v))))
    save(f"probe_e2e_{tag}", rec)


if __name__ == "__main__":
    torch.set_num_threads(4)
    os.makedirs(OUT, exist_ok=True)
    #          tag        dataset   N     d   held  scale shift const noise seed
    probe_case("mosi_a", "mosi", 1284, 40, 400, 2.0, 5.0, 3, 0.5, 100)        # constant column, column means far from 0
    probe_case("mosi_b", "mosi", 300, 80, 300, 1.5, 0.0, None, 0.7, 200)      # d > N / 4
    probe_case("mosei_a", "mosei", 2000, 40, 400, 1.0, 0.2, None, 0.5, 300)
    probe_case("mosei_b", "mosei", 1500, 80, 400, 1.5, 0.5, None, 0.6, 400)
    probe_case("humor_c", "humor", 800, 33, 300, 1.0, 0.1, None, 0.4, 500)    # d not a multiple of the 8-column MFMA block
    e2e_case("mosi", "mosi", 11)
    e2e_case("humor", "humor", 12)
