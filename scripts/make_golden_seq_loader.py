"""Golden batches of the affect datasets' loader: runs the reference's own get_dataloader
(MultiBench/datasets/affect/get_data.py) on CPU torch with num_workers=0 on seeded synthetic pickles and writes
tests/golden/seq_loader.npz + seq_loader.partK.npz (every file under 1 MiB).  Needs the reference checkout (REFERENCE_ROOT,
default ../reference next to the repo); no test reads it.  The reference module is imported at run time; h5py, torchtext and
robustness.* (imported there, used only by options this project does not implement) get empty stub modules.

Datasets (train / valid / test = 23 / 9 / 9 samples; valid is float64, the others float32):
  toy_a, toy_b    T = 12, D = (5, 4, 7)          wide_a, wide_b    T = 50, D = (130, 3, 67)
Every train split holds a dropped sample (text all zero), a start = 0 sample, a start = T - 1 sample (length 1), one -inf in
audio, a -0.0 in a text front row, constant columns, and front rows of vision / audio that are not zero.  The *_a sets also put a
NaN into the text row that decides a sample's start; the *_b sets (used under z_norm) hold none, and every (sample, column) of
them is either exactly constant with a small-integer value or has a sample std of at least 2^-3 of its largest magnitude.
Values are multiples of 1/8 (float32) or of 1/10 (float64: not representable in fp32), so the files compress.

Cases: data types mosi (plain), sarcasm with vision_norm, mosei with z_norm on both shapes at batch size 4, and mosi at batch
size 11 (which divides the 22 kept train samples).  Per case: two epochs of the shuffled train loader and the valid loader, batch
by batch (blocks, lengths, inds, labels)."""
import importlib.util
import io
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", os.path.join(os.path.dirname(ROOT), "reference"))
N_SPLIT = {"train": 23, "valid": 9, "test": 9}
SHAPES = {"toy": (12, (5, 4, 7)), "wide": (50, (130, 3, 67))}
DATASETS = {"toy_a": ("toy", True, 11), "toy_b": ("toy", False, 12), "wide_a": ("wide", True, 13), "wide_b": ("wide", False, 14)}
CASES = {            # name: (dataset, data_type, z_norm, vision_norm, batch size)
    "toy_mosi": ("toy_a", "mosi", False, False, 4),
    "toy_sarcasm_vnorm": ("toy_a", "sarcasm", False, True, 4),
    "toy_mosei_znorm": ("toy_b", "mosei", True, False, 4),
    "toy_mosi_bs11": ("toy_a", "mosi", False, False, 11),
    "wide_mosi": ("wide_a", "mosi", False, False, 4),
    "wide_sarcasm_vnorm": ("wide_a", "sarcasm", False, True, 4),
    "wide_mosei_znorm": ("wide_b", "mosei", True, False, 4),
}
PART_BYTES = 900 * 1024


def load_reference():
    for name in ("h5py", "torchtext", "robustness", "robustness.text_robust", "robustness.timeseries_robust"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["robustness.text_robust"].add_text_noise = None
    sys.modules["robustness.timeseries_robust"].add_timeseries_noise = None
    spec = importlib.util.spec_from_file_location("ref_affect_get_data", os.path.join(REF, "MultiBench", "datasets", "affect", "get_data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _values(rng, shape, dtype, offset=0.0, scale=1.0):
    q = 8.0 if dtype == np.float32 else 10.0
    return (np.round((rng.standard_normal(shape) * scale + offset) * q) / q).astype(dtype)


def z_norm_condition(seq):
    """(ok, constant) per column of one trimmed [L, D] sequence: constant with a small-integer value, or a sample std of at least
    2^-3 of the largest magnitude."""
    seq = np.asarray(seq, dtype=np.float64)
    const = (seq == seq[0]).all(0)
    small_int = const & (seq[0] == np.round(seq[0])) & (np.abs(seq[0]) <= 8)
    with np.errstate(all="ignore"):
        sd = seq.std(0, ddof=1) if seq.shape[0] > 1 else np.zeros(seq.shape[1])
    return np.where(const, small_int, sd >= 2.0 ** -3 * np.abs(seq).max(0)), const


def make_split(rng, n, T, dims, dtype, with_nan, special):
    off = [rng.uniform(-3, 3, d) for d in dims]
    sc = [rng.uniform(0.5, 2.0, d) for d in dims]
    x = [_values(rng, (n, T, d), dtype, o, s) for d, o, s in zip(dims, off, sc)]
    start = rng.integers(0, T - 1, n)
    if special:
        start[0], start[1], start[4] = 0, T - 1, max(3, start[4])
    for i in range(n):
        s = int(start[i])
        x[2][i, :s] = 0.0
        if i % 2 == 0:
            x[0][i, :s] = 0.0                                      # odd samples keep nonzero vision in front of their text
        x[1][i, :min(s + (i % 3), T - 1)] = 0.0                    # audio's own first row is often later than the text's
        if x[2][i, s, 0] == 0:
            x[2][i, s, 0] = 1.0
        if T - s == 1:                                             # a length-1 sequence: small integers (exact fp32 means)
            for a in x:
                a[i, s] = rng.integers(-3, 4, a.shape[2])
            x[2][i, s, 0] = 2.0
    if special:
        x[2][2] = 0.0                                              # the dropped sample; its vision and audio stay
        s5 = int(start[5])
        x[0][5, s5:, 0], x[1][5, s5:, 0], x[2][5, s5:, 1] = 3.0, 0.0, -2.0      # constant columns
        s4 = int(start[4])
        x[2][4, s4 - 2, 1] = -0.0                                  # a front row: -0.0 is not a nonzero
        if with_nan:
            x[2][4, s4] = 0.0
            x[2][4, s4, 2] = np.nan                                # the element that decides this sample's start
    for i in range(n):                                             # the z_norm condition, column by column
        s = int(start[i])
        if special and i == 2:
            continue
        for m, a in enumerate(x):
            for _ in range(200):
                ok, _c = z_norm_condition(a[i, s:])
                bad = np.flatnonzero(~ok & ~np.isnan(a[i, s:]).any(0))
                if bad.size == 0:
                    break
                a[i, s + 1:, bad] = _values(rng, (bad.size, T - s - 1), dtype, 0.0, 2.0)
            else:
                raise RuntimeError("could not meet the z_norm condition")
    if special:
        s3 = int(start[3])
        x[1][3, T - 1, 1] = -np.inf                                # becomes 0 before anything else looks at it
        ok, _c = z_norm_condition(np.where(np.isinf(x[1][3, s3:]), 0.0, x[1][3, s3:]))
        assert ok.all(), "the -inf broke the z_norm condition: change the seed"
    for i in range(n):                                             # the two drop rules must agree on every sample (the reference
        if not (special and i == 2) and x[2][i].sum() == 0:        # drops on text.sum() == 0)
            x[2][i, int(start[i]), 0] += 1.0
    labels = _values(rng, (n, 1, 1), dtype, 0.8, 1.5)
    return {"vision": x[0], "audio": x[1], "text": x[2], "labels": labels, "id": np.arange(100, 100 + n, dtype=np.int64).reshape(n, 1)}


def make_dataset(name):
    shape, with_nan, seed = DATASETS[name]
    T, dims = SHAPES[shape]
    rng = np.random.default_rng(seed)
    return {s: make_split(rng, N_SPLIT[s], T, dims, np.float64 if s == "valid" else np.float32, with_nan, s == "train")
            for s in ("train", "valid", "test")}


def record_case(ref, name, data, out):
    import torch
    dataset, data_type, z_norm, vision_norm, bs = CASES[name]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "data.pkl")
        with open(path, "wb") as f:
            pickle.dump(data, f)                                   # the reference reads (and modifies) its own copy
        train, valid, _test = ref.get_dataloader(path, batch_size=bs, num_workers=0, train_shuffle=True, data_type=data_type,
                                                 z_norm=z_norm, vision_norm=vision_norm)
        for loader, it in (("train0", train), ("train1", train), ("valid", valid)):
            batches = list(it)
            out[f"case/{name}/{loader}/batches"] = np.int64(len(batches))
            for i, (xs, ls, inds, labels) in enumerate(batches):
                for m in range(3):
                    assert xs[m].dtype == torch.float32 and ls[m].dtype == torch.int64
                    out[f"case/{name}/{loader}/{i}/x{m}"] = xs[m].numpy()
                    out[f"case/{name}/{loader}/{i}/l{m}"] = ls[m].numpy()
                assert inds.dtype == torch.int64 and labels.dtype == torch.float32
                out[f"case/{name}/{loader}/{i}/inds"] = inds.numpy()
                out[f"case/{name}/{loader}/{i}/labels"] = labels.numpy()
    out[f"case/{name}/config"] = np.array([dataset, data_type, str(int(z_norm)), str(int(vision_norm)), str(bs)])


def _packed_size(arr):
    buf = io.BytesIO()
    np.savez_compressed(buf, a=arr)
    return buf.tell()


def main():
    ref = load_reference()
    np.seterr(all="ignore")
    out = {}
    datasets = {name: make_dataset(name) for name in DATASETS}
    for name, data in datasets.items():
        for split in ("train", "valid"):
            for k, v in data[split].items():
                out[f"data/{name}/{split}/{k}"] = v
    for name in CASES:
        record_case(ref, name, datasets[CASES[name][0]], out)
    out_dir = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(out_dir, "seq_loader.npz"), cases=np.array(list(CASES)), datasets=np.array(list(DATASETS)))
    parts, cur, size = [], {}, 0
    for k, v in out.items():
        b = _packed_size(v) + 200
        if cur and size + b > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += b
    parts.append(cur)
    for i, p_ in enumerate(parts, 1):
        path = os.path.join(out_dir, f"seq_loader.part{i}.npz")
        np.savez_compressed(path, **p_)
        assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
