"""Golden data of the robustness test sets: runs the reference's own time-series noise
(MultiBench/robustness/timeseries_robust.py) and its own drop_entry, Affectdataset and _process_1
(MultiBench/datasets/affect/get_data.py) on CPU, in the order of get_data.py:349-404, on seeded synthetic arrays, and writes
tests/golden/robust_noise.npz (under 1 MiB).  Needs the reference checkout (REFERENCE_ROOT, default ../reference next to the
repo) and scripts/make_golden_seq_loader.py (its synthetic splits); no test reads either.  h5py, torchtext and
robustness.text_robust (imported by get_data.py, used only for the text family) get empty stub modules.

noise/<case>/...   the noise function alone, ``add_timeseries_noise(list, noise_level=p, rand_drop=False)`` after
                   ``np.random.seed(seed)``, for p in 0, 0.3, 1.0:
    table      one float32 [7, 5, 3] table with a NaN, +-Inf, a -0.0 and a denormal
    list3      three float32 tables [6, 4, d], d = 2, 5, 1, in one call
    table64    one float64 [7, 5, 3] table (fp32-representable values): the sum is formed in float64 there
    steps      per time step: three samples, for each in order one call on its list of three [5, d] float32 arrays
fam/<case>/<family>/<level>/...   every batch of levels 0, 3 and 9 of robust_vision, robust_audio and robust_timeseries
    (all ten levels are run: the draws of a family are one stream, ``np.random.seed(seed)`` before its level 0) on a float32
    test split of make_golden_seq_loader's kind (23 samples, T = 12, D = (5, 4, 7): one text-less sample, one -inf in audio),
    batch size 4, data_type mosi; case 'plain' without normalisation, case 'vnorm' with vision_norm."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", os.path.join(os.path.dirname(ROOT), "reference"))
LEVELS_P = (0.0, 0.3, 1.0)
FAMILIES = ("robust_vision", "robust_audio", "robust_timeseries")
RECORDED = (0, 3, 9)
CASES = {"plain": (False, 4, 101), "vnorm": (True, 4, 201)}       # vision_norm, batch size, seed of the first family
NOISE_SEEDS = {"table": 11, "list3": 21, "table64": 31, "steps": 41}


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    noise = _load("robustness.timeseries_robust", os.path.join(REF, "MultiBench", "robustness", "timeseries_robust.py"))
    for name in ("h5py", "torchtext", "robustness", "robustness.text_robust"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["robustness.text_robust"].add_text_noise = None
    sys.modules["robustness.timeseries_robust"] = noise
    return _load("ref_affect_get_data", os.path.join(REF, "MultiBench", "datasets", "affect", "get_data.py")), noise


def noise_inputs():
    rng = np.random.default_rng(7)
    table = rng.standard_normal((7, 5, 3)).astype(np.float32)
    table[1, 0, 0], table[1, 2, 1], table[2, 1, 1] = np.nan, np.inf, -np.inf
    table[3, 0, 2], table[3, 4, 0], table[4, 2, 2] = -0.0, 1e-40, -3e-39
    return {"table": [table],
            "list3": [rng.standard_normal((6, 4, d)).astype(np.float32) for d in (2, 5, 1)],
            "table64": [rng.standard_normal((7, 5, 3)).astype(np.float32).astype(np.float64)],
            "steps": [rng.standard_normal((3, 5, d)).astype(np.float32) for d in (2, 3, 1)]}


def record_noise(noise, out):
    for case, arrays in noise_inputs().items():
        for k, a in enumerate(arrays):
            out[f"noise/{case}/in{k}"] = a
        out[f"noise/{case}/seed"] = np.int64(NOISE_SEEDS[case])
        for li, p in enumerate(LEVELS_P):
            np.random.seed(NOISE_SEEDS[case] + li)
            if case == "steps":
                got = [np.empty_like(a) for a in arrays]
                for s in range(arrays[0].shape[0]):
                    res = noise.add_timeseries_noise([a[s].copy() for a in arrays], noise_level=p, rand_drop=False)
                    for k, r in enumerate(res):
                        got[k][s] = r
            else:
                got = noise.add_timeseries_noise([a.copy() for a in arrays], noise_level=p, rand_drop=False)
            for k, r in enumerate(got):
                assert r.dtype == arrays[k].dtype
                out[f"noise/{case}/p{li}/out{k}"] = r


def record_family(ref, noise, test, family, vision_norm, bs, seed, prefix, out):
    import torch
    np.random.seed(seed)
    sizes = []
    for i in range(10):
        t = {m: test[m].copy() for m in ("vision", "audio", "text")}
        if family == "robust_timeseries":
            t["vision"], t["audio"], t["text"] = noise.add_timeseries_noise([t["vision"], t["audio"], t["text"]],
                                                                           noise_level=i / (10 * 3), rand_drop=False)
        else:
            m = family[len("robust_"):]
            t[m] = noise.add_timeseries_noise([t[m]], noise_level=i / 10, rand_drop=False)[0]
        t["labels"] = test["labels"]
        t = ref.drop_entry(t)
        sizes.append(t["vision"].shape[0])
        if i not in RECORDED:
            continue
        loader = torch.utils.data.DataLoader(ref.Affectdataset(t, False, task=None, max_pad=False, max_pad_num=50, data_type="mosi",
                                                               z_norm=False, vision_norm=vision_norm),
                                             shuffle=False, num_workers=0, batch_size=bs, collate_fn=ref._process_1)
        batches = list(loader)
        out[f"{prefix}/{i}/batches"] = np.int64(len(batches))
        for j, (xs, ls, inds, labels) in enumerate(batches):
            for m in range(3):
                assert xs[m].dtype == torch.float32 and ls[m].dtype == torch.int64
                out[f"{prefix}/{i}/{j}/x{m}"] = xs[m].numpy()
                out[f"{prefix}/{i}/{j}/l{m}"] = ls[m].numpy()
            out[f"{prefix}/{i}/{j}/inds"] = inds.numpy()
            out[f"{prefix}/{i}/{j}/labels"] = labels.numpy()
    return sizes


def main():
    ref, noise = load_reference()
    np.seterr(all="ignore")
    out = {}
    record_noise(noise, out)
    seq = _load("make_golden_seq_loader", os.path.join(ROOT, "scripts", "make_golden_seq_loader.py"))
    T, dims = seq.SHAPES["toy"]
    test = seq.make_split(np.random.default_rng(2024), 23, T, dims, np.float32, False, True)
    for k, v in test.items():
        out[f"fam/data/test/{k}"] = v
    dropped = ref.drop_entry({k: v.copy() for k, v in test.items()})        # get_data.py:305
    assert dropped["vision"].shape[0] == 22
    for case, (vision_norm, bs, seed) in CASES.items():
        out[f"fam/{case}/config"] = np.array([int(vision_norm), bs, seed], dtype=np.int64)
        for f, family in enumerate(FAMILIES):
            sizes = record_family(ref, noise, dropped, family, vision_norm, bs, seed + f, f"fam/{case}/{family}", out)
            out[f"fam/{case}/{family}/sizes"] = np.array(sizes, dtype=np.int64)
            print(case, family, sizes)
            if family == "robust_timeseries":
                assert sizes[0] == 22 and min(sizes[3], sizes[9]) < 22, "no text dropped by the noise: change the seed"
            else:
                assert sizes == [22] * 10
    path = os.path.join(ROOT, "tests", "golden", "robust_noise.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
