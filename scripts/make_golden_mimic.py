"""Golden data of the MIMIC loader: runs the reference's own ``datasets/mimic/get_data.py:get_dataloader`` (with its
``robustness/tabular_robust.py`` and ``timeseries_robust.py``) on CPU on seeded synthetic ``im.pk`` dicts and writes
tests/golden/mimic.npz, mimic.part1.npz and mimic.part2.npz (each under 1 MiB).  Needs the reference checkout (REFERENCE_ROOT,
default ../reference next to the repo); no test reads it.  The reference's modules are loaded by path; ``tqdm`` gets a stub when
it is missing.  The reference unpickles its datafile and then cleans and standardises the arrays in place: its ``pickle.load`` is
pointed at the script's own dict, so that those arrays can be recorded and a batch row can be traced to its sample.

<case>/in/...            adm_features_all [N, 5] and ep_tdata [N, 24, 12] (float64; NaN, +Inf and -Inf planted in both; column
                         means up to 8 std from 0), y_icd9 [N, 20] (int64), adm_labels_all [N, 6] (float64)
<case>/std/...           the two arrays after the call: cleaned and standardised
<case>/split/...         valid, test, train: sample indices in dataset order
<case>/labels/<task>/... the labels of the three splits for task = 7 and task = -1, as the unshuffled loaders give them
<case>/epoch/...         one unshuffled and one shuffled train epoch (``torch.manual_seed(seed)`` right before the latter): the
                         sample indices of every batch in one list and the batch sizes; the first and last batch in full
<case>/level/<k>/...     levels 0, 3 and 10 of tests['timeseries'] in full (``np.random.seed(seed)`` before the call)
n57/notab, n57/nots      level 3 with tabular_robust=False, and with timeseries_robust=False: the same seed, so each family gets
                         the draws the other one would have taken
<case>/config            N, batch size, numpy seed, torch seed

Cases: n57 and n203 (N divisible by neither 5 nor 10), const31 (one constant column in each table: its std is 0)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", os.path.join(os.path.dirname(ROOT), "reference"))
CASES = {"n57": (57, 8, 1234, 77, False), "n203": (203, 40, 4321, 78, False), "const31": (31, 8, 99, 79, True)}
FILES = {"n57": "mimic.npz", "const31": "mimic.npz", "n203/in": "mimic.part1.npz", "n203": "mimic.part2.npz"}
RECORDED = (0, 3, 10)
T, DS, DT = 24, 5, 12


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    try:
        import tqdm  # noqa: F401
    except ImportError:
        stub = types.ModuleType("tqdm")
        stub.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = stub
    sys.modules.setdefault("robustness", types.ModuleType("robustness"))
    for name in ("tabular_robust", "timeseries_robust"):
        _load(f"robustness.{name}", os.path.join(REF, "MultiBench", "robustness", f"{name}.py"))
    return _load("ref_mimic_get_data", os.path.join(REF, "MultiBench", "datasets", "mimic", "get_data.py"))


def make_datafile(n, seed, constant):
    rng = np.random.default_rng(seed)
    xs = (rng.standard_normal((n, DS)) + rng.uniform(-7.5, 7.5, DS)) * rng.uniform(0.5, 20.0, DS)       # |mean| up to 7.5 std
    xt = (rng.standard_normal((n, T, DT)) + rng.uniform(-7.5, 7.5, DT)) * rng.uniform(0.1, 5.0, DT)
    xs[1, 0], xs[2, 3], xs[n - 1, 4], xs[3, 1] = np.nan, np.inf, -np.inf, -0.0
    xt[0, 0, 0], xt[1, 5, 3], xt[n - 1, T - 1, DT - 1], xt[2, 2, 2], xt[4, 7, 7] = np.nan, np.inf, -np.inf, np.nan, -0.0
    if constant:
        xs[:, 2], xt[:, :, 5] = 2.5, -3.0
    adm = np.zeros((n, 6))
    adm[np.arange(n), rng.integers(0, 6, n)] = 1.0            # column 0 set: class 0 unless a later column is too
    extra = rng.random((n, 6)) < 0.15
    adm[extra] = 1.0
    return {"adm_features_all": xs, "ep_tdata": xt, "y_icd9": rng.integers(0, 2, (n, 20)).astype(np.int64), "adm_labels_all": adm}


def call(ref, datafile, task, seed, **kw):
    """The reference's get_dataloader on a deep copy of ``datafile`` -> (loaders, the copy it cleaned and standardised)."""
    own = {k: v.copy() for k, v in datafile.items()}
    load = ref.pickle.load                                    # ref.pickle IS the pickle module: patched for this call only
    ref.pickle.load = lambda f: own
    try:
        np.random.seed(seed)
        return ref.get_dataloader(task, num_workers=0, imputed_path=os.devnull, **kw), own
    finally:
        ref.pickle.load = load


def index_of(series_rows, table):
    """positions in ``table`` [N, T, DT] of the rows of ``series_rows`` [b, T, DT], matched bit for bit"""
    where = {table[i].tobytes(): i for i in range(table.shape[0])}
    assert len(where) == table.shape[0]
    return np.array([where[np.ascontiguousarray(r).tobytes()] for r in series_rows], dtype=np.int64)


def whole(loader):
    batches = list(loader)
    return [np.concatenate([b[k].numpy() for b in batches]) for k in range(3)], batches


def record(ref, case, n, bs, seed, tseed, constant, out):
    datafile = make_datafile(n, seed, constant)
    for k, v in datafile.items():
        out[f"{case}/in/{k}"] = v
    out[f"{case}/config"] = np.array([n, bs, seed, tseed], dtype=np.int64)
    (trains, valids, tests), own = call(ref, datafile, 7, seed, batch_size=bs, train_shuffle=False)
    xs, xt = own["adm_features_all"], own["ep_tdata"]
    assert xs.dtype == np.float64 and xt.dtype == np.float64
    out[f"{case}/std/static"], out[f"{case}/std/series"] = xs, xt
    (_, _, clean_tests), _ = call(ref, datafile, 7, seed, batch_size=bs, train_shuffle=False, tabular_robust=False, timeseries_robust=False)
    split = {}
    for name, loader in (("valid", valids), ("test", clean_tests["timeseries"][0]), ("train", trains)):
        (st, se, y), batches = whole(loader)
        assert batches[0][0].dtype == torch.float64 and batches[0][1].dtype == torch.float64 and batches[0][2].dtype == torch.int64
        split[name] = index_of(se, xt)
        assert np.array_equal(st, xs[split[name]], equal_nan=True)
        out[f"{case}/split/{name}"] = split[name]
        out[f"{case}/labels/7/{name}"] = y
    assert sorted(np.concatenate(list(split.values())).tolist()) == list(range(n))
    (tr1, va1, te1), _ = call(ref, datafile, -1, seed, batch_size=bs, train_shuffle=False, tabular_robust=False, timeseries_robust=False)
    for name, loader in (("valid", va1), ("test", te1["timeseries"][0]), ("train", tr1)):
        out[f"{case}/labels/-1/{name}"] = whole(loader)[0][2]
    # two train epochs
    (shuffled, _, _), _ = call(ref, datafile, 7, seed, batch_size=bs, tabular_robust=False, timeseries_robust=False)
    for name, loader in (("plain", trains), ("shuffled", shuffled)):
        if name == "shuffled":
            torch.manual_seed(tseed)
        (st, se, y), batches = whole(loader)
        out[f"{case}/epoch/{name}/index"] = index_of(se, xt)
        out[f"{case}/epoch/{name}/sizes"] = np.array([b[0].shape[0] for b in batches], dtype=np.int64)
        for which, b in (("first", batches[0]), ("last", batches[-1])):
            for k, key in enumerate(("static", "series", "labels")):
                out[f"{case}/epoch/{name}/{which}/{key}"] = b[k].numpy()
    # noise levels
    for k in RECORDED:
        (st, se, y), _ = whole(tests["timeseries"][k])
        out[f"{case}/level/{k}/static"], out[f"{case}/level/{k}/series"], out[f"{case}/level/{k}/labels"] = st, se, y
    if case == "n57":
        for name, kw in (("notab", {"tabular_robust": False}), ("nots", {"timeseries_robust": False})):
            (_, _, te), _ = call(ref, datafile, 7, seed, batch_size=bs, train_shuffle=False, **kw)
            (st, se, _), _ = whole(te["timeseries"][3])
            out[f"{case}/{name}/static"], out[f"{case}/{name}/series"] = st, se
    print(case, {k: len(v) for k, v in split.items()})


def main():
    ref = load_reference()
    np.seterr(all="ignore")
    out = {}
    for case, cfg in CASES.items():
        record(ref, case, *cfg, out)
    files = {}
    for key, v in out.items():
        case = key.split("/")[0]
        name = FILES.get("/".join(key.split("/")[:2]), FILES[case])
        files.setdefault(name, {})[key] = v
    for name, arrays in files.items():
        path = os.path.join(ROOT, "tests", "golden", name)
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
