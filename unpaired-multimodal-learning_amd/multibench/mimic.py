"""Device-resident MIMIC loader: the reference's MultiBench/datasets/mimic/get_data.py (cleaning, population standardisation,
the fixed ``random.seed(10)`` split, DataLoaders over lists of tuples, eleven noise levels of the test split) as two tables
built once on the GPU and one HIP launch per batch (kernels: umlh_kernels_tabular.hip through ``umlh.seqload``; DESIGN section
24).  ``main.py --ds_name mimic`` of the reference (main.py:89-96,116-122) is ``build_run``.

The reference's loader works; its consumers of ``'mimic'`` do not (train.py:369-371 reads elements 2 and 3 of a 3-tuple,
train.py:143-144 raises for its labels).  So the batches here come in the ``_process_1`` layout every consumer of this project
already takes -- the static table as a sequence of length 1 -- under a dataset name OTHER than ``'mimic'``
(``'mimic_icd9'`` / ``'mimic_mortality'``): that name keeps its pinned behaviour (``evaluate`` without ``label_fn`` and
``take_fixed_samples`` raise for it, ``train._unpack`` reads the reference's flat tuple under it), any other name takes the
``_process_1`` path and the lbfgs probe, which is what the reference's ``make_classifier`` gives MIMIC.

The tabular noise: the reference's ``swap_entry`` swaps nothing.  ``data[i][j] = data[i][j-1]`` copies the already updated left
neighbour to the right and ``data[i][j-1] = data[i][j]`` writes back what it has just read: a carry, restated here as one.
The mortality labels: the reference overwrites ``adm_labels_all[:, 1]`` in place while it reads it (row i's column 1 is read
before it is written, so the rule sees the original values); here the rule runs on a copy and the caller's array stays as it was.

Declared differences and limitations:
  * the caller's arrays are not modified (the reference cleans and standardises them in place);
  * the statistics are always fp64, also for a float32 pickle (the reference then standardises in float32);
  * the tables are fp32: a batch is the reference's float64 batch rounded once (within 1 fp32 ulp), and the Gaussian noise of a
    level is added to the fp32 table value in fp64 and rounded once;
  * ``num_workers`` is ignored;
  * ``capture_embeddings_during_training`` stays unusable with MIMIC: ``take_fixed_samples`` needs equal totals of valid rows
    and 1 against 24 per sample is not equal (the reference's branch collects no lengths and crashes later);
  * ``datasets/mimic/multitask.py`` is not mirrored.
"""
from __future__ import annotations

import random

import numpy as np
import torch

from .data import DeviceLoader, LevelSequence, _build_model, _device, _open_pickle

# main.py:89-96: batch size, [x, y] input widths (static, series), the pickle's name and the icd9 task; 40 is the default
# batch size of the reference's get_dataloader, which its evaluation loaders run with
MIMIC = {"batch_size": 128, "eval_batch_size": 40, "indims": [5, 12], "file": "im.pk", "task": 7}
LEVELS = 11


def labels_for_task(datafile, task):
    """The labels of get_data.py:58-77 as a new array [N]: ``y_icd9[:, task]`` for ``task >= 0``; for ``task < 0`` the
    six-class mortality rule on ``adm_labels_all`` -- the first of columns 1..5 that is > 0, else 0 -- in that array's dtype.
    The reference writes the result into column 1 of the array it reads; row i's own column 1 is read before it is written, so
    the rule sees original values throughout.  Here it runs on a copy."""
    if task >= 0:
        return np.array(np.asarray(datafile["y_icd9"])[:, task], copy=True)
    adm = np.array(datafile["adm_labels_all"], copy=True)
    y = adm[:, 1]                                             # a view of the copy, as the reference's y is of the original
    y[...] = np.select([adm[:, c] > 0 for c in range(1, 6)], [1, 2, 3, 4, 5], 0)
    return np.ascontiguousarray(y)


def split_indices(n):
    """(valid, test, train) index lists of get_data.py:78-86: ``random.seed(10); random.shuffle(datasets)`` on a private
    ``random.Random(10)`` -- the same permutation, the global ``random`` state untouched -- then ``[0 : n//10]``,
    ``[n//10 : n//5]`` and ``[n//5 :]``."""
    perm = list(range(int(n)))
    random.Random(10).shuffle(perm)
    return perm[:n // 10], perm[n // 10:n // 5], perm[n // 5:]


class MimicTable:
    """The whole ``im.pk`` on the device.  ``datafile``: the unpickled dict with 'adm_features_all' [N, ds],
    'ep_tdata' [N, T, dt] and 'y_icd9' / 'adm_labels_all', or its path; it is not modified.

    The build uploads both arrays in their own dtype (float64 stays float64) and makes two ``umlh.seqload.tab_standardize``
    calls, static as [N, ds] and series as [N * T, dt]: the statistics are over ALL samples, before the split, as in the
    reference.  It makes no synchronisation.  After it: ``static`` [N, ds] and ``series`` [N, T, dt] fp32 device tables,
    ``stats_static`` / ``stats_series`` ([2, d] float64 device: mean | std), and on the host ``labels`` [N] and the index lists
    ``valid``, ``test``, ``train`` of the fixed split."""

    def __init__(self, datafile, task, device=None):
        from umlh import seqload
        datafile = _open_pickle(datafile)
        xs, xt = np.asarray(datafile["adm_features_all"]), np.asarray(datafile["ep_tdata"])
        if xs.ndim != 2 or xt.ndim != 3 or xt.shape[0] != xs.shape[0] or min(xs.shape) < 1 or min(xt.shape) < 1:
            raise ValueError(f"MimicTable: adm_features_all {xs.shape} and ep_tdata {xt.shape}; expected [N, ds] and [N, T, dt]")
        self.device, self.task = _device(device), int(task)
        self.labels = labels_for_task(datafile, self.task)
        if self.labels.shape[0] != xs.shape[0]:
            raise ValueError(f"MimicTable: {self.labels.shape[0]} labels for {xs.shape[0]} samples")
        n, t_len, dt = xt.shape
        own = lambda a: np.ascontiguousarray(a, dtype=a.dtype if a.dtype in (np.float32, np.float64) else np.float64)
        with torch.cuda.device(self.device):
            self.static, self.stats_static = seqload.tab_standardize(torch.from_numpy(own(xs)).to(self.device))
            series, self.stats_series = seqload.tab_standardize(torch.from_numpy(own(xt)).to(self.device).view(n * t_len, dt))
        self.series = series.view(n, t_len, dt)
        self.valid, self.test, self.train = split_indices(n)

    def __len__(self):
        return int(self.static.shape[0])


class MimicLoader(DeviceLoader):
    """Batches of the rows ``rows`` (host positions into the two device tables ``static`` [n, ds] and ``series`` [n, T, dt])
    with ``labels`` (host array, one per entry of ``rows``): ``SequenceSampler`` for the order, one ``umlh_rows_gather`` launch
    per batch.  Default layout, the ``_process_1`` one: ``([static [b, 1, ds], None, series [b, T, dt]], [ones [b], None,
    full(T) [b]], inds [b, 1], labels [b, 1])`` with blocks and lengths on the device, ``inds`` (positions in this loader's
    dataset) and ``labels`` on the host.  ``reference_layout``: the reference's own ``(static [b, ds], series [b, T, dt],
    labels [b])``.  ``flatten_time_series``: the series block as [b, T * dt], a view of the same block."""

    def __init__(self, static, series, rows, labels, batch_size, shuffle=False, generator=None, reference_layout=False,
                 flatten_time_series=False):
        self.static, self.series = static, series
        self.rows = torch.as_tensor(np.asarray(rows, dtype=np.int64))
        self.labels = torch.as_tensor(np.ascontiguousarray(labels))
        if self.rows.ndim != 1 or self.labels.shape != self.rows.shape:
            raise ValueError(f"MimicLoader: rows {tuple(self.rows.shape)} and labels {tuple(self.labels.shape)} (one label per row)")
        self.reference_layout, self.flatten = bool(reference_layout), bool(flatten_time_series)
        super().__init__(len(self.rows), batch_size, shuffle, generator)

    def _prepare(self, order):
        from umlh import seqload
        dev = self.static.device
        ids = self.rows[order].to(dev)
        ones = torch.ones(min(self.batch_size, len(order)), dtype=torch.int64, device=dev)
        return seqload.rows_gather, order, ids, self.labels[order], ones, torch.full_like(ones, self.series.shape[1])

    def _batch(self, epoch, i, lo, hi):
        rows_gather, order, ids, labels, ones, full = epoch
        st, se = rows_gather([self.static, self.series], ids[lo:hi])
        if self.flatten:
            se = se.view(se.shape[0], -1)
        if self.reference_layout:
            return st, se, labels[lo:hi]
        return [st.unsqueeze(1), None, se], [ones[:hi - lo], None, full[:hi - lo]], order[lo:hi].view(-1, 1), labels[lo:hi].view(-1, 1)


def draw_mimic_noise(n_test, levels=LEVELS, tabular_robust=True, timeseries_robust=True, rng=None, static_dim=5, series_shape=(24, 12)):
    """The host draws of the reference's eleven test sets (get_data.py:91-111), pure numpy, in its order.  Per level k, with
    p = k / 10 and n = ``n_test``: ``n * static_dim`` uniforms (drop_entry), ``n * (static_dim - 1)`` uniforms (swap_entry),
    then n normals N(0, p), one per SAMPLE (white_noise on the one-element list of tables), ``n * T * dt`` uniforms
    (random_drop, per element) and n uniforms (structured_drop, per sample).  A disabled family draws nothing.  ``rng``: a numpy
    RandomState, an int seed, or None for numpy's global legacy stream (the reference); one stream runs through all levels.
    Returns per level a dict: 'drop' uint8 [n, static_dim] and 'carry' uint8 [n, static_dim - 1] (1 where
    ``random_sample() < p``), 'eps' float64 [n], 'elem' uint8 [n, T * dt] (1 where dropped) and 'keep' uint8 [n] (0 where
    dropped); None for a disabled family.  Level 0 still draws."""
    from .robustness import _draw, _rng
    g = _rng(rng)                                             # one stream for all levels, also when ``rng`` is an int seed
    n, words = int(n_test), int(series_shape[0]) * int(series_shape[1])
    out = []
    for k in range(int(levels)):
        p = k / 10
        lv = dict.fromkeys(("drop", "carry", "eps", "elem", "keep"))
        if tabular_robust:
            lv["drop"] = (g.random_sample((n, static_dim)) < p).astype(np.uint8)
            lv["carry"] = (g.random_sample((n, static_dim - 1)) < p).astype(np.uint8)
        if timeseries_robust:                                 # the series are float64 in the reference: eps is not rounded
            lv["eps"] = _draw(g, [n], p, True, False, [np.float64])[0][0]
            lv["elem"] = (g.random_sample((n, words)) < p).astype(np.uint8)
            lv["keep"] = _draw(g, [n], p, False, True, [np.float32])[0][1]
        out.append(lv)
    return out


def _level_tables(static, series, lv):
    """(static [n, ds], series [n, T, dt]) of one level from its draws ``lv``: one ``tab_perturb`` on the static rows; on the
    series one ``umlh_seq_perturb`` with a draw per sample (Gaussian noise and the per-sample drop) and one ``tab_perturb`` on
    its [n, T * dt] view with the element mask as ``drop`` and no carry -- zeroing commutes with the rest."""
    from umlh import seqload
    from .robustness import _perturb
    dev = static.device
    up = lambda a: torch.from_numpy(a).to(dev)
    with torch.cuda.device(dev):
        if lv["drop"] is not None:
            static = seqload.tab_perturb(static, up(lv["drop"]), up(lv["carry"]) if static.shape[1] > 1 else None)
        if lv["eps"] is not None:
            series = _perturb(series, lv["eps"], lv["keep"])
            flat = series.view(series.shape[0], -1)
            seqload.tab_perturb(flat, up(lv["elem"]), None, out=flat)
    return static, series


def get_dataloader(task, batch_size=40, num_workers=1, train_shuffle=True, imputed_path="im.pk", flatten_time_series=False,
                   tabular_robust=True, timeseries_robust=True, device=None, generator=None, rng=None, reference_layout=False,
                   table=None):
    """The reference's ``get_dataloader`` (get_data.py:16-113): ``(trains, valids, tests)``.  ``trains`` and ``valids`` are
    MimicLoaders over the fixed split of one ``MimicTable`` (``table``: one built already for the same ``task``, which then
    stands for ``imputed_path`` and ``device``; else built from ``imputed_path``, the pickle's path or its dict); ``trains`` shuffles with ``generator`` (None: torch's global one, as the reference).
    ``tests = {'timeseries': levels}``: a lazy sequence of eleven unshuffled loaders over the test split, one per noise level
    k / 10; all host draws happen here, in level order (``draw_mimic_noise``, ``rng``).  ``num_workers`` is ignored."""
    from umlh import seqload
    tb = table if table is not None else MimicTable(imputed_path, task, device)
    if tb.task != int(task):
        raise ValueError(f"get_dataloader: task={task} with a table built for task {tb.task} (its labels are that task's)")
    opts = {"reference_layout": reference_layout, "flatten_time_series": flatten_time_series}
    lab = lambda idx: tb.labels[np.asarray(idx, dtype=np.int64)]
    trains = MimicLoader(tb.static, tb.series, tb.train, lab(tb.train), batch_size, shuffle=train_shuffle, generator=generator, **opts)
    valids = MimicLoader(tb.static, tb.series, tb.valid, lab(tb.valid), batch_size, **opts)
    n_test = len(tb.test)
    levels = []
    if n_test:
        draws = draw_mimic_noise(n_test, LEVELS, tabular_robust, timeseries_robust, rng, tb.static.shape[1], tuple(tb.series.shape[1:]))
        with torch.cuda.device(tb.device):
            static, series = seqload.rows_gather([tb.static, tb.series], torch.tensor(tb.test, dtype=torch.int64).to(tb.device))
        test_labels = lab(tb.test)
        levels = LevelSequence(len(draws), lambda k: _level_tables(static, series, draws[k]),
                               lambda t: MimicLoader(t[0], t[1], np.arange(t[0].shape[0]), test_labels, batch_size, **opts),
                               (static, series))
    return trains, valids, {"timeseries": levels}


def _int_labels(y):
    return np.asarray(y).astype(np.int64)


def build_run(data, zdim, task=MIMIC["task"], modality="xy", lr=1e-4, infoNCE_loss=False, pos_embd=False, pos_learnable=False,
              device=None, batch_size=MIMIC["batch_size"], eval_batch_size=MIMIC["eval_batch_size"], generator=None,
              generator_2=None, rng=None):
    """Loaders, model and optimizer wired as the reference's main.py:89-96,116-122: two shuffled train loaders of batch 128 on
    one table (``generator`` / ``generator_2``; None: torch's global one, as the reference), the unshuffled evaluation loaders
    with the reference's default batch 40 -- 'test' IS the valid loader ("as per FACTOR-CL codebase", main.py:96) --, the UML
    model with indims [static width, series width] on the device and Adam.  ``data``: the pickle's dict or its path.
    Returns a dict with 'train_loader', 'train_loader_2', 'eval_config' (batch lists, freq 100, 'label_fn': the labels as
    integers -- 0/1 for an icd9 task, the six mortality classes for ``task < 0`` --, 'ds_name'), 'robust' (the eleven noise
    levels of the test split, for ``evaluate_robustness``), 'table', 'model', 'optimizer', 'indims', 'batch_size' and
    'ds_name': 'mimic_icd9' or 'mimic_mortality', the name to pass to ``train`` / ``evaluate`` (NOT 'mimic', see the module's
    docstring)."""
    dev = _device(device)
    ds_name = "mimic_mortality" if task < 0 else "mimic_icd9"
    table = MimicTable(data, task, dev)
    train_loader, _, _ = get_dataloader(task, batch_size, table=table, generator=generator, tabular_robust=False, timeseries_robust=False)
    train_loader_2 = MimicLoader(table.static, table.series, train_loader.rows, train_loader.labels, batch_size, shuffle=True,
                                 generator=generator_2)
    eval_train, valid, robust = get_dataloader(task, eval_batch_size, train_shuffle=False, table=table, rng=rng)
    indims = [int(table.static.shape[1]), int(table.series.shape[2])]
    model, optimizer = _build_model(indims, zdim, modality, lr, infoNCE_loss, pos_embd, pos_learnable, dev)
    valid_batches = list(valid)
    return {"train_loader": train_loader, "train_loader_2": train_loader_2, "model": model, "optimizer": optimizer,
            "eval_config": {"train": list(eval_train), "val": valid_batches, "test": valid_batches, "freq": 100,
                            "label_fn": _int_labels, "ds_name": ds_name},
            "robust": robust, "table": table, "indims": indims, "batch_size": batch_size, "ds_name": ds_name}
