"""Device-resident loader of the affect datasets (mosi, mosei, humor, sarcasm): the reference's
MultiBench/datasets/affect/get_data.py (a CPU Dataset + collate_fn behind a DataLoader) as a table built once on the GPU and
one HIP launch per batch (kernels: umlh_kernels_seqload.hip through ``umlh.seqload``).

``AffectTable`` does once, at build, what ``Affectdataset.__getitem__`` redoes for every sample of every epoch: the drop of
text-less samples, ``audio[audio == -inf] = 0``, ``vision_norm``, the front trim (kept as a per-sample ``start``) and ``z_norm``.
``SequenceLoader`` yields batches in exactly the ``_process_1`` layout, ``([vision, audio, text], [lv, la, lt], inds, labels)``,
so ``multibench.train.train`` / ``evaluate`` / ``evaluate_raw_data`` and ``multibench.capture.take_fixed_samples`` take them
unchanged: blocks and lengths are device tensors, ``inds`` and ``labels`` host tensors (the consumers move them where they
need them; nothing is read back).  ``SequenceSampler`` is the batch order, pure host code that follows torch's DataLoader
protocol draw for draw, so a run here visits the samples in the reference's order.  ``DeviceLoader`` (sampler, epoch driver,
deep copy) and ``LevelSequence`` (the lazy sequence of loaders over noise levels) are what this loader shares with
``multibench.mimic``, as are the pickle opener and the model builder of ``build_run``.

Declared differences from the reference:
  * drop: a sample is dropped when its text has no nonzero element; the reference drops on ``text.sum() == 0``.  A text whose
    nonzero elements sum to exactly 0 is kept here and dropped there; an all-zero text that survived there would crash its
    ``__getitem__``.
  * dtype: arrays are converted to fp32 at upload.  Without normalisation that is the reference's own ``.float()``, bit for bit;
    with ``vision_norm`` on a float64 pickle the statistics come from the fp32-rounded values.
  * statistics are accumulated in fp64 (the reference: numpy / torch fp32 sums).  In ``z_norm`` the reference's fp32 mean of a
    constant column is not always that constant (seven rows of 0.1f give -0.926 everywhere instead of 0); here every constant
    column is exactly 0.
  * ``aligned=False``, ``flatten_time_series``, ``max_pad`` (``_process_2``), ``task='classification'`` and ``robust_test`` raise
    NotImplementedError; the mimic loader is ``multibench.mimic`` (its own config and ``build_run``: ``DATASETS`` holds the affect sets only).

``robust_loaders`` is the time-series part of the reference's ``robust_test=True`` (get_data.py:349-404): per
noise level the test split after the drop, Gaussian noise and structured drop on vision, on audio, or on all three tables (host
draws in the reference's order, one ``umlh_seq_perturb`` launch per table), then the build above on the noisy tables -- the
second drop, ``vision_norm`` and the front trim see the noise.  The flag itself stays refused: the reference's return under it
begins with the text family, which needs raw words and GloVe vectors.
"""
from __future__ import annotations

import copy
import pickle

import numpy as np
import torch

MODALITIES = ("vision", "audio", "text")
# main.py:66-103: batch size, [x, y] input widths (vision, text), the pickle's name, data_type and vision_norm per ds_name
DATASETS = {
    "mosi": {"batch_size": 32, "indims": [20, 300], "file": "mosi_data.pkl", "data_type": "mosi", "vision_norm": False},
    "sarcasm": {"batch_size": 128, "indims": [371, 300], "file": "sarcasm.pkl", "data_type": "sarcasm", "vision_norm": True},
    "humor": {"batch_size": 128, "indims": [371, 300], "file": "humor.pkl", "data_type": "humor", "vision_norm": False},
    "mosei": {"batch_size": 32, "indims": [35, 300], "file": "mosei_senti_data.pkl", "data_type": "mosei", "vision_norm": False},
}
_DEFAULTS = {"aligned": True, "flatten_time_series": False, "max_pad": False, "task": None, "robust_test": False}
_IGNORED = ("num_workers", "max_seq_len", "max_pad_num", "raw_path")      # host-loader knobs with nothing to configure here


def _refuse_unsupported(who, options):
    """The reference's options this loader does not implement raise with their name; unknown ones are a TypeError."""
    for name, value in options.items():
        if name in _IGNORED:
            continue
        if name not in _DEFAULTS:
            raise TypeError(f"{who}: unexpected argument {name!r}")
        if name == "task" and value == "regression":          # the reference treats 'regression' as None (get_data.py:239)
            continue
        if name == "robust_test" and value:
            raise NotImplementedError(f"{who}: robust_test={value!r} is not implemented: the reference's return under that flag "
                                      "begins with the text family (raw words and GloVe).  The time-series families are "
                                      "multibench.data.robust_loaders")
        if value != _DEFAULTS[name]:
            raise NotImplementedError(f"{who}: {name}={value!r} is not implemented (only {name}={_DEFAULTS[name]!r}: the "
                                      "aligned, unflattened _process_1 path of get_data.py)")


def _device(device):
    if not torch.cuda.is_available():
        raise RuntimeError("multibench.data needs a GPU: the table is built and the batches are formed by HIP kernels only")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _open_pickle(data):
    """``data`` itself when it is the unpickled dict, else the dict in the pickle at that path."""
    if isinstance(data, dict):
        return data
    with open(data, "rb") as f:
        return pickle.load(f)


def _affect_arrays(split):
    """The three arrays of a split, and the index of the first that is not [N, T, D] with vision's N and T (None: all are)."""
    arrays = [np.asarray(split[m]) for m in MODALITIES]
    bad = [m for m, a in enumerate(arrays) if a.ndim != 3 or a.shape[:2] != arrays[0].shape[:2] or min(a.shape) < 1]
    return arrays, bad[0] if bad else None


def _upload(arrays, dev):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in arrays]


def _drop_textless(tables, start, none_left):
    """drop_entry (get_data.py:27-44) on three device tables [n, T, D_m]: the samples whose text has a nonzero element.
    ``start``: the text's first-nonzero rows when the caller has them already.  Returns the kept tables, their ``start``, the
    kept positions and the kept lengths T - start (host arrays); ``none_left`` is the error text when nothing is kept.  The
    read-back of ``start`` is the one synchronisation; the caller holds the device."""
    from umlh import seqload
    n_all, t_len = tables[0].shape[:2]
    if start is None:
        start = seqload.first_nonzero(tables[2])
    start_host = start.cpu().numpy()
    keep = np.flatnonzero(start_host < t_len)
    if keep.size == 0:
        raise ValueError(none_left)
    if keep.size < n_all:
        idx = torch.from_numpy(keep).to(tables[0].device)
        tables = [t.index_select(0, idx) for t in tables]
        start = start.index_select(0, idx).contiguous()
    return tables, start, keep, (t_len - start_host[keep]).astype(np.int64)


class AffectTable:
    """One split of an affect pickle on the device.  ``split``: the unpickled dict with 'vision', 'audio', 'text' as
    [N, T, D_m] numpy arrays and 'labels' (and 'id'); it is not modified.

    After the build: ``tables`` = the three fp32 device tables [n, T, D_m] of the kept samples (normalised as asked),
    ``start`` = int32 device [n], the first kept row of every sample, and on the host ``lengths`` (int64 numpy [n], T - start),
    ``labels`` (float32 tensor [n, 1], humor / sarcasm mapped to -1 / +1), ``ids`` (the split's 'id' rows of the kept samples,
    or None) and ``kept`` (their positions in the split).  A sample's index in a batch's ``inds`` is its position among the
    kept samples, as in the reference.  The build reads ``start`` back once; that is its only synchronisation."""

    def __init__(self, split, data_type="mosi", z_norm=False, vision_norm=False, device=None, **options):
        _refuse_unsupported("AffectTable", options)
        arrays, bad = _affect_arrays(split)
        if bad is not None:
            raise ValueError(f"AffectTable: {MODALITIES[bad]} has shape {arrays[bad].shape}; expected [N, T, D] with the N and T "
                             f"of vision {arrays[0].shape[:2]}")
        labels = np.asarray(split["labels"])
        n_all, t_len = arrays[0].shape[:2]
        if labels.shape[0] != n_all or labels.size != n_all:
            raise NotImplementedError(f"AffectTable: labels of shape {labels.shape} for {n_all} samples (one value per sample)")
        self.device, self.data_type, self.t_len = _device(device), data_type, t_len
        with torch.cuda.device(self.device):
            tables = _upload(arrays, self.device)
        self._build(tables, labels.reshape(n_all), np.asarray(split["id"]) if "id" in split else None, z_norm, vision_norm)

    @classmethod
    def _from_device(cls, tables, labels, ids, data_type="mosi", z_norm=False, vision_norm=False, start=None, positions=None):
        """The build from three fp32 device tables [n, T, D_m], which it may modify in place (``robust_loaders``: the noisy
        tables of one level).  ``labels`` [n] and ``ids`` are host arrays; ``start`` is the text's first-nonzero rows when the
        caller has them already; ``positions`` maps a row of the tables to its position in the split (``kept``)."""
        self = cls.__new__(cls)
        self.device, self.data_type, self.t_len = tables[0].device, data_type, tables[0].shape[1]
        self._build(list(tables), labels, ids, z_norm, vision_norm, start, positions)
        return self

    def _build(self, tables, labels, ids, z_norm, vision_norm, start=None, positions=None):
        from umlh import seqload
        with torch.cuda.device(self.device):
            tables[1].masked_fill_(tables[1] == float("-inf"), 0.0)                   # get_data.py:182
            tables, start, keep, self.lengths = _drop_textless(tables, start, "AffectTable: every sample's text is all zero")
            if vision_norm:                                                          # get_data.py:185-191
                seqload.column_standardize(tables[0], out=tables[0])
            if z_norm:                                                                # get_data.py:223-226
                for t in tables:
                    seqload.standardize_(t, start)
        self.tables, self.start = tables, start
        self.kept = keep if positions is None else np.asarray(positions)[keep]
        self.dims = tuple(t.shape[2] for t in tables)
        lab = labels[keep]
        if self.data_type in ("humor", "sarcasm"):                                    # get_data.py:238-243, task=None
            lab = np.where(lab < 1, -1.0, 1.0)
        self.labels = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.float32)).view(-1, 1)
        self.ids = ids[keep] if ids is not None else None

    def __len__(self):
        return int(self.kept.size)


def _copy_generator(g):
    if g is None:
        return None
    c = torch.Generator(device=g.device)
    c.set_state(g.get_state())
    return c


class _BatchOrder:
    """One epoch of a SequenceSampler.  ``order`` is the epoch's whole index stream once the first batch has been asked for."""

    def __init__(self, sampler):
        self.n, self.batch_size, self.shuffle = sampler.n, sampler.batch_size, sampler.shuffle
        self.generator, self.order, self.pos, self.dry = sampler.generator, None, 0, False
        # torch's loader iterator draws its base seed when it is made, from the loader's generator (None: the global one)
        torch.empty((), dtype=torch.int64).random_(generator=sampler.generator)

    def __iter__(self):
        return self

    def _first_request(self):
        if not self.shuffle:
            self.order = list(range(self.n))
            return
        if self.generator is None:                            # RandomSampler without a generator: a private one, seeded globally
            self.generator = torch.Generator()
            self.generator.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        self.order = torch.randperm(self.n, generator=self.generator).tolist()

    def __next__(self):
        if self.order is None:
            self._first_request()
        if self.dry:
            raise StopIteration
        left = self.n - self.pos
        if left < self.batch_size:                            # the index stream runs dry inside this request
            self.dry = True
            if self.shuffle:
                torch.randperm(self.n, generator=self.generator)      # RandomSampler's remainder draw, [: n % n] of it
            if left == 0:
                raise StopIteration
        batch = self.order[self.pos:self.pos + self.batch_size]
        self.pos += len(batch)
        return batch


class SequenceSampler:
    """The batch order of ``torch.utils.data.DataLoader(dataset of n, batch_size, shuffle, generator=generator,
    drop_last=False)`` as lists of indices, draw for draw.  Pure host code: no device, no library.

    With a generator GIVEN (the reference's train loaders: ``Generator().manual_seed(42)``) torch's protocol is
      * ``iter()`` draws the iterator's base seed from the generator;
      * the first batch request draws ``randperm(n)`` from the same generator -- no private generator, no seed draw;
      * RandomSampler's remainder draw, a second ``randperm(n)`` of which nothing is used, happens when the index stream runs
        dry: with a partial last batch while that batch is fetched, otherwise only when the iterator is asked past the end;
      * the generator's state carries over to the next epoch.
    A consequence for the reference's two train loaders, which both start from seed 42: under ``zip`` the second one is never
    asked past the end, so it skips the remainder draw whenever the first one makes it at the end.  When ``n % batch_size != 0``
    both make it inside the last batch and the two orders are identical in every epoch; when ``batch_size`` divides ``n`` the
    orders are equal in epoch 0 and differ from epoch 1 on.
    Without a generator the loader's draws come from the global one (base seed, and for ``shuffle`` the seed of a private
    generator per epoch), as torch's do.  ``copy.deepcopy`` copies the generator's state: the copy replays the epochs the
    original would run next and leaves the original's generator alone."""

    def __init__(self, n, batch_size, shuffle=False, generator=None):
        if n < 1 or batch_size < 1:
            raise ValueError(f"SequenceSampler: n={n} batch_size={batch_size} (need both >= 1)")
        self.n, self.batch_size, self.shuffle, self.generator = int(n), int(batch_size), bool(shuffle), generator

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        return _BatchOrder(self)

    def __deepcopy__(self, memo):
        return SequenceSampler(self.n, self.batch_size, self.shuffle, _copy_generator(self.generator))


class DeviceLoader:
    """What the device loaders share: a ``SequenceSampler`` for the order and the epoch driver.  An epoch uploads nothing
    before its first batch is asked for; then the order is known, ``_prepare(order)`` (int64 host tensor, the epoch's whole
    index stream) makes the epoch's device ids and host slices once, and ``_batch(epoch, i, lo, hi)`` yields batch ``i``, the
    entries ``lo:hi`` of the order, from what ``_prepare`` returned.  ``iter_index()`` runs the same epoch as host id lists.
    ``copy.deepcopy`` shares everything but the sampler, whose generator state it copies (``take_fixed_samples`` and
    ``train``'s effective-rank sample iterate deep copies of their loaders)."""

    def __init__(self, n, batch_size, shuffle, generator):
        self.batch_size = int(batch_size)
        self.sampler = SequenceSampler(n, batch_size, shuffle, generator)

    @property
    def generator(self):
        return self.sampler.generator

    def __len__(self):
        return len(self.sampler)

    def iter_index(self):
        return iter(self.sampler)

    def __iter__(self):
        return self._epoch(iter(self.sampler))                # the base-seed draw happens here, not at the first batch

    def _epoch(self, batches):
        bs, epoch = self.batch_size, None
        for i, ids in enumerate(batches):
            if epoch is None:                                 # the epoch's order is known now: one upload, host slices prepared
                epoch = self._prepare(torch.tensor(batches.order, dtype=torch.int64))
            yield self._batch(epoch, i, i * bs, i * bs + len(ids))

    def __deepcopy__(self, memo):
        c = copy.copy(self)
        c.sampler = copy.deepcopy(self.sampler, memo)
        return c


class SequenceLoader(DeviceLoader):
    """Batches of an ``AffectTable`` in the ``_process_1`` layout: ``([v, a, t], [lv, la, lt], inds, labels)`` with fp32 device
    blocks [b, Lmax, D_m] (Lmax = the longest trimmed sequence of that batch, zero padding behind every sequence), int64 device
    lengths [b], ``inds`` int64 [b, 1] and ``labels`` float32 [b, 1] on the host.  Entries of ``modalities`` (indices into
    vision, audio, text) that are not requested are None in both lists; the requested ones share one lengths tensor (the trim
    is common to the three modalities).

    An epoch uploads its order once, at the first batch, and then enqueues one ``umlh_seq_gather_pad`` launch per batch on the
    current stream; the host side of a batch is three slices."""

    def __init__(self, table, batch_size, shuffle=False, generator=None, modalities=(0, 1, 2)):
        self.table = table
        self.modalities = tuple(sorted(set(int(m) for m in modalities)))
        if not self.modalities or self.modalities[0] < 0 or self.modalities[-1] > 2:
            raise ValueError(f"SequenceLoader: modalities={modalities!r} (indices into vision, audio, text)")
        super().__init__(len(table), batch_size, shuffle, generator)

    def _prepare(self, order):
        from umlh import seqload
        tb = self.table
        sources = [tb.tables[m] if m in self.modalities else None for m in range(3)]
        t_out = np.maximum.reduceat(tb.lengths[order.numpy()], np.arange(0, len(order), self.batch_size))
        return seqload.gather_pad, sources, order, order.to(tb.device), tb.labels[order], t_out

    def _batch(self, epoch, i, lo, hi):
        gather_pad, sources, order, order_dev, labels, t_out = epoch
        blocks, lengths = gather_pad(sources, self.table.start, order_dev[lo:hi], int(t_out[i]))
        return blocks, [None if b is None else lengths for b in blocks], order[lo:hi].view(-1, 1), labels[lo:hi]


class LevelSequence:
    """A lazy sequence of loaders over noise levels.  ``build(level)`` makes one level's tables from ``base``, the clean
    device tables, which stay; ``loader(built)`` is an unshuffled loader over what it returned.  A level is built when its
    loader is first asked for, and only the latest one is kept: the previous level is released before the next is built.
    ``table(level)`` / ``tables(level)`` give what ``build`` made for that level (from the cache when it is the latest)."""

    def __init__(self, n, build, loader, base=None):
        self._n, self._build, self._loader, self.base = int(n), build, loader, base
        self._last = (None, None)

    def __len__(self):
        return self._n

    def table(self, level):
        if self._last[0] == level:
            return self._last[1]
        self._last = (None, None)                               # release the previous level before this one is built
        self._last = (level, self._build(level))
        return self._last[1]

    tables = table

    def __getitem__(self, level):
        if isinstance(level, slice):
            return [self[i] for i in range(len(self))[level]]
        level = int(level)
        if level < 0:
            level += len(self)
        if not 0 <= level < len(self):
            raise IndexError(level)
        return self._loader(self.table(level))


def get_dataloader(data, batch_size=32, train_shuffle=True, data_type="mosi", z_norm=False, vision_norm=False, device=None,
                   **options):
    """The reference's ``get_dataloader`` (get_data.py:268-416): ``(train, valid, test)`` SequenceLoaders.  ``data``: the
    ``{'train', 'valid', 'test'}`` dict of splits, or the path of its pickle.  The train loader shuffles with a generator seeded
    42 when ``train_shuffle`` (get_data.py:313-319); valid and test run in order.  Every split is normalised with its own
    statistics, as there."""
    _refuse_unsupported("get_dataloader", options)
    data = _open_pickle(data)
    tables = {s: AffectTable(data[s], data_type=data_type, z_norm=z_norm, vision_norm=vision_norm, device=device)
              for s in ("train", "valid", "test")}
    g = torch.Generator().manual_seed(42) if train_shuffle else None
    return (SequenceLoader(tables["train"], batch_size, shuffle=train_shuffle, generator=g),
            SequenceLoader(tables["valid"], batch_size), SequenceLoader(tables["test"], batch_size))


ROBUST_FAMILIES = {"robust_vision": ((0,), 10.0), "robust_audio": ((1,), 10.0), "robust_timeseries": ((0, 1, 2), 30.0)}


def robust_loaders(data, family, batch_size=32, data_type="mosi", z_norm=False, vision_norm=False, device=None, levels=10,
                   rng=None, per_step=False):
    """The noisy test sets of one family of the reference's ``get_dataloader(robust_test=True)`` (get_data.py:349-404):
    a sequence of ``levels`` unshuffled SequenceLoaders over the test split of ``data`` (the dict of splits or its pickle's
    path).  ``family``: 'robust_vision' / 'robust_audio' (that modality at noise level i / 10, the others clean) or
    'robust_timeseries' (all three in one call at i / 30: the draws are eps for vision, audio, text, then the drops for
    vision, audio, text); 'robust_text' needs raw words and GloVe vectors and raises NotImplementedError.
    Per level: the test split after the drop of text-less samples, Gaussian noise and structured drop with one draw per
    sample (``per_step``: per time step, see ``multibench.robustness``), then the normal build -- the second drop, ``-inf``,
    ``vision_norm`` and the front trim all see the noisy tables.  ``rng``: a numpy RandomState, an int seed, or None for numpy's
    global state (the reference).  All host draws happen here, in level order; a level's table is built when its loader is
    first asked for."""
    from .robustness import _draw, _perturb, _rng
    if family == "robust_text":
        raise NotImplementedError("robust_loaders: 'robust_text' needs the raw words and GloVe vectors of the test split "
                                  "(text_robust.py, get_rawtext, _glove_embeddings); only the time-series families are implemented")
    if family not in ROBUST_FAMILIES:
        raise ValueError(f"robust_loaders: unknown family {family!r} (known: {sorted(ROBUST_FAMILIES)})")
    split = _open_pickle(data)["test"]
    noisy, scale = ROBUST_FAMILIES[family]
    arrays, bad = _affect_arrays(split)
    if bad is not None:
        raise ValueError(f"robust_loaders: the test split's tables have shapes {[a.shape for a in arrays]}; expected [N, T, D_m]")
    t_len = arrays[0].shape[1]
    dev = _device(device)
    with torch.cuda.device(dev):                                # the first drop; audio keeps its -inf: noise comes before that
        base, clean_start, kept, _ = _drop_textless(_upload(arrays, dev), None, "robust_loaders: every test sample's text is all zero")
    g = _rng(rng)                                               # one stream for all levels
    counts = [(int(kept.size), t_len) if per_step else int(kept.size) for _ in noisy]
    dtypes = [arrays[m].dtype for m in noisy]
    draws = [_draw(g, counts, i / scale, True, True, dtypes) for i in range(int(levels))]
    labels = np.asarray(split["labels"]).reshape(-1)[kept]
    ids = np.asarray(split["id"])[kept] if "id" in split else None

    def build(level):
        """The AffectTable of one level (get_data.py:349-404 for that level, then Affectdataset)."""
        tables, start = [], clean_start
        with torch.cuda.device(dev):
            for m, x in enumerate(base):
                if m not in noisy:
                    tables.append(x.clone())                    # the build works in place
                    continue
                eps, keep = draws[level][noisy.index(m)]
                if m == 2:                                      # the trim and the second drop come from the noisy text
                    start = torch.empty(x.shape[0], dtype=torch.int32, device=dev)
                tables.append(_perturb(x, eps, keep, per_step=per_step, start_out=start if m == 2 else None))
        return AffectTable._from_device(tables, labels, ids, data_type, z_norm, vision_norm, start, kept)

    return LevelSequence(len(draws), build, lambda table: SequenceLoader(table, batch_size), base)


def _build_model(indims, zdim, modality, lr, infoNCE_loss, pos_embd, pos_learnable, dev):
    """The UML model of main.py:104-122 on ``dev`` and its Adam: the shared encoder is constructed first, then the two
    in-projections and the two decoders (the order in which the initialisation draws from torch's global generator)."""
    from .models import UML, Linear, Transformer
    encoder = Transformer(zdim, zdim, nhead=5, num_layers=5, conv1d=True, out_last=False, pos_embd=pos_embd,
                          pos_learnable=pos_learnable, max_len=128)
    model = UML(Linear(indims[0], zdim), Linear(indims[1], zdim), encoder, [Linear(zdim, indims[0]), Linear(zdim, indims[1])],
                modality=modality, infoNCE_loss=infoNCE_loss).to(dev)
    return model, torch.optim.Adam(model.parameters(), lr=lr)


def build_run(ds_name, data, zdim, modality="xy", lr=1e-4, infoNCE_loss=False, pos_embd=False, pos_learnable=False, device=None):
    """Loaders, model and optimizer wired as the reference's main.py:66-122 for ``ds_name`` (a key of ``DATASETS``): two
    shuffled train loaders (both seeded 42; they share one table), the three unshuffled evaluation loaders, the UML model on
    the device and Adam.  ``data``: the pickle's dict or its path.  Returns a dict with 'train_loader', 'train_loader_2',
    'eval_config' (the batch lists ``train`` expects, freq 100), 'model', 'optimizer', 'indims' and 'batch_size'."""
    if ds_name not in DATASETS:
        raise NotImplementedError(f"build_run: dataset {ds_name!r} (known: {sorted(DATASETS)})")
    cfg = DATASETS[ds_name]
    dev = _device(device)
    data = _open_pickle(data)
    kw = {"batch_size": cfg["batch_size"], "data_type": cfg["data_type"], "vision_norm": cfg["vision_norm"], "device": dev}
    train_loader, valid, test = get_dataloader(data, train_shuffle=True, **kw)
    train_loader_2 = SequenceLoader(train_loader.table, cfg["batch_size"], shuffle=True, generator=torch.Generator().manual_seed(42))
    eval_train = SequenceLoader(train_loader.table, cfg["batch_size"])
    indims = cfg["indims"]
    model, optimizer = _build_model(indims, zdim, modality, lr, infoNCE_loss, pos_embd, pos_learnable, dev)
    return {"train_loader": train_loader, "train_loader_2": train_loader_2, "model": model, "optimizer": optimizer,
            "eval_config": {"train": list(eval_train), "val": list(valid), "test": list(test), "freq": 100},
            "indims": indims, "batch_size": cfg["batch_size"]}
