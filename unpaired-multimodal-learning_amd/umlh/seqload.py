"""The kernels of the affect datasets' device loader (umlh_kernels_seqload.hip; C ABI: ``umlh_seq_first_nonzero``,
``umlh_seq_column_standardize``, ``umlh_seq_standardize``, ``umlh_seq_gather_pad``, ``umlh_seq_perturb``) as thin torch
wrappers: what MultiBench/datasets/affect/get_data.py does per sample (front trim, vision_norm, z_norm) and per batch
(_process_1's pad_sequence) on the host, and the time-series noise of its robustness test sets.  Every call enqueues on ``torch.cuda.current_stream`` and returns device tensors; nothing is read
back.  There is no CPU compute path.  The loader built on them is ``multibench.data``.
The second part holds the kernels of the MIMIC loader (umlh_kernels_tabular.hip; ``umlh_tab_standardize``, ``umlh_tab_perturb``,
``umlh_rows_gather``): MultiBench/datasets/mimic/get_data.py and robustness/tabular_robust.py on [n, d] device matrices; the loader
built on them is ``multibench.mimic``."""
from __future__ import annotations

import ctypes as C

import torch

from . import _glue as glue
from ._lib import check, load_library

MAX_SOURCES = 3          # UMLH_SEQ_GATHER_MAX_SOURCES
MAX_BATCH = 65535


def _table(x: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.ndim != 3 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous fp32 device tensor [n, T, d], got "
                         f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    if min(x.shape) < 1:
        raise ValueError(f"{what}: empty table {tuple(x.shape)}")
    return x


def _start(start: torch.Tensor, n: int, dev: torch.device, what: str) -> torch.Tensor:
    if not isinstance(start, torch.Tensor) or start.dtype != torch.int32 or start.device != dev or tuple(start.shape) != (n,) \
            or not start.is_contiguous():
        raise ValueError(f"{what}: start must be a contiguous int32 tensor [{n}] on {dev}")
    return start


def first_nonzero(x: torch.Tensor) -> torch.Tensor:
    """int32 [n]: per sample of the [n, T, d] table the row of its first element != 0 (NaN counts, -0.0 does not), T when it
    has none -- ``text.nonzero()[0][0]`` of the reference."""
    x = _table(x, "first_nonzero")
    n, T, d = x.shape
    start = torch.empty(n, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        check(load_library().umlh_seq_first_nonzero(x.data_ptr(), n, T, d, start.data_ptr(), glue.stream(x.device)),
              "umlh_seq_first_nonzero")
    return start


def column_standardize(x: torch.Tensor, out: torch.Tensor | None = None):
    """``(x - mu) / sigma`` per column over all n * T rows of the [n, T, d] table (population std, fp64 statistics): the
    reference's vision_norm.  ``out=x`` works in place; default: a new table.  Returns (out, stats) with stats the float64
    device tensor [2, d] = mean | std.  A zero std is not special-cased."""
    x = _table(x, "column_standardize")
    n, T, d = x.shape
    out = torch.empty_like(x) if out is None else _table(out, "column_standardize (out)")
    if out.shape != x.shape or out.device != x.device:
        raise ValueError(f"column_standardize: out {tuple(out.shape)} on {out.device} for x {tuple(x.shape)} on {x.device}")
    stats = torch.empty((2, d), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        scratch, nbytes = glue.scratch("umlh_seq_column_standardize_scratch", x.device, rows=n * T, d=d)
        check(load_library().umlh_seq_column_standardize(x.data_ptr(), n * T, d, d, out.data_ptr(), d, stats.data_ptr(),
                                                         scratch.data_ptr(), nbytes, glue.stream(x.device)),
              "umlh_seq_column_standardize")
    return out, stats


def standardize_(x: torch.Tensor, start: torch.Tensor) -> torch.Tensor:
    """In place: per sample and column over the rows ``start[i]..T-1`` of the [n, T, d] table,
    ``nan_to_num((x - mean) / std)`` with the unbiased std (fp64 statistics, fp32 arithmetic): the reference's z_norm.  A
    constant column and a length-1 sequence become all 0.  Returns ``x``."""
    x = _table(x, "standardize_")
    n, T, d = x.shape
    start = _start(start, n, x.device, "standardize_")
    with torch.cuda.device(x.device):
        check(load_library().umlh_seq_standardize(x.data_ptr(), n, T, d, start.data_ptr(), glue.stream(x.device)),
              "umlh_seq_standardize")
    return x


def _draws(a, dtype, units: int, dev: torch.device, name: str):
    if a is None:
        return 0
    if not isinstance(a, torch.Tensor) or a.dtype != dtype or a.device != dev or a.numel() != units or not a.is_contiguous():
        raise ValueError(f"perturb: {name} must be a contiguous {dtype} tensor of {units} entries on {dev}")
    return a.data_ptr()


def perturb(x: torch.Tensor, eps: torch.Tensor | None = None, keep: torch.Tensor | None = None, per_step: bool = False,
            elem_p: float = 0.0, seed: int = 0, out: torch.Tensor | None = None, start_out: torch.Tensor | None = None):
    """The reference's time-series noise (robustness/timeseries_robust.py) on the [n, T, d] table ``x``, one launch.  A unit is
    a sample, or a time step with ``per_step``; ``eps`` (float64) and ``keep`` (uint8) are device tensors with one entry per
    unit (n, or n * T), either may be None.  A unit with ``keep == 0`` is written as +0.0; otherwise an element becomes
    ``float32(float64(x) + eps[u])`` (``x`` itself, bit for bit, without ``eps``).  ``elem_p > 0`` also zeroes element i of the
    counter stream ``seed`` with that probability (the reference's random_drop; not numpy's draws).  ``out=x`` works in place;
    default: a new table.  ``start_out`` (int32 [n]) receives ``first_nonzero`` of the result from the same pass.
    Returns ``out``."""
    x = _table(x, "perturb")
    n, T, d = x.shape
    out = torch.empty_like(x) if out is None else _table(out, "perturb (out)")
    if out.shape != x.shape or out.device != x.device:
        raise ValueError(f"perturb: out {tuple(out.shape)} on {out.device} for x {tuple(x.shape)} on {x.device}")
    units = n * T if per_step else n
    eps_p = _draws(eps, torch.float64, units, x.device, "eps")
    keep_p = _draws(keep, torch.uint8, units, x.device, "keep")
    start_p = 0 if start_out is None else _start(start_out, n, x.device, "perturb").data_ptr()
    with torch.cuda.device(x.device):
        check(load_library().umlh_seq_perturb(x.data_ptr(), n, T, d, 1 if per_step else T, eps_p, keep_p, float(elem_p),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(), start_p, glue.stream(x.device)),
              "umlh_seq_perturb")
    return out


def gather_pad(sources, start: torch.Tensor, ids: torch.Tensor, t_out: int, outs=None, lengths: torch.Tensor | None = None):
    """One launch: the batch of the samples ``ids`` (int64 device tensor [b]) of up to three [n, T, d_m] tables, an entry of
    ``sources`` may be None (skipped).  Returns (blocks, lengths): blocks[m] is the fp32 [b, t_out, d_m] block with
    ``blocks[m][j, t] = sources[m][ids[j], start[ids[j]] + t]`` for t < len_j = min(T - start[ids[j]], t_out) and +0.0 behind
    (None for a skipped source), lengths the int64 [b] tensor of len_j.  An id outside [0, n) gives a zero block and length
    0.  ``outs`` / ``lengths``: destinations to write into instead of new tensors."""
    sources = list(sources)
    given = [s for s in sources if s is not None]
    if not 1 <= len(sources) <= MAX_SOURCES or not given:
        raise ValueError(f"gather_pad: {len(sources)} sources, {len(given)} given (need 1..{MAX_SOURCES} with at least one given)")
    for s in given:
        _table(s, "gather_pad")
    dev, (n, T) = given[0].device, given[0].shape[:2]
    if any(s.device != dev or tuple(s.shape[:2]) != (n, T) for s in given):
        raise ValueError("gather_pad: the sources must share the device, n and T")
    start = _start(start, n, dev, "gather_pad")
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.device != dev or ids.ndim != 1 or not ids.is_contiguous():
        raise ValueError(f"gather_pad: ids must be a contiguous int64 tensor [b] on {dev}")
    b, t_out = ids.shape[0], int(t_out)
    if not 1 <= b <= MAX_BATCH or t_out < 1:
        raise ValueError(f"gather_pad: b={b} t_out={t_out} (need 1 <= b <= {MAX_BATCH}, t_out >= 1)")
    if outs is None:
        outs = [None if s is None else torch.empty((b, t_out, s.shape[2]), dtype=torch.float32, device=dev) for s in sources]
    else:
        outs = list(outs)
        for s, o in zip(sources, outs):
            if s is not None and (_table(o, "gather_pad (out)").shape != (b, t_out, s.shape[2]) or o.device != dev):
                raise ValueError(f"gather_pad: out {tuple(o.shape)} for a block {(b, t_out, s.shape[2])}")
    if lengths is None:
        lengths = torch.empty(b, dtype=torch.int64, device=dev)
    elif lengths.dtype != torch.int64 or lengths.device != dev or tuple(lengths.shape) != (b,) or not lengths.is_contiguous():
        raise ValueError(f"gather_pad: lengths must be a contiguous int64 tensor [{b}] on {dev}")
    k = len(sources)
    srcs = (C.c_void_p * k)(*[None if s is None else s.data_ptr() for s in sources])
    dsts = (C.c_void_p * k)(*[None if s is None else o.data_ptr() for s, o in zip(sources, outs)])
    dims = (C.c_int32 * k)(*[0 if s is None else s.shape[2] for s in sources])
    with torch.cuda.device(dev):
        check(load_library().umlh_seq_gather_pad(srcs, dims, k, n, T, start.data_ptr(), ids.data_ptr(), b, t_out, dsts,
                                                 lengths.data_ptr(), glue.stream(dev)), "umlh_seq_gather_pad")
    return [o if s is not None else None for s, o in zip(sources, outs)], lengths


# ---- MIMIC loader (umlh_kernels_tabular.hip; C ABI: umlh_tab_standardize, umlh_tab_perturb, umlh_rows_gather) ----
def _matrix(x, what: str, dtypes=(torch.float32,)) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.ndim != 2 or x.dtype not in dtypes or not x.is_cuda or x.stride(1) != 1 \
            or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise ValueError(f"{what}: expected a {' / '.join(str(t) for t in dtypes)} device matrix [n, d] with unit column stride, "
                         f"got {getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    if min(x.shape) < 1:
        raise ValueError(f"{what}: empty matrix {tuple(x.shape)}")
    return x


def _ld(x: torch.Tensor) -> int:
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


def tab_standardize(x: torch.Tensor, out: torch.Tensor | None = None):
    """get_data.py:38-51 of the MIMIC loader on the [rows, d] device matrix ``x`` (float32 or float64, row stride >= d):
    NaN and +-Inf count as 0, then ``(x - mu) / sigma`` per column with the population std, statistics and arithmetic in fp64,
    one rounding to fp32.  ``out=x`` works in place for a float32 ``x``; default: a new fp32 matrix.  ``x`` is not modified
    otherwise.  Returns (out, stats) with stats the float64 device tensor [2, d] = mean | std.  A zero std is not
    special-cased."""
    x = _matrix(x, "tab_standardize", (torch.float32, torch.float64))
    rows, d = x.shape
    out = torch.empty((rows, d), dtype=torch.float32, device=x.device) if out is None else _matrix(out, "tab_standardize (out)")
    if out.shape != x.shape or out.device != x.device:
        raise ValueError(f"tab_standardize: out {tuple(out.shape)} on {out.device} for x {tuple(x.shape)} on {x.device}")
    stats = torch.empty((2, d), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        scratch, nbytes = glue.scratch("umlh_tab_standardize_scratch", x.device, rows=rows, d=d)
        check(load_library().umlh_tab_standardize(x.data_ptr(), int(x.dtype == torch.float64), rows, d, _ld(x), out.data_ptr(),
                                                  _ld(out), stats.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(x.device)),
              "umlh_tab_standardize")
    return out, stats


def _mask(a, shape, dev: torch.device, name: str):
    if a is None:
        return 0
    if not isinstance(a, torch.Tensor) or a.dtype != torch.uint8 or a.device != dev or tuple(a.shape) != shape or not a.is_contiguous():
        raise ValueError(f"tab_perturb: {name} must be a contiguous uint8 tensor {list(shape)} on {dev}")
    return a.data_ptr()


def tab_perturb(x: torch.Tensor, drop: torch.Tensor | None = None, carry: torch.Tensor | None = None, p_drop: float = 0.0,
                p_carry: float = 0.0, seed: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """The reference's tabular noise (robustness/tabular_robust.py) on the fp32 [n, d] device matrix ``x``, one launch:
    ``drop`` (uint8 [n, d]) writes +0.0 where it is set, then ``carry`` (uint8 [n, d - 1], entry j - 1 for column j) copies
    the already updated left neighbour into column j -- what the reference's swap_entry does.  Both are device tensors of host
    draws in the reference's order; either may be None.  With a mask None, ``p_drop`` / ``p_carry`` > 0 take the decisions
    from the project's counter streams ``seed`` / ``seed + 1`` (not numpy's draws).  ``out=x`` works in place; default: a new
    matrix.  Returns ``out``."""
    x = _matrix(x, "tab_perturb")
    n, d = x.shape
    out = torch.empty((n, d), dtype=torch.float32, device=x.device) if out is None else _matrix(out, "tab_perturb (out)")
    if out.shape != x.shape or out.device != x.device:
        raise ValueError(f"tab_perturb: out {tuple(out.shape)} on {out.device} for x {tuple(x.shape)} on {x.device}")
    drop_p = _mask(drop, (n, d), x.device, "drop")
    carry_p = _mask(carry, (n, d - 1), x.device, "carry")
    with torch.cuda.device(x.device):
        check(load_library().umlh_tab_perturb(x.data_ptr(), n, d, _ld(x), drop_p, carry_p, float(p_drop), float(p_carry),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(), _ld(out), glue.stream(x.device)),
              "umlh_tab_perturb")
    return out


def rows_gather(sources, ids: torch.Tensor, outs=None):
    """One launch: the rows ``ids`` (int64 device tensor [b]) of up to three dense fp32 device tables that share n; a table
    may have any number of trailing dimensions (its row is their flattened words) and an entry of ``sources`` may be None
    (skipped).  Returns the blocks [b, *sources[m].shape[1:]] (None for a skipped source), ``blocks[m][j] = sources[m][ids[j]]``
    bit for bit; an id outside [0, n) gives a zero row.  ``outs``: destinations to write into instead of new tensors."""
    sources = list(sources)
    given = [s for s in sources if s is not None]
    if not 1 <= len(sources) <= MAX_SOURCES or not given:
        raise ValueError(f"rows_gather: {len(sources)} sources, {len(given)} given (need 1..{MAX_SOURCES} with at least one given)")
    for s in given:
        if not isinstance(s, torch.Tensor) or s.ndim < 2 or s.dtype != torch.float32 or not s.is_cuda or not s.is_contiguous() \
                or min(s.shape) < 1:
            raise ValueError(f"rows_gather: expected contiguous non-empty fp32 device tables [n, ...], got "
                             f"{getattr(s, 'dtype', type(s))} {tuple(getattr(s, 'shape', ()))}")
    dev, n = given[0].device, given[0].shape[0]
    if any(s.device != dev or s.shape[0] != n for s in given):
        raise ValueError("rows_gather: the sources must share the device and n")
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.device != dev or ids.ndim != 1 or not ids.is_contiguous():
        raise ValueError(f"rows_gather: ids must be a contiguous int64 tensor [b] on {dev}")
    b = ids.shape[0]
    if not 1 <= b <= MAX_BATCH:
        raise ValueError(f"rows_gather: b={b} (need 1 <= b <= {MAX_BATCH})")
    if outs is None:
        outs = [None if s is None else torch.empty((b, *s.shape[1:]), dtype=torch.float32, device=dev) for s in sources]
    else:
        outs = list(outs)
        for s, o in zip(sources, outs):
            if s is not None and (not isinstance(o, torch.Tensor) or o.dtype != torch.float32 or o.device != dev
                                  or tuple(o.shape) != (b, *s.shape[1:]) or not o.is_contiguous()):
                raise ValueError(f"rows_gather: out {tuple(getattr(o, 'shape', ()))} for a block {(b, *s.shape[1:])}")
    k = len(sources)
    srcs = (C.c_void_p * k)(*[None if s is None else s.data_ptr() for s in sources])
    dsts = (C.c_void_p * k)(*[None if s is None else o.data_ptr() for s, o in zip(sources, outs)])
    widths = (C.c_int32 * k)(*[0 if s is None else s[0].numel() for s in sources])
    with torch.cuda.device(dev):
        check(load_library().umlh_rows_gather(srcs, widths, k, n, ids.data_ptr(), b, dsts, glue.stream(dev)), "umlh_rows_gather")
    return [o if s is not None else None for s, o in zip(sources, outs)]
