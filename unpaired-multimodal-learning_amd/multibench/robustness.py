"""The reference's time-series noise (MultiBench/robustness/timeseries_robust.py) on [n, T, d] device tables: the draws on the
host, in the reference's order and from numpy's legacy generator, the arithmetic in one HIP launch per table
(``umlh.seqload.perturb``).

What the reference does, as opposed to what its docstrings say: ``white_noise`` adds ONE normal draw to every axis-0 slice of
every array of the list, ``structured_drop`` zeroes an axis-0 slice of one array when one uniform draw is below p (the arrays
drop independently), and all draws of one step precede the next step's.  Handed whole [N, T, D] tables, as get_data.py:349-404
does, the slice that shares a draw is the sample; handed one sample's [T, D] arrays it is the time step (``per_step``).

The sum: numpy adds the Python float of a draw to a float32 slice in float32, the draw rounded to float32 first, and to a
float64 slice in float64.  Both are ``float32(float64(x) + e)`` of the kernel -- with e the draw rounded through float32 in the
first case (the fp64 sum of two fp32 values rounds to fp32 as their fp32 sum does) and the draw itself in the second.
``table_dtype`` names the case; the device tables here are fp32, so float32 is the default.

``random_drop`` draws one host uniform per element in the reference; here the mask comes from the project's counter stream
(``seed``), which is declared NOT draw-compatible.  The families of get_data.py use ``rand_drop=False``."""
from __future__ import annotations

import numpy as np
import torch


def _rng(rng):
    if rng is None:
        return np.random                                       # the global legacy state, which is what the reference draws from
    if isinstance(rng, np.random.RandomState):
        return rng
    if isinstance(rng, (int, np.integer)):
        return np.random.RandomState(int(rng))
    raise TypeError(f"rng: a numpy RandomState, an int seed or None, not {type(rng).__name__}")


def _round_eps(eps, dtype):
    return eps.astype(np.float32).astype(np.float64) if np.dtype(dtype) == np.float32 else eps


def draw_timeseries_noise(counts, noise_level, gaussian_noise=True, struct_drop=True, rng=None, table_dtype=np.float32):
    """The host draws of one ``add_timeseries_noise`` call, pure numpy.  ``counts``: per array of the list its number of units
    n (one draw per sample: the reference's call on whole tables), or a pair (n, T) for all of them (one draw per time step:
    for each sample in order, the reference's call on that sample's list of [T, d] arrays).  Returns per array
    ``(eps, keep)``: float64 and uint8 arrays of shape [n] or [n, T], None for a step that is off.  ``keep`` is 0 where the
    reference's ``random_sample() < noise_level`` holds.  ``table_dtype``: one dtype, or one per array, of the arrays the
    reference would add into (see the module's docstring).  ``rng`` is resolved here; ``_draw`` is the same on a resolved
    stream, for callers that run one stream through several calls."""
    g, counts = _rng(rng), list(counts)
    dtypes = list(table_dtype) if isinstance(table_dtype, (list, tuple)) else [table_dtype] * len(counts)
    if len(dtypes) != len(counts):
        raise ValueError(f"draw_timeseries_noise: {len(dtypes)} dtypes for {len(counts)} arrays")
    if any(isinstance(c, (tuple, list)) for c in counts):
        shapes = {tuple(int(v) for v in c) for c in counts}
        if len(shapes) != 1 or len(next(iter(shapes))) != 2:
            raise ValueError(f"draw_timeseries_noise: per-step counts must be one (n, T) for every array, got {counts}")
    return _draw(g, counts, float(noise_level), gaussian_noise, struct_drop, dtypes)


def _draw(g, counts, p, gaussian_noise, struct_drop, dtypes):
    """``draw_timeseries_noise`` on the resolved stream ``g`` (``_rng``), with checked ``counts`` and one dtype per array."""
    if not (counts and isinstance(counts[0], (tuple, list))):
        eps = [g.normal(0, p, size=int(c)) if gaussian_noise else None for c in counts]
        keep = [(~(g.random_sample(int(c)) < p)).astype(np.uint8) if struct_drop else None for c in counts]
    else:
        (n, T), k = (int(v) for v in counts[0]), len(counts)
        e = np.empty((n, k, T)) if gaussian_noise else None
        u = np.empty((n, k, T)) if struct_drop else None
        for s in range(n):                                     # one reference call per sample: its normals, then its uniforms
            if gaussian_noise:
                e[s] = g.normal(0, p, size=(k, T))
            if struct_drop:
                u[s] = g.random_sample((k, T))
        eps = [np.ascontiguousarray(e[:, a]) if gaussian_noise else None for a in range(k)]
        keep = [(~(u[:, a] < p)).astype(np.uint8) if struct_drop else None for a in range(k)]
    return [(None if e_ is None else _round_eps(e_, dt), k_) for e_, k_, dt in zip(eps, keep, dtypes)]


def _perturb(x, eps, keep, **options):
    """One table's host draws uploaded to its device and its one ``umlh_seq_perturb`` launch (``umlh.seqload.perturb``)."""
    from umlh import seqload
    up = lambda a: None if a is None else torch.from_numpy(a).to(x.device)
    return seqload.perturb(x, up(eps), up(keep), **options)


def _counts(tests, per_step):
    tests = list(tests)
    for x in tests:
        if not isinstance(x, torch.Tensor) or x.ndim != 3:
            raise ValueError("robustness: expected a list of [n, T, d] device tables")
    return tests, [(x.shape[0], x.shape[1]) if per_step else x.shape[0] for x in tests]


def add_timeseries_noise(tests, noise_level=0.3, gaussian_noise=True, rand_drop=True, struct_drop=True, rng=None, seed=0,
                         per_step=False, table_dtype=np.float32):
    """The reference's function of this name on a list of fp32 device tables [n, T, d_i]; returns new tables, the inputs are
    not modified (the reference modifies its arguments).  The three steps commute element by element once the draws are
    fixed -- a dropped element is 0 whatever was added before -- so one launch per table applies them together.  ``rng``: the
    source of the host draws (RandomState, int seed, None for numpy's global state); ``seed``: the counter stream of
    ``rand_drop``, table i uses ``seed + i``."""
    tests, counts = _counts(tests, per_step)
    draws = draw_timeseries_noise(counts, noise_level, gaussian_noise, struct_drop, rng, table_dtype)
    elem_p = min(max(float(noise_level), 0.0), 1.0) if rand_drop else 0.0     # a probability: `uniform < p` beyond [0, 1] is 0 or 1
    return [_perturb(x, eps, keep, per_step=per_step, elem_p=elem_p, seed=int(seed) + i)
            for i, (x, (eps, keep)) in enumerate(zip(tests, draws))]


def white_noise(data, p, rng=None, per_step=False, table_dtype=np.float32):
    """Zero-mean Gaussian noise of standard deviation p, one draw per unit."""
    return add_timeseries_noise(data, p, True, False, False, rng, 0, per_step, table_dtype)


def random_drop(data, p, seed=0):
    """Every element becomes 0 with probability p (counter stream ``seed + i`` for table i)."""
    return add_timeseries_noise(data, p, False, True, False, None, seed)


def structured_drop(data, p, rng=None, per_step=False):
    """Every unit of every table becomes 0 with probability p, the tables independently."""
    return add_timeseries_noise(data, p, False, False, True, rng, 0, per_step)
