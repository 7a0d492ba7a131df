"""What the robustness test sets compute (multibench/robustness.py, multibench.data.robust_loaders, include/umlh.h
``umlh_seq_perturb``), stated in numpy, and the fixture tests/golden/robust_noise.npz that holds what the
reference's own code gave for the same inputs (scripts/make_golden_robustness.py).

The kernel contract (``perturb``): a unit -- a sample, or a time step -- shares one draw; an element of a unit with keep == 0 is
ASSIGNED +0.0; otherwise it is float32(float64(x) + eps[u]), one fp64 add and one rounding, and x itself without eps; ``start`` is
the first row of the result with an element != 0.

The draws (``draws``): scalar calls on numpy's legacy generator in the reference's order -- all normals of a call, array by
array, then all uniforms.  numpy adds the Python float of a draw to a float32 slice in float32, the draw rounded to float32
first, and to a float64 slice in float64; the fp64 sum of two fp32 values rounds to fp32 as their fp32 sum does, so both are the
kernel's expression, with the draw rounded through float32 in the first case (``round_eps``).

``variant`` names one deliberately wrong reading; tests/test_robust_cpu.py shows that each is caught on the fixture.

The families (``family_table``): first drop, noise, then ``_seqload_ref.build_table`` (second drop, -inf, vision_norm, trim)."""
import numpy as np

import _seqload_ref as R
from conftest import load_golden

VARIANTS = ("per_step_noise", "shared_drop", "multiply_drop", "fp32_add", "drops_first")
LEVELS_P = (0.0, 0.3, 1.0)
FAMILIES = {"robust_vision": ((0,), 10.0), "robust_audio": ((1,), 10.0), "robust_timeseries": ((0, 1, 2), 30.0)}
RECORDED = (0, 3, 9)
# log2 of the bound on max |got - ref64| / max |ref64| per block of the vision_norm case, per family: 8 times the reference's own
# fp32 error against the statement, rounded up to a power of two (tests/test_robust_cpu.py measures it and holds this table to it)
VNORM_BOUND_LOG2 = {"robust_vision": -15, "robust_audio": -17, "robust_timeseries": -17}


def load_fixture():
    return load_golden("robust_noise")


def noise_inputs(fx, case):
    out, k = [], 0
    while f"noise/{case}/in{k}" in fx:
        out.append(fx[f"noise/{case}/in{k}"])
        k += 1
    return out


def noise_outputs(fx, case, li):
    return [fx[f"noise/{case}/p{li}/out{k}"] for k in range(len(noise_inputs(fx, case)))]


def family_batches(fx, case, family, level):
    n = int(fx[f"fam/{case}/{family}/{level}/batches"])
    key = lambda i, what: fx[f"fam/{case}/{family}/{level}/{i}/{what}"]
    return [([key(i, f"x{m}") for m in range(3)], [key(i, f"l{m}") for m in range(3)], key(i, "inds"), key(i, "labels"))
            for i in range(n)]


def test_split(fx):
    return {k: fx[f"fam/data/test/{k}"] for k in R.MODALITIES + ("labels", "id")}


def round_eps(eps, dtype):
    return eps.astype(np.float32).astype(np.float64) if np.dtype(dtype) == np.float32 else eps


def perturb(x, eps=None, keep=None, variant=None):
    """The kernel contract on one float32 [n, T, d] table.  eps / keep: [n] (unit = sample) or [n, T] (unit = time step), or
    None.  Returns (float32 result, int64 start [n])."""
    x = np.asarray(x, dtype=np.float32)
    shape = lambda a: a.reshape(a.shape + (1,) * (3 - a.ndim))
    with np.errstate(all="ignore"):
        if eps is None:
            out = x.copy()
        elif variant == "fp32_add":
            out = x + shape(eps).astype(np.float32)
        else:
            out = (x.astype(np.float64) + shape(np.asarray(eps, dtype=np.float64))).astype(np.float32)
        if keep is not None:
            k = np.broadcast_to(shape(np.asarray(keep)) != 0, x.shape)
            out = out * k.astype(np.float32) if variant == "multiply_drop" else np.where(k, out, np.float32(0.0))
    return out.astype(np.float32), R.first_rows(out)


def draws(counts, p, rng, variant=None, t_len=None, per_step=False):
    """Scalar draws on a numpy RandomState in the reference's order (gaussian_noise and struct_drop on, rand_drop off).
    counts: samples per array; ``t_len``: the T of the tables.  Sample units: the normals of array 0, 1, ..., then the
    uniforms of array 0, 1, ...  ``per_step``: for each sample in order, the normals of its arrays' T rows, then the uniforms.
    Returns per array (eps float64, keep uint8), [n] or [n, T]."""
    k, counts = len(counts), [int(c) for c in counts]
    normal = lambda size: np.array([rng.normal(0, p) for _ in range(size)])
    uniform = lambda size: np.array([rng.random_sample() for _ in range(size)])
    if per_step:
        n = counts[0]
        e, u = [np.empty((n, t_len)) for _ in range(k)], [np.empty((n, t_len)) for _ in range(k)]
        for s in range(n):
            for a in range(k):
                e[a][s] = normal(t_len)
            for a in range(k):
                u[a][s] = uniform(t_len)
    else:
        def normals():
            if variant == "per_step_noise":
                return [normal(c * t_len).reshape(c, t_len) for c in counts]
            return [normal(c) for c in counts]

        def uniforms():
            if variant == "shared_drop":
                return [uniform(counts[0])] * k
            return [uniform(c) for c in counts]
        if variant == "drops_first":
            u = uniforms()
            e = normals()
        else:
            e = normals()
            u = uniforms()
    return [(a, (~(b < p)).astype(np.uint8)) for a, b in zip(e, u)]


def add_timeseries_noise(tables, p, rng, per_step=False, variant=None):
    """The reference's call (rand_drop=False) on a list of [n, T, d] arrays, restated: the float32 results.  A float64 array
    stands for itself rounded to float32 (the fixture's are exact) and takes the unrounded draws: the reference adds into it
    in float64 and its loader rounds once, later."""
    tables = [np.asarray(a) for a in tables]
    d = draws([a.shape[0] for a in tables], p, rng, variant, tables[0].shape[1], per_step)
    return [perturb(a.astype(np.float32), round_eps(eps, a.dtype), keep, variant)[0] for a, (eps, keep) in zip(tables, d)]


def family_levels(split, family, seed, levels=10):
    """Per level the split dict the build sees: first drop, then the noise of that level (one stream of draws per family)."""
    arrays = [np.asarray(split[m]).astype(np.float32) for m in R.MODALITIES]
    kept = np.flatnonzero(R.first_rows(arrays[2]) < arrays[2].shape[1])
    arrays = [a[kept] for a in arrays]
    noisy, scale = FAMILIES[family]
    rng = np.random.RandomState(seed)
    out = []
    for i in range(levels):
        res = add_timeseries_noise([arrays[m] for m in noisy], i / scale, rng)
        t = {m: a for m, a in zip(R.MODALITIES, arrays)}
        for m, r in zip(noisy, res):
            t[R.MODALITIES[m]] = r
        t["labels"] = np.asarray(split["labels"])[kept]
        t["id"] = np.asarray(split["id"])[kept]
        t["positions"] = kept
        out.append(t)
    return out


def family_table(level_split, data_type="mosi", vision_norm=False):
    """``_seqload_ref.build_table`` of one level's split; 'kept' becomes positions in the original split."""
    t = R.build_table(level_split, data_type, False, vision_norm)
    t["kept"] = level_split["positions"][t["kept"]]
    return t


def vnorm_bound(family):
    return 2.0 ** VNORM_BOUND_LOG2[family]


same_bits = R.same_bits
