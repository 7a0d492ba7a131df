"""The contract of ``umlh_rollout`` and ``umlh_seq_spectrum`` restated in numpy: the closed form of the reference's rollout
(MultiBench/train.py:268-292) at T = 1, where the causal softmax over one key is exactly 1 and attention is
out_proj(v_proj(h)), and the spectrum of train.py:248-251.  ``rollout`` evaluates it in float64 (the yardstick) or, with
``dtype=np.float32``, in fp32 (what any fp32 implementation of the same formulas reaches: the source of the bounds).

A parameter set is a dict: w_in [Z, D], b_in [Z], conv [Z, Z] or None, pos0 [Z] or None, layers = list of 12-tuples in the order
of ``multibench.encoder.layer_params`` (in_w [3Z, Z], in_b, out_w, out_b, w1 [F, Z], b1, w2 [Z, F], b2, g1, be1, g2, be2), eps,
w_out [D, Z], b_out [D].

Criterion table.  Per generated step s, err(s) = max|got[:, s] - ref64[:, s]| / max|ref64[:, s]|; "fp32" is the largest err(s) of
the fp32 numpy evaluation over all steps and the four data seeds of DATA_SEEDS, "growth" the largest ratio of a seed's worst
err(s) to its err(1), bound = 8 x fp32 rounded up to a power of two.  Re-measured by
tests/test_rollout_cpu.py::test_criterion_table_is_current.  The seed row (s = 0) is a copy and must be exact.

    case                        fp32   growth   bound
    z10_d5_long             2.27e-06     6.3   2^-15
    z10_d7_nopos            6.33e-06     8.7   2^-14
    z10_d1_one_row          1.46e-07     4.0   2^-19
    z40_d35                 5.29e-07     2.1   2^-17
    z40_d35_noconv_sin      3.55e-07     2.7   2^-18
    z40_d371                1.98e-06     5.8   2^-15
    z300_d300               1.37e-06     2.4   2^-16
    z300_d35_ff72           1.07e-06     2.3   2^-16
    z300_d300_long          5.60e-06     9.2   2^-14
    z40_d35_steps0                 -       -   exact
    z40_d35_steps1          3.08e-07     1.0   2^-18
    z10_d5_nolayers         2.93e-07     1.8   2^-18
    z10_d5_eps              1.03e-06     4.6   2^-16

z10_d7_nopos is the long-horizon case: its rows are still 1.3 max|ref| apart after 49 steps (the other 49-step cases collapse
onto one trajectory, where a comparison only sees that trajectory).  z10_d5_eps runs with eps = 1e-2 (EPS): with nn's 1e-5
dropping eps moves the values by less than fp32 rounding does, so "eps dropped" can only be told apart there."""
import numpy as np

VARIANTS = ("pos_row1", "q_rows", "pre_norm", "no_conv", "no_eps")


def _ln(h, g, b, eps):
    mu = h.mean(axis=-1, keepdims=True)
    var = ((h - mu) ** 2).mean(axis=-1, keepdims=True)
    return ((h - mu) / np.sqrt(var + h.dtype.type(eps)) * g + b).astype(h.dtype)


def cast(p, dtype):
    c = lambda a: None if a is None else np.asarray(a, dtype=dtype)
    q = {k: c(p.get(k)) for k in ("w_in", "b_in", "conv", "pos0", "pos1", "w_out", "b_out")}
    q["layers"] = [tuple(c(t) for t in layer) for layer in p["layers"]]
    q["eps"] = float(p["eps"])
    return q


def step(p, cur, variant=None):
    """One generated frame: cur [n, D] -> [n, D], in the dtype of ``p``'s arrays (use ``cast`` first)."""
    Z = p["w_in"].shape[0]
    eps = 0.0 if variant == "no_eps" else p["eps"]
    h = cur @ p["w_in"].T + p["b_in"]
    if p["conv"] is not None and variant != "no_conv":
        h = h @ p["conv"].T
    pos = p["pos1"] if variant == "pos_row1" else p["pos0"]
    if pos is not None:
        h = h + pos
    lo = 0 if variant == "q_rows" else 2 * Z
    for in_w, in_b, out_w, out_b, w1, b1, w2, b2, g1, be1, g2, be2 in p["layers"]:
        if variant == "pre_norm":
            a = _ln(h, g1, be1, eps)
            h = h + ((a @ in_w[lo:lo + Z].T + in_b[lo:lo + Z]) @ out_w.T + out_b)
            a = _ln(h, g2, be2, eps)
            h = h + (np.maximum(a @ w1.T + b1, 0) @ w2.T + b2)
            continue
        a = (h @ in_w[lo:lo + Z].T + in_b[lo:lo + Z]) @ out_w.T + out_b
        h = _ln(h + a, g1, be1, eps)
        f = np.maximum(h @ w1.T + b1, 0) @ w2.T + b2
        h = _ln(h + f, g2, be2, eps)
    return h @ p["w_out"].T + p["b_out"]


def rollout(p, x0, steps, dtype=np.float64, variant=None):
    """[n, steps + 1, D]: the seed rows then ``steps`` generated frames."""
    q = cast(p, dtype)
    cur = np.asarray(x0, dtype=dtype)
    out = [cur]
    for _ in range(int(steps)):
        cur = step(q, cur, variant).astype(dtype)
        out.append(cur)
    return np.stack(out, axis=1)


def spectrum(x):
    """abs(rfft(x, axis=1)).mean(axis=(0, 2)) in float64."""
    return np.abs(np.fft.rfft(np.asarray(x, dtype=np.float64), axis=1)).mean(axis=(0, 2))


def step_errors(got, ref):
    """max|got - ref| / max|ref| per generated step s = 1..steps (ref float64)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.array([np.abs(got[:, s] - ref[:, s]).max() / np.abs(ref[:, s]).max() for s in range(1, ref.shape[1])])


def row_spread(ref, s):
    """How far apart the rows of step s are, relative to max|ref[:, s]|: 0 when every row has collapsed onto one trajectory."""
    blk = np.asarray(ref, dtype=np.float64)[:, s]
    return np.abs(blk - blk.mean(axis=0, keepdims=True)).max() / np.abs(blk).max()


def random_params(rng, Z, D, d_ff, n_layers, conv=True, pos="learn", eps=1e-5):
    """nn-style initial scales with every tensor random (no zero bias, no unit gain), so that each of them matters.  Iterating
    the map behaves like power iteration: with nn's own scales the rows collapse onto one trajectory within a few steps and a
    comparison would stop seeing them.  The in-projection is therefore 6 x, the decoder 3 x its nn scale and a learnable
    position row 0.3 x a normal one, which keeps the rows apart (asserted by tests/test_rollout_cpu.py) without making the map
    chaotic (also asserted).  pos: None | 'learn' (normal rows) | 'sin' (the sinusoidal table's rows 0 and 1)."""
    u = lambda shape, fan: rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan)
    layers = []
    for _ in range(n_layers):
        layers.append((u((3 * Z, Z), Z) * 1.7, 0.1 * rng.standard_normal(3 * Z), u((Z, Z), Z), 0.1 * rng.standard_normal(Z),
                       u((d_ff, Z), Z), u((d_ff,), Z), u((Z, d_ff), d_ff), u((Z,), d_ff),
                       1.0 + 0.2 * rng.standard_normal(Z), 0.1 * rng.standard_normal(Z),
                       1.0 + 0.2 * rng.standard_normal(Z), 0.1 * rng.standard_normal(Z)))
    p = {"w_in": 6.0 * u((Z, D), D), "b_in": u((Z,), D), "conv": u((Z, Z), Z) if conv else None, "pos0": None, "pos1": None,
         "layers": layers, "eps": eps, "w_out": 3.0 * u((D, Z), Z), "b_out": u((D,), Z)}
    if pos == "learn":
        p["pos0"], p["pos1"] = 0.3 * rng.standard_normal(Z), 0.3 * rng.standard_normal(Z)
    elif pos == "sin":
        div = np.exp(np.arange(0, Z, 2) * (-np.log(10000.0) / Z))
        tab = np.zeros((2, Z))
        tab[:, 0::2] = np.sin(np.arange(2)[:, None] * div)
        tab[:, 1::2] = np.cos(np.arange(2)[:, None] * div)
        p["pos0"], p["pos1"] = tab[0], tab[1]
    return cast(p, np.float32)                              # what a device holds: fp32 values, the same for every evaluation


# name -> (Z, D, d_ff, n_layers, conv, pos, n, steps); one case per edge of tests/test_rollout_gpu.py
CASES = {
    "z10_d5_long": (10, 5, 2048, 5, True, "learn", 33, 49),
    "z10_d7_nopos": (10, 7, 2048, 5, True, None, 17, 49),
    "z10_d1_one_row": (10, 1, 72, 1, False, "sin", 1, 4),
    "z40_d35": (40, 35, 2048, 5, True, "learn", 16, 4),
    "z40_d35_noconv_sin": (40, 35, 72, 1, False, "sin", 15, 4),
    "z40_d371": (40, 371, 72, 5, True, None, 17, 4),
    "z300_d300": (300, 300, 2048, 1, True, "learn", 33, 4),
    "z300_d35_ff72": (300, 35, 72, 5, False, None, 16, 4),
    "z300_d300_long": (300, 300, 72, 1, True, "sin", 15, 49),
    "z40_d35_steps0": (40, 35, 72, 1, True, "learn", 17, 0),
    "z40_d35_steps1": (40, 35, 2048, 1, True, "learn", 33, 1),
    "z10_d5_nolayers": (10, 5, 72, 0, True, "learn", 17, 4),
    "z10_d5_eps": (10, 5, 72, 2, True, "learn", 17, 4),
}
EPS = {"z10_d5_eps": 1e-2}                                   # LayerNorm eps where it is not nn's 1e-5: large enough to matter
DATA_SEEDS = (0, 1, 2, 3)


def make_case(name, data_seed=0):
    Z, D, d_ff, n_layers, conv, pos, n, steps = CASES[name]
    import zlib
    p = random_params(np.random.default_rng(zlib.crc32(name.encode())), Z, D, d_ff, n_layers, conv=conv, pos=pos, eps=EPS.get(name, 1e-5))
    x0 = np.random.default_rng(1000 + data_seed).standard_normal((n, D)).astype(np.float32)
    return p, x0, steps


def measure_fp32(name):
    """(worst fp32 error over steps and data seeds, worst ratio of a seed's worst error to its step-1 error)."""
    worst, growth = 0.0, 0.0
    for seed in DATA_SEEDS:
        p, x0, steps = make_case(name, seed)
        if steps == 0:
            continue
        e = step_errors(rollout(p, x0, steps, np.float32), rollout(p, x0, steps, np.float64))
        worst, growth = max(worst, e.max()), max(growth, e.max() / e[0])
    return worst, growth


def bound_from(err):
    return 2.0 ** int(np.ceil(np.log2(8.0 * err))) if err > 0 else 2.0 ** -20


# bound = 8 x the fp32 numpy evaluation's worst error over DATA_SEEDS, rounded up to a power of two (measure_fp32; kept current by
# tests/test_rollout_cpu.py::test_criterion_table_is_current)
BOUNDS = {"z10_d5_long": 2.0 ** -15, "z10_d7_nopos": 2.0 ** -14, "z10_d1_one_row": 2.0 ** -19, "z40_d35": 2.0 ** -17,
          "z40_d35_noconv_sin": 2.0 ** -18, "z40_d371": 2.0 ** -15, "z300_d300": 2.0 ** -16, "z300_d35_ff72": 2.0 ** -16,
          "z300_d300_long": 2.0 ** -14, "z40_d35_steps0": 2.0 ** -20, "z40_d35_steps1": 2.0 ** -18, "z10_d5_nolayers": 2.0 ** -18,
          "z10_d5_eps": 2.0 ** -16}
LONG_CASE = "z10_d7_nopos"


def params_from_state(sd, x_side, with_pos, n_layers, eps=1e-5):
    """A parameter set from a reference-keyed state dict ({name: array}): modality x (decoders.0) or y (decoders.1)."""
    a = lambda k: np.asarray(sd[k])
    pre = "encoder.transformer.layers.%d."
    names = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
             "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
             "norm2.bias")
    proj, dec = ("xproj_in", "decoders.0") if x_side else ("yproj_in", "decoders.1")
    pos = a("encoder.pos_embedding.weight") if with_pos else None
    return {"w_in": a(proj + ".fc.weight"), "b_in": a(proj + ".fc.bias"), "conv": a("encoder.conv.weight")[:, :, 0],
            "pos0": None if pos is None else pos[0], "pos1": None if pos is None else pos[1],
            "layers": [tuple(a(pre % l + n) for n in names) for l in range(n_layers)], "eps": eps,
            "w_out": a(dec + ".fc.weight"), "b_out": a(dec + ".fc.bias")}
