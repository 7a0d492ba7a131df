"""The contract of the standalone optimizer entry points of include/umlh.h (umlh_optimizer_step, umlh_optimizer_step_multi) and of
umlh_to_bf16 restated in numpy, the accuracy criterion the HIP kernels must meet against the float64 evaluation, the case tables of
tests/test_optstep_gpu.py and a set of deliberately wrong variants that the criterion must reject.  No GPU, no `umlh` import.

opt_ref is the torch.optim single-tensor recurrence in float64 (SGD with momentum and L2 decay, Adam with L2 decay, AdamW with
decoupled decay; oracle/uml_oracle.py: optimizer_step cites the sources).  kernel_form restates csrc/umlh_common.h: opt_update
with the constants csrc/umlh_api.cpp: make_opt hands it: computed in double and rounded to fp32 once (lr, decay = 1 - lr wd,
-(lr / bc1), sqrt(bc2), beta1, 1 - beta1, beta2, 1 - beta2, eps, momentum, wd), step < 1 counted as step 1.  In float64 it is the
same recurrence up to those roundings; in float32 it is "an honest fp32 implementation", evaluated once with every multiply and
add rounded separately and once with each a * b + c fused (the compiler may contract), and is what the bound is calibrated on.

Criterion.  The error of p, m and v is |got - ref64| per element in fp32 ulps of the larger of the element's magnitude before and
after the step (a cancelling update cannot be resolved below the ulp of its operands).  The bound is 8 x the largest error of
the fp32 evaluation (the larger of the separate and the fused form) over wd in {0.1, 0}, step in {0, 1, 2, 1000, 10^6}, lr = 1e-2
and four data seeds of 4096 elements, rounded up to a power of two.  Data: p and g over six decades with independent signs, every
seventh g near 1e-8 (with v near 1e-16: eps decides the step there), m and v non-zero.  Measured on the CPU in ulps (level ->
bound; tests/test_optstep_cpu.py re-measures them):

        kind   output  level  bound   |  kind   output  level  bound   |  kind   output  level  bound
        sgd    p       18.82    256   |  adam   p        7.55     64   |  adamw  p        7.55     64
        sgd    m        3.20     32   |  adam   m        4.25     64   |  adamw  m        1.21     16
                                      |  adam   v        4.46     64   |  adamw  v        1.20     16

    The levels above 2 ulps are carried in, not made by the last operation: g + wd p and momentum m + g cancel, and p - lr m then
    sees m's rounding (ulps of a large |m| before the step) on the scale of a small p.

SGD leaves v alone (it may be NULL).  umlh_to_bf16 is round-to-nearest-even and must be bit-equal to torch's conversion on the CPU;
a NaN stays a NaN (any payload).
"""
import numpy as np

F32, F64 = np.float32, np.float64
KINDS = ("sgd", "adam", "adamw")
OPT_ID = {"sgd": 0, "adam": 1, "adamw": 2}
LR = 1e-2
WDS = (0.1, 0.0)
STEPS = (0, 1, 2, 1000, 10 ** 6)
BETAS, EPS, MOMENTUM = (0.9, 0.999), 1e-8, 0.9
DATA_SEEDS = (0, 1, 2, 3)
N_LEVEL = 4096

WRONG_VARIANTS = ("adamw_l2", "decay_after_update", "eps_inside_sqrt", "no_bc2", "no_bc1", "step_off_by_one", "dampened_momentum",
                  "sgd_no_wd")
VARIANT_KINDS = {"adamw_l2": ("adamw",), "decay_after_update": ("adamw",), "eps_inside_sqrt": ("adam", "adamw"),
                 "no_bc2": ("adam", "adamw"), "no_bc1": ("adam", "adamw"), "step_off_by_one": ("adam", "adamw"),
                 "dampened_momentum": ("sgd",), "sgd_no_wd": ("sgd",)}


def opt_ref(kind, p, g, m, v, lr, step, betas=BETAS, eps=EPS, momentum=MOMENTUM, wd=0.0, wrong=()):
    """(p, m, v) after one step, float64.  step < 1 counts as step 1 (the entry points' rule); SGD returns v unchanged."""
    p, g, m = (np.asarray(a, F64).copy() for a in (p, g, m))
    v = None if v is None else np.asarray(v, F64).copy()
    t = max(int(step), 1) + (1 if "step_off_by_one" in wrong else 0)
    b1, b2 = betas
    if kind == "sgd":
        if wd != 0 and "sgd_no_wd" not in wrong:
            g = g + wd * p
        m = momentum * m + ((1 - momentum) * g if "dampened_momentum" in wrong else g)
        return p - lr * m, m, v
    decoupled = kind == "adamw" and "adamw_l2" not in wrong
    after = "decay_after_update" in wrong
    if decoupled and not after:
        p = p * (1 - lr * wd)
    if not decoupled and wd != 0:
        g = g + wd * p
    m = m + (g - m) * (1 - b1)
    v = b2 * v + (1 - b2) * g * g
    bc1 = 1.0 if "no_bc1" in wrong else 1 - b1 ** t
    bc2 = 1.0 if "no_bc2" in wrong else 1 - b2 ** t
    denom = np.sqrt(v / bc2 + eps) if "eps_inside_sqrt" in wrong else np.sqrt(v) / np.sqrt(bc2) + eps
    p = p - (lr / bc1) * m / denom
    if decoupled and after:
        p = p * (1 - lr * wd)
    return p, m, v


def make_opt(lr, step, betas=BETAS, eps=EPS, momentum=MOMENTUM, wd=0.0):
    """The fp32 constants of one step (csrc/umlh_api.cpp: make_opt)."""
    t = float(max(int(step), 1))
    b1, b2 = betas
    return dict(lr=F32(lr), decay=F32(1.0 - lr * wd), neg_step_size=F32(-(lr / (1.0 - b1 ** t))), bc2_sqrt=F32(np.sqrt(1.0 - b2 ** t)),
                beta1=F32(b1), one_m_beta1=F32(1.0 - b1), beta2=F32(b2), one_m_beta2=F32(1.0 - b2), eps=F32(eps), momentum=F32(momentum),
                wd=F32(wd))


def kernel_form(kind, p, g, m, v, lr, step, betas=BETAS, eps=EPS, momentum=MOMENTUM, wd=0.0, dtype=F64, fused=False):
    """opt_update's statement order on make_opt's constants, in `dtype`; fused: every a * b + c with one rounding."""
    dt = dtype
    o = {k: dt(x) for k, x in make_opt(lr, step, betas, eps, momentum, wd).items()}
    p, g, m = (np.asarray(a).astype(dt) for a in (p, g, m))
    v = None if v is None else np.asarray(v).astype(dt)

    def fma(a, b, c):
        if fused and dt == F32:
            return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)
        return (a * b + c).astype(dt)
    if kind == "sgd":
        if o["wd"] != 0:
            g = fma(o["wd"], p, g)
        m = fma(o["momentum"], m, g)
        return fma(-o["lr"], m, p), m, v
    if kind == "adamw":
        p = (p * o["decay"]).astype(dt)
    elif o["wd"] != 0:
        g = fma(o["wd"], p, g)
    m = fma((g - m).astype(dt), o["one_m_beta1"], m)
    v = fma((o["one_m_beta2"] * g).astype(dt), g, (v * o["beta2"]).astype(dt))
    denom = (np.sqrt(v).astype(dt) / o["bc2_sqrt"]).astype(dt) + o["eps"]
    p = (p + ((o["neg_step_size"] * m).astype(dt) / denom.astype(dt)).astype(dt)).astype(dt)
    return p, m, v


def ulp_err(got, ref, before):
    """The largest |got - ref| in fp32 ulps of max(|before|, |ref|), element by element; a non-finite got is an infinite error."""
    got, ref, before = (np.asarray(a, F64).ravel() for a in (got, ref, before))
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return np.inf
    scale = np.maximum(np.abs(before), np.abs(ref)).astype(F32)
    return float((np.abs(got - ref) / np.spacing(scale).astype(F64)).max())


def build_data(n, seed, tag="opt"):
    """p, g, m, v [n] fp32: |p|, |g| log-uniform over 10^-3 .. 10^3 with independent signs, every seventh g near 1e-8, m of g's
    magnitude (0.2 .. 1 of it, either sign), v of g^2's (0.5 .. 2 of it)."""
    rng = np.random.default_rng([sum(ord(ch) for ch in tag), int(seed), int(n)])
    sign = lambda: rng.choice([-1.0, 1.0], n)
    p = sign() * 10.0 ** rng.uniform(-3, 3, n)
    g = sign() * 10.0 ** rng.uniform(-3, 3, n)
    g[::7] = np.sign(g[::7]) * 1e-8 * rng.uniform(0.5, 2.0, g[::7].size)
    m = sign() * np.abs(g) * rng.uniform(0.2, 1.0, n)
    v = g * g * rng.uniform(0.5, 2.0, n)
    return tuple(a.astype(F32) for a in (p, g, m, v))


def outputs_of(kind):
    return ("p", "m") if kind == "sgd" else ("p", "m", "v")


def settings():
    return [(wd, step) for wd in WDS for step in STEPS]


def errors_against_ref(kind, got, data, wd, step):
    """output -> ulp error of got = (p, m, v) against opt_ref on data = (p, g, m, v)."""
    ref = opt_ref(kind, *data, LR, step, wd=wd)
    before = dict(p=data[0], m=data[2], v=data[3])
    return {k: ulp_err(got["pmv".index(k)], ref["pmv".index(k)], before[k]) for k in outputs_of(kind)}


# measured levels in ulps (rounded up to 0.01), the table of the module docstring
LEVELS_ULP = {
    "sgd": {"p": 18.82, "m": 3.20},
    "adam": {"p": 7.55, "m": 4.25, "v": 4.46},
    "adamw": {"p": 7.55, "m": 1.21, "v": 1.20},
}


def measure_levels():
    lv = {k: {o: 0.0 for o in outputs_of(k)} for k in KINDS}
    for kind in KINDS:
        for seed in DATA_SEEDS:
            data = build_data(N_LEVEL, seed)
            for wd, step in settings():
                for fused in (False, True):
                    got = kernel_form(kind, *data, LR, step, wd=wd, dtype=F32, fused=fused)
                    for o, e in errors_against_ref(kind, got, data, wd, step).items():
                        lv[kind][o] = max(lv[kind][o], e)
    return lv


def bound_of(level_ulp):
    """8 x the level, rounded up to a power of two."""
    return 2.0 ** int(np.ceil(np.log2(8.0 * level_ulp) - 1e-9))


BOUNDS = {k: {o: bound_of(v) for o, v in d.items()} for k, d in LEVELS_ULP.items()}


def variant_excess(name):
    """The largest error / bound of the float64 wrong variant against opt_ref over its kinds and the settings (must be >= 8)."""
    worst = 0.0
    for kind in VARIANT_KINDS[name]:
        data = build_data(N_LEVEL, 0)
        for wd, step in settings():
            got = opt_ref(kind, *data, LR, step, wd=wd, wrong=(name,))
            for o, e in errors_against_ref(kind, got, data, wd, step).items():
                worst = max(worst, e / BOUNDS[kind][o])
    return worst


# ---------------------------------------------------------------------------------------------------------------------------- #
# case tables (tests/test_optstep_gpu.py runs exactly these)
# ---------------------------------------------------------------------------------------------------------------------------- #
SINGLE_N = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4099)        # the float4 / scalar split of reduce_update: n % 4, one block +- 1
MULTI_MAX = 48                                            # csrc/umlh_common.h: UMLH_MULTI_OPT_MAX, tensors per launch


def multi_lists():
    """id -> element counts of one umlh_optimizer_step_multi call: zero-length tensors at either end, the 48-tensor launch seam."""
    out = {"one_empty": [0], "one": [1], "empty_between": [1024, 0, 5], "empty_first": [0, 5], "empty_last": [5, 0],
           "block_edges": [1025, 1023, 1]}
    for k in (48, 49, 70, 97):
        rng = np.random.default_rng(k)
        n = rng.integers(0, 3001, k)
        n[rng.choice(k, 5, replace=False)] = 0
        n[0], n[k - 1] = 0, 0
        if k > MULTI_MAX:
            n[MULTI_MAX - 1], n[MULTI_MAX] = 0, 3000          # the last tensor of launch 0 is empty, the first of launch 1 is not
        out[f"tensors_{k}"] = [int(x) for x in n]
    return out


def encode_p(t, n):
    """p of tensor t: (1 + t) + e / 4096, exact in fp32 and distinct for every (t, e) of the tables."""
    return (F32(1 + t) + np.arange(n, dtype=F32) / F32(4096)).astype(F32)


BF16_N = (0, 1, 7, 8, 9, 2047, 2048, 2049)


def bf16_specials():
    """uint32 bit patterns: every tie with an even and an odd kept bit and its two neighbours, both signs; +-0; fp32 denormals;
    +-inf; NaNs of several payloads; the largest float (rounds to inf)."""
    bits = []
    for sign in (0, 0x80000000):
        for hi in (0x3F80, 0x3F81, 0x0001, 0x0000, 0x7F7E, 0x7F7F, 0x4049):
            for lo in (0x7FFF, 0x8000, 0x8001, 0x0000, 0xFFFF):
                bits.append(sign | (hi << 16) | lo)
        bits += [sign, sign | 0x00000001, sign | 0x007FFFFF, sign | 0x00008000, sign | 0x00018000, sign | 0x7F800000,
                 sign | 0x7FC00000, sign | 0x7F800001, sign | 0x7FFFFFFF, sign | 0x7FBADBAD, sign | 0x7F80FFFF, sign | 0x7F7FFFFF]
    return np.array(bits, np.uint32)


def build_bf16_input(n):
    """float32[n]: random bit patterns with the specials at the front (the 8-wide path) and, reversed, at the back (the tail)."""
    rng = np.random.default_rng(n)
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    sp = bf16_specials()
    k = min(n, sp.size)
    bits[:k] = sp[:k]
    if n:
        bits[n - k:] = sp[:k][::-1]
    return bits.view(F32)
