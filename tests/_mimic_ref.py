"""What the MIMIC loader computes (multibench/mimic.py, include/umlh.h ``umlh_tab_standardize`` / ``umlh_tab_perturb`` /
``umlh_rows_gather``), stated in numpy float64, and the fixture tests/golden/mimic*.npz that holds what the
reference's own loader gave for the same inputs (scripts/make_golden_mimic.py).

  clean, standardize   X[isinf] = 0; X[isnan] = 0, then (X - average) / std with numpy's own reductions over the axes the
                       reference names (population std), on copies
  split                random.Random(10).shuffle(range(n)) -> valid [0 : n//10], test [n//10 : n//5], train [n//5 :]
  labels               y_icd9[:, task], or the six-class rule on adm_labels_all for task < 0, row by row as the reference
  tabular              drop: x[i, j] = 0 where the mask is set; then for j = 1 .. d-1 in order: x[i, j] = x[i, j-1] where the
                       carry mask is set -- the left neighbour AS UPDATED SO FAR (the reference's swap_entry)
  series_noise         x + eps[sample] in float64, elements with the element mask set = 0, samples with keep == 0 = 0
  levels               the eleven test sets from one RandomState: per level n*5 and n*4 uniforms, n normals, n*288 uniforms,
                       n uniforms; p = k / 10

``variant`` names one deliberately wrong reading; tests/test_mimic_cpu.py shows that each differs from the fixture."""
import random

import numpy as np

from conftest import load_golden

CASES = ("n57", "n203", "const31")
RECORDED = (0, 3, 10)
VARIANTS = ("true_swap", "carry_undropped", "carry_before_drop", "sample_std", "stats_before_clean", "noise_per_step",
            "sample_drop_per_step")


def load_fixture():
    return load_golden("mimic")


def config(fx, case):
    n, bs, seed, tseed = (int(v) for v in fx[f"{case}/config"])
    return n, bs, seed, tseed


def datafile(fx, case):
    return {k: fx[f"{case}/in/{k}"].copy() for k in ("adm_features_all", "ep_tdata", "y_icd9", "adm_labels_all")}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_values(a, b):
    """equal element by element with NaN == NaN and +0.0 != -0.0 (NaN payloads are not compared: numpy's arithmetic may change them)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b))))


def clean(a):
    a = np.array(a, copy=True)
    a[np.isinf(a)] = 0
    a[np.isnan(a)] = 0
    return a


def standardize(df, variant=None):
    """(static [N, ds], series [N, T, dt]) float64, get_data.py:35-51"""
    xs, xt = clean(df["adm_features_all"]), clean(df["ep_tdata"])
    ss, st = (np.asarray(df["adm_features_all"]), np.asarray(df["ep_tdata"])) if variant == "stats_before_clean" else (xs, xt)
    ddof = 1 if variant == "sample_std" else 0
    with np.errstate(all="ignore"):
        s_avg, s_std = np.average(ss, axis=0), np.std(ss, axis=0, ddof=ddof)
        t_avg, t_std = np.average(st, axis=(0, 1)), np.std(st, axis=(0, 1), ddof=ddof)
        return (xs - s_avg) / s_std, (xt - t_avg) / t_std


def split(n):
    perm = list(range(n))
    random.Random(10).shuffle(perm)
    return {"valid": perm[:n // 10], "test": perm[n // 10:n // 5], "train": perm[n // 5:]}


def labels(df, task):
    if task >= 0:
        return np.asarray(df["y_icd9"])[:, task].copy()
    adm = np.array(df["adm_labels_all"], copy=True)
    y = adm[:, 1]
    for i in range(len(y)):
        for c in range(1, 6):
            if adm[i][c] > 0:
                y[i] = c
                break
        else:
            y[i] = 0
    return y.copy()


def tabular(x, drop, carry, variant=None):
    """add_tabular_noise on [n, d] with the two masks ([n, d], [n, d-1], nonzero = the reference's uniform was below p; None =
    that step off).  Elements are assigned or copied, never computed on: the bits of every surviving value are the input's."""
    x0 = np.array(x, copy=True)
    x = x0.copy()
    d = x.shape[1]

    def do_drop():
        if drop is not None:
            x[np.asarray(drop, dtype=bool)] = 0

    def do_carry():
        if carry is None:
            return
        c = np.asarray(carry, dtype=bool)
        for j in range(1, d):
            sel = c[:, j - 1]
            if variant == "true_swap":
                tmp = x[sel, j].copy()
                x[sel, j] = x[sel, j - 1]
                x[sel, j - 1] = tmp
            elif variant == "carry_undropped":
                x[sel, j] = x0[sel, j - 1]
            else:
                x[sel, j] = x[sel, j - 1]

    if variant == "carry_before_drop":
        do_carry(), do_drop()
    else:
        do_drop(), do_carry()
    return x


def series_noise(x, eps, elem, keep, out_dtype=None):
    """add_timeseries_noise on the one-element list [x], x = [n, T, dt]: eps [n] or [n, T], elem [n, T * dt] (nonzero = dropped),
    keep [n] or [n, T] (0 = dropped).  The sum is formed in float64; ``out_dtype`` rounds it once (the device tables are fp32)."""
    n, T, dt = x.shape
    with np.errstate(all="ignore"):
        y = x.astype(np.float64) + (eps[:, None, None] if eps.ndim == 1 else eps[:, :, None])
    if out_dtype is not None:
        y = y.astype(out_dtype)
    y[np.asarray(elem, dtype=bool).reshape(n, T, dt)] = 0
    y[(keep == 0) if keep.ndim == 2 else np.broadcast_to((keep == 0)[:, None], (n, T))] = 0
    return y


def draws(n, seed, levels=11, tabular_robust=True, timeseries_robust=True, variant=None, ds=5, T=24, dt=12):
    """Per level the dict of draws in the reference's order from RandomState(seed): 'drop', 'carry' (bool, True = below p), 'eps',
    'elem' (True = dropped), 'keep' (uint8, 0 = dropped); None for a disabled family."""
    rs = np.random.RandomState(seed)
    out = []
    for k in range(levels):
        p = k / 10
        lv = dict.fromkeys(("drop", "carry", "eps", "elem", "keep"))
        if tabular_robust:
            lv["drop"] = rs.random_sample(n * ds).reshape(n, ds) < p
            lv["carry"] = rs.random_sample(n * (ds - 1)).reshape(n, ds - 1) < p
        if timeseries_robust:
            lv["eps"] = rs.normal(0, p, size=(n, T) if variant == "noise_per_step" else n)
            lv["elem"] = rs.random_sample(n * T * dt).reshape(n, T * dt) < p
            lv["keep"] = (~(rs.random_sample((n, T) if variant == "sample_drop_per_step" else n) < p)).astype(np.uint8)
        out.append(lv)
    return out


def levels(static, series, seed, variant=None, tabular_robust=True, timeseries_robust=True):
    """[(static, series)] of the eleven levels from the standardised test rows (float64)"""
    out = []
    for lv in draws(static.shape[0], seed, 11, tabular_robust, timeseries_robust, variant):
        st = tabular(static, lv["drop"], lv["carry"], variant) if tabular_robust else static.copy()
        se = series_noise(series, lv["eps"], lv["elem"], lv["keep"]) if timeseries_robust else series.copy()
        out.append((st, se))
    return out


def ulp_distance(a32, b32):
    """elementwise distance in units of fp32 representable values between two float32 arrays (NaN: 0 when both are, else huge)"""
    a, b = np.ascontiguousarray(a32, dtype=np.float32), np.ascontiguousarray(b32, dtype=np.float32)

    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    both = np.isnan(a) & np.isnan(b)
    either = np.isnan(a) ^ np.isnan(b)
    return np.where(both, 0, np.where(either, 1 << 40, d))
