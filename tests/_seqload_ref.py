"""What the affect datasets' device loader computes (multibench/data.py, include/umlh.h `umlh_seq_*`), stated
in numpy float64, and the fixture tests/golden/seq_loader*.npz that holds what the reference's own loader
(MultiBench/datasets/affect/get_data.py, CPU, num_workers=0) gave for the same inputs (scripts/make_golden_seq_loader.py).

The statement follows the issue's table step by step: fp32 rounding at upload, drop of samples whose text has no nonzero
element, audio -inf -> 0, vision_norm (population std over all kept N*T rows), front trim at the first nonzero text row, z_norm
(unbiased std over the trimmed rows, nan_to_num), labels, and the _process_1 batch with Lmax of the batch.  ``variant`` names one
deliberately wrong reading; the CPU tests show that each breaks a check against the fixture."""
import numpy as np

from conftest import load_golden

MODALITIES = ("vision", "audio", "text")
VARIANTS = ("biased_z", "unbiased_vision", "untrimmed_stats", "vision_with_dropped", "own_first_row", "lmax_T")
FLT_MAX = float(np.finfo(np.float32).max)
# log2 of the bound on max |got - ref64| / max |ref64| per block and per case of the fixture, in the fixture's order: 8 times the
# reference's own fp32 error against the statement, rounded up to a power of two (tests/test_seqload_cpu.py measures it and holds
# this table to it); None: no normalisation, compared bit for bit.
BOUND_LOG2 = {"toy_mosi": None, "toy_sarcasm_vnorm": -18, "toy_mosei_znorm": -18, "toy_mosi_bs11": None, "wide_mosi": None,
              "wide_sarcasm_vnorm": -15, "wide_mosei_znorm": -19}


def bound(case):
    return 0.0 if BOUND_LOG2[case] is None else 2.0 ** BOUND_LOG2[case]


def load_fixture():
    """Every array of tests/golden/seq_loader.npz and its parts in one dict."""
    return load_golden("seq_loader")


def fixture_split(fx, dataset, split):
    """The split dict ('vision', 'audio', 'text', 'labels', 'id') the reference's loader was given."""
    return {k: fx[f"data/{dataset}/{split}/{k}"] for k in MODALITIES + ("labels", "id")}


def fixture_batches(fx, case, loader):
    """The reference's batches of one recorded pass ('train0', 'train1', 'valid'): a list of
    ([v, a, t], [lv, la, lt], inds, labels) numpy tuples."""
    n = int(fx[f"case/{case}/{loader}/batches"])
    key = lambda i, what: fx[f"case/{case}/{loader}/{i}/{what}"]
    return [([key(i, f"x{m}") for m in range(3)], [key(i, f"l{m}") for m in range(3)], key(i, "inds"), key(i, "labels"))
            for i in range(n)]


def first_rows(x):
    """Row of the first element != 0 per sample of [N, T, D] (NaN counts, -0.0 does not), T when there is none."""
    rows = (np.asarray(x) != 0).any(axis=2)
    return np.where(rows.any(axis=1), rows.argmax(axis=1), x.shape[1]).astype(np.int64)


def nan_to_num(v):
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(v, -FLT_MAX, FLT_MAX)


def build_table(split, data_type="mosi", z_norm=False, vision_norm=False, variant=None):
    """The table of one split: {'tables': three float64 [n, T, D_m] arrays (rows before ``start`` are whatever the passes left
    there; no batch reads them), 'start': int64 [n] per modality list (the same array three times except in the
    'own_first_row' variant), 'lengths', 'labels': float32 [n, 1], 'kept': positions in the split}."""
    with np.errstate(all="ignore"):
        x = [np.asarray(split[m]).astype(np.float32).astype(np.float64) for m in MODALITIES]      # fp32 at upload
        n_all, T = x[0].shape[:2]
        start_all = first_rows(x[2])
        keep = np.flatnonzero(start_all < T)
        x[1] = np.where(x[1] == -np.inf, 0.0, x[1])
        if vision_norm and variant == "vision_with_dropped":
            rows = x[0].reshape(-1, x[0].shape[2])
            x[0] = (x[0] - rows.mean(0)) / rows.std(0)
        x = [a[keep] for a in x]
        start = start_all[keep]
        if vision_norm and variant != "vision_with_dropped":
            rows = x[0].reshape(-1, x[0].shape[2])
            x[0] = (x[0] - rows.mean(0)) / rows.std(0, ddof=1 if variant == "unbiased_vision" else 0)
        starts = [start, start, start]
        if variant == "own_first_row":
            starts = [np.minimum(first_rows(a), T - 1) for a in x[:2]] + [start]
        if z_norm:
            for a, st in zip(x, starts):
                for i in range(a.shape[0]):
                    s = 0 if variant == "untrimmed_stats" else st[i]
                    seq = a[i, s:]
                    sd = seq.std(0, ddof=0 if variant == "biased_z" else 1) if seq.shape[0] > 1 or variant == "biased_z" \
                        else np.full(seq.shape[1], np.nan)
                    a[i, s:] = nan_to_num((seq - seq.mean(0)) / sd)
        lab = np.asarray(split["labels"]).reshape(n_all)[keep].astype(np.float64)
        if data_type in ("humor", "sarcasm"):
            lab = np.where(lab < 1, -1.0, 1.0)
    return {"tables": x, "start": starts, "lengths": [T - s for s in starts], "labels": lab.astype(np.float32).reshape(-1, 1),
            "kept": keep, "T": T}


def batch(table, ids, variant=None, t_out=None):
    """The _process_1 batch of the kept samples ``ids``: ([v, a, t] float64 [b, Lmax, D_m], [lv, la, lt] int64 [b], inds int64
    [b, 1], labels float32 [b, 1]).  Lmax is the longest trimmed sequence of the batch (per modality; they agree except in the
    'own_first_row' variant), or ``t_out`` when given (rows and lengths clipped to it).  An id outside the table gives a zero
    block and length 0 (no label: its row of ``labels`` is NaN)."""
    ids = np.asarray(ids, dtype=np.int64)
    inside = (ids >= 0) & (ids < table["tables"][0].shape[0])
    blocks, lens = [], []
    for a, st, ln in zip(table["tables"], table["start"], table["lengths"]):
        l_b = np.where(inside, ln[np.where(inside, ids, 0)], 0)
        lmax = table["T"] if variant == "lmax_T" else int(l_b.max())
        if t_out is not None:
            lmax, l_b = t_out, np.minimum(l_b, t_out)
        out = np.zeros((len(ids), lmax, a.shape[2]))
        for j, i in enumerate(ids):
            if inside[j]:
                out[j, :l_b[j]] = a[i, st[i]:st[i] + l_b[j]]
        blocks.append(out)
        lens.append(l_b.astype(np.int64))
    labels = np.where(inside[:, None], table["labels"][np.where(inside, ids, 0)], np.float32(np.nan))
    return blocks, lens, ids.reshape(-1, 1), labels


def same_bits(a, b):
    """fp32 arrays equal bit for bit (any NaN equals any NaN; +0.0 and -0.0 differ)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | both_nan).all())


def rel_err(got, want):
    """max |got - want| / max |want| over finite entries of ``want`` (float64); inf when the NaN patterns differ."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or (np.isnan(got) != np.isnan(want)).any():
        return float("inf")
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    scale = np.abs(want[ok]).max()
    return float(np.abs(got[ok] - want[ok]).max() / (scale if scale > 0 else 1.0))
