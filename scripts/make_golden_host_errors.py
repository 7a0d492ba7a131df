"""Records what the stateless entry points of include/umlh.h answer to bad arguments: tests/golden/host_errors.json, replayed by
tests/test_host_errors_cpu.py.  The file pins the full message and, through the two-fault rows, the order of the checks.

    python scripts/make_golden_host_errors.py [--lib path/to/libumlh.so]

Run it against a library built from the commit whose behaviour is to be kept, on a machine WITHOUT a GPU: every pointer below
is a fake address, a call that passes its checks there returns a HIP error, and on a machine with a GPU it would launch on the
fake address.  Only rows answered with UMLH_E_INVALID are written; every other row is listed on stdout and dropped.

One legal base call per entry point; rows change one argument at a time (a required pointer to NULL, a count to 0, -1 and one
past its limit, a stride to d - 1, a floating-point argument to NaN and -1, scratch_bytes to 0 and need - 1, scratch to an address
that is 2 mod 8), then two at a time (neighbouring arguments, and the first with the last).  The entry points of
umlh_encoder.cpp are not covered: they refuse without a message."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import _host_errors as H  # noqa: E402

FAKE = 256
ROWS = (1 << 31) - 1          # "n < 2^31"
ALIGN_ROWS = 1 << 30          # "n <= 2^30"
FEATS, MEANS = 1 << 20, 1 << 24      # two fake buffers far enough apart for the overlap checks


# ---- argument descriptions: (base value, [alternatives]) ----
def P(addr=FAKE):                      # required pointer
    return addr, [None]


def O(addr=None):                      # optional pointer (NULL is legal: nothing to change)
    return addr, []


def n(v, limit=None):                  # count
    return v, [0, -1] + ([limit + 1] if limit is not None else [])


def s(v, d):                           # stride of rows of d elements
    return v, [d - 1]


def f(v):                              # floating-point argument
    return v, ["nan", -1.0]


def v(x, *alts):                       # anything else, with explicit alternatives
    return x, list(alts)


def ptrs(k):                           # host array of k pointers
    return {"ptrs": [FAKE] * k}, [None, {"ptrs": [FAKE] * (k // 2) + [0] + [FAKE] * (k - k // 2 - 1)}]


SCRATCH = (FAKE, [None, FAKE + 2])
STREAM = (None, [])


def nbytes(query, *args):              # scratch_bytes: the library's own query; need - 1 is added once the need is known
    return ("query", query, args), [0]


def rollout_cfg():
    base = [8, 16, 5, 1, 3, 1e-5]      # Z, d_ff, D, n_layers, steps, eps
    alts = [None]
    for i, vals in enumerate(([0, -1, 513], [0, -1, 2049], [0, -1, 1025], [-1, 17], [-1, 4097], ["nan", -1.0])):
        alts += [{"cfg": base[:i] + [x] + base[i + 1:]} for x in vals]
    return {"cfg": base}, alts


def calls():
    """entry -> list of argument descriptions, in the order of include/umlh.h."""
    c = {}
    c["umlh_to_bf16"] = [P(), P(), n(8), STREAM]
    c["umlh_seq_mse_forward"] = [P(), P(), P(), P(), O(), n(2), n(3), n(4, 8192), n(5), O(), P(), P(), P(), STREAM]
    c["umlh_seq_mse_backward"] = [P(), P(), P(), P(), P(), n(2), n(3), n(4), n(5, 8192), P(), P(), P(), O(), STREAM]
    c["umlh_infonce_forward"] = [P(), P(), n(4), n(8), f(0.1), P(), P(), P(), P(), P(), P(), STREAM]
    c["umlh_infonce_backward"] = [P(), P(), P(), P(), P(), n(4), n(8), f(0.1), P(), P(), STREAM]
    c["umlh_gemm_f32"] = [P(), P(), P(), n(4), n(5), n(6), s(6, 6), s(6, 6), s(5, 5), n(0, 1), n(0, 1), O(), O(), f(1.0), n(1), O(), STREAM]
    c["umlh_bias_act"] = [P(), O(), n(4), n(5), v(1), STREAM]
    c["umlh_relu_backward"] = [P(), P(), n(8), STREAM]
    c["umlh_dropout"] = [P(), n(8), f(0.1), v(1), STREAM]
    c["umlh_add_inplace"] = [P(), P(), n(8), STREAM]
    c["umlh_colsum"] = [P(), n(4), n(5), P(), STREAM]
    c["umlh_add_layernorm_forward"] = [P(), O(), P(), P(), n(4), n(5), f(1e-5), P(), P(), P(), P(), STREAM]
    c["umlh_layernorm_backward"] = [P(), P(), P(), P(), P(), n(4), n(5), P(), P(), P(), STREAM]
    c["umlh_add_positions"] = [P(), P(), n(3), n(2), n(4), STREAM]
    c["umlh_positions_backward"] = [P(), n(3), n(2), n(4), P(), STREAM]
    c["umlh_gather_rows"] = [P(), P(), n(3), n(4), P(), v(0), STREAM]
    c["umlh_attention_forward"] = [P(), O(), n(3, 128), n(2), n(8), n(2), f(0.1), v(1), P(), P(), STREAM]
    c["umlh_attention_backward"] = [P(), O(), P(), P(), n(3, 128), n(2), n(8), n(2), f(0.1), v(1), P(), STREAM]
    c["umlh_random_permutation"] = [n(8), v(1), P(), STREAM]
    hyper = [f(1e-3), v(1), f(0.9), f(0.999), f(1e-8), f(0.9), f(0.01)]
    c["umlh_optimizer_step"] = [n(2, 2), P(), P(), P(), P(), n(8)] + hyper + [STREAM]
    c["umlh_optimizer_step_multi"] = [n(2, 2), v(2, -1), ptrs(2), ptrs(2), ptrs(2), ptrs(2), ({"i64s": [8, 8]}, [None, {"i64s": [8, -1]}])] + hyper + [STREAM]
    # alignment metrics
    c["umlh_align_knn"] = [P(), n(16, ALIGN_ROWS), n(8), s(8, 8), n(4, 32), v(0, -1), P(), O(), SCRATCH,
                           nbytes("umlh_align_scratch_bytes", 16, 8, 8, 4, 0), STREAM]
    c["umlh_align_mutual_knn"] = [P(), P(), n(16, ALIGN_ROWS), n(4, 32), P(), SCRATCH, nbytes("umlh_align_scratch_bytes", 16, 8, 8, 4, 0), STREAM]
    cka = [P(), s(8, 8), n(8), P(), s(6, 6), n(6), n(16, ALIGN_ROWS)]
    c["umlh_align_cka"] = cka + [v(0, -1), P(), SCRATCH, nbytes("umlh_align_scratch_bytes", 16, 8, 6, 0, 0), STREAM]
    c["umlh_align_cka_unbiased"] = cka + [v(0, -1), P(), SCRATCH, nbytes("umlh_align_ext_scratch_bytes", 0, 16, 8, 6, 0, 0), STREAM]
    c["umlh_align_cka_rbf"] = cka + [f(1.0), v(1, 0), v(0, -1), P(), SCRATCH, nbytes("umlh_align_ext_scratch_bytes", 1, 16, 8, 6, 0, 0), STREAM]
    c["umlh_align_cknna"] = [P(), P(), P(), P(), n(16, ALIGN_ROWS), n(4, 32), P(), SCRATCH,
                             nbytes("umlh_align_ext_scratch_bytes", 2, 16, 8, 8, 4, 0), STREAM]
    c["umlh_align_list_stats"] = [P(), P(), n(16, ALIGN_ROWS), n(4, 32), O(), P(), SCRATCH,
                                  nbytes("umlh_align_ext_scratch_bytes", 3, 16, 8, 8, 4, 0), STREAM]
    # linear probes
    c["umlh_masked_mean"] = [P(), n(2), n(3), n(4), s(12, 4), s(4, 4), O(), P(), s(4, 4), STREAM]
    c["umlh_probe_column_stats"] = [P(), n(16, ROWS), n(8, 1024), s(8, 8), P(), SCRATCH, nbytes("umlh_probe_scratch_bytes", 16, 8, 0), STREAM]
    c["umlh_probe_fit"] = [P(), n(16, ROWS), n(8, 1024), s(8, 8), P(), O(), n(0, 1), f(1.0), n(10, 1000), f(1e-4), P(), P(), O(), SCRATCH,
                           nbytes("umlh_probe_scratch_bytes", 16, 8, 10), STREAM]
    c["umlh_probe_score"] = [P(), n(16, ROWS), n(8, 1024), s(8, 8), O(), P(), P(), P(), P(), STREAM]
    # k-NN probe
    c["umlh_knn_search"] = [P(), n(16, ROWS), s(8, 8), P(), n(4, ROWS), s(8, 8), n(8), n(3, 24), v(0, -1), P(), O(), SCRATCH,
                            nbytes("umlh_knn_scratch_bytes", 16, 4, 8, 3, 0), STREAM]
    c["umlh_knn_vote"] = [P(), n(4, ROWS), n(3, 24), P(), n(16, ROWS), P(), P(), P(), P(), STREAM]
    # singular values, effective rank, subspaces, SVCCA
    spectral = [P(), n(2, 65535), n(5, ROWS), n(4, 512), s(20, 4), s(4, 4)]
    c["umlh_svdvals"] = spectral + [P(), SCRATCH, nbytes("umlh_spectral_scratch_bytes", 2, 5, 4), STREAM]
    c["umlh_effective_rank"] = spectral + [f(1e-12), P(), O(), SCRATCH, nbytes("umlh_spectral_scratch_bytes", 2, 5, 4), STREAM]
    c["umlh_effective_rank_seq"] = [P(), n(2), n(3), n(4, 512), s(12, 4), s(4, 4), O(), v(1, -1), f(1e-12), P(), O(), SCRATCH,
                                    nbytes("umlh_spectral_scratch_bytes", 1, 6, 4), STREAM]
    c["umlh_principal_subspace"] = [P(), n(16, ROWS), n(8, 512), s(8, 8), n(2, 64), n(1, 1), P(), P(), SCRATCH,
                                    nbytes("umlh_subspace_scratch_bytes", 16, 8, 0, 2), STREAM]
    c["umlh_svcca"] = [P(), P(), n(16, ROWS), n(8, 512), n(6, 512), s(8, 8), s(6, 6), n(2, 64), P(), O(), O(), SCRATCH,
                       nbytes("umlh_subspace_scratch_bytes", 16, 8, 6, 2), STREAM]
    # embedding capture, step statistics
    c["umlh_seq_compact"] = [P(), n(2, 65535), n(3), n(4), s(12, 4), s(4, 4), O(), v(0, -1), P(), s(4, 4), v(6, -1), P(), STREAM]
    c["umlh_paired_cosine"] = [P(), s(8, 8), P(), s(8, 8), n(16), n(8), f(1e-8), P(), O(), SCRATCH,
                               nbytes("umlh_paired_cosine_scratch_bytes", 16, 8), STREAM]
    c["umlh_seq_step_stats"] = [P(), s(12, 4), s(4, 4), O(FAKE), s(12, 4), s(4, 4), n(2, 65535), n(3), n(4), O(), P(), SCRATCH,
                                nbytes("umlh_seq_step_stats_scratch_bytes", 2, 3, 4), STREAM]
    # rollout and spectra
    c["umlh_rollout"] = [rollout_cfg(), ptrs(12), O(), O(), P(), P(), P(), P(), P(), s(5, 5), n(4, 1 << 20), P(), s(20, 20), s(5, 5), STREAM]
    c["umlh_seq_spectrum"] = [P(), s(12, 4), s(4, 4), n(2, 1 << 20), n(3, 1024), n(4), P(), SCRATCH,
                              nbytes("umlh_seq_spectrum_scratch_bytes", 2, 3, 4), STREAM]
    # class index and class statistics
    c["umlh_class_index"] = [P(), n(16, ROWS), n(4), P(), P(), SCRATCH, nbytes("umlh_class_index_scratch_bytes", 16, 4), STREAM]
    c["umlh_class_stats"] = [P(FEATS), s(8, 8), n(16, ROWS), n(8), P(), P(), n(4), (MEANS, [None, FEATS + 64]), s(8, 8), P(), P(), SCRATCH,
                             nbytes("umlh_class_stats_scratch_bytes", 16, 8, 4), STREAM]
    # class-wise report
    c["umlh_eval_topk"] = [P(), n(10, ROWS), s(8, 8), P(), n(100, ROWS), s(8, 8), n(8), O(), O(), n(5, 24), v(0, -1), P(), O(), SCRATCH,
                           nbytes("umlh_eval_topk_scratch_bytes", 10, 100, 8, 5, 0), STREAM]
    c["umlh_eval_classwise"] = [P(), n(10, ROWS), n(5, 24), P(), n(100, ROWS), P(), P(), P(), O(), P(), STREAM]
    # outlier clamp
    c["umlh_row_abs_quantile"] = [P(), n(4), n(8, ROWS), s(8, 8), (0.95, ["nan", -1.0, 1.0]), O(), O(), P(), O(), P(), SCRATCH,
                                  nbytes("umlh_outlier_scratch_bytes", 0, 4, 8), STREAM]
    c["umlh_abs_kth"] = [P(), n(4), n(8, ROWS), s(8, 8), v(5, -1, 32), P(), SCRATCH, nbytes("umlh_outlier_scratch_bytes", 1, 4, 8), STREAM]
    c["umlh_clamp_rows"] = [P(FEATS), n(4), n(8, ROWS), s(8, 8), P(), v(1), (MEANS, [None]), s(8, 8), STREAM]
    c["umlh_knn_accuracy"] = [P(), n(4, ROWS), n(3, ROWS), s(3, 3), P(), SCRATCH, nbytes("umlh_outlier_scratch_bytes", 2, 4, 3), STREAM]
    return c


# two-fault rows that neighbouring arguments do not give
EXTRA = {
    "umlh_clamp_rows": [[(6, FEATS), (7, 9)]],                      # in place with another row stride
    "umlh_probe_score": [[(7, None), (8, None)]],                   # nothing to compute
    "umlh_knn_vote": [[(6, None), (7, None), (8, None)]],
    "umlh_random_permutation": [[(0, -1), (2, None)]],              # (n = 0 takes no output: the neighbours' row is legal)
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="libumlh.so to record (default: the in-tree build)")
    ap.add_argument("--out", default=H.GOLDEN)
    a = ap.parse_args()
    import torch
    assert not torch.cuda.is_available(), "a GPU is visible: a call that passes its checks would launch on a fake address"
    lib = H.load(a.lib)
    entries, dropped, kept = [], [], 0
    for entry, desc in calls().items():
        base, alts = [], []
        for val, alt in desc:
            if isinstance(val, tuple) and val[0] == "query":
                val = int(getattr(lib, val[1])(*val[2]))
                assert val > 0, (entry, "the scratch query refuses the base shape")
            base.append(val)
            alts.append(list(alt))
        rc, msg = H.call(lib, entry, base)
        assert rc != H.E_INVALID, (entry, "the base call is refused", msg)
        rows = []

        def record(changes):
            nonlocal kept
            rc, msg = H.call(lib, entry, H.with_changes(base, changes))
            if rc == H.E_INVALID:
                rows.append({"set": [list(ch) for ch in changes], "rc": rc, "msg": msg})
                kept += 1
            else:
                dropped.append((entry, changes, rc))
            return rc, msg

        for i, alt in enumerate(alts):
            for x in alt:
                rc, msg = record([(i, x)])
                m = re.search(r"(\d+) needed$", msg) if rc == H.E_INVALID and x == 0 and isinstance(desc[i][0], tuple) else None
                if m:                                               # scratch_bytes = 0 names the need: add need - 1
                    record([(i, int(m.group(1)) - 1)])
        first = [(i, alt[0]) for i, alt in enumerate(alts) if alt]   # one fault per argument, in argument order
        pairs = [[p, q] for p, q in zip(first, first[1:])] + ([[first[0], first[-1]]] if len(first) > 2 else [])
        for changes in pairs + EXTRA.get(entry, []):
            record(changes)
        print(f"{entry}: {len(rows)} rows")
        entries.append({"entry": entry, "base": base, "rows": rows})
    print(f"dropped {len(dropped)} rows that were not answered with UMLH_E_INVALID:")
    for entry, changes, rc in dropped:
        print(f"  {entry} {changes} -> {rc}")
    blocks = ['{"entry": %s, "base": %s, "rows": [\n%s\n]}' % (json.dumps(e["entry"]), json.dumps(e["base"]),
                                                              ",\n".join(" " + json.dumps(r) for r in e["rows"])) for e in entries]
    with open(a.out, "w") as fo:                                    # one row per line
        fo.write('{"entries": [\n' + ",\n".join(blocks) + "\n]}\n")
    print(f"{a.out}: {kept} rows of {len(entries)} entry points, {len(dropped)} dropped, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
