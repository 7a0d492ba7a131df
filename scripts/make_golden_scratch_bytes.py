"""Records what the fourteen public scratch-size queries of include/umlh.h answer: tests/golden/scratch_bytes.json, rows
[name, args, bytes], replayed by tests/test_scratch_layout_cpu.py.  Every metric launcher carves its scratch block by the same
plan its query sizes it with, so a change to a plan that keeps every row keeps every layout's end.

    python scripts/make_golden_scratch_bytes.py [--lib path/to/libumlh.so]

Run it against a library built from the commit whose sizes are to be kept.  The queries are host arithmetic: no GPU is needed.

Per query the grid holds the smallest and the largest legal shape, both sides of every threshold of the plan code (row counts
around 32, 64, 128, 256 and 4096, widths around 4, 32, 64 and 1024, splits 0 and explicit, max_iter 0 / 1 / 1000, history
1 / 32, classes 2 / 4096), and tuples with one illegal argument, which answer 0: every one-at-a-time change of a mid-sized
tuple, the largest tuple and its neighbours, and a seeded sample of the product of the value lists (grid()).  The feature widths of the CKA
forms, the k-NN searches and the class statistics have no upper limit; their lists stop at 4096 (2^31 - 1 for the class
statistics, whose plan is linear in d)."""
import argparse
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd")):
    sys.path.insert(0, p)

I31 = (1 << 31) - 1
ROWS = [1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 65536, 1 << 20]
WIDTHS = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 1023, 1024]
SPLITS = [0, 1, 3, 64, 5000]


def grid(legal, illegal, sample, seed):
    """Tuples over the per-argument lists `legal`: the first, the middle and the last tuple; every one-at-a-time change of the
    middle one (each value of each list: both sides of every threshold); the last one with each argument at its first and
    its middle value (the largest shapes); a seeded sample of `sample` tuples of the product for the interactions.  Then,
    per argument, its `illegal` values in the middle tuple."""
    first, mid, last = (tuple(v[0] for v in legal), tuple(v[len(v) // 2] for v in legal), tuple(v[-1] for v in legal))
    rows = [first, mid, last]
    for i, vals in enumerate(legal):
        rows += [mid[:i] + (x,) + mid[i + 1:] for x in vals]
        rows += [last[:i] + (x,) + last[i + 1:] for x in (vals[0], vals[len(vals) // 2])]
    rng = random.Random(seed)
    rows += [tuple(rng.choice(v) for v in legal) for _ in range(sample)]
    for i, vals in enumerate(illegal):
        rows += [mid[:i] + (x,) + mid[i + 1:] for x in vals]
    return list(dict.fromkeys(rows))


def queries():
    """name -> list of argument tuples"""
    q = {}
    n_align = ROWS + [1 << 30]
    d_cka = WIDTHS + [1025, 4096]
    q["umlh_align_scratch_bytes"] = grid([n_align, d_cka, d_cka, [0, 1, 10, 32], SPLITS],
                                         [[0, -1, (1 << 30) + 1], [0, -1], [0], [-1, 33], [-1]], 20, 1)
    ext = []
    for kind in (0, 1):                                                   # unbiased, RBF
        ext += [(kind,) + t for t in grid([n_align, d_cka, d_cka, [0], SPLITS], [[0, (1 << 30) + 1], [0], [0, -1], [], [-1]], 15, 2 + kind)]
    for kind in (2, 3):                                                   # CKNNA, list statistics
        ext += [(kind,) + t for t in grid([n_align, [1], [1], [1, 2, 10, 32], [0]], [[0, (1 << 30) + 1], [], [], [0, 33], []], 5, 2 + kind)]
    ext += [(4, 100, 8, 8, 4, 0), (-1, 100, 8, 8, 4, 0)]
    q["umlh_align_ext_scratch_bytes"] = ext
    n_probe = ROWS[1:] + [I31]
    q["umlh_probe_scratch_bytes"] = grid([n_probe, WIDTHS, [0, 1, 2, 100, 1000]], [[0, 1, I31 + 1], [0, 1025], [-1, 1001]], 20, 6)
    q["umlh_softmax_probe_scratch_bytes"] = grid([ROWS[1:] + [(1 << 30) - 1], WIDTHS + [1025, 2047, 2048], [2, 3, 4, 5, 63, 64, 65, 1000, 4096],
                                                  [0, 1, 1000], [1, 2, 32]],
                                                 [[1, I31], [0, 2049], [1, 4097], [-1, 1001], [0, 33]], 30, 7)
    n_knn = ROWS + [I31]
    q["umlh_knn_scratch_bytes"] = grid([n_knn, n_knn, [1, 64, 4096], [1, 5, 16, 24], SPLITS],
                                       [[0, I31 + 1], [0, I31 + 1], [0], [0, 25], [-1]], 20, 8)
    q["umlh_spectral_scratch_bytes"] = grid([[1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 65535], ROWS + [I31], [1, 4, 31, 32, 33, 64, 65, 511, 512]],
                                            [[0, 65536], [0, I31 + 1], [0, 513]], 20, 9)
    d_sub = [1, 2, 4, 31, 32, 33, 63, 64, 65, 511, 512]
    q["umlh_subspace_scratch_bytes"] = grid([ROWS[1:] + [I31], d_sub, [0] + d_sub, [1, 2, 31, 32, 33, 63, 64]],
                                            [[1, I31 + 1], [0, 513], [-1, 513], [0, 65]], 30, 10)
    q["umlh_paired_cosine_scratch_bytes"] = grid([ROWS + [4098, I31, 1 << 40, 1 << 62], [1, 4, 1024, I31]], [[0, -1], [0]], 10, 11)
    q["umlh_seq_step_stats_scratch_bytes"] = grid([[1, 2, 31, 32, 33, 64, 4096, 65535], [1, 2, 3, 64, 65, 66, 129, 4097, 1 << 20],
                                                   WIDTHS + [1025, 2049, 1 << 20]], [[0, 65536], [0], [0]], 20, 12)
    q["umlh_seq_spectrum_scratch_bytes"] = grid([[1, 2, 15, 16, 17, 32, 33, 4096, 1 << 20], [1, 2, 3, 4, 63, 64, 65, 1023, 1024],
                                                 WIDTHS + [15, 16, 17, 1025, 1 << 20]], [[0, (1 << 20) + 1], [0, 1025], [0]], 20, 13)
    classes = [1, 2, 3, 32, 33, 255, 256, 257, 4096, 1 << 20, 1 << 28, I31]
    q["umlh_class_index_scratch_bytes"] = grid([ROWS + [(1 << 28) - 1, 1 << 28, (1 << 28) + 1, I31], classes], [[0, I31 + 1], [0, -1]], 20, 14)
    q["umlh_class_stats_scratch_bytes"] = grid([ROWS + [I31], [1, 4, 64, 1024, I31], classes], [[0, I31 + 1], [0], [0]], 20, 15)
    q["umlh_eval_topk_scratch_bytes"] = grid([n_knn, n_knn, [1, 64, 4096], [1, 5, 16, 24], SPLITS],
                                             [[0, I31 + 1], [0, I31 + 1], [0], [0, 25], [-1]], 20, 16)
    out = []
    for kind in (0, 2):                                                   # row quantile, k-NN accuracy
        out += [(kind,) + t for t in grid([ROWS + [4098, 16384, 16385, I31, I31 + 1, (1 << 40) - 1], [1, 4, 64, 1024]],
                                          [[0, 1 << 40], [0, I31 + 1]], 5, 17 + kind)]
    out += [(1,) + t for t in grid([[1, 256, (1 << 40) - 1], [1, 1024]], [[0, 1 << 40], [0, I31 + 1]], 0, 18)]      # global k-th: one size
    out += [(3, 100, 8), (-1, 100, 8), (0, 1 << 30, 1 << 20)]
    q["umlh_outlier_scratch_bytes"] = out
    return q


def record(lib):
    rows = []
    for name, tuples in queries().items():
        fn = getattr(lib, name)
        rows += [[name, list(t), int(fn(*t))] for t in tuples]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="libumlh.so to record (default: the in-tree build)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "scratch_bytes.json"))
    args = ap.parse_args()
    from umlh import _lib
    if args.lib:
        lib = ctypes.CDLL(args.lib)
        for name, (restype, argtypes) in _lib.PROTOTYPES.items():
            if name.endswith("_scratch_bytes"):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, list(argtypes)
    else:
        import umlh
        lib = umlh.load_library()
    rows = record(lib)
    lines = [""]                                   # several rows to a line of about 300 characters
    for r in rows:
        text = json.dumps(r, separators=(",", ":"))
        if lines[-1] and len(lines[-1]) + len(text) > 300:
            lines.append("")
        lines[-1] += ("," if lines[-1] else "") + text
    with open(args.out, "w") as f:
        f.write("[\n" + ",\n".join(lines) + "\n]\n")
    zeros = sum(1 for r in rows if r[2] == 0)
    print(f"{len(rows)} rows ({zeros} answer 0) of {len(queries())} queries -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
