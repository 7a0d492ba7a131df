#!/usr/bin/env python3
"""One umlh.align.measure_pairs call against the loop of single calls (align.cka + align.mutual_knn per pair) over the same
tensors, on the same GPU in the same process.  The loop of single calls is the yardstick; the grouped call is never its own.

    python scripts/bench_align_group.py [--reps R] [--calls K] [--out profiles/align_group_bench.txt]

A window is a pair of device events around K back-to-back evaluations of all pairs of a case (grouped: K measure_pairs calls;
single: K times the loop), so it holds what a training loop pays per evaluation: the launches and the host code that issues
them.  Both paths are warmed up by one window each; then R windows of each, alternating; median with min and max, in us per
evaluation.  ``spread``: (max - min) / median of the single-call windows.  ``gain``: single median / grouped median.
``host_us``: the host clock around issuing the K evaluations of a window, before any wait, per evaluation (medians): where it is
below the window's device time the window is bound by the device, not by the code that issues the calls.

Cases: G in {1, 2, 6, 12, 48} pairs at N 2 000 (the Gaussian toy's validation embeddings) with d 10 + 10 and d 128 + 128, topk
10; and the four pairs of one embedding capture at the MOSEI shape (N 27 500: 40 + 40 twice, 35 + 300, and 40 + 300 CKA only)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

DEV = "cuda:0"


def summary(ts):
    return {"median": round(statistics.median(ts), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}


def event_us(fn, calls):
    """(device us, host us to issue) per evaluation of one window."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    host = time.perf_counter() - t0
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls, host * 1e6 / calls


def case(name, pairs, calls, reps):
    from umlh import align

    def grouped():
        return align.measure_pairs(pairs, topk=10)

    def single():
        out = []
        for pr in pairs:
            a, b = pr[0], pr[1]
            out.append(align.cka(a, b))
            if len(pr) == 2:
                out.append(align.mutual_knn(a, b, 10))
        return out

    for fn in (grouped, single):
        event_us(fn, calls)
    tg, ts, hg, hs = [], [], [], []
    for _ in range(reps):
        d, h = event_us(grouped, calls)
        tg.append(d); hg.append(h)
        d, h = event_us(single, calls)
        ts.append(d); hs.append(h)
    mg, ms = statistics.median(tg), statistics.median(ts)
    return {"case": name, "pairs": len(pairs), "grouped_us": summary(tg), "single_us": summary(ts),
            "grouped_host_us": round(statistics.median(hg), 1), "single_host_us": round(statistics.median(hs), 1),
            "grouped_us_per_pair": round(mg / len(pairs), 1), "single_us_per_pair": round(ms / len(pairs), 1),
            "spread": round((max(ts) - min(ts)) / ms, 3), "spread_grouped": round((max(tg) - min(tg)) / mg, 3), "gain": round(ms / mg, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_group_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align_group.py measures on the GPU; none is visible")
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# scripts/bench_align_group.py on {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs), "
             f"reps={args.reps}, evaluations per window={args.calls}",
             "# grouped: one align.measure_pairs call; single: align.cka + align.mutual_knn(topk 10) pair after pair; us per evaluation"]

    def emit(obj):
        lines.append(obj if isinstance(obj, str) else json.dumps(obj))
        print(lines[-1], flush=True)

    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    for d in (10, 128):
        emit(f"# N 2000, d {d} + {d}")
        z = torch.randn(48, 2000, d, device=DEV, generator=g)
        w = z * 0.5 + torch.randn(48, 2000, d, device=DEV, generator=g)
        for G in (1, 2, 6, 12, 48):
            emit(case(f"N=2000 d={d}+{d} G={G}", [(z[i], w[i]) for i in range(G)], args.calls, args.reps))
        del z, w
    emit("# the four pairs of one embedding capture at the MOSEI shape")
    n = 27500
    mk = lambda d: torch.randn(n, d, device=DEV, generator=g)
    pairs = [(mk(40), mk(40)), (mk(40), mk(40)), (mk(35), mk(300)), (mk(40), mk(300), {"topk": 0})]
    emit(case("capture N=27500 (40+40, 40+40, 35+300, 40+300 cka only)", pairs, max(2, args.calls // 4), args.reps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
