"""Device + host time of one embedding capture (multibench.capture.EmbeddingCapture.measure) at the MOSEI shape against the
reference's form of the same work in torch on the same GPU, and of the two kernels of umlh_kernels_capture.hip alone.

    python scripts/bench_capture.py [--reps R] [--out profiles/capture_bench.txt]

MOSEI shape: 1000 sequences in batches of 32, T 50, vision 35-d / text 300-d, the 5-layer z = 40 model of
scripts/bench_multibench.py.  The reference's form (MultiBench/train.py:456-512): the same eval forwards, then one ``.item()``
and six slices per sequence, ``torch.cat``, ``F.cosine_similarity(...).mean().item()`` and the metrics as
vision_language/metrics.py writes them (the forms scripts/bench_align.py times), each read back with ``.item()``.  The
capture synchronises, so wall-clock time around a synchronised call is what a training loop pays."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import umlh  # noqa: E402
from bench_align import ref_cka, ref_mknn, timed  # noqa: E402
from bench_multibench import build  # noqa: E402
from multibench.capture import EmbeddingCapture, take_fixed_samples  # noqa: E402

DEV = "cuda:0"


def wall(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def mosei_loaders(n=1000, bs=32, T=50):
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(n, T, 35, generator=g), torch.randn(n, T, 300, generator=g)
    lx = torch.randint(5, T + 1, (n,), generator=g)
    ly = torch.cat([lx[s:s + bs].roll(1) for s in range(0, n, bs)])               # equal totals, different layout
    mk = lambda a, la: [([a[s:s + bs], None, a[s:s + bs]], [la[s:s + bs], None, la[s:s + bs]]) for s in range(0, n, bs)]
    return mk(x, lx), [([None, None, y[s:s + bs]], [None, None, ly[s:s + bs]]) for s in range(0, n, bs)]


def reference_measure(model, cap, metrics=True):
    """train.py:456-512 on the capture's device batches: per-sequence .item() + slices, cat, the reference metric forms."""
    model.eval()
    keys = ("zx", "zy", "x_proj", "y_proj", "x_recon", "y_recon")
    parts = {k: [] for k in keys}
    with torch.no_grad():
        for x1, x2, l1, l2 in zip(cap.x1, cap.x2, cap.l1, cap.l2):
            out = model(x1, x2, l1, l2)
            for j in range(x1.shape[0]):
                n1, n2 = l1[j].item(), l2[j].item()
                for k in keys:
                    parts[k].append(out[k][j, :(n1 if k in ("zx", "x_proj", "x_recon") else n2), :])
    m = {k: torch.cat(v, dim=0) for k, v in parts.items()}
    res = [F.cosine_similarity(m["x_proj"], m["y_proj"], dim=1).mean().item(), F.cosine_similarity(m["zx"], m["zy"], dim=1).mean().item()]
    if metrics:
        for a, b in (("x_proj", "y_proj"), ("zx", "zy"), ("x_recon", "y_recon")):
            res += [ref_cka(m[a], m[b]).item(), ref_mknn(m[a], m[b], 10).item()]
        res.append(ref_cka(m["zy"], cap.raw_y).item())
    model.train()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_bench.txt"))
    args = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    torch.manual_seed(0)
    model = build(40).train()
    l1, l2 = mosei_loaders()
    cap = EmbeddingCapture(take_fixed_samples(l1, l2, [0, 2], "mosei"), DEV)
    n = cap.rows
    r = {"what": "one capture at the MOSEI shape, wall ms incl. the read-back (median, min, max)", "sequences": 1000, "T": 50, "rows": n}
    r["hip_measure_ms"] = [round(v, 2) for v in wall(lambda: cap.measure(model), args.reps)]
    say(r)
    free, _ = torch.cuda.mem_get_info()
    fits = 8 * n * n * 4 < 0.8 * free
    r = {"what": "the reference's form of the same capture on the same GPU, wall ms (median, min, max)", "rows": n}
    r["ref_slices_cat_cosine_ms"] = [round(v, 2) for v in wall(lambda: reference_measure(model, cap, metrics=False), max(2, args.reps // 2))]
    if fits:
        r["ref_with_metrics_ms"] = [round(v, 2) for v in wall(lambda: reference_measure(model, cap), 1, warm=0)]
    else:
        r["ref_with_metrics_ms"] = f"does not fit: the reference metric forms need several {n} x {n} fp32 arrays"
    say(r)
    # the forwards alone, to read the figures above against
    def forwards():
        model.eval()
        with torch.no_grad():
            for x1, x2, a, b in zip(cap.x1, cap.x2, cap.l1, cap.l2):
                model(x1, x2, a, b)
        model.train()
    say({"what": "the 32 eval forwards alone, wall ms (median, min, max)", "forwards_ms": [round(v, 2) for v in wall(forwards, args.reps)]})
    # the kernels alone (device time, events)
    g = torch.Generator(device=DEV).manual_seed(2)
    z = torch.randn(1000, 50, 300, device=DEV, generator=g)
    lens = torch.randint(5, 51, (1000,), device=DEV, generator=g)
    rows = int(lens.sum())
    out = torch.empty(rows, 300, device=DEV)
    us = timed(lambda: umlh.seq_compact(z, lens, out=out), 20)
    say({"what": "umlh.seq_compact alone", "shape": "1000 x 50 x 300", "rows": rows, "us": round(us, 1),
         "GB_per_s": round(2 * rows * 300 * 4 / (us * 1e-6) / 1e9, 1)})
    ref = timed(lambda: torch.cat([z[j, :k] for j, k in enumerate(lens.tolist())], dim=0), 5)
    say({"what": "per-sequence slices + cat (lengths already on the host)", "shape": "1000 x 50 x 300", "us": round(ref, 1)})
    a, b = torch.randn(50000, 300, device=DEV, generator=g), torch.randn(50000, 300, device=DEV, generator=g)
    us = timed(lambda: umlh.paired_cosine(a, b), 20)
    say({"what": "umlh.paired_cosine alone", "shape": "50000 x 300", "us": round(us, 1),
         "GB_per_s": round(2 * 50000 * 300 * 4 / (us * 1e-6) / 1e9, 1)})
    ref = timed(lambda: F.cosine_similarity(a, b, dim=1).mean(), 20)
    say({"what": "F.cosine_similarity(a, b, dim=1).mean() (fp32, torch ops)", "shape": "50000 x 300", "us": round(ref, 1)})
    z2 = torch.randn(1000, 50, 40, device=DEV, generator=g)
    out2 = torch.empty(rows, 40, device=DEV)
    say({"what": "umlh.seq_compact alone", "shape": "1000 x 50 x 40", "us": round(timed(lambda: umlh.seq_compact(z2, lens, out=out2), 20), 1)})
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
