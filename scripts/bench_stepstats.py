#!/usr/bin/env python3
"""Time of the per-step logged statistics (umlh.seq_step_stats, multibench.train.train(step_diagnostics=True)).

    python scripts/bench_stepstats.py [--reps R] [--runs N] [--parent-json FILE ...] [--out profiles/stepstats_bench.txt]

1. One ``umlh.seq_step_stats(x, lengths, recon)`` call against the reference's torch-op form of the same three values
   (MultiBench/train.py:404-426, with its ``.item()`` reads) on the same GPU, at B 32 x T 50 x D 35, B 32 x T 50 x D 300 and
   B 128 x T 50 x D 371.  Wall-clock time around a device-synchronised call, after a warm-up, the two forms alternating; the HIP
   call is timed with one read of its four values, which the training loop does not even pay per step.
2. The MOSEI-shaped alternation step of scripts/bench_multibench.py (z = 40, 100 steps) through ``multibench.train.train``:
   flag off and flag on at this tree, alternating in one process; and flag off at the parent commit, read from
   ``--parent-json`` files.  ms per step: median, min and max over the runs; the parent's max - min is its run-to-run spread.

``--train-only`` prints part 2, flag off, for the tree the script file lives in, as one JSON line: copy this script into
scripts/ of a built checkout of the parent commit, run it there with ``--train-only > FILE`` before and after the main run on
the same GPU, and hand the files to ``--parent-json``."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)
import torch  # noqa: E402

DEV = "cuda:0"
SHAPES = ((32, 50, 35), (32, 50, 300), (128, 50, 371))


def reference_form(x, lengths, recon):
    """train.py:415-424 and :431 for one modality: the torch ops, the [B, T, D] temporaries and the two reads to the host."""
    trivial = x[:, :-1, :] - x[:, 1:, :]
    mask = torch.arange(x.shape[1], device=lengths.device).unsqueeze(0) < lengths.unsqueeze(1)
    mask_expanded = mask.unsqueeze(-1).expand_as(x)
    trivial = (trivial ** 2) * mask_expanded[:, :-1, :].float()
    trivial = trivial.sum() / (mask_expanded[:, :-1, :].float().sum() + 1e-8)
    rec = ((recon[:, :-1, :] - x[:, 1:, :]) ** 2 * mask_expanded[:, 1:, :].float()).sum() / (mask_expanded[:, 1:, :].float().sum() + 1e-8)
    return rec.item(), trivial.item()


def wall_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def bench_call(B, T, D, reps):
    import umlh
    g = torch.Generator(device=DEV).manual_seed(B + D)
    x, recon = torch.randn(B, T, D, device=DEV, generator=g), torch.randn(B, T, D, device=DEV, generator=g)
    lengths = torch.randint(5, T + 1, (B,), device=DEV, generator=g)
    hip = lambda: umlh.seq_step_stats(x, lengths, recon).tolist()
    enqueue = lambda: umlh.seq_step_stats(x, lengths, recon)
    ref = lambda: reference_form(x, lengths, recon)
    got, want = hip(), ref()
    assert abs(got[0] - want[1]) <= 1e-5 * want[1] and abs(got[2] - want[0]) <= 1e-5 * want[0], (got, want)
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < 0.5:
        hip(), ref(), enqueue()
    t = {"hip": [], "hip_no_read": [], "torch": []}
    for _ in range(reps):
        t["hip"].append(wall_us(hip))
        t["torch"].append(wall_us(ref))
        t["hip_no_read"].append(wall_us(enqueue))
    med = {k: round(statistics.median(v), 1) for k, v in t.items()}
    return {"what": "one call, wall us around a synchronised call (median)", "B": B, "T": T, "D": D,
            "hip_seq_step_stats_with_read_us": med["hip"], "hip_seq_step_stats_enqueue_and_sync_us": med["hip_no_read"],
            "reference_torch_ops_with_items_us": med["torch"], "min_us": {k: round(min(v), 1) for k, v in t.items()}}


def bench_train(runs, steps=100, flags=(False, True)):
    """ms per step of multibench.train.train over `steps` MOSEI-shaped batch pairs (z = 40), `runs` runs per flag, alternating."""
    import inspect
    from bench_multibench import build
    from engine.optimizer.optim import build_optimizer
    from multibench.train import train
    has_flag = "step_diagnostics" in inspect.signature(train).parameters
    torch.manual_seed(0)
    m = build(40)
    opt = build_optimizer(m.parameters(), "adam", 1e-3, 0.0)
    g = torch.Generator(device=DEV).manual_seed(1)
    B, T = 32, 50
    x, y = torch.randn(B, T, 35, generator=g, device=DEV), torch.randn(B, T, 300, generator=g, device=DEV)
    lx, ly = torch.randint(5, T + 1, (B,), generator=g, device=DEV), torch.randint(5, T + 1, (B,), generator=g, device=DEV)
    loader = [([x, None, y], [lx, None, ly])] * steps

    def one(flag):
        kw = {"step_diagnostics": True} if flag else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train(m, "xy", loader, loader, opt, num_epoch=1, step_k=-1, ds_name="mosei", device=DEV, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    flags = [f for f in flags if has_flag or not f]
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < 2.0:                  # warm-up: clocks, allocator, every code path
        for f in flags:
            one(f)
    t = {f: [] for f in flags}
    for _ in range(runs):
        for f in flags:
            t[f].append(one(f))
    return {("flag_on" if f else "flag_off"): [round(v, 4) for v in ts] for f, ts in t.items()}


def summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": min(ts), "max": max(ts), "spread": round(max(ts) - min(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-json", nargs="*", default=[], help="outputs of --train-only runs in a checkout of the parent commit")
    ap.add_argument("--train-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stepstats_bench.txt"))
    args = ap.parse_args()
    if args.train_only:
        print(json.dumps(bench_train(args.runs, flags=(False,))), flush=True)
        return
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    for shape in SHAPES:
        say(bench_call(*shape, args.reps))
    parent = []
    for path in args.parent_json:
        with open(path) as f:
            parent += json.loads(f.read().strip().splitlines()[-1])["flag_off"]
    here = bench_train(args.runs)
    r = {"what": "MOSEI-shaped alternation step through multibench.train.train, z = 40, 100 steps per run, ms per step",
         "flag_off_runs": here["flag_off"], "flag_off": summary(here["flag_off"]), "flag_on_runs": here["flag_on"],
         "flag_on": summary(here["flag_on"])}
    r["flag_on_minus_off_median_ms"] = round(r["flag_on"]["median"] - r["flag_off"]["median"], 4)
    if parent:
        r.update(parent_flag_off_runs=parent, parent_flag_off=summary(parent))
        r["flag_off_minus_parent_median_ms"] = round(r["flag_off"]["median"] - r["parent_flag_off"]["median"], 4)
        r["flag_off_within_parent_spread"] = bool(r["flag_off_minus_parent_median_ms"] <= r["parent_flag_off"]["spread"])
    else:
        r["parent_flag_off"] = "not measured: no --parent-json given"
    say(r)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
