#!/usr/bin/env python3
"""Grouped sweeps of the Gaussian toy (gaussian.fused.GroupedTrainer on umlh_ae_train_steps_grouped: two launches per step for
a whole group of runs) against the same runs stepped one after another through FusedTrainer.steps, on the same GPU in the same
process.  The sequential fused path is the yardstick everywhere; the grouped code is never its own yardstick.

    python scripts/bench_gaussian_sweep.py [--reps R] [--steps N] [--only-sweeps] [--out profiles/gaussian_sweep_bench.txt]

A window is a pair of device events around N >= 2 000 steps of every member (grouped: one GroupedTrainer.steps(N); sequential:
FusedTrainer.steps(N) member after member).  Every trainer holds one id span of N steps that each window walks again (its
counter is put back before the window), so a window has no host id generation and no upload in it; every shape is warmed up by
one window of each path; R windows of each path, alternating; median with min and max.  ``member_us``: us per step and member.
``spread_seq``: (max - min) / median of the sequential windows.  ``gain``: sequential member_us / grouped member_us (medians).

1. Train steps alone at the paper's widths (50, 128, 10, batch 512), members alternating 'xy' / 'x' as the YAMLs do,
   G in {1, 2, 3, 6, 12, 24, 48}.
2. The diff_dim_latent.yaml group (L in {5, 10, 20, 50, 100} x 3 seeds x 2 modes = 30 members) as one group, as five groups of
   six in grid order, and sequentially; the diff_batch_sizes.yaml group (batch 1 .. 512 x 3 x 2 = 60 members) as one group, as
   ten groups of six, and sequentially.
3. Whole sweeps: original.yaml's six runs x 1 000 steps through gaussian.sweep.sweep_grouped (one group of six) and through six
   build_run + train_model_steps_fused calls, (eval_every, alignment) = (1, False), (1, True), (100, True): host clock around
   everything from building the models to a final synchronise, after a 20-step warm-up of both."""
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
PAPER = dict(dim_common=128, dim_latent=10, data_dim_common=10, data_dim_x=5, data_dim_y=5, dim_obs=50, num_steps=10000, noise_std=0.09,
             train_num_samples=10000, batch_size=512, val_num_samples=2000, lr=1.0e-3, seed=[0, 1, 2], alpha_x=1.0, alpha_y=1.0,
             mode=["xy", "x"], attenuation=0.05, tag="original", unrelated_info=False)
GROUP_SIZES = (1, 2, 3, 6, 12, 24, 48)


def summary(ts, digits=2):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits)}


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def members(points, steps):
    """One FusedTrainer per point over shared device tables, each with one id span of ``steps`` steps, and the points' settings."""
    from gaussian import sweep
    from gaussian.fused import FusedTrainer
    trainers, settings = [], []
    for p in points:
        p = sweep._full(p)
        ds, gen, model, opt = sweep.build_point(p, DEV)
        dev = sweep._device_data(p, DEV)
        tables = (dev["x"], dev["y2"] if (p["mode"] != "xy" or p["unrelated_info"]) else dev["y"])
        trainers.append(FusedTrainer(model, opt, ds, p["batch_size"], gen, DEV, span_steps=steps, tables=tables))
        settings.append((p["mode"], p["alpha_x"], p["alpha_y"]))
    return trainers, settings


def rewind(trainers):
    for t in trainers:
        t._used = 0


def windows(trainers, settings, splits, steps, reps):
    """us per step of all members: grouped in the consecutive groups ``splits`` (a list of group lengths), and sequential."""
    from gaussian.fused import GroupedTrainer
    groups, at = [], 0
    for n in splits:
        groups.append(GroupedTrainer(trainers[at:at + n], settings[at:at + n]))
        at += n
    assert at == len(trainers)

    def grouped():
        for g in groups:
            g.steps(steps)

    def sequential():
        for t, (mode, ax, ay) in zip(trainers, settings):
            t.steps(steps, mode=mode, alpha_x=ax, alpha_y=ay)

    for fn in (grouped, sequential):                      # warm-up: the first call also draws every trainer's id span
        fn()
        rewind(trainers)
    tg, ts = [], []
    for _ in range(reps):
        tg.append(event_us(grouped) / steps)
        rewind(trainers)
        ts.append(event_us(sequential) / steps)
        rewind(trainers)
    return tg, ts


def row(name, n, tg, ts):
    mg, ms = statistics.median(tg), statistics.median(ts)
    return {"case": name, "members": n, "grouped_us_per_step": summary(tg), "sequential_us_per_step": summary(ts),
            "grouped_member_us": round(mg / n, 2), "sequential_member_us": round(ms / n, 2),
            "spread_seq": round((max(ts) - min(ts)) / ms, 3), "gain": round(ms / mg, 2)}


def paper_points(g):
    from gaussian.sweep import expand_grid
    base = expand_grid(dict(PAPER, seed=0))                # 'xy', 'x'
    return [dict(base[i % 2], seed=i // 2) for i in range(g)]


def train_step_parts(args, emit):
    """Parts 1 and 2: windows of train steps alone."""
    from gaussian import sweep
    emit("# 1. train steps alone, (D, C, L, batch) = (50, 128, 10, 512), members alternating 'xy' / 'x'")
    best = None
    for g in GROUP_SIZES:
        trainers, settings = members(paper_points(g), args.steps)
        r = row(f"paper G={g}", g, *windows(trainers, settings, [g], args.steps, args.reps))
        emit(r)
        if best is None or r["grouped_member_us"] < best[1]:
            best = (g, r["grouped_member_us"])
        del trainers
    emit(f"# best member-step: G = {best[0]} ({best[1]} us)")

    for name, key, values in (("diff_dim_latent", "dim_latent", [5, 10, 20, 50, 100]),
                              ("diff_batch_sizes", "batch_size", [1, 2, 4, 8, 16, 32, 64, 128, 256, 512])):
        emit(f"# 2. {name}.yaml: {key} in {values} x 3 seeds x 2 modes")
        grid = {k: (values if k == key else v) for k, v in PAPER.items()}          # key order as in the file
        points = sweep.expand_grid(grid)
        trainers, settings = members(points, args.steps)
        n = len(points)
        emit(row(f"{name} one group of {n}", n, *windows(trainers, settings, [n], args.steps, args.reps)))
        emit(row(f"{name} {n // 6} groups of 6", n, *windows(trainers, settings, [6] * (n // 6), args.steps, args.reps)))
        del trainers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussian_sweep_bench.txt"))
    ap.add_argument("--skip-sweeps", action="store_true", help="leave out part 3")
    ap.add_argument("--only-sweeps", action="store_true", help="part 3 alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gaussian_sweep.py measures on the GPU; none is visible")
    if args.steps < 2000:
        raise SystemExit("a window is at least 2000 steps")
    from gaussian import sweep
    from gaussian.train import train_model_steps_fused
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# scripts/bench_gaussian_sweep.py on {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs), "
             f"reps={args.reps}, steps per window={args.steps}",
             "# grouped: GroupedTrainer.steps (two launches per step for the group); sequential: FusedTrainer.steps member after member"]

    def emit(obj):
        lines.append(obj if isinstance(obj, str) else json.dumps(obj))
        print(lines[-1], flush=True)

    if not args.only_sweeps:
        train_step_parts(args, emit)

    if not args.skip_sweeps:
        emit("# 3. original.yaml: six runs x 1000 steps, wall seconds from building the models to a final synchronise")
        points = sweep.expand_grid(PAPER)

        def grouped(n, ev, al):
            sweep.sweep_grouped(points, num_steps=n, eval_every=ev, alignment=al, group_size=6, device=DEV)

        def sequential(n, ev, al):
            for p in points:
                _, _, val = sweep.make_data(p)
                ds, gen, model, opt = sweep.build_point(p, DEV)
                train_model_steps_fused(model, ds, opt, n, val["x"], val["y"], DEV, batch_size=p["batch_size"], generator=gen, mode=p["mode"],
                                        alpha_x=p["alpha_x"], alpha_y=p["alpha_y"], eval_every=ev, alignment=al)

        def wall(fn, *a):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(*a)
            torch.cuda.synchronize()
            return time.perf_counter() - t

        for ev, al in ((1, False), (1, True), (100, True)):
            grouped(20, ev if ev == 1 else 10, al)
            sequential(20, ev if ev == 1 else 10, al)
            tg, ts = [], []
            for _ in range(3):
                tg.append(wall(grouped, 1000, ev, al))
                ts.append(wall(sequential, 1000, ev, al))
            emit({"case": f"original.yaml eval_every={ev} alignment={al}", "grouped_s": summary(tg, 4), "sequential_s": summary(ts, 4), "gain": round(statistics.median(ts) / statistics.median(tg), 2)})

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
