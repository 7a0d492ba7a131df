#!/usr/bin/env python3
"""Time of the robustness test sets (multibench/robustness.py, multibench.data.robust_loaders,
multibench.train.evaluate_robustness; kernel sl_perturb of umlh_kernels_seqload.hip) on one GPU.

    python scripts/bench_robustness.py [--runs N] [--out profiles/robustness_bench.txt] [--skip-evaluate]

Synthetic fp32 splits of MOSEI's size (train 16 265, valid 1 869, test 4 643 samples x 50 x 35/74/300, batch 32), front-padded
with zeros to random lengths.
  1. the kernel alone at 4 643 x 50 x 300 and 4 643 x 50 x 35, sample units with eps and keep: ten launches enqueued back to
     back behind a fill (so that all ten are queued before the first may start) between two device events, time / 10, as a
     median with the range over ``--runs`` repetitions, and the achieved bytes/s, bytes = what a launch must move (4 bytes
     read and 4 written per word, 9 per unit of draws, 4 per sample of start).  With start_out, without it, and without it
     followed by umlh_seq_first_nonzero as a second pass; the per-step unit as well.
  2. one level's table build through robust_loaders (family robust_timeseries, level 3: upload of the draws, three perturb
     launches, the build with its one read-back): wall clock around a synchronised build; the same arithmetic in torch ops
     on the same GPU (fp64 add, where, the first nonzero row by ne / any / argmax); and this script's own restatement of the
     reference's host loop (one numpy slice update per sample and draw) on the CPU.
  3. one whole evaluate_robustness (3 families x 10 levels; z = 40, the model of scripts/bench_multibench.py) next to one
     evaluate on the same config, wall clock, synchronised.
No threshold is fixed in advance: the file records every side measured in the same run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
BACK_TO_BACK = 10
T_LEN, DIMS, BATCH = 50, (35, 74, 300), 32
N_SPLIT = {"train": 16265, "valid": 1869, "test": 4643}


def make_split(n, seed):
    g = np.random.default_rng(seed)
    start = g.integers(0, T_LEN - 4, n)
    front = np.arange(T_LEN)[None, :, None] < start[:, None, None]
    split = {k: np.where(front, np.float32(0), g.standard_normal((n, T_LEN, d), dtype=np.float32))
             for k, d in zip(("vision", "audio", "text"), DIMS)}
    split["text"][np.arange(n), start, 0] = 1.0
    split["labels"] = g.standard_normal((n, 1, 1), dtype=np.float32)
    split["id"] = np.arange(n).reshape(n, 1)
    return split


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def bench_kernel(n, d, runs):
    from umlh import seqload
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((n, T_LEN, d), device=DEV, generator=g)
    out = torch.empty_like(x)
    start = torch.empty(n, dtype=torch.int32, device=DEV)
    head = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)                  # the fill the launches queue behind
    words = x.numel()
    res = {"shape": [n, T_LEN, d], "MB_table": round(4 * words / 1e6, 1)}
    for per_step in (False, True):
        units = n * T_LEN if per_step else n
        eps = torch.randn(units, dtype=torch.float64, device=DEV, generator=g) * 0.3
        keep = (torch.rand(units, device=DEV, generator=g) >= 0.3).to(torch.uint8)
        forms = {"fused_start": lambda: seqload.perturb(x, eps, keep, per_step=per_step, out=out, start_out=start),
                 "no_start": lambda: seqload.perturb(x, eps, keep, per_step=per_step, out=out),
                 "two_pass": lambda: seqload.first_nonzero(seqload.perturb(x, eps, keep, per_step=per_step, out=out))}
        if per_step:
            forms.pop("no_start")
        for name, fn in forms.items():
            us = []
            for rep in range(runs + 2):                                        # the first two repetitions warm up
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                head.zero_()
                e0.record()
                for _ in range(BACK_TO_BACK):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    us.append(e0.elapsed_time(e1) * 1e3 / BACK_TO_BACK)
            nbytes = 8 * words + 9 * units + (4 * n if name != "no_start" else 0)    # two_pass: what the fused form must move
            key = ("step_" if per_step else "sample_") + name
            res[key] = {"us": spread(us), "GB_per_s_at_median": round(nbytes / (statistics.median(us) * 1e-6) / 1e9, 1)}
    return res


def torch_level(base, draws):
    """One level of robust_timeseries in torch ops: fp64 add and one rounding, assignment on drop, first nonzero text row."""
    out = []
    for x, (eps, keep) in zip(base, draws):
        e = torch.from_numpy(eps).to(DEV)
        k = torch.from_numpy(keep).to(DEV)
        y = (x.double() + e[:, None, None]).float()
        out.append(torch.where(k[:, None, None] != 0, y, torch.zeros((), device=DEV)))
    rows = (out[2] != 0).any(dim=2)
    start = torch.where(rows.any(dim=1), rows.int().argmax(dim=1), torch.full((), T_LEN, device=DEV)).int()
    start.cpu()
    return out, start


def host_level(arrays, p, rng):
    """The reference's host loop, restated: one slice update per sample and draw, all normals before all uniforms."""
    for a in arrays:
        for u in range(a.shape[0]):
            a[u] += rng.normal(0, p)
    for a in arrays:
        for u in range(a.shape[0]):
            if rng.random_sample() < p:
                a[u] = np.zeros(a[u].shape)
    return arrays


def bench_build(test, runs):
    from multibench.data import robust_loaders
    from multibench.robustness import draw_timeseries_noise
    levels = robust_loaders({"test": test}, "robust_timeseries", batch_size=BATCH, data_type="mosei", device=DEV, rng=0)
    levels.table(1)                                                            # warm-up
    t_dev = []
    for _ in range(runs):
        levels.table(0)
        t_dev.append(wall(lambda: levels.table(3))[0] * 1e3)
    n = levels.base[0].shape[0]
    draws = draw_timeseries_noise([n, n, n], 0.1, rng=1)
    torch_level(levels.base, draws)
    t_torch = [wall(lambda: torch_level(levels.base, draws))[0] * 1e3 for _ in range(runs)]
    rng = np.random.RandomState(2)
    t_host = []
    for _ in range(max(1, runs // 3)):
        arrays = [test[k].copy() for k in ("vision", "audio", "text")]
        t0 = time.perf_counter()
        host_level(arrays, 0.1, rng)
        t_host.append((time.perf_counter() - t0) * 1e3)
    return {"samples": n, "robust_loaders_level_build_ms": spread(t_dev), "torch_ops_same_arithmetic_ms": spread(t_torch),
            "host_loop_numpy_ms": spread(t_host)}


def bench_evaluate(data, runs):
    from bench_multibench import build
    from multibench.data import get_dataloader, robust_loaders
    from multibench.train import evaluate, evaluate_robustness
    torch.manual_seed(0)
    model = build(40, DIMS[0], DIMS[2])
    train, valid, test = get_dataloader(data, batch_size=BATCH, train_shuffle=False, data_type="mosei", device=DEV)
    cfg = {"train": list(train), "val": list(valid), "test": list(test)}
    families = ("robust_vision", "robust_audio", "robust_timeseries")
    t_build = wall(lambda: {f: robust_loaders(data, f, batch_size=BATCH, data_type="mosei", device=DEV, rng=i)
                            for i, f in enumerate(families)})
    robust = t_build[1]
    evaluate(model, cfg, "mosei", device=DEV)                                  # warm-up
    t_eval, t_rob = [], []
    for _ in range(runs):
        t_eval.append(wall(lambda: evaluate(model, cfg, "mosei", device=DEV))[0])
        s, res = wall(lambda: evaluate_robustness(model, cfg, robust, "mosei", device=DEV))
        t_rob.append(s)
    return {"evaluate_s": spread(t_eval, 3), "evaluate_robustness_30_levels_s": spread(t_rob, 3),
            "robust_loaders_construction_3_families_s": round(t_build[0], 3),
            "batches": {"train": len(cfg["train"]), "test": len(cfg["test"])},
            "mean_score_xy": {f: round(res[f"robust/{f}/mean_score_xy"], 4) for f in families},
            "n_last_level": {f: res[f"robust/{f}/n"][-1] for f in families}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--skip-evaluate", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robustness_bench.txt"))
    args = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}",
             "note: kernel times are device events around ten back-to-back launches / 10, median and range over the runs; builds and "
             "evaluations are wall clock around synchronised work"]

    def record(name, value):
        lines.append(json.dumps({name: value}))
        print(lines[-1], flush=True)
    for d in (300, 35):
        record("kernel", bench_kernel(N_SPLIT["test"], d, args.runs))
    test = make_split(N_SPLIT["test"], 7)
    record("level_build", bench_build(test, args.runs))
    if not args.skip_evaluate:
        data = {"train": make_split(N_SPLIT["train"], 5), "valid": make_split(N_SPLIT["valid"], 6), "test": test}
        record("evaluate", bench_evaluate(data, max(1, args.runs // 3)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
