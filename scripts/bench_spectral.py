"""Device time (events, medians) and accuracy of umlh.spectral against the reference's form on the same GPU
(torch.linalg.svdvals in fp32 + the formula of MultiBench/utilis.py:27-36), and the per-step cost of
``multibench.train.train(effective_rank=True)`` on the MOSEI-shaped alternation step of scripts/bench_multibench.py.

    python scripts/bench_spectral.py [--reps R] [--steps S] [--only-kernels]

Writes profiles/spectral_bench.txt (times; no speed bar is set) and profiles/spectral_accuracy.txt (errors of both routes
against float64 numpy and their ratio).  ``--only-kernels`` runs the HIP op once per size and writes nothing: the run
to put under a kernel trace."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import umlh  # noqa: E402
import _spectral_ref as R  # noqa: E402
from bench_align import DEV, timed  # noqa: E402

SIZES = ((1, 1600, 35), (1, 1600, 300), (1, 50000, 300), (8, 1600, 300))


def ref_effective_rank(a, eps=1e-6):
    sv = torch.linalg.svdvals(a)
    p = sv / sv.sum(dim=-1, keepdim=True)
    return torch.exp(-torch.sum(p * torch.log(p + eps), dim=-1)), sv


def accuracy_cases():
    g = np.random.default_rng(0)
    yield "gaussian 1600x300", g.standard_normal((1600, 300))
    yield "column scales over 1e5, 1600x300", g.standard_normal((1600, 300)) * np.logspace(0, -5, 300)
    yield "exact rank 12, 700x300", g.standard_normal((700, 12)) @ g.standard_normal((12, 300))
    yield "offset columns 257x35", 3.0 + g.standard_normal((257, 35))
    yield "wide 40x64", g.standard_normal((40, 64))
    yield "common mean 5000x300", 5.0 + g.standard_normal((5000, 300))


def step_time(steps, with_rank, B=32, T=50, z=40):
    """ms per alternation step through multibench.train.train on a fixed batch pair (bench_multibench.py's shapes)."""
    from engine.optimizer.optim import build_optimizer
    from bench_multibench import build
    from multibench import train as mbt
    torch.manual_seed(0)
    m = build(z)
    opt = build_optimizer(m.parameters(), "adam", 1e-3, 0.0)
    g = torch.Generator(device=DEV).manual_seed(1)
    x, y = torch.randn(B, T, 35, generator=g, device=DEV), torch.randn(B, T, 300, generator=g, device=DEV)
    lx, ly = (torch.randint(5, T + 1, (B,), generator=g, device=DEV) for _ in range(2))
    batch = [[x, None, y], [lx, None, ly]]
    run = lambda n: mbt.train(m, "xy", [batch] * n, [batch] * n, opt, modalities=[0, 2], num_epoch=1, step_k=-1, device=DEV,
                              effective_rank=with_rank)
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < 1.0:                  # >= 1 s of warm-up: the first steps run at idle clocks
        run(5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--only-kernels", action="store_true")
    args = ap.parse_args()
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    if args.only_kernels:
        for batch, n, d in SIZES:
            umlh.effective_rank(torch.randn(batch, n, d, device=DEV, generator=g))
        torch.cuda.synchronize()
        return
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "unit": "us, median of device-event times"})]
    for batch, n, d in SIZES:
        a = torch.randn(batch, n, d, device=DEV, generator=g)
        r = {"batch": batch, "n": n, "d": d}
        r["hip_effective_rank_us"] = timed(lambda: umlh.effective_rank(a), args.reps)
        r["torch_svdvals_formula_us"] = timed(lambda: ref_effective_rank(a), max(3, args.reps // 2), warm=1)
        r["torch_over_hip"] = r["torch_svdvals_formula_us"] / r["hip_effective_rank_us"]
        r["values"] = [umlh.effective_rank(a).cpu().tolist(), ref_effective_rank(a)[0].cpu().tolist()]
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    off_ms, off = step_time(args.steps, False)
    on_ms, on = step_time(args.steps, True)
    r = {"step": "MOSEI-shaped alternation step (B 32, T 50, x 35, y 300, z 40) through multibench.train.train",
         "effective_rank_off_ms": round(off_ms, 4), "effective_rank_on_ms": round(on_ms, 4),
         "cost_of_the_switch_ms_per_step": round(on_ms - off_ms, 4), "steps": args.steps,
         "last_pred_effective_rank_y": on["pred_effective_rank_y"][-1],
         "gt_effective_rank_y": on["gt_effective_rank_y"]}
    lines.append(json.dumps(r))
    print(lines[-1], flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "spectral_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")

    acc = [json.dumps({"device": torch.cuda.get_device_name(0), "errors": "max|sv - sv64| / sigma_max and |erank - erank64| / erank64 "
                       "against float64 numpy; torch = torch.linalg.svdvals fp32 on this GPU and on the CPU"})]
    for name, a64 in accuracy_cases():
        a = a64.astype(np.float32)
        sv64, er64 = R.svdvals64(a), R.erank64(a)
        x = torch.from_numpy(a).to(DEV)
        er, sv = umlh.effective_rank(x, return_svdvals=True)
        hip = R.errors(sv.cpu().numpy(), float(er), sv64, er64)
        ter, tsv = ref_effective_rank(x)
        gpu = R.errors(tsv.cpu().numpy(), float(ter), sv64, er64)
        cer, csv = ref_effective_rank(torch.from_numpy(a))
        cpu = R.errors(csv.numpy(), float(cer), sv64, er64)
        r = {"case": name, "hip_sv_err": hip[0], "hip_erank_err": hip[1], "torch_gpu_sv_err": gpu[0], "torch_gpu_erank_err": gpu[1],
             "torch_cpu_sv_err": cpu[0], "torch_cpu_erank_err": cpu[1],
             "torch_cpu_over_hip_sv": cpu[0] / hip[0] if hip[0] else float("inf"),
             "torch_cpu_over_hip_erank": cpu[1] / hip[1] if hip[1] else float("inf")}
        acc.append(json.dumps(r))
        print(acc[-1], flush=True)
    with open(os.path.join(ROOT, "profiles", "spectral_accuracy.txt"), "w") as f:
        f.write("\n".join(acc) + "\n")


if __name__ == "__main__":
    main()
