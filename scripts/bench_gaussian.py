#!/usr/bin/env python3
"""Step time of the Gaussian toy: the composed path (gaussian.train.train_model_steps over the LinearFn / _DecoderNextStepMSE
autograd nodes, a host DataLoader and an H2D copy per step) against the fused path (gaussian.fused.FusedTrainer on
umlh_ae_train_steps: two launches per step, batches gathered by index on the device), on the same GPU in the same process.

    python scripts/bench_gaussian.py [--reps R] [--out profiles/gaussian_bench.txt]

1. us per step at (D, C, L, batch) = (50, 128, 10, 512), (50, 128, 500, 512), (100, 128, 100, 512), (50, 256, 10, 512),
   (50, 128, 10, 1), modes 'xy' and 'x', 10 000 training rows.  Both paths are warmed up at every shape; a window is a host clock
   around N steps that end in a device synchronise (composed: 200 steps, fused: 10 000 steps in one trainer call, the index
   upload of the span included: about half a second each); R windows of each, alternating; median, min and max.
2. The two launches alone (umlh_ae_bench_steps, the benchmark-only entry of csrc/umlh_launch.h: part 1 / 2 of every step; not
   a training call and not part of the C ABI), device events around 5 000 steps of one C loop.  ``B_GFLOP_per_s``: 2 rows N K
   over the tensors launch B forms a gradient for (rows of the views that feed each) over its time.  ``A_GB_per_s``: the bytes launch A moves over its time: per 16-row tile the eleven weight matrices it walks
   (six forward, five backward) and their biases, per row the table row twice (gather, residual) and the 2 D + 4 C + 6 L
   floats it leaves in scratch.  Both are the algorithm's counts from the shapes, not counters.
3. 1 000 steps with eval_every = 1 and alignment = True on 2 000 validation rows through both loops (host clock, one window each
   after a 20-step warm-up): the loop the reference's configs run."""
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
SHAPES = [(50, 128, 10, 512), (50, 128, 500, 512), (100, 128, 100, 512), (50, 256, 10, 512), (50, 128, 10, 1)]
N_TRAIN = 10000
COMPOSED_STEPS, FUSED_STEPS, LAUNCH_STEPS = 200, 10000, 5000


def summary(ts):
    return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}


def data(D, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(n, D, generator=g), "y": torch.randn(n, D, generator=g)}


def host_us_per_step(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / steps


def event_us_per_step(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def bench_steps(tr, n, mode, part):
    """n steps of the trainer's current id span through umlh_ae_bench_steps: part 0 = whole steps, 1 = launch A, 2 = launch B."""
    import ctypes as C
    from umlh import _glue as glue
    from umlh import gauss
    from umlh._lib import OPT_IDS, AeCfg, check, load_library
    fn = load_library().umlh_ae_bench_steps
    vp, pv, i32, f64 = C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_double
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(AeCfg), pv, pv, pv, vp, C.c_int64, vp, i32, vp, C.c_int64, vp, i32, i32, i32, C.c_float,
                                        C.c_float, i32, f64, C.c_int64, f64, f64, f64, f64, f64, vp, vp, C.c_uint64, i32, vp]
    params = [p.data for p in tr.params]
    Cc, D = params[0].shape
    cfg = AeCfg(D, Cc, params[4].shape[0])
    b, g = tr.batch_size, tr.optimizer.param_groups[0]
    scratch, nbytes = gauss._scratch(tr.device, cfg, b, b, 1)
    losses = torch.empty((n, 3), dtype=torch.float32, device=tr.device)
    check(fn(C.byref(cfg), glue.ptr_array(params), glue.ptr_array(tr.m), glue.ptr_array(tr.v), glue.ptr(tr.x), D, glue.ptr(tr._idx_x), b,
             glue.ptr(tr.y), D, glue.ptr(tr._idx_y), b, n, 1 if mode == "xy" else 0, 1.0, 1.0, OPT_IDS[tr.optimizer.name], g["lr"],
             tr.optimizer.step_count + 1, g["betas"][0], g["betas"][1], g["eps"], g["momentum"], g["weight_decay"], losses.data_ptr(),
             scratch.data_ptr(), nbytes, part, glue.stream(tr.device)), "umlh_ae_bench_steps")


def launch_counts(D, C, L, batch, mode):
    """(flops of launch B, bytes of launch A) of one step, from the shapes."""
    rows = {"x": batch, "y": batch}
    back = {"x": True, "y": mode == "xy"}
    both = sum(rows[v] for v in "xy" if back[v])
    flops = 0
    for v in "xy":
        if back[v]:
            flops += 2 * rows[v] * (C * D + D * C)
    flops += 2 * both * (L * C + L * L + L * L + C * L)
    weights = 4 * (C * D + L * C + L * L + L * L + C * L + D * C + 2 * C + 3 * L + D)
    bytes_a = 0
    for v in "xy":
        tiles = (rows[v] + 15) // 16
        walks = 2 if back[v] else 1
        bytes_a += tiles * weights * walks + rows[v] * 4 * (2 * D + (2 * D + 4 * C + 6 * L if back[v] else 0))
    return flops, bytes_a


def bench_shape(D, C, L, batch, mode, reps):
    from gaussian.fused import FusedTrainer
    from gaussian.train import build_run, train_model_steps
    d = data(D, N_TRAIN)
    kw = dict(mode=mode, train_num_samples=N_TRAIN, batch_size=batch, seed=0, dim_obs=D, dim_common=C, dim_latent=L, device=DEV)
    loader, model_c, opt_c = build_run(d, d, **kw)
    ds, gen, model_f, opt_f = build_run(d, d, fused=True, **kw)
    trainer = FusedTrainer(model_f, opt_f, ds, batch, gen, DEV, span_steps=FUSED_STEPS)
    vx, vy = d["x"][:64].to(DEV), d["y"][:64].to(DEV)
    composed = lambda n: train_model_steps(model_c, loader, opt_c, n, vx, vy, DEV, mode=mode, eval_every=0)
    fused = lambda n: trainer.steps(n, mode=mode)
    composed(20)
    fused(FUSED_STEPS)
    tc, tf = [], []
    for _ in range(reps):
        tc.append(host_us_per_step(lambda: composed(COMPOSED_STEPS), COMPOSED_STEPS))
        tf.append(host_us_per_step(lambda: fused(FUSED_STEPS), FUSED_STEPS))
    row = {"shape": [D, C, L, batch], "mode": mode, "composed_us_per_step": summary(tc), "fused_us_per_step": summary(tf),
           "speedup_of_medians": round(statistics.median(tc) / statistics.median(tf), 1)}
    # the launches alone: a trainer whose index span covers one window (every window re-reads the same ids: no host work, no upload)
    wide = FusedTrainer(model_f, opt_f, ds, batch, gen, DEV, span_steps=LAUNCH_STEPS)
    wide.steps(LAUNCH_STEPS, mode=mode)
    both, ta, tb = [], [], []
    for _ in range(reps):
        for part, dst in ((0, both), (1, ta), (2, tb)):
            dst.append(event_us_per_step(lambda: bench_steps(wide, LAUNCH_STEPS, mode, part), LAUNCH_STEPS))
    flops, bytes_a = launch_counts(D, C, L, batch, mode)
    row.update(step_device_us=summary(both), launch_A_us=summary(ta), launch_B_us=summary(tb),
               B_GFLOP_per_s=round(flops / statistics.median(tb) / 1e3, 1), A_GB_per_s=round(bytes_a / statistics.median(ta) / 1e3, 1))
    return row


def bench_eval_loop():
    from gaussian.train import build_run, train_model_steps, train_model_steps_fused
    D, C, L, batch = SHAPES[0]
    d = data(D, N_TRAIN)
    val = data(D, 2000, seed=1)
    vx, vy = val["x"].to(DEV), val["y"].to(DEV)
    kw = dict(mode="xy", train_num_samples=N_TRAIN, batch_size=batch, seed=0, dim_obs=D, dim_common=C, dim_latent=L, device=DEV)
    out = {}
    loader, model, opt = build_run(d, d, **kw)
    run = lambda n: train_model_steps(model, loader, opt, n, vx, vy, DEV, eval_every=1, alignment=True)
    run(20)
    out["composed_us_per_step"] = round(host_us_per_step(lambda: run(1000), 1000), 1)
    ds, gen, model, opt = build_run(d, d, fused=True, **kw)
    run = lambda n: train_model_steps_fused(model, ds, opt, n, vx, vy, DEV, batch_size=batch, generator=gen, eval_every=1, alignment=True)
    run(20)
    out["fused_us_per_step"] = round(host_us_per_step(lambda: run(1000), 1000), 1)
    out["speedup"] = round(out["composed_us_per_step"] / out["fused_us_per_step"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussian_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gaussian.py measures on the GPU; none is visible")
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# scripts/bench_gaussian.py on {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs), reps={args.reps}",
             "# composed: train_model_steps (autograd nodes, host loader); fused: FusedTrainer.steps (two launches per step)"]
    for D, C, L, batch in SHAPES:
        for mode in ("xy", "x"):
            row = bench_shape(D, C, L, batch, mode, args.reps)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    lines.append("# 1000 steps, eval_every=1, alignment=True, 2000 validation rows, shape (50, 128, 10, 512), mode xy")
    lines.append(json.dumps(bench_eval_loop()))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
