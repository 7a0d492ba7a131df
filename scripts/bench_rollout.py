#!/usr/bin/env python3
"""Time of the one-launch rollout (multibench.train.rollout on umlh.rollout_rows) and of umlh.seq_spectrum.

    python scripts/bench_rollout.py [--reps R] [--out profiles/rollout_bench.txt]

1. A 49-step rollout of one modality of the MOSEI-shaped model (5 layers, d_ff 2048, conv1d, sinusoidal positions) at batch 32 and
   1000, modality widths 35 and 300, z = 40 and z = 300, three ways on the same GPU:
     one_launch    multibench.train.rollout: every step of every row in one launch;
     hip_modules   the reference's loop (train.py:277-281) through this project's xproj_in / encoder / decoder modules at T = 1;
     torch_nn      the same loop through torch.nn ops (nn.Linear, nn.TransformerEncoder in eval mode) on the same parameters.
   Device events around each call, every variant warmed up for every shape, the three alternating within one process;
   median, min and max in ms.  ``GB_per_s_per_workgroup`` = the weight bytes one workgroup walks per step,
   4 (D Z + Z^2 + L (2 Z^2 + 2 Z d_ff) + Z D), over the one-launch time per step.
2. ``umlh.seq_spectrum`` against ``torch.abs(torch.fft.rfft(x, dim=1)).mean(dim=(0, 2))`` at 32 x 50 x 300 and 1000 x 50 x 300."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)
import torch  # noqa: E402

DEV = "cuda:0"
STEPS, LAYERS, D_FF = 49, 5, 2048


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


@torch.no_grad()
def module_loop(m, proj, dec, x, steps):
    frames, cur = [x], x
    for _ in range(steps):
        cur = dec(m.encoder(proj(cur[:, -1, :].unsqueeze(1))))
        frames.append(cur)
    return torch.cat(frames, dim=1)


@torch.no_grad()
def torch_loop(m, proj, dec, x, steps):
    enc = m.encoder
    frames, cur = [x], x
    for _ in range(steps):
        h = proj.fc(cur[:, -1, :].unsqueeze(1))                               # [B, 1, Z]
        h = enc.conv(h.transpose(1, 2)).permute(2, 0, 1) + enc.pos_table[:1].unsqueeze(1)    # [1, B, Z]
        cur = dec.fc(enc.transformer(h).transpose(0, 1))
        frames.append(cur)
    return torch.cat(frames, dim=1)


def bench_rollout(B, D, z, reps):
    from bench_multibench import build
    from multibench.train import rollout
    torch.manual_seed(z + D)
    m = build(z).eval()
    x_side = D == 35
    proj, dec = (m.xproj_in, m.decoders[0]) if x_side else (m.yproj_in, m.decoders[1])
    x = torch.randn(B, 1, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(B))
    variants = {"one_launch": lambda: rollout(m, x, None, steps=STEPS)[0] if x_side else rollout(m, None, x, steps=STEPS)[1],
                "hip_modules": lambda: module_loop(m, proj, dec, x, STEPS), "torch_nn": lambda: torch_loop(m, proj, dec, x, STEPS)}
    outs = {k: f() for k, f in variants.items()}                              # also the first warm-up
    agree = {k: float((outs[k] - outs["one_launch"]).abs().max() / outs["one_launch"].abs().max()) for k in ("hip_modules", "torch_nn")}
    for f in variants.values():
        f()
    t = {k: [] for k in variants}
    for r in range(reps):
        for k, f in variants.items():
            if k == "one_launch" or r < max(3, reps // 4):                    # the launched loops take tens of ms each
                t[k].append(event_ms(f))
    step_bytes = 4 * (D * z + z * z + LAYERS * (2 * z * z + 2 * z * D_FF) + z * D)
    per_step_us = statistics.median(t["one_launch"]) * 1e3 / STEPS
    return {"what": "49-step rollout, ms per call (device events)", "B": B, "D": D, "z": z, "workgroups": (B + 15) // 16,
            **{k: summary(v) for k, v in t.items()}, "one_launch_us_per_step": round(per_step_us, 1),
            "weight_MB_per_step": round(step_bytes / 1e6, 2), "GB_per_s_per_workgroup": round(step_bytes / per_step_us / 1e3, 1),
            "max_rel_diff_to_one_launch": {k: float(f"{v:.2e}") for k, v in agree.items()}}


def bench_spectrum(B, T, d, reps):
    import umlh
    x = torch.randn(B, T, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(B))
    variants = {"hip_seq_spectrum": lambda: umlh.seq_spectrum(x),
                "torch_rfft_abs_mean": lambda: torch.abs(torch.fft.rfft(x, dim=1)).mean(dim=(0, 2))}
    a, b = (f() for f in variants.values())
    rel = float((a - b.double()).abs().max() / a.abs().max())
    for _ in range(5):
        for f in variants.values():
            f()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            t[k].append(event_ms(f) * 1e3)
    return {"what": "spectrum of a [B, T, d] block, us per call (device events)", "B": B, "T": T, "d": d,
            **{k: summary(v) for k, v in t.items()}, "max_rel_diff": float(f"{rel:.2e}")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_bench.txt"))
    args = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    for z in (40, 300):
        for D in (35, 300):
            for B in (32, 1000):
                say(bench_rollout(B, D, z, args.reps))
    for B in (32, 1000):
        say(bench_spectrum(B, 50, 300, 10 * args.reps))


if __name__ == "__main__":
    main()
