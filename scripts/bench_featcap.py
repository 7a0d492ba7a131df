"""Time of the fine-tune loop's feature capture (feature_capture.FeatureCapture.step), of umlh.class_stats alone and of the
reference's torch-op form of the same quantities (vision_language/finetune.py:209-233: the per-class loop with ``nonzero``,
two reductions and an ``.item()``) on the same GPU, and of finetune.train() with the capture off.

    python scripts/bench_featcap.py [--reps R] [--out profiles/featcap_bench.txt]
    python scripts/bench_featcap.py --train-flag-off [--root TREE] [--repeats R] [--steps K]

Shapes of the first form: 1000 classes x 16 rows at d = 512 and d = 1024, 100 x 16 at d = 512; the model is UML with an
img_proj of d -> d, the text sample has one row per class (so CKA runs and mutual k-NN, whose row counts disagree, does not:
what the ImageNet configuration gives).  ``class_stats`` moves 2 n d 4 bytes (the rows are read twice); its rate is that over
the device time between two events.  A capture step and the reference form end in a read-back, so they are wall-clock times
around a synchronised call.

``--train-flag-off`` times ``train()`` for K steps at the cfg2 shape (d 512, 1000 classes, batches of 4096 image + 4096 text
rows from a 200 000-row image table and a 29 940-row text table, bf16 step) without the capture argument; ``--root`` names
another checkout of this repository to import from (it uses nothing this script's own commit adds), so two commits can be
timed alternately on one machine."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths(root):
    for p in (root, os.path.join(root, "unpaired-multimodal-learning_amd"), os.path.join(HERE, "scripts")):
        sys.path.insert(0, p)


DEV = "cuda:0"


def wall(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return [round(ts[len(ts) // 2], 1), round(ts[0], 1), round(ts[-1], 1)]


def reference_class_part(img_features, labels, n_class):
    """finetune.py:222-231 on device tensors, as written."""
    import numpy as np
    import torch
    means, dists = [], []
    for label in range(n_class):
        indices = (labels == label).nonzero(as_tuple=True)[0]
        m = img_features[indices].mean(dim=0)
        dists.append(torch.norm(img_features[indices] - m.unsqueeze(0), dim=1).mean().item())
        means.append(m.unsqueeze(0))
    return torch.cat(means, dim=0), np.mean(dists)


def capture_timings(args):
    import torch
    import umlh
    from bench_align import ref_cka, timed
    from engine.models.head import UML
    from feature_capture import FeatureCapture
    lines = [json.dumps({"device": torch.cuda.get_device_name(0)})]

    def say(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    for n_class, d in ((1000, 512), (1000, 1024), (100, 512)):
        g = torch.Generator(device=DEV).manual_seed(n_class + d)
        n = n_class * 16
        rows = torch.nn.functional.normalize(torch.randn(n, d, device=DEV, generator=g), dim=1)
        labels = torch.arange(n_class, device=DEV).repeat_interleave(16)[torch.randperm(n, device=DEV, generator=g)]
        text = torch.nn.functional.normalize(torch.randn(n_class, d, device=DEV, generator=g), dim=1)
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            model = UML(d, d, n_class).to(DEV)
            cap = FeatureCapture(model, rows, labels, text, n_class, keep_features=False)
        feats = torch.empty(n, d, device=DEV)
        cap._features_into(feats)
        shape = f"{n_class} x 16 rows, d {d}"
        step = wall(lambda: [float(v) for v in cap.step()], args.reps)
        us = timed(lambda: umlh.class_stats(feats, cap.order, cap.offsets, n_class, means_out=cap.means), 30)
        idx = timed(lambda: umlh.class_index(labels, n_class), 10)
        feat_us = timed(lambda: cap._features_into(feats), 20)
        cka_us = timed(lambda: umlh.align.cka(cap.means, text), 20)
        say({"what": "FeatureCapture.step() incl. the read-back of its three scalars, wall us (median, min, max)", "shape": shape,
             "step_us": step, "of_which_device_us": {"extract_features": round(feat_us, 1), "class_stats": round(us, 1),
                                                      "cka": round(cka_us, 1)}})
        say({"what": "umlh.class_stats alone, device us between events (median of 30)", "shape": shape, "us": round(us, 1),
             "bytes_moved": 2 * n * d * 4, "GB_per_s": round(2 * n * d * 4 / (us * 1e-6) / 1e9, 1),
             "class_index_once_per_run_us": round(idx, 1)})

        def ref_step():
            with torch.no_grad():
                f = torch.cat([model.extract_features(rows[j:j + 512]).detach() for j in range(0, n, 512)], dim=0)
                means, dist = reference_class_part(f, labels, n_class)
                return dist, ref_cka(means, text).item()
        say({"what": "the reference's torch-op form on the same GPU, wall us (median, min, max)", "shape": shape,
             "class_loop_with_item_us": wall(lambda: reference_class_part(feats, labels, n_class), max(2, args.reps // 2), warm=1),
             "whole_step_us": wall(ref_step, max(2, args.reps // 2), warm=1)})
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def train_flag_off(args, what="capture off"):
    import torch
    import finetune as ft
    from engine.datasets.utils import FeatureLoader, FeatureTable
    from engine.models.head import UMLClip
    from engine.optimizer.optim import build_optimizer
    from engine.optimizer.scheduler import build_lr_scheduler
    d, c, b = 512, 1000, 4096

    def rows(n, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        return (torch.nn.functional.normalize(torch.randn(n, d, device=DEV, generator=g), dim=1),
                torch.randint(0, c, (n,), device=DEV, generator=g))
    ti, tt, tv = FeatureTable(*rows(200_000, 1), DEV), FeatureTable(*rows(29_940, 2), DEV), FeatureTable(*rows(4096, 3), DEV)

    def once(steps):
        torch.manual_seed(5)
        model = UMLClip(d, c, logit_scale_init=4.60517).to(DEV)
        opt = build_optimizer(model.parameters(), "adamw", 1e-3, 0.01)
        sch = build_lr_scheduler(opt, "cosine", 50, 12800, warmup_type="linear", warmup_lr=1e-5)
        mk = lambda t, kind, sh: FeatureLoader(t, b, shuffle=sh, kind=kind, order_rng="device")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            ft.train(model, mk(ti, "image", True), mk(tt, "text", True), mk(tv, "image", False), None, opt, sch, device=DEV,
                     max_iters=steps, alpha=1.0, eval_freq=10 ** 6, patience=5, precision="bf16")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    once(50)
    ts = [round(once(args.steps), 2) for _ in range(args.repeats)]
    print(json.dumps({"what": f"train() {args.steps} steps, cfg2 shape, bf16, {what}, wall ms per run", "root": args.root,
                      "ms": ts, "median_ms": sorted(ts)[len(ts) // 2]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "featcap_bench.txt"))
    ap.add_argument("--train-flag-off", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    _paths(os.path.abspath(a.root))
    train_flag_off(a) if a.train_flag_off else capture_timings(a)
