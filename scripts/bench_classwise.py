"""Time of the class-wise validation report (finetune.validate_classwise), of umlh.topk_classes and umlh.class_report alone and
of the torch-op form of the same quantities on the same GPU (``x @ w.T * s``, ``topk``, ``bincount``, the confusion matrix by
``bincount(label * C + pred)``: it materialises the n x C logits), and of finetune.train() with the report off.

    python scripts/bench_classwise.py [--reps R] [--out profiles/classwise_bench.txt]
    python scripts/bench_classwise.py --train-flag-off [--root TREE] [--repeats R] [--steps K]

Shapes of the first form: 50 000 rows x 1000 classes at d = 512 and d = 1024, 2 500 rows x 100 classes at d = 512; the model is
UMLClip (scale 100) over an unshuffled FeatureLoader, top-5, with and without the confusion matrix.  ``topk_classes`` does
2 n C d flops in its candidate pass and reads x and w once per 32-row strip / column chunk; its time is device time between two
events.  ``validate_classwise`` and the torch-op form end in a read-back, so they are wall-clock times around a synchronised
call.

``--train-flag-off`` times ``train()`` for K steps at the cfg2 shape (d 512, 1000 classes, batches of 4096 image + 4096 text
rows from a 200 000-row image table and a 29 940-row text table, bf16 step) without the ``classwise`` argument; ``--root``
names another checkout of this repository to import from (it uses nothing this script's own commit adds), so two commits can
be timed alternately on one machine."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths(root):
    for p in (root, os.path.join(root, "unpaired-multimodal-learning_amd"), os.path.join(HERE, "scripts")):
        sys.path.insert(0, p)


DEV = "cuda:0"


def torch_form(x, w, scale, labels, n_class, k, confusion):
    """The same report from torch ops on the n x C logits; one read-back, as validate_classwise makes."""
    import torch
    z = (x @ w.T) * scale
    top = z.topk(k, dim=1).indices
    pred = top[:, 0]
    parts = [torch.bincount(labels, minlength=n_class), torch.bincount(labels[pred == labels], minlength=n_class),
             torch.bincount(labels[(top == labels[:, None]).any(1)], minlength=n_class)]
    if confusion:
        parts.append(torch.bincount(labels * n_class + pred, minlength=n_class * n_class))
    return torch.cat(parts).cpu()


def report_timings(args):
    import torch
    import umlh
    import finetune as ft
    from bench_align import timed
    from bench_featcap import wall
    from engine.datasets.utils import FeatureLoader, FeatureTable
    from engine.models.head import UMLClip
    lines = [json.dumps({"device": torch.cuda.get_device_name(0)})]

    def say(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    k = 5
    for n, n_class, d in ((50_000, 1000, 512), (50_000, 1000, 1024), (2_500, 100, 512)):
        g = torch.Generator(device=DEV).manual_seed(n_class + d)
        x = torch.nn.functional.normalize(torch.randn(n, d, device=DEV, generator=g), dim=1)
        labels = torch.randint(0, n_class, (n,), device=DEV, generator=g)
        torch.manual_seed(0)
        model = UMLClip(d, n_class, logit_scale_init=4.60517).to(DEV)
        with torch.no_grad():
            model.head.weight.copy_(torch.nn.functional.normalize(torch.randn(n_class, d, device=DEV, generator=g), dim=1))
        loader = FeatureLoader(FeatureTable(x, labels, DEV), 32, shuffle=False)
        w, scale = model.head.weight.detach(), model._scales[0]
        shape = f"{n} rows x {n_class} classes, d {d}, top-{k}"
        cls, _ = umlh.topk_classes(x, w, None, scale, k=k)
        us = timed(lambda: umlh.topk_classes(x, w, None, scale, k=k), 20)
        rep_us = timed(lambda: umlh.class_report(cls, labels, n_class), 20)
        conf_us = timed(lambda: umlh.class_report(cls, labels, n_class, confusion=True), 20)
        say({"what": "umlh.topk_classes alone (one call over all rows), device us between events (median of 20)", "shape": shape,
             "us": round(us, 1), "candidate_pass_flops": 2 * n * n_class * d,
             "TFLOP_per_s_fp32": round(2 * n * n_class * d / (us * 1e-6) / 1e12, 2),
             "class_report_us": round(rep_us, 1), "class_report_with_confusion_incl_its_memset_us": round(conf_us, 1)})
        for confusion in (False, True):
            ours = wall(lambda: ft.validate_classwise(model, loader, topk=k, confusion=confusion), args.reps)
            ref = wall(lambda: torch_form(x, w, scale, labels, n_class, k, confusion), args.reps)
            say({"what": "validate_classwise (4096-row slabs, one read-back) against the torch-op form on the n x C logits, wall us "
                         "(median, min, max)", "shape": shape, "confusion": confusion, "validate_classwise_us": ours,
                 "torch_form_us": ref, "logits_bytes_the_torch_form_materialises": n * n_class * 4})
        got = ft.validate_classwise(model, loader, topk=k, confusion=True)
        want = torch_form(x, w, scale, labels, n_class, k, True)
        same = [bool(torch.equal(got[a], want[j * n_class:(j + 1) * n_class])) for j, a in enumerate(("support", "correct", "correct_topk"))]
        say({"what": "rows on which the two forms count differently (fp64 refinement against fp32 logits)", "shape": shape,
             "support_equal": same[0], "top1_count_difference": int((got["correct"] - want[n_class:2 * n_class]).abs().sum()),
             "topk_count_difference": int((got["correct_topk"] - want[2 * n_class:3 * n_class]).abs().sum()),
             "top1_acc": got["top1_acc"], "topk_acc": got["topk_acc"]})
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "classwise_bench.txt"))
    ap.add_argument("--train-flag-off", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    _paths(os.path.abspath(a.root))
    if a.train_flag_off:
        from bench_featcap import train_flag_off          # the same loop: train() without any of the optional arguments
        train_flag_off(a, what="classwise off")
    else:
        report_timings(a)
