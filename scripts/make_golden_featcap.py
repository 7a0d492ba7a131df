#!/usr/bin/env python3
"""Golden vectors for the feature capture of the fine-tune loop by RUNNING THE REFERENCE's vision_language/finetune.py train()
on the CPU with capture_features_during_training=True.  Build machine only: needs the reference checkout and goes through the
import stubs and the identity backbone of oracle/make_golden.py.  Writes tests/golden/feature_capture.npz (data only,
allow_pickle=False).

The reference's ``get_few_shot_image_samples`` (a seed-1 16-shot split of the raw dataset through an image loader) is replaced
by a function that returns fixed feature rows: the first ``shot`` rows of each class of the training table, in table order,
which is what ``finetune.take_capture_samples`` of this build returns.  What the reference logs per step is recorded where it
is formed: ``np.mean(inclass_distances)`` (finetune.py:231; the per-class ``.item()`` values are kept too), the returns of
``cka`` and ``mknn`` (:232-233), every training ``F.cross_entropy``; the five files it saves are read back.

Run A: image modality, UML with img_proj (24 -> 16), 12 classes x 5 sample rows, 6 steps: nontrivial in-class distances, both
       scores 0 (no text sample).  No logger: with text absent the reference's log line calls ``.item()`` on an int (:206,:240).
Run B: crossmodal, 12 sample rows (one per class) and a 12-row text set, 6 steps, with a logger whose rows are compared with
       the recorded values: both scores nontrivial, the in-class distance 0.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as MG            # noqa: E402
RF = MG.ref_finetune
OUT = os.path.join(ROOT, "tests", "golden", "feature_capture.npz")
C, D_IMG, D_TXT, B, STEPS, EVAL_FREQ, LR, WD, ALPHA = 12, 24, 16, 16, 6, 3, 0.05, 0.01, 1.0
FILES = ("all_iter_image_raw_features", "all_iter_image_features", "all_iter_image_labels", "all_iter_text_features",
         "all_iter_text_labels")


class _RecordingNumpy:
    """Stands where finetune.py's ``np`` stands while train() runs: ``mean`` records its argument and its result."""

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, a, *args, **kw):
        v = np.mean(a, *args, **kw)
        self.log.append((np.asarray(a, dtype=np.float64), float(v)))
        return v


def rows(gen, proto, y, noise):
    return torch.nn.functional.normalize(proto[y] + noise * torch.randn(y.numel(), proto.shape[1], generator=gen), dim=1).float()


def first_rows_per_class(y, shot):
    seen, keep = {}, []
    for i, c in enumerate(y.tolist()):
        seen[c] = seen.get(c, 0) + 1
        if seen[c] <= shot:
            keep.append(i)
    return torch.tensor(keep)


def run(tag, modality, shot, n_txt, seed):
    from torch.utils.data import DataLoader
    gen = torch.Generator().manual_seed(4000 + seed)
    proto_i, proto_t = torch.randn(C, D_IMG, generator=gen), torch.randn(C, D_TXT, generator=gen)
    yi = torch.arange(C).repeat_interleave(8)[torch.randperm(C * 8, generator=gen)]        # table order is not class order
    xi = rows(gen, proto_i, yi, 0.6)
    yt = torch.arange(C)[torch.randperm(C, generator=gen)] if n_txt == C else torch.randint(0, C, (n_txt,), generator=gen)
    xt = rows(gen, proto_t, yt, 0.6)
    yv, ye = torch.randint(0, C, (40,), generator=gen), torch.randint(0, C, (47,), generator=gen)
    xv, xe = rows(gen, proto_i, yv, 0.6), rows(gen, proto_i, ye, 0.6)
    keep = first_rows_per_class(yi, shot)
    sx, sy = xi[keep].clone(), yi[keep].clone()

    MG.set_random_seed(seed)
    text_ds = MG.quiet(MG.RefTextDS, xt, yt, torch.zeros(n_txt, dtype=torch.long), n_shots=None)
    model = MG.make_uml(D_IMG, D_TXT, C, False)
    w_head_init, w_proj_init = model.head.weight.detach().clone(), model.img_proj.weight.detach().clone()
    optimizer = MG.ref_build_optimizer(model.parameters(), "adamw", LR, WD)
    scheduler = MG.ref_build_sched(optimizer, "cosine", 50, 1000, warmup_type="linear", warmup_lr=1e-5)
    il = DataLoader(MG.RecordingImageDS(xi, yi), batch_size=B, shuffle=True, num_workers=0, drop_last=False)
    tl = DataLoader(text_ds, batch_size=B, shuffle=True, num_workers=0, drop_last=False) if modality == "crossmodal" else None
    vl = DataLoader(MG.RecordingImageDS(xv, yv), batch_size=B, shuffle=False)
    te = DataLoader(MG.RecordingImageDS(xe, ye), batch_size=B, shuffle=False)

    F = torch.nn.functional
    orig = dict(ce=F.cross_entropy, np=RF.np, cka=RF.cka, mknn=RF.mknn, samples=RF.get_few_shot_image_samples)
    train_ce, means_log, cka_log, mknn_log, logged = [], [], [], [], []

    def rec_ce(a, b, *x, **k):
        v = orig["ce"](a, b, *x, **k)
        if torch.is_grad_enabled():
            train_ce.append(float(v))
        return v

    def rec(fn, log):
        def wrapped(a, b):
            v = fn(a, b)
            log.append(float(v))
            return v
        return wrapped
    F.cross_entropy = rec_ce
    RF.np, RF.cka, RF.mknn = _RecordingNumpy(means_log), rec(orig["cka"], cka_log), rec(orig["mknn"], mknn_log)
    RF.get_few_shot_image_samples = lambda args, shot=1: (sx, sy)
    logger = types.SimpleNamespace(log=lambda d: logged.append(dict(d))) if modality == "crossmodal" else None
    with tempfile.TemporaryDirectory() as tmp:
        try:
            MG.quiet(RF.train, model, il, tl, vl, te, optimizer, scheduler, device="cpu", max_iters=STEPS, alpha=ALPHA,
                     eval_freq=EVAL_FREQ, patience=100, capture_features_during_training=True, features_pth=tmp,
                     args=types.SimpleNamespace(nclasses=C), logger=logger)
        finally:
            F.cross_entropy = orig["ce"]
            RF.np, RF.cka, RF.mknn, RF.get_few_shot_image_samples = orig["np"], orig["cka"], orig["mknn"], orig["samples"]
        saved = {f: torch.load(os.path.join(tmp, f + ".pth")) for f in FILES if os.path.exists(os.path.join(tmp, f + ".pth"))}
    assert len(means_log) == STEPS and len(train_ce) == STEPS * (2 if tl is not None else 1)
    inclass = np.asarray([v for _, v in means_log])
    cka_v = np.asarray(cka_log) if tl is not None else np.zeros(STEPS)
    mknn_v = np.asarray(mknn_log) if tl is not None else np.zeros(STEPS)
    if logger is not None:
        steps = [d for d in logged if "train/inclass_distance" in d]
        assert [float(d["train/inclass_distance"]) for d in steps] == inclass.tolist()
        assert [float(d["train/cka_score"]) for d in steps] == cka_v.tolist()
        assert [float(d["train/mknn_score"]) for d in steps] == mknn_v.tolist()
    rec_ = dict(x_img=xi, y_img=yi, x_txt=xt, y_txt=yt, x_val=xv, y_val=yv, x_test=xe, y_test=ye, sample_x=sx, sample_y=sy,
                w_head_init=w_head_init, w_proj_init=w_proj_init, train_ce=np.asarray(train_ce, dtype=np.float64),
                inclass_distance=inclass, inclass_per_class=np.stack([a for a, _ in means_log]), cka_score=cka_v, mknn_score=mknn_v,
                cfg=np.asarray([D_IMG, D_TXT, C, B, STEPS, EVAL_FREQ, LR, WD, ALPHA, shot, seed], dtype=np.float64),
                modality=modality, saved_files=np.asarray(sorted(saved)))
    for f, t in saved.items():
        rec_["file::" + f] = t.numpy()
    print(f"  {tag}: inclass {inclass} cka {cka_v} mknn {mknn_v} files {sorted(saved)}")
    return {f"{tag}::{k}": (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in rec_.items()}


if __name__ == "__main__":
    torch.set_num_threads(4)
    rec = {}
    rec.update(run("A", "image", 5, C, 31))
    rec.update(run("B", "crossmodal", 1, C, 32))
    np.savez_compressed(OUT, **rec)
    with np.load(OUT, allow_pickle=False) as z:
        assert set(z.files) == set(rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")
