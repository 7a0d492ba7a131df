"""The UML supervised fine-tune loop on the fused HIP step.

Mirror of the hot path of the reference's ``vision_language/finetune.py``:
``fetch_next`` (:33-39), ``train`` (:120-288), ``validate`` (:291-315) -- same
signatures, step order, loss weighting, evaluation cadence, early stopping,
best-snapshot restore and returned dict -- with the per-step body
(:180-195: forward, 2x cross-entropy, backward, optimizer.step) executed by
``HeadEngine.train_step`` (one launch sequence, logits never leave registers,
no host synchronisation inside a step).

What the reference does per step only for logging (two extra backward passes for
per-modality gradient statistics :190-191,200-206, a second backbone forward :183)
is not on this path.

``capture_features_during_training=True`` (:127-155, 208-233, 280-287) runs ``feature_capture.FeatureCapture`` after
every step, on the per-step path.  One deviation: the reference draws its image sample as a seed-1 16-shot split of the raw
dataset through an image loader (``get_few_shot_image_samples``); raw images are outside this build, so
``take_capture_samples`` takes the first 16 rows of each class of the image table instead, or the caller passes
``capture_samples``.
"""
from __future__ import annotations

import os
import sys
import threading
from types import SimpleNamespace
from typing import Optional

import torch

import umlh
from engine.datasets.utils import FeatureLoader, FeatureTable, TextTensorDataset  # noqa: F401
from engine.models.head import UML, UMLClip  # noqa: F401
from engine.optimizer.default import HYPER_DICT  # noqa: F401
from engine.optimizer.optim import build_optimizer  # noqa: F401
from engine.optimizer.scheduler import build_lr_scheduler  # noqa: F401
from feature_capture import FeatureCapture
from metrics import AlignmentMetrics, cka, mknn  # noqa: F401  finetune.py:111-118 (CKA and mKNN metrics)

EVAL_FREQ = 100   # evaluate on the val set every 100 iterations (early stopping)


def fetch_next(loader, loader_iter):
    """next(loader_iter), restarting the loader when it is exhausted: each modality
    cycles independently of the other (that is the 'unpaired' pairing)."""
    try:
        batch = next(loader_iter)
    except StopIteration:
        loader_iter = iter(loader)
        batch = next(loader_iter)
    return batch, loader_iter


def get_n_text_features(text_loader, n):
    """The first ``n`` rows the text loader delivers, with their labels (finetune.py:96-108).  It iterates the loader, so it
    consumes the loader's RNG draws exactly as the reference does; ``train`` calls it before the training iterators are made."""
    text_samples, text_labels = [], []
    for i, batch in enumerate(text_loader):
        if (i + 1) * text_loader.batch_size >= n:
            text_samples.append(batch[0][:n - i * text_loader.batch_size])
            text_labels.append(batch[1][:n - i * text_loader.batch_size])
            break
        text_features, labels, _ = batch
        text_samples.append(text_features)
        text_labels.append(labels)
    return torch.cat(text_samples, dim=0), torch.cat(text_labels, dim=0)


def take_capture_samples(image_loader, shot=16):
    """(rows, labels) of the first ``shot`` rows of each class of the image loader's table, in table order: this build's
    stand-in for the reference's ``get_few_shot_image_samples(args, shot=16)`` (finetune.py:79-94, a seed-1 few-shot split
    of the raw dataset, which is outside this path).  One host read of the labels; runs once per run."""
    table = getattr(image_loader, "table", None)
    if table is None:
        raise umlh.UmlhError("take_capture_samples needs a FeatureLoader (a device-resident table); pass capture_samples to train()")
    y = table.labels.cpu()
    by_class = torch.argsort(y, stable=True)
    ys = y[by_class]
    first = torch.searchsorted(ys, ys, right=False)                  # position of each class's first row in the sorted order
    keep = by_class[torch.arange(ys.numel()) - first < shot].sort().values.to(table.device)
    return table.features[keep], table.labels[keep]


class _RowSource:
    """Adapts a loader to the fused step.  A ``FeatureLoader`` is consumed as index
    vectors into its device-resident table; any other iterable (e.g. a torch
    DataLoader yielding the reference's dict / tuple batches) is consumed as dense
    batches moved to ``device``."""

    def __init__(self, loader, device, kind, precision="fp32"):
        self.loader, self.device, self.kind, self.precision = loader, device, kind, precision
        self.indexed = hasattr(loader, "iter_index")
        self._make_iter = loader.iter_index if self.indexed else loader.__iter__
        self.it = self._make_iter()

    @property
    def capacity(self):
        return int(getattr(self.loader, "batch_size", None) or 4096)

    def next_index(self):
        idx, self.it = fetch_next(_Reiter(self._make_iter), self.it)
        return idx

    def next_span(self):
        """``next_index()`` for the blockwise loop: the same batch (same RNG draws, same restart at the end of an epoch) as a
        ``umlh.IndexSpan`` where the iterator can say it that way, so that no index tensor is made for it."""
        if not hasattr(self.it, "next_span"):
            return self.next_index()
        try:
            return self.it.next_span()
        except StopIteration:
            self.it = self._make_iter()
            return self.it.next_span()

    def remaining(self):
        return self.it.remaining() if self.indexed and hasattr(self.it, "remaining") else 0

    def take_span(self, k):
        return self.it.take_span(k)

    def table(self, precision):
        t = self.loader.table
        return (t.features, t.labels, t.features_bf16()) if precision == "bf16" else (t.features, t.labels)

    def save(self):
        """Position of the batch stream (iterator, epoch order, offset): ``restore`` rewinds to it."""
        it = self.it
        return it, getattr(it, "epoch", None), getattr(it, "pos", None)      # (the epoch's description: nothing is materialised)

    def restore(self, st):
        self.it = st[0]
        if st[2] is not None:
            self.it.epoch, self.it.pos = st[1], st[2]

    def next(self) -> umlh.RowBatch:
        batch, self.it = fetch_next(_Reiter(self._make_iter), self.it)
        if self.indexed:
            t = self.loader.table
            return umlh.RowBatch(t.features, t.labels, batch,
                                 feats_bf16=t.features_bf16() if self.precision == "bf16" else None)
        if self.kind == "image":
            x, y = batch["img"], batch["label"]
        else:
            x, y = batch[0], batch[1]
        return umlh.RowBatch(x.to(self.device, torch.float32).contiguous(), y.to(self.device, torch.int64).contiguous())


class _Reiter:
    def __init__(self, make):
        self.make = make

    def __iter__(self):
        return self.make()


def _rows(rb):
    return rb.feats if rb.index is None else umlh.gather_rows(rb.feats, rb.index)


def feature_direction_sim(model, img_rows, txt_rows):
    """cos(mean image feature after extract_features, mean text feature) of one step's batches
    (finetune.py:182-183,239); 0 without text.  Row gather, projection and the column sums run on the HIP ops;
    the final ratio is formed on the host from the two d-vectors."""
    if img_rows is None or txt_rows is None:
        return 0.0
    n_of = lambda rb: rb.feats.shape[0] if rb.index is None else rb.index.numel()
    with torch.no_grad():
        fi = umlh.column_sums(model.extract_features(_rows(img_rows)).contiguous()).double().cpu() / n_of(img_rows)
        ft = umlh.column_sums(_rows(txt_rows)).double().cpu() / n_of(txt_rows)
    den = float(fi.norm() * ft.norm())
    return float(fi @ ft) / den if den > 0 else float("nan")


def _state_dict_snapshot(model):
    """Best-model snapshot (finetune.py:249) kept ON THE DEVICE: an asynchronous clone instead of a device-to-host copy
    and a host sync at every evaluation point; it is moved to the CPU once, when train() returns it."""
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _to_cpu(sd):
    return {k: v.cpu() for k, v in sd.items()}


def _check_micro(engine, scalars=None, where=""):
    """Evaluation-point health check.  A bounded in-launch wait that gave up (micro-step kernel, one-launch step) raises
    UmlhError -- the device-side status words are read on every call, not only when the scalars look wrong.  Non-finite step
    scalars with a clean status are a diverged run: the reference prints 'nan' and trains on (finetune.py:236-244; its
    val_acc comparisons then keep the old best and patience ends the run), so this only says so loudly."""
    engine.check_status()
    if scalars is not None and not bool(torch.isfinite(scalars).all()):
        print(f"=> WARNING: non-finite step scalars{where}: the run has diverged (device status clean); continuing as the "
              "reference does", file=sys.stderr)


def _block_end(i, max_iters, eval_freq):
    """Last iteration of the block that starts at ``i``: the next evaluation point (or the final iteration)."""
    return i if i % eval_freq == 0 else min(max_iters - 1, (i // eval_freq + 1) * eval_freq)


def _draw_block(img_src, txt_src, n):
    """Index batches of the next ``n`` steps of both loaders.  Consecutive batches inside both loaders' current epochs are
    taken as ONE span each; a step at which a loader starts an epoch goes through next_span() -- image then
    text, the reference's draw order (finetune.py:164-174) -- so the RNG protocol is untouched.  The entries are
    ``umlh.IndexSpan`` s (positions of an epoch order, not ids): ``HeadEngine.prepare_steps`` writes the ids of both
    modalities with one launch, and no epoch permutation is materialised for the block."""
    bi = [] if img_src is not None else None
    bt = [] if txt_src is not None else None
    k = 0
    while k < n:
        span = min([n - k] + [src.remaining() for src in (img_src, txt_src) if src is not None])
        if span == 0:
            if img_src is not None:
                bi.append(img_src.next_span())
            if txt_src is not None:
                bt.append(txt_src.next_span())
            k += 1
        else:
            if img_src is not None:
                bi.append(img_src.take_span(span))
            if txt_src is not None:
                bt.append(txt_src.take_span(span))
            k += span
    return bi, bt


def _rewind_point(img_src, txt_src, optimizer, scheduler):
    """Everything a training block advances besides the weights, captured before the block is drawn: loader positions, the
    RNG streams the loaders draw their epoch seeds from, optimizer moments and counters, the scheduler's epoch."""
    gens = []
    for src in (img_src, txt_src):
        g = getattr(src.loader, "generator", None) if src is not None else None
        if src is not None and all(g is not q for q, _ in gens):
            gens.append((g, g.get_state() if g is not None else torch.get_rng_state()))
    moments = [(t, t.clone()) for st in optimizer.state.values() for t in st.values() if torch.is_tensor(t)]
    return {"src": [(src, src.save()) for src in (img_src, txt_src) if src is not None], "gens": gens, "moments": moments,
            "step_count": optimizer.step_count, "epoch": scheduler.last_epoch}


def _rewind(r, optimizer, scheduler):
    for src, st in r["src"]:
        src.restore(st)
    for g, st in r["gens"]:
        g.set_state(st) if g is not None else torch.set_rng_state(st)
    for t, old in r["moments"]:
        t.copy_(old)
    optimizer.step_count = r["step_count"]
    scheduler.step(r["epoch"])


class _Run:
    """One head's training state, driven by ``train`` (alone) and ``train_grouped`` (many in lockstep): position, the
    per-step scalars, the best evaluation so far and the patience counter.

    Evaluation results may be read one block LATE: the evaluation and its device-to-host copy are enqueued, then the next
    training block, and only then does the host wait for the copy -- the GPU goes from the evaluation straight into the
    next block instead of idling while the host reads, decides and prepares.  If the late result says "early stop",
    everything the extra block advanced is rewound to the evaluation point (loader positions and RNG streams, optimizer /
    scheduler counters and moments; the weights are replaced by the best snapshot anyway), so every object is left exactly
    as the reference's loop would leave it (finetune.py:247-271)."""

    def __init__(self, *, max_iters, patience, alpha=1.0, precision="fp32", model=None, val_loader=None, test_loader=None,
                 optimizer=None, scheduler=None, img_src=None, txt_src=None, engine=None, scalars=None, name=None):
        self.max_iters, self.patience, self.alpha, self.precision, self.name = max_iters, patience, alpha, precision, name
        self.model, self.val_loader, self.test_loader = model, val_loader, test_loader
        self.optimizer, self.scheduler = optimizer, scheduler
        self.img_src, self.txt_src, self.engine, self.scalars = img_src, txt_src, engine, scalars
        self.out = {"iter": None, "val_acc": None, "model": None, "val_classwise": None, "val_loss": None,
                    "model_records": []}
        self.i, self.last_i = 0, -1     # iteration being run / last iteration that counts
        self.live = max_iters > 0       # False once the head has stopped early or run all its iterations
        self.no_improve = 0
        self.snap = None                # device snapshot of the evaluation that has not been settled yet
        self.back = None                # rewind point of the block drawn since that evaluation began

    @classmethod
    def of(cls, model, image_loader, text_loader, val_loader, test_loader, optimizer, scheduler, max_iters, alpha, patience,
           precision, diagnostics, name=None):
        """The state of a run of ``train`` with these arguments, with its row sources, engine and scalar buffer."""
        model.train()
        assert image_loader is not None or text_loader is not None, "At least one of the loaders should be provided"
        dev = model.head.weight.device
        img_src = _RowSource(image_loader, dev, "image", precision) if image_loader is not None else None
        txt_src = _RowSource(text_loader, dev, "text", precision) if text_loader is not None else None
        engine = model.fused_engine(optimizer, max_rows_img=img_src.capacity if img_src else 32,
                                    max_rows_txt=txt_src.capacity if txt_src else 32, precision=precision)
        # (heads with bias: the engine restricts the diagnostics to the weight columns of the packed [weight | bias | padding]
        # rows -- the reference's are over head.weight only, finetune.py:190-191)
        engine.enable_diagnostics(diagnostics)
        return cls(max_iters=max_iters, patience=patience, alpha=alpha, precision=precision, model=model,
                   val_loader=val_loader, test_loader=test_loader, optimizer=optimizer, scheduler=scheduler,
                   img_src=img_src, txt_src=txt_src, engine=engine, name=name,
                   scalars=torch.zeros(max_iters, umlh.N_SCALARS, dtype=torch.float32, device=dev))

    @property
    def indexed(self):
        return all(src is None or src.indexed for src in (self.img_src, self.txt_src))

    def next_block(self, eval_freq, rewindable=False):
        """Draw all steps up to and including the next evaluation point (or the final iteration) and advance the optimizer's
        step count, the scheduler and ``i`` past them; returns (n, the keyword arguments of ``HeadEngine.train_steps``).
        ``rewindable``: an evaluation is still unread -- take the rewind point ``settle`` needs if it turns out a stop."""
        self.back = _rewind_point(self.img_src, self.txt_src, self.optimizer, self.scheduler) if rewindable else None
        i_end = _block_end(self.i, self.max_iters, eval_freq)
        n = i_end - self.i + 1
        bi, bt = _draw_block(self.img_src, self.txt_src, n)
        opt, sch, img, txt = self.optimizer, self.scheduler, self.img_src, self.txt_src
        kw = dict(img_table=img.table(self.precision) if img else None, img_index_batches=bi,
                  txt_table=txt.table(self.precision) if txt else None, txt_index_batches=bt, lrs=sch.lr_table(n),
                  first_step=opt.step_count + 1, alpha=self.alpha, img_alpha=1.0, scalars_out=self.scalars[self.i:self.i + n])
        opt.step_count += n
        sch.step(sch.last_epoch + n)
        self.i = self.last_i = i_end
        return n, kw

    def advance(self):
        self.i += 1
        self.live = self.live and self.i < self.max_iters

    def begin_eval(self):
        """Evaluation at iteration ``i``: keeps the device snapshot a new best would need and returns the (model, loader)
        pairs and the step's scalar row for ``validate_many_begin`` (the caller puts the model in eval mode around it)."""
        self.snap = _state_dict_snapshot(self.model)          # device-side clone; moved to the CPU by finish()
        self.back = None
        pairs = [(self.model, self.val_loader)] + ([(self.model, self.test_loader)] if self.test_loader is not None else [])
        return pairs, self.scalars[self.i]

    def settle(self, i_eval, val_loss, val_acc):
        """Bookkeeping of the evaluation begun at iteration ``i_eval``: strict-improvement best, patience.  True = the head
        stops at ``i_eval``; a block drawn since the evaluation began is taken back."""
        snap, self.snap = self.snap, None
        if self.out["val_acc"] is None or val_acc > self.out["val_acc"]:
            self.out.update(iter=i_eval, val_acc=val_acc, val_loss=val_loss, model=snap)
            self.no_improve = 0
        else:
            self.no_improve += 1
        if self.no_improve < self.patience:
            return False
        if self.back is not None:
            _rewind(self.back, self.optimizer, self.scheduler)
        self.live = False
        self.i = self.last_i = i_eval
        return True

    def finish(self):
        """Status check, best weights back into the model; the returned dict holds them (on the CPU) and the per-step
        losses / accuracies (``train_scalars``, an extension)."""
        _check_micro(self.engine)
        self.model.load_state_dict(self.out["model"])
        self.out["model"] = _to_cpu(self.out["model"])
        self.out["train_scalars"] = self.scalars[:self.last_i + 1].cpu()
        return self.out


def train(model, image_loader, text_loader, val_loader, test_loader, optimizer, scheduler, device="cuda",
          max_iters=1000, alpha=1.0, eval_freq=EVAL_FREQ, patience=5, capture_features_during_training=False,
          features_pth="./", args=None, logger=None, precision="fp32", diagnostics=None, capture_samples=None,
          capture_options=None, classwise=False):
    """``capture_samples``: the (rows, labels) of the image sample of the feature capture (default:
    ``take_capture_samples(image_loader, 16)``); ``capture_options``: keyword arguments of ``FeatureCapture``
    (``keep_features``, ``strict``).  Both are read only with ``capture_features_during_training``.

    ``classwise``: True, or a dict of keyword arguments of ``validate_classwise`` (``topk``, ``confusion``), fills
    ``out['val_classwise']`` with the class-wise report of the model the run returns: ONCE, after the best weights are back in
    the model, next to the closing ``validate``.  Nothing is added to the loop or its evaluation points; off (the default)
    the slot stays None as in the reference."""
    capture = None
    if capture_features_during_training:
        # finetune.py:127-155: the samples are drawn BEFORE the training iterators exist (the text sample iterates the text
        # loader once, which consumes its RNG draws); the raw features are saved right away
        print(f"=> Ready to save captured features during training at {features_pth}")
        n_class = args.nclasses if args is not None else model.head.weight.shape[0]
        rows, labels = capture_samples if capture_samples is not None else take_capture_samples(image_loader, shot=16)
        text_rows, text_labels = get_n_text_features(text_loader, n=1000) if text_loader is not None else (None, None)
        capture = FeatureCapture(model, rows, labels, text_rows, n_class, text_labels=text_labels, **(capture_options or {}))
        capture.save_raw(features_pth)
    # per-step gradient diagnostics (finetune.py:190-191,203-206): the reference computes them on every
    # step; here they cost ~2.5 us per step, so they are on when a logger asks for them (or on request)
    want_diag = bool(diagnostics) if diagnostics is not None else logger is not None
    run = _Run.of(model, image_loader, text_loader, val_loader, test_loader, optimizer, scheduler, max_iters, alpha,
                  patience, precision, want_diag)
    img_src, txt_src, engine, scalars = run.img_src, run.txt_src, run.engine, run.scalars
    blockwise = logger is None and run.indexed and capture is None
    captured = torch.zeros(max_iters, 3, dtype=torch.float64, device=scalars.device) if capture is not None else None

    def eval_end(i, handle):
        """Reads the evaluation begun at iteration i, settles it and reports as the reference does; True = stop training."""
        res, (s,) = validate_many_end(handle)
        val_loss, val_acc = res[0]
        stop = run.settle(i, val_loss, val_acc)
        if logger is not None:
            logger.log({"val/val_loss": val_loss, "val/val_acc": val_acc, "iter": i})
        _check_micro(engine, s, f" at iter {i}")
        testlog = f" | Test Acc: {res[1][1]:.4f}" if test_loader is not None else ""
        print(f"Iter {i} | Img Loss: {s[umlh.S_LOSS_IMG]:.4f} | Text Loss: {s[umlh.S_LOSS_TXT]:.4f} | "
              f"Img Acc: {s[umlh.S_ACC_IMG]:.4f} | Text Acc: {s[umlh.S_ACC_TXT]:.4f} | Val Loss: {val_loss:.4f} | "
              f"Val Acc {val_acc:.4f}{testlog} | Count {run.no_improve}/{patience}")
        if stop:
            print(f"=> Early stopping at Iter {i}")
        return stop

    pending = None            # (iteration, handle) of the evaluation whose results have not been read yet (blockwise runs only)
    while run.live:
        if blockwise:
            # all steps up to and including the next evaluation point in ONE C call:
            # no Python, no host sync between steps
            n, kw = run.next_block(eval_freq, rewindable=pending is not None)
            engine.train_steps(**kw)
            if pending is not None:
                p, pending = pending, None
                if eval_end(*p):                              # the block just enqueued ran past an early stop: taken back
                    break
        else:
            img_rows = img_src.next() if img_src is not None else None
            txt_rows = txt_src.next() if txt_src is not None else None
            if logger is not None:                   # with the pre-update projection, as the reference (:182-183)
                feat_sim = feature_direction_sim(model, img_rows, txt_rows)
            engine.train_step(img_rows, txt_rows, lr=optimizer.param_groups[0]["lr"], step=optimizer.step_count + 1,
                              alpha=alpha, img_alpha=1.0, scalars_out=scalars[run.i])
            optimizer.step_count += 1
            scheduler.step()
            run.last_i = run.i
        i = run.i
        if capture is not None:                       # after the update of step i (finetune.py:194 is followed by :209)
            torch.stack(capture.step(), out=captured[i])
        if logger is not None:
            if capture is None:
                s = scalars[i].cpu()                  # host sync: only when a logger asks for per-step values
            else:                                     # the capture's three scalars ride on the same read
                s = torch.cat([scalars[i].double(), captured[i]]).cpu()
                cap, s = s[umlh.N_SCALARS:], s[:umlh.N_SCALARS].float()
            gd = umlh.grad_diagnostics(s, model.head.weight.numel(), 0 if img_src is None else 1, 0 if txt_src is None else 1)
            row = {"train/image_loss": float(s[umlh.S_LOSS_IMG]), "train/text_loss": float(s[umlh.S_LOSS_TXT]),
                   "train/image_acc": float(s[umlh.S_ACC_IMG]), "train/text_acc": float(s[umlh.S_ACC_TXT]),
                   "train/lr": scheduler.get_last_lr()[0],
                   "train/grad_direction_sim": gd["grad_direction_sim"], "train/img_grad_norm": gd["img_grad_norm"],
                   "train/txt_grad_norm": gd["txt_grad_norm"], "train/grad_agreement_rate": gd["grad_agreement_rate"],
                   "train/feature_direction_sim": feat_sim}
            if capture is not None:                   # finetune.py:241-243
                row.update({"train/cka_score": float(cap[1]), "train/mknn_score": float(cap[2]),
                            "train/inclass_distance": float(cap[0])})
            logger.log(row)
        if i % eval_freq == 0:
            pairs, row = run.begin_eval()
            model.eval()
            p = (i, validate_many_begin(pairs, extra=[row]))
            model.train()
            if blockwise and i + 1 < max_iters:
                pending = p                                   # read after the next block has been enqueued
            elif eval_end(*p):
                break
        run.advance()
    out = run.finish()
    val_loss, val_acc = validate(model, val_loader, device=device)
    if logger is not None:
        logger.log({"val/best_val_loss": val_loss, "val/best_val_acc": val_acc, "iter": out["iter"]})
    print(f"=> Best Val Loss {val_loss:.4f}, Val Acc {val_acc:.4f} at Iter {out['iter']}")
    cw = _classwise_kwargs(classwise)
    if cw is not None:
        out["val_classwise"] = validate_classwise(model, val_loader, **cw)
    if capture is not None:                           # finetune.py:280-287
        capture.save(features_pth)
        out["capture_scalars"] = captured[:run.last_i + 1].cpu()     # (an extension, like train_scalars): per step
                                                                      # {inclass_distance, cka_score, mknn_score}
    return out


def train_grouped(runs, device="cuda", eval_freq=EVAL_FREQ, precision="fp32"):
    """``train`` for MANY independent heads in lockstep: the grid points of a sweep (finetune.py:406-448) share the
    feature tables and differ in hyper-parameters, seeds and batch orders.  Between two evaluation points all live heads
    advance inside the same grouped persistent launches (``umlh_train_steps_grouped``); at an evaluation point every
    head's validation / test passes are enqueued and read back with one host synchronisation.  Each head keeps the
    exact semantics of ``train`` (evaluation cadence, strict-improvement best snapshot, patience, restored weights,
    returned dict); ``runs`` = dicts with the arguments of ``train`` (model, image_loader, text_loader, val_loader,
    test_loader, optimizer, scheduler, max_iters, alpha, patience, and optionally ``classwise``: that run's
    ``out['val_classwise']`` is filled after its best weights are back, as in ``train``)."""
    st = [_Run.of(r["model"], r.get("image_loader"), r.get("text_loader"), r["val_loader"], r.get("test_loader"),
                  r["optimizer"], r["scheduler"], r["max_iters"], r["alpha"], r["patience"], precision, False,
                  name=r.get("name", k)) for k, r in enumerate(runs)]
    if not all(h.indexed for h in st):
        raise umlh.UmlhError("train_grouped needs FeatureLoader inputs (device-resident tables)")
    # Evaluation results are read one round LATE, as in train(): a round enqueues the next block of every live head first and
    # only then waits for the previous round's evaluation copy.  Needs private loader generators (a generator shared between
    # heads cannot be rewound for one of them): otherwise every round reads its own evaluation before the next block is drawn.
    pipelined = all(src is None or getattr(src.loader, "generator", None) is not None
                    for h in st for src in (h.img_src, h.txt_src))

    def settle(due, at, handle):
        """Reads the evaluations `handle` holds (head due[k] evaluated at iteration at[k]) and settles each head's."""
        res, ex = validate_many_end(handle)
        k = 0
        for h, i_eval, s in zip(due, at, ex):
            if not bool(torch.isfinite(s).all()):                   # (status words are read for every head when the sweep ends)
                _check_micro(h.engine, s, f" at iter {i_eval} of grid point {h.name}")
            h.settle(i_eval, *res[k])
            k += 2 if h.test_loader is not None else 1

    pending = None                      # (due heads, their evaluation iterations, validate_many_begin handle)
    while any(h.live for h in st) or pending is not None:
        # ---- one block per live head: all steps up to and including its next evaluation point ----
        by_n = {}
        awaited = {id(h) for h in pending[0]} if pending is not None else set()
        for h in st:
            if h.live:
                n, kw = h.next_block(eval_freq, rewindable=id(h) in awaited)
                by_n.setdefault(n, []).append(dict(kw, engine=h.engine))
        for n, jobs in by_n.items():
            umlh.train_steps_grouped(jobs, n)
        # ---- the previous round's evaluations (the blocks above are already running) ----
        if pending is not None:
            p, pending = pending, None
            settle(*p)
        # ---- evaluation points (every live head sits on one, or on its final iteration) ----
        due = [h for h in st if h.live and h.i % eval_freq == 0]
        if due:
            pairs, extra = [], []
            for h in due:
                head_pairs, row = h.begin_eval()
                h.model.eval()
                pairs += head_pairs
                extra.append(row)
            handle = validate_many_begin(pairs, extra=extra)
            for h in due:
                h.model.train()
            pending = (due, [h.i for h in due], handle)
            if not pipelined:                                       # shared generators: decide before the next block is drawn
                p, pending = pending, None
                settle(*p)
        for h in st:
            if h.live:
                h.advance()
    outs = [h.finish() for h in st]
    for r, h, out in zip(runs, st, outs):
        cw = _classwise_kwargs(r.get("classwise"))
        if cw is not None:
            out["val_classwise"] = validate_classwise(h.model, h.val_loader, **cw)
    return outs


EVAL_SLAB = 4096     # rows per forward launch of a whole-table evaluation


def _slab_evaluable(loader):
    return hasattr(loader, "iter_index") and not loader.shuffle and not loader.drop_last and len(loader.table) > 0


def _eval_enqueue(model, val_loader):
    """Enqueue the whole-table evaluation of an unshuffled ``FeatureLoader`` (one ``umlh_eval_rows`` launch per
    4096-row slab) and return the device tensor of per-row {CE, correct} -- no host synchronisation."""
    dev = model.head.weight.device
    val_loader.iter_index()                       # iter(loader): the iterator's base seed is drawn as in the reference
    t = val_loader.table
    n = len(t)
    stats = torch.empty(n, 2, dtype=torch.float32, device=dev)
    engine = model._infer_engine(min(n, EVAL_SLAB))
    for s0 in range(0, n, EVAL_SLAB):
        m = min(EVAL_SLAB, n - s0)
        engine.eval_rows(umlh.RowBatch(t.features[s0:s0 + m], t.labels[s0:s0 + m]), stats[s0:s0 + m])
    return stats


def _eval_finish(stats_cpu, bs):
    """(val_loss, val_acc) from per-row stats: mean over batches of the per-batch mean CE, global mean of correct."""
    st = stats_cpu.double().numpy()
    n = st.shape[0]
    nb = (n + bs - 1) // bs
    import numpy as np
    sums = np.add.reduceat(st[:, 0], np.arange(0, n, bs))           # per-batch CE sums, in row order
    counts = np.full(nb, bs, dtype=np.float64)
    counts[-1] = n - (nb - 1) * bs
    return float((sums / counts).sum() / nb), float(st[:, 1].sum() / n)


_PINNED = threading.local()   # per thread (sweep_farm runs train() on worker threads): ring of pinned host buffers for the
                              # evaluation read-backs (hipHostMalloc per call would cost more than the copy)


def _pinned(n):
    ring = getattr(_PINNED, "ring", None)
    if ring is None:
        ring = _PINNED.ring = []
    for k, buf in enumerate(ring):
        if buf.numel() >= n:
            ring.append(ring.pop(k))                       # least recently handed out first
            return ring[-1][:n]
    if len(ring) >= 4:
        ring.pop(0)
    ring.append(torch.empty(max(n, 1 << 16), dtype=torch.float32, pin_memory=True))
    return ring[-1][:n]


def validate_many_begin(pairs, extra=None):
    """First half of ``validate_many``: enqueue every evaluation and ONE asynchronous device-to-host copy of all per-row
    statistics (+ ``extra``) into pinned memory; returns a handle for ``validate_many_end``.  Nothing waits for the GPU:
    the caller can enqueue the next training block before it looks at the results."""
    extra = list(extra or [])
    if not all(_slab_evaluable(ld) for _, ld in pairs):
        return {"done": ([validate(m, ld) for m, ld in pairs], [e.cpu() for e in extra])}
    stats = [_eval_enqueue(m, ld) for m, ld in pairs]
    dev_flat = torch.cat([st.reshape(-1) for st in stats] + [e.reshape(-1).to(torch.float32) for e in extra])
    host = _pinned(dev_flat.numel())
    host.copy_(dev_flat, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev_flat.device))
    return {"host": host, "event": ev, "keep": dev_flat, "pairs": pairs, "sizes": [st.numel() for st in stats], "extra": extra}


def validate_many_end(h):
    """(results, extras on the CPU) of a ``validate_many_begin`` handle; waits for its copy only."""
    if "done" in h:
        return h["done"]
    h["event"].synchronize()
    flat = h["host"].clone()                               # the pinned buffer goes back to the ring
    out, pos = [], 0
    for (m, ld), n in zip(h["pairs"], h["sizes"]):
        out.append(_eval_finish(flat[pos:pos + n].reshape(-1, 2), ld.batch_size))
        pos += n
    ex = []
    for e in h["extra"]:
        ex.append(flat[pos:pos + e.numel()].reshape(e.shape))
        pos += e.numel()
    return out, ex


def validate_many(pairs, extra=None):
    """``validate`` for several (model, loader) pairs with ONE host synchronisation: every evaluation is enqueued
    first (``_eval_enqueue``), then all per-row statistics come back in a single device-to-host copy.  Used at the
    evaluation points of ``train`` (val + test) and of the grouped sweep (every head's val + test).  ``extra``: device
    float tensors (e.g. the step's scalar rows) that ride on the same copy; returns (results, extras on the CPU)."""
    return validate_many_end(validate_many_begin(pairs, extra))


def validate(model, val_loader, device="cuda"):
    """val_acc = mean over all rows of (argmax == label); val_loss = mean over batches
    of the per-batch mean CE (not sample weighted) -- finetune.py:291-315.  One host read at the end.

    An unshuffled ``FeatureLoader`` is evaluated as whole 4096-row slabs of its device table
    (``umlh_eval_rows`` keeps the per-row CE / correct flag, the per-batch means are formed from them), i.e. one
    launch per slab instead of one per batch: at the reference's batch size of 32 a validation pass over
    Caltech101's val + test rows is 1 + 1 launches instead of 13 + 78."""
    dev = model.head.weight.device
    model.eval()
    src_indexed = hasattr(val_loader, "iter_index")
    if _slab_evaluable(val_loader):
        out = _eval_finish(_eval_enqueue(model, val_loader).cpu(), val_loader.batch_size)
        model.train()
        return out
    rows, slots = [], []
    it = val_loader.iter_index() if src_indexed else iter(val_loader)
    engine = None
    for batch in it:
        if src_indexed:
            t = val_loader.table
            rb = umlh.RowBatch(t.features, t.labels, batch)
        else:
            rb = umlh.RowBatch(batch["img"].to(dev, torch.float32).contiguous(),
                               batch["label"].to(dev, torch.int64).contiguous())
        n = rb.n_rows()
        if engine is None or engine.cfg.max_rows_img < n:
            engine = model._infer_engine(n)
        slot = torch.zeros(umlh.N_SCALARS, dtype=torch.float32, device=dev)
        engine.eval_batch(rb, slot)
        rows.append(n)
        slots.append(slot)
    s = torch.stack(slots).cpu()
    counts = torch.tensor(rows, dtype=torch.float32)
    val_acc = (s[:, umlh.S_CORRECT].sum() / counts.sum()).item()
    val_loss = (s[:, umlh.S_LOSS_SUM] / counts).mean().item()
    model.train()
    return val_loss, val_acc


def validate_classwise(model, val_loader, topk=5, confusion=False):
    """The class-wise report of ``model`` on ``val_loader`` (what ``train(classwise=...)`` puts into ``out['val_classwise']``,
    the slot the reference creates and never fills): a dict of CPU values --

      ``support``, ``correct``, ``correct_topk``   int64 [C]: rows of each true class, and how many of them have the label as
                                                   the best class / among the ``topk`` best classes
      ``acc``, ``acc_topk``                        float64 [C]: the two ratios, NaN for a class without rows
      ``mean_class_acc``, ``mean_class_acc_topk``  their means over the classes that have rows (mean per-class accuracy)
      ``top1_acc``, ``topk_acc``                   correct / rows, over the rows with a label in [0, C)
      ``topk``, ``n`` (all rows), ``ignored`` (rows with a label outside [0, C), counted nowhere else), ``no_prediction``
                                                   (rows with NaN features: counted in ``support`` and ``n``, never correct)
      ``confusion``                                int64 [C, C] when asked for: row = true class, column = best class

    The best classes come from ``model.predict_topk`` (``umlh.topk_classes``: the [rows, C] logits are never formed, ties go to
    the smaller class index) and are counted by ``umlh.class_report``.  An unshuffled ``FeatureLoader`` is evaluated as
    ``EVAL_SLAB``-row slabs of its device table, any other loader batch by batch; all of them add into one set of device
    counters and there is ONE host read at the end.  The slab path makes no iterator, so it draws nothing from the loader's
    RNG.  ``topk`` is clamped to the number of classes and to the kernels' 24.

    ``top1_acc`` and ``validate``'s accuracy come from different arithmetic: the fp64 re-evaluation of the candidates here,
    the fp32 forward kernel's argmax there.  They agree except on rows whose two best logits lie within fp32 rounding of each
    other, where either class may win there (and an exact tie goes to the smaller index here)."""
    dev = model.head.weight.device
    n_class = model.head.weight.shape[0]
    k = max(1, min(int(topk), n_class, umlh.report.MAX_K))
    model.eval()
    counters, rows = None, 0
    if _slab_evaluable(val_loader):
        t = val_loader.table
        batches = ((t.features[s0:s0 + EVAL_SLAB], t.labels[s0:s0 + EVAL_SLAB]) for s0 in range(0, len(t), EVAL_SLAB))
    else:
        batches = ((b["img"].to(dev, torch.float32), b["label"].to(dev)) for b in val_loader)
    for x, y in batches:
        cls, _ = model.predict_topk(x, k=k)
        counters = umlh.class_report(cls, y, n_class, confusion=confusion, out=counters)
        rows += int(y.numel())
    model.train()
    if counters is None:
        raise umlh.UmlhError("validate_classwise: the loader delivered no rows")
    names = ["support", "hit1", "hitk", "misc"] + (["confusion"] if confusion else [])
    flat = torch.cat([counters[nm].reshape(-1) for nm in names]).cpu()                  # the one host read
    support, correct, correct_k = (flat[j * n_class:(j + 1) * n_class].clone() for j in range(3))
    ignored, no_pred = (int(v) for v in flat[3 * n_class:3 * n_class + 2])
    seen = support > 0
    nan = torch.full((n_class,), float("nan"), dtype=torch.float64)
    acc = torch.where(seen, correct.double() / support.double(), nan)
    acc_k = torch.where(seen, correct_k.double() / support.double(), nan)
    labelled = int(support.sum())
    ratio = lambda a: float(a.sum()) / labelled if labelled else float("nan")
    out = {"support": support, "correct": correct, "correct_topk": correct_k, "acc": acc, "acc_topk": acc_k,
           "mean_class_acc": float(acc[seen].mean()) if labelled else float("nan"),
           "mean_class_acc_topk": float(acc_k[seen].mean()) if labelled else float("nan"),
           "top1_acc": ratio(correct), "topk_acc": ratio(correct_k), "topk": k, "n": rows, "ignored": ignored,
           "no_prediction": no_pred}
    if confusion:
        out["confusion"] = flat[3 * n_class + 2:].reshape(n_class, n_class).clone()
    return out


def _classwise_kwargs(classwise):
    """``train``'s ``classwise`` argument as keyword arguments of ``validate_classwise``, or None when it is off."""
    if isinstance(classwise, dict):
        return dict(classwise)
    return {} if classwise else None


def hparam_str(optim, lr, wd, batch_size, iters, dropout, learnable_temp):
    base = f"optim_{optim}-lr_{lr}-wd_{wd}-bs_{batch_size}-iters_{iters}"
    if dropout is not None:
        base += f"-dropout_{dropout}"
    if learnable_temp is True:
        base += "-learnable_temp"
    return base


def feature_tables(img_train, img_val, img_test, text_ds, device):
    """The four device-resident tables of one dataset (uploaded once; a sweep shares them)."""
    return {"train": FeatureTable(*img_train, device), "val": FeatureTable(*img_val, device),
            "test": FeatureTable(*img_test, device),
            "text": FeatureTable(text_ds.input_tensor, text_ds.label_tensor, device, text_ds.eot_indices)}


def wants_zero_shot_init(classifier_init, modality, common_dim, text_indim):
    """reference finetune.py:362-363: the text-derived head only for crossmodal runs, or an image-only run whose
    ``common_dim`` equals the text width; every other unimodal run (default ``common_dim`` = 0, and all text-only
    runs) keeps nn.Linear's random init."""
    return classifier_init == "zeroshot" and (modality == "crossmodal" or
                                              (modality == "image" and int(common_dim or 0) == int(text_indim)))


def _build_model(tables, hparams, num_classes, modality, use_clip, clip_logit, text_indim):
    """The head of one grid point, on the CPU, initialised from the global RNG (reference :343-346)."""
    d_img, d_txt = tables["train"].features.shape[1], tables["text"].features.shape[1]
    if use_clip:
        return UMLClip(d_img, num_classes, logit_scale_init=clip_logit, bias=False, learnable_temp=hparams["learnable_temp"])
    tin = (d_txt if text_indim is None else text_indim) if modality == "crossmodal" else (text_indim or 0)
    return UML(d_img, tin, num_classes, bias=False, learnable_temp=hparams["learnable_temp"])


def _build_run(tables, text_ds, hparams, *, num_classes, modality, classifier_init, use_clip, clip_logit, text_indim,
               device, generator, order_rng, common_dim=None, model=None):
    """One grid point with the reference's wiring (:343-391), as the arguments of ``train``: (model, image_loader,
    text_loader, val_loader, test_loader, optimizer, scheduler); the test loader is always built.  The order -- model,
    ``.to(device)``, zero-shot init, optimizer, scheduler, loaders -- is the order of the RNG draws, which the bit-for-bit
    equality of farm, grouped and isolated runs rests on."""
    if model is None:
        model = _build_model(tables, hparams, num_classes, modality, use_clip, clip_logit, text_indim)
    model.to(device)
    if common_dim is None:
        common_dim = 0 if modality == "crossmodal" else (text_indim or 0)
    if wants_zero_shot_init(classifier_init, modality, common_dim, tables["text"].features.shape[1]):
        model.zero_shot_init(text_ds)
    optimizer = build_optimizer(model.parameters(), hparams["optim"], hparams["lr"], hparams["weight_decay"])
    scheduler = build_lr_scheduler(optimizer, hparams["lr_scheduler"], hparams["warmup_iter"], hparams["max_iter"],
                                   warmup_type=hparams["warmup_type"], warmup_lr=hparams["warmup_min_lr"])
    bs = hparams["batch_size"]
    kw = {"order_rng": order_rng, "generator": generator}
    image_loader = FeatureLoader(tables["train"], bs, shuffle=True, kind="image", **kw) if modality != "text" else None
    text_loader = FeatureLoader(tables["text"], bs, shuffle=True, kind="text", **kw) if modality != "image" else None
    val_loader = FeatureLoader(tables["val"], bs, shuffle=False, kind="image", **kw)
    test_loader = FeatureLoader(tables["test"], bs, shuffle=False, kind="image", **kw)
    return model, image_loader, text_loader, val_loader, test_loader, optimizer, scheduler


def setup_feature_run(img_train, img_val, img_test, text_ds, hparams, *, num_classes, modality="crossmodal",
                      alpha=1.0, classifier_init="zeroshot", use_clip=False, clip_logit=4.60517, text_indim=None,
                      device="cuda:0", eval_test=True, precision="fp32", eval_freq=EVAL_FREQ, tables=None,
                      generator=None, order_rng="torch-cpu", model=None, common_dim=None,
                      capture_features_during_training=False, features_pth="./", capture_samples=None):
    """``setup()`` (finetune.py:323-404) for pre-extracted features: builds the model,
    optimizer, scheduler and the four loaders with the reference's wiring, trains, tests.

    img_* are (features [N,d], labels [N]) pairs; text_ds a TextTensorDataset.  ``tables`` (from
    ``feature_tables``), ``generator`` (private seed source of the loaders) and a pre-built ``model``
    are what the concurrent sweep passes in.  ``text_indim`` is ``args.text_indim`` in crossmodal mode and
    ``args.common_dim`` otherwise (the second argument of ``UML(...)``, reference :343-346); ``common_dim``
    overrides the latter.  ``capture_features_during_training`` (the reference's setup() hard-codes True, :386; off here
    unless asked for), ``features_pth`` and ``capture_samples`` are passed on to ``train``."""
    if tables is None:
        tables = feature_tables(img_train, img_val, img_test, text_ds, device)
    model, image_loader, text_loader, val_loader, test_loader, optimizer, scheduler = _build_run(
        tables, text_ds, hparams, num_classes=num_classes, modality=modality, classifier_init=classifier_init, use_clip=use_clip,
        clip_logit=clip_logit, text_indim=text_indim, common_dim=common_dim, device=device, generator=generator,
        order_rng=order_rng, model=model)
    result = train(model, image_loader, text_loader, val_loader, test_loader if eval_test else None, optimizer,
                   scheduler, device=device, max_iters=hparams["max_iter"], alpha=alpha, eval_freq=eval_freq,
                   patience=hparams["patience"], precision=precision,
                   capture_features_during_training=capture_features_during_training, features_pth=features_pth,
                   args=SimpleNamespace(nclasses=num_classes), capture_samples=capture_samples)
    test_loss, test_acc = validate(model, test_loader, device=device)
    return {"test_acc": test_acc, "test_loss": test_loss, "val_acc": result["val_acc"], "model": result["model"],
            "iter": result["iter"], "train_scalars": result["train_scalars"]}


def linear_probe(img_train, img_val, img_test, *, num_classes, C_grid=(0.01, 0.1, 1.0, 10.0, 100.0), max_iter=200, standardize=False,
                 classwise=False, device="cuda:0", tables=None, warm_start=True):
    """The linear-probe baseline of few-shot papers on pre-extracted features: an L2-regularised multinomial logistic
    regression fitted to its optimum by L-BFGS (``umlh.SoftmaxProbe``), C chosen on the validation split.

    img_* are the (features [N, d], labels [N]) pairs of ``setup_feature_run`` (labels 0 .. num_classes - 1, every class present
    in the train split); ``tables`` (from ``feature_tables``) are used instead where given.  The grid is walked in ascending C,
    each fit started from the previous one's coefficients (``warm_start=False``: every fit from zero); val and test are scored
    for every C and nothing is read back until all fits are enqueued.  The best C has the highest val accuracy, ties to the
    smaller C.  Returns {'best_C', 'val_acc', 'test_acc', 'per_C': [{'C', 'val_acc', 'test_acc'}], 'records': [probe.record()],
    'probe'} and, with ``classwise=True``, 'classwise': ``validate_classwise``'s kind of report (``umlh.report.class_report``)
    of the best probe on the test split."""
    if num_classes < 2:
        raise ValueError(f"linear_probe: num_classes={num_classes} < 2")
    grid = sorted(float(c) for c in C_grid)
    if not grid or grid[0] <= 0:
        raise ValueError(f"linear_probe: C_grid={C_grid} must hold positive values")
    dev = torch.device(device)
    if tables is not None:
        split = {t: (tables[t].features, tables[t].labels) for t in ("train", "val", "test")}
    else:
        split = {"train": img_train, "val": img_val, "test": img_test}
    with torch.cuda.device(dev):
        split = {t: (f.to(device=dev, dtype=torch.float32), torch.as_tensor(l).to(device=dev, dtype=torch.int64)) for t, (f, l) in split.items()}
        probes, counts = [], []
        for c in grid:
            pr = umlh.SoftmaxProbe(C=c, max_iter=max_iter, standardize=standardize)
            pr.fit(*split["train"], coef_init=probes[-1] if (warm_start and probes) else None, check_classes=False, n_classes=num_classes)
            probes.append(pr)
            counts += [pr.correct(*split["val"]), pr.correct(*split["test"])]
        got = torch.stack(counts).cpu().tolist()
        nv, nt = split["val"][0].shape[0], split["test"][0].shape[0]
        per_c = [{"C": c, "val_acc": got[2 * i] / nv, "test_acc": got[2 * i + 1] / nt} for i, c in enumerate(grid)]
        best = max(range(len(grid)), key=lambda i: (per_c[i]["val_acc"], -i))
        out = {"best_C": grid[best], "val_acc": per_c[best]["val_acc"], "test_acc": per_c[best]["test_acc"], "per_C": per_c,
               "records": [p.record() for p in probes], "probe": probes[best]}
        if classwise:
            from umlh.report import class_report, topk_classes
            pr = probes[best]
            cls, _ = topk_classes(split["test"][0], pr.raw_weight_, pr.raw_bias_, k=min(5, num_classes))
            rep = {k: v.cpu() for k, v in class_report(cls, split["test"][1], num_classes).items()}
            rep["top1_acc"] = float(rep["hit1"].sum()) / nt
            rep["topk_acc"] = float(rep["hitk"].sum()) / nt
            out["classwise"] = rep
    return out


# --------------------------------------------------------------------------------------------- #
# sweep / main over feature files  (reference: finetune.py:58-77 naming, :323-448 setup/sweep,
# :451-510 main).  Same flag names on `args`; wandb / Tee logging and raw-image loading are out
# of scope -- images come from the feature files features.py wrote.
# --------------------------------------------------------------------------------------------- #
FLAG = 0   # run despite an existing result file when set to 1 (reference finetune.py:31)


def savedir(outdir, dataset, encoder, train_shot, seed, text_type, text_shots, image_augmentation, mode,
            init_mode="zeroshot", alpha=0.0, text_bs=0, custom_name="", args=None):
    from features import get_few_shot_setup_name
    benchname = "-".join([dataset, get_few_shot_setup_name(train_shot, seed)])
    text_name = f"text_{text_type}" + (f"_n_{text_shots}" if text_shots is not None else "")
    image_name = f"image_{image_augmentation}_{custom_name}"
    mod_name = (f"finetune-{text_name}-{image_name}" if mode == "crossmodal"
                else f"finetune-{image_name}" if mode == "image" else text_name)
    if mode == "crossmodal":
        mod_name = f"{mod_name}-alpha_{alpha}"
    if text_bs > 0:
        mod_name = f"{mod_name}-text_bs_{text_bs}"
    if args is not None and mode != "crossmodal":
        mod_name = f"{mod_name}-common_dim_{getattr(args, 'common_dim', 0)}"
    return os.path.join(outdir, benchname, encoder.replace("/", "-"), mod_name, init_mode)


def _point_args(args):
    """What a grid point's model and loaders take from ``args``, as keywords of ``setup_feature_run`` / ``_build_run``."""
    text_indim = getattr(args, "text_indim", None) if args.modality == "crossmodal" else getattr(args, "common_dim", 0)
    return dict(num_classes=args.nclasses, modality=args.modality, classifier_init=args.classifier_init,
                use_clip=args.use_clip, clip_logit=args.logit, text_indim=text_indim)


def _result_file(savepath, hparams):
    """(path of a grid point's ``test_result.pth`` in its own, newly made directory, the result stored there or None).  An
    existing file is loaded instead of running the point again unless FLAG is set (reference :330-333)."""
    ckpt_dir = os.path.join(savepath, hparam_str(hparams["optim"], hparams["lr"], hparams["weight_decay"], hparams["batch_size"],
                                                 hparams["max_iter"], hparams["dropout"], hparams["learnable_temp"]))
    os.makedirs(ckpt_dir, exist_ok=True)
    test_path = os.path.join(ckpt_dir, "test_result.pth")
    if os.path.exists(test_path) and not FLAG:
        print(f"=> Skipping {ckpt_dir} as it already exists!")
        return test_path, torch.load(test_path, map_location="cpu", weights_only=True)
    return test_path, None


def setup(datasets, hparams, args, capture_features_during_training=False):
    """One hyper-parameter point: build model / optimizer / scheduler / loaders, train, test, save
    ``test_result.pth`` (skipped when it exists and FLAG is 0, reference :330-333).  ``capture_features_during_training``
    (default off; the reference hard-codes True, :386) writes the captured features next to the result file."""
    test_path, done = _result_file(args.savepath, hparams)
    if done is not None:
        return done
    res = setup_feature_run(datasets["img_tr"], datasets["img_val"], datasets["img_te"], datasets["text_ds"], hparams,
                            alpha=args.alpha, device=args.device, eval_test=getattr(args, "eval_test", True),
                            precision=getattr(args, "precision", "fp32"), tables=datasets.get("tables"),
                            capture_features_during_training=capture_features_during_training,
                            features_pth=os.path.dirname(test_path), **_point_args(args))
    test_dict = {"test_acc": res["test_acc"], "val_acc": res["val_acc"], "model": res["model"], "iter": res["iter"]}
    print(f"=> Test Acc: {res['test_acc']:.4f}")
    torch.save(test_dict, test_path)
    return test_dict


def _grid(hyperparams):
    from itertools import product
    grid = {k: (v if isinstance(v, list) else [v]) for k, v in hyperparams.items()}
    keys = list(grid)
    return [dict(zip(keys, combo)) for combo in product(*[grid[k] for k in keys])]


def _report(results, args):
    torch.save(results, os.path.join(args.savepath, "results.pth"))
    best = int(torch.argmax(torch.tensor(results["val_acc"])))
    print(f"=> [FINAL] Best Val Acc: {results['val_acc'][best]:.4f} | Best Test Acc: {results['test_acc'][best]:.4f}")
    print(f"=> [FINAL] Best Hyperparameters: {results['hparams'][best]}")
    return results, results["val_acc"][best], results["test_acc"][best]


def sweep(datasets, hyperparams, args):
    """Cartesian product over the list-valued entries of a HYPER_DICT grid, in key order
    (reference :406-448); returns (results, best_val_acc, best_test_acc).

    ``args.sweep_workers > 1`` runs the grid points concurrently on one GPU (``sweep_farm``)."""
    if getattr(args, "sweep_mode", "") == "grouped":
        return sweep_grouped(datasets, hyperparams, args)
    if int(getattr(args, "sweep_workers", 1) or 1) > 1:
        return sweep_farm(datasets, hyperparams, args, int(args.sweep_workers))
    results = {"test_acc": [], "val_acc": [], "hparams": [], "model_records": []}
    # the four feature tables are uploaded once for the whole sweep (every grid point reads the same rows)
    if "tables" not in datasets and isinstance(datasets.get("img_tr"), (tuple, list)):
        datasets = dict(datasets, tables=feature_tables(datasets["img_tr"], datasets["img_val"], datasets["img_te"],
                                                        datasets["text_ds"], torch.device(getattr(args, "device", "cuda:0"))))
    for idx, hp in enumerate(_grid(hyperparams)):
        print(f"=> Running {idx + 1}: {hp}")
        out = setup(datasets, hp, args)
        results["test_acc"].append(out["test_acc"])
        results["val_acc"].append(out["val_acc"])
        results["hparams"].append(hp)
    return _report(results, args)


def farm_seed(base_seed, idx):
    """Seed of grid point ``idx``'s private generator (loader orders) and of its model init."""
    return (int(base_seed) if base_seed is not None and int(base_seed) >= 0 else 0) * 100003 + 7919 * (idx + 1)


def _sweep_tables(datasets, args):
    """The device tables the points of a grouped or farmed sweep share, with their bf16 shadows in bf16 mode."""
    tables = feature_tables(datasets["img_tr"], datasets["img_val"], datasets["img_te"], datasets["text_ds"],
                            torch.device(args.device))
    if getattr(args, "precision", "fp32") == "bf16":
        for t in tables.values():
            t.features_bf16()
    return tables


def sweep_grouped(datasets, hyperparams, args):
    """The sweep as ONE grouped job (``args.sweep_mode = "grouped"``): every grid point becomes a head of the same
    persistent launches (``train_grouped`` / ``umlh_train_steps_grouped``), all reading the same device-resident
    feature tables -- the [G, C, d] grouped multi-head farm of SURVEY 8(f) rank 2.  Like ``sweep_farm`` every point
    draws its loader orders from a private generator seeded by ``farm_seed(args.seed, k)`` and initialises its model
    under that seed, so a point's result is independent of which other points run beside it: it equals the isolated run
    of that point (``setup_feature_run`` with the same generator) bit for bit."""
    points = _grid(hyperparams)
    dev = torch.device(args.device)
    precision = getattr(args, "precision", "fp32")
    tables = _sweep_tables(datasets, args)
    runs, slots = [], []
    results = [None] * len(points)
    for idx, hp in enumerate(points):
        test_path, results[idx] = _result_file(args.savepath, hp)
        if results[idx] is not None:
            continue
        torch.manual_seed(farm_seed(args.seed, idx))
        gen = torch.Generator()
        gen.manual_seed(farm_seed(args.seed, idx))
        model, image_loader, text_loader, val_loader, test_loader, optimizer, scheduler = _build_run(
            tables, datasets["text_ds"], hp, device=dev, generator=gen,
            order_rng=getattr(args, "order_rng", "torch-cpu"), **_point_args(args))
        runs.append(dict(model=model, image_loader=image_loader, text_loader=text_loader, val_loader=val_loader,
                         test_loader=test_loader if getattr(args, "eval_test", True) else None, optimizer=optimizer,
                         scheduler=scheduler, max_iters=hp["max_iter"], alpha=args.alpha, patience=hp["patience"],
                         final_test_loader=test_loader))
        slots.append((idx, test_path))
    outs = train_grouped(runs, device=dev, precision=precision)
    finals, _ = validate_many([(r["model"], r["final_test_loader"]) for r in runs]) if runs else ([], [])
    for (idx, test_path), out, (test_loss, test_acc) in zip(slots, outs, finals):
        test_dict = {"test_acc": test_acc, "val_acc": out["val_acc"], "model": out["model"], "iter": out["iter"]}
        torch.save(test_dict, test_path)
        results[idx] = test_dict
    res = {"test_acc": [o["test_acc"] for o in results], "val_acc": [o["val_acc"] for o in results],
           "hparams": points, "model_records": []}
    return _report(res, args)


def sweep_farm(datasets, hyperparams, args, workers):
    """The sweep as a farm: the grid points of one dataset are independent head fine-tunes over the
    SAME feature tables (18 AdamW points in ``clip_linear``), each far too small to fill 256 CUs
    (batch 32: a handful of workgroups per kernel).  The tables are uploaded once; every grid point
    gets its own engine, its own HIP stream and a host thread that enqueues whole evaluation
    intervals through ``umlh_train_steps`` (a C loop, no GIL), so the small kernels of different
    points can overlap on the chip.  No collective, no shared mutable state.  Measured on MI355X this
    does not beat the sequential sweep for batch-32 steps -- the dispatch rate of dependent small kernels is the
    limit -- so ``sweep_workers`` defaults to 1; the farm is for grids whose steps are large enough to be GPU-bound
    individually yet too small to fill the chip.

    Unlike the sequential sweep -- where point k's shuffles depend on how much global RNG the
    points before it consumed -- every point draws from a private generator seeded by
    ``farm_seed(args.seed, k)``: results are reproducible and independent of scheduling, but not
    batch-for-batch those of the sequential order (``sweep_workers=1`` keeps that)."""
    from concurrent.futures import ThreadPoolExecutor
    points = _grid(hyperparams)
    dev = torch.device(args.device)
    tables = _sweep_tables(datasets, args)
    point_args = _point_args(args)
    jobs = []
    for idx, hp in enumerate(points):                      # models built here, in order: deterministic inits
        test_path, done = _result_file(args.savepath, hp)
        model = None
        if done is None:
            torch.manual_seed(farm_seed(args.seed, idx))
            model = _build_model(tables, hp, args.nclasses, args.modality, args.use_clip, args.logit, point_args["text_indim"])
        jobs.append((idx, hp, test_path, model, done))
    main_stream = torch.cuda.current_stream(dev)

    def run(job):
        idx, hp, test_path, model, done = job
        if done is not None:
            return done
        gen = torch.Generator()
        gen.manual_seed(farm_seed(args.seed, idx))
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(main_stream)                    # the shared tables were uploaded there
        with torch.cuda.stream(stream):
            res = setup_feature_run(datasets["img_tr"], datasets["img_val"], datasets["img_te"], datasets["text_ds"], hp,
                                    alpha=args.alpha, device=dev, eval_test=getattr(args, "eval_test", True),
                                    precision=getattr(args, "precision", "fp32"), tables=tables, generator=gen,
                                    order_rng=getattr(args, "order_rng", "torch-cpu"), model=model, **point_args)
            stream.synchronize()
        test_dict = {"test_acc": res["test_acc"], "val_acc": res["val_acc"], "model": res["model"], "iter": res["iter"]}
        torch.save(test_dict, test_path)
        return test_dict

    import umlh.head_engine as _he
    _he.ENQUEUE_LOCK = threading.Lock()
    try:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            outs = list(pool.map(run, jobs))
    finally:
        _he.ENQUEUE_LOCK = None
    results = {"test_acc": [o["test_acc"] for o in outs], "val_acc": [o["val_acc"] for o in outs],
               "hparams": points, "model_records": []}
    return _report(results, args)


def main(args):
    """``finetune.main`` (reference :451-510) over pre-extracted feature files: seeds, resolves the
    feature paths with the reference's scheme, builds the text dataset, sweeps HYPER_DICT[args.hyperparams]."""
    import features as F_
    from engine.tools.utils import set_random_seed
    if args.seed >= 0:
        set_random_seed(args.seed)
    args.device = getattr(args, "device", None) or "cuda:0"
    args.use_clip = getattr(args, "vision_model", "") == "" and getattr(args, "language_model", "") == ""
    enc_img = args.clip_encoder if args.use_clip else args.vision_model
    enc_txt = args.clip_encoder if args.use_clip else args.language_model
    encoder_name = enc_img if args.use_clip else f"{args.vision_model}-{args.language_model}"
    args.savepath = savedir(args.result_dir, args.dataset, encoder_name, args.train_shot, args.seed, args.text_type,
                            args.text_shot, args.image_augmentation, args.modality, args.classifier_init, args.alpha,
                            getattr(args, "text_batch_size", 0), getattr(args, "custom_name", ""), args)
    os.makedirs(args.savepath, exist_ok=True)
    text = F_.load_text_features(F_.text_outdir(args.feature_dir, enc_txt, args.dataset, args.text_type))
    shots = args.text_shot
    text_ds = TextTensorDataset(text["features"], text["labels"], text["eot_indices"],
                                n_shots=int(shots) if (shots != "average" and shots is not None) else shots)
    tr = F_.load_image_train_features(F_.img_outdir(args.feature_dir, enc_img, args.dataset, args.image_augmentation,
                                                    args.train_shot, args.seed, "train"))
    te = F_.load_image_test_features(F_.img_outdir(args.feature_dir, enc_img, args.dataset, args.image_augmentation,
                                                   args.train_shot, args.seed, "test"))
    args.img_indim, args.text_indim = tr["train"][0].shape[1], text["features"].shape[1]
    lab2cname = tr.get("lab2cname") or text.get("lab2cname")
    args.nclasses = len(lab2cname) if lab2cname else int(max(tr["train"][1].max(), te["test"][1].max())) + 1
    datasets = {"img_tr": tr["train"], "img_val": tr["val"], "img_te": te["test"], "text_ds": text_ds}
    return sweep(datasets, HYPER_DICT[args.hyperparams] if isinstance(args.hyperparams, str) else args.hyperparams, args)
