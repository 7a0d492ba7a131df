"""The feature capture of the reference's fine-tune loop (vision_language/finetune.py:127-155, 208-233, 280-287) on the HIP
kernels of ``umlh``: after every optimizer step a fixed sample of image rows is projected through ``extract_features`` in
eval mode, and the step logs

    train/inclass_distance   mean over classes of the mean distance of a class's rows to the class mean   (umlh.class_stats)
    train/cka_score          linear CKA of the class means against a fixed text sample                    (umlh.align.cka)
    train/mknn_score         mutual 10-NN of the image features against the text sample                   (umlh.align.knn)

and keeps the step's features; at the end five ``.pth`` files are written.  The reference forms the class part in a Python
loop over the classes with a ``nonzero``, two reductions and an ``.item()`` each; here the sample's class index is built once
and a step is a handful of launches with no host synchronisation: ``step()`` returns three device scalars for the caller to
read with whatever it reads anyway.

Shape rules.  The reference's CKA needs as many text rows as classes and its mutual k-NN as many text rows as image rows;
with its hard-coded 16 shots one of the two raises at step 0.  Here a score whose row counts disagree (and mutual k-NN on 10
rows or fewer) is disabled at construction with one printed line and reported as NaN; ``strict=True`` raises ``ValueError``
instead.  With no text sample both scores are 0, as in the reference (:232-233).
"""
from __future__ import annotations

import os

import torch

import umlh

TOPK = 10          # finetune.py:116-118
ROWS_PER_PASS = 512    # finetune.py:149,213
BLOCK_BYTES = 64 << 20
FILES = {"raw": "all_iter_image_raw_features.pth", "image": "all_iter_image_features.pth", "image_labels": "all_iter_image_labels.pth",
         "text": "all_iter_text_features.pth", "text_labels": "all_iter_text_labels.pth"}


class FeatureCapture:
    """``FeatureCapture(model, image_rows, image_labels, text_rows, n_class)``; ``text_rows`` may be None.  ``text_labels``
    are only saved.  ``keep_features=False`` keeps no per-step features (``save`` then writes no stack)."""

    def __init__(self, model, image_rows, image_labels, text_rows, n_class, *, text_labels=None, keep_features=True, strict=False):
        dev = model.head.weight.device
        if dev.type != "cuda":
            raise umlh.UmlhError("FeatureCapture needs the model on a GPU: the statistics run only as HIP kernels")
        self.model, self.n_class, self.keep_features = model, int(n_class), bool(keep_features)
        self.image_rows = image_rows.detach().to(dev, torch.float32).contiguous()
        self.image_labels = image_labels.detach().to(dev, torch.int64).contiguous()
        n = self.image_rows.shape[0]
        if self.image_rows.ndim != 2 or n < 1 or self.image_labels.shape != (n,):
            raise ValueError(f"FeatureCapture: image sample of shape {tuple(image_rows.shape)} with labels {tuple(image_labels.shape)}")
        self.n, self.d = n, int(model.shared_dim)
        self.order, self.offsets = umlh.class_index(self.image_labels, self.n_class)
        self.text_rows = self.text_labels = self.text_knn = None
        self.with_cka = self.with_mknn = False
        if text_rows is not None:
            self.text_rows = text_rows.detach().to(dev, torch.float32).contiguous()
            self.text_labels = None if text_labels is None else text_labels.detach().to("cpu")
            m = self.text_rows.shape[0]
            self.with_cka = self._rule(m == self.n_class, strict,
                                       f"train/cka_score: {m} text rows against {self.n_class} class means")
            self.with_mknn = self._rule(m == n and n > TOPK, strict,
                                        f"train/mknn_score: {m} text rows against {n} image rows (needs equal counts above {TOPK})")
            if self.with_mknn:
                self.text_knn = umlh.align.knn(self.text_rows, TOPK)
        per_step = n * self.d * 4
        self.block_steps = max(1, BLOCK_BYTES // per_step) if self.keep_features else 1
        self.block = torch.empty((self.block_steps, n, self.d), dtype=torch.float32, device=dev)
        self.means = torch.empty((self.n_class, self.d), dtype=torch.float32, device=dev)
        self.filled, self.host_blocks, self.steps = 0, [], 0
        self._zero = torch.zeros((), dtype=torch.float64, device=dev)
        self._nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        self._raw_saved = None

    @staticmethod
    def _rule(ok, strict, what):
        if not ok:
            if strict:
                raise ValueError(f"FeatureCapture: {what}")
            print(f"=> {what}: disabled, logged as NaN")
        return ok

    def _features_into(self, dst):
        for j in range(0, self.n, ROWS_PER_PASS):
            self.model.extract_features(self.image_rows[j:j + ROWS_PER_PASS], out=dst[j:j + ROWS_PER_PASS])

    def _flush(self):
        """The filled part of the device block as a pinned host tensor; the copy is enqueued behind the steps that filled it
        and ahead of the steps that will overwrite it, and is waited for in ``features``."""
        if self.filled:
            host = torch.empty((self.filled, self.n, self.d), dtype=torch.float32, pin_memory=True)
            host.copy_(self.block[:self.filled], non_blocking=True)
            self.host_blocks.append(host)
            self.filled = 0

    def step(self):
        """One capture -> (inclass_distance, cka_score, mknn_score): three 0-d float64 device tensors, no host sync."""
        with torch.no_grad():
            self.model.eval()
            if self.keep_features and self.filled == self.block_steps:
                self._flush()
            feats = self.block[self.filled]
            self._features_into(feats)
            _, _, out2 = umlh.class_stats(feats, self.order, self.offsets, self.n_class, means_out=self.means)
            if self.text_rows is None:
                cka = mknn = self._zero
            else:
                cka = umlh.align.cka(self.means, self.text_rows) if self.with_cka else self._nan
                mknn = (umlh.align.mutual_knn_lists(umlh.align.knn(feats, TOPK), self.text_knn) if self.with_mknn else self._nan)
            if self.keep_features:
                self.filled += 1
            self.steps += 1
            self.model.train()
        return out2[0], cka, mknn

    def raw_features(self):
        """``extract_raw_features`` of the sample in eval mode, on the CPU (finetune.py:146-155)."""
        with torch.no_grad():
            self.model.eval()
            raw = torch.cat([self.model.extract_raw_features(self.image_rows[j:j + ROWS_PER_PASS]).detach().cpu()
                             for j in range(0, self.n, ROWS_PER_PASS)], dim=0)
            self.model.train()
        return raw

    def features(self):
        """Every kept step's features, [steps, rows, shared_dim] on the CPU (None with ``keep_features=False``)."""
        if not self.keep_features:
            return None
        self._flush()
        torch.cuda.current_stream(self.block.device).synchronize()
        if not self.host_blocks:
            return torch.empty((0, self.n, self.d), dtype=torch.float32)
        if len(self.host_blocks) > 1:
            self.host_blocks = [torch.cat(self.host_blocks, dim=0)]
        return self.host_blocks[0]

    def save_raw(self, features_pth):
        os.makedirs(features_pth, exist_ok=True)
        torch.save(self.raw_features(), os.path.join(features_pth, FILES["raw"]))
        self._raw_saved = os.path.abspath(features_pth)

    def save(self, features_pth):
        """The reference's five files (finetune.py:155, 280-287): raw features [rows, raw_dim], the per-step features
        [steps, rows, shared_dim], the sample's labels, and the text sample with its labels when there is one."""
        os.makedirs(features_pth, exist_ok=True)
        if self._raw_saved != os.path.abspath(features_pth):
            self.save_raw(features_pth)
        if self.keep_features:
            torch.save(self.features().clone(), os.path.join(features_pth, FILES["image"]))
        torch.save(self.image_labels.cpu(), os.path.join(features_pth, FILES["image_labels"]))
        if self.text_rows is not None:
            torch.save(self.text_rows.cpu(), os.path.join(features_pth, FILES["text"]))
            if self.text_labels is not None:
                torch.save(self.text_labels, os.path.join(features_pth, FILES["text_labels"]))
