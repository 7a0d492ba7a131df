"""The embedding capture of the reference's MultiBench loop (MultiBench/train.py:300-347,456-512,533-536): a fixed sample of
up to 1000 sequence pairs taken once from copies of the two loaders, run through the model at every evaluation, its valid
rows packed into matrices and compared with linear CKA, mutual k-NN (topk 10) and the mean paired cosine.

``take_fixed_samples`` is host code; ``EmbeddingCapture`` keeps the sample on the device and measures on HIP kernels only:
``umlh.seq_compact`` packs the rows at row offsets known on the host, ``umlh.align.cka`` / ``umlh.align.mutual_knn`` /
``umlh.paired_cosine`` are enqueued back to back and all nine values come back in one transfer.  The reference's one
``.item()`` per sequence and per evaluation is gone."""
from __future__ import annotations

import copy

import torch

MKNN_TOPK = 10                                   # utilis.py:23-25
KEYS = ("val/cka_proj", "val/mknn_proj", "val/cos_sim_proj", "val/cka_embed", "val/mknn_embed", "val/cos_sim_embed",
        "val/cka_out", "val/mknn_out", "val/cka_text_embeddings_features", "val/cka_raw", "val/mknn_raw")


def _offsets(seqs, lens):
    """Host row offsets of every batch in the packed matrix, by the row predicate of umlh.seq_compact."""
    from umlh.capture import valid_rows
    off = [0]
    for s, l in zip(seqs, lens):
        off.append(off[-1] + int(valid_rows(l, s.shape[1]).sum()))
    return off


def take_fixed_samples(loader_1, loader_2, modalities, ds_name, n_samples=1000):
    """The reference's selection (train.py:302-331): deep copies of the two loaders, zipped; from pair i the first
    min(batch_size, n_samples - i * batch_size) rows; stop once (i + 1) * batch_size >= n_samples.  ``batch_size`` is
    ``loader_1.batch_size``, or the first batch's row count when the loader has no such attribute (a list of batches).

    Returns {'x1', 'x2': per-batch fp32 [b, T, d] tensors, 'lx1', 'lx2': per-batch lengths, 'x1_label', 'x2_label': the
    concatenated element 3 of the batches or None when they carry none, 'off1', 'off2': host row offsets of every batch
    (len(batches) + 1 entries, rows counted as clamp(len, 0, T)), 'rows': the common total}."""
    if ds_name == "mimic":
        raise NotImplementedError("the embedding capture collects no sequence lengths for 'mimic' (train.py:321-327 keeps none, "
                                  ":337 then needs them)")
    batch_size = getattr(loader_1, "batch_size", None)
    s = {"x1": [], "x2": [], "lx1": [], "lx2": []}
    lab1, lab2 = [], []
    for i, (b1, b2) in enumerate(zip(copy.deepcopy(loader_1), copy.deepcopy(loader_2))):
        x1, x2 = b1[0][modalities[0]].float(), b2[0][modalities[1]].float()
        if batch_size is None:
            batch_size = x1.shape[0]
        take = batch_size if (i + 1) * batch_size <= n_samples else n_samples - i * batch_size
        x1, x2 = (x.unsqueeze(1) if x.ndim == 2 else x for x in (x1, x2))
        s["x1"].append(x1[:take])
        s["x2"].append(x2[:take])
        s["lx1"].append(torch.as_tensor(b1[1][modalities[0]])[:take])
        s["lx2"].append(torch.as_tensor(b2[1][modalities[1]])[:take])
        if len(b1) > 3 and len(b2) > 3:
            lab1.append(torch.as_tensor(b1[3])[:take])
            lab2.append(torch.as_tensor(b2[3])[:take])
        if (i + 1) * batch_size >= n_samples:
            break
    s["x1_label"] = torch.cat(lab1, dim=0) if lab1 and len(lab1) == len(s["x1"]) else None
    s["x2_label"] = torch.cat(lab2, dim=0) if lab2 and len(lab2) == len(s["x2"]) else None
    s["off1"], s["off2"] = _offsets(s["x1"], s["lx1"]), _offsets(s["x2"], s["lx2"])
    n1, n2 = s["off1"][-1], s["off2"][-1]
    if n1 != n2:
        raise ValueError(f"embedding capture: the fixed sample has {n1} valid rows of modality x and {n2} of modality y; "
                         "CKA, mutual k-NN and the paired cosine compare row i with row i and need equal counts")
    if n1 <= MKNN_TOPK:
        raise ValueError(f"embedding capture: the fixed sample has {n1} valid rows of modality x and {n2} of modality y; "
                         f"mutual k-NN with topk {MKNN_TOPK} needs at least {MKNN_TOPK + 1}")
    s["rows"] = n1
    return s


def _clip_raw(v):
    return min(max(v, 0.0), 1.0)                  # train.py:346-347


def _clip(v):
    return max(min(v, 1.0), 0.0)                  # train.py:492,497,502,507


class EmbeddingCapture:
    """The fixed sample on ``device`` and its raw-feature baselines.  ``measure(model)`` is one capture; ``matrices`` then
    holds the six packed [N, .] matrices of the latest one ('zx', 'zy', 'x_proj', 'y_proj', 'x_recon', 'y_recon')."""

    def __init__(self, samples, device):
        import umlh
        self.dev = torch.device(device)
        self.rows = samples["rows"]
        self.off1, self.off2 = samples["off1"], samples["off2"]
        self.labels = (samples["x1_label"], samples["x2_label"])
        up = lambda ts, dt: [torch.as_tensor(t).to(device=self.dev, dtype=dt) for t in ts]
        self.x1, self.x2 = up(samples["x1"], torch.float32), up(samples["x2"], torch.float32)
        self.l1, self.l2 = up(samples["lx1"], torch.int64), up(samples["lx2"], torch.int64)
        self.matrices = {}
        with torch.cuda.device(self.dev):
            self.raw_x = self._pack(self.x1, self.l1, self.off1)
            self.raw_y = self._pack(self.x2, self.l2, self.off2)
            raw = torch.stack([umlh.align.cka(self.raw_x, self.raw_y),
                               umlh.align.mutual_knn(self.raw_x, self.raw_y, topk=MKNN_TOPK)]).cpu().tolist()
        self.cka_raw, self.mknn_raw = _clip_raw(raw[0]), _clip_raw(raw[1])

    def _pack(self, blocks, lens, off, out=None):
        """The valid rows of every batch's block at the host offsets of one [N, d] matrix."""
        import umlh
        if out is None:
            out = torch.empty((self.rows, blocks[0].shape[-1]), dtype=torch.float32, device=self.dev)
        for i, (z, l) in enumerate(zip(blocks, lens)):
            umlh.seq_compact(z, l, out=out[off[i]:off[i + 1]])
        return out

    def _matrix(self, name, d, fresh):
        m = self.matrices.get(name)
        if fresh or m is None or m.shape[1] != d:
            m = self.matrices[name] = torch.empty((self.rows, d), dtype=torch.float32, device=self.dev)
        return m

    @torch.no_grad()
    def measure(self, model):
        """One capture (train.py:456-512) -> (the eleven ``val/*`` values, zx [N, z], zy [N, z]).  The model runs in eval mode
        and is put into train mode afterwards, as the reference's evaluation branch leaves it.  zx and zy are fresh device
        matrices (the caller keeps them); the other four are reused by the next capture.  One device-to-host transfer."""
        import umlh
        names = (("zx", 1), ("x_proj", 1), ("x_recon", 1), ("zy", 2), ("y_proj", 2), ("y_recon", 2))
        model.eval()
        with torch.cuda.device(self.dev):
            outs = [model(x1, x2, l1, l2) for x1, x2, l1, l2 in zip(self.x1, self.x2, self.l1, self.l2)]
            m = {}
            for name, side in names:
                lens, off = (self.l1, self.off1) if side == 1 else (self.l2, self.off2)
                m[name] = self._pack([o[name] for o in outs], lens, off,
                                     out=self._matrix(name, outs[0][name].shape[-1], fresh=name in ("zx", "zy")))
            al = umlh.align.measure_pairs([(m["x_proj"], m["y_proj"]), (m["zx"], m["zy"]), (m["x_recon"], m["y_recon"]),
                                           (m["zy"], self.raw_y, {"topk": 0})], topk=MKNN_TOPK)      # the seven metrics in one call
            got = torch.stack([al[0, 0], al[0, 4], umlh.paired_cosine(m["x_proj"], m["y_proj"]),
                               al[1, 0], al[1, 4], umlh.paired_cosine(m["zx"], m["zy"]),
                               al[2, 0], al[2, 4], al[3, 0]]).cpu().tolist()
        model.train()
        res = dict(zip(KEYS[:9], got))
        for k in ("val/cka_proj", "val/cka_embed", "val/cka_out", "val/cka_text_embeddings_features"):
            res[k] = _clip(res[k])
        res["val/cka_raw"], res["val/mknn_raw"] = self.cka_raw, self.mknn_raw
        return res, m["zx"], m["zy"]
