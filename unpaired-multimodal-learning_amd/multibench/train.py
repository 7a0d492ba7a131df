"""The MultiBench unpaired alternation loop (reference: MultiBench/train.py:354-399): two
INDEPENDENTLY shuffled loaders zipped, x loss switched off while epoch <= step_k in 'xy' mode,
loss = alpha_x*loss_x + alpha_y*loss_y, one optimizer step per batch pair, and the reference's
``evaluate`` / ``evaluate_raw_data`` (train.py:31-240): every train / val / test batch through the model
in eval mode, masked-mean pooling and binary logistic probes, all on the HIP kernels of ``umlh.probe``.
``train(effective_rank=True)`` adds the reference's per-step effective rank of the predicted y rows and of a fixed sample
of the y modality (train.py:302-345,380-389) on the HIP kernels of ``umlh.spectral``.
``train(capture_embeddings_during_training=True)`` adds the reference's embedding capture (train.py:300-347,456-512,533-536):
a fixed sample of sequence pairs through the model at every in-loop evaluation, its valid rows packed by ``umlh.seq_compact``
and compared by ``umlh.align`` and ``umlh.paired_cosine`` (``multibench.capture``).
``train(step_diagnostics=True)`` records the remaining ``train/*`` values the reference logs after every optimizer step
(train.py:403-439): the trivial next-frame losses and ``recon_y_loss`` on the HIP kernel of ``umlh.seq_step_stats``, and the
norms, ``loss_private`` and ``diff_next_*`` the forward already returns.
``rollout`` (train.py:268-292) generates every step of every row in one launch of ``umlh.rollout_rows``; ``spectral_bias`` /
``analyze_spectral_bias`` (train.py:245-266) take their spectra from ``umlh.seq_spectrum``; ``train(rollout_spectra=True)`` is
the reference's block train.py:474-482.  ``evaluate_robustness`` scores the probes ``evaluate`` fits on the noisy test sets of
``multibench.data.robust_loaders``, level by level.  The covariance matrices the reference forms and drops (train.py:386,388) and wandb
itself are outside this port."""
from __future__ import annotations

import copy

import numpy as np
import torch


# ---- labels (train.py:18-29) ----
def mosi_label(y_batch):
    """MOSI / MOSEI sentiment -> 0/1: >= 0 (which -0.0 is) becomes 1, < 0 becomes 0; NaN stays."""
    res = copy.deepcopy(y_batch)
    res[y_batch >= 0] = 1
    res[y_batch < 0] = 0
    return res


def sarcasm_label(y_batch):
    """Sarcasm / humor -1/+1 -> 0/1: only -1 is rewritten."""
    res = copy.deepcopy(y_batch)
    res[y_batch == -1] = 0
    return res


_LABELS = {"mosi": mosi_label, "mosei": mosi_label, "sarcasm": sarcasm_label, "humor": sarcasm_label}
_NAN_KEYS = [f"{t}/score_{k}" for k in ("x_private", "y_private", "x_complete", "y_complete", "xy_complete") for t in ("test", "val")]
_TYPES = ("train", "val", "test")


def _label_fn(ds_name):
    if ds_name not in _LABELS:                       # the reference accepts no other name here ('mimic' included)
        raise NotImplementedError("Dataset not implemented yet")
    return _LABELS[ds_name]


def _labels01(batches, ds_name, label_fn=None):
    """Integer labels of one split on the host: 0/1 by the dataset's rule (train.py:41-47), or what ``label_fn`` makes of them."""
    fn = label_fn if label_fn is not None else _label_fn(ds_name)
    lab = np.concatenate([np.asarray(b[3].detach().cpu().numpy() if isinstance(b[3], torch.Tensor) else b[3]) for b in batches])
    return np.asarray(fn(lab)).reshape(-1).astype(int)


def _two_classes(y, what):
    """The check sklearn makes before a fit; here on the host labels, so that the fits need no read-back."""
    if len(np.unique(y)) < 2:
        raise ValueError(f"This solver needs samples of at least 2 classes in the data, but the data contains only one class: {y[0]!r} ({what})")
    if y.min() < 0 or y.max() > 1:
        raise ValueError(f"{what}: the probes are binary, got labels {np.unique(y)[:5]}")


def _class_labels(lab, label_fn):
    """The label arrays of the three splits as the probes take them, and the number of classes.  Without ``label_fn`` the
    reference's binary labels, checked as before.  With one: two classes 0/1 stay as they are; anything else is remapped to
    the index in unique(train labels), as sklearn does (-1 for a value the train split does not hold: it counts as wrong)."""
    if label_fn is None:
        _two_classes(lab["train"], "train labels")
        return lab, 2
    classes = np.unique(lab["train"])
    if len(classes) < 2:
        raise ValueError(f"This solver needs samples of at least 2 classes in the data, but the data contains only one class: {lab['train'][0]!r} (train labels)")
    if len(classes) == 2 and classes[0] == 0 and classes[1] == 1:
        return lab, 2
    out = {}
    for t, y in lab.items():
        idx = np.minimum(np.searchsorted(classes, y), len(classes) - 1)
        out[t] = np.where(classes[idx] == y, idx, -1).astype(int)
    return out, len(classes)


def _kind(ds_name):
    return "liblinear" if ds_name == "mosi" else "lbfgs"         # train.py:97-99


class _Probes:
    """The fits and scores of one evaluate call: everything is enqueued first, ``read`` brings all counts back at once."""

    def __init__(self, ds_name, dev, n_classes=2):
        self.kind, self.dev, self.n_classes = _kind(ds_name), dev, n_classes
        self.counts, self.names, self.rows, self.clfs = [], [], [], []

    def fit(self, X, y, classifier_type="logistic", binary=False):
        """make_classifier(classifier_type, ds_name) of the reference (train.py:96-102), fitted.  More than two label classes
        make the logistic probe a ``SoftmaxProbe`` (what sklearn's LogisticRegression is then), unless ``binary`` says that
        this fit's own labels are 0/1 (the modality-separation probe)."""
        from umlh.probe import KNeighborsProbe, LogisticProbe, logistic_probe
        if classifier_type == "logistic" and self.n_classes > 2 and not binary:
            self.clfs.append(logistic_probe(self.kind, self.n_classes).fit(X, y, check_classes=False, n_classes=self.n_classes))
        elif classifier_type == "logistic":
            self.clfs.append(LogisticProbe(self.kind).fit(X, y, check_classes=False))
        elif classifier_type == "knn":
            self.clfs.append(KNeighborsProbe().fit(X, y))
        else:
            raise ValueError(f"Unsupported classifier type: {classifier_type}")
        return self.clfs[-1]

    def score(self, name, clf, X, y):
        self.counts.append(clf.correct(X, y))
        self.names.append(name)
        self.rows.append(X.shape[0])

    def read(self):
        got = torch.stack(self.counts).cpu().tolist()
        return {k: c / n for k, c, n in zip(self.names, got, self.rows)}


def _fit_three(pr, emb, lab, z, splits, name_of, classifier_type="logistic"):
    """The x, y and xy probes (train.py:163-183): each fitted on 'train' and scored on every key of ``splits``, under the name
    ``name_of(split, 'x' | 'y' | 'xy')``.  emb[k] is [N_k, zx + zy] with the x block in the first zx columns: the three
    feature sets are views of it (the row stride travels to the kernels)."""
    ytr = torch.from_numpy(lab["train"]).to(pr.dev)
    yev = {t: torch.from_numpy(lab[t]).to(pr.dev) for t in splits}
    for name, cols in (("x", slice(0, z[0])), ("y", slice(z[0], z[0] + z[1])), ("xy", slice(0, z[0] + z[1]))):
        clf = pr.fit(emb["train"][:, cols], ytr, classifier_type)
        for t in splits:
            pr.score(name_of(t, name), clf, emb[t][:, cols], yev[t])


def _pooled(parts, dims, dev):
    """The [N, dims[0] + dims[1]] fp32 device matrix of the masked means of ``parts``, a list of per-batch
    ``(x, x_lengths, y, y_lengths)`` (lengths None: the plain mean over time), batch under batch in their order."""
    import umlh
    emb = torch.empty((sum(p[0].shape[0] for p in parts), dims[0] + dims[1]), dtype=torch.float32, device=dev)
    off = 0
    for x, lx, y, ly in parts:
        bs = x.shape[0]
        umlh.masked_mean(x.float(), lx, out=emb[off:off + bs, :dims[0]])
        umlh.masked_mean(y.float(), ly, out=emb[off:off + bs, dims[0]:])
        off += bs
    return emb


def evaluate_raw_data(config, ds_name="mosi", device=None, return_probes=False, label_fn=None):
    """The raw-feature baselines (train.py:31-91): each modality's plain mean over time, probes on x, y and [x, y].
    ``return_probes`` adds the pooled [N, dx + dy] device matrices per split and the three fitted probes.  ``label_fn``: see
    ``evaluate``."""
    lab, n_classes = _class_labels({t: _labels01(config[t], ds_name, label_fn) for t in _TYPES}, label_fn)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        emb, dims = {}, None
        for t in _TYPES:
            dims = (config[t][0][0][0].shape[-1], config[t][0][0][2].shape[-1])
            emb[t] = _pooled([(b[0][0], None, b[0][2], None) for b in config[t]], dims, dev)
        pr = _Probes(ds_name, dev, n_classes)
        _fit_three(pr, emb, lab, dims, ("val", "test"), lambda t, name: f"{t}/score_{name}_raw")
        got = pr.read()
    results = {k: got[k] for k in ("val/score_x_raw", "val/score_y_raw", "test/score_x_raw", "test/score_y_raw", "test/score_xy_raw",
                                   "val/score_xy_raw")}
    return (results, emb, pr.clfs) if return_probes else results


def _embed_split(model, batches, dev, who="evaluate"):
    """One split through the eval-mode model and the masked mean (train.py:104-141): the pooled [N, zx + zy] device matrix,
    the (loss_x, loss_y) means over its batches as device doubles, and (zx, zy).  Everything is enqueued, nothing read back;
    the caller holds ``torch.no_grad`` and the device."""
    outs, lens = [], []
    for b in batches:
        x, y, lx, ly = b[0][0], b[0][2], b[1][0].to(dev), b[1][2].to(dev)
        outs.append(model(x.to(dev), y.to(dev), x_lengths=lx, y_lengths=ly))
        lens.append((lx, ly))
    z = (outs[0]["zx"].shape[-1], outs[0]["zy"].shape[-1])
    if z[0] != z[1]:
        raise ValueError(f"{who}: zx and zy have different widths {z}; the modality-separation probe stacks them")
    emb = _pooled([(o["zx"], lx, o["zy"], ly) for o, (lx, ly) in zip(outs, lens)], z, dev)
    loss = (torch.stack([o["loss_x"].reshape(()) for o in outs]).double().mean(),
            torch.stack([o["loss_y"].reshape(()) for o in outs]).double().mean())
    return emb, loss, z


def _begin_evaluation(model, ds_name, device, classifier_types, label_fn):
    """What ``evaluate`` and ``evaluate_robustness`` do before they touch a batch: the dataset's label rule must exist (unless
    ``label_fn`` replaces it), every classifier type must be known, and the model goes into eval mode.  Returns the types as a
    tuple and the device."""
    if label_fn is None:
        _label_fn(ds_name)
    classifier_types = tuple(classifier_types)
    for ct in classifier_types:
        if ct not in ("logistic", "knn"):
            raise ValueError(f"Unsupported classifier type: {ct}")
    dev = torch.device(device)
    model.eval()
    return classifier_types, dev


@torch.no_grad()
def evaluate(model, config, ds_name="mosi", device="cuda:0", return_embeddings=False, classifier_types=("logistic",), label_fn=None):
    """The reference's evaluate (train.py:93-240) with its batch layout and result keys.  The model forward is this
    project's eval-mode mirror; pooling, scaler statistics, fits and scores are HIP kernels, the embeddings never leave
    the device, and all six fits (three modality-separation probes, x, y, xy) are enqueued before anything is read back.
    The reference shuffles the rows of the modality-separation probe with np.random.permutation; the optimum of a fit does
    not depend on row order, so no shuffle is done here.  ``separate`` is False in the reference: the *_private and
    *_complete keys are NaN there and here.  ``return_embeddings`` adds the pooled [N, zx + zy] device matrices per split
    and the fitted probes (separation x 3, then x, y, xy per classifier type).
    ``classifier_types`` is the list the reference's loop iterates (train.py:165): 'logistic' or 'knn'
    (``umlh.KNeighborsProbe()``, train.py:99-100); a later type overwrites the score keys of an earlier one, as
    ``results.update`` inside that loop does, and any other name raises the reference's ValueError.  The modality-separation
    probe is always logistic (train.py:151).
    ``label_fn`` (default None: the dataset's binary rule, nothing changes): a callable that maps a batch's label array to
    integer labels, for a dataset name the reference raises on ('mimic' and its 6 classes) or a caller's own task.  With more
    than two classes in the train labels the x / y / xy logistic probes are ``umlh.SoftmaxProbe``s; the modality-separation
    probe stays binary."""
    classifier_types, dev = _begin_evaluation(model, ds_name, device, classifier_types, label_fn)
    lab, n_classes = _class_labels({t: _labels01(config[t], ds_name, label_fn) for t in _TYPES}, label_fn)
    emb, loss, z = {}, {}, None
    with torch.cuda.device(dev):
        for t in _TYPES:
            emb[t], loss[t], z = _embed_split(model, config[t], dev)
        pr = _Probes(ds_name, dev, n_classes)
        for t in _TYPES:                                            # which modality a pooled embedding came from (train.py:146-151)
            n = emb[t].shape[0]
            both = torch.cat([emb[t][:, :z[0]], emb[t][:, z[0]:]], dim=0)
            which = torch.cat([torch.zeros(n, dtype=torch.int32, device=dev), torch.ones(n, dtype=torch.int32, device=dev)])
            pr.score(f"sep/{t}", pr.fit(both, which, binary=True), both, which)
        for ct in classifier_types:
            _fit_three(pr, emb, lab, z, ("val", "test"), lambda t, name: f"{t}/score_{name}", ct)
        got = pr.read()
        losses = torch.stack([loss["val"][0], loss["test"][0], loss["val"][1], loss["test"][1]]).cpu().tolist()
    results = {"val/modality_separate": float(np.mean([got[f"sep/{t}"] for t in _TYPES]))}
    results.update({k: got[k] for k in ("test/score_x", "test/score_y", "test/score_xy", "val/score_x", "val/score_y", "val/score_xy")})
    results.update({k: float("nan") for k in _NAN_KEYS})
    results.update({"val/loss_x": losses[0], "test/loss_x": losses[1], "val/loss_y": losses[2], "test/loss_y": losses[3]})
    if return_embeddings:
        return results, emb, pr.clfs
    return results


@torch.no_grad()
def evaluate_robustness(model, config, robust, ds_name="mosi", device="cuda:0", classifier_types=("logistic",), label_fn=None):
    """Score curves over noise levels: what the reference's robustness protocol asks of a trained model (test sets corrupted
    at increasing levels, get_data.py:349-404), with ``evaluate``'s embeddings and probes.  ``config`` is ``evaluate``'s config
    (only 'train' is read); ``robust`` maps a family name to a sequence over levels of batch lists or loaders
    (``multibench.data.robust_loaders``).  The x / y / xy probes are fitted once on the clean train embeddings, exactly as
    ``evaluate`` fits them; every level's batches then go through the eval-mode forward and the masked mean and are scored with
    those fitted probes.  Levels are consumed one at a time (a lazily built loader's table is released with the next one);
    all scores are read back at once, the losses in a second read.
    Returns ``robust/{family}/score_x``, ``score_y``, ``score_xy``, ``loss_x``, ``loss_y`` as lists over the levels, ``n`` the
    rows per level (drops shrink it), and ``mean_score_x`` / ``_y`` / ``_xy``, the plain mean over the levels.  With several
    ``classifier_types`` a later one overwrites an earlier one's scores, as in ``evaluate``."""
    classifier_types, dev = _begin_evaluation(model, ds_name, device, classifier_types, label_fn)
    lab = {"train": _labels01(config["train"], ds_name, label_fn)}
    emb, loss, keys = {}, [], []
    with torch.cuda.device(dev):
        emb["train"], _loss, z = _embed_split(model, config["train"], dev, "evaluate_robustness")
        for family, levels in robust.items():
            for i in range(len(levels)):
                batches = levels[i]
                batches = batches if isinstance(batches, list) else list(batches)
                key = (family, i)
                lab[key] = _labels01(batches, ds_name, label_fn)
                emb[key], l_xy, _z = _embed_split(model, batches, dev, "evaluate_robustness")
                loss.extend(l_xy)
                keys.append(key)
                del batches
        lab, n_classes = _class_labels(lab, label_fn)
        pr = _Probes(ds_name, dev, n_classes)
        for ct in classifier_types:
            _fit_three(pr, emb, lab, z, keys, lambda key, name: f"{key[0]}/{key[1]}/{name}", ct)
        got = pr.read()
        losses = torch.stack(loss).cpu().tolist() if loss else []
    results = {}
    for family, levels in robust.items():
        idx = [j for j, k in enumerate(keys) if k[0] == family]
        for name in ("x", "y", "xy"):
            scores = [got[f"{family}/{keys[j][1]}/{name}"] for j in idx]
            results[f"robust/{family}/score_{name}"] = scores
            results[f"robust/{family}/mean_score_{name}"] = float(np.mean(scores)) if scores else float("nan")
        results[f"robust/{family}/loss_x"] = [losses[2 * j] for j in idx]
        results[f"robust/{family}/loss_y"] = [losses[2 * j + 1] for j in idx]
        results[f"robust/{family}/n"] = [int(emb[keys[j]].shape[0]) for j in idx]
    return results


def alternation_alphas(epoch, step_k, train_mode, alpha_x=1.0, alpha_y=1.0):
    """[alpha_x, alpha_y] for this epoch (train.py:355-358)."""
    alphas = [alpha_x, alpha_y]
    if epoch <= step_k and train_mode == "xy":
        alphas[0] = 0.0
    return alphas


def _unpack(batch, modality, ds_name, which):
    if ds_name != "mimic":
        return batch[0][modality].float(), batch[1][modality]          # _process_1 layout (get_data.py:418-444)
    return (batch[0].float(), batch[2]) if which == 0 else (batch[1].float(), batch[3])


def _sample_rank(seqs, lens, dev):
    """Effective rank of the valid rows (t < len) of per-batch [b, T, d] device blocks pooled into one matrix: a 0-d float64
    device tensor.  Batches may differ in T; each is padded with zero rows, which the row predicate leaves out anyway."""
    import umlh
    T = max(s.shape[1] for s in seqs)
    block = torch.cat([torch.nn.functional.pad(s, (0, 0, 0, T - s.shape[1])) for s in seqs], dim=0)
    with torch.cuda.device(dev):
        return umlh.effective_rank_seq(block, torch.cat(lens), drop_last=0)[0]


def _fixed_sample_rank(loader, modality, ds_name, dev, n_samples=1000):
    """``_sample_rank`` of the first ``n_samples`` sequences of a deep copy of ``loader``, y side only (train.py:302-345,387)."""
    seqs, lens, left = [], [], n_samples
    for batch in copy.deepcopy(loader):
        y, ly = _unpack(batch, modality, ds_name, 1)
        y = y.unsqueeze(1) if y.ndim == 2 else y
        seqs.append(y[:left].to(dev))
        lens.append(torch.as_tensor(ly)[:left].reshape(-1).to(dev))
        left -= seqs[-1].shape[0]
        if left <= 0:
            break
    if not seqs:
        raise ValueError("train(effective_rank=True): train_loader_2 yields no batch")
    return _sample_rank(seqs, lens, dev)


def _record_diagnostics(diag, out, x1, l1, x2, l2, dev):
    """Appends one step's logged values (train.py:403-433) to the lists of ``diag`` as 0-d device tensors; nothing is read back.
    x and y take one ``umlh.seq_step_stats`` call each, y's with ``y_recon`` so that its rows t + 1 serve both statistics.
    The two loss norms need no device work: ``train`` takes |loss| of the values it reads back anyway."""
    import umlh
    seq = lambda t: t.unsqueeze(1) if t.ndim == 2 else t
    put = lambda k, v: diag.setdefault(k, []).append(v.detach())
    with torch.cuda.device(dev):
        if x1 is not None:
            put("trivial_loss_x", umlh.seq_step_stats(seq(x1), l1)[umlh.stepstats.TRIVIAL])
        if x2 is not None:
            s = umlh.seq_step_stats(seq(x2), l2, recon=out["y_recon"].detach())
            put("trivial_loss_y", s[umlh.stepstats.TRIVIAL])
            put("recon_y_loss", s[umlh.stepstats.RECON])
    put("loss_private", out["loss_private"])
    for k in ("diff_next_x", "diff_next_y"):
        if out[k] is not None:
            put(k, out[k])


# ---- rollout and spectral bias (train.py:245-292) ----
def _rollout_params(model, proj_in, dec):
    """The arguments of ``umlh.rollout_rows`` for one modality of ``model``."""
    from .encoder import layer_params
    enc = model.encoder
    if getattr(enc, "out_last", False):
        raise ValueError("rollout: the encoder returns only its last token (out_last=True); the decoder needs [B, T, Z] "
                         "(the reference's own indexing fails there)")
    pos0 = None
    if enc.pos_embd:
        pos0 = enc.pos_embedding.weight[0] if enc.pos_learnable else enc.pos_table[0]
    layers = enc.transformer.layers
    lp = [t for layer in layers for t in layer_params(layer)]
    eps = float(layers[0].norm1.eps) if len(layers) else 1e-5
    return proj_in.fc.weight, proj_in.fc.bias, enc.conv.weight if enc.conv1d else None, pos0, lp, eps, dec.fc.weight, dec.fc.bias


@torch.no_grad()
def rollout(model, x, y, steps=10):
    """The reference's rollout (train.py:268-292): each input [B, T0, D] is continued from its LAST frame for ``steps``
    frames through in-projection, shared encoder and decoder, and returned as [B, T0 + steps, D] (the input followed by the
    generated frames); an input that is None gives None.  All steps of a modality are one launch of ``umlh.rollout_rows``,
    which writes the generated frames straight into the result.  Puts the model into eval mode and, like the reference,
    leaves it there."""
    import umlh
    model.eval()
    preds = []
    for seq, proj_in, dec in ((x, model.xproj_in, model.decoders[0]), (y, model.yproj_in, model.decoders[1])):
        if seq is None:
            preds.append(None)
            continue
        if seq.ndim != 3:
            raise ValueError(f"rollout: expected [B, T0, D] inputs, got {tuple(seq.shape)}")
        if not seq.is_cuda:
            raise RuntimeError("rollout runs on the HIP kernels only: move the model and inputs to the GPU")
        w_in, b_in, conv_w, pos0, lp, eps, w_out, b_out = _rollout_params(model, proj_in, dec)
        B, T0, D = seq.shape
        steps = int(steps)
        with torch.cuda.device(seq.device):
            full = torch.empty((B, T0 + steps, D), dtype=torch.float32, device=seq.device)
            full[:, :T0] = seq
            umlh.rollout_rows(full[:, T0 - 1], w_in, b_in, conv_w, pos0, lp, eps, w_out, b_out, steps, out=full[:, T0 - 1:])
        preds.append(full)
    return preds[0], preds[1]


def spectral_bias(ground_truth, prediction):
    """(mag_gt, mag_pred) of train.py:246-251: ``abs(rfft(., dim=1)).mean(dim=(0, 2))`` of the two [B, T, D] blocks, float64
    device tensors from ``umlh.seq_spectrum``."""
    import umlh

    def one(t):
        if not t.is_cuda:
            return umlh.seq_spectrum(t)                     # moved to the current device
        with torch.cuda.device(t.device):
            return umlh.seq_spectrum(t)
    return one(ground_truth.detach()), one(prediction.detach())


def analyze_spectral_bias(ground_truth, prediction, loss_value, iteration, modality_name='modality', postfix=""):
    """The reference's analyze_spectral_bias (train.py:245-266): the two spectra from the HIP kernel, drawn into the
    reference's log-log figure ``spectral_analysis{postfix}/spectral_analysis_{modality_name}_{iteration}_loss_{loss:.4f}.png``
    when matplotlib can be imported (it is not a dependency: without it no file is written).  Always returns
    (mag_gt, mag_pred)."""
    import os
    mag_gt, mag_pred = spectral_bias(ground_truth, prediction)
    try:
        import matplotlib.pyplot as plt
    except ImportError:
        return mag_gt, mag_pred
    gt, pred = mag_gt.cpu(), mag_pred.cpu()
    freqs = torch.arange(gt.shape[0])
    plt.figure(figsize=(10, 6))
    plt.plot(freqs, gt, label='Ground Truth (High Freq Source)', alpha=0.8, color='black')
    plt.plot(freqs, pred, label='Prediction (Transformer Output)', alpha=0.8, color='red', linestyle='--')
    plt.xscale('log')
    plt.yscale('log')
    plt.title(f'Spectral Analysis: {modality_name} (Log-Log Scale)')
    plt.xlabel('Frequency (Log scale)')
    plt.ylabel('Magnitude (Log scale)')
    plt.legend()
    plt.grid(True, which="both", ls="-", alpha=0.2)
    os.makedirs(f'spectral_analysis{postfix}', exist_ok=True)
    plt.savefig(f'spectral_analysis{postfix}/spectral_analysis_{modality_name}_{iteration}_loss_{loss_value:.4f}.png', dpi=300)
    return mag_gt, mag_pred


def _capture_spectra(model, capture):
    """train.py:474-482 with sample_idx = 0: the first batch of the fixed sample rolled out from its first frames for T - 1
    steps, and the spectra of the sample and of the rollout, per modality."""
    x, y = capture.x1[0], capture.x2[0]
    x_pred, _ = rollout(model, x[:, :1], None, steps=x.shape[1] - 1)
    _, y_pred = rollout(model, None, y[:, :1], steps=y.shape[1] - 1)
    x_gt, x_pr = spectral_bias(x, x_pred)
    y_gt, y_pr = spectral_bias(y, y_pred)
    return {"x_gt": x_gt, "x_pred": x_pr, "y_gt": y_gt, "y_pred": y_pr}


def train(model, train_mode, train_loader_1, train_loader_2, optimizer, modalities=[0, 2], num_epoch=100, step_k=30,
          ds_name="mosi", eval_config={}, alpha_x=1.0, alpha_y=1.0, capture_embeddings_during_training=False, augment=False,
          debug=False, args=None, device="cuda:0", step_diagnostics=False, rollout_spectra=False, on_step=None, effective_rank=False):
    """Returns {'loss_x': [...], 'loss_y': [...], 'loss': [...]} with one entry per batch pair
    (device tensors are read back once at the end).  With a non-empty ``eval_config`` ({'train', 'val', 'test': batch
    lists, 'freq': int, optionally 'classifier_types': the probes of ``evaluate``, default ('logistic',), and 'label_fn': ``evaluate``'s label rule, default None}) it evaluates as the reference does (train.py:350,440-451,519-523): ``evaluate_raw_data`` once,
    ``evaluate`` whenever i_batch % freq == 0 and once more after the last epoch, the model back in train mode after
    each; the dict then also holds 'raw' and 'eval' = [(epoch, i_batch, results), ...], where results are what the
    reference logs (evaluate's keys without the *_private / *_complete ones, plus the raw baselines) and the closing
    evaluation is the entry with i_batch = None.

    ``effective_rank=True`` with 'y' in ``train_mode`` adds 'pred_effective_rank_y': per batch pair the effective rank
    (utilis.py:27-36) of the rows y_recon[b, t], t < len_b - 1, of the step's own forward (train.py:381-389), enqueued on the
    training stream and read back at the end with the losses; and 'gt_effective_rank_y': that of the valid rows of the
    first up-to-1000 sequences of a copy of ``train_loader_2`` (train.py:302-345,387), a constant the reference recomputes
    every step and this loop computes once.

    ``capture_embeddings_during_training=True`` (needs a non-empty ``eval_config``: the reference captures only inside its
    evaluation branch) takes the reference's fixed sample of up to 1000 sequence pairs once (``multibench.capture``,
    train.py:302-347) and, after every in-loop evaluation, runs it through the model and adds the eleven ``val/cka_*``,
    ``val/mknn_*`` and ``val/cos_sim_*`` values of train.py:492-512 to that entry of 'eval' (not to the closing one, as in the
    reference).  The dict then also holds 'embeddings' = {'x1': [E, N, z], 'x2': [E, N, z] (fp32 device stacks of the packed zx
    and zy rows, one per capture, in capture order), 'x1_label', 'x2_label'} (train.py:533-536).  With ``effective_rank`` as
    well, 'gt_effective_rank_y' is computed from the capture's y sample, as the reference does (:345,:387).

    ``step_diagnostics=True`` adds the other values the reference logs at every step (train.py:403-439), one list per key and
    one entry per batch pair, enqueued on the training stream and read back at the end with the losses: 'trivial_loss_x' (with
    'x' in ``train_mode``) and 'trivial_loss_y', 'recon_y_loss' (with 'y' in it) from ``umlh.seq_step_stats`` on the step's own
    inputs and ``y_recon``; 'loss_x_norm', 'loss_y_norm' (``torch.norm`` of a 0-d tensor is |loss|: taken from the losses read back); 'loss_private'; and
    'diff_next_x' / 'diff_next_y' for the modalities present.

    ``rollout_spectra=True`` (needs ``capture_embeddings_during_training=True``) is the reference's block train.py:474-482: after
    each in-loop capture the first batch of the fixed sample (its ``sample_idx = 0``) is rolled out from its first frames for
    T - 1 steps per modality (``rollout``) and 'spectra' gets (epoch, i_batch, {'x_gt', 'x_pred', 'y_gt', 'y_pred'}), the
    float64 spectra of ``spectral_bias`` as host lists.  No figure is drawn.  With the flag off nothing changes."""
    if rollout_spectra and not capture_embeddings_during_training:
        raise ValueError("train(rollout_spectra=True) needs capture_embeddings_during_training=True: the reference rolls out "
                         "the capture's fixed sample (train.py:457-482)")
    spectra = []
    model.train()
    dev = torch.device(device)
    rec_x, rec_y, rec_l, rec_rank = [], [], [], []
    want_rank = bool(effective_rank) and "y" in train_mode
    diag = {} if step_diagnostics else None
    capture, cap_x, cap_y = None, [], []
    if capture_embeddings_during_training:
        from .capture import EmbeddingCapture, take_fixed_samples
        if not eval_config:
            raise ValueError("train(capture_embeddings_during_training=True) needs an eval_config: the capture runs after each "
                             "in-loop evaluation (train.py:440-457)")
        capture = EmbeddingCapture(take_fixed_samples(train_loader_1, train_loader_2, modalities, ds_name), dev)
    if want_rank and capture is not None:
        gt_rank = _sample_rank(capture.x2, capture.l2, dev)
    else:
        gt_rank = _fixed_sample_rank(train_loader_2, modalities[1], ds_name, dev) if want_rank else None
    raw_results, evals = None, []
    classifier_types = tuple(eval_config.get("classifier_types", ("logistic",)))
    if eval_config:
        raw_results = evaluate_raw_data(eval_config, ds_name=ds_name, device=device, label_fn=eval_config.get("label_fn"))

    def logged_evaluation():
        score = evaluate(model, eval_config, ds_name, device=device, classifier_types=classifier_types, label_fn=eval_config.get("label_fn"))
        out = {k: v for k, v in score.items() if not ("private" in k or "complete" in k)}
        out.update(raw_results)
        return out

    for epoch in range(num_epoch):
        alphas = alternation_alphas(epoch, step_k, train_mode, alpha_x, alpha_y)
        for i_batch, (b1, b2) in enumerate(zip(train_loader_1, train_loader_2)):
            x1, l1 = _unpack(b1, modalities[0], ds_name, 0)
            x2, l2 = _unpack(b2, modalities[1], ds_name, 1)
            x1, x2, l1, l2 = x1.to(dev), x2.to(dev), l1.to(dev), l2.to(dev)
            if "x" not in train_mode:
                x1 = None
            if "y" not in train_mode:
                x2 = None
            out = model(x1, x2, l1, l2)
            loss = alphas[0] * out["loss_x"] + alphas[1] * out["loss_y"]
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            rec_x.append(out["loss_x"].detach())
            rec_y.append(out["loss_y"].detach())
            rec_l.append(loss.detach())
            if want_rank:
                import umlh
                with torch.cuda.device(dev):
                    rec_rank.append(umlh.effective_rank_seq(out["y_recon"].detach(), l2, drop_last=1)[0])
            if diag is not None:
                _record_diagnostics(diag, out, x1, l1, x2, l2, dev)
            if on_step is not None:
                on_step(epoch, i_batch, out, loss)
            if eval_config and i_batch % eval_config["freq"] == 0:
                evals.append((epoch, i_batch, logged_evaluation()))
                if capture is not None:
                    values, zx, zy = capture.measure(model)
                    evals[-1][2].update(values)
                    cap_x.append(zx)
                    cap_y.append(zy)
                    if rollout_spectra:
                        spectra.append((epoch, i_batch, _capture_spectra(model, capture)))
                model.train()
        if eval_config and epoch == num_epoch - 1:
            evals.append((epoch, None, logged_evaluation()))
            model.train()
    stack = lambda v: torch.stack([t.reshape(()) for t in v]).cpu().tolist() if v else []
    res = {"loss_x": stack(rec_x), "loss_y": stack(rec_y), "loss": stack(rec_l)}
    if want_rank:
        res["pred_effective_rank_y"] = stack(rec_rank)
        res["gt_effective_rank_y"] = float(gt_rank.cpu())
    if diag is not None:
        res.update({k: stack(v) for k, v in diag.items()})
        res["loss_x_norm"], res["loss_y_norm"] = [abs(v) for v in res["loss_x"]], [abs(v) for v in res["loss_y"]]
    if eval_config:
        res["raw"], res["eval"] = raw_results, evals
    if capture is not None:
        res["embeddings"] = {"x1": torch.stack(cap_x) if cap_x else None, "x2": torch.stack(cap_y) if cap_y else None,
                             "x1_label": capture.labels[0], "x2_label": capture.labels[1]}
    if rollout_spectra:
        res["spectra"] = [(e, i, {k: v.cpu().tolist() for k, v in sp.items()}) for e, i, sp in spectra]
    return res
