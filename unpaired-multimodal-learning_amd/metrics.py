"""The reference's alignment-metrics module (vision_language/metrics.py; the same in MultiBench/ and Gaussian_experiment/)
on the HIP kernels of ``umlh.align``.

Built: ``cka`` with ``kernel_metric='ip'`` and ``unbiased=False`` (what every caller uses), ``mutual_knn`` and
``compute_nearest_neighbors``.  The other names of ``SUPPORTED_METRICS`` raise ``NotImplementedError`` here (all but
``svcca`` run as HIP kernels through ``umlh.align.measure``, which takes the same names and keyword arguments; ``svcca``
is ``umlh.align.svcca(feats_A, feats_B, cca_dim)``); unknown names raise ``ValueError`` as the reference does.  Like the reference's ``.item()``, ``measure`` returns Python floats.

The module-level ``remove_outliers`` and ``compute_knn_accuracy`` are built too (``umlh.align.remove_outliers``,
``umlh.align.knn_accuracy``: a radix select instead of the reference's sorts), so every name of the reference's module exists here.

Neighbours are by raw inner product with self excluded; exact ties go to the smaller column index (the reference leaves
that order to torch's sort).  Importing this module does not touch the GPU.
"""
from __future__ import annotations

import torch

import umlh

BUILT_METRICS = ("mutual_knn", "cka")


def _not_built(what: str):
    raise NotImplementedError(f"{what} is not built here; supported: AlignmentMetrics.cka(kernel_metric='ip', unbiased=False), "
                              "AlignmentMetrics.mutual_knn, compute_nearest_neighbors; the other metrics are in "
                              "umlh.align.measure(metric, feats_A, feats_B, **kwargs)")


class AlignmentMetrics:

    SUPPORTED_METRICS = [
        "cycle_knn",
        "mutual_knn",
        "lcs_knn",
        "cka",
        "unbiased_cka",
        "cknna",
        "svcca",
        "edit_distance_knn",
    ]

    @staticmethod
    def measure(metric, *args, **kwargs):
        """metric is a string for the function (metrics.py:28-34)"""
        if metric not in AlignmentMetrics.SUPPORTED_METRICS:
            raise ValueError(f"Unrecognized metric: {metric}")
        return getattr(AlignmentMetrics, metric)(*args, **kwargs)

    @staticmethod
    def mutual_knn(feats_A, feats_B, topk):
        """Mean over rows of |knn_A(i) n knn_B(i)| / topk (metrics.py:55-84)."""
        return float(umlh.align.mutual_knn(feats_A, feats_B, topk).item())

    @staticmethod
    def cka(feats_A, feats_B, kernel_metric="ip", rbf_sigma=1.0, unbiased=False):
        """hsic_kl / (sqrt(hsic_kk * hsic_ll) + 1e-6) with the biased HSIC of the linear kernel (metrics.py:96-119)."""
        if kernel_metric == "rbf":
            _not_built("cka(kernel_metric='rbf')")
        if kernel_metric != "ip":
            raise ValueError(f"Invalid kernel metric {kernel_metric}")
        if unbiased:
            _not_built("cka(unbiased=True)")
        return float(umlh.align.cka(feats_A, feats_B).item())

    @staticmethod
    def unbiased_cka(*args, **kwargs):
        _not_built("unbiased_cka")

    @staticmethod
    def cycle_knn(*args, **kwargs):
        _not_built("cycle_knn")

    @staticmethod
    def lcs_knn(*args, **kwargs):
        _not_built("lcs_knn")

    @staticmethod
    def cknna(*args, **kwargs):
        _not_built("cknna")

    @staticmethod
    def svcca(*args, **kwargs):
        _not_built("svcca")

    @staticmethod
    def edit_distance_knn(*args, **kwargs):
        _not_built("edit_distance_knn")


def compute_nearest_neighbors(feats, topk=1):
    """The topk neighbours of each row by raw inner product, self excluded (metrics.py:272-285): int64 [N, topk] on the
    device, like the reference's argsort."""
    assert feats.ndim == 2, f"Expected feats to be 2D, got {feats.ndim}"
    return umlh.align.knn(feats, topk).long()


def compute_knn_accuracy(knn):
    """The share of rows i of ``knn`` [N, topk, topk] that contain i (metrics.py:258-269; what ``cycle_knn`` passes): a 0-d fp32
    device tensor, like the reference's ``.float()...mean()``.  For a 2-D ``knn`` [N, topk] the reference's comparison against
    ``arange(n).view(-1, 1, 1)`` broadcasts to [N, N, topk], so its value is the share of indices found ANYWHERE in the list; that
    is reproduced (``umlh.align.knn_accuracy(knn)`` is the per-row form for either shape)."""
    return umlh.align.knn_accuracy(knn, whole_table=knn.ndim == 2).to(torch.float32)


def remove_outliers(feats, q, exact=False, max_threshold=None):
    """``feats.clamp(-q_val, q_val)`` with ``q_val`` the mean over rows of the q-quantile of ``|feats|`` flattened from dim 1, or
    with ``exact`` the element ``int(q * feats.numel())`` of all sorted ``|feats|`` (metrics.py:327-341); an fp32 device tensor.
    ``q == 1`` returns ``feats`` itself.  An ``exact`` index outside the tensor raises ``ValueError`` (the reference: ``IndexError``).
    ``max_threshold`` is accepted and has no effect: the reference computes ``max(max_threshold, q_val)`` into a local and never
    uses it (:338-339), and this keeps that behaviour."""
    if q == 1:
        return feats
    return umlh.align.remove_outliers(feats, q, exact=exact, max_threshold=max_threshold)


# the callers' fixed arguments (vision_language/finetune.py:111-118, Gaussian_experiment/main.py:20-26)
def cka(feats_A, feats_B):
    kwargs = {"kernel_metric": "ip"}
    return AlignmentMetrics.measure("cka", feats_A, feats_B, **kwargs)


def mknn(feats_A, feats_B):
    kwargs = {"topk": 10}
    return AlignmentMetrics.measure("mutual_knn", feats_A, feats_B, **kwargs)
