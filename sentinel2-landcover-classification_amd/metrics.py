"""On-GPU segmentation metrics without a host sync per step.

The reference keeps four torchmetrics objects per mode (train_segmentation.py:53-63) and feeds them
`logits.argmax(dim=1)` and the labels every step (:145-159): MulticlassConfusionMatrix(ignore_index = 0 if
masked_loss, normalize="true"), JaccardIndex ("iou"), Accuracy, F1Score (multiclass, torchmetrics defaults; binary task
when num_classes == 2).  All four are functions of ONE integer histogram hist[true][pred] over all pixels; this class
accumulates that histogram on the device with the CONFUSION stage (int64, bit-exact) and derives the numbers at
`compute()` (epoch end), following torchmetrics' published definitions (third party, not installed here: the derived
formulas are restated, the histogram itself is exact by construction).
"""
from __future__ import annotations

import torch

from . import classmap as CM
from .stage_call import StageCall, cached

_CALLS = {}      # the packed CONFUSION calls of this process (stage_call.cached)


class SegMetrics:
    def __init__(self, num_classes: int, ignore_index: int | None = 0, device=None):
        self.C, self.ignore_index = int(num_classes), ignore_index
        self.hist = torch.zeros(self.C * self.C, dtype=torch.int64, device=device or "cuda")

    def reset(self) -> None:
        self.hist.zero_()

    @torch.no_grad()
    def update(self, predictions: torch.Tensor, labels: torch.Tensor) -> None:
        """predictions: int64 class ids (e.g. `class_mask(logits)`), labels: int64, same shape."""
        if not predictions.is_cuda:
            raise RuntimeError("SegMetrics accumulates on the GPU (there is no CPU fallback)")
        if predictions.shape != labels.shape or predictions.dtype != torch.int64 or labels.dtype != torch.int64:
            raise ValueError("predictions and labels must be int64 tensors of the same shape")
        if self.hist.device != predictions.device:
            self.hist = self.hist.to(predictions.device)
        predictions, labels = predictions.contiguous(), labels.contiguous()
        cached(_CALLS, confusion_call, predictions, labels, self.hist, C=self.C).run()

    def compute(self) -> dict:
        """{"confusion_matrix" [C,C] rows normalised over the true class, "iou", "accuracy", "f1"} as CPU tensors."""
        return metrics_from_hist(self.hist.view(self.C, self.C).cpu(), self.ignore_index)


def confusion_call(predictions, labels, hist, C: int) -> StageCall:
    n = predictions.numel()
    call = StageCall()
    call.add("CONFUSION", PRED=call.t(predictions, (n,)), LABELS=call.t(labels, (n,)), HIST=call.t(hist), COUNT=n, C=C)
    return call


def metrics_from_hist(h: torch.Tensor, ignore_index: int | None) -> dict:
    """h[t][p] int64 counts over ALL pixels.  Definitions (torchmetrics):
    confusion matrix: samples whose target == ignore_index removed, rows divided by their sums (0 where empty);
    multiclass IoU: macro mean of TP / (TP + FP + FN) over the classes that occur in target or prediction;
    multiclass accuracy and F1: micro (= sum TP / N); binary task (C == 2): statistics of the positive class 1."""
    C = h.shape[0]
    hd = h.double()
    cm = hd.clone()
    if ignore_index is not None and 0 <= ignore_index < C:
        cm[ignore_index, :] = 0
    rows = cm.sum(1, keepdim=True)
    cmn = torch.where(rows > 0, cm / rows.clamp(min=1), torch.zeros_like(cm))
    tp = hd.diag()
    fp = hd.sum(0) - tp
    fn = hd.sum(1) - tp
    n = hd.sum()
    if C == 2:
        tn = hd[0, 0]
        iou = tp[1] / (tp[1] + fp[1] + fn[1]) if (tp[1] + fp[1] + fn[1]) > 0 else torch.tensor(0.0, dtype=torch.float64)
        acc = (tp[1] + tn) / n if n > 0 else torch.tensor(0.0, dtype=torch.float64)
        f1 = 2 * tp[1] / (2 * tp[1] + fp[1] + fn[1]) if (2 * tp[1] + fp[1] + fn[1]) > 0 else torch.tensor(0.0, dtype=torch.float64)
    else:
        union = tp + fp + fn
        present = union > 0
        per = torch.where(present, tp / union.clamp(min=1), torch.zeros_like(tp))
        iou = per[present].mean() if present.any() else torch.tensor(0.0, dtype=torch.float64)
        acc = tp.sum() / n if n > 0 else torch.tensor(0.0, dtype=torch.float64)
        f1 = acc
    return {"confusion_matrix": cmn.float(), "iou": iou.float(), "accuracy": acc.float(), "f1": f1.float()}


class DistanceBinnedMetrics:
    """Confusion counts binned by the distance of a pixel to the nearest class boundary of the LABELS: do the errors sit where two
    classes meet (where rasterised polygons are wrong by a pixel or so), or inside the regions?  `edges` are distances in pixels
    (1 to 8, finite, >= 0); a pixel of Euclidean distance d to the nearest boundary pixel falls into bin b = the number of edges with
    d > edge, i.e. bin 0 holds d <= edges[0] and the last bin d > edges[-1] - and every pixel of a tile without any boundary.  The
    comparison is made on squared distances, `dist2 > floor(edge^2)`, which is the same thing for integer dist2; the converted edges
    must ascend strictly.  The boundaries are those of `classmap.distance_transform(labels, K, "boundary", connectivity,
    exclude=(ignore_index,))`; the counts themselves ignore nothing (the CONFUSION convention: `ignore_index` acts in `compute()`), so
    `total()` is exactly what `SegMetrics` accumulates over the same pairs.  The counts come from the launch that computes the
    distances (csrc/distance.hip): exact integer sums, no separate CONFUSION pass."""

    def __init__(self, num_classes: int, edges=(1, 2, 4, 8), ignore_index: int | None = 0, connectivity: int = 4, device=None):
        self.C = CM.check_classes(num_classes)
        self.thresholds = CM.check_edges(edges)
        self.edges = [float(e) for e in edges]
        self.connectivity = CM.check_connectivity(connectivity)
        self.ignore_index = None if ignore_index is None else CM.check_ignore_index(ignore_index, self.C)
        self.hist = torch.zeros(len(self.thresholds) + 1, self.C, self.C, dtype=torch.int64, device=device or "cuda")

    @property
    def num_classes(self) -> int:
        return self.C

    @property
    def exclude(self) -> int:
        return 0 if self.ignore_index is None else 1 << self.ignore_index

    def reset(self) -> None:
        self.hist.zero_()

    @torch.no_grad()
    def update(self, predictions: torch.Tensor, labels: torch.Tensor) -> None:
        """predictions, labels: int64 [B, H, W] class ids on the GPU; `hist` is added to."""
        if (not isinstance(predictions, torch.Tensor) or not isinstance(labels, torch.Tensor) or predictions.shape != labels.shape
                or predictions.dtype != torch.int64 or labels.dtype != torch.int64 or labels.dim() != 3 or labels.numel() == 0):
            raise ValueError("predictions and labels must be int64 [B, H, W] tensors of the same shape")
        if labels.shape[1] > CM.EDT_MAX_DIM or labels.shape[2] > CM.EDT_MAX_DIM:
            raise ValueError(f"the distance transform takes maps of at most {CM.EDT_MAX_DIM} x {CM.EDT_MAX_DIM}")
        if not predictions.is_cuda or not labels.is_cuda:
            raise RuntimeError("DistanceBinnedMetrics accumulates on the GPU (there is no CPU fallback)")
        if self.hist.device != labels.device:
            self.hist = self.hist.to(labels.device)
        CM.count_by_distance(labels.contiguous(), predictions.contiguous(), self.C, self.connectivity, self.exclude, self.thresholds, self.hist)

    def total(self) -> torch.Tensor:
        """int64 [C, C] on the device: the counts of all bins together - `SegMetrics.hist` over the same pairs"""
        return self.hist.sum(0)

    def compute(self) -> list:
        """one dict per bin: {"lo", "hi": the bin's bounds in pixels (lo < d <= hi; the first lo is 0 and inclusive, the last hi inf),
        "pixels": the counted pairs, and the entries of `metrics_from_hist` over the bin's counts}"""
        h = self.hist.cpu()
        lo = [0.0] + self.edges
        hi = self.edges + [float("inf")]
        return [{"lo": lo[b], "hi": hi[b], "pixels": int(h[b].sum()), **metrics_from_hist(h[b], self.ignore_index)} for b in range(h.shape[0])]
