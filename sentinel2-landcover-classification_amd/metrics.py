"""On-GPU segmentation metrics without a host sync per step.

The reference keeps four torchmetrics objects per mode (train_segmentation.py:53-63) and feeds them
`logits.argmax(dim=1)` and the labels every step (:145-159): MulticlassConfusionMatrix(ignore_index = 0 if
masked_loss, normalize="true"), JaccardIndex ("iou"), Accuracy, F1Score (multiclass, torchmetrics defaults; binary task
when num_classes == 2).  All four are functions of ONE integer histogram hist[true][pred] over all pixels; this class
accumulates that histogram on the device with the CONFUSION stage (int64, bit-exact) and derives the numbers at
`compute()` (epoch end), following torchmetrics' published definitions (third party, not installed here: the derived
formulas are restated, the histogram itself is exact by construction).

`DistanceBinnedMetrics` bins the same counts by the distance to the nearest label boundary.  `CalibrationMetrics` and
`fit_temperature` are the metrics that look at the probabilities instead of argmax: reliability, ECE, NLL and temperature scaling from
the integer sums of one launch over the scores (csrc/calibration.hip).
"""
from __future__ import annotations

import math

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


# ---- calibration: is the map's confidence worth anything? (csrc/calibration.hip) ----------------------------------------------------------
def calibration_from_sums(hist, totals, skipped: int = 0) -> dict:
    """The calibration figures of `CalibrationMetrics.compute`, in float64, from the integer sums of s2k_calibration alone
    (include/s2k.h): hist [K][bins][3] = {pixels, correct pixels, sum of rint(c * 2^20)} per predicted class and confidence bin,
    totals [2] = {pixels, sum of rint(nll * 2^20)}.  A bin holds floor(c * bins), the last one c = 1 as well.  Empty bins, classes
    and sums give 0."""
    h = torch.as_tensor(hist).to(torch.int64).cpu()
    K, bins = int(h.shape[0]), int(h.shape[1])
    tot = [int(v) for v in torch.as_tensor(totals).reshape(-1)[:2]]
    one = float(CM.CAL_ONE)

    def table(cells):
        """(rows, n, correct, ece, mce) of a [bins][3] table"""
        n = [int(v) for v in cells[:, 0]]
        ok = [int(v) for v in cells[:, 1]]
        cs = [int(v) for v in cells[:, 2]]
        N = sum(n)
        rows, ece, mce = [], 0.0, 0.0
        for b in range(bins):
            acc = ok[b] / n[b] if n[b] else 0.0
            conf = cs[b] / one / n[b] if n[b] else 0.0
            rows.append({"lo": b / bins, "hi": (b + 1) / bins, "count": n[b], "accuracy": acc, "confidence": conf})
            if n[b]:
                ece += n[b] / N * abs(acc - conf)
                mce = max(mce, abs(acc - conf))
        return rows, N, sum(ok), ece, mce

    rows, N, correct, ece, mce = table(h.sum(0))
    per_class = []
    for a in range(K):
        r, n, ok, e, m = table(h[a])
        per_class.append({"pixels": n, "accuracy": ok / n if n else 0.0, "ece": e, "mce": m, "reliability": r})
    coverage, kept, kept_ok = [], 0, 0
    for j in reversed(range(bins)):                     # the pixels with floor(c * bins) >= j: c >= j / bins
        kept += rows[j]["count"]
        kept_ok += int(h[:, j, 1].sum())
        coverage.append({"min_confidence": j / bins, "coverage": kept / N if N else 0.0, "accuracy": kept_ok / kept if kept else 0.0})
    coverage.reverse()
    return {"ece": ece, "mce": mce, "nll": tot[1] / one / tot[0] if tot[0] else 0.0, "accuracy": correct / N if N else 0.0, "pixels": N,
            "skipped": int(skipped), "reliability": rows, "per_class": per_class, "coverage": coverage}


class CalibrationMetrics:
    """Top-label calibration of a probability map against the labels: the reliability table (per confidence bin: pixels, accuracy, mean
    confidence), the expected and the maximum calibration error, the negative log-likelihood and the risk-coverage table behind a choice
    of `min_confidence`.  The reference trains with focal loss, label smoothing and class-weighted cross-entropy (src/losses.py), which
    shift a network's confidence away from its accuracy, and whole-tile blending shifts it again; its metrics are functions of argmax
    alone.  `update` is one launch over the scores (csrc/calibration.hip): integer sums on the device, bit-identical from run to run and
    independent of how the pixels are batched; `compute` derives everything from those sums on the host, in float64.

    ignore_index: a label class that is not counted (None: every class in [0, num_classes) is); labels outside [0, num_classes) never
    are.  temperature: logits are divided by it before the softmax; probabilities are taken as given.  A labelled pixel whose confidence
    is not in [0, 1] (NaN, or `kind="probs"` handed something else) is left out and counted in `skipped`."""

    def __init__(self, num_classes: int, bins: int = 15, ignore_index: int | None = 0, temperature: float = 1.0, device=None):
        self.C = CM.check_classes(num_classes)
        self.bins = CM.check_bins(bins)
        self.ignore_index = None if ignore_index is None else CM.check_ignore_index(ignore_index, self.C)
        self.temperature = CM.check_temperature(temperature)
        dev = device or "cuda"
        self.hist = torch.zeros(self.C, self.bins, 3, dtype=torch.int64, device=dev)
        self.totals = torch.zeros(1, 2, dtype=torch.int64, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int64, device=dev)

    @property
    def num_classes(self) -> int:
        return self.C

    @property
    def exclude(self) -> int:
        return 0 if self.ignore_index is None else 1 << self.ignore_index

    def reset(self) -> None:
        self.hist.zero_()
        self.totals.zero_()
        self.skipped.zero_()

    @torch.no_grad()
    def update(self, scores: torch.Tensor, labels: torch.Tensor, kind: str = "logits", label_lut=None) -> None:
        """scores: float32 [B, K, H, W] on the GPU, K = num_classes; labels: int64 or uint8 [B, H, W]; kind "logits" or "probs".
        label_lut (int32 [256], with uint8 labels): the class of a pixel is label_lut[label], read inside the kernel."""
        k = CM.check_kind(kind)
        if k == 0 and self.temperature != 1.0:
            raise ValueError("probabilities are taken as given: a temperature other than 1 needs kind='logits'")
        s = _check_scores_and_labels(scores, labels, self.C, label_lut)
        if not s.is_cuda or not labels.is_cuda:
            raise RuntimeError("CalibrationMetrics accumulates on the GPU (there is no CPU fallback)")
        if self.hist.device != s.device:
            self.hist, self.totals, self.skipped = self.hist.to(s.device), self.totals.to(s.device), self.skipped.to(s.device)
        CM.launch_calibration(s, k, [self.temperature if k else 1.0], self.bins, labels=labels.contiguous(), label_lut=label_lut,
                              exclude=self.exclude, hist=self.hist, totals=self.totals, skipped=self.skipped)

    def compute(self) -> dict:
        """{"ece", "mce", "nll", "accuracy" floats; "pixels", "skipped" ints; "reliability": one {"lo", "hi", "count", "accuracy",
        "confidence"} per bin; "per_class": for each PREDICTED class {"pixels", "accuracy", "ece", "mce", "reliability"}; "coverage": for
        each bin edge j / bins {"min_confidence", "coverage": the share of the counted pixels with a confidence at or above the edge,
        "accuracy": the accuracy among them}}.  ece = sum over the bins of n_b / N * |accuracy_b - confidence_b| (top label)."""
        return calibration_from_sums(self.hist.cpu(), self.totals.cpu()[0], int(self.skipped.cpu()[0]))


def _check_scores_and_labels(scores, labels, K: int, label_lut=None) -> torch.Tensor:
    s = CM.check_scores(scores)
    if scores.dim() != 4 or int(s.shape[1]) != K:
        raise ValueError(f"scores must be float32 [B, {K}, H, W]")
    if (not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int64, torch.uint8) or labels.dim() != 3
            or tuple(labels.shape) != (s.shape[0], s.shape[2], s.shape[3])):
        raise ValueError("labels must be an int64 or uint8 [B, H, W] tensor that matches scores")
    if label_lut is not None and (labels.dtype != torch.uint8 or not isinstance(label_lut, torch.Tensor) or label_lut.dtype != torch.int32
                                  or label_lut.numel() != 256):
        raise ValueError("label_lut must be an int32 [256] tensor and reads uint8 labels only")
    return s


def temperature_grid(lo: float, hi: float, n: int = CM.CAL_MAX_TEMPS) -> list:
    """n temperatures from lo to hi, evenly spaced in log T, both ends included"""
    a, b = math.log(lo), math.log(hi)
    return [lo] + [math.exp(a + (b - a) * i / (n - 1)) for i in range(1, n - 1)] + [hi]


def refine_temperature(evaluate, lo: float = 0.05, hi: float = 20.0, rounds: int = 6, return_step: bool = False):
    """Grid refinement in log T: each round hands `evaluate` the 8 temperatures of `temperature_grid(lo, hi)` and gets their 8 losses
    back (anything that orders: the integer NLL sums of one s2k_calibration launch), takes the point of least loss - the lowest index
    among equals - and makes its two neighbours (the point itself at an end of the grid) the next bracket.  Returns the last best
    point; return_step=True adds the spacing of the last grid in log T.  For a loss with one minimum in log T, as the NLL has (it is
    convex in 1 / T), the minimiser stays inside every bracket it was inside of.  A pure function of `evaluate`."""
    if isinstance(rounds, bool) or not isinstance(rounds, int) or rounds < 1:
        raise ValueError("rounds must be a positive integer")
    if not (isinstance(lo, (int, float)) and isinstance(hi, (int, float)) and math.isfinite(lo) and math.isfinite(hi) and 0 < lo < hi):
        raise ValueError("0 < lo < hi, both finite")
    lo, hi = float(lo), float(hi)
    best, step = lo, 0.0
    for _ in range(rounds):
        grid = temperature_grid(lo, hi)
        loss = list(evaluate(grid))
        if len(loss) != len(grid):
            raise ValueError("evaluate must return one loss per temperature")
        i = min(range(len(grid)), key=lambda j: (loss[j], j))
        best, step = grid[i], (math.log(hi) - math.log(lo)) / (len(grid) - 1)
        lo, hi = grid[max(i - 1, 0)], grid[min(i + 1, len(grid) - 1)]
    return (best, step) if return_step else best


@torch.no_grad()
def fit_temperature(logits, labels, num_classes: int, ignore_index: int | None = 0, lo: float = 0.05, hi: float = 20.0, rounds: int = 6,
                    label_lut=None) -> float:
    """The temperature T that minimises the negative log-likelihood of softmax(logits / T) against the labels (temperature scaling):
    `refine_temperature` over one s2k_calibration launch per round, which evaluates 8 temperatures in one pass over the logits.  The
    losses are integer sums, so the result repeats bit for bit.  logits: float32 [B, K, H, W] on the GPU; labels int64 or uint8
    [B, H, W]; `rounds` launches and as many host reads."""
    K = CM.check_classes(num_classes)
    exclude = 0 if ignore_index is None else 1 << CM.check_ignore_index(ignore_index, K)
    if not CM.check_temperature(lo) < CM.check_temperature(hi):
        raise ValueError("lo must be below hi")
    if isinstance(rounds, bool) or not isinstance(rounds, int) or rounds < 1:
        raise ValueError("rounds must be a positive integer")
    s = _check_scores_and_labels(logits, labels, K, label_lut)
    if not s.is_cuda or not labels.is_cuda:
        raise RuntimeError("fit_temperature runs on the GPU (there is no CPU fallback)")
    labels = labels.contiguous()
    totals = torch.zeros(CM.CAL_MAX_TEMPS, 2, dtype=torch.int64, device=s.device)

    def evaluate(temps):
        totals.zero_()
        CM.launch_calibration(s, 1, temps, labels=labels, label_lut=label_lut, exclude=exclude, totals=totals)
        return [int(v) for v in totals[:, 1].cpu()]

    return refine_temperature(evaluate, lo, hi, rounds)
