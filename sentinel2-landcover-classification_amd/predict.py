"""Whole-tile prediction: sliding-window inference over the resident tiles of a `GpuTilePipeline`, blended on the GPU.

The reference stops at per-crop logits (`predict_step`, src/train_segmentation.py:106; src/experiments/inference_demo.py), and its
validation numbers come from the centre crop.  A land-cover user asks for the class map of a whole 512 x 512 Sentinel-2 tile; Prithvi
has fixed position tables and only ever sees S x S = 224 x 224, so the tile is predicted as overlapping windows whose logits are
combined.  Everything around that step exists already - TILE_PREP cuts windows from explicit {tile, y0, x0, flips} params in one
launch, `metrics.SegMetrics` defines the metrics - and the step itself is one stage, WINDOW_BLEND (plan/opdefs.py, csrc/predict.hip):
a gather with a fixed summation order, so a prediction is bit-identical from run to run and independent of `windows_per_batch`.

    predictor = TilePredictor(model, pipe, num_classes=4)               # stride S // 2, Hann profile, softmax blended
    class_map = predictor.predict([3, 17])                              # int64 [2, H, W] on the device
    predictor.evaluate(metrics)                                         # whole-tile confusion counts into metrics.hist
    metrics.compute()                                                   # whole-tile IoU / accuracy / F1
    class_map = predictor.predict([3, 17], majority=5)                  # after the 5 x 5 majority filter (classmap.py); so evaluate, render
    class_map = predictor.predict([3, 17], majority=5, min_area=16)     # then without its patches below 16 pixels (classmap.sieve)
    predictor.evaluate_by_distance(binned)                              # confusion counts by distance to the label boundaries (metrics.DistanceBinnedMetrics)
    class_map, conf = predictor.predict_with_confidence([3, 17], min_confidence=0.6)     # the confidence raster; unsure pixels become class 0
    predictor.evaluate_calibration(cal)                                 # reliability, ECE and NLL of the blend (metrics.CalibrationMetrics)
"""
from __future__ import annotations

import math

import torch

from . import classmap as CM
from . import zonal as ZN
from .data import quicklook as QL
from .render import overlay
from .stage_call import StageCall

MAX_CLASSES = 32                 # WINDOW_BLEND keeps a pixel quad's K sums in registers
MAX_LOGITS = (1 << 31) - 1       # elements of one LOGITS buffer (the stage's bound)


def window_origins(size: int, S: int, stride: int) -> list[int]:
    """Origins of the S-wide windows that cover [0, size): 0, stride, 2 * stride, ... and a final size - S where the run does not end
    there.  Ascending and unique; stride <= S, so consecutive windows leave no gap."""
    size, S, stride = int(size), int(S), int(stride)
    if S < 1 or S > size:
        raise ValueError("the window must fit the tile (1 <= S <= size)")
    if not 1 <= stride <= S:
        raise ValueError("stride must be in 1..S (a larger one leaves pixels uncovered)")
    out = list(range(0, size - S + 1, stride))
    if out[-1] != size - S:
        out.append(size - S)
    return out


def check_origins(origins, size: int, S: int) -> None:
    """What WINDOW_BLEND assumes of YS / XS and does not check on the device: ascending, unique, first 0, last size - S, gaps <= S."""
    o = [int(v) for v in origins]
    if not o or o[0] != 0 or o[-1] != size - S or any(b <= a or b - a > S for a, b in zip(o[:-1], o[1:])):
        raise ValueError("window origins must ascend from 0 to size - S in steps of 1..S")


def window_profile(S: int, kind: str = "hann") -> torch.Tensor:
    """float32 [S], strictly positive and symmetric: the 1-D blending profile; a window pixel (a, b) weighs profile[a] * profile[b].
    "hann": sin^2(pi (i + 1/2) / S) - the half-sample shift keeps the ends above zero; "uniform": ones."""
    S = int(S)
    if S < 1:
        raise ValueError("S must be positive")
    if kind == "uniform":
        return torch.ones(S, dtype=torch.float32)
    if kind != "hann":
        raise ValueError("window must be 'hann' or 'uniform'")
    half = [math.sin(math.pi * (i + 0.5) / S) ** 2 for i in range((S + 1) // 2)]
    return torch.tensor(half + half[:S // 2][::-1], dtype=torch.float64).to(torch.float32)      # mirrored: symmetric bit for bit


def add_window_blend(call: StageCall, logits, ys, xs, flips, w1, mode: int, H: int, W: int, nsrc: int, blend=None, mask=None,
                     labels=None, index=None, lut=None, hist=None) -> None:
    """Append the WINDOW_BLEND record over `logits` [M, F, NY, NX, K, S, S] into BLEND [M, K, H, W] and / or MASK [M, H, W]; with `hist`
    ([K, K] int64) the confusion counts against `lut[labels[index]]`.  YS, XS, FLIPS and INDEX are host values: they travel in the call's
    one upload."""
    M, F, NY, NX, K, S = logits.shape[:6]
    call.add("WINDOW_BLEND", LOGITS=call.t(logits), YS=call.const(ys, "i32"), XS=call.const(xs, "i32"), FLIPS=call.const(flips, "i32"),
             W1=call.t(w1), BLEND=call.t(blend, (M, K, H, W)), MASK=call.t(mask, (M, H, W)),
             LABELS=call.t(labels if hist is not None else None), INDEX=call.const(index, "i32") if hist is not None else None,
             LUT=call.t(lut if hist is not None else None), HIST=call.t(hist, (K, K)),
             M=M, F=F, NY=NY, NX=NX, K=K, H=H, W=W, S=S, NSRC=nsrc, MODE=mode)


class TilePredictor:
    """model: any callable from the pipeline's batch `x` ([B, C, S, S], or [B, C, 1, S, S] unless the pipeline squeezes the time
    dimension) to float32 logits [B, num_classes, S, S]; an `nn.Module` is run in eval mode.  blend="probs" averages the windows'
    softmax, "logits" their raw values; `flips` are the test-time flip variants (bit 0 horizontal, bit 1 vertical), each window is
    predicted under every one of them and un-flipped by the stage.  `tiles_per_launch` tiles share one LOGITS buffer and one
    WINDOW_BLEND launch (default: as many as keep the buffer below 2 GiB, at most 8)."""

    def __init__(self, model, pipeline, num_classes: int, stride: int | None = None, window: str = "hann", blend: str = "probs",
                 flips=(0,), windows_per_batch: int = 32, tiles_per_launch: int | None = None):
        self.model, self.pipe, self.K, self.S = model, pipeline, int(num_classes), int(pipeline.S)
        self.stride = self.S // 2 if stride is None else int(stride)
        self.flips = [int(f) for f in flips]
        self.wpb = int(windows_per_batch)
        self.tpl = None if tiles_per_launch is None else int(tiles_per_launch)
        if not 1 <= self.K <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in 1..{MAX_CLASSES}")
        if not 1 <= self.stride <= self.S:
            raise ValueError("stride must be in 1..random_crop_size")
        if blend not in ("probs", "logits"):
            raise ValueError("blend must be 'probs' or 'logits'")
        if not 1 <= len(self.flips) <= 4 or len(set(self.flips)) != len(self.flips) or any(not 0 <= f <= 3 for f in self.flips):
            raise ValueError("flips: 1..4 different values out of 0..3")
        if self.wpb < 1 or (self.tpl is not None and self.tpl < 1):
            raise ValueError("windows_per_batch and tiles_per_launch must be positive")
        self.mode = 1 if blend == "probs" else 0
        self.profile = window_profile(self.S, window)

    # ---- public surface ------------------------------------------------------------------------------------------------------
    def predict(self, indices=None, majority: int | None = None, iterations: int = 1, min_area: int | None = None,
                connectivity: int = 4) -> torch.Tensor:
        """int64 [M, H, W] on the device: the class of every pixel of the selected tiles (None = every resident tile).  majority=k:
        after `iterations` passes of the k x k majority filter (`classmap.majority_filter`: every class votes, none is fixed).
        min_area=a: after one pass of the minimum-area sieve (`classmap.sieve(map, K, a, connectivity)`: the donor rule, no class
        fixed), which runs after the majority filter when both are given."""
        size, its, area, conn = self._post(majority, iterations, min_area, connectivity)
        out = self._run(indices, want="mask")
        if size is not None:
            out = CM.run_majority(out, self.K, size, its, CM.class_bits(None, self.K, "votes"), 0)
        if area is not None:
            out = CM.run_sieve(out, self.K, area, conn, 1, 0, -1)
        return out

    def predict_blend(self, indices=None) -> torch.Tensor:
        """float32 [M, K, H, W] on the device: the blended probabilities (blend="probs") or logits."""
        return self._run(indices, want="blend")

    def evaluate(self, metrics, indices=None, majority: int | None = None, iterations: int = 1, min_area: int | None = None,
                 connectivity: int = 4) -> None:
        """Add the whole-tile confusion counts of the selected tiles - hist[true][predicted] against the pipeline's resident labels
        after its label map - into `metrics.hist` (a `metrics.SegMetrics`), inside the blending launch itself.  majority=k: the counts
        of the map after `iterations` passes of the k x k majority filter, added by the last filter launch (no separate CONFUSION
        pass, no int64 label tensor).  min_area=a: the counts of the map after the sieve (after the majority filter, if given), added
        by the sieve's relabel launch in the same way."""
        if int(metrics.C) != self.K:
            raise ValueError("metrics.num_classes differs from the predictor's")
        size, its, area, conn = self._post(majority, iterations, min_area, connectivity)
        if size is None and area is None:
            self._run(indices, want="hist", metrics=metrics)
            return
        pipe = self.pipe
        if pipe.raw is None:
            raise RuntimeError("call load() first")
        idx = pipe._stats_index(indices, need_labels=True)               # ValueError first, then the refusal to run off the GPU
        mask = self._run(idx, want="mask")
        if metrics.hist.device != pipe.device:
            metrics.hist = metrics.hist.to(pipe.device)
        last = (pipe.labels, idx.to(pipe.device), pipe.lut, metrics.hist)
        if size is not None:
            mask = CM.run_majority(mask, self.K, size, its, CM.class_bits(None, self.K, "votes"), 0, last=None if area is not None else last)
        if area is not None:
            CM.run_sieve(mask, self.K, area, conn, 1, 0, -1, last=last)

    @torch.no_grad()
    def evaluate_by_distance(self, binned, indices=None, majority: int | None = None, iterations: int = 1, min_area: int | None = None,
                             connectivity: int = 4) -> None:
        """Add the confusion counts of the selected tiles, binned by the distance of every pixel to the nearest class boundary of the
        pipeline's resident labels, into `binned.hist` (a `metrics.DistanceBinnedMetrics`).  The class maps are those of
        `predict(indices, majority, iterations, min_area, connectivity)`; the labels are the gathered uint8 labels read through the
        pipeline's label table inside the kernel (no int64 label tensor is built), and the counts come from the launch that computes
        the distances.  The boundaries follow `binned.connectivity`; `connectivity` is the sieve's."""
        if int(binned.num_classes) != self.K:
            raise ValueError("binned.num_classes differs from the predictor's")
        size, its, area, conn = self._post(majority, iterations, min_area, connectivity)
        pipe = self.pipe
        if pipe.raw is None:
            raise RuntimeError("call load() first")
        idx = pipe._stats_index(indices, need_labels=True)               # ValueError first, then the refusal to run off the GPU
        mask = self._run(idx, want="mask")
        if size is not None:
            mask = CM.run_majority(mask, self.K, size, its, CM.class_bits(None, self.K, "votes"), 0)
        if area is not None:
            mask = CM.run_sieve(mask, self.K, area, conn, 1, 0, -1)
        if binned.hist.device != pipe.device:
            binned.hist = binned.hist.to(pipe.device)
        labels = pipe.labels.index_select(0, idx.to(pipe.device))
        CM.count_by_distance(labels, mask, self.K, binned.connectivity, binned.exclude, binned.thresholds, binned.hist, src_lut=pipe.lut)

    def predict_with_confidence(self, indices=None, measure: str = "max", min_confidence=None, reject_to: int = 0):
        """(class_map int64 [M, H, W], conf float32 [M, H, W]) on the device, from `predict_blend(indices)` in one more launch
        (`classmap.confidence`): the confidence is the largest blended probability (measure="max") or its lead over the runner-up
        ("margin"); with blend="logits" the softmax of the blended logits is taken first.  min_confidence=c puts every pixel whose
        confidence is below c into class `reject_to`.  Without it the class map is `predict(indices)` bit for bit: both take the first
        maximum of the same stored values."""
        CM.check_measure(measure)
        return CM.confidence(self.predict_blend(indices), "probs" if self.mode == 1 else "logits", measure, 1.0, min_confidence, reject_to)

    @torch.no_grad()
    def predict_zones(self, zones, num_zones: int, indices=None, votes=None, min_count: int = 1, paint: bool = False,
                      majority: int | None = None, iterations: int = 1, min_area: int | None = None, connectivity: int = 4):
        """Object-based classification of the selected tiles: (zone_class int32 [num_zones], hist int64 [num_zones, num_classes]) on
        the device - `zonal.histogram` of `predict(indices, majority, iterations, min_area, connectivity)` inside every zone of `zones`
        (int32 or int64 [M, H, W], one raster per selected tile, global ids, negative = no zone) and its `zonal.majority(hist, votes,
        min_count)`: the lowest class with the most predicted pixels, -1 for a zone with fewer than `min_count` of them.  paint=True
        adds int64 [M, H, W]: the predicted maps with every classified zone painted in its class, all other pixels as predicted."""
        Z, _ = ZN._check_num_zones(num_zones, 1, False)
        vb = CM.class_bits(votes, self.K, "votes")
        if vb == 0:
            raise ValueError("votes must name at least one class")
        n = ZN._check_count(min_count)
        self._post(majority, iterations, min_area, connectivity)
        pipe = self.pipe
        if pipe.raw is None:
            raise RuntimeError("call load() first")
        z = ZN._check_zones(zones)
        M = pipe.raw.shape[0] if indices is None else torch.as_tensor(indices).numel()
        if zones.dim() != 3 or tuple(z.shape) != (M,) + tuple(pipe.raw.shape[2:]):
            raise ValueError("zones must be [M, H, W]: one raster of the tiles' size per selected tile")
        idx = pipe._stats_index(indices, need_labels=False)              # ValueError first, then the refusal to run off the GPU
        ZN._need_gpu(z)
        mask = self.predict(idx, majority, iterations, min_area, connectivity)
        hist = torch.zeros(Z, self.K, dtype=torch.int64, device=mask.device)
        cls = torch.empty(Z, dtype=torch.int32, device=mask.device)
        status = CM.new_status(mask.device)
        ZN.launch_histogram(z, 0, mask, Z, self.K, hist, status)
        ZN.launch_majority(hist, Z, self.K, vb, n, -1, cls)
        if paint:
            ZN.launch_paint(z, 0, cls, Z, mask, ZN.KEEP, 0, status)
        ZN.raise_status(status)
        return (cls, hist, mask) if paint else (cls, hist)

    @torch.no_grad()
    def evaluate_calibration(self, cal, indices=None) -> None:
        """Add the calibration sums of the selected tiles' blend - `predict_blend(indices)`, as probabilities (blend="probs") or logits
        under `cal.temperature` - against the pipeline's resident labels into `cal` (a `metrics.CalibrationMetrics`).  The labels are
        the gathered uint8 labels read through the pipeline's label table inside the kernel: no int64 label tensor is built."""
        if int(cal.num_classes) != self.K:
            raise ValueError("cal.num_classes differs from the predictor's")
        pipe = self.pipe
        if pipe.raw is None:
            raise RuntimeError("call load() first")
        idx = pipe._stats_index(indices, need_labels=True)               # ValueError first, then the refusal to run off the GPU
        blend = self._run(idx, want="blend")
        cal.update(blend, pipe.labels.index_select(0, idx.to(pipe.device)), "probs" if self.mode == 1 else "logits", label_lut=pipe.lut)

    def render(self, indices, palette, alpha: float = 0.5, majority: int | None = None, iterations: int = 1, min_area: int | None = None,
               connectivity: int = 4) -> torch.Tensor:
        """uint8 [M, H, W, 3] on the device: the whole-tile quicklook of the selected tiles (`GpuTilePipeline.quicklook`, its default
        bands and percentile) with the predicted class map (`predict(indices, majority, iterations, min_area, connectivity)`) laid
        over it in the colours of `palette` (uint8 [>= num_classes, 3]) at opacity `alpha` (`render.overlay`)."""
        self._post(majority, iterations, min_area, connectivity)
        pal = QL.check_palette(palette)
        QL.alpha_code(alpha)
        if pal.shape[0] < self.K:
            raise ValueError("palette needs one colour per class")
        picture = self.pipe.quicklook(indices, whole_tile=True)          # ValueError first, then the refusal to run off the GPU
        return overlay(picture, self.predict(indices, majority, iterations, min_area, connectivity), pal, alpha)

    # ---- implementation ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _post(majority, iterations, min_area, connectivity):
        """(size, iterations, min_area, connectivity) of the map filters, validated; size / min_area None where not asked for"""
        size = its = area = conn = None
        if majority is not None:
            size, its = CM.check_size(majority), CM.check_iterations(iterations)
        if min_area is not None:
            area, conn = CM.check_min_area(min_area), CM.check_connectivity(connectivity)
        return size, its, area, conn

    def _geometry(self):
        H, W = (int(v) for v in self.pipe.raw.shape[2:])
        ys, xs = window_origins(H, self.S, self.stride), window_origins(W, self.S, self.stride)
        check_origins(ys, H, self.S)
        check_origins(xs, W, self.S)
        per_tile = len(self.flips) * len(ys) * len(xs) * self.K * self.S * self.S
        if per_tile > MAX_LOGITS:
            raise ValueError("one tile's window logits exceed 2^31 - 1 elements: raise the stride or drop flip variants")
        tpl = max(1, min(8, MAX_LOGITS // per_tile)) if self.tpl is None else self.tpl
        if tpl * per_tile > MAX_LOGITS:
            raise ValueError(f"tiles_per_launch = {tpl} needs a LOGITS buffer beyond 2^31 - 1 elements")
        return H, W, ys, xs, tpl

    @torch.no_grad()
    def _run(self, indices, want: str, metrics=None):
        pipe = self.pipe
        if pipe.raw is None:
            raise RuntimeError("call load() first")
        H, W, ys, xs, tpl = self._geometry()
        idx = pipe._stats_index(indices, need_labels=want == "hist")       # ValueError first, then the refusal to run off the GPU
        dev, K, S, F, NY, NX = pipe.device, self.K, self.S, len(self.flips), len(ys), len(xs)
        M = idx.numel()
        blend = torch.empty(M, K, H, W, dtype=torch.float32, device=dev) if want == "blend" else None
        mask = torch.empty(M, H, W, dtype=torch.int64, device=dev) if want == "mask" else None
        hist = None
        if want == "hist":
            if metrics.hist.device != dev:
                metrics.hist = metrics.hist.to(dev)
            hist = metrics.hist
        w1 = self.profile.to(dev)
        was_training = isinstance(self.model, torch.nn.Module) and self.model.training
        if was_training:
            self.model.eval()
        try:
            for g0 in range(0, M, tpl):
                tiles = idx[g0:g0 + tpl]
                Mg = tiles.numel()
                # {tile, y0, x0, flips} of every window in LOGITS order [Mg][F][NY][NX]
                par = torch.empty(Mg, F, NY, NX, 4, dtype=torch.int32)
                par[..., 0] = tiles.view(Mg, 1, 1, 1)
                par[..., 1] = torch.tensor(ys, dtype=torch.int32).view(1, 1, NY, 1)
                par[..., 2] = torch.tensor(xs, dtype=torch.int32).view(1, 1, 1, NX)
                par[..., 3] = torch.tensor(self.flips, dtype=torch.int32).view(1, F, 1, 1)
                par = par.view(-1, 4)
                n = par.shape[0]
                logits = torch.empty(n, K, S, S, dtype=torch.float32, device=dev)
                for b0 in range(0, n, self.wpb):
                    out = self.model(pipe(params=par[b0:b0 + self.wpb]).x)
                    b = min(self.wpb, n - b0)
                    if tuple(out.shape) != (b, K, S, S) or out.dtype != torch.float32:
                        raise ValueError(f"the model must return float32 [B, {K}, {S}, {S}] logits, got {out.dtype} {tuple(out.shape)}")
                    logits[b0:b0 + b].copy_(out)
                self._blend(logits, tiles, ys, xs, w1, H, W,
                            None if blend is None else blend[g0:g0 + Mg], None if mask is None else mask[g0:g0 + Mg], hist)
        finally:
            if was_training:
                self.model.train()
        return blend if want == "blend" else mask

    def _blend(self, logits, tiles, ys, xs, w1, H, W, blend, mask, hist) -> None:
        """one WINDOW_BLEND over a group's LOGITS buffer"""
        pipe, call = self.pipe, StageCall()
        add_window_blend(call, logits.view(tiles.numel(), len(self.flips), len(ys), len(xs), self.K, self.S, self.S), ys, xs, self.flips, w1,
                         self.mode, H, W, pipe.raw.shape[0], blend, mask, pipe.labels, tiles, pipe.lut, hist)
        call.run()
