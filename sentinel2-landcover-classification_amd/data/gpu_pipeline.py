"""GPU-side input pipeline: the per-sample transform chain of the reference's loaders as ONE stage.

What it replaces (all on the CPU, per sample, one DataLoader worker in the reference's configs):
  * `S2OSMDataset.__getitem__` (src/data/s2osm_dataset.py:51-71): CNES label remap with `np.vectorize`
    (src/configs/cnes_labell_mappings.py:78-95), `c h w -> h w c` and back, `.float()`, `.long()`, `unsqueeze(1)` unless
    `squeeze_time_dim`;
  * the albumentations `Compose` of `S2OSMDatamodule.setup` (src/data/s2osm_datamodule.py:75-87) and `MAEDatamodule.setup`
    (src/data/mae_datamodule.py:60-73): RandomCrop | CenterCrop -> HorizontalFlip(p) -> VerticalFlip(p) -> Normalize(mean, std)
    (albumentations' Normalize scales mean and std by max_pixel_value = 255 — the reference passes the defaults).
Decoding the GeoTIFFs (rasterio) stays on the host: the decoded int16 tiles (12.4 k tiles x 6 x 512 x 512 x 2 B = 39 GB for
the reference's largest area) are uploaded once and stay resident in HBM; every step then costs one TILE_PREP launch.

Randomness: albumentations draws from Python's `random`; here crop offsets and flips are drawn from a `torch.Generator`
on the host with the same formulas (`int((H - S + 1) * u)`, `u < p`) and passed to the stage, like every other random
draw of this library (drop-connect, MAE masking).  Given the same draws the output is bit-identical to the reference's.

Dataset statistics: the three passes the reference makes over the whole dataset on the CPU before a run starts read only what is
resident here, so each is one streaming read on the GPU (stages TILE_MOMENTS / TILE_LABEL_HIST, host derivations in
data/dataset_stats.py): `band_mean_std` (calculate_mean_std -> the `mean`, `std` of this class), `class_probabilities`
(get_class_probabilities -> `EfficientNetConfig.class_distribution`, `losses.get_loss`) and `sample_weights` + `weighted_indices`
(get_sample_weights + WeightedRandomSampler -> the tile indices given to `draw_params`).

Quicklooks: `quicklook` is the reference's percentile-stretched picture of a crop (src/plotting.py:75-96), `band_percentiles` the
exact order statistics behind it (per tile, or per band over the dataset) and `zero_fraction` the per-tile nodata share of
src/experiments/sentinel_EDA.py - a radix select over the resident tiles, no sort and no host copy (data/quicklook.py).
"""
from __future__ import annotations

import typing

import numpy as np
import torch

from .. import classmap as CM
from .. import zonal as ZN
from ..plan import opdefs as D
from . import dataset_stats as DS
from . import quicklook as QL
from ..stage_call import StageCall, cached

# CNES land-cover classes 1..23 grouped as in src/configs/cnes_labell_mappings.py:47-75 (class 0 = outside France)
_CNES_GROUP = {**{k: "impervious_surface" for k in (1, 2, 3, 4)},
               **{k: "agriculture" for k in (5, 6, 7, 8, 9, 10, 11, 12, 14, 15)},
               **{k: "nature" for k in (13, 16, 17, 18, 19, 20, 21, 22, 23)}}
CNES_LABEL_MAPS = {   # key order = class index (cnes_labell_mappings.py:42-45)
    "cnes-multiclass": ["other", "agriculture", "nature", "impervious_surface"],
    "cnes-impervious-binary": ["other", "impervious_surface"],
    "cnes-nature-binary": ["other", "nature"],
    "cnes-agriculture-binary": ["other", "agriculture"],
}


def label_lut(label_map_name: str) -> torch.Tensor:
    """256-entry int32 table equal to `get_cnes_transform(label_map_name, ...)` applied to every uint8 value
    (cnes_labell_mappings.py:78-95): identity unless the map is a simplified CNES one; there, label 0, labels without a
    group and groups missing from the map go to 0, the rest to the group's position in the map."""
    lut = torch.arange(256, dtype=torch.int32)
    if "cnes" in label_map_name and label_map_name != "cnes-full":
        keys = CNES_LABEL_MAPS[label_map_name]
        for v in range(256):
            g = _CNES_GROUP.get(v, "_")
            lut[v] = 0 if (v == 0 or g not in keys) else keys.index(g)
    return lut


_CALLS = {}      # the packed TILE_PREP calls of this process (stage_call.cached)


class S2OSMSample(typing.NamedTuple):
    x: torch.Tensor
    y: torch.Tensor


def tile_prep_call(raw, labels, par, norm, lut, x, y) -> StageCall:
    """TILE_PREP of the crops `par` (int32 [B, 4] on the device) of `raw` into `x` [B, C, S, S]; `y` None: no labels, no LUT"""
    N, C, H, W = raw.shape
    call = StageCall()
    call.add("TILE_PREP", RAW=call.t(raw), LABELS=call.t(labels if y is not None else None), PARAMS=call.t(par), NORM=call.t(norm),
             LUT=call.t(lut if y is not None else None), X=call.t(x), Y=call.t(y), B=x.shape[0], C=C, H=H, W=W, S=x.shape[2], NSRC=N)
    return call


class GpuTilePipeline:
    def __init__(self, mean, std, random_crop_size: int = 224, augment: bool = False, random_horizontal_flip_p: float = 0.0,
                 random_vertical_flip_p: float = 0.0, label_map: str = "osm-multiclass", squeeze_time_dim: bool = False,
                 n_time_frames: int = 1, max_pixel_value: float = 255.0, device="cuda"):
        self.S, self.augment = int(random_crop_size), bool(augment)
        self.hp, self.vp = float(random_horizontal_flip_p), float(random_vertical_flip_p)
        self.squeeze, self.frames = bool(squeeze_time_dim), int(n_time_frames)
        self.device = torch.device(device)
        # albumentations.normalize: mean, std as float32 scaled by max_pixel_value (float32 products), float32 reciprocal
        m = np.array(torch.as_tensor(mean).tolist(), dtype=np.float32)
        s = np.array(torch.as_tensor(std).tolist(), dtype=np.float32)
        m *= np.float32(max_pixel_value)
        s *= np.float32(max_pixel_value)
        self.norm = torch.from_numpy(np.stack([m, np.reciprocal(s, dtype=np.float32)])).to(self.device)
        lut = label_lut(label_map)
        self.label_classes = int(lut.max()) + 1      # of the label map: what `ignore_label_boundaries` filters over
        self.lut = lut.to(self.device)
        self.raw = self.labels = None
        if self.S % 4:
            raise ValueError("random_crop_size must be a multiple of 4")

    def load(self, raw: torch.Tensor, labels: torch.Tensor | None) -> None:
        """raw: int16 [N, C, H, W] decoded tiles; labels: uint8 [N, H, W] (None for the MAE loaders).  Kept resident."""
        if raw.dtype != torch.int16 or raw.dim() != 4:
            raise ValueError("raw tiles must be int16 [N, C, H, W]")
        if labels is not None and (labels.dtype != torch.uint8 or labels.shape != (raw.shape[0],) + tuple(raw.shape[2:])):
            raise ValueError("labels must be uint8 [N, H, W]")
        if raw.shape[1] != self.norm.shape[1]:
            raise ValueError("mean / std length differs from the number of bands")
        if self.S > raw.shape[2] or self.S > raw.shape[3]:
            raise ValueError("crop larger than the tile")   # albumentations raises ValueError here too
        self.raw = raw.to(self.device).contiguous()
        self.labels = None if labels is None else labels.to(self.device).contiguous()

    def draw_params(self, indices, training: bool, generator: torch.Generator | None = None) -> torch.Tensor:
        """int32 [B, 4] = {tile, y0, x0, flips}: albumentations' coordinate formulas on host-drawn uniforms."""
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
        B, (H, W), S = idx.numel(), self.raw.shape[2:], self.S
        par = torch.zeros(B, 4, dtype=torch.int32)
        par[:, 0] = idx.to(torch.int32)
        if training and self.augment:
            u = torch.rand(B, 4, generator=generator, dtype=torch.float64)
            par[:, 1] = ((H - S + 1) * u[:, 0]).to(torch.int32)        # get_random_crop_coords: int((height - crop + 1) * h_start)
            par[:, 2] = ((W - S + 1) * u[:, 1]).to(torch.int32)
            par[:, 3] = (u[:, 2] < self.hp).to(torch.int32) + 2 * (u[:, 3] < self.vp).to(torch.int32)
        else:
            par[:, 1], par[:, 2] = (H - S) // 2, (W - S) // 2            # get_center_crop_coords
        return par

    @torch.no_grad()
    def __call__(self, indices=None, training: bool = True, params: torch.Tensor | None = None,
                 generator: torch.Generator | None = None) -> S2OSMSample:
        if self.raw is None:
            raise RuntimeError("call load() first")
        if not self.raw.is_cuda:
            raise RuntimeError("GpuTilePipeline runs on the GPU (there is no CPU fallback)")
        par = self.draw_params(indices, training, generator) if params is None else torch.as_tensor(params, dtype=torch.int32).cpu()
        N, C, H, W = self.raw.shape
        S, B = self.S, par.shape[0]
        ok = (par[:, 0] >= 0) & (par[:, 0] < N) & (par[:, 1] >= 0) & (par[:, 1] <= H - S) & (par[:, 2] >= 0) & (par[:, 2] <= W - S) \
            & (par[:, 3] >= 0) & (par[:, 3] <= 3)
        if par.shape[1:] != (4,) or not bool(ok.all()):
            raise ValueError("params out of range (tile index, crop offsets, flip bits)")
        par_d = par.contiguous().to(self.device)
        x = torch.empty(B, C, S, S, dtype=torch.float32, device=self.device)
        y = torch.empty(B, S, S, dtype=torch.int64, device=self.device) if self.labels is not None else None
        cached(_CALLS, tile_prep_call, self.raw, self.labels, par_d, self.norm, self.lut, x, y).run()
        if not self.squeeze and self.frames == 1:
            x = x.unsqueeze(2)            # per sample (c, 1, h, w), s2osm_dataset.py:64-66
        return S2OSMSample(x=x, y=y)

    # ---- dataset statistics over the resident tiles (data/dataset_stats.py) --------------------------------------------------
    def _stats_index(self, indices, need_labels: bool, limit: int | None = None) -> torch.Tensor:
        """int32 [M] tile indices (None = all resident tiles), validated on the host: the stages do not range-check them.
        Argument errors come first (ValueError), then the refusal to run anywhere but on the GPU."""
        if self.raw is None:
            raise RuntimeError("call load() first")
        if need_labels and self.labels is None:
            raise ValueError("the pipeline was loaded without labels")
        N = self.raw.shape[0]
        idx = torch.arange(N, dtype=torch.int64) if indices is None else torch.as_tensor(indices, dtype=torch.int64).reshape(-1).cpu()
        if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= N:
            raise ValueError("tile indices out of range (or none given)")
        if limit is not None and idx.numel() > limit:
            raise ValueError(f"at most {limit} tiles per call (the exact-integer bound of TILE_MOMENTS)")
        if not self.raw.is_cuda:
            raise RuntimeError("GpuTilePipeline runs on the GPU (there is no CPU fallback)")
        return idx.to(torch.int32)

    def _window(self, window) -> tuple[int, int, int, int]:
        H, W = self.raw.shape[2:]
        if isinstance(window, str):
            if window == "tile":
                return 0, 0, H, W
            if window == "center":                  # get_center_crop_coords, as draw_params(training=False)
                return (H - self.S) // 2, (W - self.S) // 2, self.S, self.S
            raise ValueError("window must be 'tile', 'center' or (y0, x0, h, w)")
        y0, x0, h, w = (int(v) for v in window)
        if y0 < 0 or x0 < 0 or h <= 0 or w <= 0 or y0 + h > H or x0 + w > W:
            raise ValueError("window outside the tile")
        return y0, x0, h, w

    @torch.no_grad()
    def _moments(self, indices=None):
        """(SUMS int64 [C, 2], SDPART float64 [C, NB], M, H*W) of one TILE_MOMENTS stage over the selected tiles, on the device."""
        idx = self._stats_index(indices, need_labels=False, limit=DS.MAX_MOMENT_TILES)
        M = idx.numel()
        N, C, H, W = self.raw.shape
        NB = D.moments_blocks(H * W)
        idx_d = idx.to(self.device)
        sums = torch.zeros(C, 2, dtype=torch.int64, device=self.device)
        sdpart = torch.zeros(C, NB, dtype=torch.float64, device=self.device)
        call = StageCall()
        call.add("TILE_MOMENTS", RAW=call.t(self.raw), INDEX=call.t(idx_d), SUMS=call.t(sums), SDPART=call.t(sdpart),
                 M=M, C=C, H=H, W=W, NSRC=N, NB=NB)
        call.run()
        return sums, sdpart, M, H * W

    def band_mean_std(self, indices=None, pooled: bool = False):
        """(mean, std) float32 CPU tensors [C] over the selected raw tiles - the two tensors the reference's `calculate_mean_std`
        stores in mean_std.pt, ready for `GpuTilePipeline(mean, std)`.  `std` is the reference's statistic, the mean over pixel
        positions of the per-position standard deviation across tiles; pooled=True returns the standard deviation over all values
        of the band instead (dataset_stats.mean_std_from_moments)."""
        sums, sdpart, M, HW = self._moments(indices)
        mean, std, pooled_std = DS.mean_std_from_moments(sums.cpu(), sdpart.cpu(), M, HW)
        return mean, (pooled_std if pooled else std)

    @torch.no_grad()
    def label_histogram(self, num_classes: int, indices=None, window="tile") -> torch.Tensor:
        """int64 [M, num_classes] on the device: per selected tile, how often each class (after the label map's remap) occurs in
        the window - "tile", "center" (the S x S centre crop: what `dataset[i]` yields under the reference's deterministic
        transform) or (y0, x0, h, w).  Remapped labels outside [0, num_classes) are not counted."""
        idx = self._stats_index(indices, need_labels=True)
        K, M = int(num_classes), idx.numel()
        if not 1 <= K <= 256:
            raise ValueError("num_classes must be in 1..256")
        y0, x0, wh, ww = self._window(window)
        N, H, W = self.labels.shape
        idx_d = idx.to(self.device)
        hist = torch.zeros(M, K, dtype=torch.int64, device=self.device)
        call = StageCall()
        call.add("TILE_LABEL_HIST", LABELS=call.t(self.labels), INDEX=call.t(idx_d), LUT=call.t(self.lut), HIST=call.t(hist),
                 M=M, H=H, W=W, K=K, Y0=y0, X0=x0, WH=wh, WW=ww, NSRC=N)
        call.run()
        return hist

    def class_probabilities(self, num_classes: int, ignore_zero_label: bool, indices=None, max_tiles: int = 2500,
                            generator: torch.Generator | None = None) -> torch.Tensor:
        """float32 CPU tensor [num_classes]: the reference's `get_class_probabilities` over whole tiles (it runs on the dataset
        before any crop transform is attached).  Like its `random.sample`, a subset of max_tiles tiles is drawn on the host
        (without replacement, from `generator`) when more are selected."""
        idx = self._stats_index(indices, need_labels=True)
        if idx.numel() > max_tiles:
            idx = idx[torch.randperm(idx.numel(), generator=generator)[:max_tiles]]
        return DS.probabilities_from_hist(self.label_histogram(num_classes, idx, "tile").cpu(), ignore_zero_label)

    def sample_weights(self, class_distribution, ignore_zero_label: bool = False, indices=None, window="center") -> torch.Tensor:
        """float32 CPU tensor [M]: the reference's `get_sample_weights` for the selected tiles, in their order."""
        K = len(torch.as_tensor(class_distribution).reshape(-1))
        return DS.sample_weights_from_hist(self.label_histogram(K, indices, window).cpu(), class_distribution, ignore_zero_label)

    @torch.no_grad()
    def ignore_label_boundaries(self, size: int = 3, ignore_index: int = 0) -> None:
        """Rewrite the resident labels ONCE so that a band around class boundaries is ignored: the new labels are
        `classmap.boundary_to_ignore(lut[labels], num_classes, size, ignore_index)` stored as uint8 CLASSES (no longer raw codes), and
        the pipeline's label table becomes the identity - TILE_PREP's `y`, `label_histogram`, `class_probabilities`, `sample_weights`
        and `TilePredictor.evaluate` then see the band as class `ignore_index` with no further change.  Rasterised polygon labels are
        wrong by a pixel or so wherever two classes meet; with the reference's `masked_loss` convention (class 0 ignored) the default
        takes those pixels out of loss, metrics and sampling weights.  `num_classes` is the label map's: its largest class + 1.
        Both tensors are REPLACED, not written (load() may have kept the caller's own label tensor): the packed TILE_PREP call binds
        its tensors anew at every use (`stage_call.cached`), and every other call over them is built per use, so none serves the old
        ones.  One launch; after a second call the band is that of the already banded labels."""
        size = CM.check_size(size)
        if self.raw is None:
            raise RuntimeError("call load() first")
        if self.labels is None:
            raise ValueError("the pipeline was loaded without labels")
        if self.label_classes > CM.MAX_CLASSES:
            raise ValueError(f"the label map has {self.label_classes} classes: boundaries are marked for at most {CM.MAX_CLASSES}")
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not 0 <= ignore_index < self.label_classes:
            raise ValueError(f"ignore_index must be a class id in [0, {self.label_classes})")
        if not self.labels.is_cuda:
            raise RuntimeError("GpuTilePipeline runs on the GPU (there is no CPU fallback)")
        new = torch.empty_like(self.labels)
        CM.launch(self.labels, new, self.label_classes, size, CM.BOUNDARY, ignore=ignore_index, src_lut=self.lut)
        self.labels = new
        self.lut = torch.arange(256, dtype=torch.int32).to(self.device)

    @torch.no_grad()
    def ignore_label_boundaries_within(self, distance, connectivity: int = 4, ignore_index: int = 0) -> None:
        """Rewrite the resident labels ONCE so that every labelled pixel within `distance` pixels (Euclidean) of a class boundary is
        ignored: the new labels are `classmap.boundary_band(lut[labels], num_classes, distance, connectivity, ignore_index)` stored as
        uint8 CLASSES, and the pipeline's label table becomes the identity - exactly what `ignore_label_boundaries` does for its
        square window, with the same consequences for TILE_PREP's `y`, the label statistics and `TilePredictor.evaluate`, and the same
        replace-not-write rule for both tensors.  distance = 0 marks the boundary pixels themselves; `DistanceBinnedMetrics` says how
        wide the band should be.  The label map must map into a byte: a table value outside [0, 256) is stored as its low byte."""
        conn, threshold = CM.check_connectivity(connectivity), CM.squared_threshold(distance)
        if self.raw is None:
            raise RuntimeError("call load() first")
        if self.labels is None:
            raise ValueError("the pipeline was loaded without labels")
        if self.label_classes > CM.MAX_CLASSES:
            raise ValueError(f"the label map has {self.label_classes} classes: boundaries are marked for at most {CM.MAX_CLASSES}")
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not 0 <= ignore_index < self.label_classes:
            raise ValueError(f"ignore_index must be a class id in [0, {self.label_classes})")
        if not self.labels.is_cuda:
            raise RuntimeError("GpuTilePipeline runs on the GPU (there is no CPU fallback)")
        self.labels = CM.run_band(self.labels, self.label_classes, threshold, conn, ignore_index, src_lut=self.lut)
        self.lut = torch.arange(256, dtype=torch.int32).to(self.device)

    @torch.no_grad()
    def ignore_small_label_regions(self, min_area: int, connectivity: int = 4, ignore_index: int = 0) -> None:
        """Rewrite the resident labels ONCE so that label regions below `min_area` pixels are ignored: the new labels are
        `classmap.sieve(lut[labels], num_classes, min_area, connectivity, to=ignore_index, fixed=(ignore_index,))` stored as uint8
        CLASSES, and the pipeline's label table becomes the identity - exactly what `ignore_label_boundaries` does for the boundary
        band, with the same consequences for TILE_PREP's `y`, the label statistics and `TilePredictor.evaluate`.  Rasterised polygons
        leave slivers of a few pixels; with the reference's `masked_loss` convention (class 0 ignored) the default takes them out of
        loss, metrics and sampling weights.  Both tensors are REPLACED, not written, for the reasons given there.  The label map must
        map into a byte: a table value outside [0, 256) is stored as its low byte (300 becomes class 44)."""
        area, conn = CM.check_min_area(min_area), CM.check_connectivity(connectivity)
        if self.raw is None:
            raise RuntimeError("call load() first")
        if self.labels is None:
            raise ValueError("the pipeline was loaded without labels")
        if self.label_classes > CM.MAX_CLASSES:
            raise ValueError(f"the label map has {self.label_classes} classes: regions are labelled for at most {CM.MAX_CLASSES}")
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not 0 <= ignore_index < self.label_classes:
            raise ValueError(f"ignore_index must be a class id in [0, {self.label_classes})")
        if not self.labels.is_cuda:
            raise RuntimeError("GpuTilePipeline runs on the GPU (there is no CPU fallback)")
        self.labels = CM.run_sieve(self.labels, self.label_classes, area, conn, 1, 1 << ignore_index, ignore_index, src_lut=self.lut)
        self.lut = torch.arange(256, dtype=torch.int32).to(self.device)

    @torch.no_grad()
    def rasterize_labels(self, polygons, origins, fill: int = 0, onto: bool = False) -> torch.Tensor:
        """Build the resident labels from polygons (`classmap.PolygonSet`) whose values are CLASSES of the pipeline's label map - what
        the reference does on the host with rasterio.features.rasterize (src/data/download_labels.py:203-227), here for every resident
        tile at once and under whatever tag-to-class mapping the values were made with.  `origins`: one (ox, oy) per resident tile, the
        tile's corner in the polygons' pixel frame.  A pixel inside several polygons takes the last; one inside none gets class `fill`.
        onto=True: the current labels are first taken through the label table and the polygons are burned over them, pixels inside no
        polygon keeping their class (`fill` is not used and must be left at 0) - corrections, or a mask: a value equal to the ignored
        class masks a polygon out.  The labels become uint8 classes and the label table the identity; both tensors are REPLACED, not
        written, exactly as `ignore_label_boundaries` documents.  Works on a pipeline loaded without labels (onto=False only).
        Returns int64 [N] on the device: the pixels of every tile inside no polygon, the numerator of the reference's MAX_UNLABELED
        test."""
        if not isinstance(polygons, CM.PolygonSet):
            raise ValueError("polygons must be a classmap.PolygonSet")
        if self.raw is None:
            raise RuntimeError("call load() first")
        N, _, H, W = self.raw.shape
        vals = polygons.host["values"]
        if vals is None or (vals.size and (vals.min() < 0 or vals.max() >= self.label_classes)):
            raise ValueError(f"the polygons' values must be classes of the label map: in [0, {self.label_classes})")
        if isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill < self.label_classes:
            raise ValueError(f"fill must be a class id in [0, {self.label_classes})")
        if onto and self.labels is None:
            raise ValueError("the pipeline was loaded without labels: there is nothing to burn onto")
        if onto and fill != 0:
            raise ValueError("fill is not used with onto=True: leave it at 0")
        o = CM.check_origins(origins, N)
        if not self.raw.is_cuda:
            raise RuntimeError("GpuTilePipeline runs on the GPU (there is no CPU fallback)")
        if onto:
            base = self.lut[self.labels.long()].to(torch.uint8)      # a new tensor; a table value outside a byte is stored as its low byte
            new, unfilled = CM.rasterize(polygons, o, fill=None, out=base, return_unfilled=True)
        else:
            new, unfilled = CM.rasterize(polygons, o, (H, W), fill=fill, dtype=torch.uint8, return_unfilled=True)
        self.labels = new
        self.lut = torch.arange(256, dtype=torch.int32).to(self.device)
        return unfilled

    @torch.no_grad()
    def label_components(self, num_classes: int | None = None, indices=None, connectivity: int = 4) -> torch.Tensor:
        """int64 [M, num_classes] on the device: per selected tile (None = every resident tile), how many connected regions each class
        (after the label map's remap) forms - the patch count behind the pixel counts of `label_histogram`.  num_classes=None: the
        label map's own class count.  Remapped labels outside [0, num_classes) belong to no region."""
        conn = CM.check_connectivity(connectivity)
        K = CM.check_classes(self.label_classes if num_classes is None else num_classes)
        idx = self._stats_index(indices, need_labels=True)
        H, W = self.labels.shape[1:]
        counts = torch.zeros(idx.numel(), K, dtype=torch.int64, device=self.device)
        status = CM.new_status(self.device)
        step = CM.maps_per_chunk(H, W, 9)                       # labels, areas and the gathered label rasters of a chunk
        for m0 in range(0, idx.numel(), step):
            src = self.labels.index_select(0, idx[m0:m0 + step].to(self.device))
            work = torch.empty(2, *src.shape, dtype=torch.int32, device=self.device)
            CM.launch_components(src, K, conn, 0, work[0], work[1], status, counts[m0:m0 + step], src_lut=self.lut)
        CM.raise_status(status)
        return counts

    def _zone_rasters(self, zones, indices, need_labels: bool):
        """(idx, zones) for the zonal methods: `zones` int32 / int64 [M, H, W], one raster per selected tile, of the tiles' size"""
        if self.raw is None:
            raise RuntimeError("call load() first")
        z = ZN._check_zones(zones)
        N, _, H, W = self.raw.shape
        M = N if indices is None else torch.as_tensor(indices).numel()
        if zones.dim() != 3 or tuple(z.shape) != (M, H, W):
            raise ValueError(f"zones must be [M, H, W] = [{M}, {H}, {W}]: one raster per selected tile")
        return self._stats_index(indices, need_labels), z

    @torch.no_grad()
    def zonal_label_histogram(self, zones, num_zones: int, indices=None, num_classes: int | None = None) -> torch.Tensor:
        """int64 [num_zones, num_classes] on the device (num_classes=None: the label map's own class count, at most 32): how many pixels of every label class (after the label map's remap) lie in
        every zone of `zones` (int32 or int64 [M, H, W], one raster per selected tile, global zone ids, negative = no zone:
        `classmap.rasterize(..., burn="index", fill=-1)`) - `zonal.histogram` of the resident labels read through the pipeline's label
        table inside the kernel.  Remapped labels outside [0, num_classes) are not counted."""
        K = CM.check_classes(self.label_classes if num_classes is None else num_classes)
        Z, _ = ZN._check_num_zones(num_zones, 1, False)
        idx, z = self._zone_rasters(zones, indices, need_labels=True)
        ZN._need_gpu(z)
        hist = torch.zeros(Z, K, dtype=torch.int64, device=self.device)
        status = CM.new_status(self.device)
        H, W = z.shape[1:]
        step = CM.maps_per_chunk(H, W, 1)                       # the gathered label rasters of a chunk
        for m0 in range(0, idx.numel(), step):
            src = self.labels.index_select(0, idx[m0:m0 + step].to(self.device))
            ZN.launch_histogram(z[m0:m0 + step], 0, src, Z, K, hist, status, src_lut=self.lut)
        ZN.raise_status(status)
        return hist

    @torch.no_grad()
    def zonal_band_stats(self, zones, num_zones: int, indices=None, nodata=None):
        """`zonal.ZonalStats` [num_zones, C] of the resident raw tiles inside every zone of `zones` (as for `zonal_label_histogram`):
        count, sum, sum of squares, minimum and maximum per zone and band, exact; nodata=v leaves a band value equal to v out."""
        Z, _ = ZN._check_num_zones(num_zones, 1, False)
        nd = None if nodata is None else ZN._check_int(nodata, ZN.INT32_MIN, ZN.INT32_MAX, "nodata")
        idx, z = self._zone_rasters(zones, indices, need_labels=False)
        C, H, W = self.raw.shape[1:]
        if C > ZN.MAX_BANDS:
            raise ValueError(f"zonal band statistics take at most {ZN.MAX_BANDS} bands")
        ZN._need_gpu(z)
        stats = ZN.new_stats((Z, C), self.device)
        status = CM.new_status(self.device)
        step = CM.maps_per_chunk(H, W, 2 * C)                   # the gathered tiles of a chunk
        for m0 in range(0, idx.numel(), step):
            vals = self.raw.index_select(0, idx[m0:m0 + step].to(self.device))
            ZN.launch_bands(z[m0:m0 + step], 0, vals, Z, nd, stats, status)
        ZN.raise_status(status)
        return stats

    def weighted_indices(self, weights, num_samples: int, generator: torch.Generator | None = None) -> torch.Tensor:
        """int64 [num_samples] positions drawn with replacement in proportion to `weights`, on the host: exactly what
        `WeightedRandomSampler(weights, num_samples, True, generator=generator)` yields.  They index the tiles the weights were
        computed for (`indices[drawn]` for a subset) and go straight into `draw_params`."""
        if self.raw is None:
            raise RuntimeError("call load() first")
        if not self.raw.is_cuda:
            raise RuntimeError("GpuTilePipeline runs on the GPU (there is no CPU fallback)")
        return DS.weighted_indices(weights, num_samples, generator)

    # ---- exact percentiles and quicklooks of the resident tiles (data/quicklook.py) -------------------------------------------
    def _loaded_shape(self):
        if self.raw is None:
            raise RuntimeError("call load() first")
        return tuple(int(v) for v in self.raw.shape)

    def band_percentiles(self, q, indices=None, bands=None, pooled: bool = True) -> torch.Tensor:
        """float64 CPU tensor of exact percentiles `q` (numpy's linear method on the values as float64) of the selected raw tiles:
        pooled=True [len(bands), len(q)], every band (None = all) over all selected tiles - robust clipping bounds beside
        `band_mean_std` where clouds and nodata make the moments useless; pooled=False [M, len(q)], per tile over the pixels of
        `bands` taken jointly (the quicklook's statistic).  A tile listed twice counts twice.  Any number of percentiles: they are
        selected four at a time (eight ranks per program)."""
        N, C, H, W = self._loaded_shape()
        qs = QL.check_q(q)
        bl = QL.check_bands(range(C) if bands is None else bands, C)
        idx = self._stats_index(indices, need_labels=False)
        n = (idx.numel() if pooled else len(bl)) * H * W
        out = []
        for i in range(0, len(qs), QL.MAX_RANKS // 2):
            ranks, frac = QL.rank_plan(qs[i:i + QL.MAX_RANKS // 2], n)
            out.append(QL.run_selection(self.raw, idx, bl, bool(pooled), ranks, frac)[1].cpu())
        return torch.cat(out, 1)

    def zero_fraction(self, indices=None, band: int = 0) -> torch.Tensor:
        """float64 CPU tensor [M]: the share of pixels of `band` that are exactly 0 in every selected tile - the nodata share
        src/experiments/sentinel_EDA.py:20-27 computes per tile on the CPU, as a fraction."""
        N, C, H, W = self._loaded_shape()
        b = QL.check_bands([band], C)[0]
        idx = self._stats_index(indices, need_labels=False)
        return QL.run_zero_count(self.raw, idx, b).cpu().double() / float(H * W)

    @torch.no_grad()
    def stretch_bounds(self, params, bands=(2, 1, 0), percentile: float = 98.0) -> torch.Tensor:
        """float64 [B, 2] on the device: for every row of `params` ({tile, y0, x0, flips}) the bounds (lo, hi) between which
        `quicklook(params=params, bands=bands, percentile=percentile)` stretches that row's picture - the percentiles
        (100 - percentile, percentile) over the three bands of the row's WHOLE tile, i.e. `band_percentiles([100 - p, p], tiles,
        bands, pooled=False)` gathered per sample.  Every distinct tile is selected once.  They put other pictures of the same crops
        (`render.mae_panels`) on the quicklook's colour scale."""
        N, C, H, W = self._loaded_shape()
        bl = QL.check_bands(bands, C, count=3)
        p = QL.check_percentile(percentile)
        if params is None:
            raise ValueError("params must be an integer array [B, 4] = {tile, y0, x0, flips}")
        par = QL.check_params(params, N, H, W, self.S, self.S)
        if not self.raw.is_cuda:
            raise RuntimeError("GpuTilePipeline runs on the GPU (there is no CPU fallback)")
        tiles, slot = torch.unique(par[:, 0], return_inverse=True)
        ranks, frac = QL.rank_plan([100.0 - p, p], 3 * H * W)
        pct = QL.run_selection(self.raw, tiles.to(torch.int32), bl, False, ranks, frac)[1]
        return pct.index_select(0, slot.to(self.device))

    @torch.no_grad()
    def quicklook(self, indices=None, params=None, bands=(2, 1, 0), percentile: float = 98.0, whole_tile: bool = False) -> torch.Tensor:
        """uint8 [B, S, S, 3] (h w rgb) on the device: the reference's percentile-stretched picture of `bands` for every sample -
        the crop `params` names (the same {tile, y0, x0, flips} array given to `__call__`: the picture is what the model saw), or
        the centre crop of the tiles `indices` (None = all).  whole_tile=True: [B, H, W, 3], the whole tile (params offsets 0).
        The bounds are the percentiles (100 - percentile, percentile) over ALL pixels of the three bands of the WHOLE tile jointly,
        as in src/plotting.py:75-96, then `clip((v - lo) / (hi - lo) * 255, 0, 255)` truncated to uint8, bit for bit numpy's.

        A tile whose two bounds coincide (a constant tile, or one that is mostly nodata) gives a black picture: the reference
        divides by zero there and stores whatever the cast makes of NaN / inf."""
        N, C, H, W = self._loaded_shape()
        bl = QL.check_bands(bands, C, count=3)
        p = QL.check_percentile(percentile)
        SH, SW = (H, W) if whole_tile else (self.S, self.S)
        if params is None:
            idx = torch.arange(N, dtype=torch.int64) if indices is None else torch.as_tensor(indices, dtype=torch.int64).reshape(-1).cpu()
            if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= N:
                raise ValueError("tile indices out of range (or none given)")
            params = self.draw_params(idx, training=False)
            if whole_tile:
                params[:, 1:3] = 0
        par = QL.check_params(params, N, H, W, SH, SW)
        if not self.raw.is_cuda:
            raise RuntimeError("GpuTilePipeline runs on the GPU (there is no CPU fallback)")
        B = par.shape[0]
        tiles, slot = torch.unique(par[:, 0], return_inverse=True)      # every tile's bounds are selected once
        ranks, frac = QL.rank_plan([100.0 - p, p], 3 * H * W)
        out = torch.empty(B, SH, SW, 3, dtype=torch.uint8, device=self.device)

        QL.run_selection(self.raw, tiles.to(torch.int32), bl, False, ranks, frac,
                         extra=lambda call, pct: QL.add_quicklook(call, self.raw, par, slot, bl, pct, out, int(tiles.numel())))
        return out
