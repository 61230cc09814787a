"""Class-map neighbourhood filters on the GPU: the k x k majority (mode) filter of a class map, and the ignore band around label
boundaries.

A per-pixel argmax at 10 m carries salt-and-pepper - isolated pixels and specks of two or three - and every land-cover product removes
it with a majority filter before anyone looks at the map or counts areas.  The labels have the opposite problem: rasterised OSM
polygons (src/data/s2osm_dataset.py:51-71) are wrong by a pixel or so wherever two classes meet, and the usual remedy is to put a
band around class boundaries into the ignored class, which the reference's `masked_loss` then leaves out of loss, metrics and sampling
weights.  The reference has neither operation.  Both are one kernel, the per-pixel histogram of classes over a size x size window
clipped to the image (csrc/classmap.hip; the definition is in include/s2k.h at s2k_classmap_filter), integer work with an exact answer.

    smooth = majority_filter(class_map, num_classes=4, size=5)               # same dtype and shape, the centre wins ties
    smooth, n = majority_filter(class_map, 4, size=3, iterations=2, votes=(1, 2, 3), fixed=(0,), return_changed=True)
    labels = boundary_to_ignore(labels, num_classes=4, size=3, ignore_index=0)

`TilePredictor.predict / evaluate / render(majority=k)` and `GpuTilePipeline.ignore_label_boundaries` are built on them.

What a window cannot see is the REGIONS of a map.  Every land-cover product removes patches below a minimum mapping unit (the "sieve"),
after or instead of the majority filter - a 5 x 5 window cannot remove a 30-pixel speck, and it erodes the thin roads a sieve keeps;
rasterised polygons leave slivers of a few pixels; and the number and size of patches per class is the question after the per-class
pixel counts of the reference's experiments/label_EDA.py.  All three rest on connected-component labelling, which is block-local
union-find in LDS, a merge across tile edges and a flatten (csrc/components.hip: three launches whatever the map looks like, where the
`max_pool2d` propagation idiom needs as many passes as the longest path in a component); the definitions are in include/s2k.h at
s2k_classmap_components.  Integer work with one exact answer; labels are canonical (a component's smallest linear index).

    labels, areas, counts = connected_components(class_map, 4, connectivity=8, return_areas=True, return_counts=True)
    clean = sieve(class_map, num_classes=4, min_area=16)                     # small patches take the class of their best neighbour
    clean, n = sieve(class_map, 4, 16, connectivity=8, iterations=2, fixed=(0,), to=0, return_changed=True)

`TilePredictor.predict / evaluate / render(min_area=a)`, `GpuTilePipeline.ignore_small_label_regions` and `label_components` are built
on them.  The kernels' loops are bounded by construction and carry that bound; a `status` word the wrappers read once, at the end of a
public call, reports an overrun as `_lib.S2kError` (it is the only host read they make).

What neither a window nor a region gives is a DISTANCE: how far a pixel is from the nearest class boundary, or from the nearest pixel of
some classes.  It is the quantity behind the band itself (`boundary_to_ignore` can only draw a square window of 3 to 15 pixels),
behind the question whether a model's errors sit at the label boundaries (`metrics.DistanceBinnedMetrics`: confusion counts binned by
the distance to the nearest boundary), and behind filling no-data from the nearest labelled pixel.  All rest on the exact Euclidean
distance transform (csrc/distance.hip: a column pass and a row pass, two launches whatever the map looks like; the definitions are in
include/s2k.h at s2k_classmap_distance).  Integer work with one exact answer: squared distances, and the nearest site with a canonical
tie rule (the smallest linear index).  Every loop of the kernels is bounded by its trip limit; there is no status word to read.

    d2 = distance_transform(class_map, 4)                                    # int32 squared distance to the nearest class boundary
    d2, site = distance_transform(class_map, 4, to=(2, 3), return_nearest=True)      # ... to the nearest pixel of class 2 or 3
    labels = boundary_band(labels, num_classes=4, distance=2.5, ignore_index=0)      # the Euclidean sibling of boundary_to_ignore
    filled = fill_nearest(class_map, 4, fill=(0,))                           # class 0 and no-data take their nearest other pixel's class

`GpuTilePipeline.ignore_label_boundaries_within`, `metrics.DistanceBinnedMetrics` and `TilePredictor.evaluate_by_distance` are built on
them.

All of the above read a class map, and a class map does not say how SURE it is.  `confidence` turns [B, K, H, W] probabilities or
logits into the class map and a confidence raster - the largest probability, or its margin over the runner-up - and can put every pixel
below a confidence into an abstention class (csrc/calibration.hip, one launch; the definitions are in include/s2k.h at
s2k_calibration).  Whether that confidence means anything is `metrics.CalibrationMetrics`' question, from the same launch.

    class_map, conf = confidence(probs)                                      # int64 [B, H, W], float32 [B, H, W]
    class_map, conf = confidence(logits, "logits", "margin", temperature=1.7, min_confidence=0.2, reject_to=0, dtype=torch.uint8)

`TilePredictor.predict_with_confidence` and `evaluate_calibration` are built on it.

And all of the above CONSUME label rasters.  The reference makes its own on the host, burning OSM polygons into 512 x 512 uint8 tiles
with rasterio.features.rasterize (src/data/download_labels.py:203-227: the last of overlapping features wins, then the MAX_UNLABELED test
on the share of pixels left at 0).  `PolygonSet` keeps the polygons resident and `rasterize` burns them into any number of tiles on the
GPU (csrc/rasterize.hip, three launches whatever the geometry looks like; the definitions are in include/s2k.h at s2k_rasterize):
fixed-point vertices, 256 units per pixel, the even-odd rule over half-open edges with the crossing compared exactly in int64 - the
top-left rule, so polygons that share an edge partition the pixel centres on it.  Integer work with one exact answer.

    ps = PolygonSet.from_geojson(geometries, values, west, north, xsize, ysize)         # or PolygonSet(shapes, values) in AOI pixels
    labels, unfilled = rasterize(ps, origins, (512, 512), fill=0, return_unfilled=True)      # uint8 [M, 512, 512], int64 [M]
    zones = rasterize(ps, origins, (512, 512), fill=-1, dtype=torch.int32, burn="index")      # the polygon index per pixel
    rasterize(corrections, origins, fill=None, out=labels)                                    # burn onto what is there

`GpuTilePipeline.rasterize_labels` is built on it.  How the result compares with GDAL's on real data has not been measured: it is
expected to agree except within 1 / 512 pixel of an edge (the quantisation) and exactly on one (GDAL has its own tie rule).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

MAX_CLASSES = 32        # four byte counters to a dword, at most eight dwords of window histogram in registers
MIN_SIZE, MAX_SIZE = 3, 15      # 15 x 15 = 225 votes still fit a byte counter
STRIP = 64              # columns a wave holds (CLASSMAP_STRIP): STRIP - 2 * (size // 2) of them are outputs
BAND = 16               # output rows a wave walks (CLASSMAP_BAND)
MAJORITY, BOUNDARY = _lib.CLASSMAP_MODES["majority"], _lib.CLASSMAP_MODES["boundary"]
CC_TILE_H, CC_TILE_W = 16, 64   # the tile one workgroup labels in LDS (csrc/components.hip)
WORKSPACE_BYTES = 512 << 20     # labels + areas + best of one chunk of maps stay below this
NO_SITE = 2**31 - 1             # dist2 where a map has no site (nearest is -1 there)
EDT_COLS, EDT_ROWS = 64, 8      # columns of a column-pass workgroup; rows a row-pass workgroup walks (csrc/distance.hip)
EDT_MAX_EDGES, EDT_MAX_DIM = 8, 16384
TO_CLASSES, TO_BOUNDARY = _lib.CLASSMAP_DISTANCE_MODES["classes"], _lib.CLASSMAP_DISTANCE_MODES["boundary"]


def strip_outputs(size: int) -> int:
    """output columns of one wave's strip"""
    return STRIP - 2 * (int(size) // 2)


def check_size(size) -> int:
    if isinstance(size, bool) or not isinstance(size, int) or not MIN_SIZE <= size <= MAX_SIZE or size % 2 == 0:
        raise ValueError(f"size must be an odd integer in {MIN_SIZE}..{MAX_SIZE}")
    return size


def check_classes(num_classes) -> int:
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"num_classes must be an integer in 1..{MAX_CLASSES}")
    return num_classes


def check_iterations(iterations) -> int:
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
        raise ValueError("iterations must be a positive integer")
    return iterations


def class_bits(ids, K: int, what: str) -> int:
    """the bit mask of the class ids `ids` (None: every class)"""
    if ids is None:
        return (1 << K) - 1
    bits = 0
    for c in ids:
        if isinstance(c, bool) or int(c) != c or not 0 <= int(c) < K:
            raise ValueError(f"{what} must hold class ids in [0, {K})")
        bits |= 1 << int(c)
    return bits


def _check_map(class_map) -> torch.Tensor:
    """[M, H, W] view of a uint8 / int64 class map given as [M, H, W] or [H, W]"""
    if not isinstance(class_map, torch.Tensor) or class_map.dtype not in (torch.uint8, torch.int64):
        raise ValueError("class_map must be a uint8 or int64 tensor")
    if class_map.dim() not in (2, 3) or class_map.numel() == 0:
        raise ValueError("class_map must be [M, H, W] or [H, W] and not empty")
    m = class_map.contiguous()
    return m.view(1, *m.shape) if m.dim() == 2 else m


def launch(src, dst, K: int, size: int, mode: int, votes: int = 0, fixed: int = 0, ignore: int = 0, src_lut=None, labels=None,
           index=None, lut=None, hist=None, changed=None) -> None:
    """One s2k_classmap_filter launch from `src` into `dst` ([M, H, W], uint8 or int64 each) on src's device and current stream."""
    if not src.is_cuda:
        raise RuntimeError("class-map filters run on the GPU (there is no CPU fallback)")
    M, H, W = src.shape
    with torch.cuda.device(src.device):
        _lib.check(_lib.classmap_filter(src, src_lut, dst, (M, H, W, K), size, mode, votes, fixed, ignore, labels, index, lut,
                                        0 if labels is None else labels.shape[0], hist, changed,
                                        torch.cuda.current_stream(src.device).cuda_stream))


def run_majority(src, K: int, size: int, iterations: int, votes: int, fixed: int, changed=None, last=None) -> torch.Tensor:
    """`iterations` majority launches from `src` ([M, H, W]), ping-pong between two new buffers; `last`: the hist operands (labels,
    index, lut, hist) of the final launch.  `src` is left as it is."""
    bufs = [torch.empty_like(src) for _ in range(min(iterations, 2))]
    cur = src
    for it in range(iterations):
        dst = bufs[it % 2]
        extra = dict(zip(("labels", "index", "lut", "hist"), last)) if last is not None and it == iterations - 1 else {}
        launch(cur, dst, K, size, MAJORITY, votes, fixed, changed=changed, **extra)
        cur = dst
    return cur


@torch.no_grad()
def majority_filter(class_map, num_classes: int, size: int = 3, iterations: int = 1, votes=None, fixed=(), return_changed: bool = False):
    """The size x size majority filter of `class_map` (uint8 or int64, [M, H, W] or [H, W], on the GPU), `iterations` times: the same
    dtype and shape.  Windows are clipped to the map.  Only the classes in `votes` vote (None: all); a pixel keeps its class if that
    class has the most votes, ties included, if nobody voted, if its class is in `fixed`, or if it lies outside [0, num_classes);
    otherwise it takes the lowest class among those with the most votes.  return_changed=True adds int64 [M]: the pixels changed,
    summed over the iterations."""
    K, size, iterations = check_classes(num_classes), check_size(size), check_iterations(iterations)
    vb, fb = class_bits(votes, K, "votes"), class_bits(fixed, K, "fixed")
    src = _check_map(class_map)
    if not src.is_cuda:
        raise RuntimeError("class-map filters run on the GPU (there is no CPU fallback)")
    changed = torch.zeros(src.shape[0], dtype=torch.int64, device=src.device) if return_changed else None
    out = run_majority(src, K, size, iterations, vb, fb, changed).view(class_map.shape)
    return (out, changed) if return_changed else out


@torch.no_grad()
def boundary_to_ignore(class_map, num_classes: int, size: int = 3, ignore_index: int = 0) -> torch.Tensor:
    """`class_map` with every pixel whose size x size window (clipped to the map) holds another class - other than its own and other
    than `ignore_index` - set to `ignore_index`: the band around class boundaries.  A pixel that only touches the ignored class keeps
    its class, so the ignored region does not grow on its own; pixels outside [0, num_classes) are copied and mark nothing."""
    K, size = check_classes(num_classes), check_size(size)
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not 0 <= ignore_index < K:
        raise ValueError(f"ignore_index must be a class id in [0, {K})")
    src = _check_map(class_map)
    if not src.is_cuda:
        raise RuntimeError("class-map filters run on the GPU (there is no CPU fallback)")
    dst = torch.empty_like(src)
    launch(src, dst, K, size, BOUNDARY, ignore=ignore_index)
    return dst.view(class_map.shape)


# ---- connected components and the minimum-area sieve (csrc/components.hip) ----------------------------------------------------------------
def check_connectivity(connectivity) -> int:
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    return connectivity


def check_min_area(min_area) -> int:
    if isinstance(min_area, bool) or not isinstance(min_area, int) or not 1 <= min_area < 1 << 31:
        raise ValueError("min_area must be a positive integer (below 2^31)")
    return min_area


def check_to(to, K: int) -> int:
    """the C entry's `to`: -1 for None (the donor rule), else the class id"""
    if to is None:
        return -1
    if isinstance(to, bool) or not isinstance(to, int) or not 0 <= to < K:
        raise ValueError(f"to must be None or a class id in [0, {K})")
    return to


def new_status(device) -> torch.Tensor:
    """the zeroed `status` word of the component kernels (include/s2k.h): OR-ed into by every launch that is handed it"""
    return torch.zeros(1, dtype=torch.int32, device=device)


def raise_status(status: torch.Tensor) -> None:
    """The one host read of a public call: S2kError if a kernel overran the step bound of its union-find loops (bits 1, 2, 4) or the
    sieve met labels outside [-1, H * W) (bit 8)."""
    code = int(status.item())
    if code:
        raise _lib.S2kError(f"connected components: status {code:#x} (1 tile pass, 2 edge merge, 4 flatten overran their step bound; "
                            "8 labels out of range): the outputs are not to be used")


def maps_per_chunk(H: int, W: int, bytes_per_pixel: int) -> int:
    """maps whose workspace of `bytes_per_pixel` stays below WORKSPACE_BYTES (at least one)"""
    return max(1, (WORKSPACE_BYTES - 1) // (bytes_per_pixel * H * W))


def launch_components(src, K: int, connectivity: int, exclude: int, labels, areas, status, counts=None, src_lut=None) -> None:
    """One s2k_classmap_components call over `src` ([M, H, W], uint8 or int64) on src's device and current stream: three launches."""
    if not src.is_cuda:
        raise RuntimeError("connected components run on the GPU (there is no CPU fallback)")
    M, H, W = src.shape
    with torch.cuda.device(src.device):
        _lib.check(_lib.classmap_components(src, src_lut, (M, H, W, K), connectivity, exclude, labels, areas, counts, status,
                                            torch.cuda.current_stream(src.device).cuda_stream))


def launch_sieve(src, dst, K: int, min_area: int, fixed: int, to: int, labels, areas, best, status, src_lut=None, hist_labels=None,
                 index=None, lut=None, hist=None, changed=None) -> None:
    """One s2k_classmap_sieve call (one pass) from `src` into `dst` over the labels and areas of `launch_components(src, ...)`."""
    if not src.is_cuda:
        raise RuntimeError("the sieve runs on the GPU (there is no CPU fallback)")
    M, H, W = src.shape
    with torch.cuda.device(src.device):
        _lib.check(_lib.classmap_sieve(src, src_lut, dst, (M, H, W, K), min_area, fixed, to, labels, areas, best, hist_labels, index, lut,
                                       0 if hist_labels is None else hist_labels.shape[0], hist, changed, status,
                                       torch.cuda.current_stream(src.device).cuda_stream))


def run_sieve(src, K: int, min_area: int, connectivity: int, iterations: int, fixed: int, to: int, changed=None, last=None,
              src_lut=None) -> torch.Tensor:
    """`iterations` passes of label -> sieve over `src` ([M, H, W]) into a new tensor of src's dtype; the count is fixed, nothing is read
    between passes.  M is walked in chunks whose workspace (labels, areas and, without `to`, best) stays below WORKSPACE_BYTES.
    `src_lut` (int32 [256]) reads a uint8 src through a table in the first pass; `last`: the hist operands (labels, index, lut, hist) of
    the final pass, `index` an int32 [M] device tensor.  `src` is left as it is.  Ends with the status read.  With `src_lut` the
    result is one byte per pixel: a table value outside [0, 256) is stored as its low byte, and is that byte to every later pass."""
    M, H, W = src.shape
    dev = src.device
    step = maps_per_chunk(H, W, 8 if to >= 0 else 16)
    n = min(step, M)
    labels = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    areas = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    best = torch.empty(n, H, W, dtype=torch.int64, device=dev) if to < 0 else None
    ping = [torch.empty(n, H, W, dtype=src.dtype, device=dev) for _ in range(min(iterations - 1, 2))]
    out = torch.empty_like(src)
    status = new_status(dev)
    for m0 in range(0, M, step):
        m1 = min(m0 + step, M)
        k = m1 - m0
        cur, table = src[m0:m1], src_lut
        for it in range(iterations):
            final = it == iterations - 1
            dst = out[m0:m1] if final else ping[it % 2][:k]
            extra = {}
            if final and last is not None:
                extra = dict(hist_labels=last[0], index=last[1][m0:m1], lut=last[2], hist=last[3])
            launch_components(cur, K, connectivity, 0, labels[:k], areas[:k], status, src_lut=table)
            launch_sieve(cur, dst, K, min_area, fixed, to, labels[:k], areas[:k], None if best is None else best[:k], status, src_lut=table,
                         changed=None if changed is None else changed[m0:m1], **extra)
            cur, table = dst, None
    raise_status(status)
    return out


@torch.no_grad()
def connected_components(class_map, num_classes: int, connectivity: int = 4, exclude=(), return_areas: bool = False,
                         return_counts: bool = False):
    """int32 labels of `class_map`'s shape (uint8 or int64, [M, H, W] or [H, W], on the GPU): every pixel whose class lies in
    [0, num_classes) and not in `exclude` gets the smallest linear index y * W + x of its component - same class, joined through 4- or
    8-neighbours, inside its own map - and every other pixel -1.  return_areas=True adds int32 root areas of the same shape (the pixel
    count of the component at its root, 0 elsewhere), return_counts=True int64 [M, num_classes]: components per class and map.
    WORKSPACE_BYTES bounds workspace only: the labels, and the areas when they are asked for, are outputs and are allocated for all
    M maps at once; areas nobody asked for are workspace and M is walked in chunks."""
    K, conn = check_classes(num_classes), check_connectivity(connectivity)
    eb = class_bits(exclude, K, "exclude")
    src = _check_map(class_map)
    if not src.is_cuda:
        raise RuntimeError("connected components run on the GPU (there is no CPU fallback)")
    M, H, W = src.shape
    dev = src.device
    labels = torch.empty(M, H, W, dtype=torch.int32, device=dev)
    counts = torch.zeros(M, K, dtype=torch.int64, device=dev) if return_counts else None
    status = new_status(dev)
    step = M if return_areas else maps_per_chunk(H, W, 4)      # areas nobody asked for are workspace
    areas = torch.empty(min(step, M), H, W, dtype=torch.int32, device=dev)
    for m0 in range(0, M, step):
        m1 = min(m0 + step, M)
        launch_components(src[m0:m1], K, conn, eb, labels[m0:m1], areas[:m1 - m0], status, None if counts is None else counts[m0:m1])
    raise_status(status)
    out = [labels.view(class_map.shape)]
    if return_areas:
        out.append(areas.view(class_map.shape))
    if return_counts:
        out.append(counts)
    return out[0] if len(out) == 1 else tuple(out)


@torch.no_grad()
def sieve(class_map, num_classes: int, min_area: int, connectivity: int = 4, iterations: int = 1, fixed=(), to=None,
          return_changed: bool = False):
    """`class_map` (uint8 or int64, [M, H, W] or [H, W], on the GPU) without its components below `min_area` pixels, `iterations` times:
    the same dtype and shape.  A small component whose class is not in `fixed` becomes `to`, or without `to` takes the class of its best
    donor: the components that share a pixel edge with it, those of at least `min_area` first, then the larger area, then the lower
    root; one without a donor stays.  All relabelling of a pass is simultaneous; pixels outside [0, num_classes) are copied and donate
    nothing.  return_changed=True adds int64 [M]: the pixels changed, summed over the iterations."""
    K, area, conn, iterations = check_classes(num_classes), check_min_area(min_area), check_connectivity(connectivity), check_iterations(iterations)
    fb, t = class_bits(fixed, K, "fixed"), check_to(to, K)
    src = _check_map(class_map)
    if not src.is_cuda:
        raise RuntimeError("the sieve runs on the GPU (there is no CPU fallback)")
    changed = torch.zeros(src.shape[0], dtype=torch.int64, device=src.device) if return_changed else None
    out = run_sieve(src, K, area, conn, iterations, fb, t, changed).view(class_map.shape)
    return (out, changed) if return_changed else out


# ---- the exact Euclidean distance transform (csrc/distance.hip) ----------------------------------------------------------------------------
def check_ignore_index(ignore_index, K: int) -> int:
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not 0 <= ignore_index < K:
        raise ValueError(f"ignore_index must be a class id in [0, {K})")
    return ignore_index


def squared_threshold(distance, what: str = "distance") -> int:
    """floor(distance^2) of a distance in pixels (finite, >= 0): the threshold on dist2 that `dist2 <= t` is `d <= distance` for"""
    if isinstance(distance, bool) or not isinstance(distance, (int, float)) or not math.isfinite(distance) or distance < 0:
        raise ValueError(f"{what} must be a finite number of pixels >= 0")
    return min(math.floor(distance * distance), NO_SITE - 1)


def check_edges(edges) -> list:
    """the thresholds on dist2 of 1..EDT_MAX_EDGES bin edges in pixels: floor(edge^2), strictly ascending"""
    try:
        edges = list(edges)
    except TypeError:
        raise ValueError("edges must be a sequence of distances in pixels") from None
    if not 1 <= len(edges) <= EDT_MAX_EDGES:
        raise ValueError(f"edges must hold 1..{EDT_MAX_EDGES} distances")
    out = [squared_threshold(e, "an edge") for e in edges]
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"edges must ascend strictly after floor(edge^2): got {out}")
    return out


def check_sites(to, K: int, exclude: int):
    """(mode, sites) of the C entry for `to`: "boundary", or an iterable of class ids that `exclude` does not name"""
    if isinstance(to, str):
        if to != "boundary":
            raise ValueError('to must be "boundary" or an iterable of class ids')
        return TO_BOUNDARY, 0
    try:
        ids = list(to)
    except TypeError:
        raise ValueError('to must be "boundary" or an iterable of class ids') from None
    sites = class_bits(ids, K, "to")
    if sites == 0:
        raise ValueError("to must name at least one class")
    if sites & exclude:
        raise ValueError("to and exclude overlap")
    return TO_CLASSES, sites


def _check_dims(src) -> None:
    if src.shape[1] > EDT_MAX_DIM or src.shape[2] > EDT_MAX_DIM:
        raise ValueError(f"the distance transform takes maps of at most {EDT_MAX_DIM} x {EDT_MAX_DIM}")


def launch_distance(src, K: int, mode: int, sites: int, connectivity: int, exclude: int, work, dist2, nearest=None, src_lut=None, other=None,
                    edges=None, hist=None) -> None:
    """One s2k_classmap_distance call over `src` ([M, H, W], uint8 or int64) on src's device and current stream: two launches."""
    if not src.is_cuda:
        raise RuntimeError("the distance transform runs on the GPU (there is no CPU fallback)")
    M, H, W = src.shape
    with torch.cuda.device(src.device):
        _lib.check(_lib.classmap_distance(src, src_lut, (M, H, W, K), mode, sites, connectivity, exclude, work, dist2, nearest, other, edges,
                                          hist, torch.cuda.current_stream(src.device).cuda_stream))


def run_distance(src, K: int, mode: int, sites: int, connectivity: int, exclude: int, want_nearest: bool = False, src_lut=None):
    """(dist2, nearest or None), int32 [M, H, W], of `src` ([M, H, W]); M is walked in chunks whose workspace (the 16-bit column offsets)
    stays below WORKSPACE_BYTES.  The outputs are allocated for all M maps at once."""
    M, H, W = src.shape
    dev = src.device
    step = maps_per_chunk(H, W, 2)
    work = torch.empty(min(step, M), H, W, dtype=torch.int16, device=dev)
    dist2 = torch.empty(M, H, W, dtype=torch.int32, device=dev)
    nearest = torch.empty(M, H, W, dtype=torch.int32, device=dev) if want_nearest else None
    for m0 in range(0, M, step):
        m1 = min(m0 + step, M)
        launch_distance(src[m0:m1], K, mode, sites, connectivity, exclude, work[:m1 - m0], dist2[m0:m1],
                        None if nearest is None else nearest[m0:m1], src_lut=src_lut)
    return dist2, nearest


def count_by_distance(src, other, K: int, connectivity: int, exclude: int, edges, hist, src_lut=None) -> None:
    """Add the confusion counts hist[bin][src class][other class] of `src` against `other` ([M, H, W] each), binned by the squared
    distance to the nearest class boundary of `src` (mode 1) at the thresholds `edges`, into `hist` (int64 [len(edges) + 1, K, K]) -
    from the launch that computes the distances.  Here dist2 is workspace too: M is walked in chunks of 6 bytes a pixel."""
    M, H, W = src.shape
    dev = src.device
    step = maps_per_chunk(H, W, 6)
    n = min(step, M)
    work = torch.empty(n, H, W, dtype=torch.int16, device=dev)
    dist2 = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    for m0 in range(0, M, step):
        m1 = min(m0 + step, M)
        launch_distance(src[m0:m1], K, TO_BOUNDARY, 0, connectivity, exclude, work[:m1 - m0], dist2[:m1 - m0], src_lut=src_lut,
                        other=other[m0:m1], edges=edges, hist=hist)


def run_band(src, K: int, threshold: int, connectivity: int, ignore_index: int, src_lut=None) -> torch.Tensor:
    """`src` ([M, H, W]) with every labelled pixel other than class `ignore_index` whose dist2 to the nearest class boundary (mode 1,
    `ignore_index` excluded) is at most `threshold` set to `ignore_index`.  With `src_lut` (int32 [256]) the classes are src_lut[src]
    and the result is stored as uint8 classes.  The band itself is a torch expression over dist2, chunk by chunk."""
    M, H, W = src.shape
    dev = src.device
    step = maps_per_chunk(H, W, 6 + (8 if src_lut is not None else 0))
    n = min(step, M)
    work = torch.empty(n, H, W, dtype=torch.int16, device=dev)
    dist2 = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    out = torch.empty_like(src)
    for m0 in range(0, M, step):
        m1 = min(m0 + step, M)
        part = src[m0:m1]
        launch_distance(part, K, TO_BOUNDARY, 0, connectivity, 1 << ignore_index, work[:m1 - m0], dist2[:m1 - m0], src_lut=src_lut)
        cls = part if src_lut is None else src_lut[part.long()]
        mark = (cls >= 0) & (cls < K) & (cls != ignore_index) & (dist2[:m1 - m0] <= threshold)
        out[m0:m1] = torch.where(mark, torch.full_like(cls, ignore_index), cls).to(src.dtype)
    return out


@torch.no_grad()
def distance_transform(class_map, num_classes: int, to="boundary", connectivity: int = 4, exclude=(), return_nearest: bool = False):
    """int32 SQUARED Euclidean distances of `class_map`'s shape (uint8 or int64, [M, H, W] or [H, W], on the GPU): for every pixel the
    squared distance to the nearest SITE of its own map, 0 at a site, NO_SITE where the map has none.  A pixel is labelled if its class
    lies in [0, num_classes) and not in `exclude`.  to="boundary": the sites are the labelled pixels with a labelled 4- or 8-neighbour
    of a different class (both sides of a boundary; unlabelled pixels make no boundary).  to=(ids): the labelled pixels of those classes.
    return_nearest=True adds the int32 linear index y * W + x of the nearest site (-1 where there is none); among equally near sites it
    is the one with the smallest index."""
    K, conn = check_classes(num_classes), check_connectivity(connectivity)
    eb = class_bits(exclude, K, "exclude")
    mode, sites = check_sites(to, K, eb)
    src = _check_map(class_map)
    _check_dims(src)
    if not src.is_cuda:
        raise RuntimeError("the distance transform runs on the GPU (there is no CPU fallback)")
    dist2, nearest = run_distance(src, K, mode, sites, conn, eb, bool(return_nearest))
    dist2 = dist2.view(class_map.shape)
    return (dist2, nearest.view(class_map.shape)) if return_nearest else dist2


@torch.no_grad()
def boundary_band(class_map, num_classes: int, distance, connectivity: int = 4, ignore_index: int = 0) -> torch.Tensor:
    """`class_map` with every labelled pixel within `distance` pixels (Euclidean: dist2 <= floor(distance^2)) of a class boundary set to
    `ignore_index`: the Euclidean sibling of `boundary_to_ignore`.  The boundaries are those of `distance_transform(...,
    to="boundary", exclude=(ignore_index,))`: a pixel that only touches the ignored class or a pixel outside [0, num_classes) is no
    boundary, so the ignored region does not grow on its own.  distance = 0 marks the boundary pixels themselves.  Same dtype and
    shape."""
    K, conn = check_classes(num_classes), check_connectivity(connectivity)
    threshold = squared_threshold(distance)
    ignore = check_ignore_index(ignore_index, K)
    src = _check_map(class_map)
    _check_dims(src)
    if not src.is_cuda:
        raise RuntimeError("the distance transform runs on the GPU (there is no CPU fallback)")
    return run_band(src, K, threshold, conn, ignore).view(class_map.shape)


@torch.no_grad()
def fill_nearest(class_map, num_classes: int, fill) -> torch.Tensor:
    """`class_map` with every pixel that lies outside [0, num_classes), or whose class is in `fill`, replaced by the class of its nearest
    pixel that is neither (of the smallest linear index among equally near ones, so the result is exact).  A map without such a pixel is
    returned unchanged.  `fill` must leave at least one class.  Same dtype and shape."""
    K = check_classes(num_classes)
    fb = class_bits(fill, K, "fill")
    sites = ((1 << K) - 1) & ~fb
    if sites == 0:
        raise ValueError("fill must leave at least one class to fill from")
    src = _check_map(class_map)
    _check_dims(src)
    if not src.is_cuda:
        raise RuntimeError("the distance transform runs on the GPU (there is no CPU fallback)")
    M, H, W = src.shape
    _, nearest = run_distance(src, K, TO_CLASSES, sites, 4, 0, True)
    flat = src.view(M, H * W)
    holes = (flat < 0) | (flat >= K) if src.dtype == torch.int64 else flat >= K
    for c in range(K):
        if (fb >> c) & 1:
            holes |= flat == c
    near = nearest.view(M, H * W).long()
    taken = torch.gather(flat, 1, near.clamp(min=0))
    return torch.where(holes & (near >= 0), taken, flat).view(class_map.shape)


# ---- confidence, abstention and the calibration sums (csrc/calibration.hip) -----------------------------------------------------------------
CAL_MAX_BINS, CAL_MAX_TEMPS = 64, 8
CAL_ONE = 1 << 20               # the quantum of the confidence and NLL sums: 2^-20 per pixel
CAL_MAX_GRID = 1024             # workgroups of one launch; a workgroup walks passes of 256 pixel quads
KINDS, MEASURES = _lib.CALIBRATION_MODES, _lib.CALIBRATION_MEASURES


def check_kind(kind) -> int:
    if kind not in KINDS:
        raise ValueError('kind must be "probs" or "logits"')
    return KINDS[kind]


def check_measure(measure) -> int:
    if measure not in MEASURES:
        raise ValueError('measure must be "max" or "margin"')
    return MEASURES[measure]


def check_bins(bins) -> int:
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= CAL_MAX_BINS:
        raise ValueError(f"bins must be an integer in 1..{CAL_MAX_BINS}")
    return bins


def check_temperature(temperature, kind: int = 1) -> float:
    """a finite temperature above 0 whose float32 value and reciprocal are too; probabilities (kind 0) take 1 only"""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or not 1e-30 <= temperature <= 1e30:
        raise ValueError("temperature must be a finite number in [1e-30, 1e30]")
    if kind == 0 and temperature != 1:
        raise ValueError("probabilities are taken as given: temperature must be 1 (scale the logits instead)")
    return float(temperature)


def check_scores(scores) -> torch.Tensor:
    """[N, K, H, W] view of float32 scores given as [N, K, H, W] or [K, H, W]"""
    if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32:
        raise ValueError("scores must be a float32 tensor")
    if scores.dim() not in (3, 4) or scores.numel() == 0:
        raise ValueError("scores must be [B, K, H, W] or [K, H, W] and not empty")
    s = scores.contiguous()
    s = s.view(1, *s.shape) if s.dim() == 3 else s
    check_classes(int(s.shape[1]))
    if s.shape[2] * s.shape[3] >= 1 << 31 or s.shape[0] * ((s.shape[2] * s.shape[3] + 3) // 4) >= 1 << 31:
        raise ValueError("scores: H * W and B * ceil(H * W / 4) must stay below 2^31")
    return s


def launch_calibration(scores, kind: int, temps, bins: int = 1, measure: int = 0, labels=None, label_lut=None, exclude: int = 0,
                       reject_below: float = 0.0, reject_to: int = -1, conf=None, pred=None, hist=None, totals=None, skipped=None) -> None:
    """One s2k_calibration launch over `scores` ([N, K, H, W] float32) on its device and current stream; labels [N, H, W] uint8 / int64."""
    if not scores.is_cuda:
        raise RuntimeError("calibration runs on the GPU (there is no CPU fallback)")
    N, K, H, W = scores.shape
    with torch.cuda.device(scores.device):
        _lib.check(_lib.calibration(scores, kind, labels, label_lut, (N, K, H * W), exclude, temps, bins, measure, reject_below, reject_to,
                                    conf, pred, hist, totals, skipped, torch.cuda.current_stream(scores.device).cuda_stream))


@torch.no_grad()
def confidence(scores, kind: str = "probs", measure: str = "max", temperature: float = 1.0, min_confidence=None, reject_to: int = 0,
               dtype=torch.int64):
    """(class_map, conf) of `scores` (float32 [B, K, H, W] or [K, H, W], on the GPU): the class of every pixel - the first maximum of its K
    scores, the rule of `TilePredictor.predict` - as `dtype` (int64 or uint8), and a float32 confidence raster.  kind="probs": the scores
    are probabilities and are taken as given; "logits": softmax(scores / temperature).  measure="max": the largest probability;
    "margin": its lead over the runner-up.  min_confidence=c: every pixel whose confidence is below c becomes class `reject_to` in the
    class map (an abstention; the reference's class 0, "other", is what its masked loss ignores).  One launch, scores read once."""
    k, m = check_kind(kind), check_measure(measure)
    T = check_temperature(temperature, k)
    if dtype not in (torch.int64, torch.uint8):
        raise ValueError("dtype must be torch.int64 or torch.uint8")
    s = check_scores(scores)
    K = int(s.shape[1])
    to = -1
    if min_confidence is not None:
        if isinstance(min_confidence, bool) or not isinstance(min_confidence, (int, float)) or math.isnan(min_confidence):
            raise ValueError("min_confidence must be None or a number")
        to = check_to(reject_to, K)
        if to < 0:
            raise ValueError(f"reject_to must be a class id in [0, {K})")
    if not s.is_cuda:
        raise RuntimeError("calibration runs on the GPU (there is no CPU fallback)")
    N, _, H, W = s.shape
    pred = torch.empty(N, H, W, dtype=dtype, device=s.device)
    conf = torch.empty(N, H, W, dtype=torch.float32, device=s.device)
    launch_calibration(s, k, [T], measure=m, reject_below=0.0 if min_confidence is None else float(min_confidence), reject_to=to, conf=conf,
                       pred=pred)
    shape = scores.shape[:-3] + scores.shape[-2:]
    return pred.view(shape), conf.view(shape)


# ---- exact polygon rasterisation into label tiles (csrc/rasterize.hip) ------------------------------------------------------------------------
RAST_Q = 256                    # fixed-point units per pixel
RAST_MAX_COORD = 2 ** 28        # largest magnitude of a vertex coordinate, and of 256 * a tile origin, in units
RAST_BLOCK_H, RAST_BLOCK_W = 32, 512    # the block of a tile one workgroup burns in LDS
RAST_BOX_INTS = 8               # ints of workspace per shape: its box in units, its ring range and its vertex range
RAST_DTYPES = (torch.uint8, torch.int32, torch.int64)
FILL, ONTO = _lib.RASTERIZE_MODES["fill"], _lib.RASTERIZE_MODES["onto"]


def quantise(coords) -> np.ndarray:
    """int64 units of float64 AOI-pixel coordinates: floor(v * 256 + 0.5); ValueError for a value that is not finite or whose units
    lie beyond +-RAST_MAX_COORD"""
    v = np.asarray(coords, dtype=np.float64)
    if not np.isfinite(v).all():
        raise ValueError("coordinates must be finite")
    q = np.floor(v * RAST_Q + 0.5)
    if q.size and np.abs(q).max() > RAST_MAX_COORD:
        raise ValueError(f"a coordinate lies beyond +-{RAST_MAX_COORD // RAST_Q} pixels (2^28 units)")
    return q.astype(np.int64)


def _ring(ring) -> np.ndarray:
    try:
        r = np.asarray(ring, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("a ring must be an [n, 2] array of coordinates") from None
    if r.ndim != 2 or r.shape[1] != 2:
        raise ValueError("a ring must be an [n, 2] array of coordinates")
    return r


class PolygonSet:
    """Polygons in the pixel frame of an area of interest (x to the right, y down, pixel (i, j) of a tile at origin (ox, oy) centred at
    (ox + j + 1/2, oy + i + 1/2)), quantised to 256 units per pixel and resident on `device` as the tables of s2k_rasterize
    (include/s2k.h).  `shapes`: a sequence of shapes, each a sequence of rings - exterior, holes and the parts of a multi-polygon alike;
    a centre is inside a shape by the even-odd rule over all of them - each ring an [n, 2] array-like of float64 (x, y) with n >= 3 and
    the closing edge implied.  A shape without rings covers nothing.  `values`: one integer per shape (None: the set can only burn shape
    indices).  Everything is checked and laid out in numpy on the host before the device is touched; the host copies stay in `host`."""

    def __init__(self, shapes, values=None, device="cuda"):
        try:
            shapes = [list(rings) for rings in shapes]
        except TypeError:
            raise ValueError("shapes must be a sequence of shapes, each a sequence of rings") from None
        rings = [[_ring(r) for r in sh] for sh in shapes]
        if any(len(r) < 3 for sh in rings for r in sh):
            raise ValueError("a ring needs at least 3 vertices (the closing edge is implied)")
        flat = [r for sh in rings for r in sh]
        verts = quantise(np.concatenate(flat, axis=0) if flat else np.zeros((0, 2))).astype(np.int32)
        ring_start = np.zeros(len(flat) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in flat], out=ring_start[1:])
        if ring_start[-1] >= 1 << 31:
            raise ValueError("too many vertices (V must stay below 2^31)")
        ring_shape = np.repeat(np.arange(len(rings), dtype=np.int32), [len(sh) for sh in rings]) if rings else np.zeros(0, np.int32)
        if values is not None:
            try:
                vals = np.asarray(values)
            except (TypeError, ValueError):
                raise ValueError("values must be one integer per shape") from None
            if vals.shape != (len(rings),) or (vals.size and vals.dtype.kind not in "iu"):
                raise ValueError("values must be one integer per shape")
            vals = vals.astype(np.int64)
            if vals.size and (vals.min() < -(1 << 31) or vals.max() >= 1 << 31):
                raise ValueError("values must fit int32")
            values = vals.astype(np.int32)
        self._shapes = len(rings)
        self.host = {"verts": verts.reshape(-1, 2), "ring_start": ring_start.astype(np.int32), "ring_shape": ring_shape, "values": values}
        self.device = torch.device(device)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)      # noqa: E731
        # one spare element each: an empty table still has an address
        self.verts = dev(np.concatenate([self.host["verts"], np.zeros((1, 2), np.int32)]))
        self.ring_start = dev(self.host["ring_start"])
        self.ring_shape = dev(np.concatenate([ring_shape, np.zeros(1, np.int32)]))
        self.values = None if values is None else dev(np.concatenate([values, np.zeros(1, np.int32)]))

    @classmethod
    def from_world(cls, shapes, values, west: float, north: float, xsize: float, ysize: float, device="cuda") -> "PolygonSet":
        """`shapes` in world coordinates through the reference's `from_origin(west, north, xsize, ysize)` transform:
        px = (x - west) / xsize, py = (north - y) / ysize."""
        for v in (west, north, xsize, ysize):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError("west, north, xsize and ysize must be finite numbers")
        if xsize <= 0 or ysize <= 0:
            raise ValueError("xsize and ysize must be positive")
        try:
            shapes = [list(rings) for rings in shapes]
        except TypeError:
            raise ValueError("shapes must be a sequence of shapes, each a sequence of rings") from None
        out = []
        for sh in shapes:
            out.append([])
            for ring in sh:
                r = _ring(ring)
                out[-1].append(np.stack([(r[:, 0] - west) / xsize, (north - r[:, 1]) / ysize], axis=1))
        return cls(out, values, device)

    @classmethod
    def from_geojson(cls, geometries, values, west=None, north=None, xsize=None, ysize=None, device="cuda") -> "PolygonSet":
        """One shape per GeoJSON-style geometry: a mapping {"type": "Polygon" | "MultiPolygon", "coordinates": ...} (what
        `shapely.geometry.mapping` gives) or an object with `__geo_interface__`.  The repeated closing vertex of a ring is dropped;
        coordinates beyond x and y are ignored.  Any other geometry type is a ValueError.  With west, north, xsize and ysize the
        coordinates are world coordinates (`from_world`), without them AOI pixels."""
        shapes = []
        for g in geometries:
            g = getattr(g, "__geo_interface__", g)
            try:
                kind, coords = g["type"], g["coordinates"]
            except (TypeError, KeyError):
                raise ValueError('a geometry must be a mapping with "type" and "coordinates"') from None
            if kind == "Polygon":
                polys = [coords]
            elif kind == "MultiPolygon":
                polys = list(coords)
            else:
                raise ValueError(f"geometry type {kind!r}: only Polygon and MultiPolygon are rasterised")
            rings = []
            for poly in polys:
                for ring in poly:
                    try:
                        r = np.asarray(ring, dtype=np.float64)
                    except (TypeError, ValueError):
                        raise ValueError("a ring must be an [n, 2] array of coordinates") from None
                    if r.ndim != 2 or r.shape[1] < 2:
                        raise ValueError("a ring must be an [n, 2] array of coordinates")
                    r = r[:, :2]
                    if len(r) > 1 and np.array_equal(r[0], r[-1]):
                        r = r[:-1]
                    rings.append(r)
            shapes.append(rings)
        world = (west, north, xsize, ysize)
        if all(v is None for v in world):
            return cls(shapes, values, device)
        if any(v is None for v in world):
            raise ValueError("give west, north, xsize and ysize together, or none of them")
        return cls.from_world(shapes, values, west, north, xsize, ysize, device)

    @property
    def num_shapes(self) -> int:
        return self._shapes

    @property
    def num_rings(self) -> int:
        return len(self.host["ring_shape"])

    @property
    def num_vertices(self) -> int:
        return len(self.host["verts"])


def rasterize_workspace_bytes(M: int, S: int) -> int:
    """s2k_rasterize_workspace(M, S): RAST_BOX_INTS ints per shape, M list lengths, M * S list entries"""
    return 4 * (RAST_BOX_INTS * S + M + M * S)


def tiles_per_chunk(S: int, max_workspace_bytes: int) -> int:
    """tiles whose workspace over S shapes stays within `max_workspace_bytes` (at least one)"""
    return max(1, (max_workspace_bytes - 4 * RAST_BOX_INTS * S) // (4 * (S + 1)))


def check_origins(origins, M=None):
    """`origins` as an int32 [M, 2] tensor.  What lies on the host is range-checked here (256 * origin within +-RAST_MAX_COORD); a device
    tensor is taken as it is: the kernels check it and report through the status word."""
    if isinstance(origins, torch.Tensor):
        o = origins
        if o.dtype not in (torch.int32, torch.int64) or o.dim() != 2 or o.shape[1] != 2 or o.shape[0] < 1:
            raise ValueError("origins must be an integer [M, 2] tensor or sequence of (ox, oy), M >= 1")
    else:
        try:
            a = np.asarray(origins)
        except (TypeError, ValueError):
            raise ValueError("origins must be an integer [M, 2] tensor or sequence of (ox, oy), M >= 1") from None
        if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1 or a.dtype.kind not in "iu":
            raise ValueError("origins must be an integer [M, 2] tensor or sequence of (ox, oy), M >= 1")
        o = torch.from_numpy(a.astype(np.int64))
    if not o.is_cuda and int(o.abs().max()) > RAST_MAX_COORD // RAST_Q:
        raise ValueError(f"an origin lies beyond +-{RAST_MAX_COORD // RAST_Q} pixels")
    if M is not None and o.shape[0] != M:
        raise ValueError(f"origins must hold one (ox, oy) per tile: {M}, got {o.shape[0]}")
    return o.to(torch.int32).contiguous()


def raise_rasterize_status(status: torch.Tensor) -> None:
    """The one host read of a rasterisation: S2kError if the kernels met tables the host could not see."""
    code = int(status.item())
    if code:
        raise _lib.S2kError(f"rasterize: status {code:#x} (1 ring tables out of order or range, 2 a vertex beyond 2^28 units, 4 an origin "
                            "beyond 2^20 pixels): the outputs are not to be used")


@torch.no_grad()
def rasterize(polygons, origins, size=None, fill=0, out=None, dtype=torch.uint8, burn: str = "value", return_unfilled: bool = False,
              max_workspace_bytes: int = 256 << 20):
    """[M, H, W] rasters of `polygons` (a PolygonSet), one per tile origin (ox, oy) in `origins` ([M, 2] ints, a sequence or a tensor),
    each of size = (H, W): a pixel whose centre is inside a shape - even-odd over the shape's rings, the top-left rule on its edges,
    exact in fixed point (include/s2k.h at s2k_rasterize) - takes the value of the LAST such shape, as the reference's
    rasterio.features.rasterize does; burn="index" burns the shape index instead (int32 / int64 only: a zone raster).  A pixel inside
    no shape gets `fill`, in a new tensor of `dtype` (uint8, int32 or int64).  out=[M, H, W] (uint8, int32 or int64, contiguous, on the
    GPU): burn ONTO it and leave the pixels inside no shape as they are; `fill` must then be None, and `size`, if given, out's own.
    Values and fill must fit the raster's dtype.  return_unfilled=True adds int64 [M]: the pixels of every tile inside no shape (the
    numerator of the reference's MAX_UNLABELED test).  The tiles are walked in chunks whose workspace (a list of candidate shapes per
    tile) stays within `max_workspace_bytes`, at least one tile a chunk; three launches a chunk, and one status read at the end."""
    if not isinstance(polygons, PolygonSet):
        raise ValueError("polygons must be a PolygonSet")
    if burn not in _lib.RASTERIZE_BURN:
        raise ValueError('burn must be "value" or "index"')
    if isinstance(max_workspace_bytes, bool) or not isinstance(max_workspace_bytes, int) or max_workspace_bytes < 1:
        raise ValueError("max_workspace_bytes must be a positive integer")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype not in RAST_DTYPES or out.dim() != 3 or out.numel() == 0 or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8, int32 or int64 [M, H, W] tensor")
        if fill is not None:
            raise ValueError("fill must be None with out: pixels inside no shape keep what out holds")
        if size is not None and tuple(int(v) for v in size) != tuple(out.shape[1:]):
            raise ValueError("size differs from out's")
        dtype, (H, W) = out.dtype, out.shape[1:]
    else:
        if dtype not in RAST_DTYPES:
            raise ValueError("dtype must be torch.uint8, torch.int32 or torch.int64")
        try:
            H, W = size
        except (TypeError, ValueError):
            raise ValueError("size must be (H, W)") from None
        if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in (H, W)) or H * W >= 1 << 31:
            raise ValueError("size must be (H, W), positive integers with H * W below 2^31")
        lo, hi = (0, 255) if dtype == torch.uint8 else (-(1 << 31), (1 << 31) - 1)
        if isinstance(fill, bool) or not isinstance(fill, int) or not lo <= fill <= hi:
            raise ValueError(f"fill must be an integer in [{lo}, {hi}] for {dtype}")
    o = check_origins(origins, None if out is None else out.shape[0])
    M, S = int(o.shape[0]), polygons.num_shapes
    if burn == "index":
        if dtype == torch.uint8:
            raise ValueError('burn="index" needs an int32 or int64 raster')
    else:
        vals = polygons.host["values"]
        if vals is None:
            raise ValueError('the PolygonSet holds no values: burn="index" is all it can do')
        if dtype == torch.uint8 and vals.size and (vals.min() < 0 or vals.max() > 255):
            raise ValueError("values must lie in 0..255 for a uint8 raster")
    if M * ((H + RAST_BLOCK_H - 1) // RAST_BLOCK_H) * ((W + RAST_BLOCK_W - 1) // RAST_BLOCK_W) >= 1 << 31:
        raise ValueError("too many tiles for one call")
    if not polygons.verts.is_cuda or (out is not None and not out.is_cuda):
        raise RuntimeError("polygons are rasterised on the GPU (there is no CPU fallback)")
    dev = polygons.device
    if out is not None and out.device != polygons.verts.device:
        raise ValueError("out and the polygons are on different devices")
    o = o.to(dev)
    dst = out if out is not None else torch.empty(M, H, W, dtype=dtype, device=dev)
    unfilled = torch.zeros(M, dtype=torch.int64, device=dev) if return_unfilled else None
    status = new_status(dev)
    step = min(M, tiles_per_chunk(S, max_workspace_bytes))
    work = torch.empty(rasterize_workspace_bytes(step, S) // 4, dtype=torch.int32, device=dev)
    mode, b = (ONTO if out is not None else FILL), _lib.RASTERIZE_BURN[burn]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for m0 in range(0, M, step):
            m1 = min(m0 + step, M)
            _lib.check(_lib.rasterize(polygons.verts, polygons.ring_start, polygons.ring_shape, polygons.values, o[m0:m1], dst[m0:m1],
                                      (polygons.num_vertices, polygons.num_rings, S, m1 - m0, H, W), mode, b, 0 if fill is None else fill, work,
                                      None if unfilled is None else unfilled[m0:m1], status, stream))
    raise_rasterize_status(status)
    return (dst, unfilled) if return_unfilled else dst
