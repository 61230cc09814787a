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
"""
from __future__ import annotations

import torch

from . import _lib

MAX_CLASSES = 32        # four byte counters to a dword, at most eight dwords of window histogram in registers
MIN_SIZE, MAX_SIZE = 3, 15      # 15 x 15 = 225 votes still fit a byte counter
STRIP = 64              # columns a wave holds (CLASSMAP_STRIP): STRIP - 2 * (size // 2) of them are outputs
BAND = 16               # output rows a wave walks (CLASSMAP_BAND)
MAJORITY, BOUNDARY = _lib.CLASSMAP_MODES["majority"], _lib.CLASSMAP_MODES["boundary"]


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
