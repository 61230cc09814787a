"""Zonal statistics on the GPU: what a raster holds inside every polygon, or inside every component of another map.

`classmap.rasterize` puts polygons into rasters; with burn="index" it writes a ZONE raster, the polygon index per pixel.  This module
takes things out of a raster per zone, which is the question a land-cover user with OSM polygons asks next: what did the model predict
inside each parcel (class votes per polygon, the majority class per polygon, and that class painted back - object-based classification,
which removes salt-and-pepper along boundaries the user already has), what do the Sentinel-2 bands look like inside each polygon (count,
mean, std, min, max per band: the questions the reference's calculate_dataset_statistics.py and experiments/label_EDA.py ask per dataset
and per tile, asked per object), and how many pixels of each label class lie in each zone.  The labels of
`classmap.connected_components` are zone rasters too, with ids per map (per_map=True, num_zones = H * W).

    zones = classmap.rasterize(ps, origins, (512, 512), fill=-1, dtype=torch.int32, burn="index")
    hist  = histogram(zones, class_map, num_zones, num_classes)              # int64 [Z, K]; [M, Z, K] with per_map=True
    stats = band_stats(zones, tiles, num_zones, nodata=0)                    # ZonalStats(count, sum, sumsq, min, max), .mean() / .std()
    cls   = majority(hist, votes=(1, 2, 3), min_count=8, fill=-1)            # int32 [Z]: the lowest class with the most votes
    out   = paint(zones, cls, fill=0)                                        # uint8 [M, H, W]; out=... paints onto what is there
    clean = majority_by_zone(class_map, zones, num_zones, num_classes)       # pixels outside every zone keep their class

The torch expressions of the same - bincount(zone * K + cls), index_add_, scatter_reduce - put one global atomic per pixel on addresses
that are hot because a large polygon is ONE address, need int64 temporaries of the whole raster, and their float sums depend on the
order of arrival.  Here the work is integer work with one exact answer (csrc/zonal.hip; the definitions are in include/s2k.h at
s2k_zonal_histogram): one launch streams the rasters once, a workgroup owns a ZONAL_BLOCK_H x ZONAL_BLOCK_W block of a map and, because
zones are spatially coherent, counts in an LDS table of ZONAL_SLOTS zone keys (open addressing from `home_slot(key)`, ZONAL_PROBES
probes), so that a block issues one global atomic per non-empty (zone, bin) pair instead of one per pixel; a pixel that finds no slot
goes to global memory directly.  A negative zone value means "no zone" (the fill=-1 convention); a value at or above `num_zones` is
skipped on the device and reported: the one host read of a public call is the status word, at its end, and `_lib.S2kError` is raised
if it is set.  `GpuTilePipeline.zonal_label_histogram`, `zonal_band_stats` and `TilePredictor.predict_zones` are built on these.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from . import classmap as CM

ZONAL_BLOCK_H, ZONAL_BLOCK_W = 16, 256      # the block one workgroup owns (csrc/zonal.hip)
ZONAL_SLOT_BITS = 6
ZONAL_SLOTS = 64                            # keys of a workgroup's LDS table
ZONAL_PROBES = 8                            # slots tried from the home slot on before a pixel goes to global memory
ZONAL_HASH = 2654435761
ZONAL_BAD_ZONE = 1                          # status: a zone value at or above the limit was met
MAX_BANDS = 16
PAINT_DTYPES = (torch.uint8, torch.int32, torch.int64)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
FILL, KEEP = _lib.ZONAL_PAINT_MODES["fill"], _lib.ZONAL_PAINT_MODES["keep"]


def home_slot(key: int) -> int:
    """the slot of the LDS table where the probing for `key` starts (zonal_home in csrc/zonal.hip)"""
    return ((int(key) * ZONAL_HASH) & 0xffffffff) >> (32 - ZONAL_SLOT_BITS)


# ---- argument checks: ValueError, before anything asks where the tensors live -----------------------------------------------------------------
def _check_zones(zones) -> torch.Tensor:
    """[M, H, W] view of an int32 / int64 zone raster given as [M, H, W] or [H, W]"""
    if not isinstance(zones, torch.Tensor) or zones.dtype not in (torch.int32, torch.int64):
        raise ValueError("zones must be an int32 or int64 tensor")
    if zones.dim() not in (2, 3) or zones.numel() == 0:
        raise ValueError("zones must be [M, H, W] or [H, W] and not empty")
    z = zones.contiguous()
    z = z.view(1, *z.shape) if z.dim() == 2 else z
    if z.shape[1] * z.shape[2] >= 1 << 31:
        raise ValueError("H * W must stay below 2^31")
    return z


def _check_num_zones(num_zones, M: int, per_map: bool) -> tuple[int, int]:
    """(Z, zone_stride): the rows of the tables and the C entries' stride"""
    if isinstance(num_zones, bool) or not isinstance(num_zones, int) or not 1 <= num_zones <= INT32_MAX:
        raise ValueError("num_zones must be a positive integer below 2^31")
    if not per_map:
        return num_zones, 0
    if M * num_zones > INT32_MAX:
        raise ValueError(f"per_map: M * num_zones = {M * num_zones} rows must stay below 2^31")
    return M * num_zones, num_zones


def _check_table_bytes(Z: int, row_bytes: int, per_map: bool) -> None:
    if per_map and Z * row_bytes > CM.WORKSPACE_BYTES:
        raise ValueError(f"per_map: the output tables would take {Z * row_bytes} bytes ({Z} rows of {row_bytes}), above "
                         f"classmap.WORKSPACE_BYTES = {CM.WORKSPACE_BYTES}: pass fewer maps per call")


def _check_grid(M: int, H: int, W: int) -> None:
    if M * ((H + ZONAL_BLOCK_H - 1) // ZONAL_BLOCK_H) * ((W + ZONAL_BLOCK_W - 1) // ZONAL_BLOCK_W) >= 1 << 31:
        raise ValueError("too many maps for one call")


def _check_count(min_count) -> int:
    if isinstance(min_count, bool) or not isinstance(min_count, int) or not 1 <= min_count < 1 << 63:
        raise ValueError("min_count must be a positive integer")
    return min_count


def _check_int(v, lo: int, hi: int, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{what} must be an integer in [{lo}, {hi}]")
    return v


def _check_lut(lut, src):
    if lut is None:
        return None
    if not isinstance(lut, torch.Tensor) or lut.dtype != torch.int32 or lut.shape != (256,) or not lut.is_contiguous():
        raise ValueError("lut must be a contiguous int32 [256] tensor")
    if src.dtype != torch.uint8:
        raise ValueError("lut needs a uint8 class map")
    return lut


def _same_device(*tensors) -> None:
    dev = tensors[0].device
    if any(t is not None and t.device != dev for t in tensors):
        raise ValueError("the tensors are on different devices")


def _need_gpu(*tensors) -> None:
    if any(t is not None and not t.is_cuda for t in tensors):
        raise RuntimeError("zonal statistics run on the GPU (there is no CPU fallback)")


def raise_status(status: torch.Tensor) -> None:
    """The one host read of a public call: S2kError if a zone value at or above the limit was met."""
    code = int(status.item())
    if code:
        raise _lib.S2kError(f"zonal: status {code:#x} (1 a zone value at or above num_zones): such pixels were skipped")


# ---- launches: one C entry each, on the zone raster's device and current stream, no host read -------------------------------------------------
def launch_histogram(zones, stride: int, src, Z: int, K: int, hist, status, src_lut=None) -> None:
    """One s2k_zonal_histogram launch: `zones` and `src` [M, H, W], `hist` int64 [Z, K] (any shape of Z * K elements), added to."""
    _need_gpu(zones, src, hist)
    M, H, W = zones.shape
    with torch.cuda.device(zones.device):
        _lib.check(_lib.zonal_histogram(zones, stride, src, src_lut, (M, H, W, Z, K), hist, status,
                                        torch.cuda.current_stream(zones.device).cuda_stream))


def launch_bands(zones, stride: int, vals, Z: int, nodata, stats: "ZonalStats", status) -> None:
    """One s2k_zonal_bands launch: `vals` int16 [M, C, H, W], the five tables of `stats` added to / combined into."""
    _need_gpu(zones, vals, stats.count)
    M, C, H, W = vals.shape
    with torch.cuda.device(zones.device):
        _lib.check(_lib.zonal_bands(zones, stride, vals, (M, C, H, W, Z), nodata, stats.count, stats.sum, stats.sumsq, stats.min, stats.max,
                                    status, torch.cuda.current_stream(zones.device).cuda_stream))


def launch_majority(hist, Z: int, K: int, votes: int, min_count: int, fill: int, out_cls, out_best=None) -> None:
    """One s2k_zonal_majority launch over `hist` (int64, Z * K elements) into `out_cls` (int32, Z elements)."""
    _need_gpu(hist, out_cls)
    with torch.cuda.device(hist.device):
        _lib.check(_lib.zonal_majority(hist, (Z, K), votes, min_count, fill, out_cls, out_best,
                                       torch.cuda.current_stream(hist.device).cuda_stream))


def launch_paint(zones, stride: int, table, Z: int, dst, mode: int, fill: int, status) -> None:
    """One s2k_zonal_paint launch of `table` (int32, Z elements) through `zones` into `dst` ([M, H, W], uint8, int32 or int64)."""
    _need_gpu(zones, table, dst)
    M, H, W = zones.shape
    with torch.cuda.device(zones.device):
        _lib.check(_lib.zonal_paint(zones, stride, table, (M, H, W, Z), dst, mode, fill, status,
                                    torch.cuda.current_stream(zones.device).cuda_stream))


# ---- public functions -------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def histogram(zones, class_map, num_zones: int, num_classes: int, per_map: bool = False, lut=None, out=None) -> torch.Tensor:
    """int64 [num_zones, num_classes]: how many pixels of every class of `class_map` (uint8 or int64, the shape of `zones`) lie in every
    zone of `zones` (int32 or int64, [M, H, W] or [H, W], on the GPU).  A negative zone value is no zone; a class outside
    [0, num_classes) is not counted; `lut` (int32 [256]) reads a uint8 class map through a table.  per_map=True: zone values are ids
    inside their own map - `connected_components` labels with num_zones = H * W - and the result is [M, num_zones, num_classes].
    out=: an int64 tensor of the result's shape that is ADDED to (and returned), so that rasters too many for one call accumulate."""
    K = CM.check_classes(num_classes)
    z = _check_zones(zones)
    src = CM._check_map(class_map)
    if src.shape != z.shape:
        raise ValueError("class_map and zones must have the same shape")
    table = _check_lut(lut, src)
    Z, stride = _check_num_zones(num_zones, z.shape[0], per_map)
    shape = (z.shape[0], num_zones, K) if per_map else (num_zones, K)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int64 tensor of shape {shape}")
    _check_table_bytes(Z, 8 * K, per_map)
    _check_grid(*z.shape)
    _same_device(z, src, table, out)
    _need_gpu(z)
    hist = out if out is not None else torch.zeros(shape, dtype=torch.int64, device=z.device)
    status = CM.new_status(z.device)
    launch_histogram(z, stride, src, Z, K, hist, status, table)
    raise_status(status)
    return hist


@dataclass
class ZonalStats:
    """The five exact tables of `band_stats`, each [num_zones, C] ([M, num_zones, C] with per_map) on the device: `count`, `sum` and
    `sumsq` int64, `min` and `max` int32.  A (zone, band) without a counted value has count 0 and keeps min = 2^31 - 1 and
    max = -2^31."""
    count: torch.Tensor
    sum: torch.Tensor
    sumsq: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor

    def mean(self) -> torch.Tensor:
        """float64, NaN where count == 0"""
        n = self.count.double()
        return torch.where(self.count > 0, self.sum.double() / n, torch.full_like(n, float("nan")))

    def std(self) -> torch.Tensor:
        """float64 population standard deviation sqrt(sumsq / n - mean^2), NaN where count == 0"""
        n = self.count.double()
        m = self.sum.double() / n
        var = (self.sumsq.double() / n - m * m).clamp_min(0.0)
        return torch.where(self.count > 0, var.sqrt(), torch.full_like(n, float("nan")))


def new_stats(shape, device) -> ZonalStats:
    """empty tables: zero counts and sums, min = 2^31 - 1, max = -2^31"""
    z64 = lambda: torch.zeros(shape, dtype=torch.int64, device=device)      # noqa: E731
    return ZonalStats(z64(), z64(), z64(), torch.full(shape, INT32_MAX, dtype=torch.int32, device=device),
                      torch.full(shape, INT32_MIN, dtype=torch.int32, device=device))


@torch.no_grad()
def band_stats(zones, tiles, num_zones: int, nodata=None, per_map: bool = False) -> ZonalStats:
    """`ZonalStats` of the int16 rasters `tiles` ([M, C, H, W], or [C, H, W] with zones [H, W]; 1 <= C <= 16: the pipeline's resident
    tiles) inside every zone of `zones`: per zone and band the number of values, their sum, their sum of squares, their minimum and
    maximum - all exact integers.  nodata=v: a band value equal to v is left out, for that band only.  per_map as in `histogram`."""
    z = _check_zones(zones)
    if not isinstance(tiles, torch.Tensor) or tiles.dtype != torch.int16 or tiles.dim() not in (3, 4) or tiles.numel() == 0:
        raise ValueError("tiles must be an int16 [M, C, H, W] or [C, H, W] tensor")
    v = tiles.contiguous()
    v = v.view(1, *v.shape) if v.dim() == 3 else v
    if zones.dim() != tiles.dim() - 1 or (v.shape[0],) + tuple(v.shape[2:]) != tuple(z.shape):
        raise ValueError("tiles must be [M, C, H, W] for zones [M, H, W]")
    C = v.shape[1]
    if not 1 <= C <= MAX_BANDS:
        raise ValueError(f"tiles must hold 1..{MAX_BANDS} bands")
    nd = None if nodata is None else _check_int(nodata, INT32_MIN, INT32_MAX, "nodata")
    Z, stride = _check_num_zones(num_zones, z.shape[0], per_map)
    _check_table_bytes(Z, 32 * C, per_map)
    _check_grid(*z.shape)
    _same_device(z, v)
    _need_gpu(z)
    stats = new_stats((z.shape[0], num_zones, C) if per_map else (num_zones, C), z.device)
    status = CM.new_status(z.device)
    launch_bands(z, stride, v, Z, nd, stats, status)
    raise_status(status)
    return stats


def _check_hist(hist) -> tuple[int, int]:
    if not isinstance(hist, torch.Tensor) or hist.dtype != torch.int64 or hist.dim() not in (2, 3) or hist.numel() == 0:
        raise ValueError("hist must be a non-empty int64 [Z, K] or [M, Z, K] tensor")
    if not hist.is_contiguous():
        raise ValueError("hist must be contiguous")
    K = CM.check_classes(int(hist.shape[-1]))
    Z = hist.numel() // K
    if Z > INT32_MAX:
        raise ValueError("hist must have fewer than 2^31 rows")
    return Z, K


@torch.no_grad()
def majority(hist, votes=None, min_count: int = 1, fill: int = -1, return_count: bool = False):
    """int32 [Z] ([M, Z] for a per_map histogram): per row of `hist` (int64 [Z, K]) the LOWEST class among those with the most votes -
    only the classes in `votes` vote (None: all) - or `fill` where the most is below `min_count` (an empty zone, with the default).
    return_count=True adds int64 of the same shape: that largest count.  No host read."""
    Z, K = _check_hist(hist)
    vb = CM.class_bits(votes, K, "votes")
    if vb == 0:
        raise ValueError("votes must name at least one class")
    n, f = _check_count(min_count), _check_int(fill, INT32_MIN, INT32_MAX, "fill")
    _need_gpu(hist)
    cls = torch.empty(hist.shape[:-1], dtype=torch.int32, device=hist.device)
    best = torch.empty(hist.shape[:-1], dtype=torch.int64, device=hist.device) if return_count else None
    launch_majority(hist, Z, K, vb, n, f, cls, best)
    return (cls, best) if return_count else cls


def _check_paint_table(table, M: int, per_map: bool) -> tuple[int, int]:
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.numel() == 0 or not table.is_contiguous():
        raise ValueError("table must be a non-empty contiguous int32 tensor")
    if per_map:
        if table.dim() != 2 or table.shape[0] != M:
            raise ValueError(f"per_map: table must be [M, num_zones] with M = {M}")
        return _check_num_zones(int(table.shape[1]), M, True)
    if table.dim() != 1:
        raise ValueError("table must be [num_zones]")
    return _check_num_zones(int(table.shape[0]), M, False)


@torch.no_grad()
def paint(zones, table, fill: int = 0, out=None, dtype=torch.uint8, per_map: bool = False) -> torch.Tensor:
    """The raster of `zones`' shape in which every pixel holds its zone's entry of `table` (int32 [num_zones]; [M, num_zones] with
    per_map) - `majority`'s classes, usually.  A pixel in no zone, or whose entry is negative, gets `fill` in a new tensor of `dtype`
    (uint8, int32 or int64).  out= (a contiguous tensor of zones' shape, uint8, int32 or int64): paint ONTO it, such pixels keeping what
    it holds; `fill` is then not used and must be left at 0.  Entries must fit the raster's dtype (a uint8 raster takes the low byte)."""
    z = _check_zones(zones)
    Z, stride = _check_paint_table(table, z.shape[0], per_map)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype not in PAINT_DTYPES or tuple(out.shape) != tuple(zones.shape) or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8, int32 or int64 tensor of zones' shape")
        if fill != 0 or isinstance(fill, bool):
            raise ValueError("fill is not used with out: leave it at 0")
        dtype = out.dtype
    else:
        if dtype not in PAINT_DTYPES:
            raise ValueError("dtype must be torch.uint8, torch.int32 or torch.int64")
        lo, hi = (0, 255) if dtype == torch.uint8 else (INT32_MIN, INT32_MAX)
        _check_int(fill, lo, hi, f"fill ({dtype})")
    if z.numel() > 256 * INT32_MAX:
        raise ValueError("too many pixels for one call")
    _same_device(z, table, out)
    _need_gpu(z)
    dst = out if out is not None else torch.empty(zones.shape, dtype=dtype, device=z.device)
    status = CM.new_status(z.device)
    launch_paint(z, stride, table, Z, dst.view(z.shape), KEEP if out is not None else FILL, fill, status)
    raise_status(status)
    return dst


@torch.no_grad()
def majority_by_zone(class_map, zones, num_zones: int, num_classes: int, votes=None, min_count: int = 1) -> torch.Tensor:
    """Object-based classification: `class_map` (uint8 or int64) with every pixel of a zone set to the zone's majority class -
    `paint(zones, majority(histogram(zones, class_map, ...), votes, min_count), out=class_map.clone())`: three launches and one host
    read.  Pixels outside every zone keep their class, and so do the pixels of a zone whose best voting class has fewer than
    `min_count` pixels.  `class_map` is left as it is."""
    K = CM.check_classes(num_classes)
    z = _check_zones(zones)
    src = CM._check_map(class_map)
    if tuple(class_map.shape) != tuple(zones.shape):
        raise ValueError("class_map and zones must have the same shape")
    Z, _ = _check_num_zones(num_zones, z.shape[0], False)
    vb = CM.class_bits(votes, K, "votes")
    if vb == 0:
        raise ValueError("votes must name at least one class")
    n = _check_count(min_count)
    _check_grid(*z.shape)
    _same_device(z, src)
    _need_gpu(z)
    src = src.view(z.shape)
    hist = torch.zeros(Z, K, dtype=torch.int64, device=z.device)
    cls = torch.empty(Z, dtype=torch.int32, device=z.device)
    out = src.clone()
    status = CM.new_status(z.device)
    launch_histogram(z, 0, src, Z, K, hist, status)
    launch_majority(hist, Z, K, vb, n, -1, cls)
    launch_paint(z, 0, cls, Z, out, KEEP, 0, status)
    raise_status(status)
    return out.view(class_map.shape)
