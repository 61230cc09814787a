"""Host side of the tile quicklooks: the rank / fraction derivation of numpy's linear percentile, the argument validators of
`GpuTilePipeline.band_percentiles` / `.zero_fraction` / `.quicklook`, `render.overlay` and `TilePredictor.render`, and the stage calls
behind them (`run_selection`, `run_zero_count`, `add_quicklook`; stage_call.py).  Pure host code except the two `run_*`, which launch.

What it replaces in the reference: the picture side of `log_image_metrics` / `_log_segmentation_pred`
(src/train_segmentation.py:166-219) and src/plotting.py:75-96,

    p2, p98 = np.percentile(image, q=(2, 98))                   # image = three bands of ONE tile, all pixels jointly
    image   = np.clip((image - p2) / (p98 - p2) * 255, 0, 255).astype(np.uint8)

and the per-tile zero-pixel share of src/experiments/sentinel_EDA.py:20-27.  The percentile is an exact order statistic: stages
TILE_RADIX_HIST / TILE_RANK_PICK (plan/opdefs.py, csrc/quicklook.hip) select sorted(group)[rank] for up to eight ranks without a sort,
and interpolate pairs of them exactly as numpy does.  The host only turns a percentile into its two ranks and its fraction:

    vi = (q / 100) * (N - 1);  lo = floor(vi);  hi = min(lo + 1, N - 1);  t = vi - lo          (float64, numpy's own steps)
    percentile = a + (b - a) * t,  and  b - (b - a) * (1 - t)  where t >= 0.5;   a, b = sorted[lo], sorted[hi]

numpy evaluates `b - a` in the ARRAY's dtype: on an int16 image two neighbouring order statistics further apart than 32767 wrap
around silently.  Here a and b are exact integers held as float64, so the result is `np.percentile` of the values as float64.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..plan.program import TRef
from ..stage_call import StageCall

MAX_RANKS = 8          # ranks per selection program (TILE_RANK_PICK's R): four percentiles
MAX_BANDS = 16         # TILE_RADIX_HIST's NBND
ZERO_BUCKET = (0 + 32768) >> 8      # the coarse bin of the value 0: key(0) >> 8 = 128; its fine bin is 0


def key(v):
    """The order-preserving radix key of int16 values: (uint16)(v + 32768), as int64."""
    return np.asarray(v).astype(np.int64) + 32768


def check_q(q) -> list[float]:
    """Percentiles as a list of floats in [0, 100] (a scalar counts as one)."""
    qs = [float(v) for v in np.asarray(q, dtype=np.float64).reshape(-1)]
    if not qs or any(not (0.0 <= v <= 100.0) for v in qs):      # a NaN fails both comparisons
        raise ValueError("percentiles must lie in [0, 100] (and at least one is needed)")
    return qs


def check_bands(bands, C: int, count: int | None = None) -> list[int]:
    """Band indices as a list: distinct, inside [0, C), at most MAX_BANDS (exactly `count` when given)."""
    try:
        bl = [int(b) for b in bands]
    except TypeError as e:
        raise ValueError("bands must be a sequence of band indices") from e
    if count is not None and len(bl) != count:
        raise ValueError(f"exactly {count} bands are needed")
    if not 1 <= len(bl) <= MAX_BANDS or len(set(bl)) != len(bl) or any(not 0 <= b < C for b in bl):
        raise ValueError(f"bands must be 1..{MAX_BANDS} distinct indices in [0, {C})")
    return bl


def rank_plan(q, N: int) -> tuple[list[int], list[float]]:
    """(ranks [2 * len(q)], frac [len(q)]): per percentile the zero-based ranks {lo, hi} of the two order statistics numpy's linear
    method interpolates between in a group of N values, and the interpolation fraction t - numpy's steps in float64."""
    N = int(N)
    if N < 1:
        raise ValueError("a group needs at least one value")
    ranks, frac = [], []
    for v in check_q(q):
        vi = (v / 100.0) * (N - 1)
        lo = min(int(math.floor(vi)), N - 1)
        ranks += [lo, min(lo + 1, N - 1)]
        frac.append(vi - lo)
    return ranks, frac


def lerp(a: float, b: float, t: float) -> float:
    """TILE_RANK_PICK's interpolation (numpy's `_lerp`), every operation rounded on its own."""
    a, b, t = float(a), float(b), float(t)
    d = b - a
    r = a + d * t
    if t >= 0.5:
        r = b - d * (1.0 - t)
    return r


def check_percentile(percentile) -> float:
    p = float(percentile)
    if not 50.0 < p <= 100.0:
        raise ValueError("percentile must lie in (50, 100]: the stretch runs from 100 - percentile to percentile")
    return p


def check_palette(palette) -> torch.Tensor:
    """uint8 CPU tensor [K, 3], 1 <= K <= 256, from a uint8 tensor or numpy array of that shape."""
    if isinstance(palette, np.ndarray):
        palette = torch.from_numpy(palette)
    if not isinstance(palette, torch.Tensor) or palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 \
            or not 1 <= palette.shape[0] <= 256:
        raise ValueError("palette must be a uint8 tensor [K, 3] with 1 <= K <= 256")
    return palette.detach().cpu().contiguous()


def alpha_code(alpha) -> int:
    """CLASS_OVERLAY's ALPHA in 0..256 from an opacity in [0, 1]."""
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise ValueError("alpha must lie in [0, 1]")
    return int(round(a * 256.0))


def check_params(params, N: int, H: int, W: int, SH: int, SW: int) -> torch.Tensor:
    """int32 CPU [B, 4] = {tile, y0, x0, flips} with the SH x SW window inside the tile: what TILE_QUICKLOOK does not check."""
    par = torch.as_tensor(params).cpu()
    if par.dim() != 2 or par.shape[1] != 4 or par.shape[0] < 1 or par.is_floating_point():
        raise ValueError("params must be an integer array [B, 4] = {tile, y0, x0, flips}")
    par = par.to(torch.int64)
    ok = (par[:, 0] >= 0) & (par[:, 0] < N) & (par[:, 1] >= 0) & (par[:, 1] <= H - SH) & (par[:, 2] >= 0) & (par[:, 2] <= W - SW) \
        & (par[:, 3] >= 0) & (par[:, 3] <= 3)
    if not bool(ok.all()):
        raise ValueError("params out of range (tile index, crop offsets, flip bits)")
    return par.to(torch.int32).contiguous()


@torch.no_grad()
def run_selection(raw: torch.Tensor, index: torch.Tensor, bands: list[int], pooled: bool, ranks: list[int], frac: list[float] | None,
                  extra=None):
    """The four-record selection call over the resident tiles `raw` (on the GPU): (VALUES int32 [G, R], PCT float64 [G, R // 2] or
    None) as views of the call's zeroed scratch.  `index` int32 CPU [M] and `bands` are validated by the caller.  `extra(call, pct_ref)`
    may append records that read PCT in the same call (the quicklook stretch) before anything is uploaded or launched."""
    nsrc, C, H, W = raw.shape
    M, nb, R = int(index.numel()), len(bands), len(ranks)
    if not 1 <= R <= MAX_RANKS:
        raise ValueError(f"1..{MAX_RANKS} ranks per selection")
    G, N = (nb, M * H * W) if pooled else (M, nb * H * W)
    if any(not 0 <= r < N for r in ranks):
        raise ValueError("rank outside the group")
    call = StageCall()
    t_raw = call.t(raw)
    t_index, t_bands, t_ranks = call.const(index, "i32"), call.const(bands, "i32"), call.const(ranks, "i64")
    t_frac = call.const(frac, "f64") if frac is not None else None
    h0, h1 = call.scratch((G, 256), "i64"), call.scratch((G, R, 256), "i64")          # HIST accumulates: the scratch is zeroed
    bucket, rest, values = call.scratch((G, R), "i32"), call.scratch((G, R), "i64"), call.scratch((G, R), "i32")
    pct = call.scratch((G, R // 2), "f64") if frac is not None else None
    dims = dict(M=M, C=C, H=H, W=W, NSRC=nsrc, NBND=nb, POOLED=int(pooled), R=R)
    call.add("TILE_RADIX_HIST", RAW=t_raw, INDEX=t_index, BANDS=t_bands, BUCKET=None, HIST=h0, PASS=0, **dims)
    call.add("TILE_RANK_PICK", HIST=h0, RANKS=t_ranks, BUCKET=bucket, REST=rest, N=N, G=G, R=R, STEP=0)
    call.add("TILE_RADIX_HIST", RAW=t_raw, INDEX=t_index, BANDS=t_bands, BUCKET=bucket, HIST=h1, PASS=1, **dims)
    call.add("TILE_RANK_PICK", HIST=h1, RANKS=t_ranks, BUCKET=bucket, REST=rest, VALUES=values, FRAC=t_frac, PCT=pct, N=N, G=G, R=R, STEP=1)
    if extra is not None:
        extra(call, pct)
    call.run()
    return call.view(values), (None if pct is None else call.view(pct))


def add_quicklook(call: StageCall, raw, par, slot, bands, pct: TRef, out, nrow: int) -> None:
    """Append the TILE_QUICKLOOK record that stretches the crops `par` (int32 CPU [B, 4]) of `raw` into `out` (uint8 [B, SH, SW, 3])
    between the bounds PCT[slot[b]] (`pct`: a ref of `call`, float64 [nrow, 2])."""
    N, C, H, W = raw.shape
    B, SH, SW = out.shape[:3]
    call.add("TILE_QUICKLOOK", RAW=call.t(raw), PARAMS=call.const(par, "i32"), SLOT=call.const(slot, "i32"), BANDS=call.const(bands, "i32"),
             PCT=pct, OUT=call.t(out), B=B, C=C, H=H, W=W, SH=SH, SW=SW, NSRC=N, NROW=nrow, NQ=2)


@torch.no_grad()
def run_zero_count(raw: torch.Tensor, index: torch.Tensor, band: int) -> torch.Tensor:
    """int64 [M] on the device: how many pixels of band `band` of every selected tile are 0 - ONE fine-pass record with the coarse bin
    preset to that of the value 0, whose fine bin 0 then is the count."""
    nsrc, C, H, W = raw.shape
    M = int(index.numel())
    call = StageCall()
    hist = call.scratch((M, 1, 256), "i64")
    call.add("TILE_RADIX_HIST", RAW=call.t(raw), INDEX=call.const(index, "i32"), BANDS=call.const([band], "i32"),
             BUCKET=call.const([ZERO_BUCKET] * M, "i32", (M, 1)), HIST=hist, M=M, C=C, H=H, W=W, NSRC=nsrc, NBND=1, POOLED=0, PASS=1, R=1)
    call.run()
    return call.view(hist)[:, 0, 0]
