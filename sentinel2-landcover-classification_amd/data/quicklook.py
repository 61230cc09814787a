"""Host side of the tile quicklooks: the rank / fraction derivation of numpy's linear percentile, the argument validators of
`GpuTilePipeline.band_percentiles` / `.zero_fraction` / `.quicklook`, `render.overlay` and `TilePredictor.render`, and the one program
builder behind them (`run_selection`).  Pure host code except `run_selection`, which launches.

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

from .. import _lib
from ..plan import opdefs as D
from ..plan.program import ALIGN, ITEMSIZE, Program, TRef

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


class _Buf:
    """A byte image laid out like an arena: constants are `put`, results are `alloc`ated."""

    def __init__(self, base: str):
        self.base, self.top, self.parts = D.BASE[base], 0, []

    def alloc(self, shape, dtype: str) -> TRef:
        t = TRef(self.base, self.top, tuple(int(s) for s in shape), dtype)
        self.top += (t.nbytes + ALIGN - 1) // ALIGN * ALIGN
        return t

    def put(self, values, dtype: str, shape=None) -> TRef:
        tdt = {"i32": torch.int32, "i64": torch.int64, "f64": torch.float64}[dtype]
        data = torch.as_tensor(values, dtype=tdt).contiguous()
        ref = self.alloc(data.shape if shape is None else shape, dtype)
        assert ref.nbytes == data.numel() * ITEMSIZE[dtype]
        self.parts.append((ref.off, data.reshape(-1).view(torch.uint8)))
        return ref

    def image(self) -> torch.Tensor:
        img = torch.zeros(max(self.top, ALIGN), dtype=torch.uint8)
        for off, b in self.parts:
            img[off:off + b.numel()] = b
        return img


def view(ws: torch.Tensor, ref: TRef, dtype: torch.dtype) -> torch.Tensor:
    return ws[ref.off:ref.off + ref.nbytes].view(dtype).view(ref.shape)


@torch.no_grad()
def run_selection(raw: torch.Tensor, index: torch.Tensor, bands: list[int], pooled: bool, ranks: list[int], frac: list[float] | None,
                  extra=None):
    """The four-record selection program over the resident tiles `raw` (on the GPU): (VALUES int32 [G, R], PCT float64 [G, R // 2] or
    None) as views of one device workspace.  `index` int32 CPU [M] and `bands` are validated by the caller.  `extra(prog, const, ws,
    pct_ref, bases)` may append records that read PCT in the same program (the quicklook stretch) before anything is launched."""
    nsrc, C, H, W = raw.shape
    M, nb, R = int(index.numel()), len(bands), len(ranks)
    if not 1 <= R <= MAX_RANKS:
        raise ValueError(f"1..{MAX_RANKS} ranks per selection")
    G, N = (nb, M * H * W) if pooled else (M, nb * H * W)
    if any(not 0 <= r < N for r in ranks):
        raise ValueError("rank outside the group")
    const, ws = _Buf("AUX"), _Buf("WS")
    t_index, t_bands, t_ranks = const.put(index, "i32"), const.put(bands, "i32"), const.put(ranks, "i64")
    t_frac = const.put(frac, "f64") if frac is not None else None
    t_raw = TRef(D.BASE["X"], 0, (nsrc, C, H, W), "i16")
    h0, h1 = ws.alloc((G, 256), "i64"), ws.alloc((G, R, 256), "i64")
    bucket, rest, values = ws.alloc((G, R), "i32"), ws.alloc((G, R), "i64"), ws.alloc((G, R), "i32")
    pct = ws.alloc((G, R // 2), "f64") if frac is not None else None
    prog = Program()
    dims = dict(M=M, C=C, H=H, W=W, NSRC=nsrc, NBND=nb, POOLED=int(pooled), R=R)
    prog.add("TILE_RADIX_HIST", RAW=t_raw, INDEX=t_index, BANDS=t_bands, BUCKET=None, HIST=h0, PASS=0, **dims)
    prog.add("TILE_RANK_PICK", HIST=h0, RANKS=t_ranks, BUCKET=bucket, REST=rest, N=N, G=G, R=R, STEP=0)
    prog.add("TILE_RADIX_HIST", RAW=t_raw, INDEX=t_index, BANDS=t_bands, BUCKET=bucket, HIST=h1, PASS=1, **dims)
    prog.add("TILE_RANK_PICK", HIST=h1, RANKS=t_ranks, BUCKET=bucket, REST=rest, VALUES=values, FRAC=t_frac, PCT=pct, N=N, G=G, R=R, STEP=1)
    bases = _lib.Bases().set("X", raw)
    if extra is not None:
        extra(prog, const, ws, pct, bases)
    ws_d = torch.zeros(max(ws.top, ALIGN), dtype=torch.uint8, device=raw.device)      # HIST accumulates: zeroed here
    bases.set("AUX", const.image().to(raw.device)).set("WS", ws_d)
    _lib.run(prog.pack(), bases, torch.cuda.current_stream(raw.device).cuda_stream)
    return view(ws_d, values, torch.int32), (None if pct is None else view(ws_d, pct, torch.float64))


@torch.no_grad()
def run_zero_count(raw: torch.Tensor, index: torch.Tensor, band: int) -> torch.Tensor:
    """int64 [M] on the device: how many pixels of band `band` of every selected tile are 0 - ONE fine-pass record with the coarse bin
    preset to that of the value 0, whose fine bin 0 then is the count."""
    nsrc, C, H, W = raw.shape
    M = int(index.numel())
    const, ws = _Buf("AUX"), _Buf("WS")
    t_index, t_bands = const.put(index, "i32"), const.put([band], "i32")
    t_bucket = const.put([ZERO_BUCKET] * M, "i32", (M, 1))
    hist = ws.alloc((M, 1, 256), "i64")
    prog = Program()
    prog.add("TILE_RADIX_HIST", RAW=TRef(D.BASE["X"], 0, (nsrc, C, H, W), "i16"), INDEX=t_index, BANDS=t_bands, BUCKET=t_bucket, HIST=hist,
             M=M, C=C, H=H, W=W, NSRC=nsrc, NBND=1, POOLED=0, PASS=1, R=1)
    ws_d = torch.zeros(ws.top, dtype=torch.uint8, device=raw.device)
    bases = _lib.Bases().set("X", raw).set("AUX", const.image().to(raw.device)).set("WS", ws_d)
    _lib.run(prog.pack(), bases, torch.cuda.current_stream(raw.device).cuda_stream)
    return view(ws_d, hist, torch.int64)[:, 0, 0]
