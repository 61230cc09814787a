"""numpy restatement of the quicklook stages (TILE_RADIX_HIST, TILE_RANK_PICK, TILE_QUICKLOOK, CLASS_OVERLAY; csrc/quicklook.hip), the
yardstick of tests/test_quicklook_cpu.py and tests/test_quicklook_gpu.py: `np.sort` / `np.bincount` for the histograms and ranks,
`np.percentile` for the percentiles, the reference's two lines (src/plotting.py:75-96) for the stretch, the integer blend.

The reference function itself cannot be imported (rasterio is absent); `np.percentile` is the arithmetic it calls.  It is called on
the group's values as float64: on an int16 array numpy subtracts two order statistics in int16 and wraps around when they lie further
apart than 32767 (np.percentile(np.array([-32768, 32767], np.int16), 50) is 32767.5)."""
import numpy as np


def groups(raw, index, bands, pooled):
    """int16 [G, N]: the multiset of every group, in the stage's meaning of POOLED."""
    sel = np.asarray(raw)[np.asarray(index)][:, np.asarray(bands)]          # [M, NBND, H, W]
    if pooled:
        return sel.transpose(1, 0, 2, 3).reshape(len(bands), -1)
    return sel.reshape(len(index), -1)


def key(v):
    return np.asarray(v).astype(np.int64) + 32768


def coarse_hist(grp):
    """int64 [G, 256]: counts by key >> 8"""
    return np.stack([np.bincount(key(g) >> 8, minlength=256) for g in grp]).astype(np.int64)


def fine_hist(grp, bucket):
    """int64 [G, R, 256]: counts by key & 255 of the values whose key >> 8 == bucket[g][r]"""
    out = np.zeros(bucket.shape + (256,), dtype=np.int64)
    for g, vals in enumerate(grp):
        k = key(vals)
        for r, b in enumerate(bucket[g]):
            out[g, r] = np.bincount(k[(k >> 8) == b] & 255, minlength=256)
    return out


def pick0(hist, ranks):
    """(BUCKET int32 [G, R], REST int64 [G, R]) from the coarse histogram"""
    cum = np.cumsum(hist, axis=1)
    bucket = np.stack([np.searchsorted(c, np.asarray(ranks), side="right") for c in cum]).astype(np.int32)
    below = np.stack([np.concatenate([[0], c])[b] for c, b in zip(cum, bucket)])
    return bucket, np.asarray(ranks, dtype=np.int64)[None, :] - below


def order_statistics(grp, ranks):
    """int32 [G, R]: sorted(group)[rank]"""
    return np.sort(grp, axis=1)[:, np.asarray(ranks)].astype(np.int32)


def percentiles(grp, q):
    """float64 [G, len(q)]: np.percentile (linear) of every group's values as float64"""
    return np.stack([np.percentile(g.astype(np.float64), q) for g in grp]).reshape(len(grp), -1)


def stretch(image, lo, hi):
    """the reference's stretch of an int16 image with bounds (lo, hi); zeros where the bounds leave no range"""
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        return np.zeros(image.shape, dtype=np.uint8)
    return np.clip((image - lo) / (hi - lo) * 255, 0, 255).astype(np.uint8)


def crop(raw, par, bands, SH, SW):
    """int16 [SH, SW, 3]: TILE_PREP's window {tile, y0, x0, flips} of the three bands, h w rgb"""
    t, y0, x0, fl = (int(v) for v in par)
    win = np.asarray(raw)[t][np.asarray(bands)][:, y0:y0 + SH, x0:x0 + SW]
    if fl & 2:
        win = win[:, ::-1]
    if fl & 1:
        win = win[:, :, ::-1]
    return np.ascontiguousarray(win.transpose(1, 2, 0))


def quicklook(raw, params, bands, q, SH, SW):
    """uint8 [B, SH, SW, 3]: per sample the crop stretched between the percentiles (100 - q, q) of the three bands of its WHOLE tile"""
    out = []
    for par in np.asarray(params):
        p = np.percentile(np.asarray(raw)[int(par[0])][np.asarray(bands)].astype(np.float64), (100.0 - q, q))
        out.append(stretch(crop(raw, par, bands, SH, SW), p[0], p[1]))
    return np.stack(out)


def overlay(base, cls, palette, alpha, skip0):
    """uint8 [B, SH, SW, 3]: (base*(256 - alpha) + colour*alpha + 128) >> 8 where the class has a colour, base elsewhere"""
    cls, palette = np.asarray(cls), np.asarray(palette).astype(np.int64)
    base = np.zeros(cls.shape + (3,), dtype=np.uint8) if base is None else np.asarray(base)
    K = palette.shape[0]
    keep = (cls < 0) | (cls >= K) | ((cls == 0) & bool(skip0))
    colour = palette[np.clip(cls, 0, K - 1)]
    mixed = (base.astype(np.int64) * (256 - alpha) + colour * alpha + 128) >> 8
    return np.where(keep[..., None], base, mixed).astype(np.uint8)
