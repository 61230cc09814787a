"""numpy restatement of the four zonal definitions of include/s2k.h (s2k_zonal_histogram, s2k_zonal_bands, s2k_zonal_majority,
s2k_zonal_paint), written from the header alone: loops, np.add.at and bincount, clarity over speed.  Also the generators of the zone
rasters the GPU tests use."""
import numpy as np

BAD_ZONE = 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def keys(zone, Z: int, zone_stride: int = 0):
    """(key int64 [M, H, W] with -1 where a pixel has no key, status)"""
    zone = np.asarray(zone).astype(np.int64)
    M = zone.shape[0]
    limit = zone_stride if zone_stride > 0 else Z
    if zone_stride > 0:
        assert M * zone_stride == Z
    over = zone >= limit
    key = zone + np.arange(M, dtype=np.int64).reshape(M, 1, 1) * zone_stride
    key = np.where((zone < 0) | over, -1, key)
    return key, (BAD_ZONE if over.any() else 0)


def histogram(zone, cls, Z: int, K: int, zone_stride: int = 0, src_lut=None, hist=None):
    """(hist int64 [Z, K] - `hist` with the counts added -, status)"""
    key, status = keys(zone, Z, zone_stride)
    c = np.asarray(cls).astype(np.int64)
    if src_lut is not None:
        c = np.asarray(src_lut).astype(np.int64)[c]
    out = np.zeros((Z, K), np.int64) if hist is None else np.array(hist, dtype=np.int64).reshape(Z, K)
    ok = (key >= 0) & (c >= 0) & (c < K)
    np.add.at(out, (key[ok], c[ok]), 1)
    return out, status


def new_tables(Z: int, C: int, canary: int = 0):
    """count, sum, sumsq (int64) and min, max (int32) as a caller initialises them; `canary` is added to the three sums"""
    z = lambda: np.full((Z, C), canary, np.int64)      # noqa: E731
    return z(), z(), z(), np.full((Z, C), INT32_MAX, np.int32), np.full((Z, C), INT32_MIN, np.int32)


def bands(zone, vals, Z: int, zone_stride: int = 0, nodata=None, tables=None):
    """((count, sum, sumsq, min, max) [Z, C], status); `tables` are added to / combined into a copy"""
    key, status = keys(zone, Z, zone_stride)
    vals = np.asarray(vals).astype(np.int64)
    M, C = vals.shape[:2]
    count, total, sumsq, lo, hi = [np.array(t) for t in (new_tables(Z, C) if tables is None else tables)]
    for m in range(M):
        for c in range(C):
            v, k = vals[m, c].reshape(-1), key[m].reshape(-1)
            ok = k >= 0
            if nodata is not None:
                ok &= v != nodata
            v, k = v[ok], k[ok]
            np.add.at(count[:, c], k, 1)
            np.add.at(total[:, c], k, v)
            np.add.at(sumsq[:, c], k, v * v)
            np.minimum.at(lo[:, c], k, v.astype(np.int32))
            np.maximum.at(hi[:, c], k, v.astype(np.int32))
    return (count, total, sumsq, lo, hi), status


def majority(hist, votes: int, min_count: int = 1, fill: int = -1):
    """(out_cls int32 [Z], best int64 [Z])"""
    hist = np.asarray(hist, dtype=np.int64)
    Z, K = hist.shape
    cls, best = np.empty(Z, np.int32), np.empty(Z, np.int64)
    for z in range(Z):
        voting = [c for c in range(K) if (votes >> c) & 1]
        best[z] = max(int(hist[z, c]) for c in voting)
        lowest = min(c for c in voting if hist[z, c] == best[z])
        cls[z] = lowest if best[z] >= min_count else fill
    return cls, best


def paint(zone, table, dst_dtype, mode: int = 0, fill: int = 0, zone_stride: int = 0, base=None):
    """(dst [M, H, W] of dst_dtype, status); mode 1 paints onto a copy of `base`"""
    table = np.asarray(table, dtype=np.int64).reshape(-1)
    key, status = keys(zone, table.size, zone_stride)
    v = np.where(key >= 0, table[np.maximum(key, 0)], -1)
    out = np.full(key.shape, fill, dtype=np.int64) if mode == 0 else np.array(base, dtype=np.int64)
    out = np.where(v >= 0, v, out)
    return (out & 255).astype(np.uint8) if np.dtype(dst_dtype) == np.uint8 else out.astype(dst_dtype), status


# ---- generators ------------------------------------------------------------------------------------------------------------------------------
def home_slot(key: int, bits: int = 6, mul: int = 2654435761) -> int:
    return ((int(key) * mul) & 0xffffffff) >> (32 - bits)


def keys_sharing_a_home(n: int, bits: int = 6, start: int = 0):
    """the first n zone ids from `start` on whose home slot is that of the first"""
    out, k = [start], start + 1
    while len(out) < n:
        if home_slot(k, bits) == home_slot(start, bits):
            out.append(k)
        k += 1
    return out


def patches(M: int, H: int, W: int, ids, ph: int = 1, pw: int = 1):
    """zone raster int32 [M, H, W]: patches of ph x pw pixels take the ids in turn, row-major over the patch grid and the maps"""
    ids = np.asarray(ids, dtype=np.int64)
    gy, gx = np.arange(H) // ph, np.arange(W) // pw
    n = gy[:, None] * (gx.max() + 1) + gx[None, :]
    per = int(n.max()) + 1
    return np.stack([ids[(n + m * per) % ids.size] for m in range(M)]).astype(np.int32)


def block_ids(H: int, W: int, n: int, bh: int, bw: int, ids=None):
    """zone raster int32 [1, H, W] with exactly min(n, pixels of a block) distinct ids (ids[i], default i) inside EVERY bh x bw block, one
    pixel each in row-major order of the block, the rest of the block taking the first id"""
    y, x = np.arange(H)[:, None] % bh, np.arange(W)[None, :] % bw
    i = y * bw + x
    i = np.where(i < n, i, 0)
    ids = np.arange(max(n, 1)) if ids is None else np.asarray(ids)
    return ids[i][None].astype(np.int32)
