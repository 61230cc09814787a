"""numpy restatement of s2k_classmap_distance (include/s2k.h) and of what classmap.py builds on it, written from the definitions, not
from the kernel: the site predicate of both modes, brute-force squared distances over all sites, the nearest site by argmin over the
sites in ascending index order (which is the canonical tie: the smallest linear index), the distance-binned confusion counts with
np.add.at, and boundary_band / fill_nearest on top."""
import math

import numpy as np

NO_SITE = 2**31 - 1


def _maps(m):
    m = np.asarray(m)
    return m[None] if m.ndim == 2 else m


def labelled(m, K, exclude=()):
    """bool: the class lies in [0, K) and is not excluded"""
    m = np.asarray(m).astype(np.int64)
    ok = (m >= 0) & (m < K)
    for c in exclude:
        ok &= m != c
    return ok


def sites(m, K, to="boundary", connectivity=4, exclude=()):
    """bool [M, H, W]: the sites of the maps `m`.  to="boundary": labelled pixels with a labelled neighbour of a different class (only
    neighbours inside the map); to=(ids): labelled pixels of those classes."""
    m = _maps(m).astype(np.int64)
    lab = labelled(m, K, exclude)
    if not isinstance(to, str):
        hit = np.zeros(m.shape, bool)
        for c in to:
            hit |= m == c
        return lab & hit
    assert to == "boundary"
    M, H, W = m.shape
    cls = np.where(lab, m, -1)
    pad = np.full((M, H + 2, W + 2), -1, np.int64)
    pad[:, 1:-1, 1:-1] = cls
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    out = np.zeros(m.shape, bool)
    for dy, dx in steps:
        nb = pad[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        out |= (nb >= 0) & (nb != cls)
    return out & lab


def transform_of_sites(site, chunk=2048):
    """(dist2, nearest) int64 [M, H, W] of the bool site maps: brute force over all sites, pixel chunks at a time"""
    site = _maps(site)
    M, H, W = site.shape
    dist2 = np.full((M, H * W), NO_SITE, np.int64)
    nearest = np.full((M, H * W), -1, np.int64)
    py, px = np.divmod(np.arange(H * W), W)
    for i in range(M):
        s = np.flatnonzero(site[i].reshape(-1))                 # ascending linear index
        if s.size == 0:
            continue
        sy, sx = np.divmod(s, W)
        step = max(1, chunk * 2048 // s.size)
        for p0 in range(0, H * W, step):
            d = (py[p0:p0 + step, None] - sy[None]) ** 2 + (px[p0:p0 + step, None] - sx[None]) ** 2
            j = d.argmin(1)                                     # the first minimum: the smallest site index
            dist2[i, p0:p0 + step] = d[np.arange(d.shape[0]), j]
            nearest[i, p0:p0 + step] = s[j]
    return dist2.reshape(M, H, W), nearest.reshape(M, H, W)


def transform(m, K, to="boundary", connectivity=4, exclude=()):
    return transform_of_sites(sites(m, K, to, connectivity, exclude))


def ties(site):
    """pixels of the bool site maps with more than one nearest site"""
    site = _maps(site)
    M, H, W = site.shape
    py, px = np.divmod(np.arange(H * W), W)
    n = 0
    for i in range(M):
        s = np.flatnonzero(site[i].reshape(-1))
        if s.size == 0:
            continue
        sy, sx = np.divmod(s, W)
        step = max(1, 2048 * 2048 // s.size)
        for p0 in range(0, H * W, step):
            d = (py[p0:p0 + step, None] - sy[None]) ** 2 + (px[p0:p0 + step, None] - sx[None]) ** 2
            n += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
    return n


def thresholds(edges):
    """floor(edge^2) of bin edges in pixels"""
    return [math.floor(e * e) for e in edges]


def binned(m, other, dist2, K, edges2):
    """int64 [len(edges2) + 1, K, K]: hist[b][class of m][class of other] over the pixels where both lie in [0, K) (exclude plays no
    part), b = the number of thresholds that dist2 exceeds"""
    m, other, dist2 = _maps(m).astype(np.int64), _maps(other).astype(np.int64), _maps(dist2)
    ok = (m >= 0) & (m < K) & (other >= 0) & (other < K)
    b = np.zeros(m.shape, np.int64)
    for e in edges2:
        b += dist2 > e
    hist = np.zeros((len(edges2) + 1, K, K), np.int64)
    np.add.at(hist, (b[ok], m[ok], other[ok]), 1)
    return hist


def boundary_band(m, K, distance, connectivity=4, ignore_index=0):
    m = np.asarray(m).astype(np.int64)
    d2, _ = transform(m, K, "boundary", connectivity, (ignore_index,))
    mark = labelled(m, K, (ignore_index,)) & (d2.reshape(m.shape) <= math.floor(distance * distance))
    return np.where(mark, ignore_index, m)


def fill_nearest(m, K, fill):
    m = np.asarray(m).astype(np.int64)
    keep = [c for c in range(K) if c not in set(fill)]
    _, near = transform(m, K, keep)
    mm = _maps(m)
    flat = mm.reshape(mm.shape[0], -1)
    nr = near.reshape(flat.shape)
    holes = ~labelled(flat, K, tuple(fill)) & (nr >= 0)
    return np.where(holes, np.take_along_axis(flat, np.maximum(nr, 0), 1), flat).reshape(m.shape)
