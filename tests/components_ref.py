"""numpy restatement of s2k_classmap_components and s2k_classmap_sieve (include/s2k.h), written from their definition: union-find with
plain loops for the labels (a component's smallest linear index), root areas and per-class component counts; the sieve rule with its
donor order (area >= min_area first, then the larger area, then the lower root; pixel edges only); `changed` and `hist` come from
tests/classmap_ref.py.  The reference project has no such operation: the definition is the oracle.

Maps are integer arrays [H, W] or [M, H, W]; labels and areas come back as int64 of the map's shape, counts as [M, K]."""
import numpy as np

from tests.classmap_ref import _maps


def _labelled(cls, K, exclude=()):
    ok = (cls >= 0) & (cls < K)
    for c in exclude:
        ok &= cls != c
    return ok


_LABELS = {}     # labellings already made (the sieve cases of a map share its first pass)


def _label_one(cls, K, connectivity, exclude):
    key = (cls.tobytes(), cls.shape, K, connectivity, tuple(exclude))
    if key not in _LABELS:
        if len(_LABELS) >= 256:
            _LABELS.clear()
        _LABELS[key] = _label_loops(cls, K, connectivity, exclude)
    return _LABELS[key].copy()


def _label_loops(cls, K, connectivity, exclude):
    H, W = cls.shape
    ok = _labelled(cls, K, exclude)
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for y in range(H):
        for x in range(W):
            if not ok[y, x]:
                continue
            for dy, dx in back:
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and ok[yy, xx] and cls[yy, xx] == cls[y, x]:
                    a, b = find(y * W + x), find(yy * W + xx)
                    if a != b:
                        parent[max(a, b)] = min(a, b)       # the smaller index stays the root
    labels = np.full(H * W, -1, np.int64)
    for i in np.flatnonzero(ok.reshape(-1)):
        labels[i] = find(int(i))
    return labels.reshape(H, W)


def components(m, K, connectivity=4, exclude=()):
    """(labels, areas, counts) of the maps `m`"""
    assert connectivity in (4, 8)
    maps, squeeze = _maps(m)
    M, H, W = maps.shape
    labels = np.stack([_label_one(cls, K, connectivity, exclude) for cls in maps])
    areas = np.zeros((M, H * W), np.int64)
    counts = np.zeros((M, K), np.int64)
    for i in range(M):
        flat = labels[i].reshape(-1)
        areas[i] = np.bincount(flat[flat >= 0], minlength=H * W)
        roots = np.flatnonzero(flat == np.arange(H * W))
        counts[i] = np.bincount(maps[i].reshape(-1)[roots], minlength=K)
    areas = areas.reshape(M, H, W)
    return (labels[0], areas[0], counts) if squeeze else (labels, areas, counts)


def _sieve_one(cls, K, min_area, connectivity, fixed, to):
    """one pass over one map: (output, small components relabelled, small components kept for want of a donor)"""
    H, W = cls.shape
    labels, areas, _ = components(cls, K, connectivity)
    lab, area, flat = labels.reshape(-1), areas.reshape(-1), cls.reshape(-1)
    small = {int(r) for r in np.flatnonzero((area > 0) & (area < min_area)) if int(flat[r]) not in fixed}
    target = {}
    if to is not None:
        target = {r: to for r in small}
    else:
        donors = {r: set() for r in small}
        for y in range(H):
            for x in range(W):
                a = int(labels[y, x])
                if a < 0:
                    continue
                for yy, xx in ((y, x + 1), (y + 1, x)):         # every pixel edge once, seen from both sides
                    if yy < H and xx < W:
                        b = int(labels[yy, xx])
                        if b >= 0 and b != a and flat[a] != flat[b]:
                            if a in small:
                                donors[a].add(b)
                            if b in small:
                                donors[b].add(a)
        for r, ds in donors.items():
            if ds:
                # components at or above the minimum before small ones, then the larger area, then the lower root
                d = min(ds, key=lambda q: (0 if area[q] >= min_area else 1, -int(area[q]), q))
                target[r] = int(flat[d])                         # the donor's class in the pass's input map
    out = flat.copy()
    for r, c in target.items():
        out[lab == r] = c
    return out.reshape(H, W), len(target), len(small) - len(target)


def sieve(m, K, min_area, connectivity=4, iterations=1, fixed=(), to=None, stats=False):
    """the maps after `iterations` passes; stats=True adds (relabelled, kept without a donor, components at or above min_area or fixed)
    of the FIRST pass, summed over the maps"""
    assert min_area >= 1
    maps, squeeze = _maps(m)
    first = None
    for _ in range(iterations):
        out, relabelled, kept = maps.copy(), 0, 0
        for i, cls in enumerate(maps):
            out[i], r, k = _sieve_one(cls, K, min_area, connectivity, tuple(fixed), to)
            relabelled, kept = relabelled + r, kept + k
        if first is None:
            total = int(sum(components(cls, K, connectivity)[2].sum() for cls in maps))
            first = (relabelled, kept, total - relabelled - kept)
        maps = out
    res = maps[0] if squeeze else maps
    return (res, first) if stats else res


def tile_span(labels, th, tw):
    """(the most th x tw tiles any one component of `labels` [H, W] touches, components that touch more than one tile)"""
    H, W = labels.shape
    tile = (np.arange(H)[:, None] // th) * ((W + tw - 1) // tw) + np.arange(W)[None, :] // tw
    ok = labels >= 0
    pairs = np.unique(np.stack([labels[ok], tile[ok]]), axis=1)
    _, n = np.unique(pairs[0], return_counts=True)
    return int(n.max()), int((n > 1).sum())
