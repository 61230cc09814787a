"""numpy restatement of s2k_classmap_filter (include/s2k.h; csrc/classmap.hip), written from its definition: shifted one-hot sums for the
votes over the window clipped to the image, `argmax` for the lowest class with the most votes, the centre rule on top; the boundary
band; and the `changed` and `hist` counts.  The reference project has no such operation: the definition is the oracle.

Maps are integer arrays [H, W] or [M, H, W]; every function returns int64 classes (the caller casts to the dtype under test)."""
import numpy as np


def _maps(m):
    a = np.asarray(m).astype(np.int64)
    return (a[None], True) if a.ndim == 2 else (a, False)


def window_counts(cls, K, size, votes=None):
    """int64 [K, H, W]: how many pixels of each VOTING class lie in the window of every pixel of one map `cls` [H, W]"""
    H, W = cls.shape
    r = size // 2
    voting = np.zeros(K, bool)
    voting[list(range(K) if votes is None else votes)] = True
    onehot = np.zeros((K, H + 2 * r, W + 2 * r), np.int64)          # zero border: pixels outside the image do not exist
    for k in range(K):
        if voting[k]:
            onehot[k, r:r + H, r:r + W] = cls == k
    out = np.zeros((K, H, W), np.int64)
    for dy in range(size):
        for dx in range(size):
            out += onehot[:, dy:dy + H, dx:dx + W]
    return out


def majority(m, K, size, votes=None, fixed=(), iterations=1):
    maps, squeeze = _maps(m)
    for _ in range(iterations):
        out = maps.copy()
        for i, cls in enumerate(maps):
            n = window_counts(cls, K, size, votes)
            best, lowest = n.max(0), n.argmax(0)                     # argmax: the first, i.e. lowest, class among equals
            inr = (cls >= 0) & (cls < K)
            c = np.where(inr, cls, 0)
            own = np.take_along_axis(n, c[None], 0)[0]
            keep = ~inr | (own == best) | (best == 0) | np.isin(cls, list(fixed))
            out[i] = np.where(keep, cls, lowest)
        maps = out
    return maps[0] if squeeze else maps


def boundary(m, K, size, ignore):
    maps, squeeze = _maps(m)
    out = maps.copy()
    for i, cls in enumerate(maps):
        n = window_counts(cls, K, size)
        inr = (cls >= 0) & (cls < K)
        c = np.where(inr, cls, 0)
        present = n > 0
        present[ignore] = False
        others = present.sum(0) - np.take_along_axis(present, c[None], 0)[0]      # classes in the window other than c and ignore
        out[i] = np.where(inr & (cls != ignore) & (others > 0), ignore, cls)
    return out[0] if squeeze else out


def changed(before, after):
    """int64 [M]: pixels per map whose class differs"""
    a, _ = _maps(before)
    b, _ = _maps(after)
    return (a != b).reshape(a.shape[0], -1).sum(1)


def confusion(true, pred, K):
    """int64 [K, K]: hist[t][p] over the pixels where both lie in [0, K)"""
    t, p = np.asarray(true).astype(np.int64).reshape(-1), np.asarray(pred).astype(np.int64).reshape(-1)
    ok = (t >= 0) & (t < K) & (p >= 0) & (p < K)
    return np.bincount(t[ok] * K + p[ok], minlength=K * K).reshape(K, K)


def coverage(m, K, size):
    """(tied windows, windows where the centre wins a tie against a lower class, changed pixels) of one majority pass over `m`"""
    maps, _ = _maps(m)
    tied = centre_wins = 0
    for cls in maps:
        n = window_counts(cls, K, size)
        best, lowest = n.max(0), n.argmax(0)
        inr = (cls >= 0) & (cls < K)
        own = np.take_along_axis(n, np.where(inr, cls, 0)[None], 0)[0]
        tied += int((((n == best[None]).sum(0) >= 2) & (best > 0)).sum())
        centre_wins += int((inr & (own == best) & (lowest < cls)).sum())
    return tied, centre_wins, int(changed(maps, majority(maps, K, size)).sum())
