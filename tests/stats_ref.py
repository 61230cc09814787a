"""numpy restatements shared by the dataset-statistics tests (tests/test_dataset_stats_cpu.py, tests/test_dataset_stats_gpu.py):
the two stages TILE_LABEL_HIST / TILE_MOMENTS as plan/opdefs.py defines them, and the reference's statistics in float64."""
import numpy as np

from s2lc_amd.plan import opdefs as D


def rel(got, want) -> float:
    """largest difference relative to the largest entry of `want`"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    return float(np.abs(got - want).max() / np.abs(want).max())


def numpy_moments(raw: np.ndarray):
    """(SUMS int64 [C, 2], SDPART f64 [C, NB], M, HW) of TILE_MOMENTS over the tiles raw [M, C, H, W], blocks of D.MOMENTS_BLOCK
    positions; the sum of squares wraps into int64 as the stage's does."""
    M, C, H, W = raw.shape
    x = raw.astype(np.int64).reshape(M, C, H * W)
    s1, s2 = x.sum(0), (x * x).sum(0)
    sd = np.sqrt((M * s2 - s1 * s1).astype(np.float64) / (M * (M - 1))) if M > 1 else np.zeros((C, H * W))
    NB = D.moments_blocks(H * W)
    part = np.stack([sd[:, b * D.MOMENTS_BLOCK:(b + 1) * D.MOMENTS_BLOCK].sum(1) for b in range(NB)], 1)
    return np.stack([s1.sum(1), s2.sum(1)], 1), part, M, H * W


def numpy_hist(lab: np.ndarray, K: int, lut: np.ndarray | None = None) -> np.ndarray:
    """int64 [M, K]: per label raster of lab [M, h, w], the counts of LUT[label] inside [0, K)"""
    out = []
    for t in lab:
        v = t.reshape(-1).astype(np.int64) if lut is None else lut.astype(np.int64)[t.reshape(-1)]
        v = v[(v >= 0) & (v < K)]
        out.append(np.bincount(v, minlength=K))
    return np.stack(out).astype(np.int64)


def mean_std_f64(raw: np.ndarray):
    """the reference's statistic in float64: mean[c] over everything, std[c] = mean over positions of the unbiased standard
    deviation across the tiles (zeros for a single tile)"""
    x = raw.astype(np.float64)
    std = x.std(axis=0, ddof=1).mean(axis=(1, 2)) if raw.shape[0] > 1 else np.zeros(raw.shape[1])
    return x.mean(axis=(0, 2, 3)), std
