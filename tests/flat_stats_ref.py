"""float64 numpy restatement of the SEG_STATS / SEG_HIST / GRAD_CLIP stages (plan/opdefs.py) and the probe buffers the CPU and GPU tests
share.  The stages have no entry in oracle/ops_ref.py; tests/test_flat_stats_cpu.py pins this restatement to torch's own
`clip_grad_norm_` and `histc`."""
import functools

import numpy as np


def seg_stats_ref(x: np.ndarray, segs):
    """(STATS float64 [P, 4] = {sum, sumsq, min, max}, COUNTS int64 [P, 2] = {NaN, Inf}): sum / min / max over the finite elements,
    sumsq over all of them"""
    stats, counts = np.zeros((len(segs), 4)), np.zeros((len(segs), 2), dtype=np.int64)
    with np.errstate(all="ignore"):
        for p, (first, n) in enumerate(segs):
            v = x[first:first + n].astype(np.float64)
            fin = v[np.isfinite(v)]
            stats[p] = [fin.sum(), (v * v).sum(), fin.min() if fin.size else np.inf, fin.max() if fin.size else -np.inf]
            counts[p] = [np.isnan(v).sum(), np.isinf(v).sum()]
    return stats, counts


def seg_bins_ref(v: np.ndarray, lo: float, hi: float, nb: int) -> np.ndarray:
    """bin of every FINITE element of v (float64 throughout): floor((x - lo) / (hi - lo) * nb), nb - 1 where that gives nb"""
    v = v.astype(np.float64)
    v = v[np.isfinite(v)]
    if lo == hi:
        lo, hi = lo - 1.0, hi + 1.0
    b = np.floor((v - lo) / (hi - lo) * nb).astype(np.int64)
    b[b == nb] = nb - 1
    return b


def seg_hist_ref(x: np.ndarray, segs, stats: np.ndarray, nb: int) -> np.ndarray:
    hist = np.zeros((len(segs), nb), dtype=np.int64)
    for p, (first, n) in enumerate(segs):
        b = seg_bins_ref(x[first:first + n], float(stats[p, 2]), float(stats[p, 3]), nb)
        if b.size:
            hist[p] = np.bincount(b, minlength=nb)
    return hist


def grad_clip_ref(x: np.ndarray, segs, sumsq, max_norm: float):
    """(norm float64, coef float64 limited to 1 - a NaN stays a NaN -, the clipped copy of x): sumsq added in ascending p; where
    float32(coef) >= 1 the copy is x itself, otherwise float32(x) * float32(coef) on the segments' elements and x elsewhere"""
    total = 0.0
    for q in sumsq:
        total = total + float(q)
    with np.errstate(all="ignore"):
        norm = np.sqrt(np.float64(total))
        coef = np.float64(np.float32(max_norm)) / (norm + 1e-6)
        coef = np.float64(1.0) if coef > 1.0 else coef
        out = x.copy()
        c32 = np.float32(coef)
        if not c32 >= 1.0:
            for first, n in segs:
                out[first:first + n] = x[first:first + n] * c32
    return float(norm), float(coef), out


# ---- probe buffers ---------------------------------------------------------------------------------------------------------------
def probe_sizes(chunk: int):
    return [1, 63, 64, 65, 4095, 4096, 4097, chunk - 1, chunk, chunk + 1, 3 * chunk + 17]


SPECIAL = {"constant": 300, "zero": 129, "mixed": 1000, "infs": 200, "nonfinite": 70}      # sizes of the special segments


@functools.lru_cache(maxsize=None)
def probe(chunk: int, special: bool = False, nan_segments: bool = False, shifts=(0, 0), pad: float = float("nan")):
    """(x float32 [total], segs [(first, n)], names): the probe sizes with N(0, 1) times 10^-3 .. 10^1 (a different power per segment),
    every start on a 64-float boundary plus shifts[i % len(shifts)] floats, padding filled with `pad` between the segments (NaN: a
    stage that READS one float too many shows at once; a finite value: so does one that scales one float too many, which a NaN would
    hide) and a 256-float decoy region of 2.5 in front.  special: a constant and an all-zero segment are added; nan_segments: also one
    with NaN, +Inf and -Inf among finite values, one with +-Inf but no NaN, and one without any finite value.  The arrays are shared between tests: do not write to them."""
    rng = np.random.default_rng(7)
    sizes = [(f"n{n}", n) for n in probe_sizes(chunk)]
    if special or nan_segments:
        sizes += [("constant", SPECIAL["constant"]), ("zero", SPECIAL["zero"])]
    if nan_segments:
        sizes += [("mixed", SPECIAL["mixed"]), ("infs", SPECIAL["infs"]), ("nonfinite", SPECIAL["nonfinite"])]
    segs, names, top = [], [], 256
    for i, (name, n) in enumerate(sizes):
        first = top + shifts[i % len(shifts)]
        segs.append((first, n))
        names.append(name)
        top = (first + n + 64 + 63) // 64 * 64          # at least 64 floats of padding behind every segment
    x = np.full(top + 256, pad, dtype=np.float32)
    x[:256] = 2.5
    for i, ((first, n), name) in enumerate(zip(segs, names)):
        v = (rng.standard_normal(n) * 10.0 ** (i % 5 - 3)).astype(np.float32)
        if name == "constant":
            v[:] = np.float32(0.37)
        elif name == "zero":
            v[:] = 0.0
        elif name == "mixed":
            v[[3, 500]] = np.nan
            v[[17, 640, 999]] = np.inf
            v[[0, 64]] = -np.inf
        elif name == "infs":
            v[[5, 130]] = np.inf
            v[77] = -np.inf
        elif name == "nonfinite":
            v[0::3], v[1::3], v[2::3] = np.nan, np.inf, -np.inf
        x[first:first + n] = v
    x.setflags(write=False)
    return x, segs, names
