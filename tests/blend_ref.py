"""float64 numpy restatement of the WINDOW_BLEND stage (plan/opdefs.py; csrc/predict.hip), shared by tests/test_predict_cpu.py and
tests/test_predict_gpu.py.  The op has no entry in oracle/ops_ref.py.  It takes the same float32 profile W1 as the stage and
includes the softmax (MODE 1) and the un-flipping."""
import numpy as np


def blend_ref(logits: np.ndarray, ys, xs, flips, w1: np.ndarray, H: int, W: int, mode: int):
    """logits [M, F, NY, NX, K, S, S] as the model returned them (window (i, j) under flip variant f, still flipped).
    Returns (BLEND float64 [M, K, H, W], T): T = the largest number of terms summed on one pixel."""
    M, F, NY, NX, K, S, _ = logits.shape
    assert len(ys) == NY and len(xs) == NX and len(flips) == F and w1.shape == (S,) and w1.dtype == np.float32
    w = w1.astype(np.float64)
    w2 = w[:, None] * w[None, :]
    acc = np.zeros((M, K, H, W))
    ws = np.zeros((H, W))
    terms = np.zeros((H, W), dtype=np.int64)
    for f, fl in enumerate(flips):
        for i, y0 in enumerate(ys):
            for j, x0 in enumerate(xs):
                v = logits[:, f, i, j].astype(np.float64)
                if mode == 1:
                    e = np.exp(v - v.max(axis=1, keepdims=True))
                    v = e / e.sum(axis=1, keepdims=True)
                if fl & 1:
                    v = v[..., ::-1]
                if fl & 2:
                    v = v[..., ::-1, :]
                acc[:, :, y0:y0 + S, x0:x0 + S] += w2 * v
                ws[y0:y0 + S, x0:x0 + S] += w2
                terms[y0:y0 + S, x0:x0 + S] += 1
    assert terms.min() >= 1, "the windows do not cover the tile"
    return acc / ws, int(terms.max())


def mask_and_margin(blend: np.ndarray):
    """(first-maximum class map int64 [M, H, W], top-2 margin float64 [M, H, W]; the margin of a single class is +inf)"""
    mask = blend.argmax(axis=1)
    if blend.shape[1] == 1:
        return mask, np.full(mask.shape, np.inf)
    top = np.sort(blend, axis=1)
    return mask, top[:, -1] - top[:, -2]


def confusion(true: np.ndarray, pred: np.ndarray, K: int) -> np.ndarray:
    """int64 [K, K] counts of (true, pred) over the pixels whose true class lies in [0, K)"""
    t, p = true.reshape(-1).astype(np.int64), pred.reshape(-1).astype(np.int64)
    ok = (t >= 0) & (t < K)
    return np.bincount(t[ok] * K + p[ok], minlength=K * K).reshape(K, K).astype(np.int64)
