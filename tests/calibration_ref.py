"""numpy restatement of s2k_calibration, written from the definitions in include/s2k.h (the reference project has no such operation).

Two layers, as the header separates them:
* `argmax_first`, `confidence_probs`, `sums`, `reject`: everything that is an integer function of the per-pixel confidence c, in the
  float32 arithmetic the header names (`np.float32(c) * np.float32(bins)`, `np.rint(c * 2**20)`).  In mode 0 c is a copy of a score and
  the margin one float32 subtraction, so this layer is the whole answer there, bit for bit.
* `softmax64`: the float64 softmax, margin and negative log-likelihood that mode 1 is held to within a derived tolerance
  (`conf_tolerance`, `nll_tolerance`), and the figures `metrics.calibration_from_sums` must reproduce (`figures`)."""
import numpy as np

ONE = 2 ** 20
NLL_MAX = 128.0
EXPF_ULP, LOGF_ULP = 1.0, 1.0       # the largest errors of expf and logf in ulp that ROCm's HIP math API documents; a division is exact (0.5)
U = 2.0 ** -24                      # unit roundoff of float32; one ulp is at most 2 * U relative


def argmax_first(scores):
    """scores [N, K, P] -> (a, top) [N, P]: top = s[0], then `if s[k] > top` for k = 1.. - strict >, a NaN is never chosen over s[0]"""
    s = np.asarray(scores, np.float32)
    a = np.zeros((s.shape[0], s.shape[2]), np.int64)
    top = s[:, 0].copy()
    for k in range(1, s.shape[1]):
        with np.errstate(invalid="ignore"):
            better = s[:, k] > top
        top = np.where(better, s[:, k], top)
        a = np.where(better, k, a)
    return a, top


def second_largest(p, a):
    """the largest p[k], k != a, scanned from -infinity with strict > (NaN never taken)"""
    p = np.asarray(p)
    sec = np.full(a.shape, -np.inf, p.dtype)
    for k in range(p.shape[1]):
        with np.errstate(invalid="ignore"):
            better = (a != k) & (p[:, k] > sec)
        sec = np.where(better, p[:, k], sec)
    return sec


def confidence_probs(scores, measure=0):
    """mode 0: (a, c, conf) - c the maximum, conf the written value (c, or the float32 c - second; c itself when K == 1)"""
    s = np.asarray(scores, np.float32)
    a, c = argmax_first(s)
    if measure == 0 or s.shape[1] == 1:
        return a, c, c.copy()
    with np.errstate(invalid="ignore"):
        return a, c, (c - second_largest(s, a)).astype(np.float32)


def classes(labels, lut=None):
    """the label class after the table, int64"""
    lab = np.asarray(labels)
    return np.asarray(lut, np.int64)[lab] if lut is not None else lab.astype(np.int64)


def labelled(cls, K, exclude=()):
    ok = (cls >= 0) & (cls < K)
    for e in exclude:
        ok &= cls != e
    return ok


def sums(a, c, cls, K, bins, exclude=()):
    """(hist int64 [K, bins, 3], counted bool [N, P], skipped int) from the argmax a, the binning confidence c (float32) and the label
    classes: the integer part of the contract"""
    c = np.asarray(c, np.float32)
    lab = labelled(cls, K, exclude)
    with np.errstate(invalid="ignore"):
        unit = (c >= 0) & (c <= 1)
    counted = lab & unit
    skipped = int((lab & ~unit).sum())
    cc, aa, ll = c[counted], a[counted], cls[counted]
    b = np.minimum(bins - 1, (cc * np.float32(bins)).astype(np.int64))      # a float32 product, truncated
    q = np.rint(cc * np.float32(ONE)).astype(np.int64)
    hist = np.zeros((K, bins, 3), np.int64)
    np.add.at(hist, (aa, b, 0), 1)
    np.add.at(hist, (aa, b, 1), (ll == aa).astype(np.int64))
    np.add.at(hist, (aa, b, 2), q)
    return hist, counted, skipped


def reject(a, conf, reject_below, reject_to):
    """pred = (reject_to >= 0 && conf < reject_below) ? reject_to : a, the comparison in float32; a NaN is never below"""
    if reject_to < 0:
        return a.copy()
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(conf, np.float32) < np.float32(reject_below), reject_to, a)


def softmax64(scores, T=1.0):
    """float64 (p [N, K, P], lse - z: the negative log-likelihood of every class [N, K, P]) of softmax(scores / float32(T)), the
    maximum subtracted first"""
    z = np.asarray(scores, np.float64) / float(np.float32(T))
    z = z - z.max(1, keepdims=True)
    e = np.exp(z)
    S = e.sum(1, keepdims=True)
    return e / S, np.log(S) - z


def confidence64(scores, T=1.0, measure=0):
    """float64 written confidence of mode 1: the maximum of softmax64, or its lead over the runner-up (the maximum when K == 1)"""
    p, _ = softmax64(scores, T)
    srt = np.sort(p, axis=1)
    if measure == 0 or p.shape[1] == 1:
        return srt[:, -1]
    return srt[:, -1] - srt[:, -2]


def nll64(scores, cls, counted, T=1.0, probs=False):
    """float64 sum over the counted pixels of min(max(nll, 0), 128): -log p[label] of the given probabilities, or of softmax64"""
    s = np.asarray(scores, np.float64)
    idx = np.where(counted, cls, 0)[:, None, :]
    if probs:
        pl = np.take_along_axis(s, idx, 1)[:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            nll = np.where(pl > 0, -np.log(np.where(pl > 0, pl, 1.0)), NLL_MAX)
    else:
        nll = np.take_along_axis(softmax64(scores, T)[1], idx, 1)[:, 0]
    return float(np.clip(nll, 0.0, NLL_MAX)[counted].sum())


def conf_tolerance(K, measure=0):
    """Bound on |conf - float64 reference| in mode 1, from the operation order of include/s2k.h (u = 2^-24, one ulp <= 2u relative):
    d[k] = s[k] - s[a] rounds once, d[k] * r_t once, and r_t = 1.0f / T once: the exponent x <= 0 is off by at most 3u|x|, which moves
    exp(x) by at most 3u |x| exp(x) <= 3u / e; expf adds EXPF_ULP * 2u * exp(x); e[a] = expf(0) = 1 is exact.  S >= 1 sums K terms
    with K - 1 roundings: relative (K - 1) u.  So S is off by at most u * (3 (K - 1) / e + 2 EXPF_ULP (S - 1) + (K - 1) S), and with
    (S - 1) / S < 1: relative u * (3 (K - 1) / e + 2 EXPF_ULP + K - 1).  c = 1.0f / S adds u; c <= 1, so that is absolute too.
    The margin subtracts second = e2 / S, e2 <= 1: e2's own error u * (3 / e + 2 EXPF_ULP), S's relative error again, the division's u
    and the subtraction's u.  Second-order terms: 1 % on top."""
    dS = 3.0 * (K - 1) / np.e + 2.0 * EXPF_ULP + (K - 1)
    tol = dS + 1.0
    if measure == 1 and K > 1:
        tol += (3.0 / np.e + 2.0 * EXPF_ULP) + dS + 1.0 + 1.0
    return 1.01 * U * tol


def nll_tolerance(K, scores, T, probs=False):
    """Bound per counted pixel on |quantised nll - float64 nll|.  Mode 1: nll = logf(S) - d[label] * r_t.  log S is off by the relative
    error of S (see conf_tolerance: an absolute error of the logarithm) plus LOGF_ULP * 2u * log S, log S <= log K; the product
    x = d[label] * r_t by 3u |x|, |x| <= the largest spread of the scores / T; the subtraction by u * (log K + |x|); the quantisation
    by 2^-21.  Mode 0: nll = -logf(p): LOGF_ULP * 2u * |log p| with |log p| <= 128 after the clamp (p is exact), and 2^-21."""
    if probs:
        return 1.01 * (LOGF_ULP * 2.0 * U * NLL_MAX) + 2.0 ** -21
    s = np.asarray(scores, np.float64)
    spread = float((s.max(1) - s.min(1)).max()) / float(np.float32(T))
    dS = 3.0 * (K - 1) / np.e + 2.0 * EXPF_ULP + (K - 1)
    logK = np.log(K)
    return 1.01 * U * (dS + 2.0 * LOGF_ULP * logK + 3.0 * spread + (logK + spread)) + 2.0 ** -21


def figures(hist, totals, skipped=0):
    """float64 calibration figures from the integer sums alone, written from the definitions of CalibrationMetrics.compute with numpy
    array operations: ece = sum_b n_b / N |acc_b - conf_b| over the non-empty bins, mce their maximum, nll, accuracy, the reliability
    rows, the same per predicted class, and the risk-coverage table (coverage and accuracy of the pixels with floor(c * bins) >= j)."""
    h = np.asarray(hist, np.int64)
    K, bins = h.shape[:2]

    def tab(cells):
        n, ok, cs = (cells[:, i].astype(np.float64) for i in range(3))
        N = n.sum()
        full = n > 0
        acc = np.where(full, ok / np.where(full, n, 1), 0.0)
        conf = np.where(full, cs / ONE / np.where(full, n, 1), 0.0)
        gap = np.abs(acc - conf)
        ece = float((n[full] / N * gap[full]).sum()) if N else 0.0
        mce = float(gap[full].max()) if N else 0.0
        return n, ok, acc, conf, ece, mce

    n, ok, acc, conf, ece, mce = tab(h.sum(0))
    N = n.sum()
    kept = n[::-1].cumsum()[::-1]
    kept_ok = ok[::-1].cumsum()[::-1]
    out = {"ece": ece, "mce": mce, "nll": float(totals[1]) / ONE / float(totals[0]) if totals[0] else 0.0,
           "accuracy": float(ok.sum() / N) if N else 0.0, "pixels": int(N), "skipped": int(skipped),
           "count": n.astype(np.int64).tolist(), "bin_accuracy": acc.tolist(), "bin_confidence": conf.tolist(),
           "coverage": (kept / N if N else np.zeros(bins)).tolist(),
           "coverage_accuracy": np.where(kept > 0, kept_ok / np.where(kept > 0, kept, 1), 0.0).tolist(), "per_class": []}
    for a in range(K):
        pn, pok, pacc, pconf, pece, pmce = tab(h[a])
        out["per_class"].append({"pixels": int(pn.sum()), "accuracy": float(pok.sum() / pn.sum()) if pn.sum() else 0.0, "ece": pece,
                                 "mce": pmce, "count": pn.astype(np.int64).tolist(), "bin_accuracy": pacc.tolist(),
                                 "bin_confidence": pconf.tolist()})
    return out


def synthetic_logits(s, shape=(3, 4, 65, 67), seed=0):
    """(logits float32 [B, K, H, W] = s * z0, labels int64 [B, H, W] drawn from softmax(z0)): a model whose logits are s times too
    sharp, so the temperature that calibrates it is close to s.  A share of the labels is class 0 by the draw itself."""
    rng = np.random.default_rng(seed)
    B, K, H, W = shape
    z0 = rng.normal(0.0, 1.5, shape)
    p = np.exp(z0 - z0.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    u = rng.random((B, 1, H, W))
    labels = (p.cumsum(1) < u).sum(1).clip(0, K - 1)
    return (s * z0).astype(np.float32), labels.astype(np.int64)


def dense_scan(logits, labels, K, exclude=(), lo=0.05, hi=20.0, n=301):
    """(T, spacing): the minimiser of the float64 NLL over a dense scan in log T - n points over [lo, hi], then n points between the two
    neighbours of the best one (the NLL has one minimum in log T) - and the spacing of that second scan in log T, which is how far T
    can be from the true minimiser"""
    evaluate = nll_evaluator(logits, labels, K, exclude)
    a, b = np.log(lo), np.log(hi)
    for _ in range(2):
        grid = np.linspace(a, b, n)
        i = int(np.argmin(evaluate(np.exp(grid))))
        a, b = grid[max(i - 1, 0)], grid[min(i + 1, n - 1)]
    return float(np.exp(grid[i])), float(grid[1] - grid[0])


def nll_evaluator(logits, labels, K, exclude=()):
    """a float64 numpy `evaluate` for metrics.refine_temperature: temperatures -> NLL sums over the labelled pixels"""
    z = np.asarray(logits, np.float64).reshape(logits.shape[0], K, -1)
    cls = np.asarray(labels).reshape(labels.shape[0], -1)
    keep = labelled(cls, K, exclude)
    zz = np.moveaxis(z, 1, 2)[keep]
    ll = cls[keep]

    def evaluate(temps):
        out = []
        for T in temps:
            x = zz / T
            x = x - x.max(1, keepdims=True)
            out.append(float((np.log(np.exp(x).sum(1)) - x[np.arange(len(ll)), ll]).sum()))
        return out

    return evaluate
