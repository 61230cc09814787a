"""numpy restatement of `s2k_mae_panels` (include/s2k.h, csrc/mae_render.hip), the yardstick of tests/test_mae_render_cpu.py and
tests/test_mae_render_gpu.py.  It is written from the definition, not from the kernel: patches are formed by reshapes, everything is
float64, the edge cases are set explicitly instead of being left to a cast.

Geometry: C channels, T frames, H = W, patch P, tubelet TUB; g = H / P, L = (T / TUB) * g * g patches of PD = TUB * P * P * C features
in (tt, py, px, c) order.  Panel codes: 0 original, 1 masked, 2 pasted, 3 reconstruction."""
import numpy as np

ORIGINAL, MASKED, PASTED, RECONSTRUCTION = 0, 1, 2, 3
CODES = {"original": ORIGINAL, "masked": MASKED, "pasted": PASTED, "reconstruction": RECONSTRUCTION}


def patchify(imgs, P, TUB):
    """[B, C, T, H, W] -> [B, L, PD]: token (t, gi, gj), feature (tt, py, px, c)"""
    B, C, T, H, W = imgs.shape
    g = H // P
    x = np.asarray(imgs).reshape(B, C, T // TUB, TUB, g, P, g, P)          # b c t tt gi py gj px
    return x.transpose(0, 2, 4, 6, 3, 5, 7, 1).reshape(B, (T // TUB) * g * g, TUB * P * P * C)


def unpatchify(x, C, T, H, P, TUB):
    """[B, L, PD] -> [B, C, T, H, H], the inverse of `patchify`"""
    B, g = x.shape[0], H // P
    x = np.asarray(x).reshape(B, T // TUB, g, g, TUB, P, P, C)             # b t gi gj tt py px c
    return x.transpose(0, 7, 1, 4, 2, 5, 3, 6).reshape(B, C, T, H, H)


def patch_stats(imgs, P, TUB):
    """(mean [B, L, 1], sqrt(var + 1e-6) [B, L, 1]) over the PD features of every patch of `imgs`, unbiased variance, float64"""
    p = patchify(imgs, P, TUB).astype(np.float64)
    return p.mean(-1, keepdims=True), np.sqrt(p.var(-1, ddof=1, keepdims=True) + 1e-6)


def patch_mse(imgs, pred, P, TUB, norm_pix):
    """float64 [B, L]: mean over PD of (pred - target)^2, target = the patch of imgs, standardised when norm_pix"""
    target = patchify(imgs, P, TUB).astype(np.float64)
    with np.errstate(all="ignore"):
        if norm_pix:
            mean, sd = patch_stats(imgs, P, TUB)
            target = (target - mean) / sd
        return ((np.asarray(pred).astype(np.float64) - target) ** 2).mean(-1)


def stretched(x, norm, bounds, bands):
    """float64 [B, H, W, 3]: the value before truncation of x [B, 3, H, W] (float64, the three bands in display order): de-normalised,
    stretched between the sample's bounds and clipped to [0, 255]; 0 for a NaN, for -inf and where the bounds leave no range, 255 for
    +inf"""
    norm, bounds = np.asarray(norm).astype(np.float64), np.asarray(bounds).astype(np.float64)
    b = np.asarray(bands)
    with np.errstate(all="ignore"):
        v = x / norm[1][b][None, :, None, None] + norm[0][b][None, :, None, None]
        lo, hi = bounds[:, 0][:, None, None, None], bounds[:, 1][:, None, None, None]
        r = (v - lo) / (hi - lo) * 255.0
    out = np.clip(r, 0.0, 255.0)
    out[np.isnan(r)] = 0.0
    out[r == np.inf] = 255.0
    out[r == -np.inf] = 0.0
    good = np.isfinite(bounds[:, 0]) & np.isfinite(bounds[:, 1]) & (bounds[:, 1] > bounds[:, 0])
    out[~good] = 0.0
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1))


def panels(imgs, pred, mask, norm, bounds, P, TUB, bands=(2, 1, 0), frame=0, codes=(ORIGINAL, MASKED, PASTED, RECONSTRUCTION), fill=128,
           norm_pix=False):
    """(OUT uint8 [B, NP, H, W, 3], before float64 [B, NP, H, W, 3]): the panels and their values before truncation (a removed patch
    of the masked panel holds `fill` in both)."""
    imgs, pred, mask = np.asarray(imgs), np.asarray(pred), np.asarray(mask)
    B, C, T, H, W = imgs.shape
    g = H // P
    full = pred.astype(np.float64)
    with np.errstate(all="ignore"):
        if norm_pix:
            mean, sd = patch_stats(imgs, P, TUB)
            full = full * sd + mean
    b = np.asarray(bands)
    x_pred = unpatchify(full, C, T, H, P, TUB)[:, b, frame]
    x_orig = imgs[:, b, frame].astype(np.float64)
    orig, reco = stretched(x_orig, norm, bounds, bands), stretched(x_pred, norm, bounds, bands)
    t = frame // TUB
    removed = (mask[:, t * g * g:(t + 1) * g * g].reshape(B, g, g) != 0).repeat(P, 1).repeat(P, 2)[..., None]      # [B, H, W, 1]
    before = []
    for code in codes:
        if code == ORIGINAL:
            before.append(orig)
        elif code == RECONSTRUCTION:
            before.append(reco)
        elif code == PASTED:
            before.append(np.where(removed, reco, orig))
        elif code == MASKED:
            before.append(np.where(removed, float(fill), orig))
        else:
            raise ValueError(code)
    before = np.stack(before, 1)
    return np.floor(before).astype(np.uint8), before
