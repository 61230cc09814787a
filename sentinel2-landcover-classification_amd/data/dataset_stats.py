"""Host derivations of the dataset statistics a segmentation run needs before it starts, from what the TILE_MOMENTS and
TILE_LABEL_HIST stages leave behind (`GpuTilePipeline.band_mean_std`, `.label_histogram`).  Pure functions on CPU tensors, like
`metrics.metrics_from_hist`: the kernels hand over exact integers (and one f64 partial sum per workgroup), every float step is here.

What they replace in the reference, and what their results feed:
  * `calculate_mean_std` (src/data/calculate_dataset_statistics.py:10-43)  ->  `GpuTilePipeline(mean, std)`;
  * `get_class_probabilities` (src/utils.py:152-171)  ->  `EfficientNetConfig.class_distribution`, `losses.get_loss`;
  * `get_sample_weights` (src/utils.py:191-217)  ->  the weights of `GpuTilePipeline.weighted_indices`.
"""
from __future__ import annotations

import math

import torch

MAX_MOMENT_TILES = 65535      # TILE_MOMENTS: |sum_m x| < 2^31 and M * sum_m x^2 < 2^63 for int16 x up to this many tiles


def mean_std_from_moments(sums: torch.Tensor, sdpart: torch.Tensor, M: int, HW: int):
    """(mean, std, pooled_std), float32 [C], from SUMS int64 [C, 2] and SDPART float64 [C, NB] of one TILE_MOMENTS stage over M
    tiles of HW pixels.

    The reference's `WelfordsMethod` keeps a running mean and M2 PER PIXEL POSITION across the samples and reduces over the
    positions only in `finalize`, so what it stores in mean_std.pt is
        mean[c] = mean_p(mean_m x)           = the global mean, and
        std[c]  = mean_p(unbiased std_m x)   - the average of the per-position standard deviations, NOT the pooled one.
    `std` is that statistic (the contract of `A.Normalize(mean, std)` in a run that is to match the reference); `pooled_std` is the
    unbiased standard deviation over all M * HW values of the band, which the same sums give for free.  With fewer than two tiles
    the reference returns a zero std; so do both here."""
    sums = torch.as_tensor(sums).cpu()
    sdpart = torch.as_tensor(sdpart).cpu().double()
    C, n = sums.shape[0], int(M) * int(HW)
    mean, std, pooled = [], [], []
    for c in range(C):
        s1 = int(sums[c, 0])
        s2 = int(sums[c, 1]) & ((1 << 64) - 1)      # the sum of squares is unsigned (opdefs.py, TILE_MOMENTS)
        mean.append(s1 / n)
        acc = 0.0
        for v in sdpart[c].tolist():                # the NB partials in index order
            acc += v
        std.append(acc / HW if M > 1 else 0.0)
        pooled.append(math.sqrt((n * s2 - s1 * s1) / (n * (n - 1))) if M > 1 else 0.0)      # exact integers up to the division
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float()      # noqa: E731
    return f32(mean), f32(std), f32(pooled)


def _counts(hist: torch.Tensor, ignore_zero_label: bool) -> torch.Tensor:
    h = torch.as_tensor(hist).cpu().to(torch.int64).clone()
    if h.dim() != 2:
        raise ValueError("hist must be [M, K]")
    if ignore_zero_label:
        h[:, 0] = 0
    return h


def probabilities_from_hist(hist: torch.Tensor, ignore_zero_label: bool) -> torch.Tensor:
    """float32 [K]: class frequencies over all tiles of `hist` [M, K], the zero class counted as 0 when ignored - the reference's
    `counts / counts.sum()`, an int64-over-int64 true division in float32.

    Always of length K with every class at its own index.  The reference builds the vector from `torch.unique` of the labels it
    sampled, so when a class does not occur there the later classes move down one place, and its fill-up (utils.py:167-170)
    appends zeros at the END - and none at all when the missing class is the highest - so its vector is then mis-ordered or
    short.  The two agree whenever every class occurs.  All counts zero: 0 / 0 = NaN in every entry, as in the reference."""
    counts = _counts(hist, ignore_zero_label).sum(0)
    return counts / counts.sum()


def sample_weights_from_hist(hist: torch.Tensor, class_distribution, ignore_zero_label: bool = False) -> torch.Tensor:
    """float32 [M]: per tile |local class distribution - class_distribution|.sum(), normalised to sum 1, with the reference's
    float32 steps (int64 / int64 -> float32, float32 subtract / abs / sum, float32 normalisation).

    A tile whose counted window is empty (every pixel of the ignored zero class, or outside the LUT's classes) gets weight 0: it
    holds nothing to learn from, so it is never drawn.  The reference divides 0 / 0 there, and that one NaN turns the whole weight
    vector into NaN in its final normalisation."""
    h = _counts(hist, ignore_zero_label)
    g = torch.tensor(torch.as_tensor(class_distribution).tolist(), dtype=torch.float32)
    if g.shape != (h.shape[1],):
        raise ValueError("class_distribution must have one entry per histogram class")
    tot = h.sum(1, keepdim=True)
    local = h / tot.clamp(min=1)
    w = (local - g).abs().sum(1)
    w = torch.where(tot[:, 0] > 0, w, torch.zeros_like(w))
    return w / w.sum()


def weighted_indices(weights, num_samples: int, generator: torch.Generator | None = None) -> torch.Tensor:
    """int64 [num_samples]: `torch.multinomial` with replacement over the weights held as double - the one call
    `torch.utils.data.WeightedRandomSampler(weights, num_samples, True, generator=generator)` makes per epoch, so the same
    generator state gives the same indices.  A host draw, like every other random draw of this library."""
    w = torch.as_tensor(weights, dtype=torch.double).cpu()
    if w.dim() != 1:
        raise ValueError("weights must be a 1-d sequence")
    return torch.multinomial(w, int(num_samples), True, generator=generator)
