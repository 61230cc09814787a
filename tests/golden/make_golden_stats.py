"""Dataset-statistics fixture from the *imported reference* (build container only - /root/reference never travels).

    python tests/golden/make_golden_stats.py

dataset_stats.npz: for seeded synthetic datasets of N int16 tiles [C, H, W] with uint8 label rasters [H, W] (K classes), wrapped in
a tiny Dataset whose items are `(x.float(), y.long())` named tuples (what S2OSMDataset yields without a transform), the results of
the reference's three dataset passes:
  * `WelfordsMethod(dim=(0, 2, 3))` fed by a `DataLoader(dataset, shuffle=False)` exactly as `calculate_mean_std` does
    (src/data/calculate_dataset_statistics.py:10-43; the function itself only adds a progress bar and a torch.save)  -> mean, std;
  * `get_class_probabilities(dataset, ignore_zero_label)` (src/utils.py:152-171)                                         -> prob;
  * `get_sample_weights(dataset, prob.tolist(), ignore_zero_label)` (src/utils.py:191-217)                               -> weights,
the last two with ignore_zero_label False (suffix .ign0) and True (.ign1).  Every tile holds every class, so neither the
missing-class fill-up of get_class_probabilities nor the 0 / 0 of get_sample_weights is in play.  Stored per case: the inputs
(raw, labels) and the float32 results.

Cases (N, C, H, W, K): (5, 3, 8, 12, 4), (37, 6, 16, 20, 4), (300, 6, 8, 8, 4).

The reference computes in float32.  Its distance from a float64 restatement of the same formulas, largest over the cases, relative
to the largest entry of each vector (printed by this script):
    mean 9.5e-8    std 1.1e-7    class probabilities 5.2e-8    sample weights 2.7e-7
The tests compare with the fixture at 1e-6 (about eight float32 ulps, 4x the worst of these): wide enough for the reference's own
rounding, far below any indexing or window error.  The file is about 350 KB, nearly all of it the stored int16 inputs.
"""
from __future__ import annotations

import sys
import typing
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

import ref_harness  # noqa: E402

CASES = [(5, 3, 8, 12, 4), (37, 6, 16, 20, 4), (300, 6, 8, 8, 4)]


class Sample(typing.NamedTuple):
    x: torch.Tensor
    y: torch.Tensor


class Tiles(torch.utils.data.Dataset):
    def __init__(self, raw: torch.Tensor, labels: torch.Tensor):
        self.raw, self.labels = raw, labels

    def __len__(self) -> int:
        return self.raw.shape[0]

    def __getitem__(self, i: int) -> Sample:
        return Sample(x=self.raw[i].float(), y=self.labels[i].long())


def synth(N, C, H, W, K, seed):
    g = torch.Generator().manual_seed(seed)
    offs = torch.randint(0, 4000, (1, C, 1, 1), generator=g, dtype=torch.int32)       # bands differ in level, as Sentinel-2's do
    raw = (torch.randint(-200, 5000, (N, C, H, W), generator=g, dtype=torch.int32) + offs).to(torch.int16)
    lab = torch.randint(0, K, (N, H, W), generator=g, dtype=torch.int32)
    lab.view(N, -1)[:, :K] = torch.arange(K, dtype=torch.int32)                          # every class in every tile
    lab = lab.view(N, -1)[:, torch.randperm(H * W, generator=g)].view(N, H, W).contiguous()
    return raw, lab.to(torch.uint8)


def float64_restatement(raw: np.ndarray, lab: np.ndarray, K: int, ignore: bool):
    x = raw.astype(np.float64)
    mean = x.mean(axis=(0, 2, 3))
    std = x.std(axis=0, ddof=1).mean(axis=(1, 2))
    hist = np.stack([np.bincount(t.reshape(-1), minlength=K) for t in lab]).astype(np.float64)
    if ignore:
        hist[:, 0] = 0
    prob = hist.sum(0) / hist.sum()
    w = np.abs(hist / hist.sum(1, keepdims=True) - prob).sum(1)
    return mean, std, prob, w / w.sum()


def main() -> None:
    ref = ref_harness.load()
    from src.data.calculate_dataset_statistics import WelfordsMethod

    out, worst = {}, {"mean": 0.0, "std": 0.0, "prob": 0.0, "weights": 0.0}
    rel = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())      # noqa: E731
    for ci, (N, C, H, W, K) in enumerate(CASES):
        name = f"n{N}_c{C}_{H}x{W}_k{K}"
        raw, lab = synth(N, C, H, W, K, seed=100 + ci)
        ds = Tiles(raw, lab)
        welford = WelfordsMethod(dim=(0, 2, 3))
        for batch in torch.utils.data.DataLoader(ds, shuffle=False):
            welford.update(batch.x)
        mean, std = welford.finalize(keepdim=False)
        out[f"{name}.raw"], out[f"{name}.labels"] = raw.numpy(), lab.numpy()
        out[f"{name}.mean"], out[f"{name}.std"] = mean.numpy().astype(np.float32), std.numpy().astype(np.float32)
        for ign in (False, True):
            prob = ref.utils.get_class_probabilities(ds, ign)
            assert prob.shape == (K,), "a class is missing from the synthetic labels"
            weights = ref.utils.get_sample_weights(ds, prob.tolist(), ign)
            out[f"{name}.prob.ign{int(ign)}"] = prob.numpy().astype(np.float32)
            out[f"{name}.weights.ign{int(ign)}"] = weights.numpy().astype(np.float32)
            m64, s64, p64, w64 = float64_restatement(raw.numpy(), lab.numpy(), K, ign)
            for key, got, want in (("mean", mean.numpy(), m64), ("std", std.numpy(), s64), ("prob", prob.numpy(), p64),
                                   ("weights", weights.numpy(), w64)):
                worst[key] = max(worst[key], rel(got, want))
    out["cases"] = np.asarray(CASES, dtype=np.int64)
    np.savez_compressed(HERE / "dataset_stats.npz", **out)
    print("wrote dataset_stats.npz;  reference (float32) vs float64 restatement, max relative to the vector's maximum:")
    for k, v in worst.items():
        print(f"  {k:8s} {v:.1e}")


if __name__ == "__main__":
    main()
