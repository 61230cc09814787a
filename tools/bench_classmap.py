"""Time of the class-map filters (classmap.majority_filter / boundary_to_ignore: one launch of s2k_classmap_filter, csrc/classmap.hip)
on 256 maps of 512 x 512 - K = 4 and 10, sizes 3, 5, 7 and 15, both modes, the uint8 path, and the confusion count fused into the
launch or taken afterwards - against the torch expression of the same job on the same device and seeded maps, alternating with it
in the same run.

    python tools/bench_classmap.py [--maps 256] [--iters 200] [--reps 5]

Times are HIP events around `iters` whole calls (output allocation and the host's argument checks included) after a warm-up; every
configuration is timed `reps` times, alternating with its baseline (a tenth as many calls: it is that much slower), and the median and
the range are printed.  Bytes are algorithmic, from the shapes: the map read once and written once.  The torch baseline is the chain
a user would write: one-hot planes, `avg_pool2d` as a box sum (zero padding, divisor 1), `argmax` - K float planes per map and the
LOWEST class on a tie, where the kernel lets the centre win; the share of pixels on which the two rules differ is printed (0 for the
boundary band, whose baseline is the same box sums compared with zero).  Nothing here is a pass bar."""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from s2lc_amd import classmap  # noqa: E402
from s2lc_amd.metrics import SegMetrics  # noqa: E402

COPY_CEILING = 6.3e12      # bytes / s, the float4 stream copy of an MI355X


def timed(fn, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def box_counts(m, K, size):
    """float32 [M, K, H, W]: votes per class in the window clipped to the image"""
    onehot = (m.unsqueeze(1) == torch.arange(K, device=m.device, dtype=m.dtype).view(1, K, 1, 1)).float()
    return F.avg_pool2d(onehot, size, stride=1, padding=size // 2, divisor_override=1)


def torch_majority(m, K, size):
    return box_counts(m, K, size).argmax(1).to(m.dtype)


def torch_boundary(m, K, size, ignore):
    present = box_counts(m, K, size) > 0
    present[:, ignore] = False
    others = present.sum(1) - present.gather(1, m.long().unsqueeze(1)).squeeze(1).long()
    return torch.where((m != ignore) & (others > 0), torch.full_like(m, ignore), m)


def alternate(ours, base, iters, reps):
    for fn in (ours, base):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(ours, iters))
        b.append(timed(base, max(2, iters // 10)))
    return a, b


def line(name, a, b, pix, byts, differ):
    med, bmed = statistics.median(a), statistics.median(b)
    span = f"{med:8.4f} ({min(a):.4f} .. {max(a):.4f})"
    bspan = f"{bmed:8.3f} ({min(b):.3f} .. {max(b):.3f})"
    print(f"{name:34s} {span:>28s} {pix / med / 1e6:8.2f} {byts / med / 1e9:6.3f} {100.0 * byts / (med * 1e-3) / COPY_CEILING:6.1f}% "
          f"{bspan:>30s} {bmed / med:6.1f}x {differ:>9s}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classmap.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    M, H, W = a.maps, 512, 512
    pix = M * H * W
    print(f"{M} maps of {H} x {W}, {a.iters} calls per window ({max(2, a.iters // 10)} of the baseline), {a.reps} windows each, "
          f"{torch.cuda.get_device_name(0)}")
    print(f"{'configuration':34s} {'ms median (min .. max)':>28s} {'Gpix/s':>8s} {'TB/s':>6s} {'of 6.3':>7s} {'torch ms median (min .. max)':>30s} "
          f"{'ratio':>7s} {'tie rule':>9s}")
    g = torch.Generator().manual_seed(0)
    for K in (4, 10):
        # a blocky map with salt on it: what an argmax at 10 m looks like (uniform noise would make every window a tie)
        coarse = torch.randint(0, K, (M, 1, H // 16, W // 16), generator=g).float()
        m = F.interpolate(coarse, size=(H, W), mode="nearest").squeeze(1).long()
        salt = torch.rand(M, H, W, generator=g) < 0.08
        m[salt] = torch.randint(0, K, (int(salt.sum()),), generator=g)
        m = m.to(dev)
        for size in (3, 5, 7, 15):
            ours = lambda: classmap.majority_filter(m, K, size)      # noqa: E731
            base = lambda: torch_majority(m, K, size)                # noqa: E731
            got, ref = ours(), base()
            differ = float((got != ref).float().mean())
            t, b = alternate(ours, base, a.iters, a.reps)
            line(f"majority int64 K={K} size={size}", t, b, pix, 16 * pix, f"{100 * differ:.3f}%")
            del got, ref
        if K == 4:
            for size in (3, 5, 7, 15):
                ours = lambda: classmap.boundary_to_ignore(m, K, size, 0)      # noqa: E731
                base = lambda: torch_boundary(m, K, size, 0)                  # noqa: E731
                assert torch.equal(ours(), base())
                t, b = alternate(ours, base, a.iters, a.reps)
                line(f"boundary int64 K={K} size={size}", t, b, pix, 16 * pix, "equal")
            m8 = m.to(torch.uint8)
            ours = lambda: classmap.majority_filter(m8, K, 5)                 # noqa: E731
            base = lambda: torch_majority(m8, K, 5)                           # noqa: E731
            differ = float((ours() != base()).float().mean())
            t, b = alternate(ours, base, a.iters, a.reps)
            line(f"majority uint8 K={K} size=5", t, b, pix, 2 * pix, f"{100 * differ:.3f}%")
            # the confusion count of TilePredictor.evaluate(majority=5): fused into the filter launch, or a CONFUSION pass afterwards
            # over an int64 label tensor (metrics.SegMetrics.update)
            labels = torch.randint(0, 24, (M, H, W), generator=g, dtype=torch.int32).to(torch.uint8).to(dev)
            lut = (torch.arange(256, dtype=torch.int32) % K).to(dev)
            index = torch.arange(M, dtype=torch.int32, device=dev)
            votes = classmap.class_bits(None, K, "votes")
            fused_m, staged_m = SegMetrics(K, device=dev), SegMetrics(K, device=dev)
            fused = lambda: classmap.run_majority(m, K, 5, 1, votes, 0, last=(labels, index, lut, fused_m.hist))      # noqa: E731
            staged = lambda: staged_m.update(classmap.run_majority(m, K, 5, 1, votes, 0), lut.long()[labels.long()])  # noqa: E731
            fused(), staged()
            assert torch.equal(fused_m.hist, staged_m.hist)
            t, b = alternate(fused, staged, a.iters, a.reps)
            line(f"majority + confusion K={K} size=5", t, b, pix, 17 * pix, "fused/not")


if __name__ == "__main__":
    main()
