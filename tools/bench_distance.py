"""Time of the exact Euclidean distance transform of class maps (classmap.distance_transform: s2k_classmap_distance,
csrc/distance.hip) on 256 int64 maps of 512 x 512: blob maps with K = 4 and 10 to their class boundaries, the same after a 5 x 5
majority filter, the distance to one class, and the extremes - one class everywhere (no site: the row pass searches nothing), a
checkerboard (every pixel a site) and ONE SITE IN A CORNER of each map, the worst case of the pruned search (about W steps a pixel).

    python tools/bench_distance.py [--maps 256] [--iters 20] [--reps 5] [--base-maps 4]

Times are HIP events around `iters` whole calls (allocation of outputs and workspace and the host's argument checks included) after a
warm-up; every configuration is timed `reps` times, alternating with its baseline, and the median and the range are printed.  Baselines
run on `--base-maps` maps and are scaled to the full count (printed as such); both compute dist2 only (no nearest site) and their
results are compared with the kernel's:
  torch      the expression a user would write: the column pass as a cumulative maximum of the site rows from above and from below,
             the row pass as the broadcast minimum over x' of (x - x')^2 + dy(x')^2, in chunks of rows.
  numpy      the same two passes on the host after a copy (printed in the note).
  binned     `DistanceBinnedMetrics.update` (the counts from the launch that computes the distances) against the same transform with
             a torch bucketise and one CONFUSION pass per bin behind it.
Bytes are algorithmic, from the shapes, per call: 20 B / pixel (the int64 map read once by the column pass - the neighbours of the
boundary predicate come from the cache -, the 16-bit offsets written, read and rewritten by the two sweeps and read by the row pass,
dist2 written), 36 B / pixel with the counts (the map and the predictions read by the row pass); the share of the 6.3 TB/s copy
ceiling is printed beside them.  Nothing here is a pass bar."""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from s2lc_amd import classmap  # noqa: E402
from s2lc_amd.metrics import DistanceBinnedMetrics, SegMetrics  # noqa: E402

COPY_CEILING = 6.3e12      # bytes / s, the float4 stream copy of an MI355X
FAR = 1 << 15              # "no site in this column": beyond every offset, its square still fits int32 twice


def timed(fn, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def torch_sites(m, K, to, exclude):
    """bool sites of the int64 maps `m`, connectivity 4"""
    lab = (m >= 0) & (m < K)
    for c in exclude:
        lab &= m != c
    if to != "boundary":
        hit = torch.zeros_like(lab)
        for c in to:
            hit |= m == c
        return lab & hit
    cls = F.pad(torch.where(lab, m, torch.full_like(m, -1)), (1, 1, 1, 1), value=-1)
    mid = cls[:, 1:-1, 1:-1]
    out = torch.zeros_like(lab)
    for nb in (cls[:, :-2, 1:-1], cls[:, 2:, 1:-1], cls[:, 1:-1, :-2], cls[:, 1:-1, 2:]):
        out |= (nb >= 0) & (nb != mid)
    return out & lab


def torch_transform(m, K, to, exclude, rows=64):
    site = torch_sites(m, K, to, exclude)
    M, H, W = m.shape
    y = torch.arange(H, device=m.device, dtype=torch.int32).view(1, H, 1)
    above = torch.where(site, y, torch.full_like(y, -FAR)).cummax(1).values
    below = torch.where(site, y, torch.full_like(y, 2 * FAR)).flip(1).cummin(1).values.flip(1)
    dy = torch.minimum(y - above, below - y).clamp(max=FAR)
    dy2 = dy * dy
    x = torch.arange(W, device=m.device, dtype=torch.int32)
    dx2 = ((x.view(W, 1) - x.view(1, W)) ** 2).view(1, 1, W, W)
    out = torch.empty(M, H, W, dtype=torch.int32, device=m.device)
    for y0 in range(0, H, rows):
        out[:, y0:y0 + rows] = (dx2 + dy2[:, y0:y0 + rows].unsqueeze(2)).amin(3)
    return torch.where(out >= FAR * FAR, torch.full_like(out, classmap.NO_SITE), out)


def numpy_transform(site, rows=32):
    """dist2 of the host copy of the bool sites [M, H, W]: the same two passes, vectorised"""
    M, H, W = site.shape
    y = np.arange(H, dtype=np.int32).reshape(1, H, 1)
    above = np.maximum.accumulate(np.where(site, y, -FAR), 1)
    below = np.minimum.accumulate(np.where(site, y, 2 * FAR)[:, ::-1], 1)[:, ::-1]
    dy = np.minimum(np.minimum(y - above, below - y), FAR).astype(np.int32)
    dy2 = dy * dy
    x = np.arange(W, dtype=np.int32)
    dx2 = ((x[:, None] - x[None]) ** 2).reshape(1, 1, W, W)
    out = np.empty((M, H, W), np.int32)
    for y0 in range(0, H, rows):
        out[:, y0:y0 + rows] = (dx2 + dy2[:, y0:y0 + rows, None]).min(3)
    return np.where(out >= FAR * FAR, classmap.NO_SITE, out)


def alternate(ours, base, iters, reps):
    ours(), ours()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    base()
    torch.cuda.synchronize()
    breps = reps if time.perf_counter() - t0 < 1.0 else 1
    a, b = [], []
    for r in range(reps):
        a.append(timed(ours, iters))
        if r < breps:
            t0 = time.perf_counter()
            base()
            torch.cuda.synchronize()
            b.append((time.perf_counter() - t0) * 1e3)
    return a, b


def line(name, a, b, scale, pix, byts, note):
    med, bmed = statistics.median(a), statistics.median(b) * scale
    span = f"{med:8.4f} ({min(a):.4f} .. {max(a):.4f})"
    bspan = f"{bmed:10.1f} ({min(b) * scale:.1f} .. {max(b) * scale:.1f}; {len(b)} run{'s' * (len(b) > 1)})"
    print(f"{name:38s} {span:>28s} {pix / med / 1e6:8.2f} {byts / med / 1e9:6.3f} {100.0 * byts / (med * 1e-3) / COPY_CEILING:6.1f}% "
          f"{bspan:>44s} {bmed / med:8.1f}x  {note}", flush=True)


def blob_maps(M, H, W, K, g):
    coarse = torch.randint(0, K, (M, 1, H // 16, W // 16), generator=g).float()
    m = F.interpolate(coarse, size=(H, W), mode="nearest").squeeze(1).long()
    salt = torch.rand(M, H, W, generator=g) < 0.10
    m[salt] = torch.randint(0, K, (int(salt.sum()),), generator=g)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-maps", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distance.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    M, H, W, B = a.maps, 512, 512, min(a.base_maps, a.maps)
    pix, scale = M * H * W, M / B
    print(f"{M} maps of {H} x {W}, {a.iters} calls per window, {a.reps} windows each; baselines on {B} maps, scaled by {scale:g}; "
          f"{torch.cuda.get_device_name(0)}")
    print(f"{'configuration':38s} {'ms median (min .. max)':>28s} {'Gpix/s':>8s} {'TB/s':>6s} {'of 6.3':>7s} "
          f"{'baseline ms, scaled: median (min .. max)':>44s} {'ratio':>9s}  note")
    g = torch.Generator().manual_seed(0)
    cases = []
    for K in (4, 10):
        m = blob_maps(M, H, W, K, g).to(dev)
        cases.append((f"boundary blob K={K}", m, K, "boundary", (0,)))
        cases.append((f"boundary blob K={K} after majority 5", classmap.majority_filter(m, K, 5), K, "boundary", (0,)))
    cases.append(("to class 1 blob K=4", cases[0][1], 4, (1,), ()))
    cases.append(("one class (no site)", torch.ones(M, H, W, dtype=torch.int64, device=dev), 2, "boundary", ()))
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    cases.append(("checkerboard (all sites)", ((yy + xx) % 2).unsqueeze(0).repeat(M, 1, 1).to(dev), 2, "boundary", ()))
    corner = torch.zeros(M, H, W, dtype=torch.int64)
    corner[:, 0, 0] = 1
    cases.append(("one site in a corner", corner.to(dev), 2, (1,), ()))
    for name, m, K, to, exclude in cases:
        ours = lambda: classmap.distance_transform(m, K, to, 4, exclude)      # noqa: E731
        got = ours()
        state = {}

        def base():
            state["out"] = torch_transform(m[:B], K, to, exclude)

        t0 = time.perf_counter()
        host = numpy_transform(torch_sites(m[:B], K, to, exclude).cpu().numpy())
        host_ms = (time.perf_counter() - t0) * 1e3 * scale
        t, b = alternate(ours, base, a.iters, a.reps)
        same = torch.equal(got[:B], state["out"]) and np.array_equal(got[:B].cpu().numpy(), host)
        finite = got[got < classmap.NO_SITE]
        far = int(finite.max()) if finite.numel() else -1
        line(f"distance {name}", t, b, scale, pix, 20 * pix,
             f"torch; numpy on the host {host_ms:.0f} ms scaled (one run, sites given); results {'equal' if same else 'DIFFER'}; largest dist2 {far}")
        del got, state, host
    # DistanceBinnedMetrics.update: the counts from the transform's own launch, or a bucketise and a CONFUSION pass per bin behind it
    name, labels, K, _, _ = cases[0]
    pred = cases[1][1]
    fused_m = DistanceBinnedMetrics(K, (1, 2, 4, 8), device=dev)
    bounds = torch.tensor(fused_m.thresholds, dtype=torch.int32, device=dev)
    staged_m = [SegMetrics(K, device=dev) for _ in range(len(fused_m.thresholds) + 1)]
    fused = lambda: fused_m.update(pred, labels)      # noqa: E731

    def staged():
        d2 = classmap.distance_transform(labels, K, "boundary", 4, (0,))
        b = torch.bucketize(d2, bounds)
        for i, s in enumerate(staged_m):
            s.update(pred, torch.where(b == i, labels, torch.full_like(labels, -1)))

    fused(), staged()
    assert torch.equal(fused_m.hist.view(len(staged_m), -1), torch.stack([s.hist for s in staged_m]))
    t, b = alternate(fused, staged, a.iters, a.reps)
    line("binned counts blob K=4, 4 edges", t, b, 1.0, pix, 36 * pix, "fused / bucketise + 5 CONFUSION passes (all maps, not scaled)")


if __name__ == "__main__":
    main()
