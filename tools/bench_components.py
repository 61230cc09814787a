"""Time of connected-component labelling and the minimum-area sieve (classmap.connected_components / sieve: s2k_classmap_components
and s2k_classmap_sieve, csrc/components.hip) on 256 int64 maps of 512 x 512: blob maps with K = 4 and 10, the same after a 5 x 5
majority filter, and the two extremes - one class everywhere, and a one-pixel serpentine through every row.

    python tools/bench_components.py [--maps 256] [--iters 20] [--reps 5] [--base-maps 8] [--max-passes 20000]

Times are HIP events around `iters` whole calls (allocation of outputs and workspace, the host's argument checks and the one status
read included) after a warm-up; every configuration is timed `reps` times, alternating with its baseline, and the median and the range
are printed.  Baselines run on `--base-maps` maps and are scaled to the full count (printed as such):
  labelling  the torch idiom a user would write: per-class index planes propagated by a masked 3 x 3 `max_pool2d` (a plus-shaped pair
             of pools at connectivity 4) until nothing changes, looked at every 16 passes.  Its pass count is printed: it grows with
             the longest path inside a component, which is the point (a run that has not converged after --max-passes stops there and
             says so; it is timed once when a run takes longer than a second).
  sieve      numpy union-find on the host after a copy (hooking under the smaller root and pointer jumping, vectorised), then the same
             donor keys and relabelling in numpy; its result is compared with the kernel's.
  evaluate   the sieve that `TilePredictor.evaluate(min_area=16)` launches, called directly (`classmap.run_sieve`, no model): the
             confusion count fused into its relabel launch against a CONFUSION pass behind it (SegMetrics.update).
Bytes are algorithmic, from the shapes, per call: labelling 24 B / pixel (the int64 map read once, labels written, read and written
again by the flatten, areas zeroed), a sieve pass 60 B / pixel (labelling, then the donor keys zeroed, labels read by the donor pass,
map, labels and areas read and the map written by the relabel); the share of the 6.3 TB/s copy ceiling is printed beside them.
Nothing here is a pass bar."""
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
from s2lc_amd.metrics import SegMetrics  # noqa: E402

COPY_CEILING = 6.3e12      # bytes / s, the float4 stream copy of an MI355X
ROOT_MASK = (1 << 31) - 1


def timed(fn, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def torch_labels(m, K, connectivity, max_passes):
    """(labels, passes, converged): the LARGEST linear index of every pixel's component, by propagation"""
    M, H, W = m.shape
    idx = torch.arange(H * W, device=m.device, dtype=torch.float32).view(1, 1, H, W)      # exact below 2^24
    mask = m.unsqueeze(1) == torch.arange(K, device=m.device, dtype=m.dtype).view(1, K, 1, 1)
    lab = torch.where(mask, idx, torch.full_like(idx, -1.0))
    passes = 0
    while passes < max_passes:
        before = lab
        for _ in range(16):
            if connectivity == 8:
                grown = F.max_pool2d(lab, 3, 1, 1)
            else:
                grown = torch.maximum(F.max_pool2d(lab, (1, 3), 1, (0, 1)), F.max_pool2d(lab, (3, 1), 1, (1, 0)))
            lab = torch.where(mask, grown, lab)
        passes += 16
        if torch.equal(lab, before):
            return lab.amax(1).long(), passes, True
    return lab.amax(1).long(), passes, False


def same_partition(lo, hi) -> bool:
    """the kernel names a component by its smallest index, the baseline by its largest: the same partition iff each is constant on
    the other's components, i.e. lo at pixel hi[p] is lo[p] and hi at pixel lo[p] is hi[p] wherever p is labelled"""
    ok = lo >= 0
    if not torch.equal(ok, hi >= 0):
        return False
    a, b = lo.flatten(1), hi.flatten(1)
    return bool(((a.gather(1, b.clamp(min=0)) == a) | ~ok.flatten(1)).all() and ((b.gather(1, a.clamp(min=0)) == b) | ~ok.flatten(1)).all())


def numpy_components(cls, K, connectivity):
    """(labels, areas) of one map [H, W]: vectorised union-find - hook the larger root under the smaller, then pointer jumping"""
    H, W = cls.shape
    idx = np.arange(H * W).reshape(H, W)
    ok = (cls >= 0) & (cls < K)
    pairs = [(idx[:, 1:], idx[:, :-1]), (idx[1:], idx[:-1])]
    if connectivity == 8:
        pairs += [(idx[1:, 1:], idx[:-1, :-1]), (idx[1:, :-1], idx[:-1, 1:])]
    flat, okf = cls.reshape(-1), ok.reshape(-1)
    a = np.concatenate([p[0].reshape(-1) for p in pairs])
    b = np.concatenate([p[1].reshape(-1) for p in pairs])
    same = okf[a] & okf[b] & (flat[a] == flat[b])
    a, b = a[same], b[same]
    parent = np.arange(H * W)
    while True:
        ra, rb = parent[a], parent[b]
        ne = ra != rb
        if not ne.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[ne], np.minimum(ra, rb)[ne])
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    labels = np.where(okf, parent, -1)
    return labels.reshape(H, W), np.bincount(labels[okf], minlength=H * W)


def numpy_sieve(m, K, min_area, connectivity):
    """one pass of the donor rule over the host copy `m` [M, H, W]"""
    out = m.copy()
    for i, cls in enumerate(m):
        H, W = cls.shape
        labels, areas = numpy_components(cls, K, connectivity)
        lab = labels.reshape(-1)
        idx = np.arange(H * W).reshape(H, W)
        a = np.concatenate([idx[:, 1:].reshape(-1), idx[1:].reshape(-1)])
        b = np.concatenate([idx[:, :-1].reshape(-1), idx[:-1].reshape(-1)])
        a, b = np.concatenate([a, b]), np.concatenate([b, a])                 # every pixel edge, seen from both sides
        la, lb = lab[a], lab[b]
        use = (la >= 0) & (lb >= 0) & (la != lb)
        la, lb = la[use], lb[use]
        use = areas[la] < min_area
        la, lb = la[use], lb[use]
        key = ((areas[lb] >= min_area).astype(np.uint64) << np.uint64(62)) | (areas[lb].astype(np.uint64) << np.uint64(31)) \
            | (ROOT_MASK - lb).astype(np.uint64)
        best = np.zeros(H * W, np.uint64)
        np.maximum.at(best, la, key)
        donor = ROOT_MASK - (best & np.uint64(ROOT_MASK)).astype(np.int64)
        small = (lab >= 0) & (areas[np.maximum(lab, 0)] < min_area) & (best[np.maximum(lab, 0)] > 0)
        flat = out[i].reshape(-1)
        flat[small] = cls.reshape(-1)[donor[lab[small]]]
    return out


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


def serpentine(M, H, W):
    m = torch.zeros(H, W, dtype=torch.int64)
    m[0::2] = 1
    m[1::4, W - 1] = 1
    m[3::4, 0] = 1
    return m.unsqueeze(0).repeat(M, 1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-maps", type=int, default=8)
    ap.add_argument("--max-passes", type=int, default=20000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_components.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    M, H, W, B = a.maps, 512, 512, min(a.base_maps, a.maps)
    pix, scale = M * H * W, M / B
    print(f"{M} maps of {H} x {W}, {a.iters} calls per window, {a.reps} windows each; baselines on {B} maps, scaled by {scale:g}; "
          f"{torch.cuda.get_device_name(0)}")
    print(f"{'configuration':38s} {'ms median (min .. max)':>28s} {'Gpix/s':>8s} {'TB/s':>6s} {'of 6.3':>7s} "
          f"{'baseline ms, scaled: median (min .. max)':>44s} {'ratio':>9s}  note")
    g = torch.Generator().manual_seed(0)
    maps = {}
    for K in (4, 10):
        m = blob_maps(M, H, W, K, g).to(dev)
        maps[f"blob K={K}"] = (m, K)
        maps[f"blob K={K} after majority 5"] = (classmap.majority_filter(m, K, 5), K)
    maps["one class"] = (torch.ones(M, H, W, dtype=torch.int64, device=dev), 2)
    maps["serpentine"] = (serpentine(M, H, W).to(dev), 2)
    for name, (m, K) in maps.items():
        for conn in (4, 8):
            ours = lambda: classmap.connected_components(m, K, conn, return_areas=True, return_counts=True)      # noqa: E731
            got = ours()
            state = {}

            def base():
                state["out"] = torch_labels(m[:B], K, conn, a.max_passes)

            t, b = alternate(ours, base, a.iters, a.reps)
            ref, passes, converged = state["out"]
            if converged:
                same = same_partition(got[0][:B].long(), ref)
                note = f"{passes} passes, partition {'equal' if same else 'DIFFERS'}"
            else:
                note = f"not converged after {passes} passes (timed to there)"
            line(f"components {name} c{conn}", t, b, scale, pix, 24 * pix, note + f"; {int(got[2].sum())} components")
            del got, state
    for name in ("blob K=4", "blob K=10", "blob K=4 after majority 5", "blob K=10 after majority 5"):
        m, K = maps[name]
        ours = lambda: classmap.sieve(m, K, 16)      # noqa: E731
        host = {}

        def base():
            host["out"] = numpy_sieve(m[:B].cpu().numpy(), K, 16, 4)

        got = ours()
        t, b = alternate(ours, base, a.iters, a.reps)
        same = np.array_equal(got[:B].cpu().numpy(), host["out"])
        line(f"sieve 16 {name}", t, b, scale, pix, 60 * pix, f"numpy on the host, result {'equal' if same else 'DIFFERS'}; "
             f"{float((got != m).float().mean()) * 100:.2f}% of the pixels changed")
    # what TilePredictor.evaluate(min_area=16) launches after the model, timed on its own (run_sieve, not the predictor): the confusion
    # count fused into the relabel launch, or a CONFUSION pass afterwards
    m, K = maps["blob K=4"]
    labels = torch.randint(0, 24, (M, H, W), generator=g, dtype=torch.int32).to(torch.uint8).to(dev)
    lut = (torch.arange(256, dtype=torch.int32) % K).to(dev)
    index = torch.arange(M, dtype=torch.int32, device=dev)
    fused_m, staged_m = SegMetrics(K, device=dev), SegMetrics(K, device=dev)
    fused = lambda: classmap.run_sieve(m, K, 16, 4, 1, 0, -1, last=(labels, index, lut, fused_m.hist))      # noqa: E731
    staged = lambda: staged_m.update(classmap.run_sieve(m, K, 16, 4, 1, 0, -1), lut.long()[labels.long()])  # noqa: E731
    fused(), staged()
    assert torch.equal(fused_m.hist, staged_m.hist)
    t, b = alternate(fused, staged, a.iters, a.reps)
    line("sieve 16 + confusion blob K=4", t, b, 1.0, pix, 61 * pix, "fused / CONFUSION pass behind (all maps, not scaled)")


if __name__ == "__main__":
    main()
