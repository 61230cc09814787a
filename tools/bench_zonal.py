"""Time of zonal statistics (csrc/zonal.hip; zonal.histogram, zonal.band_stats, zonal.majority_by_zone) on 256 maps of 512 x 512 - fewer
where per-map tables would not fit classmap.WORKSPACE_BYTES - for five kinds of zone raster, against the torch expressions of the same
results on the same device and against the same kernels with the LDS table compiled out.

    python tools/bench_zonal.py [--grid 16] [--iters 3] [--reps 3] [--buildings 200000] [--landuse 2000] [--no-table PATH]
    python tools/bench_zonal.py --build-no-table        # on a machine with hipcc, after build(): writes libs2k_zonal_notable.so

Zone rasters (seeded):
  buildings    rasterize(burn="index", fill=-1) of 200 k rotated rectangles of 3 - 14 pixels over a 8192 x 8192 area cut into 256 tiles.
  land use     the same of 2 k star polygons of 200 - 2000 vertices and 60 - 400 pixels radius.
  one zone     zone 0 everywhere: every workgroup adds to the same table row, the worst contention.
  components   connected_components labels of blob maps (32 x 32 blobs of 4 classes), ids per map (per_map, num_zones = 512 * 512), 16 maps.
  random       uniformly random ids in [0, 200 k): no locality, so nearly every pixel overflows the LDS table.
Calls timed: whole public calls (the host's argument checks, the allocation and zeroing of the tables, the launches and the status read),
HIP events around `iters` calls after a warm-up, `reps` windows alternating with the torch baseline, median (min .. max).  The rate is
the bytes a call must read and write (zone raster + class map or bands; majority_by_zone: both passes and the copy) over the median,
beside the copy ceiling s2k_measure_peaks measures in the same run.  Baselines: bincount(zone * K + cls) for the histogram; index_add_
(count, sum, sum of squares) and scatter_reduce (amin, amax) for the bands; bincount, argmax and a gather for majority_by_zone.  Each
result is compared with ours once (note column): it must be equal.
The no-table rows time the ENTRY alone (tables zeroed outside the window) of the product library and of the variant built with
-DS2K_ZONAL_NO_TABLE, in which every pixel is a global atomic; that variant exists for this measurement only.  Nothing here is a pass bar."""
import argparse
import ctypes
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from s2lc_amd import _lib, classmap, zonal  # noqa: E402
from tools.bench_rasterize import buildings, landuse, timed  # noqa: E402

T = 512
NO_TABLE = ROOT / "sentinel2-landcover-classification_amd" / "libs2k_zonal_notable.so"


def build_no_table() -> Path:
    """libs2k_zonal_notable.so: the objects build() left beside the sources, with zonal.hip compiled again under -DS2K_ZONAL_NO_TABLE"""
    import __graft_entry__ as g

    hipcc = "/opt/rocm/bin/hipcc"
    objs = [g.CSRC / (s + ".o") for s in g.SOURCES if s != "zonal.hip"]
    if not all(o.exists() for o in objs):
        raise SystemExit("run build() first: the other sources' objects are linked as they are")
    var = g.CSRC / "zonal_notable.o"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-DS2K_ZONAL_NO_TABLE", "-c",
                    str(g.CSRC / "zonal.hip"), "-o", str(var)], check=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(NO_TABLE)] + [str(o) for o in objs] + [str(var)], check=True)
    return NO_TABLE


def span(ts):
    return f"{statistics.median(ts):9.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def windows(ours, base, iters, reps):
    ours(); base(); torch.cuda.synchronize()      # noqa: E702  warm-up
    ts, bs = [], []
    for _ in range(reps):
        ts.append(timed(ours, iters))
        bs.append(timed(base, 1))
    return ts, bs


def keys_of(zone, stride):
    """int64 keys and the mask of pixels that have one"""
    z = zone.long()
    if stride:
        z = z + torch.arange(zone.shape[0], device=zone.device).view(-1, 1, 1) * stride * (z >= 0)
    return z, z >= 0


def torch_hist(zone, cls, Z, K, stride):
    z, ok = keys_of(zone, stride)
    ok = ok & (cls < K)
    return torch.bincount((z * K + cls.long())[ok], minlength=Z * K).view(Z, K)


def torch_bands(zone, vals, Z, stride):
    z, ok = keys_of(zone, stride)
    k = z[ok]
    v = vals.permute(0, 2, 3, 1)[ok].long()
    C, dev = v.shape[1], v.device
    n = torch.zeros(Z, dtype=torch.int64, device=dev).index_add_(0, k, torch.ones_like(k))
    s = torch.zeros(Z, C, dtype=torch.int64, device=dev).index_add_(0, k, v)
    ss = torch.zeros(Z, C, dtype=torch.int64, device=dev).index_add_(0, k, v * v)
    idx = k.view(-1, 1).expand(-1, C)
    lo = torch.full((Z, C), zonal.INT32_MAX, dtype=torch.int64, device=dev).scatter_reduce_(0, idx, v, "amin")
    hi = torch.full((Z, C), zonal.INT32_MIN, dtype=torch.int64, device=dev).scatter_reduce_(0, idx, v, "amax")
    return n, s, ss, lo, hi


def torch_majority_by_zone(zone, cls, Z, K):
    hist = torch_hist(zone, cls, Z, K, 0)
    best, arg = hist.max(1)
    table = torch.where(best >= 1, arg, torch.full_like(arg, -1))
    v = table[zone.long().clamp_min(0)]
    return torch.where((zone >= 0) & (v >= 0), v.to(cls.dtype), cls)


def entry_only(L, zone, stride, cls, vals, Z, K, iters, reps):
    """ms of the histogram entry and of the bands entry of library L alone: tables zeroed outside the timed window"""
    dev, (M, H, W) = zone.device, zone.shape
    st = classmap.new_status(dev)
    stream = torch.cuda.current_stream().cuda_stream
    hist = torch.zeros(Z, K, dtype=torch.int64, device=dev)
    tabs = zonal.new_stats((Z, vals.shape[1]), dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    h = lambda: L.s2k_zonal_histogram(p(zone), 4, stride, p(cls), 1, None, M, H, W, Z, K, p(hist), p(st), ctypes.c_void_p(stream))      # noqa: E731
    b = lambda: L.s2k_zonal_bands(p(zone), 4, stride, p(vals), M, vals.shape[1], H, W, Z, 0, 0, p(tabs.count), p(tabs.sum), p(tabs.sumsq),      # noqa: E731
                                  p(tabs.min), p(tabs.max), p(st), ctypes.c_void_p(stream))
    out = []
    for fn in (h, b):
        assert fn() == 0
        torch.cuda.synchronize()
        out.append([timed(fn, iters) for _ in range(reps)])
    return out, hist, tabs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--buildings", type=int, default=200_000)
    ap.add_argument("--landuse", type=int, default=2000)
    ap.add_argument("--bands", type=int, default=6)
    ap.add_argument("--no-table", default=str(NO_TABLE))
    ap.add_argument("--build-no-table", action="store_true")
    a = ap.parse_args()
    if a.build_no_table:
        print(build_no_table())
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_zonal.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    G, size, C = a.grid, a.grid * T, a.bands
    M = G * G
    origins = [(x * T, y * T) for y in range(G) for x in range(G)]
    rng = np.random.default_rng(0)
    g = torch.Generator(device=dev).manual_seed(0)
    cls = torch.randint(0, 10, (M, T, T), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
    vals = torch.randint(-500, 9000, (M, C, T, T), generator=g, device=dev, dtype=torch.int32).to(torch.int16)
    variant = None
    if Path(a.no_table).exists():
        variant = ctypes.CDLL(a.no_table)
    ceiling = _lib.measure_peaks(dev)["copy_gbps"] * 1e9
    print(f"{M} maps of {T} x {T}, {a.iters} calls per window, {a.reps} windows each, one run; {torch.cuda.get_device_name(0)}; "
          f"measured copy ceiling {ceiling / 1e12:.2f} TB/s (read + write)")
    print(f"{'zones':11s} {'case':22s} {'maps':>4s} {'ms median (min .. max)':>30s} {'TB/s':>6s} {'of copy':>7s} {'torch ms median (min .. max)':>32s} "
          f"{'torch / ours':>12s}  note")

    def polygons(shapes):
        ps = classmap.PolygonSet(shapes, None, device=dev)
        return classmap.rasterize(ps, origins, (T, T), fill=-1, dtype=torch.int32, burn="index"), len(shapes), 0

    def components():
        m = 16
        blobs = torch.randint(0, 4, (m, T // 32, T // 32), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
        blobs = blobs.repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous()
        return classmap.connected_components(blobs, 4), T * T, T * T

    sets = (("buildings", lambda: polygons(buildings(rng, a.buildings, size))), ("land use", lambda: polygons(landuse(rng, a.landuse, size))),
            ("one zone", lambda: (torch.zeros(M, T, T, dtype=torch.int32, device=dev), 1, 0)), ("components", components),
            ("random", lambda: (torch.randint(0, a.buildings, (M, T, T), generator=g, device=dev, dtype=torch.int32), a.buildings, 0)))
    for name, make in sets:
        zone, nz, stride = make()
        per_map = stride > 0

        def row(case, m, ours, base, byts, same):
            ts, bs = windows(ours, base, a.iters, a.reps)
            med = statistics.median(ts)
            print(f"{name:11s} {case:22s} {m:4d} {span(ts):>30s} {byts / med / 1e9:6.3f} {100.0 * byts / (med * 1e-3) / ceiling:6.1f}% {span(bs):>32s} "
                  f"{statistics.median(bs) / med:11.1f}x  {'equal' if same else 'DIFFERS'}", flush=True)

        def fit(row_bytes):      # maps whose per-map tables stay within the workspace
            return min(zone.shape[0], classmap.WORKSPACE_BYTES // (nz * row_bytes)) if per_map else zone.shape[0]

        share = float((zone >= 0).float().mean())
        print(f"{name}: {nz} zones{' per map' if per_map else ''}, {share:.3f} of the pixels in a zone")
        for K in (4, 10):
            m = fit(8 * K)
            z, c = zone[:m], cls[:m]
            ours = lambda: zonal.histogram(z, c, nz, K, per_map=per_map)      # noqa: E731
            base = lambda: torch_hist(z, c, m * nz if per_map else nz, K, stride)      # noqa: E731
            row(f"histogram K={K}", m, ours, base, 5 * z.numel(), torch.equal(ours().view(-1, K), base()))
        m = fit(32 * C)
        z, v = zone[:m], vals[:m]
        ours = lambda: zonal.band_stats(z, v, nz, per_map=per_map)      # noqa: E731
        base = lambda: torch_bands(z, v, m * nz if per_map else nz, stride)      # noqa: E731
        st, want = ours(), base()
        same = (torch.equal(st.count.view(-1, C)[:, 0], want[0]) and torch.equal(st.sum.view(-1, C), want[1]) and torch.equal(st.sumsq.view(-1, C), want[2])
                and torch.equal(st.min.view(-1, C).long(), want[3]) and torch.equal(st.max.view(-1, C).long(), want[4]))
        del st, want
        row(f"band_stats C={C}", m, ours, base, (4 + 2 * C) * z.numel(), same)
        if not per_map:
            ours = lambda: zonal.majority_by_zone(cls, zone, nz, 10)      # noqa: E731
            base = lambda: torch_majority_by_zone(zone, cls, nz, 10)      # noqa: E731
            row("majority_by_zone K=10", M, ours, base, 12 * zone.numel(), torch.equal(ours(), base()))
        if variant is not None:
            m = fit(32 * C)
            z, c, v = zone[:m].contiguous(), cls[:m].contiguous(), vals[:m].contiguous()
            Z = m * nz if per_map else nz
            (th, tb), h0, b0 = entry_only(_lib.lib(), z, stride, c, v, Z, 10, a.iters, a.reps)
            (vh, vb), h1, b1 = entry_only(variant, z, stride, c, v, Z, 10, a.iters, a.reps)
            # both libraries ran the same number of calls on tables of their own, so the tables must agree
            same = torch.equal(h0, h1) and all(torch.equal(x, y) for x, y in zip((b0.count, b0.sum, b0.sumsq, b0.min, b0.max), (b1.count, b1.sum, b1.sumsq, b1.min, b1.max)))
            for case, t, w in ((f"entry histogram K=10", th, vh), (f"entry bands C={C}", tb, vb)):
                print(f"{name:11s} {case:22s} {m:4d} {span(t):>30s} {'':6s} {'':7s} {'no table ' + span(w):>32s} {statistics.median(w) / statistics.median(t):11.2f}x  "
                      f"{'equal' if same else 'DIFFERS'}", flush=True)
        del zone
    if variant is None:
        print(f"no-table variant not found at {a.no_table}: build it with --build-no-table where hipcc is")


if __name__ == "__main__":
    main()
