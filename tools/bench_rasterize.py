"""Time of polygon rasterisation (s2k_rasterize, csrc/rasterize.hip; `classmap.rasterize`) on 256 tiles of 512 x 512 cut from one
8192 x 8192 area of interest, for three geometries, against the same definition as a torch broadcast expression on the same device and
against PIL.ImageDraw.polygon and matplotlib.path on the host.

    python tools/bench_rasterize.py [--grid 16] [--iters 5] [--reps 5] [--buildings 200000] [--landuse 2000] [--big 100000]

Geometries (seeded):
  buildings   200 k rotated rectangles of 3 - 14 pixels, four vertices each, anywhere in the area.
  land use    2 k star polygons of 200 - 2000 vertices and 60 - 400 pixels radius.
  one big     one star polygon of 100 k vertices over the whole area.
Calls timed: `classmap.rasterize` over all tiles into a new uint8 raster with the unfilled counts (whole calls: the host's argument
checks, the allocation of raster and workspace, three launches a chunk of tiles and the status read), HIP events around `iters` calls
after a warm-up, `reps` windows alternating with the torch baseline, median (min .. max).  The three launches of one call are taken from
a torch.profiler trace of one call (device time per kernel name); where the profiler does not see them the column says so.
Baselines, ONE tile each (the tile in the middle of the area) and only the shapes whose box meets it, which the host picks beforehand
and which is not timed: the torch expression evaluates the definition's int64 inequality for a chunk of edges x all pixels and paints
shape after shape; PIL draws shape after shape with ImageDraw.polygon (its fill convention differs: a time baseline only, never a
correctness yardstick); matplotlib asks Path.contains_points for every pixel centre per ring, XOR-ed (skipped above 2e9 edge-pixel
pairs).  The torch raster of that tile is compared with the kernel's (note column): it must be equal.  Nothing here is a pass bar."""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from s2lc_amd import classmap  # noqa: E402

T = 512
KERNELS = ("rast_box_kernel", "rast_list_kernel", "rast_fill_kernel")


def buildings(rng, n, size):
    c = rng.uniform(0, size, (n, 2))
    half = rng.uniform(1.5, 7.0, (n, 2))
    ang = rng.uniform(0, np.pi, n)
    ux = np.stack([np.cos(ang), np.sin(ang)], 1)
    uy = np.stack([-np.sin(ang), np.cos(ang)], 1)
    corners = [c + sx * half[:, :1] * ux + sy * half[:, 1:] * uy for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    v = np.clip(np.stack(corners, 1), -size, 2 * size)
    return [[v[i]] for i in range(n)]


def star(rng, cx, cy, rmin, rmax, n):
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(rmin, rmax, n)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)


def landuse(rng, n, size):
    out = []
    for _ in range(n):
        r = rng.uniform(60, 400)
        out.append([star(rng, rng.uniform(0, size), rng.uniform(0, size), 0.5 * r, r, int(rng.integers(200, 2001)))])
    return out


def timed(fn, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def per_kernel(fn):
    """device microseconds per kernel name of one call, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for k in KERNELS:
                if k in ev.name:
                    out[k] = out.get(k, 0.0) + float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
        return out if len(out) == len(KERNELS) else None
    except Exception as e:      # noqa: BLE001
        print(f"  (profiler: {type(e).__name__}: {e})")
        return None


def tile_subset(ps, ox, oy):
    """indices of the shapes whose box meets the tile at (ox, oy), and their rings in units (host, not timed)"""
    v, rs, sh = ps.host["verts"].astype(np.int64), ps.host["ring_start"], ps.host["ring_shape"]
    keep = []
    for r in range(len(sh)):
        ring = v[rs[r]:rs[r + 1]]
        lo, hi = ring.min(0), ring.max(0)
        if lo[0] <= 256 * (ox + T) and hi[0] >= 256 * ox and lo[1] <= 256 * (oy + T) and hi[1] >= 256 * oy:
            keep.append((int(sh[r]), ring))
    return keep


def torch_tile(rings, values, ox, oy, dev, chunk=256):
    """the definition as a broadcast expression: uint8 [T, T] of one tile"""
    cx = (256 * (ox + torch.arange(T, device=dev, dtype=torch.int64)) + 128).view(1, 1, T)
    cy = (256 * (oy + torch.arange(T, device=dev, dtype=torch.int64)) + 128).view(1, T, 1)
    out = torch.zeros(T, T, dtype=torch.uint8, device=dev)
    for s, ring in rings:
        a = torch.from_numpy(ring).to(dev)
        b = torch.roll(a, -1, 0)
        up = a[:, 1] < b[:, 1]
        xlo, ylo = torch.where(up, a[:, 0], b[:, 0]), torch.where(up, a[:, 1], b[:, 1])
        xhi, yhi = torch.where(up, b[:, 0], a[:, 0]), torch.where(up, b[:, 1], a[:, 1])
        par = torch.zeros(T, T, dtype=torch.bool, device=dev)
        for e0 in range(0, len(ring), chunk):
            e = slice(e0, e0 + chunk)
            xl, yl, xh, yh = (t[e].view(-1, 1, 1) for t in (xlo, ylo, xhi, yhi))
            hit = (yl <= cy) & (cy < yh) & (xl * (yh - yl) + (cy - yl) * (xh - xl) <= cx * (yh - yl))
            par ^= (hit.sum(0) & 1).bool()
        out = torch.where(par, torch.full_like(out, int(values[s])), out)
    return out


def pil_tile(rings, values, ox, oy):
    from PIL import Image, ImageDraw
    img = Image.new("L", (T, T), 0)
    draw = ImageDraw.Draw(img)
    for s, ring in rings:
        draw.polygon([(float(x) / 256 - ox, float(y) / 256 - oy) for x, y in ring], fill=int(values[s]))
    return np.asarray(img)


def mpl_tile(rings, values, ox, oy):
    from matplotlib.path import Path as MplPath
    jj, ii = np.meshgrid(ox + np.arange(T) + 0.5, oy + np.arange(T) + 0.5)
    pts = np.stack([jj.ravel(), ii.ravel()], 1)
    out = np.zeros(T * T, np.uint8)
    for s, ring in rings:
        r = ring / 256.0
        out[MplPath(np.concatenate([r, r[:1]]), closed=True).contains_points(pts)] = values[s]
    return out.reshape(T, T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--buildings", type=int, default=200_000)
    ap.add_argument("--landuse", type=int, default=2000)
    ap.add_argument("--big", type=int, default=100_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rasterize.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    G, size = a.grid, a.grid * T
    origins = [(x * T, y * T) for y in range(G) for x in range(G)]
    mid = (G // 2) * G + G // 2
    ox, oy = origins[mid]
    rng = np.random.default_rng(0)
    sets = (("buildings", lambda: buildings(rng, a.buildings, size)), ("land use", lambda: landuse(rng, a.landuse, size)),
            ("one big", lambda: [[star(rng, size / 2, size / 2, 0.3 * size, 0.55 * size, a.big)]]))
    print(f"{G * G} tiles of {T} x {T} from one {size} x {size} area, {a.iters} calls per window, {a.reps} windows each, one run; "
          f"{torch.cuda.get_device_name(0)}")
    for name, make in sets:
        shapes = make()
        values = [1 + i % 9 for i in range(len(shapes))]
        t0 = time.perf_counter()
        ps = classmap.PolygonSet(shapes, values, device=dev)
        build = time.perf_counter() - t0
        ours = lambda: classmap.rasterize(ps, origins, (T, T), return_unfilled=True)      # noqa: E731
        out, unfilled = ours()
        rings = tile_subset(ps, ox, oy)
        base = lambda: torch_tile(rings, values, ox, oy, dev)      # noqa: E731
        same = torch.equal(base(), out[mid])
        torch.cuda.synchronize()
        ts, bs = [], []
        for _ in range(a.reps):
            ts.append(timed(ours, a.iters))
            bs.append(timed(base, 1))
        kern = per_kernel(ours)
        t0 = time.perf_counter()
        pil_tile(rings, values, ox, oy)
        pil = (time.perf_counter() - t0) * 1e3
        pairs = sum(len(r) for _, r in rings) * T * T
        mpl = None
        if pairs <= 2e9:
            t0 = time.perf_counter()
            mpl_tile(rings, values, ox, oy)
            mpl = (time.perf_counter() - t0) * 1e3
        med, bmed = statistics.median(ts), statistics.median(bs)
        chunks = -(-len(origins) // classmap.tiles_per_chunk(ps.num_shapes, 256 << 20))
        print(f"{name}: {ps.num_shapes} shapes, {ps.num_vertices} vertices (PolygonSet built on the host in {build:.2f} s); "
              f"{len(rings)} rings meet the middle tile; {chunks} chunk(s) of tiles; unfilled share {float(unfilled.sum()) / (len(origins) * T * T):.3f}")
        print(f"  classmap.rasterize, all {len(origins)} tiles   {med:9.3f} ms ({min(ts):.3f} .. {max(ts):.3f})   = {med / len(origins) * 1e3:8.1f} us a tile")
        if kern is None:
            print("  the three launches of one call        not measured (the profiler did not report them)")
        else:
            print("  the three launches of one call        " + ", ".join(f"{k} {kern[k] / 1e3:.3f} ms" for k in KERNELS))
        print(f"  torch expression, the middle tile     {bmed:9.3f} ms ({min(bs):.3f} .. {max(bs):.3f})   raster {'equal' if same else 'DIFFERS'}")
        print(f"  PIL ImageDraw.polygon, the middle tile {pil:8.3f} ms (host, one run; another fill convention)")
        print(f"  matplotlib.path, the middle tile      " + (f"{mpl:9.3f} ms (host, one run)" if mpl is not None else f"skipped ({pairs:.1e} edge-pixel pairs)"), flush=True)
        del ps, out


if __name__ == "__main__":
    main()
