"""Numpy restatement of s2k_rasterize (include/s2k.h), written from the definition and not from the kernels: per shape and per edge the
int64 inequality of the definition over the rows the edge spans and every column, XOR-ed into a parity raster; then painter's order.
Also the geometry the CPU and GPU tests share (seeded, handed out read-only)."""
import numpy as np

Q = 256
MAX_COORD = 2 ** 28


def quantise(v) -> np.ndarray:
    """int64 units of float64 pixel coordinates: floor(v * 256 + 0.5)"""
    return np.floor(np.asarray(v, dtype=np.float64) * Q + 0.5).astype(np.int64)


def tables(shapes):
    """(verts int64 [V, 2] in units, ring_start [R + 1], ring_shape [R]) of `shapes`: a list of shapes, each a list of rings, each an
    [n, 2] array-like of float64 pixel coordinates.  Nothing is checked: a ring may have any number of vertices, a shape no ring."""
    rings = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for sh in shapes for r in sh]
    verts = quantise(np.concatenate(rings) if rings else np.zeros((0, 2)))
    ring_start = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    ring_shape = np.array([s for s, sh in enumerate(shapes) for _ in sh], dtype=np.int64)
    return verts, ring_start, ring_shape


def centres(origin, n: int) -> np.ndarray:
    """the centres, in units, of n pixels from `origin` (whole pixels) on"""
    return Q * (int(origin) + np.arange(n, dtype=np.int64)) + Q // 2


def inside(rings, ox: int, oy: int, H: int, W: int) -> np.ndarray:
    """bool [H, W]: the centres of the tile at (ox, oy) inside the shape made of `rings` (int64 [n, 2] arrays in units)"""
    cx, cy = centres(ox, W), centres(oy, H)
    par = np.zeros((H, W), dtype=bool)
    for ring in rings:
        n = len(ring)
        if n < 3:
            continue
        for k in range(n):
            (x0, y0), (x1, y1) = (int(v) for v in ring[k]), (int(v) for v in ring[(k + 1) % n])
            if y0 == y1:
                continue
            (xlo, ylo, xhi, yhi) = (x0, y0, x1, y1) if y0 < y1 else (x1, y1, x0, y0)
            rows = np.nonzero((ylo <= cy) & (cy < yhi))[0]
            if rows.size == 0:
                continue
            lhs = xlo * (yhi - ylo) + (cy[rows] - ylo) * (xhi - xlo)
            par[rows] ^= lhs[:, None] <= cx[None, :] * (yhi - ylo)
    return par


def rasterize(verts, ring_start, ring_shape, values, S: int, origins, H: int, W: int, fill=0, base=None, burn_index: bool = False):
    """(int64 [M, H, W], unfilled int64 [M]): shapes 0..S-1 burned in order over `fill`, or over `base` ([M, H, W]) when given"""
    verts = np.asarray(verts, dtype=np.int64).reshape(-1, 2)
    origins = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    M = len(origins)
    out = np.full((M, H, W), fill, dtype=np.int64) if base is None else np.array(base, dtype=np.int64)
    unfilled = np.zeros(M, dtype=np.int64)
    by_shape = [[] for _ in range(S)]
    for r, s in enumerate(ring_shape):
        by_shape[int(s)].append(verts[int(ring_start[r]):int(ring_start[r + 1])])
    boxes = [(np.concatenate(rs).min(0), np.concatenate(rs).max(0)) if sum(len(r) for r in rs) else None for rs in by_shape]
    for m, (ox, oy) in enumerate(origins):
        x0, x1, y0, y1 = Q * int(ox), Q * (int(ox) + W), Q * int(oy), Q * (int(oy) + H)
        covered = np.zeros((H, W), dtype=bool)
        for s in range(S):
            if boxes[s] is None or boxes[s][0][0] > x1 or boxes[s][1][0] < x0 or boxes[s][0][1] > y1 or boxes[s][1][1] < y0:
                continue                                        # the shape's box misses the tile: it holds none of its centres
            hit = inside(by_shape[s], int(ox), int(oy), H, W)
            out[m][hit] = s if burn_index else int(values[s])
            covered |= hit
        unfilled[m] = H * W - int(covered.sum())
    return out, unfilled


def rasterize_shapes(shapes, values, origins, H: int, W: int, **kw):
    """`rasterize` of float shapes (see `tables`)"""
    v, rs, sh = tables(shapes)
    return rasterize(v, rs, sh, values, len(shapes), origins, H, W, **kw)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def _frozen(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def star(rng, cx: float, cy: float, rmin: float, rmax: float, n: int) -> np.ndarray:
    """a star-shaped ring of n vertices around (cx, cy): ascending angles, radii in [rmin, rmax]"""
    ang = np.sort(rng.uniform(0.0, 2 * np.pi, n))
    rad = rng.uniform(rmin, rmax, n)
    return _frozen(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1))


def stars(seed: int, count: int, H: int, W: int, holes: bool = True, reach: float = 0.9):
    """`count` star polygons whose centres lie in the H x W raster and whose radii go up to `reach` times its larger side, so that
    vertices lie beyond the raster on every side; every other one has a star-shaped hole around the same centre.  (shapes, values)"""
    rng = np.random.default_rng(seed)
    big = reach * max(H, W)
    shapes, values = [], []
    for i in range(count):
        cx, cy = rng.uniform(0.0, W), rng.uniform(0.0, H)
        n = int(rng.integers(3, 24))
        rings = [star(rng, cx, cy, 0.1 * big, big, n)]
        if holes and i % 2 == 0:
            rings.append(star(rng, cx, cy, 0.05 * big, 0.3 * big, int(rng.integers(3, 12))))
        shapes.append(rings)
        values.append(1 + i % 7)
    return shapes, values


def squares(count: int = 3000, per_row: int = 60, pitch: float = 2.25, side: float = 1.75):
    """`count` squares of `side` pixels on a grid of `pitch`; in every third pair the second square is moved onto the first one's right
    half, so that the later one must win there.  Sides are not whole pixels: edges fall between, and now and then through, centres."""
    shapes, values = [], []
    for i in range(count):
        x, y = (i % per_row) * pitch + 0.125, (i // per_row) * pitch + 0.375
        if i % 6 == 1:
            x -= pitch - side / 2
        shapes.append([_frozen([[x, y], [x + side, y], [x + side, y + side], [x, y + side]])])
        values.append(1 + i % 5)
    return shapes, values


def fan(hub=(10.5, 8.5), k: int = 11, radius: float = 7.75):
    """(triangles, hull): a fan of k triangles around a hub that sits exactly on a pixel centre, over the vertices of a convex k-gon whose
    coordinates are multiples of 1 / 256 (so every shared edge has the same end points in both triangles)"""
    ang = 2 * np.pi * (np.arange(k) + 0.3) / k
    pts = np.floor(np.stack([hub[0] + radius * np.cos(ang), hub[1] + radius * np.sin(ang)], axis=1) * Q + 0.5) / Q
    tris = [[_frozen([hub, pts[i], pts[(i + 1) % k]])] for i in range(k)]
    return tris, [_frozen(pts)]


E = 0
# name -> (shapes, values, (H, W), the expected raster written out).  Centres are at (j + 1/2, i + 1/2).
TIES = {
    # all four edges run through centres: left and top in, right and bottom out
    "rectangle_through_centres": ([[[(1.5, 0.5), (4.5, 0.5), (4.5, 2.5), (1.5, 2.5)]]], [7], (4, 6),
                                  [[E, 7, 7, 7, E, E], [E, 7, 7, 7, E, E], [E, E, E, E, E, E], [E, E, E, E, E, E]]),
    # a diamond with every vertex on a centre: the top and bottom vertices are out (no edge spans their row, or both do), the left one
    # is in, the right one out
    "vertices_on_centres": ([[[(2.5, 0.5), (4.5, 2.5), (2.5, 4.5), (0.5, 2.5)]]], [3], (5, 5),
                            [[E, E, E, E, E], [E, 3, 3, E, E], [3, 3, 3, 3, E], [E, 3, 3, E, E], [E, E, E, E, E]]),
    "hole": ([[[(0, 0), (6, 0), (6, 6), (0, 6)], [(2, 2), (2, 4), (4, 4), (4, 2)]]], [5], (6, 6),
             [[5] * 6, [5] * 6, [5, 5, E, E, 5, 5], [5, 5, E, E, 5, 5], [5] * 6, [5] * 6]),
    "the_same_ring_twice": ([[[(0, 0), (4, 0), (4, 3), (0, 3)], [(0, 0), (4, 0), (4, 3), (0, 3)]]], [9], (3, 4), [[E] * 4] * 3),
    # the crossings of row 0 are 0, 0.5, 3.5, 4: the centre at 0.5 is on a right edge (out), the one at 3.5 on a left edge (in)
    "bow_tie": ([[[(0, 0), (4, 4), (4, 0), (0, 4)]]], [2], (4, 4), [[E, E, E, 2], [2, E, 2, 2], [2, E, 2, 2], [E, E, E, 2]]),
    "sliver": ([[[(1.6, 0), (1.9, 0), (1.9, 4), (1.6, 4)]]], [4], (4, 4), [[E] * 4] * 4),
    "overlap_ab": ([[[(0, 0), (3, 0), (3, 3), (0, 3)]], [[(1, 1), (4, 1), (4, 4), (1, 4)]]], [1, 2], (4, 4),
                   [[1, 1, 1, E], [1, 2, 2, 2], [1, 2, 2, 2], [E, 2, 2, 2]]),
    "overlap_ba": ([[[(1, 1), (4, 1), (4, 4), (1, 4)]], [[(0, 0), (3, 0), (3, 3), (0, 3)]]], [2, 1], (4, 4),
                   [[1, 1, 1, E], [1, 1, 1, 2], [1, 1, 1, 2], [E, 2, 2, 2]]),
}
