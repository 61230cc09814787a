"""CPU: `s2k_rasterize` and `s2k_rasterize_workspace` are exported and declared (and the stage table and the ABI version did not move), the
entry validates every argument on the host before anything is launched, the numpy restatement (tests/rasterize_ref.py) gives the
hand-worked rasters of the tie cases, partitions a triangle fan and agrees with matplotlib away from the edges, `PolygonSet` quantises
and lays out its tables as documented, and `classmap.rasterize` and `GpuTilePipeline.rasterize_labels` raise ValueError for bad arguments
before they refuse to run off the GPU.  The entry is never called with valid arguments here: there is no device to launch on."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import _lib, classmap
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.plan import opdefs as D
from tests import rasterize_ref as R

ROOT = Path(__file__).resolve().parents[1]
S2K_EINVAL, S2K_EFAULT = -22, -14


def test_the_entries_are_exported_and_the_stage_table_is_unchanged():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g

    g.build()
    L = _lib.lib()
    so = ctypes.CDLL(str(g.LIB))
    assert hasattr(so, "s2k_rasterize") and hasattr(so, "s2k_rasterize_workspace")
    assert L.s2k_abi_version() == 2 and len(D.OPS) == 55
    assert "rasterize.hip" in g.SOURCES
    hdr = (ROOT / "include" / "s2k.h").read_text()
    assert re.search(r"\bint s2k_rasterize\s*\(", hdr) and re.search(r"\bsize_t s2k_rasterize_workspace\s*\(", hdr)
    assert "#define S2K_ABI_VERSION 2" in hdr
    assert _lib.RASTERIZE_MODES == {"fill": 0, "onto": 1} and _lib.RASTERIZE_BURN == {"value": 0, "index": 1}


def test_the_constants_are_the_kernel_file_s():
    src = (ROOT / "sentinel2-landcover-classification_amd" / "csrc" / "rasterize.hip").read_text()
    block = re.search(r"constexpr int RAST_BLOCK_H = (\d+), RAST_BLOCK_W = (\d+);", src)
    q = re.search(r"constexpr int RAST_Q = (\d+);", src)
    box = re.search(r"constexpr int RAST_BOX_INTS = (\d+);", src)
    assert block and q and box and "constexpr int RAST_MAX_COORD = 1 << 28;" in src
    assert (classmap.RAST_BLOCK_H, classmap.RAST_BLOCK_W) == tuple(int(v) for v in block.groups())
    assert classmap.RAST_Q == int(q.group(1)) == R.Q == 256 and classmap.RAST_MAX_COORD == 2 ** 28 == R.MAX_COORD
    assert classmap.RAST_BOX_INTS == int(box.group(1))
    assert classmap.RAST_BLOCK_W % 32 == 0 and (classmap.RAST_BLOCK_H * classmap.RAST_BLOCK_W // 32) % 256 == 0


def test_the_workspace_is_the_python_formula_s():
    for M, S in ((1, 0), (1, 1), (3, 7), (256, 200_000), (2048, 100_000)):
        assert _lib.rasterize_workspace(M, S) == classmap.rasterize_workspace_bytes(M, S) == 4 * (8 * S + M + M * S)
    assert _lib.rasterize_workspace(0, 5) == 0 and _lib.rasterize_workspace(3, -1) == 0
    for S, cap in ((0, 1), (10, 1 << 10), (3000, 40_000), (200_000, 256 << 20)):
        n = classmap.tiles_per_chunk(S, cap)
        assert n >= 1 and (n == 1 or classmap.rasterize_workspace_bytes(n, S) <= cap < classmap.rasterize_workspace_bytes(n + 1, S))


# ---- host-side validation: a valid call over CPU tensors (never made): V, R, S, M, H, W = 7, 2, 2, 3, 40, 50 ------------------------------
I32 = dict(dtype=torch.int32)
GOOD = dict(V=7, R=2, S=2, M=3, H=40, W=50, mode=0, burn=0, fill=0, dst_bytes=1)
TENSORS = dict(verts=torch.zeros(8, 2, **I32), ring_start=torch.zeros(3, **I32), ring_shape=torch.zeros(2, **I32), values=torch.zeros(2, **I32),
               origins=torch.zeros(3, 2, **I32), dst=torch.zeros(3, 40, 50, dtype=torch.int64), work=torch.zeros(64, **I32),
               unfilled=torch.zeros(3, dtype=torch.int64), status=torch.zeros(1, **I32))


def _call(**change):
    a = {**GOOD, **{k: v for k, v in change.items() if k in GOOD}}
    t = {**TENSORS, **{k: v for k, v in change.items() if k in TENSORS}}
    rc = _lib.rasterize(t["verts"], t["ring_start"], t["ring_shape"], t["values"], t["origins"], t["dst"],
                        (a["V"], a["R"], a["S"], a["M"], a["H"], a["W"]), a["mode"], a["burn"], a["fill"], t["work"], t["unfilled"], t["status"], 0,
                        dst_bytes=a["dst_bytes"])
    return rc, _lib.lib().s2k_last_error().decode()


BAD = [dict(M=0), dict(M=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1), dict(M=1 << 20, H=1 << 20, W=1 << 20), dict(H=1 << 16, W=1 << 15),
       dict(M=(1 << 31) - 1, H=512, W=512), dict(M=1 << 29, H=33, W=513), dict(V=-1), dict(R=-1), dict(S=-1), dict(V=-7, R=-2, S=-2),
       dict(V=1, R=2), dict(R=0), dict(S=0), dict(dst_bytes=0), dict(dst_bytes=2), dict(dst_bytes=3), dict(dst_bytes=16), dict(dst_bytes=-1),
       dict(mode=2), dict(mode=-1), dict(burn=2), dict(burn=-1), dict(burn=1, dst_bytes=1), dict(values=None), dict(values=None, dst_bytes=8),
       dict(fill=256), dict(fill=-1), dict(fill=1 << 20, mode=1),
       dict(verts=torch.zeros(9, **I32)[1:]), dict(origins=torch.zeros(7, **I32)[1:]), dict(work=torch.zeros(65, **I32)[1:])]


def _ids(cases):
    return [",".join(f"{k}={'t' if isinstance(v, torch.Tensor) else v}" for k, v in b.items()) for b in cases]


@pytest.mark.parametrize("bad", BAD, ids=_ids(BAD))
def test_rasterize_rejects_invalid_arguments_on_the_host(bad):
    rc, msg = _call(**bad)
    assert rc == S2K_EINVAL and msg.startswith("rasterize: ") and len(msg) > 24, (rc, msg)


@pytest.mark.parametrize("name", ["verts", "ring_start", "ring_shape", "origins", "dst", "work", "status"])
def test_rasterize_rejects_a_null_among_the_required_pointers(name):
    rc, msg = _call(**{name: None})
    assert rc == S2K_EFAULT and msg.startswith("rasterize: null pointer"), (rc, msg)
    with pytest.raises(_lib.S2kError, match="null pointer"):
        _lib.check(rc)
    rc, msg = _call(**{name: None}, dst_bytes=3, M=0)        # the NULL is reported first
    assert rc == S2K_EFAULT


def test_what_may_be_null_and_what_is_wide_enough_is_not_complained_about():
    """values with burn = index, unfilled, and a fill outside a byte for a wider dst are all fine: what is still wrong is what is reported"""
    rc, msg = _call(values=None, burn=1, dst_bytes=8, unfilled=None, fill=-5, mode=7)
    assert rc == S2K_EINVAL and "mode = 7" in msg
    rc, msg = _call(values=None, S=0, R=0, V=0, fill=300, dst_bytes=4, burn=9)
    assert rc == S2K_EINVAL and "burn = 9" in msg


# ---- the restatement against hand-worked rasters ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.TIES))
def test_the_restatement_on_the_hand_worked_tie_cases(name):
    shapes, values, (H, W), want = R.TIES[name]
    got, unfilled = R.rasterize_shapes(shapes, values, [(0, 0)], H, W, fill=R.E)
    assert got[0].tolist() == [list(r) for r in want]
    assert unfilled.tolist() == [sum(v == R.E for r in want for v in r)]


def test_the_restatement_moves_with_the_origin_and_keeps_a_base():
    shapes, values, (H, W), want = R.TIES["vertices_on_centres"]
    whole = np.array(want)
    got, _ = R.rasterize_shapes(shapes, values, [(1, 2), (-3, -1), (40, 40)], 3, 4, fill=8)
    big = np.full((20, 20), R.E)
    big[5:10, 5:10] = whole                                     # AOI pixel (x, y) at big[y + 5, x + 5]
    for m, (ox, oy) in enumerate([(1, 2), (-3, -1), (40, 40)]):
        view = big[oy + 5:oy + 8, ox + 5:ox + 9] if ox < 15 else np.zeros((3, 4), int)
        assert np.array_equal(got[m], np.where(view == R.E, 8, view)), m
    base = np.arange(25).reshape(1, 5, 5) + 100
    onto, unfilled = R.rasterize_shapes(shapes, values, [(0, 0)], 5, 5, base=base)
    assert np.array_equal(onto[0], np.where(whole == R.E, base[0], whole)) and unfilled.tolist() == [17] and base[0, 1, 1] == 106
    index, _ = R.rasterize_shapes(R.TIES["overlap_ab"][0], None, [(0, 0)], 4, 4, fill=-1, burn_index=True)
    assert index[0].tolist() == [[0, 0, 0, -1], [0, 1, 1, 1], [0, 1, 1, 1], [-1, 1, 1, 1]]


def test_a_ring_of_two_vertices_and_a_shape_without_rings_cover_nothing():
    verts = R.quantise([(0, 0), (4, 4), (1, 1), (0, 0), (4, 0), (4, 4)])
    # shape 0: a ring of 2 vertices and one of 1; shape 1: no ring; shape 2: a triangle; shape 3: a ring of 0 vertices
    got, unfilled = R.rasterize(verts, [0, 2, 3, 6, 6], [0, 0, 2, 3], [5, 6, 7, 8], 4, [(0, 0)], 4, 4)
    # the triangle's diagonal runs through the centres of the diagonal pixels: it is a left edge, so they are inside
    assert got[0].tolist() == [[7, 7, 7, 7], [0, 7, 7, 7], [0, 0, 7, 7], [0, 0, 0, 7]] and unfilled.tolist() == [6]


def test_a_fan_around_a_hub_on_a_pixel_centre_covers_every_centre_of_the_hull_once():
    tris, hull = R.fan()
    H, W = 18, 21
    count = sum(R.inside([R.quantise(r) for r in t], 0, 0, H, W).astype(int) for t in tris)
    want = R.inside([R.quantise(r) for r in hull], 0, 0, H, W)
    assert want.sum() > 150 and want[8, 10]                    # the hub's own pixel
    assert np.array_equal(count, want.astype(int))


def _edge_distance(px, py, ring):
    """float64 [P]: the distance of every point to the nearest edge of the closed ring"""
    a, b = ring, np.roll(ring, -1, axis=0)
    d = b - a
    t = ((px[:, None] - a[None, :, 0]) * d[None, :, 0] + (py[:, None] - a[None, :, 1]) * d[None, :, 1]) / np.maximum((d * d).sum(1), 1e-300)[None, :]
    t = np.clip(t, 0.0, 1.0)
    return np.hypot(px[:, None] - (a[None, :, 0] + t * d[None, :, 0]), py[:, None] - (a[None, :, 1] + t * d[None, :, 1])).min(1)


def test_the_rule_agrees_with_matplotlib_away_from_the_edges():
    """200 star polygons, every other one with a hole, on a 67 x 131 raster: among the centres farther than 1 / 128 px from every edge
    there is no disagreement with matplotlib.path (ring parities XOR-ed), and those nearer - where float rounding and matplotlib's own
    tie rule decide - are at most 1 % of all, so that the test cannot exclude its way to a pass."""
    from matplotlib.path import Path as MplPath

    H, W = 67, 131
    shapes, _ = R.stars(0, 200, H, W)
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    px, py = jj.ravel(), ii.ravel()
    wrong = excluded = 0
    for rings in shapes:
        units = [R.quantise(r) for r in rings]
        got = R.inside(units, 0, 0, H, W).ravel()
        want = np.zeros(H * W, dtype=bool)
        near = np.zeros(H * W, dtype=bool)
        for u in units:
            ring = u / R.Q                                      # the quantised geometry: what both sides are asked about
            want ^= MplPath(np.concatenate([ring, ring[:1]]), closed=True).contains_points(np.stack([px, py], axis=1))
            near |= _edge_distance(px, py, ring) <= 1 / 128
        wrong += int((got != want)[~near].sum())
        excluded += int(near.sum())
    share = excluded / (len(shapes) * H * W)
    print(f"excluded {excluded} of {len(shapes) * H * W} centres ({100 * share:.3f} %), {wrong} disagreements among the rest")
    assert wrong == 0
    assert share <= 0.01


# ---- PolygonSet -------------------------------------------------------------------------------------------------------------------------
def test_quantisation_rounds_halves_up_also_below_zero():
    v = [0.0, 1.0, 0.5 / 256, 1.5 / 256, -0.5 / 256, -1.5 / 256, 0.49 / 256, -0.51 / 256, -1.0, 3.25, 2.0 ** 20, -(2.0 ** 20)]
    want = [0, 256, 1, 2, 0, -1, 0, -1, -256, 832, 2 ** 28, -(2 ** 28)]
    assert classmap.quantise(v).tolist() == want == R.quantise(v).tolist()
    for bad in ([2.0 ** 20 + 1 / 256], [-(2.0 ** 20) - 1 / 256], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            classmap.quantise(bad)


def test_a_polygon_set_lays_out_the_tables_of_the_entry():
    shapes = [[[(0, 0), (4, 0), (4, 4)], [(1, 0.5), (3, 0.5), (3, 2)]], [], [[(0.5 / 256, -1), (2, -1), (2, 2), (0, 2.25)]]]
    p = classmap.PolygonSet(shapes, [3, 200, 1], device="cpu")
    assert (p.num_shapes, p.num_rings, p.num_vertices) == (3, 3, 10)
    assert p.host["ring_start"].tolist() == [0, 3, 6, 10] and p.host["ring_shape"].tolist() == [0, 0, 2] and p.host["values"].tolist() == [3, 200, 1]
    assert p.host["verts"][6:].tolist() == [[1, -256], [512, -256], [512, 512], [0, 576]]
    v, rs, sh = R.tables(shapes)
    assert np.array_equal(p.host["verts"], v) and np.array_equal(p.host["ring_start"], rs) and np.array_equal(p.host["ring_shape"], sh)
    for t in (p.verts, p.ring_start, p.ring_shape, p.values):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.data_ptr() != 0
    assert p.verts[:10].tolist() == p.host["verts"].tolist() and p.ring_start.tolist() == [0, 3, 6, 10]
    empty = classmap.PolygonSet([], [], device="cpu")
    assert (empty.num_shapes, empty.num_rings, empty.num_vertices) == (0, 0, 0) and empty.verts.data_ptr() != 0 and empty.ring_start.tolist() == [0]
    assert classmap.PolygonSet(shapes, None, device="cpu").values is None


def test_from_world_is_the_reference_s_from_origin_transform():
    west, north, xs, ys = 600000.0, 5400000.0, 10.0, 10.0
    world = [[[(600005.0, 5399995.0), (600105.0, 5399995.0), (600105.0, 5399897.5)]]]
    p = classmap.PolygonSet.from_world(world, [1], west, north, xs, ys, device="cpu")
    want = [[(x - west) / xs, (north - y) / ys] for x, y in world[0][0]]
    assert want == [[0.5, 0.5], [10.5, 0.5], [10.5, 10.25]]
    assert p.host["verts"].tolist() == R.quantise(want).tolist() == [[128, 128], [2688, 128], [2688, 2624]]
    for bad in (dict(xsize=0.0), dict(ysize=-10.0), dict(west=float("nan")), dict(north="n")):
        with pytest.raises(ValueError):
            classmap.PolygonSet.from_world(world, [1], **{**dict(west=west, north=north, xsize=xs, ysize=ys), **bad}, device="cpu")


def test_from_geojson_reads_polygons_and_multipolygons_and_drops_the_closing_vertex():
    poly = {"type": "Polygon", "coordinates": [[(0, 0), (6, 0), (6, 6), (0, 6), (0, 0)], [(2, 2), (2, 4), (4, 4), (4, 2), (2, 2)]]}
    multi = {"type": "MultiPolygon", "coordinates": [[[(0, 0, 9.0), (2, 0, 9.0), (2, 2, 9.0), (0, 0, 9.0)]], [[(3, 3), (5, 3), (5, 5)]]]}

    class Geo:
        __geo_interface__ = poly

    p = classmap.PolygonSet.from_geojson([poly, multi, Geo()], [5, 6, 7], device="cpu")
    assert (p.num_shapes, p.num_rings, p.num_vertices) == (3, 6, 22)
    assert p.host["ring_start"].tolist() == [0, 4, 8, 11, 14, 18, 22] and p.host["ring_shape"].tolist() == [0, 0, 1, 1, 2, 2]
    assert p.host["verts"][8:11].tolist() == [[0, 0], [512, 0], [512, 512]]          # the z coordinate is ignored
    got, _ = R.rasterize(p.host["verts"], p.host["ring_start"][:5], p.host["ring_shape"][:4], [5, 6], 2, [(0, 0)], 6, 6)      # the first two
    # the hole stays open but for the second part of the multi-polygon, whose diagonal runs through centres: a left edge, so they are in
    assert got[0].tolist() == [[6, 6, 5, 5, 5, 5], [5, 6, 5, 5, 5, 5], [5, 5, 0, 0, 5, 5], [5, 5, 0, 6, 6, 5], [5, 5, 5, 5, 6, 5], [5] * 6]
    world = classmap.PolygonSet.from_geojson([{"type": "Polygon", "coordinates": [[(100.0, 50.0), (120.0, 50.0), (120.0, 30.0), (100.0, 50.0)]]}], [1],
                                             west=100.0, north=50.0, xsize=10.0, ysize=10.0, device="cpu")
    assert world.host["verts"].tolist() == [[0, 0], [512, 0], [512, 512]]
    for bad in ({"type": "LineString", "coordinates": [(0, 0), (1, 1)]}, {"type": "Point", "coordinates": (0, 0)},
                {"type": "GeometryCollection", "geometries": []}, {"coordinates": []}, 7):
        with pytest.raises(ValueError):
            classmap.PolygonSet.from_geojson([bad], [1], device="cpu")
    with pytest.raises(ValueError, match="together"):
        classmap.PolygonSet.from_geojson([poly], [1], west=0.0, device="cpu")


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
SQUARE = [[[(0, 0), (4, 0), (4, 4), (0, 4)]]]


def _cpu_pipe(labels=True):
    p = GpuTilePipeline([0.1] * 4, [0.2] * 4, random_crop_size=8, label_map="cnes-multiclass", device="cpu")
    g = torch.Generator().manual_seed(0)
    p.load(torch.randint(-100, 100, (3, 4, 16, 16), generator=g, dtype=torch.int32).to(torch.int16),
           torch.randint(0, 24, (3, 16, 16), generator=g, dtype=torch.int32).to(torch.uint8) if labels else None)
    return p


def test_validators_raise_before_the_gpu_refusal():
    new = lambda shapes, values=(1,): classmap.PolygonSet(shapes, None if values is None else list(values), device="cpu")      # noqa: E731
    ps, wide, bare = new(SQUARE), new(SQUARE, [300]), new(SQUARE, None)
    rz = classmap.rasterize
    o = [(0, 0), (8, 8)]
    out8 = torch.zeros(2, 8, 8, dtype=torch.uint8)
    pipe = _cpu_pipe()
    o3 = [(0, 0)] * 3
    bad = [
        lambda: new([[[(0, 0), (1, 1)]]]), lambda: new([[[]]]), lambda: new([[[(0, 0, 0), (1, 1, 1), (2, 0, 0)]]]), lambda: new([[[0, 1, 2]]]),
        lambda: new(7), lambda: new([[[(0, 0), (1, 1), (float("nan"), 0)]]]), lambda: new([[[(0, 0), (1, 1), (2.0 ** 20 + 1, 0)]]]),
        lambda: new([[[(0, 0), (1, 1), (0, -(2.0 ** 20) - 0.01)]]]), lambda: new(SQUARE, [1, 2]), lambda: new(SQUARE, []), lambda: new(SQUARE, [1.5]),
        lambda: new(SQUARE, [1 << 31]), lambda: new(SQUARE, ["a"]),
        lambda: rz(SQUARE, o, (8, 8)), lambda: rz(ps, o, (8, 8), burn="id"), lambda: rz(ps, o, (8, 8), burn="index"),
        lambda: rz(ps, o, (8, 8), dtype=torch.int16), lambda: rz(ps, o, (8, 8), dtype=torch.float32), lambda: rz(ps, o, (0, 8)),
        lambda: rz(ps, o, (8, -1)), lambda: rz(ps, o, 8), lambda: rz(ps, o, (8.0, 8)), lambda: rz(ps, o, (1 << 16, 1 << 15)), lambda: rz(ps, o),
        lambda: rz(ps, o, (8, 8), fill=256), lambda: rz(ps, o, (8, 8), fill=-1), lambda: rz(ps, o, (8, 8), fill=None), lambda: rz(ps, o, (8, 8), fill=1.0),
        lambda: rz(ps, o, (8, 8), fill=1 << 31, dtype=torch.int32), lambda: rz(wide, o, (8, 8)), lambda: rz(bare, o, (8, 8)),
        lambda: rz(ps, o, (8, 8), max_workspace_bytes=0), lambda: rz(ps, o, (8, 8), max_workspace_bytes=1.5),
        lambda: rz(ps, [], (8, 8)), lambda: rz(ps, [(0, 0, 0)], (8, 8)), lambda: rz(ps, [0, 0], (8, 8)), lambda: rz(ps, [(0.5, 0)], (8, 8)),
        lambda: rz(ps, [(1 << 20) + 1, 0], (8, 8)), lambda: rz(ps, [((1 << 20) + 1, 0)], (8, 8)), lambda: rz(ps, [(0, -(1 << 20) - 1)], (8, 8)),
        lambda: rz(ps, torch.zeros(2, 2), (8, 8)), lambda: rz(ps, torch.zeros(2, 3, dtype=torch.int32), (8, 8)),
        lambda: rz(ps, o, out=out8), lambda: rz(ps, o, fill=0, out=out8), lambda: rz(ps, o, (8, 9), fill=None, out=out8),
        lambda: rz(ps, o, fill=None, out=out8.float()), lambda: rz(ps, o, fill=None, out=out8[0]), lambda: rz(ps, o, fill=None, out=out8[:, :, ::2]),
        lambda: rz(ps, o + o, fill=None, out=out8), lambda: rz(ps, o, fill=None, out=out8, burn="index"), lambda: rz(wide, o, fill=None, out=out8),
        lambda: pipe.rasterize_labels(SQUARE, o3), lambda: pipe.rasterize_labels(ps, o), lambda: pipe.rasterize_labels(ps, o3, fill=4),
        lambda: pipe.rasterize_labels(ps, o3, fill=-1), lambda: pipe.rasterize_labels(ps, o3, fill=True), lambda: pipe.rasterize_labels(new(SQUARE, [4]), o3),
        lambda: pipe.rasterize_labels(new(SQUARE, [-1]), o3), lambda: pipe.rasterize_labels(bare, o3), lambda: pipe.rasterize_labels(ps, o3, fill=1, onto=True),
        lambda: pipe.rasterize_labels(ps, [(0, 1 << 21)] * 3), lambda: _cpu_pipe(labels=False).rasterize_labels(ps, o3, onto=True),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} did not raise")


def test_the_new_functions_refuse_the_cpu():
    ps = classmap.PolygonSet(SQUARE, [1], device="cpu")
    o = [(0, 0), (8, 8)]
    pipe, bare = _cpu_pipe(), _cpu_pipe(labels=False)
    before = pipe.labels
    calls = (lambda: classmap.rasterize(ps, o, (8, 8)), lambda: classmap.rasterize(ps, torch.tensor(o), (8, 8), fill=3, dtype=torch.int64, burn="index"),
             lambda: classmap.rasterize(ps, o, (8, 8), return_unfilled=True, max_workspace_bytes=64),
             lambda: classmap.rasterize(ps, o, fill=None, out=torch.zeros(2, 8, 8, dtype=torch.int32)),
             lambda: classmap.rasterize(classmap.PolygonSet([], [], device="cpu"), o, (8, 8)),
             lambda: pipe.rasterize_labels(ps, [(0, 0)] * 3), lambda: pipe.rasterize_labels(ps, torch.zeros(3, 2, dtype=torch.int64), fill=2),
             lambda: pipe.rasterize_labels(ps, [(0, 0)] * 3, onto=True), lambda: bare.rasterize_labels(ps, [(0, 0)] * 3))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert pipe.labels is before and bare.labels is None        # nothing was replaced
    with pytest.raises(RuntimeError, match="load"):
        GpuTilePipeline([0.1] * 4, [0.2] * 4, random_crop_size=8, device="cpu").rasterize_labels(ps, [(0, 0)])
