"""GPU: s2k_rasterize against the numpy restatement (tests/rasterize_ref.py), bit for bit.  Every raster the entry writes into is prefilled
with a canary, every call is made twice on fresh buffers and the two results are compared, and the public `classmap.rasterize` is held
against the same expectation.  Sizes sit around the block of one workgroup (RAST_BLOCK_H x RAST_BLOCK_W): one short, exact, one over, and
more than two blocks each way."""
import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import _lib, classmap
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from tests import rasterize_ref as R

pytestmark = pytest.mark.gpu

BH, BW = classmap.RAST_BLOCK_H, classmap.RAST_BLOCK_W
SIZES = [(1, 1), (1, BW + 1), (BH + 1, 1), (BH - 1, BW - 1), (BH, BW), (BH + 1, BW + 1), (2 * BH + 1, 2 * BW - 1)]
CANARY = {torch.uint8: 0xAB, torch.int32: -0x5A5A5A5A, torch.int64: -0x5A5A5A5A5A5A5A5A}
DEV = "cuda"


def raw_call(tab, origins, H, W, dtype=torch.uint8, mode="fill", burn="value", fill=0, base=None, S=None, want_unfilled=True):
    """One s2k_rasterize call over the device tables `tab` = (verts [V, 2], ring_start, ring_shape, values), all int32 arrays: the raster
    starts as the canary (or `base`), the call is made twice on fresh buffers and must give the same bits.  (raster, unfilled) on the host."""
    verts, ring_start, ring_shape, values = (None if a is None else np.asarray(a, dtype=np.int32) for a in tab)
    V, Rn = len(verts), len(ring_shape)
    S = (int(ring_shape.max()) + 1 if Rn else 0) if S is None else S
    dev = lambda a, pad: torch.from_numpy(np.concatenate([a.reshape(-1), np.zeros(pad, np.int32)])).to(DEV)      # noqa: E731
    t = dict(verts=dev(verts, 2), ring_start=dev(ring_start, 0), ring_shape=dev(ring_shape, 1), values=None if values is None else dev(values, 1))
    o = torch.tensor(np.asarray(origins).reshape(-1, 2), dtype=torch.int32, device=DEV)
    M = o.shape[0]
    results = []
    for _ in range(2):
        dst = torch.full((M, H, W), CANARY[dtype], dtype=dtype, device=DEV) if base is None else torch.as_tensor(base, dtype=dtype).to(DEV).clone()
        work = torch.full((_lib.rasterize_workspace(M, S) // 4,), -7, dtype=torch.int32, device=DEV)
        unfilled = torch.full((M,), 1000, dtype=torch.int64, device=DEV) if want_unfilled else None
        status = classmap.new_status(DEV)
        _lib.check(_lib.rasterize(t["verts"], t["ring_start"], t["ring_shape"], t["values"], o, dst, (V, Rn, S, M, H, W), _lib.RASTERIZE_MODES[mode],
                                  _lib.RASTERIZE_BURN[burn], fill, work, unfilled, status, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        results.append((dst.cpu(), None if unfilled is None else unfilled.cpu() - 1000))
    assert torch.equal(results[0][0], results[1][0]) and (not want_unfilled or torch.equal(results[0][1], results[1][1]))
    return results[0]


def host_tables(shapes, values):
    v, rs, sh = R.tables(shapes)
    return v, rs, sh, None if values is None else np.asarray(values)


def check(shapes, values, origins, H, W, dtype=torch.uint8, fill=0, **public):
    """the raw entry and `classmap.rasterize` against the restatement, in mode "fill" with burn = "value"; returns the expectation"""
    tab = host_tables(shapes, values)
    want, unfilled = R.rasterize(tab[0], tab[1], tab[2], values, len(shapes), origins, H, W, fill=fill)
    want_t = torch.from_numpy(want).to(dtype)
    got, got_unfilled = raw_call(tab, origins, H, W, dtype, fill=fill, S=len(shapes))
    assert torch.equal(got, want_t), f"{int((got != want_t).sum())} pixels differ"
    assert torch.equal(got_unfilled, torch.from_numpy(unfilled))
    ps = classmap.PolygonSet(shapes, values, device=DEV)
    for _ in range(2):
        pub, pub_unfilled = classmap.rasterize(ps, origins, (H, W), fill=fill, dtype=dtype, return_unfilled=True, **public)
        assert pub.dtype == dtype and torch.equal(pub.cpu(), want_t) and torch.equal(pub_unfilled.cpu(), torch.from_numpy(unfilled))
    return want, unfilled


@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_star_polygons_with_holes_that_reach_beyond_the_raster_on_every_side(size):
    H, W = size
    shapes, values = R.stars(4, 6, H, W, reach=0.8)
    v = R.tables(shapes)[0]
    assert v[:, 0].min() < 0 and v[:, 1].min() < 0 and v[:, 0].max() > R.Q * W and v[:, 1].max() > R.Q * H
    want, unfilled = check(shapes, values, [(0, 0)], H, W)
    assert H * W == 1 or len(np.unique(want)) >= 3              # several shapes show, so edges run through the raster


@pytest.mark.parametrize("size", [(BH + 1, BW + 1), (2 * BH + 1, 2 * BW - 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_tiles_with_their_own_origins_one_negative_one_outside_every_shape(size):
    H, W = size
    shapes, values = R.stars(5, 7, H, W, reach=0.7)
    origins = [(3, 2), (-W // 2, -H // 3), (40 * W, -30 * H)]
    want, unfilled = check(shapes, values, origins, H, W, fill=9)
    assert unfilled[2] == H * W and (want[2] == 9).all() and 0 < unfilled[0] < H * W and 0 < unfilled[1] < H * W
    assert not np.array_equal(want[0], want[1])


@pytest.mark.parametrize("name", list(R.TIES))
def test_the_hand_worked_tie_cases(name):
    shapes, values, (H, W), want = R.TIES[name]
    got, unfilled = check(shapes, values, [(0, 0)], H, W, fill=R.E)
    assert got[0].tolist() == [list(r) for r in want]


def test_the_tie_cases_inside_a_far_block():
    """the same geometry moved to where a block starts at its left (columns BW - 1 .. BW + 4, rows BH - 2 ..): every edge that ran
    through a centre still does, and the parity now enters the second column block from the left"""
    for name, (shapes, values, (H, W), want) in R.TIES.items():
        dx, dy = BW - 1, BH - 2
        moved = [[np.asarray(r, dtype=np.float64) + (dx, dy) for r in sh] for sh in shapes]
        got, _ = check(moved, values, [(0, 0)], BH + 4, BW + 6, fill=R.E)
        assert got[0, dy:dy + H, dx:dx + W].tolist() == [list(r) for r in want], name
        assert int((got[0] != R.E).sum()) == sum(v != R.E for r in want for v in r), name


def test_the_fan_partitions_the_hull():
    tris, hull = R.fan()
    H, W = 18, 21
    got, _ = check(tris, list(range(1, len(tris) + 1)), [(0, 0), (-2, 3)], H, W)
    inside = R.inside([R.quantise(r) for r in hull], 0, 0, H, W)
    assert np.array_equal(got[0] > 0, inside)
    # every triangle on its own, added up: each centre of the hull exactly once
    tab = host_tables(tris, [1] * len(tris))
    count = np.zeros((H, W), dtype=np.int64)
    for s in range(len(tris)):
        one = (tab[0][3 * s:3 * s + 3], np.array([0, 3]), np.array([0]), np.array([1]))
        count += raw_call(one, [(0, 0)], H, W, S=1)[0][0].numpy()
    assert np.array_equal(count, inside.astype(np.int64))


def test_a_polygon_across_three_blocks_each_way_with_edges_that_end_on_scan_lines():
    """3 x 3 blocks; the outline's vertices sit on pixel centres (y = i + 1/2: an edge ends exactly on a scan line, half open) and its
    slanted edges enter every column block from the left"""
    H, W = 2 * BH + 7, 2 * BW + 9
    outline = [(3.5, 1.5), (W - 2.5, 0.5), (W - 0.5, BH + 0.5), (BW + 0.5, BH - 0.5), (2 * BW + 1.5, 2 * BH + 0.5), (W - 4.5, H - 0.5),
               (BW - 0.5, 2 * BH + 1.5), (0.5, H - 1.5), (BW - 1.5, BH + 1.5), (1.5, BH + 0.5)]
    hole = [(5.5, 3.5), (5.5, BH - 3.5), (2 * BW + 2.5, BH - 2.5), (2 * BW + 0.5, 3.5)]
    want, unfilled = check([[outline, hole]], [200], [(0, 0), (1, 1)], H, W)
    assert 0.2 * H * W < unfilled[0] < 0.8 * H * W


def test_vertices_at_the_end_of_the_coordinate_range():
    """a triangle over +-(2^28 - 1) units whose long edge runs through a tile at the origin and through one near 2^20 pixels: the
    products of the crossing reach 2^58"""
    top = 2 ** 28 - 1
    tri = np.array([(-top, -top), (top, top - 777), (-top + 1000, top)], dtype=np.float64) / R.Q
    H, W = BH + 1, BW + 1
    far = 2 ** 20
    origins = [(-20, -30), (far - 500, far - 520), (far, far), (-far, -far), (-far, far - H)]
    want, unfilled = check([[tri]], [77], origins, H, W, dtype=torch.int32, fill=-3)
    for m in (0, 1):
        assert 0 < unfilled[m] < H * W, m                      # the edge crosses the tile
    assert unfilled[2] == H * W


def test_three_thousand_squares_in_order():
    shapes, values = R.squares()
    H, W = BH + 1, BW + 1
    want, unfilled = check(shapes, values, [(0, 0), (-5, 40)], H, W)
    first = want[0]
    assert len(np.unique(first)) == 6 and 0 < unfilled[0] < H * W
    # where the second square of a moved pair overlaps the first, the later value is there
    tab = host_tables(shapes, values)
    a, b = R.inside([tab[0][0:4]], 0, 0, H, W), R.inside([tab[0][4:8]], 0, 0, H, W)
    assert (a & b).sum() > 0 and (first[a & b] == values[1]).all() and values[0] != values[1]


def test_empty_tables_empty_shapes_and_short_rings_through_the_raw_entry():
    z = np.zeros(0, np.int32)
    for dtype in (torch.uint8, torch.int64):
        got, unfilled = raw_call((z, np.array([0]), z, z), [(0, 0), (5, 5)], 3, 70, dtype, fill=6, S=0)      # S = 0, R = 0, V = 0
        assert (got == 6).all() and unfilled.tolist() == [210, 210]
    base = np.arange(2 * 3 * 70).reshape(2, 3, 70) % 251
    got, unfilled = raw_call((z, np.array([0]), z, z), [(0, 0), (5, 5)], 3, 70, mode="onto", base=base, S=0)
    assert np.array_equal(got.numpy(), base) and unfilled.tolist() == [210, 210]
    got, _ = raw_call((z, np.array([0]), z, np.array([4, 5])), [(0, 0)], 2, 2, fill=1, S=2)                   # two shapes, no ring at all
    assert (got == 1).all()
    verts = R.quantise([(0, 0), (4, 4), (1, 1), (0, 0), (4, 0), (4, 4)])
    tab = (verts, np.array([0, 2, 3, 6, 6]), np.array([0, 0, 2, 3]), np.array([5, 6, 7, 8]))
    want, want_unfilled = R.rasterize(*tab, 4, [(0, 0), (1, 0)], 4, 4)
    got, unfilled = raw_call(tab, [(0, 0), (1, 0)], 4, 4, S=4)
    assert np.array_equal(got.numpy(), want) and unfilled.tolist() == want_unfilled.tolist() == [6, 7]
    ps = classmap.PolygonSet([], [], device=DEV)
    out = classmap.rasterize(ps, [(0, 0)], (5, 5), fill=2, dtype=torch.int32)
    assert out.dtype == torch.int32 and (out == 2).all()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64], ids=["uint8", "int32", "int64"])
def test_every_raster_type_in_both_modes(dtype):
    H, W = BH + 1, BW + 1
    shapes, values = R.stars(11, 6, H, W, reach=0.5)
    if dtype != torch.uint8:
        values = [-(2 ** 31), 2 ** 31 - 1, -1, 0, 70000, 255]
    origins = [(0, 0), (7, -9)]
    fill = 250 if dtype == torch.uint8 else -123456
    check(shapes, values, origins, H, W, dtype, fill=fill)
    # onto: what no shape covers keeps what the raster held, canary included
    tab = host_tables(shapes, values)
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (2, H, W)) if dtype == torch.uint8 else rng.integers(-2 ** 31, 2 ** 31, (2, H, W)) * (3 if dtype == torch.int64 else 1)
    want, want_unfilled = R.rasterize(tab[0], tab[1], tab[2], values, len(shapes), origins, H, W, base=base)
    got, unfilled = raw_call(tab, origins, H, W, dtype, mode="onto", base=base, fill=0)
    assert torch.equal(got, torch.from_numpy(want).to(dtype)) and unfilled.tolist() == want_unfilled.tolist()
    assert 0 < want_unfilled[0] < H * W and np.array_equal(want[0][want[0] == base[0]], base[0][want[0] == base[0]])
    ps = classmap.PolygonSet(shapes, values, device=DEV)
    out = torch.as_tensor(base, dtype=dtype).to(DEV)
    ret, pub_unfilled = classmap.rasterize(ps, origins, fill=None, out=out, return_unfilled=True)
    assert ret is out and torch.equal(out.cpu(), got) and pub_unfilled.tolist() == want_unfilled.tolist()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_burning_the_shape_index_gives_a_zone_raster(dtype):
    H, W = BH + 1, BW + 1
    shapes, _ = R.stars(13, 300, H, W, holes=False, reach=0.03)
    origins = [(0, 0), (-3, 5)]
    tab = host_tables(shapes, None)
    want, want_unfilled = R.rasterize(tab[0], tab[1], tab[2], None, len(shapes), origins, H, W, fill=-1, burn_index=True)
    got, unfilled = raw_call(tab, origins, H, W, dtype, burn="index", fill=-1, S=len(shapes))
    assert torch.equal(got, torch.from_numpy(want).to(dtype)) and unfilled.tolist() == want_unfilled.tolist()
    assert want.max() > 256 and len(np.unique(want)) > 100
    ps = classmap.PolygonSet(shapes, None, device=DEV)
    pub = classmap.rasterize(ps, origins, (H, W), fill=-1, dtype=dtype, burn="index")
    assert torch.equal(pub.cpu(), got)


def test_a_workspace_cap_that_forces_three_chunks():
    shapes, values = R.stars(17, 40, BH, BW, reach=0.3)
    origins = [(0, 0), (10, -10), (-BW // 2, 3), (BW // 3, BH // 2), (1, 1)]
    S = len(shapes)
    cap = classmap.rasterize_workspace_bytes(2, S)              # two tiles a chunk: 2 + 2 + 1
    assert classmap.tiles_per_chunk(S, cap) == 2
    want, _ = check(shapes, values, origins, BH, BW, max_workspace_bytes=cap)
    check(shapes, values, origins, BH, BW, max_workspace_bytes=1)      # one tile a chunk, whatever the cap
    assert len({want[m].tobytes() for m in range(5)}) == 5


def test_tables_the_host_cannot_see_set_the_status_and_raise():
    """Only the tables are wrong: every pointer and every count stays valid, and the kernels clamp what they read.  The status word says
    what was met; the raster is then not to be used, so nothing is asserted about it."""
    shapes, values = R.stars(19, 5, BH, BW, reach=0.6)

    def fresh():
        return classmap.PolygonSet(shapes, values, device=DEV)

    def status_of(ps, origins=((0, 0), (3, 3))):
        with pytest.raises(_lib.S2kError, match="rasterize: status") as err:
            classmap.rasterize(ps, origins, (BH + 1, BW + 1))
        torch.cuda.synchronize()
        return int(str(err.value).split("status ")[1].split()[0], 16)

    ps = fresh()
    V = ps.num_vertices
    ps.ring_start = torch.tensor([0, 2 ** 30, -5, 7, 3, V][:ps.num_rings + 1] + [V] * max(0, ps.num_rings - 5), dtype=torch.int32, device=DEV)
    assert status_of(ps) & 1
    ps = fresh()
    ps.ring_shape = torch.flip(ps.ring_shape[:ps.num_rings], [0]).contiguous()
    ps.ring_shape = torch.cat([ps.ring_shape, ps.ring_shape[-1:]])
    assert status_of(ps) & 1
    ps = fresh()
    ps.ring_shape = ps.ring_shape + 100                         # every ring names a shape at or above S
    assert status_of(ps) & 1
    ps = fresh()
    ps.verts[3, 0] = 2 ** 30
    ps.verts[5, 1] = -(2 ** 28) - 1
    assert status_of(ps) == 2
    assert status_of(fresh(), torch.tensor([[0, 0], [2 ** 20 + 1, 0]], dtype=torch.int32, device=DEV)) == 4
    out = classmap.rasterize(fresh(), [(0, 0)], (BH + 1, BW + 1))      # and the untouched set still rasterises
    assert torch.equal(out.cpu(), torch.from_numpy(R.rasterize_shapes(shapes, values, [(0, 0)], BH + 1, BW + 1)[0]).to(torch.uint8))


def test_the_pipeline_builds_its_labels_from_polygons_in_both_modes():
    N, C, H, W, S = 3, 4, 40, 44, 24
    g = torch.Generator().manual_seed(1)
    raw = torch.randint(-100, 100, (N, C, H, W), generator=g, dtype=torch.int32).to(torch.int16)
    codes = torch.randint(0, 24, (N, H, W), generator=g, dtype=torch.int32).to(torch.uint8)
    shapes, _ = R.stars(23, 6, H, W, reach=0.45)
    values = [1, 2, 3, 0, 2, 1]                                 # classes of cnes-multiclass; 0 masks a polygon out
    origins = [(0, 0), (-7, 9), (15, -4)]
    ps = classmap.PolygonSet(shapes, values, device=DEV)
    y0, x0 = (H - S) // 2, (W - S) // 2
    want, want_unfilled = R.rasterize_shapes(shapes, values, origins, H, W, fill=3)

    bare = GpuTilePipeline([0.1] * C, [0.2] * C, random_crop_size=S, label_map="cnes-multiclass", device=DEV)
    bare.load(raw, None)
    unfilled = bare.rasterize_labels(ps, origins, fill=3)
    assert unfilled.dtype == torch.int64 and unfilled.tolist() == want_unfilled.tolist() and 0 < want_unfilled.min()
    assert bare.labels.dtype == torch.uint8 and torch.equal(bare.labels.cpu(), torch.from_numpy(want).to(torch.uint8))
    assert torch.equal(bare.lut.cpu(), torch.arange(256, dtype=torch.int32))
    y = bare([0, 1, 2], training=False).y
    assert torch.equal(y.cpu(), torch.from_numpy(want[:, y0:y0 + S, x0:x0 + S]))

    pipe = GpuTilePipeline([0.1] * C, [0.2] * C, random_crop_size=S, label_map="cnes-multiclass", device=DEV)
    pipe.load(raw, codes)
    kept, table = pipe.labels, pipe.lut
    classes = table.cpu()[codes.long()].numpy()
    onto, onto_unfilled = R.rasterize_shapes(shapes, values, origins, H, W, base=classes)
    unfilled = pipe.rasterize_labels(ps, origins, onto=True)
    assert unfilled.tolist() == onto_unfilled.tolist() == want_unfilled.tolist()
    assert pipe.labels is not kept and pipe.lut is not table and torch.equal(kept.cpu(), codes)      # replaced, not written
    assert torch.equal(pipe.labels.cpu(), torch.from_numpy(onto).to(torch.uint8)) and not np.array_equal(onto, want)
    y = pipe([2, 0], training=False).y
    assert torch.equal(y.cpu(), torch.from_numpy(onto[[2, 0], y0:y0 + S, x0:x0 + S]))
    again = pipe.rasterize_labels(ps, origins, onto=True)      # the classes are already there: nothing moves
    assert again.tolist() == unfilled.tolist() and torch.equal(pipe.labels.cpu(), torch.from_numpy(onto).to(torch.uint8))
