"""GPU: the four zonal entries and the public functions of zonal.py against the numpy restatement (tests/zonal_ref.py), bit for bit.  Every
table an entry adds to is prefilled with a non-zero canary, every call is made twice on fresh buffers and the two results are compared.
Sizes sit around the block of one workgroup (ZONAL_BLOCK_H x ZONAL_BLOCK_W): one short, exact, one over, and more than two blocks each
way; the zone rasters are built to fill the LDS table exactly, to overfill it, to exhaust the probes of one home slot, and to contend for
one table row from every block."""
import functools

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import _lib, classmap, zonal
from s2lc_amd import predict as P
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from tests import rasterize_ref as RR
from tests import zonal_ref as R

pytestmark = pytest.mark.gpu

BH, BW, SLOTS, PROBES = zonal.ZONAL_BLOCK_H, zonal.ZONAL_BLOCK_W, zonal.ZONAL_SLOTS, zonal.ZONAL_PROBES
SIZES = [(1, 1), (1, BW + 1), (BH + 1, 1), (BH - 1, BW - 1), (BH, BW), (BH + 1, BW + 1), (2 * BH + 1, 2 * BW - 1)]
MAPS = [1, 2, 3, 1, 2, 3, 2]
CANARY = 1_000_000_007
PIX = {torch.uint8: 0xAB, torch.int32: -0x5A5A5A5A, torch.int64: -0x5A5A5A5A5A5A5A5A}
NP = {torch.uint8: np.uint8, torch.int32: np.int32, torch.int64: np.int64}
DEV = "cuda"


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def run_hist(zone, cls, Z, K, stride=0, lut=None, want_status=0, zdtype=torch.int32):
    """s2k_zonal_histogram twice over canary tables, against the restatement; returns the counts without the canary"""
    want, status = R.histogram(zone, cls, Z, K, stride, lut, hist=np.full((Z, K), CANARY))
    assert status == want_status
    z, c, table = dev(zone, zdtype), dev(cls), None if lut is None else dev(lut, torch.int32)
    got = []
    for _ in range(2):
        hist, st = torch.full((Z, K), CANARY, dtype=torch.int64, device=DEV), classmap.new_status(DEV)
        _lib.check(_lib.zonal_histogram(z, stride, c, table, (*z.shape, Z, K), hist, st, stream()))
        torch.cuda.synchronize()
        assert int(st.item()) == want_status
        got.append(hist.cpu())
    assert torch.equal(got[0], got[1])
    assert torch.equal(got[0], torch.from_numpy(want)), f"{int((got[0] != torch.from_numpy(want)).sum())} bins differ"
    return want - CANARY


def run_bands(zone, vals, Z, stride=0, nodata=None, want_status=0, zdtype=torch.int32):
    """s2k_zonal_bands twice over canary tables (min / max as a caller initialises them), against the restatement"""
    C = vals.shape[1]
    want, status = R.bands(zone, vals, Z, stride, nodata, tables=R.new_tables(Z, C, CANARY))
    assert status == want_status
    z, v = dev(zone, zdtype), dev(vals, torch.int16)
    got = []
    for _ in range(2):
        st = classmap.new_status(DEV)
        t = [dev(a) for a in R.new_tables(Z, C, CANARY)]
        _lib.check(_lib.zonal_bands(z, stride, v, (v.shape[0], C, *v.shape[2:], Z), nodata, *t, st, stream()))
        torch.cuda.synchronize()
        assert int(st.item()) == want_status
        got.append([a.cpu() for a in t])
    for name, a, b, w in zip(("count", "sum", "sumsq", "min", "max"), got[0], got[1], want):
        assert torch.equal(a, b), name
        assert torch.equal(a, torch.from_numpy(w)), f"{name}: {int((a != torch.from_numpy(w)).sum())} entries differ"
    return want


def run_paint(zone, table, dtype, mode=0, fill=0, stride=0, want_status=0, zdtype=torch.int32):
    """s2k_zonal_paint twice over a canary raster, against the restatement"""
    base = np.full(np.shape(zone), PIX[dtype], dtype=NP[dtype])
    want, status = R.paint(zone, table, NP[dtype], mode, fill, stride, base=base)
    assert status == want_status
    z, t = dev(zone, zdtype), dev(table, torch.int32)
    got = []
    for _ in range(2):
        dst, st = dev(base.copy()), classmap.new_status(DEV)
        _lib.check(_lib.zonal_paint(z, stride, t, (*z.shape, t.numel()), dst, mode, fill, st, stream()))
        torch.cuda.synchronize()
        assert int(st.item()) == want_status
        got.append(dst.cpu())
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], torch.from_numpy(want)), f"{int((got[0] != torch.from_numpy(want)).sum())} pixels differ"
    return want


def rasters(seed, M, H, W, K=4, C=6, lo=-2000, hi=12000):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, K + 2, (M, H, W)).astype(np.uint8)              # two classes outside [0, K)
    vals = rng.integers(lo, hi, (M, C, H, W)).astype(np.int16)
    vals[rng.random(vals.shape) < 0.1] = 0                                # nodata
    return rng, cls, vals


# ---- every size: patches of a few pixels with ids drawn from [-1, Z) --------------------------------------------------------------------------
@pytest.mark.parametrize("size,M", list(zip(SIZES, MAPS)), ids=[f"{h}x{w}x{m}" for (h, w), m in zip(SIZES, MAPS)])
@pytest.mark.parametrize("zdtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_every_entry_and_public_function_at_every_size(size, M, zdtype):
    (H, W), Z, K = size, 37, 4
    rng, cls, vals = rasters(H * 1000 + W + M, M, H, W)
    zone = R.patches(M, H, W, rng.integers(-1, Z, 4099), ph=3, pw=5)
    hist = run_hist(zone, cls, Z, K, zdtype=zdtype)
    want_b = run_bands(zone, vals, Z, nodata=0, zdtype=zdtype)
    cls_z, _ = R.majority(hist, 0xf)
    want_p = run_paint(zone, cls_z, torch.uint8, fill=9, zdtype=zdtype)
    # the public functions on the same inputs
    z, c, v = dev(zone, zdtype), dev(cls), dev(vals)
    assert torch.equal(zonal.histogram(z, c, Z, K).cpu(), torch.from_numpy(hist))
    acc = torch.full((Z, K), 5, dtype=torch.int64, device=DEV)
    assert zonal.histogram(z, c, Z, K, out=acc) is acc and torch.equal(acc.cpu(), torch.from_numpy(hist + 5))
    st = zonal.band_stats(z, v, Z, nodata=0)
    for got, want, canary in zip((st.count, st.sum, st.sumsq, st.min, st.max), want_b, (CANARY, CANARY, CANARY, 0, 0)):
        assert torch.equal(got.cpu(), torch.from_numpy(want - canary))
    n = want_b[0] - CANARY
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(n > 0, (want_b[1] - CANARY) / n, np.nan)
    assert np.array_equal(st.mean().cpu().numpy(), mean, equal_nan=True) and bool((st.std().isnan() == (st.count == 0)).all())
    got_cls, got_best = zonal.majority(torch.from_numpy(hist).to(DEV), return_count=True)
    assert torch.equal(got_cls.cpu(), torch.from_numpy(cls_z)) and torch.equal(got_best.cpu(), torch.from_numpy(hist.max(1)))
    assert torch.equal(zonal.paint(z, got_cls, fill=9).cpu(), torch.from_numpy(want_p))
    clean = zonal.majority_by_zone(c, z, Z, K)
    want_clean, _ = R.paint(zone, cls_z, np.uint8, mode=1, base=cls)
    assert clean.dtype == torch.uint8 and torch.equal(clean.cpu(), torch.from_numpy(want_clean))


# ---- the LDS table: how many distinct zones a block holds --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, SLOTS - 1, SLOTS, SLOTS + 1, BH * BW], ids=["one", "slots-1", "slots", "slots+1", "every_pixel"])
@pytest.mark.parametrize("size", [(BH, BW), (2 * BH + 1, 2 * BW - 1)], ids=["block", "blocks"])
def test_distinct_zones_inside_one_block(n, size):
    H, W = size
    _, cls, vals = rasters(n, 1, H, W, C=2)
    zone = R.block_ids(H, W, n, BH, BW)
    assert len(np.unique(zone[0, :BH, :BW])) == n
    run_hist(zone, cls, n, 4)
    run_bands(zone, vals, n)


@pytest.mark.parametrize("n", [PROBES - 1, PROBES, PROBES + 1])
def test_zones_that_share_one_home_slot(n):
    ids = R.keys_sharing_a_home(n, zonal.ZONAL_SLOT_BITS, start=3)
    assert len({zonal.home_slot(k) for k in ids}) == 1
    H, W, Z = BH + 1, BW + 1, max(ids) + 1
    _, cls, vals = rasters(n, 2, H, W, C=3)
    zone = np.concatenate([R.block_ids(H, W, n, BH, BW, ids), R.patches(1, H, W, ids, ph=2, pw=7)])
    run_hist(zone, cls, Z, 4)
    run_bands(zone, vals, Z, nodata=0)


# ---- contention and the flush across blocks ------------------------------------------------------------------------------------------------------
def _contention(kind, M, H, W):
    y, x = np.mgrid[0:H, 0:W]
    if kind == "one_zone":
        return np.zeros((M, H, W), np.int32), 1
    if kind == "vertical_stripes":
        return np.broadcast_to(x, (M, H, W)).astype(np.int32), W
    if kind == "horizontal_stripes":
        return np.broadcast_to(y, (M, H, W)).astype(np.int32), H
    rng = np.random.default_rng(5)                                       # zone 0 in every block, between patches of other zones
    zone = R.patches(M, H, W, rng.integers(1, 200, 977), ph=4, pw=9)
    zone[:, ::3, :] = 0
    return zone, 200


@pytest.mark.parametrize("kind", ["one_zone", "vertical_stripes", "horizontal_stripes", "in_every_block"])
def test_contention_and_flush_across_blocks(kind):
    M, (H, W) = 3, SIZES[-1]
    zone, Z = _contention(kind, M, H, W)
    _, cls, vals = rasters(11, M, H, W, C=6)
    hist = run_hist(zone, cls, Z, 4)
    assert hist.sum() == int((cls < 4).sum())
    run_bands(zone, vals, Z, nodata=0)


# ---- zone values out of range ---------------------------------------------------------------------------------------------------------------------
def test_all_negative_zones_leave_the_tables_untouched():
    H, W = BH + 1, BW + 1
    _, cls, vals = rasters(1, 2, H, W)
    zone = np.full((2, H, W), -1, np.int32)
    zone[1] = -(1 << 31)
    assert not run_hist(zone, cls, 5, 4).any()
    assert not (run_bands(zone, vals, 5)[0] - CANARY).any()
    run_paint(zone, np.arange(5), torch.int32, mode=1)
    run_paint(zone.astype(np.int64) - (1 << 40), np.arange(5), torch.int32, mode=0, fill=-3, zdtype=torch.int64)


@pytest.mark.parametrize("zdtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_a_value_at_the_limit_is_skipped_and_reported(zdtype):
    H, W, Z = BH + 1, BW + 1, 9
    rng, cls, vals = rasters(2, 2, H, W)
    zone = R.patches(2, H, W, rng.integers(0, Z, 500), ph=2, pw=3)
    zone[1, H // 2, W // 3] = Z
    run_hist(zone, cls, Z, 4, want_status=R.BAD_ZONE, zdtype=zdtype)
    run_bands(zone, vals, Z, want_status=R.BAD_ZONE, zdtype=zdtype)
    run_paint(zone, np.arange(Z), torch.int64, want_status=R.BAD_ZONE, zdtype=zdtype)
    with pytest.raises(_lib.S2kError, match="zonal: status 0x1"):
        zonal.histogram(dev(zone, zdtype), dev(cls), Z, 4)
    with pytest.raises(_lib.S2kError, match="zonal: status 0x1"):
        zonal.paint(dev(zone, zdtype), torch.zeros(Z, dtype=torch.int32, device=DEV))


def test_int64_zone_values_beyond_32_bits_are_out_of_range_not_truncated():
    H, W, Z = BH, BW, 9
    rng, cls, vals = rasters(3, 1, H, W)
    zone = R.patches(1, H, W, rng.integers(0, Z, 500), ph=2, pw=3).astype(np.int64)
    zone[0, 3, 8:12] = (1 << 32) + 1                                     # the low 32 bits are a valid zone
    zone[0, 5, 0] = (1 << 31) + 2
    zone[0, 7, 255] = (1 << 62)
    hist = run_hist(zone, cls, Z, 4, want_status=R.BAD_ZONE, zdtype=torch.int64)
    assert hist.sum() == int((cls[zone < Z] < 4).sum())
    run_bands(zone, vals, Z, want_status=R.BAD_ZONE, zdtype=torch.int64)
    run_paint(zone, np.arange(Z), torch.uint8, want_status=R.BAD_ZONE, zdtype=torch.int64)


# ---- ids per map -----------------------------------------------------------------------------------------------------------------------------------
def test_per_map_ids_land_in_their_own_rows():
    M, (H, W), Zm, K = 3, (BH + 1, BW + 1), 23, 4
    rng, cls, vals = rasters(4, M, H, W)
    one = R.patches(1, H, W, rng.integers(-1, Zm, 300), ph=3, pw=4)
    zone = np.repeat(one, M, 0)                                          # the same ids in every map
    hist = run_hist(zone, cls, M * Zm, K, stride=Zm)
    assert all(hist[m * Zm:(m + 1) * Zm].sum() == int((cls[m][one[0] >= 0] < K).sum()) for m in range(M))
    want_b = run_bands(zone, vals, M * Zm, stride=Zm, nodata=0)
    table = rng.integers(-1, 200, M * Zm)
    want_p = run_paint(zone, table, torch.int32, fill=7, stride=Zm)
    zone[2, 1, 1] = Zm                                                   # map 2 has no zone Zm: not map 3's zone 0
    run_hist(zone, cls, M * Zm, K, stride=Zm, want_status=R.BAD_ZONE)
    zone[2, 1, 1] = one[0, 1, 1]
    z = dev(zone)
    got = zonal.histogram(z, dev(cls), Zm, K, per_map=True)
    assert got.shape == (M, Zm, K) and torch.equal(got.cpu().view(-1, K), torch.from_numpy(hist))
    st = zonal.band_stats(z, dev(vals), Zm, nodata=0, per_map=True)
    assert st.count.shape == (M, Zm, 6) and torch.equal(st.max.cpu().view(-1, 6), torch.from_numpy(want_b[4]))
    assert torch.equal(st.sumsq.cpu().view(-1, 6), torch.from_numpy(want_b[2] - CANARY))
    cls_z = zonal.majority(got)
    assert cls_z.shape == (M, Zm) and torch.equal(cls_z.cpu().view(-1), torch.from_numpy(R.majority(hist, 0xf)[0]))
    painted = zonal.paint(z, dev(table, torch.int32).view(M, Zm), fill=7, dtype=torch.int32, per_map=True)
    assert torch.equal(painted.cpu(), torch.from_numpy(want_p))


# ---- histogram classes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 32])
@pytest.mark.parametrize("kind", ["u8", "u8_lut", "i64"])
def test_histogram_classes(K, kind):
    M, (H, W), Z = 2, (BH + 1, BW + 4), 50
    rng = np.random.default_rng(K)
    zone = R.patches(M, H, W, rng.integers(-1, Z, 700), ph=5, pw=3)
    lut = None
    if kind == "i64":
        cls = rng.integers(-2, K + 3, (M, H, W)).astype(np.int64)
        cls[0, 0, :4] = [1 << 32, -(1 << 40), (1 << 63) - 1, K]          # all outside [0, K)
    else:
        cls = rng.integers(0, 256, (M, H, W)).astype(np.uint8)
        if kind == "u8_lut":
            lut = rng.integers(-3, K + 3, 256).astype(np.int32)
            lut[:4] = [-(1 << 31), (1 << 31) - 1, 0, K]
        else:
            cls = (cls % (K + 2)).astype(np.uint8)
    hist = run_hist(zone, cls, Z, K, lut=lut)
    if lut is not None:
        got = zonal.histogram(dev(zone), dev(cls), Z, K, lut=dev(lut))
        assert torch.equal(got.cpu(), torch.from_numpy(hist))


# ---- band values -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 6, 13, 16])
def test_band_counts(C):
    M, (H, W), Z = 2, (BH + 1, BW + 4), 40
    rng, _, vals = rasters(C, M, H, W, C=C, lo=-32768, hi=32768)
    zone = R.patches(M, H, W, rng.integers(-1, Z, 700), ph=4, pw=6)
    run_bands(zone, vals, Z, nodata=0)
    run_bands(zone, vals, Z)


def test_extreme_band_values_carry_in_the_sum_of_squares():
    H, W = 2 * BH, 2 * BW
    vals = np.full((1, 2, H, W), -32768, np.int16)
    vals[0, 1] = 32767
    zone = np.zeros((1, H, W), np.int32)
    zone[0, :, W // 2:] = 1
    want = run_bands(zone, vals, 2)
    assert (want[2][0, 0] - CANARY) == (H * W // 2) << 30 > 1 << 32 and want[3][0, 0] == -32768 and want[4][1, 1] == 32767


def test_nodata_in_one_band_and_a_zone_of_nothing_but_nodata():
    H, W, Z = BH + 1, BW + 1, 6
    rng, _, vals = rasters(9, 1, H, W, C=3)
    vals[vals == -7] = 0
    zone = R.patches(1, H, W, np.arange(Z), ph=6, pw=50)
    vals[0, 1][zone[0] == 2] = -7                                        # band 1 of zone 2 is nothing but nodata
    vals[0, :, 0, 0] = [5, -7, 5]                                        # one pixel: nodata in band 1 only
    vals[0][:, zone[0] == 4] = -7                                        # zone 4: nodata in every band
    want = run_bands(zone, vals, Z, nodata=-7)
    n = want[0] - CANARY
    assert n[2].tolist()[1] == 0 and n[2, 0] > 0 and not n[4].any() and n[0, 1] == n[0, 0] - 1
    assert (want[3][4] == R.INT32_MAX).all() and (want[4][4] == R.INT32_MIN).all() and want[3][2, 1] == R.INT32_MAX
    st = zonal.band_stats(dev(zone), dev(vals), Z, nodata=-7)
    assert bool(st.mean()[4].isnan().all()) and bool(st.std()[2, 1].isnan()) and not bool(st.mean()[0].isnan().any())


# ---- majority and paint ----------------------------------------------------------------------------------------------------------------------------
def test_majority_ties_min_count_and_votes_on_the_device():
    hist = np.array([[0, 2, 0, 1], [1, 0, 2, 0], [0, 2, 2, 0], [0, 0, 0, 0], [3, 3, 3, 3], [1 << 40, 5, 1 << 40, 0]], dtype=np.int64)
    rng = np.random.default_rng(0)
    big = np.concatenate([hist, rng.integers(0, 3, (700, 4))])           # more than one workgroup of zones, many ties
    for votes, min_count, fill in ((0xf, 1, -1), (0b1100, 2, 7), (0xf, 3, -1), (0b0010, 1, -(1 << 31)), (0b1001, 1 << 41, 255)):
        want_cls, want_best = R.majority(big, votes, min_count, fill)
        h = dev(big)
        for _ in range(2):
            cls = torch.full((len(big),), 77, dtype=torch.int32, device=DEV)
            best = torch.full((len(big),), 77, dtype=torch.int64, device=DEV)
            _lib.check(_lib.zonal_majority(h, big.shape, votes, min_count, fill, cls, best, stream()))
            assert torch.equal(cls.cpu(), torch.from_numpy(want_cls)) and torch.equal(best.cpu(), torch.from_numpy(want_best))
        _lib.check(_lib.zonal_majority(h, big.shape, votes, min_count, fill, cls, None, stream()))
        assert torch.equal(cls.cpu(), torch.from_numpy(want_cls))
    got = zonal.majority(dev(hist), votes=(2, 3), min_count=2, fill=7)
    assert got.tolist() == [7, 2, 2, 7, 2, 2]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64], ids=["u8", "i32", "i64"])
@pytest.mark.parametrize("mode", [0, 1], ids=["fill", "keep"])
def test_paint_widths_and_modes(dtype, mode):
    M, (H, W), Z = 2, SIZES[-1], 90
    rng = np.random.default_rng(6)
    zone = R.patches(M, H, W, rng.integers(-1, Z, 900), ph=3, pw=11)
    table = rng.integers(0, 256 if dtype == torch.uint8 else 1 << 30, Z)
    table[::7] = -1
    table[1] = -(1 << 31)
    want = run_paint(zone, table, dtype, mode=mode, fill=200)
    untouched = (zone < 0) | (table[np.maximum(zone, 0)] < 0)
    assert untouched.any() and (want[untouched] == (NP[dtype](PIX[dtype]) if mode else 200)).all()
    if mode:
        out = torch.full((M, H, W), PIX[dtype], dtype=dtype, device=DEV)
        assert zonal.paint(dev(zone), dev(table, torch.int32), out=out) is out and torch.equal(out.cpu(), torch.from_numpy(want))
    else:
        assert torch.equal(zonal.paint(dev(zone), dev(table, torch.int32), fill=200, dtype=dtype).cpu(), torch.from_numpy(want))


# ---- end to end, small ------------------------------------------------------------------------------------------------------------------------------
def test_rasterised_polygons_vote_and_are_painted():
    M, H, W, K = 2, 40, 300, 4
    shapes, _ = RR.stars(3, 12, H, W)
    origins = [(0, 0), (7, -5)]
    ps = classmap.PolygonSet(shapes, None, device=DEV)
    zones = classmap.rasterize(ps, origins, (H, W), fill=-1, dtype=torch.int32, burn="index")
    want_zone, _ = RR.rasterize_shapes(shapes, None, origins, H, W, fill=-1, burn_index=True)
    assert torch.equal(zones.cpu(), torch.from_numpy(want_zone).to(torch.int32))
    cls = np.random.default_rng(8).integers(0, K, (M, H, W)).astype(np.uint8)
    hist, _ = R.histogram(want_zone, cls, len(shapes), K)
    cls_z, _ = R.majority(hist, 0b1110, 5)
    got_hist = zonal.histogram(zones, dev(cls), len(shapes), K)
    got_cls = zonal.majority(got_hist, votes=(1, 2, 3), min_count=5)
    assert torch.equal(got_hist.cpu(), torch.from_numpy(hist)) and torch.equal(got_cls.cpu(), torch.from_numpy(cls_z))
    assert torch.equal(zonal.paint(zones, got_cls, fill=0).cpu(), torch.from_numpy(R.paint(want_zone, cls_z, np.uint8)[0]))
    want_clean, _ = R.paint(want_zone, cls_z, np.uint8, mode=1, base=cls)
    assert torch.equal(zonal.majority_by_zone(dev(cls), zones, len(shapes), K, votes=(1, 2, 3), min_count=5).cpu(), torch.from_numpy(want_clean))


def test_component_labels_as_per_map_zones_give_the_component_areas():
    M, H, W, K = 3, 24, 40, 3
    rng = np.random.default_rng(12)
    cls = dev(np.repeat(np.repeat(rng.integers(0, K + 1, (M, 6, 8)), 4, 1), 5, 2).astype(np.uint8))      # blobs; class K is unlabelled
    labels, areas = classmap.connected_components(cls, K, return_areas=True)
    hist = zonal.histogram(labels, cls, H * W, K, per_map=True)
    assert hist.shape == (M, H * W, K) and torch.equal(hist.sum(2), areas.view(M, H * W).long())
    assert int(hist.sum()) == int((cls < K).sum()) and int((hist > 0).sum(2).max()) == 1      # a component has one class


N_TILES, BANDS, TH, TW = 3, 4, 96, 128


@functools.lru_cache(maxsize=None)
def _pipe():
    g = torch.Generator().manual_seed(7)
    raw = torch.randint(-500, 9000, (N_TILES, BANDS, TH, TW), generator=g, dtype=torch.int32).to(torch.int16)
    labels = torch.randint(0, 24, (N_TILES, TH, TW), generator=g, dtype=torch.int32).to(torch.uint8)
    pipe = GpuTilePipeline([0.05, 0.06, 0.07, 0.08], [0.02, 0.03, 0.025, 0.035], random_crop_size=32, label_map="cnes-multiclass",
                           squeeze_time_dim=True, device=DEV)
    pipe.load(raw, labels)
    return pipe


def test_the_pipeline_and_the_predictor_against_the_same_expectation():
    pipe, idx, Z, K = _pipe(), [2, 0, 2], 31, 4
    zone = R.patches(len(idx), TH, TW, np.random.default_rng(2).integers(-1, Z, 600), ph=7, pw=9)
    z = dev(zone)
    labels, raw = pipe.labels.cpu().numpy()[idx], pipe.raw.cpu().numpy()[idx]
    want, _ = R.histogram(zone, labels, Z, K, src_lut=pipe.lut.cpu().numpy())
    assert pipe.label_classes == K and torch.equal(pipe.zonal_label_histogram(z, Z, idx).cpu(), torch.from_numpy(want))
    want_b, _ = R.bands(zone, raw, Z, nodata=100)
    st = pipe.zonal_band_stats(z, Z, idx, nodata=100)
    for got, w in zip((st.count, st.sum, st.sumsq, st.min, st.max), want_b):
        assert torch.equal(got.cpu(), torch.from_numpy(w))
    w = torch.randn(K, BANDS, generator=torch.Generator().manual_seed(3)).to(DEV)
    model = lambda x: sum(x[:, c:c + 1] * w[:, c].view(1, -1, 1, 1) for c in range(BANDS)).contiguous()      # noqa: E731  elementwise, fixed order
    pred = P.TilePredictor(model, pipe, K, windows_per_batch=16)
    mask = pred.predict(idx, majority=3)
    hist, _ = R.histogram(zone, mask.cpu().numpy(), Z, K)
    cls_z, _ = R.majority(hist, 0b0111, 30)
    got_cls, got_hist, painted = pred.predict_zones(z, Z, idx, votes=(0, 1, 2), min_count=30, paint=True, majority=3)
    assert torch.equal(got_hist.cpu(), torch.from_numpy(hist)) and torch.equal(got_cls.cpu(), torch.from_numpy(cls_z))
    want_p, _ = R.paint(zone, cls_z, np.int64, mode=1, base=mask.cpu().numpy())
    assert painted.dtype == torch.int64 and torch.equal(painted.cpu(), torch.from_numpy(want_p))
    assert len(pred.predict_zones(z, Z, idx)) == 2
