"""GPU: the quicklook stages TILE_RADIX_HIST, TILE_RANK_PICK, TILE_QUICKLOOK and CLASS_OVERLAY (csrc/quicklook.hip) as one- and
four-record programs through the C ABI against their numpy restatement (tests/quicklook_ref.py; the ops have no entry in
oracle/ops_ref.py), and the Python surface (`GpuTilePipeline.band_percentiles` / `.zero_fraction` / `.quicklook`, `render.overlay`,
`TilePredictor.render`) end to end.

Bars: none.  Every stage is integer or separately rounded float64 arithmetic in a fixed order, so every comparison is for EXACT
equality - histograms, ranks, order statistics, the float64 percentiles (`==` against `np.percentile`), the uint8 pictures - and two
runs are bit-identical."""
import functools

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import render
from s2lc_amd.data import quicklook as QL
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.predict import TilePredictor
from tests import quicklook_ref as R
from tests.test_dataset_stats_gpu import run_records
from tests.test_ops_gpu import Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# H x W: N = 1; fewer values than a wave; 880-byte planes; several waves (and, pooled, several workgroups per group); 70-byte planes -
# every plane starts at another offset from a 16-byte boundary; 34,060-byte planes - two chunks per plane, the second 646 values
SHAPES = [(1, 1), (8, 8), (20, 22), (64, 72), (5, 7), (130, 131)]
# name: (NSRC, INDEX, POOLED) - permuted, with duplicates, NSRC > M and M > NSRC; 40 pooled tiles: the slices of a group add atomically
LAYOUTS = {
    "tile_m3_of5": (5, [3, 0, 3], 0),
    "tile_m7_of3": (3, [2, 0, 1, 1, 0, 2, 2], 0),
    "pooled_m3_of5": (5, [4, 1, 4], 1),
    "pooled_m40_of5": (5, [(7 * i + 3) % 5 for i in range(40)], 1),
}
BANDS = [(4, (2, 1, 0)), (13, (11, 3, 7)), (4, (1,))]          # (C, BANDS): the quicklook's order, a non-monotone pick of 13, one band
DATA = ["uniform", "sentinel", "constant", "ties"]
Q_SETS = [(2.0, 98.0, 0.0, 100.0), (50.0, 99.9)]               # eight ranks, then four


@functools.lru_cache(maxsize=None)
def tiles(kind, nsrc, C, H, W):
    rng = np.random.default_rng(1000 * H + 10 * W + C + nsrc)
    shape = (nsrc, C, H, W)
    if kind == "uniform":                  # the whole int16 range, both ends present
        raw = rng.integers(-32768, 32768, shape)
        raw.reshape(-1)[0], raw.reshape(-1)[-1] = -32768, 32767
    elif kind == "sentinel":               # 30 % nodata zeros, reflectances in 1..4000: twenty high bytes, one of them hot
        raw = np.where(rng.random(shape) < 0.3, 0, rng.integers(1, 4001, shape))
    elif kind == "constant":
        raw = np.full(shape, 1234)
    else:                                  # long runs of ties in two coarse bins: ranks land inside a run and between the runs
        raw = rng.choice(np.array([100, 1000, 1001]), size=shape, p=[0.5, 0.3, 0.2])
    return torch.from_numpy(raw.astype(np.int16))


def selection(raw, index, bands, pooled, ranks, frac, repeat=1):
    """the four-record program; every intermediate and result tensor as numpy"""
    nsrc, C, H, W = raw.shape
    M, nb, Rn = len(index), len(bands), len(ranks)
    G, N = (nb, M * H * W) if pooled else (M, nb * H * W)
    c = Case(0)
    t_raw = c.t("raw", raw.shape, raw, "i16")
    t_index, t_bands = c.t("index", (M,), torch.tensor(index), "i32"), c.t("bands", (nb,), torch.tensor(bands), "i32")
    t_ranks = c.t("ranks", (Rn,), torch.tensor(ranks), "i64")
    t_frac = c.t("frac", (Rn // 2,), torch.tensor(frac, dtype=torch.float64), "f64") if Rn >= 2 else None
    h0, h1 = c.t("h0", (G, 256), "zeros", "i64"), c.t("h1", (G, Rn, 256), "zeros", "i64")
    bucket, rest = c.t("bucket", (G, Rn), torch.full((G, Rn), -7), "i32"), c.t("rest", (G, Rn), torch.full((G, Rn), -7), "i64")
    values = c.t("values", (G, Rn), torch.full((G, Rn), -7), "i32")
    pct = c.t("pct", (G, Rn // 2), "nan", "f64") if Rn >= 2 else None
    dims = dict(M=M, C=C, H=H, W=W, NSRC=nsrc, NBND=nb, POOLED=pooled, R=Rn)
    recs = [("TILE_RADIX_HIST", dict(RAW=t_raw, INDEX=t_index, BANDS=t_bands, BUCKET=None, HIST=h0, PASS=0, **dims)),
            ("TILE_RANK_PICK", dict(HIST=h0, RANKS=t_ranks, BUCKET=bucket, REST=rest, N=N, G=G, R=Rn, STEP=0)),
            ("TILE_RADIX_HIST", dict(RAW=t_raw, INDEX=t_index, BANDS=t_bands, BUCKET=bucket, HIST=h1, PASS=1, **dims)),
            ("TILE_RANK_PICK", dict(HIST=h1, RANKS=t_ranks, BUCKET=bucket, REST=rest, VALUES=values, FRAC=t_frac, PCT=pct, N=N, G=G,
                                    R=Rn, STEP=1))]
    img = run_records(c, recs * repeat)
    return {k: c.read(img, k).numpy().copy() for k in ("h0", "h1", "bucket", "rest", "values") + (("pct",) if pct is not None else ())}


CASES = [(s, lay, d, BANDS[(i + j + k) % 3]) for i, s in enumerate(SHAPES) for j, lay in enumerate(LAYOUTS) for k, d in enumerate(DATA)]


@pytest.mark.parametrize("shape,layout,data,bandset", CASES, ids=[f"{s[0]}x{s[1]}-{lay}-{d}-c{b[0]}n{len(b[1])}" for s, lay, d, b in CASES])
def test_selection_program_is_sort_and_percentile_exactly(shape, layout, data, bandset):
    (H, W), (nsrc, index, pooled), (C, bands) = shape, LAYOUTS[layout], bandset
    raw = tiles(data, nsrc, C, H, W)
    grp = R.groups(raw.numpy(), index, bands, pooled)
    N = grp.shape[1]
    for qs in Q_SETS:
        ranks, frac = QL.rank_plan(qs, N)
        got = selection(raw, index, bands, pooled, ranks, frac)
        want_h0 = R.coarse_hist(grp)
        want_bucket, want_rest = R.pick0(want_h0, ranks)
        assert np.array_equal(got["h0"], want_h0) and got["h0"].sum() == grp.size
        assert np.array_equal(got["bucket"], want_bucket) and np.array_equal(got["rest"], want_rest)
        assert np.array_equal(got["h1"], R.fine_hist(grp, want_bucket))
        assert np.array_equal(got["values"], R.order_statistics(grp, ranks))
        want_pct = R.percentiles(grp, qs)
        assert got["pct"].dtype == np.float64 and np.array_equal(got["pct"].view(np.int64), want_pct.view(np.int64)), (got["pct"], want_pct)
        again = selection(raw, index, bands, pooled, ranks, frac)
        assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def test_rank_pairs_inside_one_coarse_bucket_and_across_two():
    """ties data, one band of 64 x 72, per tile: the median pair straddles the runs of 100 (coarse bin 128) and 1000 (131) or sits
    inside one of them depending on the tile; the pair of q = 10 always lies inside the run of 100"""
    raw = tiles("ties", 5, 4, 64, 72)
    index, bands = [0, 1, 2, 3, 4], (1,)
    grp = R.groups(raw.numpy(), index, bands, 0)
    N = grp.shape[1]
    n100 = int((grp[0] == 100).sum())
    ranks = [n100 - 1, n100, 10, 11, N - 2, N - 1]           # across the two runs of tile 0; inside the first run; inside the last
    got = selection(raw, index, bands, 0, ranks, [0.5, 0.25, 0.75])
    assert got["bucket"][0].tolist() == [128, 131, 128, 128, 131, 131] and got["values"][0].tolist() == [100, 1000, 100, 100, 1001, 1001]
    assert got["pct"][0].tolist() == [550.0, 100.0, 1001.0]
    assert np.array_equal(got["values"], R.order_statistics(grp, ranks))


@pytest.mark.parametrize("pooled", [0, 1])
def test_both_passes_equal_bincount_and_accumulate(pooled):
    raw = tiles("sentinel", 5, 13, 64, 72)
    nsrc, index, _ = LAYOUTS["pooled_m40_of5" if pooled else "tile_m7_of3"]
    bands = (11, 3, 7)
    grp = R.groups(raw.numpy(), index, bands, pooled)
    G, M = len(grp), len(index)
    preset = np.stack([[128, 128 + (g % 5), 135, 7] for g in range(G)]).astype(np.int32)      # a repeated, a hot and an empty coarse bin
    c = Case(0)
    dims = dict(RAW=c.t("raw", raw.shape, raw, "i16"), INDEX=c.t("index", (M,), torch.tensor(index), "i32"),
                BANDS=c.t("bands", (3,), torch.tensor(bands), "i32"), M=M, C=13, H=64, W=72, NSRC=nsrc, NBND=3, POOLED=pooled, R=4)
    h0, h1 = c.t("h0", (G, 256), "zeros", "i64"), c.t("h1", (G, 4, 256), "zeros", "i64")
    bucket = c.t("bucket", (G, 4), torch.from_numpy(preset), "i32")
    recs = [("TILE_RADIX_HIST", dict(BUCKET=None, HIST=h0, PASS=0, **dims)), ("TILE_RADIX_HIST", dict(BUCKET=bucket, HIST=h1, PASS=1, **dims))]
    once, twice = run_records(c, recs), run_records(c, recs * 2)
    want0, want1 = R.coarse_hist(grp), R.fine_hist(grp, preset)
    assert want1[:, 0].sum() > 0 and not want1[:, 3].any() and np.array_equal(want1[0, 0], want1[0, 1])
    assert np.array_equal(c.read(once, "h0").numpy(), want0) and np.array_equal(c.read(once, "h1").numpy(), want1)
    assert np.array_equal(c.read(twice, "h0").numpy(), 2 * want0) and np.array_equal(c.read(twice, "h1").numpy(), 2 * want1)


# ---- TILE_QUICKLOOK -----------------------------------------------------------------------------------------------------------------
PCT_ROWS = [(100.5, 3000.25), (-5000.0, -100.0), (7.0, 7.0), (float("nan"), 5.0), (0.0, float("inf")), (9.0, 8.0)]


@pytest.mark.parametrize("SH,SW", [(4, 4), (5, 6), (7, 23), (16, 16), (24, 29)], ids=lambda v: str(v))
def test_quicklook_stretch_is_numpy_bit_for_bit(SH, SW):
    """all four flip codes at the offsets 0 and H - SH / W - SW (odd W = 29: source rows at every alignment), widths 4, 6, 23, the whole
    tile; negative values, values beyond both bounds; bounds without a range (equal, reversed, NaN, infinite) give zeros"""
    nsrc, C, H, W, bands = 3, 5, 24, 29, (4, 0, 2)
    raw = tiles("uniform", nsrc, C, H, W).clone()
    raw[1] = tiles("sentinel", nsrc, C, H, W)[1]
    par = [[(b + f) % nsrc, y0, x0, f] for f in range(4) for b, (y0, x0) in enumerate([(0, 0), (H - SH, W - SW), ((H - SH) // 2, (W - SW + 1) // 2)])]
    par += [[2, 0, 0, 1]] * (len(PCT_ROWS) - 2)
    slot = [i % 2 for i in range(12)] + list(range(2, len(PCT_ROWS)))
    B = len(par)
    c = Case(0)
    fields = dict(RAW=c.t("raw", raw.shape, raw, "i16"), PARAMS=c.t("par", (B, 4), torch.tensor(par), "i32"),
                  SLOT=c.t("slot", (B,), torch.tensor(slot), "i32"), BANDS=c.t("bands", (3,), torch.tensor(bands), "i32"),
                  PCT=c.t("pct", (len(PCT_ROWS), 3), torch.tensor([list(r) + [0.0] for r in PCT_ROWS], dtype=torch.float64), "f64"),
                  OUT=c.t("out", (B, SH, SW, 3), torch.full((B, SH, SW, 3), 77), "u8"),
                  B=B, C=C, H=H, W=W, SH=SH, SW=SW, NSRC=nsrc, NROW=len(PCT_ROWS), NQ=3)
    got = c.read(run_records(c, [("TILE_QUICKLOOK", fields)]), "out").numpy()
    want = np.stack([R.stretch(R.crop(raw.numpy(), p, bands, SH, SW), *PCT_ROWS[s]) for p, s in zip(par, slot)])
    assert want[:12].min() == 0 and want[:12].max() == 255 and len(np.unique(want[:12])) > 2        # both clips and the range between
    assert not want[12:].any()
    assert np.array_equal(got, want)


# ---- CLASS_OVERLAY ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("with_base", [True, False], ids=["base", "black"])
@pytest.mark.parametrize("K", [1, 4, 256])
@pytest.mark.parametrize("alpha", [0, 128, 256, 77])
def test_overlay_is_the_integer_blend(alpha, K, with_base, misaligned):
    B, SH, SW = 2, 5, 7                      # 70 pixels: a last thread with two
    g = torch.Generator().manual_seed(K + alpha)
    cls = torch.randint(-1, K + 1, (B, SH, SW), generator=g)             # -1 and K: no colour
    cls[0, 0, :4] = torch.tensor([-1, K, 0, K - 1])
    cls[1, 4, 6] = -(1 << 40)
    pal = torch.randint(0, 256, (K, 3), generator=g).to(torch.uint8)
    base = torch.randint(0, 256, (B, SH, SW, 3), generator=g).to(torch.uint8)
    n = B * SH * SW * 3
    off = 1 if misaligned else 0             # BASE and OUT one byte off a dword boundary: the element path
    for skip0 in (0, 1):
        c = Case(0)
        t_base = c.t("base", (n + 8,), torch.cat([torch.zeros(off), base.reshape(-1).float(), torch.zeros(8 - off)]), "u8")
        t_out = c.t("out", (n + 8,), torch.full((n + 8,), 99), "u8")
        fields = dict(CLS=c.t("cls", (B, SH, SW), cls, "i64"), PALETTE=c.t("pal", (K, 3), pal, "u8"),
                      BASE=t_base.at(off, (B, SH, SW, 3)) if with_base else None, OUT=t_out.at(off, (B, SH, SW, 3)),
                      B=B, SH=SH, SW=SW, K=K, ALPHA=alpha, SKIP0=skip0)
        flat = c.read(run_records(c, [("CLASS_OVERLAY", fields)]), "out").numpy()
        want = R.overlay(base.numpy() if with_base else None, cls.numpy(), pal.numpy(), alpha, skip0)
        assert np.array_equal(flat[off:off + n].reshape(B, SH, SW, 3), want)
        assert (flat[:off] == 99).all() and (flat[off + n:] == 99).all()          # nothing written around OUT
        if alpha == 0 and with_base:
            assert np.array_equal(want, base.numpy())
        if alpha == 256 and K > 1:
            assert np.array_equal(want[0, 0, 3], pal[K - 1].numpy())


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def surface_tiles():
    rng = np.random.default_rng(5)
    raw = np.where(rng.random((3, 6, 32, 40)) < 0.3, 0, rng.integers(1, 4001, (3, 6, 32, 40))).astype(np.int16)
    raw[1, :, :10] = 0                       # a nodata strip
    raw[2, 4] = 0                            # a band without data
    labels = rng.integers(0, 24, (3, 32, 40)).astype(np.uint8)
    return torch.from_numpy(raw), torch.from_numpy(labels)


def _pipe(S=16):
    pipe = GpuTilePipeline([0.05] * 6, [0.02] * 6, random_crop_size=S, label_map="cnes-multiclass", squeeze_time_dim=True, device=DEV)
    pipe.load(*surface_tiles())
    return pipe


def test_band_percentiles_and_zero_fraction_match_numpy():
    pipe, raw = _pipe(), surface_tiles()[0].numpy()
    q = [0.5, 2, 50, 98, 99.9]               # five: two selection programs
    got = pipe.band_percentiles(q)
    assert got.dtype == torch.float64 and not got.is_cuda and got.shape == (6, 5)
    assert np.array_equal(got.numpy(), R.percentiles(R.groups(raw, [0, 1, 2], range(6), True), q))
    idx, bands = [2, 0, 2, 1], (4, 1, 0)
    got = pipe.band_percentiles(q, indices=idx, bands=bands, pooled=True)
    assert np.array_equal(got.numpy(), R.percentiles(R.groups(raw, idx, bands, True), q))
    got = pipe.band_percentiles(q, indices=idx, bands=bands, pooled=False)
    assert got.shape == (4, 5) and np.array_equal(got.numpy(), R.percentiles(R.groups(raw, idx, bands, False), q))
    assert np.array_equal(pipe.band_percentiles(50.0, bands=[3]).numpy(), R.percentiles(R.groups(raw, [0, 1, 2], [3], True), [50.0]))
    for band in (0, 4):
        zf = pipe.zero_fraction(idx, band=band)
        assert zf.dtype == torch.float64 and np.array_equal(zf.numpy(), (raw[idx][:, band] == 0).reshape(4, -1).sum(1) / float(32 * 40))
    assert pipe.zero_fraction(band=4)[2] == 1.0


def test_quicklook_matches_the_reference_lines():
    pipe, raw = _pipe(), surface_tiles()[0].numpy()
    got = pipe.quicklook()
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (3, 16, 16, 3)
    centre = [[i, 8, 12, 0] for i in range(3)]
    assert np.array_equal(got.cpu().numpy(), R.quicklook(raw, centre, (2, 1, 0), 98.0, 16, 16))
    par = pipe.draw_params([2, 0, 2, 1, 1], training=False)
    par[:, 1], par[:, 2], par[:, 3] = torch.tensor([0, 16, 3, 9, 16]), torch.tensor([24, 0, 5, 11, 24]), torch.tensor([0, 1, 2, 3, 1])
    got = pipe.quicklook(params=par, bands=(5, 3, 0), percentile=99.5)
    want = R.quicklook(raw, par.numpy(), (5, 3, 0), 99.5, 16, 16)
    assert np.array_equal(got.cpu().numpy(), want) and want.max() == 255
    x = pipe(params=par).x                    # the picture is the crop the model saw: same window, same flips
    assert x.shape[-2:] == got.shape[1:3]
    whole = pipe.quicklook([1, 2], whole_tile=True)
    assert whole.shape == (2, 32, 40, 3)
    assert np.array_equal(whole.cpu().numpy(), R.quicklook(raw, [[1, 0, 0, 0], [2, 0, 0, 0]], (2, 1, 0), 98.0, 32, 40))
    # a band without data beside two with 30 % nodata: more than half of the pixels are 0, both bounds are 0 - a black picture
    dark = pipe.quicklook([2], bands=(4, 1, 0), percentile=51.0, whole_tile=True)
    assert np.percentile(raw[2][[4, 1, 0]].astype(np.float64), (49.0, 51.0)).tolist() == [0.0, 0.0] and not dark.any()


class Pointwise:
    """a fixed per-pixel 1 x 1 projection (the stub model of tests/test_predict_gpu.py)"""

    def __init__(self, K, C, seed=3):
        g = torch.Generator().manual_seed(seed)
        self.w = (torch.randn(K, C, generator=g) * 2).to(DEV)
        self.b = torch.randn(K, generator=g).to(DEV)

    def __call__(self, x):
        out = self.b.view(1, -1, 1, 1).expand(x.shape[0], -1, x.shape[2], x.shape[3])
        for c in range(x.shape[1]):
            out = out + x[:, c:c + 1] * self.w[:, c].view(1, -1, 1, 1)
        return out.contiguous()


def test_overlay_and_predictor_render():
    pipe, raw = _pipe(), surface_tiles()[0].numpy()
    K = 4
    pal = torch.tensor([[0, 0, 0], [250, 200, 10], [20, 160, 40], [200, 30, 30], [1, 2, 3]], dtype=torch.uint8)
    pred = TilePredictor(Pointwise(K, 6), pipe, K)
    idx = [2, 0]
    got = pred.render(idx, pal, alpha=0.25)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (2, 32, 40, 3)
    cls = pred.predict(idx)
    assert len(torch.unique(cls)) > 1
    picture = R.quicklook(raw, [[2, 0, 0, 0], [0, 0, 0, 0]], (2, 1, 0), 98.0, 32, 40)
    assert np.array_equal(got.cpu().numpy(), R.overlay(picture, cls.cpu().numpy(), pal.numpy(), 64, 0))
    # the pipeline's own label maps over the crop the model saw, the "other" class left transparent
    par = pipe.draw_params([1, 2], training=False)
    y = pipe(params=par).y
    shown = render.overlay(pipe.quicklook(params=par), y, pal[:4], alpha=0.5, skip_zero=True)
    want = R.overlay(R.quicklook(raw, par.numpy(), (2, 1, 0), 98.0, 16, 16), y.cpu().numpy(), pal[:4].numpy(), 128, 1)
    assert np.array_equal(shown.cpu().numpy(), want)
    assert np.array_equal(render.overlay(None, y, pal.numpy(), alpha=1.0).cpu().numpy(), pal.numpy()[y.cpu().numpy()])
