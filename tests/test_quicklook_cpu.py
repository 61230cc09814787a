"""CPU: the quicklook stage kinds are registered (and no earlier kind moved), their launchers check everything on the host before any
HIP call, the host's rank / fraction derivation plus the device's interpolation formula (restated in data/quicklook.py) is
`np.percentile` bit for bit, and the new methods validate their arguments before they refuse to run off the GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import render
from s2lc_amd.data import quicklook as QL
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.plan import opdefs as D
from s2lc_amd.predict import TilePredictor
from tests import quicklook_ref as R

ROOT = Path(__file__).resolve().parents[1]
# the stage kinds as they were numbered before the four quicklook kinds were appended
KINDS_BEFORE = ["MEMSET", "AXPY", "WEIGHT_PACK", "CONV", "WGRAD", "WGRAD_FINALIZE", "DWCONV_FWD", "DWCONV_DGRAD", "DWCONV_WGRAD",
                "BN_FINALIZE", "SE_POOL", "SE_FC", "SE_FC_BWD", "SE_BWD_REDUCE", "BN_BWD_REDUCE", "BN_BWD_FINALIZE", "BN_BWD_APPLY",
                "BN_RESIDUAL", "CHANNEL_SUM", "LOSS_FWD", "LOSS_BWD", "ARGMAX", "CHAN_LN_FWD", "CHAN_LN_BWD", "ACT_BWD", "ACT_FWD",
                "ATTN_FWD", "ATTN_BWD", "MAE_MASK_INDEX", "IDS_TO_DEC_IDX", "TOKEN_GATHER", "TOKEN_SCATTER", "PATCHIFY", "MAE_LOSS_FWD",
                "MAE_LOSS_BWD", "TRANSPOSE_CL", "CONFUSION", "DROP_GATE", "TILE_PREP", "SE_BN_SUMS", "SE_BN_COMBINE", "SPACE_TO_DEPTH",
                "UPSAMPLE_ZERO", "SE_FC_WGRAD", "IM2COL", "TILE_LABEL_HIST", "TILE_MOMENTS", "WINDOW_BLEND", "SEG_STATS", "SEG_HIST",
                "GRAD_CLIP"]
NEW = ["TILE_RADIX_HIST", "TILE_RANK_PICK", "TILE_QUICKLOOK", "CLASS_OVERLAY"]


def test_new_kinds_are_appended_and_named_by_the_library():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g
    from s2lc_amd import _lib

    g.build()
    assert len(KINDS_BEFORE) == 51 and [D.KIND[k] for k in KINDS_BEFORE] == list(range(1, 52))
    assert [D.KIND[k] for k in NEW] == [52, 53, 54, 55] and len(D.OPS) == 55
    L = _lib.lib()
    assert L.s2k_abi_version() == 2
    for name in NEW:
        assert L.s2k_kind_name(D.KIND[name]).decode() == name
        assert name in D.WRITES
    assert "quicklook.hip" in g.SOURCES


def _records():
    """one valid record per new kind over a 64 KiB CPU workspace (never launched: every case below fails a host check first)"""
    from s2lc_amd.plan.program import TRef

    t = lambda off, shape, dt: TRef(D.BASE["WS"], off, shape, dt)      # noqa: E731
    raw = t(0, (2, 3, 8, 8), "i16")
    hist = dict(RAW=raw, INDEX=t(1024, (2,), "i32"), BANDS=t(1280, (3,), "i32"), BUCKET=t(1536, (2, 4), "i32"), HIST=t(2048, (2, 4, 256), "i64"),
                M=2, C=3, H=8, W=8, NSRC=2, NBND=3, POOLED=0, PASS=1, R=4)
    pick = dict(HIST=t(2048, (2, 4, 256), "i64"), RANKS=t(20480, (4,), "i64"), BUCKET=t(1536, (2, 4), "i32"), REST=t(20736, (2, 4), "i64"),
                VALUES=t(20992, (2, 4), "i32"), FRAC=t(21248, (2,), "f64"), PCT=t(21504, (2, 2), "f64"), N=192, G=2, R=4, STEP=1)
    look = dict(RAW=raw, PARAMS=t(22016, (2, 4), "i32"), SLOT=t(22272, (2,), "i32"), BANDS=t(1280, (3,), "i32"), PCT=t(21504, (2, 2), "f64"),
                OUT=t(24576, (2, 4, 4, 3), "u8"), B=2, C=3, H=8, W=8, SH=4, SW=4, NSRC=2, NROW=2, NQ=2)
    over = dict(CLS=t(32768, (2, 4, 4), "i64"), PALETTE=t(34816, (4, 3), "u8"), BASE=t(24576, (2, 4, 4, 3), "u8"), OUT=t(36864, (2, 4, 4, 3), "u8"),
                B=2, SH=4, SW=4, K=4, ALPHA=128, SKIP0=0)
    return {"TILE_RADIX_HIST": hist, "TILE_RANK_PICK": pick, "TILE_QUICKLOOK": look, "CLASS_OVERLAY": over}


BAD_DIMS = {
    "TILE_RADIX_HIST": [dict(M=0), dict(C=0), dict(H=0), dict(W=-1), dict(NSRC=0), dict(NBND=0), dict(NBND=17, C=20), dict(NBND=3, C=2),
                        dict(POOLED=2), dict(PASS=2), dict(PASS=-1), dict(R=0), dict(R=9), dict(H=1 << 16, W=1 << 15)],
    "TILE_RANK_PICK": [dict(G=0), dict(G=(1 << 27) + 1), dict(R=0), dict(R=9), dict(STEP=2), dict(STEP=-1), dict(N=0), dict(R=1)],
    "TILE_QUICKLOOK": [dict(B=0), dict(B=65536), dict(C=0), dict(SH=9), dict(SW=9), dict(SH=0), dict(SW=0), dict(NSRC=0), dict(NROW=0),
                       dict(NQ=1), dict(H=0)],
    "CLASS_OVERLAY": [dict(B=0), dict(SH=0), dict(SW=0), dict(K=0), dict(K=257), dict(ALPHA=-1), dict(ALPHA=257), dict(SKIP0=2),
                      dict(B=1 << 20, SH=1 << 20, SW=4)],
}
OPTIONAL = {"TILE_RADIX_HIST": set(), "TILE_RANK_PICK": {"RANKS", "FRAC", "PCT"}, "TILE_QUICKLOOK": set(), "CLASS_OVERLAY": {"BASE"}}


@pytest.mark.parametrize("kind", NEW)
def test_launchers_reject_bad_dims_missing_tensors_and_null_bases_on_the_host(kind):
    """Every check happens before any HIP call, so it can be exercised without a GPU."""
    from s2lc_amd import _lib
    from s2lc_amd.plan.program import Program, TRef

    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    good = _records()[kind]

    def run(fields):
        p = Program()
        p.add(kind, **fields)
        _lib.run(p.pack(), _lib.Bases().set("WS", ws), 0)

    for bad in BAD_DIMS[kind]:
        with pytest.raises(_lib.S2kError, match=kind.lower() + ": bad dims"):
            run({**good, **bad})
    tensors = D.OPS[kind][0]
    for name in tensors:
        if name not in OPTIONAL[kind]:
            with pytest.raises(_lib.S2kError, match=kind.lower() + ": missing tensor"):
                run({**good, name: None})
        ref = good[name]
        with pytest.raises(_lib.S2kError, match=kind.lower() + ": tensor references a null base"):
            run({**good, name: TRef(D.BASE["GRADS"], ref.off, ref.shape, ref.dtype)})
    if kind == "TILE_RADIX_HIST":          # BUCKET is only read by the fine pass
        with pytest.raises(_lib.S2kError, match="bad dims"):
            run({**good, "BUCKET": None, "PASS": 0, "R": 0})
    if kind == "TILE_RANK_PICK":           # step 0 reads RANKS, step 1 writes VALUES, a PCT needs its FRAC
        with pytest.raises(_lib.S2kError, match="missing tensor"):
            run({**good, "RANKS": None, "STEP": 0})
        with pytest.raises(_lib.S2kError, match="missing tensor"):
            run({**good, "FRAC": None})


@pytest.mark.parametrize("N", [1, 2, 7, 192, 786432])
def test_rank_plan_and_device_lerp_equal_numpy_percentile_bit_for_bit(N):
    q = [0, 0.5, 2, 50, 98, 99.9, 100]
    rng = np.random.default_rng(N)
    for name, vals in (("uniform", rng.integers(-32768, 32768, N).astype(np.int16)),
                       ("sentinel", np.where(rng.random(N) < 0.3, 0, rng.integers(1, 4001, N)).astype(np.int16))):
        srt = np.sort(vals)
        want = np.percentile(vals.astype(np.float64), q)
        ranks, frac = QL.rank_plan(q, N)
        assert len(ranks) == 2 * len(q) and len(frac) == len(q) and all(0 <= r < N for r in ranks)
        got = np.array([QL.lerp(srt[ranks[2 * i]], srt[ranks[2 * i + 1]], frac[i]) for i in range(len(q))])
        assert np.array_equal(got.view(np.int64), np.asarray(want, dtype=np.float64).view(np.int64)), (name, N, got, want)
        assert np.array_equal(R.percentiles(vals[None], q)[0], want)


def test_restatement_of_the_selection_is_consistent():
    """the histograms, the two pick steps and the sort agree with each other in numpy: the yardstick of the GPU test is sound"""
    rng = np.random.default_rng(0)
    raw = rng.integers(-32768, 32768, (3, 4, 8, 9)).astype(np.int16)
    raw[1] = np.where(rng.random((4, 8, 9)) < 0.5, 0, 7)
    for pooled in (False, True):
        grp = R.groups(raw, [2, 0, 1, 1], [3, 0], pooled)
        N = grp.shape[1]
        ranks = [0, N // 3, N // 3 + 1, N - 1]
        bucket, rest = R.pick0(R.coarse_hist(grp), ranks)
        fine = R.fine_hist(grp, bucket)
        low = np.stack([[np.searchsorted(np.cumsum(fine[g, r]), rest[g, r], side="right") for r in range(4)] for g in range(len(grp))])
        assert np.array_equal(((bucket.astype(np.int64) << 8) | low) - 32768, R.order_statistics(grp, ranks))
    assert QL.ZERO_BUCKET == 128 and int(R.key(0)) >> 8 == 128 and int(R.key(0)) & 255 == 0


def _cpu_pipe():
    p = GpuTilePipeline([0.1] * 4, [0.2] * 4, random_crop_size=8, device="cpu")
    g = torch.Generator().manual_seed(0)
    p.load(torch.randint(-100, 100, (3, 4, 16, 16), generator=g, dtype=torch.int32).to(torch.int16), None)
    return p


PALETTE = torch.tensor([[0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=torch.uint8)


def test_validators_raise_before_the_gpu_refusal():
    p = _cpu_pipe()
    cls = torch.zeros(2, 8, 8, dtype=torch.int64)
    pred = TilePredictor(lambda x: x, p, num_classes=4)
    bad = [
        lambda: p.band_percentiles([101.0]), lambda: p.band_percentiles([-0.1]), lambda: p.band_percentiles([]),
        lambda: p.band_percentiles([float("nan")]), lambda: p.band_percentiles([50], bands=[0, 0]), lambda: p.band_percentiles([50], bands=[4]),
        lambda: p.band_percentiles([50], bands=[]), lambda: p.band_percentiles([50], indices=[3]),
        lambda: p.zero_fraction(band=4), lambda: p.zero_fraction(band=-1), lambda: p.zero_fraction(indices=[-1]),
        lambda: p.quicklook(bands=(0, 1)), lambda: p.quicklook(bands=(0, 1, 1)), lambda: p.quicklook(bands=(0, 1, 4)),
        lambda: p.quicklook(percentile=50.0), lambda: p.quicklook(percentile=100.5), lambda: p.quicklook(indices=[3]),
        lambda: p.quicklook(params=[[0, 9, 0, 0]]), lambda: p.quicklook(params=[[0, 0, 0, 4]]), lambda: p.quicklook(params=[[3, 0, 0, 0]]),
        lambda: p.quicklook(params=[[0, 1, 0, 0]], whole_tile=True), lambda: p.quicklook(params=[[0, 0, 0]]),
        lambda: render.overlay(None, cls, PALETTE.float()), lambda: render.overlay(None, cls, PALETTE[:, :2]),
        lambda: render.overlay(None, cls, torch.zeros(257, 3, dtype=torch.uint8)), lambda: render.overlay(None, cls, PALETTE, alpha=1.5),
        lambda: render.overlay(None, cls.int(), PALETTE), lambda: render.overlay(None, cls[0], PALETTE),
        lambda: render.overlay(torch.zeros(2, 8, 8, 4, dtype=torch.uint8), cls, PALETTE),
        lambda: render.overlay(torch.zeros(2, 8, 8, 3), cls, PALETTE),
        lambda: pred.render([0], PALETTE[:3]), lambda: pred.render([0], PALETTE, alpha=-0.5), lambda: pred.render([5], PALETTE),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} did not raise")


def test_every_new_method_refuses_the_cpu():
    p = _cpu_pipe()
    cls = torch.zeros(2, 8, 8, dtype=torch.int64)
    pred = TilePredictor(lambda x: x, p, num_classes=4)
    calls = (lambda: p.band_percentiles([2, 98]), lambda: p.band_percentiles(50.0, indices=[2, 0, 2], bands=[1, 3], pooled=False),
             lambda: p.zero_fraction(), lambda: p.zero_fraction([1], band=3), lambda: p.quicklook(), lambda: p.quicklook(whole_tile=True),
             lambda: p.quicklook(params=[[2, 8, 0, 3]], bands=(3, 0, 1), percentile=99.5),
             lambda: render.overlay(None, cls, PALETTE), lambda: render.overlay(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), cls, PALETTE.numpy(), 0.25, True),
             lambda: pred.render([0, 1], PALETTE), lambda: pred.render(None, PALETTE, alpha=1.0))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_host_helpers():
    assert QL.rank_plan([2, 98], 786432)[0] == [15728, 15729, 770702, 770703]      # 0.02 * 786431 = 15728.62, 0.98 * 786431 = 770702.38
    ranks, frac = QL.rank_plan([0, 100], 5)
    assert ranks == [0, 1, 4, 4] and frac == [0.0, 0.0]
    assert QL.alpha_code(0) == 0 and QL.alpha_code(0.5) == 128 and QL.alpha_code(1) == 256
    assert QL.check_bands((2, 1, 0), 6, count=3) == [2, 1, 0]
    assert QL.check_palette(PALETTE.numpy()).dtype == torch.uint8
    with pytest.raises(ValueError):
        QL.rank_plan([50], 0)
