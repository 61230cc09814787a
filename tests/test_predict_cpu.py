"""CPU: the WINDOW_BLEND stage kind is registered (and no earlier kind moved), its launcher rejects bad dims on the host, the window
geometry / profiles of predict.py hold their invariants, the numpy restatement (tests/blend_ref.py) degenerates to plain tiling, and
`TilePredictor` validates its arguments before it refuses to run off the GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import predict as P
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.plan import opdefs as D
from tests.blend_ref import blend_ref, confusion, mask_and_margin

ROOT = Path(__file__).resolve().parents[1]
# the stage kinds as they were numbered before WINDOW_BLEND was appended
KINDS_BEFORE = ["MEMSET", "AXPY", "WEIGHT_PACK", "CONV", "WGRAD", "WGRAD_FINALIZE", "DWCONV_FWD", "DWCONV_DGRAD", "DWCONV_WGRAD",
                "BN_FINALIZE", "SE_POOL", "SE_FC", "SE_FC_BWD", "SE_BWD_REDUCE", "BN_BWD_REDUCE", "BN_BWD_FINALIZE", "BN_BWD_APPLY",
                "BN_RESIDUAL", "CHANNEL_SUM", "LOSS_FWD", "LOSS_BWD", "ARGMAX", "CHAN_LN_FWD", "CHAN_LN_BWD", "ACT_BWD", "ACT_FWD",
                "ATTN_FWD", "ATTN_BWD", "MAE_MASK_INDEX", "IDS_TO_DEC_IDX", "TOKEN_GATHER", "TOKEN_SCATTER", "PATCHIFY", "MAE_LOSS_FWD",
                "MAE_LOSS_BWD", "TRANSPOSE_CL", "CONFUSION", "DROP_GATE", "TILE_PREP", "SE_BN_SUMS", "SE_BN_COMBINE", "SPACE_TO_DEPTH",
                "UPSAMPLE_ZERO", "SE_FC_WGRAD", "IM2COL", "TILE_LABEL_HIST", "TILE_MOMENTS"]


def test_window_blend_is_appended_and_named_by_the_library():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g
    from s2lc_amd import _lib

    g.build()
    assert D.KIND["WINDOW_BLEND"] == 48
    assert [D.KIND[k] for k in KINDS_BEFORE] == list(range(1, 48))
    L = _lib.lib()
    assert L.s2k_abi_version() == 2
    assert L.s2k_kind_name(48).decode() == "WINDOW_BLEND"
    assert D.WRITES["WINDOW_BLEND"] == ("BLEND", "MASK", "HIST")


def test_launcher_rejects_bad_dims_on_the_host():
    """Range checks happen before any launch, so they can be exercised without a GPU."""
    from s2lc_amd import _lib
    from s2lc_amd.plan.program import Program, TRef

    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    t = lambda off, shape, dt="f32": TRef(D.BASE["WS"], off, shape, dt)      # noqa: E731
    good = dict(LOGITS=t(0, (1, 1, 1, 1, 4, 8, 8)), YS=t(2048, (1,), "i32"), XS=t(2304, (1,), "i32"), FLIPS=t(2560, (1,), "i32"),
                W1=t(2816, (8,)), BLEND=t(4096, (1, 4, 8, 8)), MASK=t(8192, (1, 8, 8), "i64"), LABELS=t(12288, (2, 8, 8), "u8"),
                INDEX=t(12544, (1,), "i32"), LUT=t(12800, (256,), "i32"), HIST=t(14336, (4, 4), "i64"),
                M=1, F=1, NY=1, NX=1, K=4, H=8, W=8, S=8, NSRC=2, MODE=0)
    bad_cases = [dict(K=0), dict(K=33), dict(F=0), dict(F=5), dict(S=0), dict(S=9), dict(S=8, H=16, W=7), dict(M=0), dict(MODE=2),
                 dict(MODE=-1), dict(BLEND=None, MASK=None, HIST=None), dict(LABELS=None), dict(INDEX=None), dict(LUT=None),
                 dict(M=1 << 20, K=32),                       # 2^20 * 32 * 64 = 2^31 elements of LOGITS
                 dict(M=1 << 30, F=4, NY=1 << 30, NX=1 << 30, K=32, H=1 << 20, W=1 << 20, S=1 << 20)]     # a product beyond 64 bits
    for bad in bad_cases:
        p = Program()
        p.add("WINDOW_BLEND", **{**good, **bad})
        with pytest.raises(_lib.S2kError, match="window_blend: bad dims"):
            _lib.run(p.pack(), _lib.Bases().set("WS", ws), 0)
    p = Program()
    p.add("WINDOW_BLEND", **{**good, "W1": None})
    with pytest.raises(_lib.S2kError, match="window_blend: missing tensor"):
        _lib.run(p.pack(), _lib.Bases().set("WS", ws), 0)


@pytest.mark.parametrize("size,S,stride", [(40, 16, 8), (54, 16, 8), (54, 16, 12), (16, 16, 8), (512, 224, 112)])
def test_window_origins_cover_the_tile(size, S, stride):
    o = P.window_origins(size, S, stride)
    assert o[0] == 0 and o[-1] == size - S
    assert all(b > a for a, b in zip(o[:-1], o[1:]))                        # ascending and unique
    covered = np.zeros(size, dtype=bool)
    for v in o:
        assert 0 <= v <= size - S
        covered[v:v + S] = True
    assert covered.all()
    assert o[:-1] == list(range(0, size - S, stride))[:len(o) - 1]          # 0, stride, 2 stride, ... then the clamped last one
    P.check_origins(o, size, S)


def test_window_origins_expected_lists_and_errors():
    assert P.window_origins(40, 16, 8) == [0, 8, 16, 24]
    assert P.window_origins(54, 16, 8) == [0, 8, 16, 24, 32, 38]
    assert P.window_origins(54, 16, 12) == [0, 12, 24, 36, 38]
    assert P.window_origins(16, 16, 8) == [0]
    assert P.window_origins(512, 224, 112) == [0, 112, 224, 288]
    for bad in ((8, 16, 8), (40, 16, 0), (40, 16, 17), (40, 0, 1)):
        with pytest.raises(ValueError):
            P.window_origins(*bad)
    for bad in ([0, 8, 8, 24], [8, 16, 24], [0, 8, 16], [0, 24], [0, 16, 8, 24], []):
        with pytest.raises(ValueError):
            P.check_origins(bad, 40, 16)


@pytest.mark.parametrize("S", [1, 2, 12, 15, 16, 224])
def test_window_profiles_are_strictly_positive_and_symmetric(S):
    for kind in ("hann", "uniform"):
        w = P.window_profile(S, kind)
        assert w.dtype == torch.float32 and w.shape == (S,)
        assert bool((w > 0).all()) and torch.equal(w, w.flip(0))
    assert torch.equal(P.window_profile(S, "uniform"), torch.ones(S))
    want = np.sin(np.pi * (np.arange(S) + 0.5) / S) ** 2
    assert np.abs(P.window_profile(S, "hann").numpy() - want).max() <= 2.0 ** -24
    with pytest.raises(ValueError):
        P.window_profile(S, "triangle")


def test_reference_with_uniform_profile_and_stride_S_is_plain_tiling():
    rng = np.random.default_rng(0)
    M, K, S, NY, NX = 2, 3, 8, 2, 3
    H, W = NY * S, NX * S
    ys, xs = P.window_origins(H, S, S), P.window_origins(W, S, S)
    assert ys == [0, 8] and xs == [0, 8, 16]
    logits = rng.normal(0, 3, (M, 1, NY, NX, K, S, S)).astype(np.float32)
    got, T = blend_ref(logits, ys, xs, [0], P.window_profile(S, "uniform").numpy(), H, W, mode=0)
    want = logits[:, 0].transpose(0, 3, 1, 4, 2, 5).reshape(M, K, H, W).astype(np.float64)       # [M, K, NY, S, NX, S]
    assert T == 1 and np.array_equal(got, want)
    # every flip variant of a tile, predicted by the identity "model" and un-flipped, gives the tile back
    tile = rng.normal(0, 3, (1, K, H, W)).astype(np.float32)
    flips = [0, 1, 2, 3]
    lg = np.zeros((1, 4, NY, NX, K, S, S), dtype=np.float32)
    for f, fl in enumerate(flips):
        for i, y0 in enumerate(ys):
            for j, x0 in enumerate(xs):
                win = tile[0, :, y0:y0 + S, x0:x0 + S]
                win = win[..., ::-1] if fl & 1 else win
                lg[0, f, i, j] = win[..., ::-1, :] if fl & 2 else win
    got, T = blend_ref(lg, ys, xs, flips, P.window_profile(S, "hann").numpy(), H, W, mode=0)
    assert T == 4 and np.abs(got - tile).max() < 1e-12
    mask, margin = mask_and_margin(got)
    assert np.array_equal(mask, tile.argmax(axis=1)) and margin.min() >= 0
    assert confusion(np.array([0, 1, 5, 1]), np.array([1, 1, 0, 0]), 2).tolist() == [[0, 1], [1, 1]]


def _cpu_pipe(labels=True):
    p = GpuTilePipeline([0.1] * 3, [0.2] * 3, random_crop_size=8, device="cpu", squeeze_time_dim=True)
    g = torch.Generator().manual_seed(0)
    raw = torch.randint(-100, 100, (3, 3, 16, 20), generator=g, dtype=torch.int32).to(torch.int16)
    lab = torch.randint(0, 4, (3, 16, 20), generator=g, dtype=torch.int32).to(torch.uint8)
    p.load(raw, lab if labels else None)
    return p


def test_tile_predictor_validates_then_refuses_the_cpu():
    from s2lc_amd.metrics import SegMetrics

    pipe = _cpu_pipe()
    model = lambda x: x[:, :3]      # noqa: E731
    for bad in (dict(num_classes=0), dict(num_classes=33), dict(stride=0), dict(stride=9), dict(window="triangle"), dict(blend="mean"),
                dict(flips=()), dict(flips=(0, 0)), dict(flips=(4,)), dict(flips=(0, 1, 2, 3, 1)), dict(windows_per_batch=0),
                dict(tiles_per_launch=0)):
        with pytest.raises(ValueError):
            P.TilePredictor(model, pipe, **{"num_classes": 3, **bad})
    pred = P.TilePredictor(model, pipe, 3)
    assert pred.stride == 4 and pred.mode == 1 and pred.flips == [0] and torch.equal(pred.profile, P.window_profile(8, "hann"))
    for bad in ([3], [-1], []):
        with pytest.raises(ValueError, match="out of range"):
            pred.predict(bad)
        with pytest.raises(ValueError, match="out of range"):
            pred.predict_blend(bad)
    with pytest.raises(ValueError, match="num_classes"):
        pred.evaluate(SegMetrics(4, device="cpu"))
    with pytest.raises(ValueError, match="without labels"):
        P.TilePredictor(model, _cpu_pipe(labels=False), 3).evaluate(SegMetrics(3, device="cpu"))
    with pytest.raises(ValueError, match="tiles_per_launch"):
        P.TilePredictor(model, pipe, 32, stride=1, flips=(0, 1, 2, 3), tiles_per_launch=1 << 20).predict()
    for call in (lambda: pred.predict(), lambda: pred.predict([2, 0, 2]), lambda: pred.predict_blend(),
                 lambda: pred.evaluate(SegMetrics(3, device="cpu"))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
