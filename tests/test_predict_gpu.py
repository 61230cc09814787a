"""GPU: the WINDOW_BLEND stage (csrc/predict.hip) as one-record programs through the C ABI against its float64 numpy restatement
(tests/blend_ref.py; the op has no entry in oracle/ops_ref.py), and `predict.TilePredictor` end to end over a real `GpuTilePipeline`.

Bars.
* BLEND, MODE 0: (T + 4) * 2^-23 * max|v|, T = the largest number of terms on a pixel - the T products and additions, the weight
  product and the sum of weights each round at 2^-24, one division on top.
* BLEND, MODE 1: the device's exp adds an error that is measured, not derived.  Largest deviation from the float64 reference over the
  stage cases below on an MI355X: 4.157e-07 (40x54_s12, K = 23, F = 1; 48 cases, all between 8.2e-08 and 4.2e-07); the bar is 4x that,
  1.663e-06, because exp implementations differ by a few ulp between compiler versions.
* MASK: equal to the reference's first maximum on every pixel whose float64 top-2 margin exceeds twice the BLEND bar; at most 1 % of the
  pixels may be left out (the inputs leave out far fewer).
* Exact case (uniform profile, integer logits in [-8, 8], MODE 0: every sum is exact in float32): MASK equal everywhere, engineered
  ties resolved to the first class, BLEND within one float32 ulp (the division).
* HIST: exact."""
import functools

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import predict as P
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.metrics import SegMetrics
from s2lc_amd.plan.program import Program
from tests.blend_ref import blend_ref, confusion, mask_and_margin
from tests.test_ops_gpu import Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MEASURED_MODE1 = 4.157e-7        # largest |BLEND - float64 reference| of the MODE 1 stage cases, measured on an MI355X
BAR_MODE1 = 4 * MEASURED_MODE1

# name: (H, W, S, stride)
SHAPES = {
    "40x54_s8": (40, 54, 16, 8),          # origins 0,8,16,24 / 0,8,...,32,38: the last one clamped and unaligned, coverage 3 on that axis
    "40x54_s12": (40, 54, 16, 12),
    "32x48_tiling": (32, 48, 16, 16),     # no overlap: coverage 1
    "16x16_one": (16, 16, 16, 8),         # one window
    "28x36_s4": (28, 36, 12, 4),
    "23x27_odd": (23, 27, 10, 7),         # S % 4 != 0 and W % 4 != 0: no quad reads, scalar stores, a quad that hangs over the edge
}
INDEX = [2, 0, 2]                         # M = 3 tile slots, one label raster used twice
NSRC = 3


def run_records(c: Case, records) -> torch.Tensor:
    """the records through `_lib.run` over c's arena; returns the arena's bytes afterwards (c.read takes tensors out of them)"""
    from s2lc_amd import _lib

    prog = Program()
    for kind, fields in records:
        prog.add(kind, **fields)
    cpu = torch.zeros(c.arena.top + 256, dtype=torch.uint8)
    for ref, data in c.items.values():
        cpu[ref.off:ref.off + ref.nbytes] = data.contiguous().reshape(-1).view(torch.uint8)
    gpu = cpu.cuda()
    _lib.run(prog.pack(), _lib.Bases().set("WS", gpu), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return gpu.cpu()


def geometry(shape):
    H, W, S, stride = SHAPES[shape]
    return H, W, S, P.window_origins(H, S, stride), P.window_origins(W, S, stride)


@functools.lru_cache(maxsize=None)
def inputs(shape, K, F):
    """float32 N(0, 3^2) logits [3, F, NY, NX, K, S, S], labels uint8 [NSRC, H, W] and a LUT with values 0 .. K + 2 (K .. K + 2 skipped)"""
    H, W, S, ys, xs = geometry(shape)
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(len(INDEX), F, len(ys), len(xs), K, S, S, generator=g) * 3
    labels = torch.randint(0, 256, (NSRC, H, W), generator=g, dtype=torch.int32).to(torch.uint8)
    lut = torch.arange(256, dtype=torch.int32) % (K + 3)
    return logits, labels, lut


def run_stage(shape, logits, flips, profile, mode, labels=None, lut=None, want=("blend", "mask", "hist"), repeat=1):
    """one WINDOW_BLEND record (`repeat` times in one program) -> {"blend", "mask", "hist"} numpy arrays of the requested outputs"""
    H, W, S, ys, xs = geometry(shape)
    M, F, NY, NX, K = logits.shape[:5]
    c = Case(5)
    fields = dict(LOGITS=c.t("logits", tuple(logits.shape), logits), YS=c.t("ys", (NY,), torch.tensor(ys), "i32"),
                  XS=c.t("xs", (NX,), torch.tensor(xs), "i32"), FLIPS=c.t("flips", (F,), torch.tensor(flips), "i32"),
                  W1=c.t("w1", (S,), profile), M=M, F=F, NY=NY, NX=NX, K=K, H=H, W=W, S=S, NSRC=NSRC, MODE=mode)
    if "blend" in want:
        fields["BLEND"] = c.t("blend", (M, K, H, W), "nan")
    if "mask" in want:
        fields["MASK"] = c.t("mask", (M, H, W), torch.full((M, H, W), -1), "i64")
    if "hist" in want:
        fields.update(LABELS=c.t("labels", (NSRC, H, W), labels, "u8"), INDEX=c.t("index", (M,), torch.tensor(INDEX[:M]), "i32"),
                      LUT=c.t("lut", (256,), lut, "i32"), HIST=c.t("hist", (K, K), torch.zeros(K, K), "i64"))
    img = run_records(c, [("WINDOW_BLEND", fields)] * repeat)
    return {k: c.read(img, k).numpy().copy() for k in want}


def check_mask(got_mask, ref, bar, what):
    want_mask, margin = mask_and_margin(ref)
    safe = margin > 2 * bar
    left_out = 1.0 - safe.mean()
    print(f"{what}: mask pixels left out {left_out:.4%}")
    assert left_out <= 0.01
    assert np.array_equal(got_mask[safe], want_mask[safe])
    assert got_mask.min() >= 0 and got_mask.max() < ref.shape[1]


@pytest.mark.parametrize("mode", [0, 1], ids=["logits", "probs"])
@pytest.mark.parametrize("F", [1, 4])
@pytest.mark.parametrize("K", [2, 4, 5, 23])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stage_matches_the_float64_reference(shape, K, F, mode):
    H, W, S, ys, xs = geometry(shape)
    logits, labels, lut = inputs(shape, K, F)
    flips = [0, 1, 2, 3][:F]
    profile = P.window_profile(S, "hann")
    got = run_stage(shape, logits, flips, profile, mode, labels, lut)
    ref, T = blend_ref(logits.numpy(), ys, xs, flips, profile.numpy(), H, W, mode)
    bar = (T + 4) * 2.0 ** -23 * float(logits.abs().max()) if mode == 0 else BAR_MODE1
    err = float(np.abs(got["blend"] - ref).max())
    print(f"{shape} K={K} F={F} mode={mode}: T={T} blend err {err:.3e} bar {bar:.3e}")
    assert np.isfinite(got["blend"]).all() and err <= bar
    check_mask(got["mask"], ref, bar, f"{shape} K={K} F={F} mode={mode}")
    # HIST is the bincount of (LUT[labels], MASK read back); LUT values K .. K + 2 are skipped
    true = lut.numpy()[labels.numpy()[INDEX]]
    want_hist = confusion(true, got["mask"], K)
    assert 0 < want_hist.sum() < true.size
    assert np.array_equal(got["hist"], want_hist)


def _exact_inputs(shape, K, F):
    H, W, S, ys, xs = geometry(shape)
    g = torch.Generator().manual_seed(1)
    logits = torch.randint(-8, 9, (len(INDEX), F, len(ys), len(xs), K, S, S), generator=g).float()
    logits[:, :, :, :, 2] = logits[:, :, :, :, 1]        # wherever class 1 leads, class 2 ties with it: 1 must win
    logits[0] = 3.0                                      # tile slot 0: every class ties everywhere: 0 must win
    return logits


@pytest.mark.parametrize("F", [1, 4])
@pytest.mark.parametrize("K", [4, 23])
@pytest.mark.parametrize("shape", ["40x54_s8", "28x36_s4", "23x27_odd"])
def test_exact_case_mask_everywhere_and_blend_within_one_ulp(shape, K, F):
    H, W, S, ys, xs = geometry(shape)
    logits, (_, labels, lut) = _exact_inputs(shape, K, F), inputs(shape, K, F)
    flips = [0, 1, 2, 3][:F]
    profile = P.window_profile(S, "uniform")
    got = run_stage(shape, logits, flips, profile, 0, labels, lut)
    ref, _ = blend_ref(logits.numpy(), ys, xs, flips, profile.numpy(), H, W, 0)
    want_mask, _ = mask_and_margin(ref)
    assert np.array_equal(got["mask"], want_mask)
    assert not got["mask"][0].any() and 2 not in got["mask"] and (got["mask"] == 1).any()
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(got["blend"] - ref) <= ulp).all()
    assert np.array_equal(got["hist"], confusion(lut.numpy()[labels.numpy()[INDEX]], want_mask, K))      # the reference's own mask


def test_hist_accumulates_over_two_records():
    shape, K, F = "40x54_s8", 5, 1
    logits, labels, lut = inputs(shape, K, F)
    profile = P.window_profile(16, "hann")
    once = run_stage(shape, logits, [0], profile, 1, labels, lut, want=("mask", "hist"))
    twice = run_stage(shape, logits, [0], profile, 1, labels, lut, want=("hist",), repeat=2)      # HIST as the only output
    assert np.array_equal(once["hist"], confusion(lut.numpy()[labels.numpy()[INDEX]], once["mask"], K))
    assert np.array_equal(twice["hist"], 2 * once["hist"])


def test_hist_single_label_single_prediction_lands_in_one_bin():
    shape, K = "40x54_s8", 4
    H, W, S, ys, xs = geometry(shape)
    logits = inputs(shape, K, 1)[0][:1].clone()
    logits[:, :, :, :, 2] += 100.0                       # class 2 everywhere
    labels = torch.full((NSRC, H, W), 7, dtype=torch.uint8)
    lut = torch.zeros(256, dtype=torch.int32)
    lut[7] = 3
    got = run_stage(shape, logits, [0], P.window_profile(S, "hann"), 0, labels, lut, want=("mask", "hist"))
    want = np.zeros((K, K), dtype=np.int64)
    want[3, 2] = H * W
    assert (got["mask"] == 2).all() and np.array_equal(got["hist"], want)


@pytest.mark.parametrize("mode", [0, 1], ids=["logits", "probs"])
def test_two_runs_are_bit_identical(mode):
    shape, K, F = "40x54_s8", 23, 4
    logits, labels, lut = inputs(shape, K, F)
    profile = P.window_profile(16, "hann")
    a = run_stage(shape, logits, [0, 1, 2, 3], profile, mode, labels, lut)
    b = run_stage(shape, logits, [0, 1, 2, 3], profile, mode, labels, lut)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- TilePredictor end to end -------------------------------------------------------------------------------------------------
N_TILES, BANDS, TH, TW = 3, 4, 96, 128


@functools.lru_cache(maxsize=None)
def _tiles():
    g = torch.Generator().manual_seed(7)
    raw = torch.randint(-500, 9000, (N_TILES, BANDS, TH, TW), generator=g, dtype=torch.int32).to(torch.int16)
    labels = torch.randint(0, 24, (N_TILES, TH, TW), generator=g, dtype=torch.int32).to(torch.uint8)
    return raw, labels


def _pipe(S):
    pipe = GpuTilePipeline([0.05, 0.06, 0.07, 0.08], [0.02, 0.03, 0.025, 0.035], random_crop_size=S, label_map="cnes-multiclass",
                           squeeze_time_dim=True, device=DEV)
    pipe.load(*_tiles())
    return pipe


class Pointwise:
    """a fixed per-pixel 1 x 1 projection, written as elementwise multiplies and adds in a fixed order so that a pixel's logits do
    not depend on the shape of the batch it arrives in"""

    def __init__(self, K, C, seed=3):
        g = torch.Generator().manual_seed(seed)
        self.w = (torch.randn(K, C, generator=g) * 2).to(DEV)
        self.b = torch.randn(K, generator=g).to(DEV)

    def __call__(self, x):
        out = self.b.view(1, -1, 1, 1).expand(x.shape[0], -1, x.shape[2], x.shape[3])
        for c in range(x.shape[1]):
            out = out + x[:, c:c + 1] * self.w[:, c].view(1, -1, 1, 1)
        return out.contiguous()


def _whole_tiles(pipe):
    """the whole tiles normalised exactly as TILE_PREP normalises a crop: (float(x) - mean * 255) * (1 / (std * 255)), two roundings"""
    return (pipe.raw.float() - pipe.norm[0].view(1, -1, 1, 1)) * pipe.norm[1].view(1, -1, 1, 1)


@pytest.mark.parametrize("flips", [(0,), (0, 1, 2, 3)], ids=["noflip", "flips4"])
@pytest.mark.parametrize("window", ["hann", "uniform"])
@pytest.mark.parametrize("stride", [16, 20])
def test_predict_blend_of_a_pointwise_model_is_the_model_on_the_whole_tile(stride, window, flips):
    K = 5
    pipe, model = _pipe(32), Pointwise(K, BANDS)
    pred = P.TilePredictor(model, pipe, K, stride=stride, window=window, blend="logits", flips=flips, windows_per_batch=32,
                           tiles_per_launch=2)
    got = pred.predict_blend([2, 0, 1, 2])
    want = model(_whole_tiles(pipe))[[2, 0, 1, 2]]
    assert got.shape == (4, K, TH, TW) and got.dtype == torch.float32 and got.is_cuda
    cover = lambda size: max(sum(v <= q < v + 32 for v in P.window_origins(size, 32, stride)) for q in range(size))      # noqa: E731
    T = len(flips) * cover(TH) * cover(TW)
    bar = (T + 4) * 2.0 ** -23 * float(want.abs().max())
    err = float((got.double() - want.double()).abs().max())
    print(f"stride {stride} {window} flips {flips}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar


def test_windows_per_batch_does_not_change_a_byte():
    K = 4
    pipe, model = _pipe(32), Pointwise(K, BANDS)
    kw = dict(stride=16, flips=(0, 3), blend="probs")
    a = P.TilePredictor(model, pipe, K, windows_per_batch=5, **kw).predict_blend()      # 3 * 2 * 5 * 7 = 210 windows: ragged last batch
    b = P.TilePredictor(model, pipe, K, windows_per_batch=64, **kw).predict_blend()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float((a.sum(1) - 1).abs().max()) < 1e-5      # blended probabilities


def test_evaluate_leaves_the_counts_of_the_confusion_stage():
    K = 4
    pipe, model = _pipe(32), Pointwise(K, BANDS)
    pred = P.TilePredictor(model, pipe, K, flips=(0, 1), tiles_per_launch=2)
    idx = [1, 2, 2]
    fused, staged = SegMetrics(K, device=DEV), SegMetrics(K, device=DEV)
    pred.evaluate(fused, idx)
    mask = pred.predict(idx)
    assert mask.shape == (3, TH, TW) and mask.dtype == torch.int64 and mask.is_cuda
    remapped = pipe.lut.long()[pipe.labels[idx].long()]
    staged.update(mask, remapped)
    assert int(staged.hist.sum()) == 3 * TH * TW and torch.equal(fused.hist, staged.hist)
    pred.evaluate(fused, idx)                            # accumulates
    assert torch.equal(fused.hist, 2 * staged.hist)
    assert set(fused.compute()) == {"confusion_matrix", "iou", "accuracy", "f1"}


def test_unet_b0_predict_equals_the_reference_blend_of_its_own_window_logits():
    from oracle import detgen
    from oracle import efficientnet_unet_ref as R
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet

    K, S = 4, 64
    model = EfficientnetUnet(EfficientNetConfig("b0", BANDS, K, class_distribution=[0.25] * 4))
    model.load_state_dict(detgen.fill_state(R.state_shapes(R.build("b0", BANDS, K)), seed=5))
    model.to(DEV).eval()
    pipe = _pipe(S)
    pred = P.TilePredictor(model, pipe, K, windows_per_batch=6)
    got = pred.predict([1]).cpu().numpy()
    ys, xs = P.window_origins(TH, S, 32), P.window_origins(TW, S, 32)
    par = torch.tensor([[1, y0, x0, 0] for y0 in ys for x0 in xs], dtype=torch.int32)
    with torch.no_grad():
        logits = model(pipe(params=par).x).cpu().numpy().reshape(1, 1, len(ys), len(xs), K, S, S)
    ref, _ = blend_ref(logits, ys, xs, [0], pred.profile.numpy(), TH, TW, 1)
    check_mask(got, ref, BAR_MODE1, "unet b0")
    assert not model.training
