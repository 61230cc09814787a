"""GPU: `render.mae_panels` / `s2k_mae_panels` (csrc/mae_render.hip) against the numpy restatement (tests/mae_render_ref.py), the
panel algebra on the GPU output alone, PATCH_MSE against the restatement and against the loss a real model returns, and the panels
beside `GpuTilePipeline.quicklook` through `stretch_bounds`.

Bars.  Without norm_pix every byte is the restatement's (float64, every operation rounded on its own, in the same order).  With
norm_pix the order of the float64 patch sums is the kernel's own: a byte may differ by ONE level, and only where the restatement's
value before truncation lies within 1e-6 of an integer - a condition, not a share: reordering at most 4096 float64 terms moves a value
by about 1e-12 relative, and the inputs keep |v - lo| / (hi - lo) below 100.  PATCH_MSE: max |error| / max |restatement| < 2e-5, the bar
tests/test_vit_ops_gpu.py uses for MAE_LOSS; the masked mean of PATCH_MSE against the model's own loss within the same 2e-5.  The
original panel beside the quicklook of the same crop: at most one level, and only where the quicklook's value before truncation lies
within 4 ulp (float32, at the crop's largest |raw - mean*255|) * 255 / (hi - lo) of an integer - the rounding TILE_PREP's float32
result carries."""
import functools

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import _lib, render
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.modules.prithvi import MaskedAutoencoderViT
from tests import mae_render_ref as R
from tests import quicklook_ref as QR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PANELS = ("original", "masked", "pasted", "reconstruction")

# name: (B, C, T, TUB, img, P, frame, bands)
GEOMS = {
    "g2": (2, 3, 1, 1, 32, 16, 0, (2, 1, 0)),                 # two patches per side
    "t2_frame1": (3, 6, 2, 1, 32, 8, 1, (2, 1, 0)),           # the token offset t * g^2
    "tub2_frame1": (2, 4, 2, 2, 16, 4, 1, (2, 1, 0)),         # tt = 1 inside a tubelet; 16 pixels per patch, fewer than a wave
    "odd13": (2, 13, 1, 1, 48, 16, 0, (12, 0, 7)),            # odd grid, bands out of order
    "prithvi14": (1, 6, 1, 1, 224, 16, 0, (2, 1, 0)),         # a grid of 14: no multiple of a workgroup's four patches
    "p6": (2, 3, 1, 1, 12, 6, 0, (0, 2, 1)),                  # a patch side that is no multiple of 4: the element loads and byte stores
}
# samples whose bounds leave no range: hi == lo, a NaN bound
BAD_BOUNDS = {"t2_frame1": {1: (700.0, 700.0), 2: (float("nan"), 1800.0)}, "g2": {1: (900.0, 900.0)}, "odd13": {1: (400.0, float("nan"))}}


@functools.lru_cache(maxsize=None)
def model_for(C, T, TUB, S, P, norm_pix):
    """only its spec is read by render.mae_panels: it stays on the CPU"""
    return MaskedAutoencoderViT(img_size=S, patch_size=P, num_frames=T, tubelet_size=TUB, in_chans=C, embed_dim=16, depth=1, num_heads=2,
                                decoder_embed_dim=16, decoder_depth=1, decoder_num_heads=2, norm_pix_loss=norm_pix)


@functools.lru_cache(maxsize=None)
def inputs(name, norm_pix):
    """CPU tensors of one case: imgs seeded normal; pred = the (standardised) patches plus noise, one displayed patch holding NaN, +inf
    and -inf; a seeded mask with both values; bounds distinct per sample that clip at both ends (v spreads over about mean +- 3 std =
    -1300 .. 3300 raw units around bounds of 400 .. 2000)"""
    B, C, T, TUB, S, P, frame, bands = GEOMS[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + int(norm_pix))
    imgs = torch.randn(B, C, T, S, S, generator=g)
    patches = torch.from_numpy(R.patchify(imgs.numpy(), P, TUB))
    if norm_pix:
        patches = (patches - patches.mean(-1, keepdim=True)) / (patches.var(-1, keepdim=True) + 1e-6) ** 0.5
    pred = (patches + 0.1 * torch.randn(patches.shape, generator=g)).contiguous()
    L, gs = pred.shape[1], S // P
    t0, tt0 = frame // TUB, frame % TUB
    special = t0 * gs * gs + gs + 1                                      # patch (1, 1) of the displayed tubelet row, sample 0
    for px, val in enumerate((float("nan"), float("inf"), float("-inf"))):
        pred[0, special, ((tt0 * P + 1) * P + px) * C + bands[0]] = val
    mask = (torch.rand(B, L, generator=g) < 0.6).float()
    mask[0, special], mask[0, special - 1] = 1.0, 0.0
    norm = torch.stack([torch.rand(C, generator=g) * 1000 + 500, 1.0 / (torch.rand(C, generator=g) * 400 + 200)]).float()
    bounds = torch.tensor([[400.0 + 50.0 * b, 1800.0 + 100.0 * b] for b in range(B)], dtype=torch.float64)
    for b, pair in BAD_BOUNDS.get(name, {}).items():
        bounds[b] = torch.tensor(pair, dtype=torch.float64)
    return imgs, pred, mask, norm, bounds


def run(name, norm_pix, mask=None, panels=PANELS, fill=128, patch_mse=False):
    B, C, T, TUB, S, P, frame, bands = GEOMS[name]
    imgs, pred, m, norm, bounds = inputs(name, norm_pix)
    m = m if mask is None else mask
    out = render.mae_panels(model_for(C, T, TUB, S, P, norm_pix), imgs.to(DEV), pred.to(DEV), m.to(DEV), norm.to(DEV), bounds.to(DEV),
                            panels=panels, bands=bands, frame=frame, fill=fill, patch_mse=patch_mse)
    torch.cuda.synchronize()
    if patch_mse:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


def want(name, norm_pix, mask=None, codes=(0, 1, 2, 3), fill=128):
    B, C, T, TUB, S, P, frame, bands = GEOMS[name]
    imgs, pred, m, norm, bounds = inputs(name, norm_pix)
    m = m if mask is None else mask
    return R.panels(imgs.numpy(), pred.numpy(), m.numpy(), norm.numpy(), bounds.numpy(), P, TUB, bands, frame, codes, fill, norm_pix)


def compare(got, ref, before, norm_pix, what):
    """exact without norm_pix; with it, one level and only where the restatement's value sits within 1e-6 of an integer"""
    assert got.shape == ref.shape and got.dtype == np.uint8
    diff = got.astype(np.int16) - ref.astype(np.int16)
    used = int((diff != 0).sum())
    print(f"{what}: {used} of {diff.size} bytes differ from the restatement")
    if not norm_pix:
        assert used == 0, (what, used)
        return
    near = np.abs(before - np.round(before)) < 1e-6
    assert np.abs(diff).max() <= 1 and not (diff != 0)[~near].any(), (what, used, int((diff != 0)[~near].sum()))


@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm_pix"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_panels_and_patch_mse_match_the_restatement(name, norm_pix):
    B, C, T, TUB, S, P, frame, bands = GEOMS[name]
    imgs, pred, mask, norm, bounds = inputs(name, norm_pix)
    assert 0 < mask.sum() < mask.numel()
    got, mse = run(name, norm_pix, patch_mse=True)
    ref, before = want(name, norm_pix)
    assert got.shape == (B, 4, S, S, 3)
    compare(got, ref, before, norm_pix, f"{name} norm_pix={int(norm_pix)}")
    good = [b for b in range(B) if b not in BAD_BOUNDS.get(name, {})]
    assert (ref[good, 0] == 0).any() and (ref[good, 0] == 255).any() and len(np.unique(ref[good, 0])) > 100      # clips at both ends
    for b in BAD_BOUNDS.get(name, {}):
        assert not got[b, 0].any() and not got[b, 2:].any() and set(np.unique(got[b, 1])) <= {0, 128}
    # the patch with NaN, +inf, -inf in the first displayed band: 0, 255, 0 in the reconstruction (sample 0 has proper bounds)
    i, j = P + 1, P
    assert got[0, 3, i, j:j + 3, 0].tolist() == [0, 255, 0]
    # PATCH_MSE: every patch, also those of other tubelet rows; the patch holding NaN gives NaN on both sides
    ref_mse = R.patch_mse(imgs.numpy(), pred.numpy(), P, TUB, norm_pix)
    assert mse.shape == ref_mse.shape == (B, mask.shape[1]) and mse.dtype == np.float32
    fin = np.isfinite(ref_mse)
    assert np.array_equal(np.isfinite(mse), fin) and int((~fin).sum()) == 1
    err = np.abs(mse[fin] - ref_mse[fin]).max() / np.abs(ref_mse[fin]).max()
    print(f"{name} norm_pix={int(norm_pix)}: PATCH_MSE error {err:.2e}")
    assert err < 2e-5
    # two runs are bit-identical, with and without PATCH_MSE asked for
    again, mse2 = run(name, norm_pix, patch_mse=True)
    assert again.tobytes() == got.tobytes() and mse2.tobytes() == mse.tobytes()
    assert run(name, norm_pix).tobytes() == got.tobytes()


@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm_pix"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_panel_algebra_on_the_gpu_output(name, norm_pix):
    B, C, T, TUB, S, P, frame, bands = GEOMS[name]
    mask = inputs(name, norm_pix)[2]
    got = run(name, norm_pix, fill=93)
    gs, t0 = S // P, frame // TUB
    rem = (mask[:, t0 * gs * gs:(t0 + 1) * gs * gs].reshape(B, gs, gs) != 0).repeat_interleave(P, 1).repeat_interleave(P, 2).numpy()[..., None]
    orig, masked, pasted, reco = (got[:, k] for k in range(4))
    assert np.array_equal(pasted, np.where(rem, reco, orig))
    assert np.array_equal(masked, np.where(rem, np.uint8(93), orig))
    for k, panel in enumerate(PANELS):                     # one panel alone is that panel among four
        alone = run(name, norm_pix, panels=(panel,), fill=93)
        assert alone.shape == (B, 1, S, S, 3) and np.array_equal(alone[:, 0], got[:, k]), panel
    swapped = run(name, norm_pix, panels=("reconstruction", "original", "reconstruction"), fill=93)
    assert np.array_equal(swapped[:, 0], reco) and np.array_equal(swapped[:, 1], orig) and np.array_equal(swapped[:, 2], reco)


@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm_pix"])
@pytest.mark.parametrize("value", [0.0, 1.0], ids=["nothing_removed", "all_removed"])
def test_uniform_masks(value, norm_pix):
    name = "t2_frame1"
    mask = torch.full_like(inputs(name, norm_pix)[2], value)
    got = run(name, norm_pix, mask=mask, fill=200)
    ref, before = want(name, norm_pix, mask=mask, fill=200)
    compare(got, ref, before, norm_pix, f"mask={value}")
    assert np.array_equal(got[:, 2], got[:, 3] if value else got[:, 0])
    if value:
        assert (got[:, 1] == 200).all()
    else:
        assert np.array_equal(got[:, 1], got[:, 0])


@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm_pix"])
def test_masked_mean_of_patch_mse_is_the_models_loss(norm_pix):
    """a small real model: `sum(mask * PATCH_MSE) / sum(mask)` is the loss its forward returned"""
    torch.manual_seed(11)
    model = MaskedAutoencoderViT(img_size=32, patch_size=8, num_frames=1, tubelet_size=1, in_chans=3, embed_dim=32, depth=2, num_heads=2,
                                 decoder_embed_dim=16, decoder_depth=1, decoder_num_heads=2, norm_pix_loss=norm_pix).to(DEV)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 3, 1, 32, 32, generator=g).to(DEV)
    model.masking_noise = torch.rand(2, model.spec.num_patches, generator=g)
    with torch.no_grad():
        loss, pred, mask = model(x, mask_ratio=0.75)
    norm = torch.tensor([[900.0, 800.0, 700.0], [1 / 300.0, 1 / 250.0, 1 / 200.0]], device=DEV)
    bounds = torch.tensor([[300.0, 1500.0], [200.0, 1400.0]], dtype=torch.float64, device=DEV)
    pics, mse = render.mae_panels(model, x, pred, mask, norm, bounds, patch_mse=True)
    torch.cuda.synchronize()
    m = mask.double().cpu()
    assert 0 < m.sum() < m.numel()
    got = float((m * mse.double().cpu()).sum() / m.sum())
    print(f"norm_pix={int(norm_pix)}: loss {loss.item():.8f}, masked mean of PATCH_MSE {got:.8f}")
    assert abs(got - loss.item()) < 2e-5 * abs(loss.item())
    ref, before = R.panels(x.cpu().numpy(), pred.cpu().numpy(), mask.cpu().numpy(), norm.cpu().numpy(), bounds.cpu().numpy(), 8, 1,
                           norm_pix=norm_pix)
    compare(pics.cpu().numpy(), ref, before, norm_pix, "model")


# ---- with the pipeline ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pipe_tiles():
    rng = np.random.default_rng(21)
    raw = np.where(rng.random((4, 3, 64, 64)) < 0.2, 0, rng.integers(1, 4001, (4, 3, 64, 64))).astype(np.int16)
    return torch.from_numpy(raw)


def _pipe():
    pipe = GpuTilePipeline([3.0, 4.0, 5.0], [2.0, 3.0, 1.5], random_crop_size=32, device=DEV)
    pipe.load(pipe_tiles(), None)
    return pipe


def _params(pipe):
    par = pipe.draw_params([2, 0, 2, 3, 1], training=False)
    par[:, 1], par[:, 2], par[:, 3] = torch.tensor([0, 32, 7, 19, 32]), torch.tensor([32, 0, 5, 11, 24]), torch.tensor([0, 1, 2, 3, 1])
    return par


def test_stretch_bounds_are_the_per_tile_percentiles():
    pipe = _pipe()
    par = _params(pipe)
    for bands, p in (((2, 1, 0), 98.0), ((0, 2, 1), 99.5)):
        got = pipe.stretch_bounds(par, bands=bands, percentile=p)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (5, 2)
        ref = pipe.band_percentiles([100.0 - p, p], indices=par[:, 0].tolist(), bands=bands, pooled=False)
        assert torch.equal(got.cpu(), ref)
        assert np.array_equal(got.cpu().numpy(), QR.percentiles(QR.groups(pipe_tiles().numpy(), par[:, 0].tolist(), bands, False), [100.0 - p, p]))


def test_original_panel_beside_the_quicklook_of_the_same_crop():
    pipe, raw = _pipe(), pipe_tiles().numpy()
    par = _params(pipe)
    x = pipe(params=par).x
    assert tuple(x.shape) == (5, 3, 1, 32, 32)
    model = model_for(3, 1, 1, 32, 8, False)
    s = model.spec
    pred, mask = torch.zeros(5, s.num_patches, s.patch_dim, device=DEV), torch.zeros(5, s.num_patches, device=DEV)
    bounds = pipe.stretch_bounds(par)
    got = render.mae_panels(model, x, pred, mask, pipe.norm, bounds, panels=("original",))[:, 0].cpu().numpy()
    look = pipe.quicklook(params=par).cpu().numpy()
    assert np.array_equal(look, QR.quicklook(raw, par.numpy(), (2, 1, 0), 98.0, 32, 32))
    diff = got.astype(np.int16) - look.astype(np.int16)
    m255 = pipe.norm[0].cpu().numpy().astype(np.float64)
    used = 0
    for b in range(5):
        crop = QR.crop(raw, par[b].numpy(), (2, 1, 0), 32, 32).astype(np.float64)               # [32, 32, 3], h w rgb
        lo, hi = (float(v) for v in bounds[b].cpu())
        assert hi > lo
        before = np.clip((crop - lo) / (hi - lo) * 255.0, 0.0, 255.0)
        delta = 4.0 * float(np.spacing(np.float32(np.abs(crop - m255[[2, 1, 0]]).max()))) * 255.0 / (hi - lo)
        near = np.abs(before - np.round(before)) < delta
        assert np.abs(diff[b]).max() <= 1 and not (diff[b] != 0)[~near].any(), (b, delta)
        used += int((diff[b] != 0).sum())
    print(f"original panel against the quicklook: {used} of {diff.size} bytes differ by one level")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_sizes_beyond_the_launch_bounds_are_refused_and_launch_nothing():
    imgs, pred, mask = torch.zeros(1, 3, 1, 16, 16, device=DEV), torch.zeros(1, 1, 768, device=DEV), torch.zeros(1, 1, device=DEV)
    norm, bounds = torch.ones(2, 3, device=DEV), torch.tensor([[0.0, 1.0]], dtype=torch.float64, device=DEV)
    out, mse = torch.full((1, 1, 16, 16, 3), 7, dtype=torch.uint8, device=DEV), torch.full((1, 1), 7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for dims in ((65536, 3, 1, 16, 16, 16, 1), (1, 3, 1, 65536, 65536, 16, 1), (1, 3, 65536, 16, 16, 16, 1)):
        rc = _lib.mae_panels(imgs, pred, mask, norm, bounds, out, mse, dims, (2, 1, 0), 0, (0,), 128, 0, stream)
        assert rc == -22 and "mae_panels: bad dims" in _lib.lib().s2k_last_error().decode()
        with pytest.raises(_lib.S2kError, match="bad dims"):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert (out == 7).all() and (mse == 7.0).all()
