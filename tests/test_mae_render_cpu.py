"""CPU: `s2k_mae_panels` is exported (and the stage table and the ABI version did not move), it validates every argument on the host
before anything is launched, the numpy restatement (tests/mae_render_ref.py) agrees with the model's own `unpatchify` / loss formula
in torch, and `render.mae_panels` / `GpuTilePipeline.stretch_bounds` raise ValueError for bad arguments before they refuse to run off
the GPU.  The entry is never called with valid arguments here: there is no device to launch on."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import _lib, render
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.modules.prithvi import MaskedAutoencoderViT
from s2lc_amd.plan import opdefs as D
from tests import mae_render_ref as R

ROOT = Path(__file__).resolve().parents[1]
S2K_EINVAL, S2K_EFAULT = -22, -14


def test_entry_is_exported_and_the_stage_table_is_unchanged():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g

    g.build()
    L = _lib.lib()
    assert hasattr(ctypes.CDLL(str(g.LIB)), "s2k_mae_panels")
    assert L.s2k_abi_version() == 2 and len(D.OPS) == 55
    assert "mae_render.hip" in g.SOURCES
    hdr = (ROOT / "include" / "s2k.h").read_text()
    assert re.search(r"\bint s2k_mae_panels\s*\(", hdr) and "#define S2K_ABI_VERSION 2" in hdr
    assert _lib.MAE_PANELS == R.CODES


# a valid call over CPU tensors (never made): B, C, T, H, W, P, TUB = 2, 4, 2, 16, 16, 4, 2  ->  g = 4, L = 16, PD = 128
GOOD = dict(B=2, C=4, T=2, H=16, W=16, P=4, TUB=2, bands=(2, 1, 0), frame=1, panels=(0, 1, 2, 3), fill=128, norm_pix=1)
POINTERS = ("imgs", "pred", "mask", "norm", "bounds", "out")


def _call(**change):
    a = {**GOOD, **change}
    t = dict(imgs=torch.zeros(2, 4, 2, 16, 16), pred=torch.zeros(2, 16, 128), mask=torch.zeros(2, 16), norm=torch.ones(2, 4),
             bounds=torch.zeros(2, 2, dtype=torch.float64), out=torch.zeros(2, 4, 16, 16, 3, dtype=torch.uint8), patch_mse=torch.zeros(2, 16))
    t.update({k: a[k] for k in POINTERS + ("patch_mse",) if k in a})
    rc = _lib.mae_panels(t["imgs"], t["pred"], t["mask"], t["norm"], t["bounds"], t["out"], t["patch_mse"],
                         (a["B"], a["C"], a["T"], a["H"], a["W"], a["P"], a["TUB"]), a["bands"], a["frame"], a["panels"], a["fill"],
                         a["norm_pix"], 0)
    return rc, _lib.lib().s2k_last_error().decode()


BAD = [
    # every dimension positive
    dict(B=0), dict(B=-1), dict(C=0), dict(C=-4), dict(T=0), dict(T=-2), dict(H=0, W=0), dict(H=-16, W=-16), dict(W=0), dict(P=0), dict(P=-4),
    dict(TUB=0), dict(TUB=-1),
    # H == W, P | H, TUB | T
    dict(H=16, W=20), dict(H=20, W=16), dict(P=5), dict(P=32), dict(T=3, TUB=2), dict(T=2, TUB=4),
    # the unbiased variance needs two features
    dict(C=1, T=1, TUB=1, P=1, frame=0, norm_pix=1),
    # bands: distinct, inside [0, C)
    dict(bands=(2, 2, 0)), dict(bands=(0, 1, 0)), dict(bands=(1, 3, 3)), dict(bands=(4, 1, 0)), dict(bands=(2, -1, 0)), dict(bands=(0, 1, 99)),
    # frame, fill, panels, norm_pix
    dict(frame=2), dict(frame=-1), dict(fill=256), dict(fill=-1), dict(panels=(0, 4)), dict(panels=(-1,)), dict(panels=()),
    dict(panels=(0, 1, 2, 3, 0)), dict(norm_pix=2), dict(norm_pix=-1),
    # the launch grid and the 32-bit offsets inside a sample
    dict(B=65536), dict(T=65536, TUB=1, H=4, W=4), dict(H=32768, W=32768), dict(C=3, T=1, TUB=1, frame=0, H=16384, W=16384),
]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_entry_rejects_invalid_arguments_on_the_host(bad):
    rc, msg = _call(**bad)
    assert rc == S2K_EINVAL and msg.startswith("mae_panels: ") and len(msg) > 20, (rc, msg)


@pytest.mark.parametrize("name", POINTERS + ("bands", "panels"))
def test_entry_rejects_a_null_required_pointer(name):
    rc, msg = _call(**{name: None})
    assert rc == S2K_EFAULT and msg.startswith("mae_panels: null pointer"), (rc, msg)
    with pytest.raises(_lib.S2kError, match="null pointer"):
        _lib.check(rc)


# ---- the restatement against the model's own expressions ------------------------------------------------------------------------------
def _model(C, T, TUB, S, P, norm_pix):
    return MaskedAutoencoderViT(img_size=S, patch_size=P, num_frames=T, tubelet_size=TUB, in_chans=C, embed_dim=16, depth=1, num_heads=2,
                                decoder_embed_dim=16, decoder_depth=1, decoder_num_heads=2, norm_pix_loss=norm_pix)


@pytest.mark.parametrize("norm_pix", [False, True])
@pytest.mark.parametrize("geom", [(2, 3, 1, 1, 16, 8), (2, 5, 4, 2, 12, 4)], ids=["c3", "c5_t4_tub2"])
def test_restatement_is_unpatchify_and_the_loss_formula(geom, norm_pix):
    B, C, T, TUB, S, P = geom
    model = _model(C, T, TUB, S, P, norm_pix)
    g = torch.Generator().manual_seed(C)
    imgs = torch.randn(B, C, T, S, S, generator=g)
    pred = torch.randn(B, model.spec.num_patches, model.spec.patch_dim, generator=g)
    mask = (torch.rand(B, model.spec.num_patches, generator=g) < 0.6).float()
    assert 0 < mask.sum() < mask.numel()
    norm = torch.stack([torch.rand(C, generator=g) * 100 + 50, 1.0 / (torch.rand(C, generator=g) * 50 + 20)])
    bands, frame = (C - 1, 0, 1), T - 1
    # bounds so wide that nothing clips: |v| stays far below 1e4 here
    bounds = torch.tensor([[-1.0e4, 1.0e4], [-2.0e4, 3.0e4]], dtype=torch.float64)
    assert torch.equal(torch.from_numpy(R.patchify(imgs.numpy(), P, TUB)), model.patchify(imgs))
    assert torch.equal(torch.from_numpy(R.unpatchify(pred.numpy(), C, T, S, P, TUB)), model.unpatchify(pred))

    # the reference's loss (prithvi.py:333-350) in float64
    target = model.patchify(imgs).double()
    if norm_pix:
        mean, var = target.mean(dim=-1, keepdim=True), target.var(dim=-1, keepdim=True)
        target = (target - mean) / (var + 1.0e-6) ** 0.5
    per_patch = ((pred.double() - target) ** 2).mean(dim=-1)
    got_mse = R.patch_mse(imgs.numpy(), pred.numpy(), P, TUB, norm_pix)
    assert np.allclose(got_mse, per_patch.numpy(), rtol=1e-12, atol=0)
    loss = (per_patch * mask.double()).sum() / mask.double().sum()
    assert abs((got_mse * mask.numpy()).sum() / mask.numpy().sum() - loss.item()) < 1e-12 * loss.item()

    # the reference's picture: unpatchify(pred)[:, bands, frame], de-normalised and stretched
    full = pred.double()
    if norm_pix:
        full = full * (var + 1.0e-6) ** 0.5 + mean
    x = model.unpatchify(full)[:, list(bands), frame]                       # [B, 3, S, S]
    v = x / norm[1].double()[list(bands)].view(1, 3, 1, 1) + norm[0].double()[list(bands)].view(1, 3, 1, 1)
    lo, hi = bounds[:, 0].view(B, 1, 1, 1), bounds[:, 1].view(B, 1, 1, 1)
    want = ((v - lo) / (hi - lo) * 255.0).permute(0, 2, 3, 1)
    assert 0.0 < want.min() and want.max() < 255.0
    out, before = R.panels(imgs.numpy(), pred.numpy(), mask.numpy(), norm.numpy(), bounds.numpy(), P, TUB, bands, frame,
                           (R.RECONSTRUCTION, R.ORIGINAL, R.MASKED, R.PASTED), 77, norm_pix)
    assert np.allclose(before[:, 0], want.numpy(), rtol=1e-12, atol=1e-9)
    near = np.abs(want.numpy() - np.round(want.numpy())) < 1e-6
    assert np.array_equal(out[:, 0][~near], want.numpy().astype(np.uint8)[~near])
    # the other panels are the original and the reconstruction chosen patch by patch
    t0, gsz = frame // TUB, S // P
    rem = (mask[:, t0 * gsz * gsz:(t0 + 1) * gsz * gsz].reshape(B, gsz, gsz) != 0).repeat_interleave(P, 1).repeat_interleave(P, 2).numpy()
    assert rem.any() and not rem.all()
    assert np.array_equal(out[:, 2][rem], np.full((int(rem.sum()), 3), 77, np.uint8)) and np.array_equal(out[:, 2][~rem], out[:, 1][~rem])
    assert np.array_equal(out[:, 3][rem], out[:, 0][rem]) and np.array_equal(out[:, 3][~rem], out[:, 1][~rem])


def test_restatement_edge_cases_are_explicit():
    imgs = np.zeros((4, 3, 1, 4, 4), np.float32)
    imgs[0, :, 0, 0, :4] = [np.nan, np.inf, -np.inf, 5.0]
    pred = R.patchify(imgs, 2, 1).copy()
    norm = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], np.float32)
    bounds = np.array([[0.0, 10.0], [3.0, 3.0], [np.nan, 1.0], [5.0, np.inf]])
    out, _ = R.panels(imgs, pred, np.zeros((4, 4), np.float32), norm, bounds, 2, 1, codes=(R.ORIGINAL,))
    assert out[0, 0, 0, :, 0].tolist() == [0, 255, 0, 127] and not out[1:].any()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def _cpu_pipe():
    p = GpuTilePipeline([0.1] * 4, [0.2] * 4, random_crop_size=8, device="cpu")
    g = torch.Generator().manual_seed(0)
    p.load(torch.randint(-100, 100, (3, 4, 16, 16), generator=g, dtype=torch.int32).to(torch.int16), None)
    return p


def _surface():
    model = _model(4, 2, 1, 8, 4, False)
    s = model.spec
    return model, dict(imgs=torch.zeros(2, 4, 2, 8, 8), pred=torch.zeros(2, s.num_patches, s.patch_dim), mask=torch.zeros(2, s.num_patches),
                       norm=torch.ones(2, 4), bounds=torch.zeros(2, 2, dtype=torch.float64))


def test_validators_raise_before_the_gpu_refusal():
    model, t = _surface()
    p = _cpu_pipe()

    def mp(**kw):
        a = {**t, **{k: v for k, v in kw.items() if k in t}}
        rest = {k: v for k, v in kw.items() if k not in t and k != "model"}
        return lambda: render.mae_panels(kw.get("model", model), a["imgs"], a["pred"], a["mask"], a["norm"], a["bounds"], **rest)

    bad = [
        mp(model=torch.nn.Linear(2, 2)), mp(model=None),
        # shapes
        mp(imgs=torch.zeros(2, 4, 2, 8, 4)), mp(imgs=torch.zeros(2, 3, 2, 8, 8)), mp(imgs=torch.zeros(4, 2, 8, 8)), mp(imgs=torch.zeros(0, 4, 2, 8, 8)),
        mp(pred=torch.zeros(2, 8, 63)), mp(pred=torch.zeros(1, 8, 64)), mp(mask=torch.zeros(2, 7)), mp(mask=torch.zeros(2, 8, 1)),
        mp(norm=torch.ones(2, 3)), mp(norm=torch.ones(4)), mp(bounds=torch.zeros(2, 3, dtype=torch.float64)), mp(bounds=torch.zeros(1, 2, dtype=torch.float64)),
        # dtypes
        mp(imgs=torch.zeros(2, 4, 2, 8, 8, dtype=torch.float64)), mp(pred=torch.zeros(2, 8, 64, dtype=torch.float16)),
        mp(mask=torch.zeros(2, 8, dtype=torch.bool)), mp(norm=torch.ones(2, 4, dtype=torch.float64)), mp(bounds=torch.zeros(2, 2)),
        mp(imgs=np.zeros((2, 4, 2, 8, 8), np.float32)), mp(bounds=None),
        # devices: every tensor lives where imgs lives
        mp(pred=torch.zeros(2, 8, 64, device="meta")), mp(mask=torch.zeros(2, 8, device="meta")), mp(norm=torch.ones(2, 4, device="meta")),
        mp(bounds=torch.zeros(2, 2, dtype=torch.float64, device="meta")),
        # bands, frame, panels, fill
        mp(bands=(0, 1)), mp(bands=(0, 1, 1)), mp(bands=(0, 1, 4)), mp(bands=(-1, 1, 2)), mp(bands=5),
        mp(frame=2), mp(frame=-1), mp(frame=0.5), mp(frame=True),
        mp(panels=()), mp(panels=("original", "mask")), mp(panels="everything"), mp(panels=("original",) * 5), mp(panels=(0,)),
        mp(fill=256), mp(fill=-1), mp(fill=127.5),
        # stretch_bounds
        lambda: p.stretch_bounds(None), lambda: p.stretch_bounds([[0, 0, 0]]), lambda: p.stretch_bounds([[3, 0, 0, 0]]),
        lambda: p.stretch_bounds([[0, 9, 0, 0]]), lambda: p.stretch_bounds([[0, 0, 0, 4]]), lambda: p.stretch_bounds(torch.zeros(0, 4, dtype=torch.int32)),
        lambda: p.stretch_bounds([[0.5, 0, 0, 0]]), lambda: p.stretch_bounds([[0, 0, 0, 0]], bands=(0, 1)),
        lambda: p.stretch_bounds([[0, 0, 0, 0]], bands=(0, 1, 1)), lambda: p.stretch_bounds([[0, 0, 0, 0]], bands=(0, 1, 4)),
        lambda: p.stretch_bounds([[0, 0, 0, 0]], percentile=50.0), lambda: p.stretch_bounds([[0, 0, 0, 0]], percentile=100.5),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} did not raise")


def test_the_new_methods_refuse_the_cpu():
    model, t = _surface()
    p = _cpu_pipe()
    calls = (lambda: render.mae_panels(model, **t), lambda: render.mae_panels(model, **t, panels="pasted", bands=(3, 0, 1), frame=1, fill=0, patch_mse=True),
             lambda: p.stretch_bounds(p.draw_params([2, 0, 2], training=False)), lambda: p.stretch_bounds([[1, 8, 0, 3]], bands=(3, 0, 1), percentile=99.5))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
