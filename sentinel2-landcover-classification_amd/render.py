"""Class maps over pictures, on the GPU: the overlay half of the reference's `_log_segmentation_pred`
(src/train_segmentation.py:166-219), which draws the predicted and the true class mask over the stretched tile with wandb on the host.

    picture = pipe.quicklook(params=par)                              # uint8 [B, S, S, 3], data/gpu_pipeline.py
    shown   = render.overlay(picture, class_mask(logits), palette)    # uint8 [B, S, S, 3], still on the device

One stage, CLASS_OVERLAY (plan/opdefs.py, csrc/quicklook.hip), in integers: `(base*(256 - a) + colour*a + 128) >> 8` per channel with
a = round(alpha * 256).  The palette is the caller's: uint8 [K, 3], one colour per class.  Class maps come from `TilePredictor.predict`,
`losses.class_mask` or the pipeline's `y`.

MAE reconstructions, the picture the reference's MAE trainer logs every validation epoch (src/train_mae_prithvi.py:169-203: the
reconstruction beside the original; the masked input and the pasted reconstruction are a TODO there):

    par = pipe.draw_params(idx, training=False);  x = pipe(params=par).x          # [B, C, 1, S, S]
    loss, pred, mask = mae(x)
    pics = render.mae_panels(mae, x, pred, mask, pipe.norm, pipe.stretch_bounds(par))      # uint8 [B, 4, S, S, 3]

One launch of `s2k_mae_panels` (include/s2k.h, csrc/mae_render.hip) draws every panel: the values are de-normalised with the
pipeline's own mean / std and stretched between the bounds `pipe.quicklook(params=par)` uses for the same crop, so the panels and the
quicklook are comparable pixel for pixel.  What wandb then does to a float image handed to it is third party and not reproduced."""
from __future__ import annotations

import torch

from . import _lib
from .data import quicklook as QL
from .stage_call import StageCall


@torch.no_grad()
def overlay(base, classes: torch.Tensor, palette, alpha: float = 0.5, skip_zero: bool = False) -> torch.Tensor:
    """uint8 [B, SH, SW, 3] on the device: `palette[classes]` blended over `base` (uint8 [B, SH, SW, 3]; None = black) with opacity
    `alpha` in [0, 1].  A pixel whose class lies outside [0, K) - and, with skip_zero, a pixel of class 0 (the "other" / outside
    class of the label maps) - keeps `base` unchanged.  `classes` int64 [B, SH, SW]."""
    pal = QL.check_palette(palette)
    a = QL.alpha_code(alpha)
    if not isinstance(classes, torch.Tensor) or classes.dtype != torch.int64 or classes.dim() != 3 or classes.numel() == 0:
        raise ValueError("classes must be an int64 tensor [B, SH, SW]")
    B, SH, SW = (int(v) for v in classes.shape)
    if base is not None and (not isinstance(base, torch.Tensor) or base.dtype != torch.uint8 or tuple(base.shape) != (B, SH, SW, 3)
                             or base.device != classes.device):
        raise ValueError("base must be a uint8 tensor [B, SH, SW, 3] on the device of classes")
    if not classes.is_cuda:
        raise RuntimeError("render.overlay runs on the GPU (there is no CPU fallback)")
    dev, K = classes.device, int(pal.shape[0])
    classes = classes.contiguous()
    out = torch.empty(B, SH, SW, 3, dtype=torch.uint8, device=dev)
    call = StageCall()
    call.add("CLASS_OVERLAY", CLS=call.t(classes), PALETTE=call.t(pal.to(dev)), BASE=call.t(None if base is None else base.contiguous()),
             OUT=call.t(out), B=B, SH=SH, SW=SW, K=K, ALPHA=a, SKIP0=int(bool(skip_zero)))
    call.run()
    return out


def _dense(name: str, t, shape, dev, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or (dev is not None and t.device != dev):
        raise ValueError(f"{name} must be a {str(dtype).replace('torch.', '')} tensor {list(shape)} on the device of imgs")
    return t.detach().contiguous()


@torch.no_grad()
def mae_panels(model, imgs, pred, mask, norm, bounds, panels=("original", "masked", "pasted", "reconstruction"), bands=(2, 1, 0),
               frame: int = 0, fill: int = 128, patch_mse: bool = False):
    """uint8 [B, len(panels), H, W, 3] (h w rgb) on the device: pictures of what the masked autoencoder `model` made of `imgs`
    [B, C, T, H, W], from `pred` [B, L, PD] and `mask` [B, L] (non-zero = removed) as `model(imgs)` returned them.  Panels, in the
    order asked for (one to four): "original" = imgs; "masked" = imgs with the removed patches in the grey level `fill`;
    "pasted" = pred in the removed patches, imgs in the visible ones; "reconstruction" = pred everywhere.  `bands` are the three
    channels shown as r, g, b and `frame` the time step - the defaults are the reference's `[:3, 0][[2, 1, 0]]`.

    Every value is taken back to raw units with `norm` (float32 [2, C], `GpuTilePipeline.norm`: mean * 255 and 1 / (std * 255)) and
    stretched between `bounds` (float64 [B, 2], `GpuTilePipeline.stretch_bounds`) exactly as the quicklook stretches, in float64.
    A model with `norm_pix_loss` predicts standardised patches: pred is scaled back with each patch's own mean and unbiased variance.
    patch_mse=True: also float32 [B, L], the mean squared error of every patch against its target (standardised under
    norm_pix_loss); `(mask * patch_mse).sum() / mask.sum()` is the loss the model returned."""
    from .modules.prithvi import MaskedAutoencoderViT

    if not isinstance(model, MaskedAutoencoderViT):
        raise ValueError("model must be a MaskedAutoencoderViT (its spec gives the patch geometry)")
    s = model.spec
    C, T, S, P, TUB = s.in_chans, s.num_frames, s.img_size, s.patch_size, s.tubelet_size
    if not isinstance(imgs, torch.Tensor) or imgs.dim() != 5 or imgs.shape[0] < 1:
        raise ValueError(f"imgs must be a float32 tensor [B, {C}, {T}, {S}, {S}]")
    B, dev = int(imgs.shape[0]), imgs.device
    imgs = _dense("imgs", imgs, (B, C, T, S, S), None)
    pred = _dense("pred", pred, (B, s.num_patches, s.patch_dim), dev)
    mask = _dense("mask", mask, (B, s.num_patches), dev)
    norm = _dense("norm", norm, (2, C), dev)
    bounds = _dense("bounds", bounds, (B, 2), dev, torch.float64)
    names = [panels] if isinstance(panels, str) else list(panels)
    if not 1 <= len(names) <= 4 or any(n not in _lib.MAE_PANELS for n in names):
        raise ValueError(f"panels must be one to four of {sorted(_lib.MAE_PANELS)}")
    bl = QL.check_bands(bands, C, count=3)
    if isinstance(frame, bool) or not isinstance(frame, int) or not 0 <= frame < T:
        raise ValueError(f"frame must be an integer in [0, {T})")
    if isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill <= 255:
        raise ValueError("fill must be an integer grey level in 0..255")
    if not imgs.is_cuda:
        raise RuntimeError("render.mae_panels runs on the GPU (there is no CPU fallback)")
    out = torch.empty(B, len(names), S, S, 3, dtype=torch.uint8, device=dev)
    mse = torch.empty(B, s.num_patches, dtype=torch.float32, device=dev) if patch_mse else None
    with torch.cuda.device(dev):
        _lib.check(_lib.mae_panels(imgs, pred, mask, norm, bounds, out, mse, (B, C, T, S, S, P, TUB), bl, frame,
                                   [_lib.MAE_PANELS[n] for n in names], fill, bool(s.norm_pix_loss), torch.cuda.current_stream(dev).cuda_stream))
    return (out, mse) if patch_mse else out
