"""Class maps over pictures, on the GPU: the overlay half of the reference's `_log_segmentation_pred`
(src/train_segmentation.py:166-219), which draws the predicted and the true class mask over the stretched tile with wandb on the host.

    picture = pipe.quicklook(params=par)                              # uint8 [B, S, S, 3], data/gpu_pipeline.py
    shown   = render.overlay(picture, class_mask(logits), palette)    # uint8 [B, S, S, 3], still on the device

One stage, CLASS_OVERLAY (plan/opdefs.py, csrc/quicklook.hip), in integers: `(base*(256 - a) + colour*a + 128) >> 8` per channel with
a = round(alpha * 256).  The palette is the caller's: uint8 [K, 3], one colour per class.  Class maps come from `TilePredictor.predict`,
`losses.class_mask` or the pipeline's `y`."""
from __future__ import annotations

import torch

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
