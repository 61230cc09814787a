"""Which stages of an f32-SPLIT plan carry FLAG_SPLIT: the shape lists of launch_conv_split (csrc/conv_bf16.hip) and
launch_wgrad_split (csrc/wgrad_bf16.hip), restated for the planner, and the measured routing rule on top of them.

A flagged stage splits each f32 MFMA operand into three bf16 terms (x = hi + mid + lo, all 24 significand bits) and issues the six
significant cross products as bf16 MFMAs into its f32 accumulator: f32-accurate (the dropped terms are a few 2^-24 relative per
product, the order of f32's own rounding).  Unlike FLAG_BF16 there is no fall-back: a flagged stage runs on the split kernels or
fails the step with S2K_EINVAL, so these lists must accept exactly what the launchers take, their LDS and 32-bit offset guards
included.  Every stage that is not flagged computes on the f32 kernels exactly as in an "f32" plan.

Routing (ROUTE): a shape class is flagged only where the split kernel measured faster than the f32 kernel its launcher picks
today (tools/exp_split_mfma.py, profiles/split_mfma.md).  The method-path / encoder-only planners do not implement the mode."""
from __future__ import annotations

from . import opdefs as D

_PIX_PRO = (D.PRO_NONE, D.PRO_AFFINE, D.PRO_SILU, D.PRO_RELU)
_WG_PRO = (D.PRO_NONE, D.PRO_RELU, D.PRO_SILU, D.PRO_AFFINE, D.PRO_GELU)
_LDS = 160 * 1024
_W3 = {16: (8, 16), 32: (4, 32), 56: (2, 56), 28: (4, 28), 14: (8, 14), 112: (2, 56), 224: (2, 56)}

# shape class -> flagged?  (the classes of shape_class()).  Measured on the U-Net b5 training step, 13 x 256 x 256, bs 32, every stage
# of a class on the split kernels against the kernel the f32 plan runs (tools/exp_split_mfma.py -> profiles/split_mfma.md, ms summed
# over the step's stages of the class):
#   conv3x3       24 stages   f32 7.335   split 5.739   0.78   the MFMA-bound decoder convs: the f32 MFMA rate was the bound
#   convt          5          0.615       0.496         0.81
#   wgrad3x3      15          4.508       4.224         0.94
#   conv1x1       89          3.694       3.941         1.07   HBM-bound; the producer / consumer and LDS-DMA f32 kernels stream
#   conv1x1_gate  39          1.917       1.963         1.02   their operands better than the split kernels' three LDS planes
#   wgrad1x1      83          4.911       5.069         1.03   (quad-read f32 kernel)
# The 1x1 classes lose and stay exact f32.
ROUTE = {
    "conv1x1": False,
    "conv1x1_gate": False,
    "conv3x3": True,
    "convt": True,
    "wgrad1x1": False,
    "wgrad3x3": True,
}


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _conv_lds(f: dict, pix: bool, kch: int, bm: int, used: int) -> int:
    taps = 1 if pix else 9
    img = (kch // 8) * (taps * bm + used) * 16 * 3
    tab = 2 * _cdiv(f["C1"] + f["C2"], kch) * kch * 4 if f["PRO1"] != D.PRO_NONE else 0
    return img + tab


def _bm(M: int) -> int:
    return 128 if M > 64 and _cdiv(M, 128) * 128 / M <= 1.12 else 64


def conv_ok(f: dict) -> bool:
    """CONV record `f` (planner fields) is one of launch_conv_split's shapes (f32 operands: no X1_BF16)."""
    if f.get("X1_BF16", 0) or f["STRIDE"] != 1 or f["HO"] != f["H"] or f["WO"] != f["W"]:
        return False
    T = f["KH"] * f["KW"]
    hw = f["H"] * f["W"]
    gate = f.get("GATE1") is not None
    ctot = f["C1"] + f["C2"]
    if f["MODE"] == D.MODE_CONVT_SCATTER:
        if not (T == 1 and f["C2"] == 0 and hw % 4 == 0 and not gate and f["M"] > 32 and f["M"] % 4 == 0
                and f["PRO1"] in (D.PRO_RELU, D.PRO_SILU)):
            return False
        return _conv_lds(f, True, 32, _bm(f["M"]), 128) <= _LDS
    if f["MODE"] != D.MODE_CONV:
        return False
    if T == 1:
        if f["C2"] != 0 or hw % 4 or f["PAD_T"] or f["PAD_L"]:
            return False
        if not (f["PRO1"] == D.PRO_SILU if gate else f["PRO1"] in _PIX_PRO):
            return False
        n = f["B"] * hw
        deep = ctot >= 512 and f["M"] > 32 and _cdiv(n, 128) * _cdiv(f["M"], 128) <= 1024 and (gate or f["PRO1"] == D.PRO_NONE)
        kch = 64 if deep else 32
        if f["M"] <= 32:
            bm, bn = 32, 256
        elif _cdiv(n, 128) * _cdiv(f["M"], 128) < 200:
            bm, bn = 64, 64
        else:
            bm, bn = _bm(f["M"]), 128
        return _conv_lds(f, True, kch, bm, bn) <= _LDS
    if T != 9 or f["KH"] != 3 or f["PAD_T"] != 1 or f["PAD_L"] != 1 or gate or f["PRO1"] not in (D.PRO_NONE, D.PRO_RELU):
        return False
    if f["C2"] > 0 and (f["PRO2"] != f["PRO1"] or f["C1"] % 16):
        return False
    wo = f["WO"]
    if f["M"] <= 32:
        if not (wo >= 64 and wo % 64 == 0):
            return False
        return _conv_lds(f, False, 16, 32, 6 * 66) <= _LDS
    if wo >= 64 and wo % 64 == 0:
        r, xw = 2, 64
    elif wo in _W3:
        r, xw = _W3[wo]
    else:
        return False
    return _conv_lds(f, False, 16, _bm(f["M"]), (r + 2) * (xw + 2)) <= _LDS


def wgrad_ok(f: dict) -> bool:
    """WGRAD record `f` is one of launch_wgrad_split's shapes (f32 operands: no P_BF16)."""
    if f.get("P_BF16", 0) or f["MODE"] != D.MODE_CONV or f["STRIDE"] != 1 or f["H"] != f["HO"] or f["W"] != f["WO"] \
            or f.get("GATEP") is not None or f["PROP"] not in _WG_PRO or f["PROQ"] not in _WG_PRO:
        return False
    T = f["KH"] * f["KW"]
    hw = f["HO"] * f["WO"]
    if T == 1:
        if hw % 8 or f["B"] * hw < 512:
            return False
        npj = 64      # (the smallest pixel tile of the 1x1 kernels: the widest span of images)
        span = 1 if hw % npj == 0 else min(f["B"], (npj - 2) // hw + 2)
    else:
        if T != 9 or f["KH"] != 3 or f["PAD_T"] != 1 or f["PAD_L"] != 1 or f.get("GATEQ") is not None or f["PROP"] != D.PRO_NONE:
            return False
        if not (f["WO"] % 64 == 0 or f["WO"] in (32, 16)):
            return False
        span = 1
    return max(f["M"] * hw, f["C"] * f["H"] * f["W"]) * 4 * span < 0x7ffffff0


def wants_pixel_octets() -> bool:
    """Token rows of the ViT plans padded to 8 floats (as for bf16-mixed) only while the split 1x1 weight gradient - which contracts
    pixel octets - is routed: the padding costs the MAE step 2 % (1512 against 1541 samples/s at bs 64) and buys nothing when no
    Linear runs split."""
    return ROUTE["wgrad1x1"]


def shape_class(kind: str, f: dict) -> str:
    if kind == "WGRAD":
        return "wgrad1x1" if f["KH"] * f["KW"] == 1 else "wgrad3x3"
    if f["MODE"] == D.MODE_CONVT_SCATTER:
        return "convt"
    if f["KH"] * f["KW"] == 1:
        return "conv1x1_gate" if f.get("GATE1") is not None else "conv1x1"
    return "conv3x3"


def routed(kind: str, f: dict) -> bool:
    """the stage is one of the split kernels' shapes AND its class is routed to them"""
    ok = conv_ok(f) if kind == "CONV" else wgrad_ok(f)
    return ok and ROUTE[shape_class(kind, f)]
