"""Which instantiation of conv_bf16_kernel (csrc/conv_bf16.hip) or wgrad_bf16_kernel (csrc/wgrad_bf16.hip) a FLAG_BF16 (bf16-mixed,
kernel family 2) or FLAG_SPLIT (f32-split, family 5) stage runs, restated in plain Python from conv_b16_route<SPLIT>, launch_b16_pix,
launch_b16_bm, launch_b16, launch_wgrad_bf16, launch_wgrad_split and launch_wb16 at their default tuning (S2K_B16_DEEP_MIN 512,
S2K_B16_SPLIT_MAX_BLOCKS 512, S2K_WB16_SLOTS 0).  Test infrastructure.

    conv(B=, C1=, H=, W=, M=, ..., flags=) -> Cv          wgrad(B=, M=, C=, H=, W=, ..., flags=) -> Wv

The keyword arguments are the record's fields (opdefs.OPS["CONV"] / ["WGRAD"]) that decide the routing; tensors are truth values.
`result` is the kernel family (2 or 5), "declined" (the launcher returns 1 and the f32 kernels take the stage) or "error" with a
fragment of the launcher's message.  Besides the exact template arguments a Cv / Wv holds the run-time facts a test row has to
reach: tile counts and ragged edges, images per pixel tile, the K tail, the split-K / pixel-split partition, the epilogue form, the
statistics reduction width, the LDS bytes, the 3x3 tiling.  tests/test_b16_dispatch_cpu.py parses every launch site and every constant
below out of the two .hip files and compares.

Parsed instantiations (tests/test_b16_dispatch_cpu.py::test_parse_finds_every_launch_site): conv_bf16_kernel 76 bf16-mixed + 58
f32-split launched (56 reachable: the thin tile with the deep 64-channel chunks needs M <= 32 and M > 32 at once), wgrad_bf16_kernel
28 + 12."""
from __future__ import annotations

from dataclasses import dataclass

BF16, SPLIT = 2, 5                    # kernel families (include/s2k.h)
FLAG_BF16, FLAG_SPLIT = 4, 64         # plan/opdefs.py
FLAG_OTHERS = 8 | 16 | 32             # FLAG_DMA, FLAG_Q4, FLAG_RES_GELU_GRAD: excluded by FLAG_SPLIT
PRO_NONE, PRO_AFFINE, PRO_SILU, PRO_RELU, PRO_GELU = 0, 1, 2, 3, 4
MODE_CONV, MODE_CONVT_SCATTER, MODE_GATHER2X2 = 0, 1, 2
BM_PIX, BM_SPATIAL = 0, 1
WG_PIX, WG_SPATIAL = 0, 1             # tags of the parsed template arguments (the enum values are not restated)

# ---- csrc/conv_bf16.hip -------------------------------------------------------------------------------------------------------------
DEEP_MIN = 512                        # S2K_B16_DEEP_MIN
SPLIT_MAX_BLOCKS = 512                # S2K_B16_SPLIT_MAX_BLOCKS
K1 = {False: 64, True: 32}            # channels per chunk of a 1x1 stage, by SPLIT
KDEEP = {False: 128, True: 64}        # ... of a deep reduction
K3 = 16                               # ... of a 3x3 stage
PIX_SMALL_TILES = 200                 # fewer 128 x 128 tiles than this: 64 x 64 tiles
DEEP_MAX_TILES = 1024                 # deep chunks only up to this many 128 x 128 tiles
BM_PAD = 1.12                         # 128-row tiles unless they pad M by more than 12 %
THIN_M = 32                           # M <= 32: the 32 x 256 tile
SPLITK_MIN_CHUNKS, SPLITK_TARGET, SPLITK_MAX, SPLITK_PER = 8, 1024, 8, 4       # splits = min(8, cdiv(1024, blocks), nchunks / 4)
LDS_MAX = 160 * 1024
SPAN_LIMIT = 0x7ffffff0
# (R, XW) by the map width, in the launcher's order
GEOMS_3X3 = (((2, 64), "mult64"), ((4, 32), (32,)), ((8, 16), (16,)), ((2, 56), (56, 112, 224)), ((4, 28), (28,)), ((8, 14), (14,)))
THIN_3X3 = (4, 64)
PIX_PRO = (PRO_NONE, PRO_RELU, PRO_SILU, PRO_AFFINE)

# ---- csrc/wgrad_bf16.hip ------------------------------------------------------------------------------------------------------------
W_SLOTS = {True: 512, False: 256}     # workgroup slots by PIX (S2K_WB16_SLOTS 0)
W_MIN_TILES_PER_SPLIT = 4
W_MIN_PIXELS = 512                    # 1x1: B * HWp >= 512
W_PRO = (PRO_NONE, PRO_RELU, PRO_SILU, PRO_AFFINE, PRO_GELU)
# (WVM, WVC, WM, WN, XW) of a 1x1 stage by (em, ec); 32 / 64 / 128 = edge()
W_PIX = {(32, 32): (1, 1, 1, 1, 256), (32, 64): (1, 2, 1, 1, 128), (32, 128): (1, 2, 1, 1, 128), (64, 32): (2, 1, 1, 1, 128), (128, 32): (2, 1, 1, 1, 128),
         (128, 128): (2, 2, 2, 2, 64), (128, 64): (2, 2, 2, 1, 64), (64, 128): (2, 2, 1, 2, 64), (64, 64): (2, 2, 1, 1, 64)}
# 3x3: (WVM, WVC, WM, WN, R, XW); "mult64" rows by (em == 32, ec == 32)
W_3X3_BF16 = {"mult64": {(True, True): (1, 1, 1, 1, 4, 64), (True, False): (1, 2, 1, 1, 4, 64), (False, True): (2, 1, 1, 1, 4, 64), (False, False): (2, 2, 1, 1, 4, 64)},
              "mult56": (2, 2, 1, 1, 2, 56), 32: (2, 2, 1, 1, 4, 32), 16: (2, 2, 1, 1, 8, 16)}
W_3X3_SPLIT = {"mult64": {(True, True): (1, 1, 1, 1, 4, 64), (True, False): (1, 2, 1, 1, 2, 64), (False, True): (2, 1, 1, 1, 2, 64), (False, False): (2, 2, 1, 1, 2, 32)},
               32: (2, 2, 1, 1, 2, 32), 16: (2, 2, 1, 1, 4, 16)}


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _images_per_tile(ntot: int, hw: int, bn: int) -> int:
    worst = 1
    for nt in range(cdiv(ntot, bn)):
        worst = max(worst, (min((nt + 1) * bn, ntot) - 1) // hw - (nt * bn) // hw + 1)
    return worst


@dataclass
class Cv:
    result: object                    # 2, 5, "declined" or "error"
    message: str = ""                 # "error": a fragment of the launcher's message
    kernel: str = "conv_bf16_kernel"
    args: tuple = ()                  # (BMODE, WVM, WM, WN, KCH, R, XW, PRO, GATE, SCATTER, X16, SPLIT)
    BM: int = 0
    BN: int = 0
    KCH: int = 0
    n_mtiles: int = 0
    n_ntiles: int = 0
    ragged_m: bool = False
    ragged_n: bool = False            # 1x1: the last pixel tile has pixels past Ntot
    images_per_tile: int = 1
    nchunks: int = 0
    k_tail: int = 0                   # Ctot % KCH
    k_lt_chunk: bool = False
    c_mod8: bool = False              # Ctot % 8 != 0: the last octet holds channels past Ctot
    tail_in_src2: bool = False
    upper_half_past_k: bool = False   # KCH 128: the upper half of the last chunk lies past the packed K (Ctot % 128 in 1..64)
    upper_half_in_k: bool = False     # ... does not (Ctot % 128 in 65..127)
    splits: int = 1
    chunks_per_split: int = 0
    split_cap8: bool = False          # cdiv(1024, blocks) asked for more than 8
    split_cap_quarter: bool = False   # nchunks / 4 binds
    short_last_split: bool = False
    could_split: bool = False         # would split, has no SCRATCH
    epilogue: str = ""                # "transposed", "scalar", "scatter"; with splits > 1 the partial tile goes to SCRATCH instead
    G: int = 0                        # transposed store: lanes that hold one row's sums (16 / 32 / 64)
    lds: int = 0
    R: int = 0
    XW: int = 0
    tiles_x: int = 0
    tiles_y: int = 0
    partial_row: bool = False
    nrep: int = 1
    deep: bool = False

    @property
    def family(self):
        return self.result

    @property
    def inst(self) -> tuple:
        return (self.kernel, self.args)

    @property
    def edges(self) -> frozenset:
        sp = self.XW > 0 and self.args and self.args[0] == BM_SPATIAL
        named = {
            "ragged last m-tile": self.ragged_m,
            "ragged last pixel tile": self.ragged_n,
            "pixel tile over 2 images": self.images_per_tile == 2,
            "pixel tile over >= 3 images": self.images_per_tile >= 3,
            "K tail": self.k_tail > 0 and not self.k_lt_chunk,
            "K < one chunk": self.k_lt_chunk,
            "Ctot % 8 != 0": self.c_mod8,
            "K tail in source 2": self.tail_in_src2,
            "upper half of the last 128-channel chunk past the packed K": self.upper_half_past_k,
            "upper half of the last 128-channel chunk inside the packed K": self.upper_half_in_k,
            "split-K": self.splits > 1,
            "no split-K": self.splits == 1,
            "split-K: unequal splits": self.short_last_split,
            "split-K: 8 splits": self.splits == 8,
            "split-K: nchunks / 4 cap": self.split_cap_quarter,
            "would split, has no SCRATCH": self.could_split,
            "transposed store": self.epilogue == "transposed" and self.splits == 1,
            "scalar store": self.epilogue == "scalar" and self.splits == 1,
            "scatter store": self.epilogue == "scatter",
            "partial last tile row": bool(sp) and self.partial_row,
            "several x tiles per row": bool(sp) and self.tiles_x > 1,
        }
        return frozenset(k for k, v in named.items() if v)


class _P:
    pass


def _declined():
    return Cv("declined")


def _launch_b16(p, split: bool, bmode, wvm, wm, wn, kch, r, xw, pro, gate, scatter, x16, n_ntiles) -> Cv:
    pix = bmode == BM_PIX
    wvn = 4 // wvm
    BM, BN = wvm * wm * 32, wvn * wn * 32
    TT = 1 if pix else 9
    NO = kch // 8
    used = BN if pix else (r + 2) * (xw + 2)
    img = (NO * TT * BM + NO * used) * 16 * (3 if split else 1)
    nchunks = cdiv(p.Ctot, kch)
    tepi = (not scatter) and (pix or xw % 4 == 0)
    ct_bytes = wvm * 32 * (BN + 8) * 4 if tepi else 0
    lds = max(img + (2 * nchunks * kch * 4 if pro != PRO_NONE else 0), ct_bytes)
    if lds > LDS_MAX:
        return Cv("error", "f32-split stage needs") if split else _declined()
    span = 1 if (not pix or p.HW % BN == 0) else min(p.B, (BN - 2) // p.HW + 2)
    if max(p.C1, p.C2) * p.H * p.W * 4 * span >= SPAN_LIMIT:
        return Cv("error", "exceed 2 GiB")
    n_mtiles = cdiv(p.M, BM)
    blocks = n_mtiles * n_ntiles
    if blocks <= 0 or blocks > 0x7fffffff:
        return Cv("error", "bad grid")

    def partition(scratch: bool):
        out = dict(splits=1, chunks_per_split=nchunks, split_cap8=False, split_cap_quarter=False, short_last_split=False)
        if pix and not scatter and scratch and blocks <= SPLIT_MAX_BLOCKS and nchunks >= SPLITK_MIN_CHUNKS:
            want = cdiv(SPLITK_TARGET, blocks)
            splits = min(SPLITK_MAX, want)
            quarter = nchunks // SPLITK_PER < splits
            splits = min(splits, nchunks // SPLITK_PER)
            if splits > 1:
                cps = cdiv(nchunks, splits)
                n = cdiv(nchunks, cps)
                out.update(splits=n, chunks_per_split=cps, split_cap8=want > SPLITK_MAX, split_cap_quarter=quarter, short_last_split=nchunks % cps != 0)
        return out
    f = partition(bool(p.SCRATCH))
    tail = p.Ctot % kch
    cv = Cv(SPLIT if split else BF16, "", "conv_bf16_kernel", (bmode, wvm, wm, wn, kch, r, xw, pro, gate, scatter, x16, split), BM=BM, BN=BN, KCH=kch,
            n_mtiles=n_mtiles, n_ntiles=n_ntiles, ragged_m=p.M % BM != 0, ragged_n=pix and p.Ntot % BN != 0,
            images_per_tile=_images_per_tile(p.Ntot, p.HW, BN) if pix else 1, nchunks=nchunks, k_tail=tail, k_lt_chunk=p.Ctot < kch,
            c_mod8=p.Ctot % 8 != 0, tail_in_src2=p.C2 > 0 and tail > 0, upper_half_past_k=kch == 128 and 1 <= p.Ctot % 128 <= 64,
            upper_half_in_k=kch == 128 and p.Ctot % 128 >= 65, could_split=(not p.SCRATCH) and partition(True)["splits"] > 1,
            epilogue="scatter" if scatter else ("transposed" if tepi else "scalar"), G=BN // 4 if tepi else 0, lds=lds, nrep=p.NREP, deep=kch == KDEEP[split], **f)
    if not pix:
        cv.R, cv.XW, cv.tiles_x, cv.tiles_y, cv.partial_row = r, xw, cdiv(p.WO, xw), cdiv(p.HO, r), p.HO % r != 0
    return cv


def _launch_b16_bm(p, split, bmode, kch, r, xw, pro, gate, scatter, x16, n128) -> Cv:
    if p.M <= THIN_M:
        return _declined()
    big = p.M > 64 and float(cdiv(p.M, 128) * 128) / p.M <= BM_PAD
    return _launch_b16(p, split, bmode, 2, 2 if big else 1, 2, kch, r, xw, pro, gate, scatter, x16, n128)


def _launch_b16_pix(p, split, kch, pro, gate, x16=False) -> Cv:
    if kch <= 64 and p.M <= THIN_M:
        return _launch_b16(p, split, BM_PIX, 1, 1, 2, kch, 1, 64, pro, gate, False, x16, cdiv(p.Ntot, 256))
    n128 = cdiv(p.Ntot, 128)
    if n128 * cdiv(p.M, 128) < PIX_SMALL_TILES:
        return _launch_b16(p, split, BM_PIX, 2, 1, 1, kch, 1, 64, pro, gate, False, x16, cdiv(p.Ntot, 64))
    return _launch_b16_bm(p, split, BM_PIX, kch, 1, 64, pro, gate, False, x16, n128)


def _route(p, split: bool) -> Cv:
    k1, kdeep = K1[split], KDEEP[split]
    if not p.WTB or p.S != 1 or p.HO != p.H or p.WO != p.W:
        return _declined()
    T = p.KH * p.KW
    if p.X16 and p.MODE != MODE_CONV:
        return _declined()
    if p.MODE == MODE_CONVT_SCATTER:
        if T != 1 or p.C2 != 0 or (p.HW & 3) or p.GATE or p.M <= 32 or (p.M & 3):
            return _declined()
        if p.PRO1 in (PRO_RELU, PRO_SILU):
            return _launch_b16_bm(p, split, BM_PIX, k1, 1, 64, p.PRO1, False, True, False, cdiv(p.Ntot, 128))
        return _declined()
    if p.MODE != MODE_CONV:
        return _declined()
    if T == 1:
        if p.C2 != 0 or (p.HW & 3) or p.PT or p.PL:
            return _declined()
        deep = p.Ctot >= DEEP_MIN and p.M > 32 and cdiv(p.Ntot, 128) * cdiv(p.M, 128) <= DEEP_MAX_TILES
        if not split and p.X16:
            if p.GATE or p.PRO1 != PRO_NONE or (p.HW & 7):
                return Cv("error", "X1_BF16 is for plain 1x1 stages")
            return _launch_b16_pix(p, split, 128 if deep else 64, PRO_NONE, False, True)
        if p.GATE:
            if p.PRO1 == PRO_SILU:
                return _launch_b16_pix(p, split, kdeep if deep else k1, PRO_SILU, True)
            return _declined()
        if p.PRO1 == PRO_NONE:
            return _launch_b16_pix(p, split, kdeep if deep else k1, PRO_NONE, False)
        if p.PRO1 in (PRO_RELU, PRO_SILU, PRO_AFFINE):
            return _launch_b16_pix(p, split, k1, p.PRO1, False)
        return _declined()
    if T != 9 or p.KH != 3 or p.PT != 1 or p.PL != 1 or p.GATE:
        return _declined()
    if p.PRO1 not in (PRO_NONE, PRO_RELU):
        return _declined()
    if p.X16 and (p.PRO1 != PRO_NONE or p.C2 != 0):
        return _declined()
    if p.C2 > 0 and (p.PRO2 != p.PRO1 or p.C1 % 16 != 0):
        return _declined()
    x16 = (not split) and bool(p.X16)
    pro = PRO_NONE if x16 else p.PRO1
    if p.M <= THIN_M:
        if p.WO < 64 or p.WO % 64 != 0:
            return _declined()
        r, xw = THIN_3X3
        return _launch_b16(p, split, BM_SPATIAL, 1, 1, 2, K3, r, xw, pro, False, False, x16, p.B * cdiv(p.WO, xw) * cdiv(p.HO, r))
    for (r, xw), widths in GEOMS_3X3:
        if (p.WO >= 64 and p.WO % 64 == 0) if widths == "mult64" else (p.WO in widths):
            return _launch_b16_bm(p, split, BM_SPATIAL, K3, r, xw, pro, False, False, x16, p.B * cdiv(p.WO, xw) * cdiv(p.HO, r))
    return _declined()


def conv(*, B, C1, H, W, M, C2=0, KH=1, KW=1, STRIDE=1, PAD_T=0, PAD_L=0, HO=None, WO=None, PRO1=PRO_NONE, PRO2=PRO_NONE, MODE=MODE_CONV,
         GATE=False, BIAS=False, RES=False, STATS=False, SCRATCH=False, BETA=0, YC=None, NREP=1, X1_BF16=0, WTB=True, flags=FLAG_BF16) -> Cv:
    """launch_conv's hand-over of a FLAG_BF16 / FLAG_SPLIT CONV record to csrc/conv_bf16.hip"""
    assert flags & (FLAG_BF16 | FLAG_SPLIT), "an f32 stage: tests/conv_dispatch.py"
    p = _P()
    p.B, p.C1, p.C2, p.H, p.W, p.M, p.KH, p.KW, p.S, p.PT, p.PL = B, C1, C2, H, W, M, KH, KW, STRIDE, PAD_T, PAD_L
    p.HO, p.WO = (H if HO is None else HO), (W if WO is None else WO)
    p.PRO1, p.PRO2, p.MODE, p.GATE, p.SCRATCH, p.X16, p.WTB = PRO1, PRO2, MODE, bool(GATE), bool(SCRATCH), bool(X1_BF16), bool(WTB)
    p.NREP = NREP if NREP > 0 else 1
    p.Ctot, p.HW, p.Ntot = C1 + C2, H * W, B * H * W
    split = bool(flags & FLAG_SPLIT)
    if split and flags & (FLAG_BF16 | FLAG_OTHERS):
        return Cv("error", "S2K_FLAG_SPLIT excludes")
    T = KH * KW
    pixlike = (T == 1 and STRIDE == 1) or MODE != MODE_CONV
    if MODE != MODE_CONV:
        if T != 1 or STRIDE != 1 or C2 != 0 or p.HO != H or p.WO != W:
            return Cv("error", "scatter/gather modes are 1x1")
        if MODE == MODE_CONVT_SCATTER and ((M & 3) or BETA or STATS or RES):
            return Cv("error", "scatter needs M = 4*Cout")
        if MODE == MODE_GATHER2X2 and ((C1 & 3) or PRO1 != PRO_NONE or GATE):
            return Cv("error", "gather needs C1 = 4*Cout")
    if pixlike and (p.HO != H or p.WO != W or PAD_T or PAD_L):
        return Cv("error", "1x1 geometry mismatch")
    if split:
        if not p.WTB:
            return Cv("error", "f32-split stage without the split weight copy")
        if p.X16:
            return Cv("error", "f32-split stages read f32 operands (X1_BF16 set)")
        cv = _route(p, True)
        return Cv("error", "f32-split stage with a shape the split kernels do not take") if cv.result == "declined" else cv
    cv = _route(p, False)
    if cv.result == "declined" and p.X16:
        return Cv("error", "X1_BF16 on a stage the bf16 1x1 kernel does not take")
    return cv


# ---------------------------------------------------------------------------------------------------------------------------------
# csrc/wgrad_bf16.hip
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Wv:
    result: object
    message: str = ""
    kernel: str = "wgrad_bf16_kernel"
    args: tuple = ()                  # (MODE, WVM, WVC, WM, WN, R, XW, P16, SPLIT)
    em: int = 0
    ec: int = 0
    BM: int = 0
    BC: int = 0
    WVK: int = 1
    n_mtiles: int = 0
    n_ctiles: int = 0
    ragged_m: bool = False
    ragged_c: bool = False
    NPJ: int = 0                      # pixels per tile
    ntiles: int = 0
    splits: int = 1
    tiles_per_split: int = 0
    short_last_split: bool = False
    images_per_tile: int = 1
    ragged_n: bool = False            # 1x1: the last pixel tile has pixels past B * HW
    R: int = 0
    XW: int = 0
    tiles_x: int = 0
    tiles_y: int = 0
    partial_row: bool = False
    lds: int = 0

    @property
    def family(self):
        return self.result

    @property
    def inst(self) -> tuple:
        return (self.kernel, self.args)

    @property
    def edges(self) -> frozenset:
        named = {
            "ragged last m-tile": self.ragged_m,
            "ragged last c-tile": self.ragged_c,
            "ragged last pixel tile": self.ragged_n,
            "pixel tile over 2 images": self.images_per_tile == 2,
            "pixel tile over >= 3 images": self.images_per_tile >= 3,
            "one split": self.splits == 1,
            "several splits": self.splits > 1,
            "shorter last split": self.short_last_split,
            "partial last tile row": self.partial_row,
            "two x tiles per row": self.tiles_x >= 2,
            "k-waves combined": self.WVK > 1,
        }
        return frozenset(k for k, v in named.items() if v)


def edge(n: int) -> int:
    """tile edge per side: 32 for thin layers, 128 unless it pads the side by more than 12 %, else 64"""
    return 32 if n <= 32 else (128 if (n > 64 and float(cdiv(n, 128) * 128) / n <= BM_PAD) else 64)


def _launch_wb16(p, split: bool, mode, wvm, wvc, wm, wn, r, xw, p16) -> Wv:
    pix = mode == WG_PIX
    BM, BC = wvm * wm * 32, wvc * wn * 32
    NPJ = xw if pix else r * xw
    XO = xw // 8
    NPO, QR, QXO = (XO, 1, XO) if pix else (r * XO, r + 2, XO + 2)
    lds = (NPO * BM + QR * QXO * BC) * 16 * (3 if split else 1)
    assert lds <= LDS_MAX
    v = Wv(SPLIT if split else BF16, "", "wgrad_bf16_kernel", (mode, wvm, wvc, wm, wn, r, xw, p16, split), em=edge(p.M), ec=edge(p.C), BM=BM, BC=BC,
           WVK=4 // (wvm * wvc), n_mtiles=cdiv(p.M, BM), n_ctiles=cdiv(p.C, BC), ragged_m=p.M % BM != 0, ragged_c=p.C % BC != 0, NPJ=NPJ, lds=lds)
    if pix:
        v.ntiles = cdiv(p.B * p.HWp, NPJ)
        v.images_per_tile = _images_per_tile(p.B * p.HWp, p.HWp, NPJ)
        v.ragged_n = (p.B * p.HWp) % NPJ != 0
    else:
        v.R, v.XW, v.tiles_x, v.tiles_y, v.partial_row = r, xw, p.WO // xw, cdiv(p.HO, r), p.HO % r != 0
        v.ntiles = p.B * v.tiles_x * v.tiles_y
    span = 1 if (not pix or p.HWp % NPJ == 0) else min(p.B, (NPJ - 2) // p.HWp + 2)
    if max(p.M * p.HWp, p.C * p.HWq) * 4 * span >= SPAN_LIMIT:
        return Wv("error", "exceed 2 GiB") if split else Wv("declined")
    mc = v.n_mtiles * v.n_ctiles
    splits = max(1, W_SLOTS[pix] // mc)
    splits = min(splits, max(1, v.ntiles // W_MIN_TILES_PER_SPLIT))
    splits = min(splits, 65535)
    v.tiles_per_split = cdiv(v.ntiles, splits)
    v.splits = cdiv(v.ntiles, v.tiles_per_split)
    v.short_last_split = v.splits > 1 and v.ntiles % v.tiles_per_split != 0
    return v


def wgrad(*, B, M, C, H, W, CTOT=None, KH=1, KW=1, STRIDE=1, PAD_T=0, PAD_L=0, HO=None, WO=None, PROP=PRO_NONE, PROQ=PRO_NONE, MODE=MODE_CONV,
          GATEP=False, GATEQ=False, P_BF16=0, flags=FLAG_BF16) -> Wv:
    """launch_wgrad's hand-over of a FLAG_BF16 / FLAG_SPLIT WGRAD record to csrc/wgrad_bf16.hip"""
    assert flags & (FLAG_BF16 | FLAG_SPLIT)
    p = _P()
    p.B, p.M, p.C, p.H, p.W = B, M, C, H, W
    p.HO, p.WO = (H if HO is None else HO), (W if WO is None else WO)
    p.HWp, p.HWq, T = p.HO * p.WO, H * W, KH * KW
    split = bool(flags & FLAG_SPLIT)
    if split and flags & FLAG_BF16:
        return Wv("error", "S2K_FLAG_SPLIT excludes S2K_FLAG_BF16")
    if split and P_BF16:
        return Wv("error", "f32-split stages read f32 operands (P_BF16 set)")

    def no():
        if split:
            return Wv("error", "f32-split stage with a shape the split kernels do not take")
        return Wv("error", "P_BF16 on a stage the bf16 1x1 kernel does not take") if P_BF16 else Wv("declined")
    if MODE != MODE_CONV or STRIDE != 1 or H != p.HO or W != p.WO or GATEP:
        return no()
    if PROP not in W_PRO or PROQ not in W_PRO:
        return no()
    em, ec = edge(M), edge(C)
    p16 = bool(P_BF16)
    if T == 1:
        if (p.HWp & 7) or B * p.HWp < W_MIN_PIXELS:
            return no()
        if p16 and PROP != PRO_NONE:
            return Wv("error", "P_BF16 with a prologue on P")
        wvm, wvc, wm, wn, xw = W_PIX[(em, ec)]
        return _launch_wb16(p, split, WG_PIX, wvm, wvc, wm, wn, 1, xw, p16)
    if T != 9 or KH != 3 or KW != 3 or PAD_T != 1 or PAD_L != 1 or GATEQ or PROP != PRO_NONE:
        return no()
    tab = W_3X3_SPLIT if split else W_3X3_BF16
    if p.WO % 64 == 0:
        g = tab["mult64"][(em == 32, ec == 32)]
    elif not split and p.WO % 56 == 0:
        g = tab["mult56"]
    elif p.WO in (32, 16):
        g = tab[p.WO]
    else:
        return no()
    return _launch_wb16(p, split, WG_SPATIAL, *g, p16)
