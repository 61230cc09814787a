"""Which weight-gradient kernel an f32 WGRAD stage runs, restated in plain Python from launch_wgrad (csrc/wgrad.hip) and the three
launchers of its chain, in the order of the chain - launch_wgrad_q4 (csrc/wgrad_q4.hip), launch_wgrad_pc (csrc/wgrad_pc.hip), then the
generic launcher (launch_wg / launch_wg2 in csrc/wgrad.hip) - at their default tuning (tune_int defaults, listed below).  Test
infrastructure.

    dispatch(B=, M=, C=, CTOT=, H=, W=, KH=, KW=, STRIDE=, PAD_T=, PAD_L=, HO=, WO=, PROP=, PROQ=, MODE=, GATEP=, GATEQ=,
             P_ALIGNED16=, Q_ALIGNED16=, P_BF16=0, flags=0) -> Wv

The keyword arguments are the WGRAD record's fields (opdefs.OPS["WGRAD"]) that decide the routing; the gates are given as truth
values, and P_ALIGNED16 / Q_ALIGNED16 say whether the operand's address is a multiple of 16 bytes (the quad kernel's condition).
FLAG_BF16, FLAG_SPLIT and P_BF16 belong to csrc/wgrad_bf16.hip (tests/b16_dispatch.py restates it) and raise NotImplementedError.
`result` is the kernel family (the code the launcher leaves in g_s2k_variant: 0 generic, 1 producer / consumer, 4 quad reads) or
"error" with a fragment of the launcher's message.  Besides the exact template instantiation a Wv holds the run-time facts a test
row has to reach: tile counts and ragged edges, the pixel tiling (NP, or the 3x3 tile R x XW with its halo), the images one pixel
tile touches, the number of pixel pairs of a tile against the k-waves' stride, and the pixel-split partition.

The pixel-split search is the same in all three files but for its cost term; it is restated in the launchers' own floating-point
expression order, so that a tie breaks the same way (`cost < best * 0.999`).  The workgroup slot counts of the search (256 / 512 /
768) are literals in the launchers, not device queries: the partition does not depend on the device.
tests/test_wgrad_dispatch_cpu.py parses every launch site and every constant below out of the three .hip files and compares.

Parsed instantiations (tests/test_wgrad_dispatch_cpu.py::test_parse_finds_every_launch_site): wgrad_kernel 64 launched, 60
reachable (S2K_WG_WIDE is 0; the WSC = 66 form needs a stride-1 record with 64-wide tiles, which wgrad_pc takes first or, with a
prologue it lacks, the generic ladder refuses), wgrad_pc_kernel 30, wgrad_q4_kernel 16."""
from __future__ import annotations

from dataclasses import dataclass, field

GENERIC, PC, Q4 = 0, 1, 4             # kernel families (include/s2k.h, s2k_program_profile_variants)
FLAG_BF16, FLAG_SPLIT = 4, 64         # plan/opdefs.py
PRO_NONE, PRO_AFFINE, PRO_SILU, PRO_RELU, PRO_GELU = 0, 1, 2, 3, 4
MODE_CONV, MODE_CONVT_SCATTER, MODE_GATHER2X2 = 0, 1, 2
WG_PIX, WG_SPATIAL, WG_GATHER = 0, 1, 2      # csrc/wgrad.h
NTHREADS = 256
WG_EPT_MAX = 2                        # csrc/wgrad.h: halo elements per thread per channel
SPAN_LIMIT = 0x7ffffff0
LDS_MAX = 160 * 1024

# tune_int defaults
TUNE = {"wgrad_q4.hip": {"S2K_WG_Q4": 5, "S2K_WG_STREAMK": 0}, "wgrad_pc.hip": {"S2K_WG_PC": 3},
        "wgrad.hip": {"S2K_WG_EXP": 0, "S2K_WG_THIN_NP": 256, "S2K_WG_WIDE": 0}}

EDGE_PAD = 1.12                       # edge(): 128 unless it pads the side by more than 12 %
THIN_SIDE = 32                        # M <= 32 / C <= 32
THIN_M2, THIN_C2 = 64, 32             # 3x3: also M <= 64 && C <= 32
MIN_PIXELS = 1024                     # q4 and pc 1x1: B * HWp >= 1024
THIN_NP_PIXELS = 262144               # generic thin 1x1: 256-pixel tiles from here
MIN_TILES_PER_SPLIT = 4               # max_splits = cdiv(ntiles, 4)
SPLIT_ROUNDS = 4                      # s_hi = 4 * slots / mc
MAX_SPLITS = 65535
BETTER = 0.999                        # cost < best * 0.999

# ---- csrc/wgrad_q4.hip: (P, Q) prologue pairs of launch_q4w_pro ---------------------------------------------------------------------
Q4_PRO = ((PRO_NONE, PRO_NONE), (PRO_NONE, PRO_RELU), (PRO_RELU, PRO_NONE), (PRO_NONE, PRO_SILU))
# ---- csrc/wgrad_pc.hip ------------------------------------------------------------------------------------------------------------
PC_PIX_PRO = ((PRO_NONE, PRO_NONE), (PRO_NONE, PRO_RELU), (PRO_RELU, PRO_NONE))
PC_SPATIAL_PRO = ((PRO_NONE, PRO_NONE), (PRO_NONE, PRO_RELU))
PC_GEOMS = ((1, 64), (2, 32), (4, 16), (8, 8), (1, 56), (2, 28), (4, 14))      # PC_SPATIAL_CASE(R, XWE), in the launcher's order
PC_THIN_MIN_WO, PC_THIN_MIN_HO = 64, 2
PC_THIN = {True: (1, 1, 1, 1, 4), False: (1, 1, 2, 1, 2)}                        # (WM, WN, WVM, WVN, WVK) by M <= 32; NPJ 128, R 2, XWE 64
# ---- csrc/wgrad.hip: launch_wg<MODE, T, WM, WN, WVM, WVN, WVK, NPJ, EPT[, WSC]> ------------------------------------------------------
G_GATHER_THIN = (WG_GATHER, 4, 1, 1, 2, 1, 2, 32, 1)
G_GATHER = (WG_GATHER, 4, 1, 2, 2, 2, 1, 32, 1)
G_PIX_THIN256 = (WG_PIX, 1, 1, 1, 1, 1, 4, 256, 1)
G_PIX_THIN = (WG_PIX, 1, 1, 1, 1, 1, 4, 64, 1)
G_PIX = {(128, 128): (WG_PIX, 1, 2, 2, 2, 2, 1, 64, 1), (128, 64): (WG_PIX, 1, 2, 1, 2, 2, 1, 64, 1), (64, 128): (WG_PIX, 1, 1, 2, 2, 2, 1, 64, 1),
         (64, 64): (WG_PIX, 1, 1, 1, 2, 2, 1, 64, 1)}
G_SP_THIN_MC = (WG_SPATIAL, 9, 1, 1, 1, 1, 4, 128, 2)       # M <= 32 and C <= 32
G_SP_THIN_M = (WG_SPATIAL, 9, 1, 1, 1, 2, 2, 128, 2)        # M <= 32
G_SP_THIN_C = (WG_SPATIAL, 9, 1, 1, 2, 1, 2, 128, 2)        # M <= 64 and C <= 32
G_SP_WIDE = (WG_SPATIAL, 9, 1, 1, 2, 2, 1, 128, 2)          # S2K_WG_WIDE
G_SP_WSC = (WG_SPATIAL, 9, 1, 1, 2, 2, 1, 64, 1, 66)
G_SP_EPT1 = (WG_SPATIAL, 9, 1, 1, 2, 2, 1, 64, 1)
G_SP_EPT2 = (WG_SPATIAL, 9, 1, 1, 2, 2, 1, 64, 2)
# the prologue ladder of launch_wg, (P, Q) pairs by mode
G_PRO = {WG_GATHER: ((PRO_RELU, PRO_NONE), (PRO_SILU, PRO_NONE), (PRO_NONE, PRO_NONE), (PRO_GELU, PRO_NONE)),
         WG_SPATIAL: ((PRO_NONE, PRO_NONE), (PRO_NONE, PRO_RELU)),
         WG_PIX: ((PRO_NONE, PRO_NONE), (PRO_NONE, PRO_RELU), (PRO_NONE, PRO_SILU), (PRO_NONE, PRO_GELU), (PRO_RELU, PRO_NONE), (PRO_SILU, PRO_NONE),
                  (PRO_GELU, PRO_NONE))}
G_PRO_WSC = ((PRO_NONE, PRO_NONE), (PRO_NONE, PRO_RELU))


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def edge(n: int) -> int:
    """tile edge per side (all three files): 128 unless it pads the side by more than 12 %, else 64"""
    return 128 if (n > 64 and float(cdiv(n, 128)) * 128 / n <= EDGE_PAD) else 64


@dataclass
class Wv:
    result: object                    # 0, 1, 4 or "error"
    message: str = ""                 # "error": a fragment of the launcher's message
    kernel: str = ""
    args: tuple = ()                  # the exact template arguments, in the template's order
    declined: tuple = ()              # (link, reason) of every link that saw the record and passed it on
    mode: int = WG_PIX
    T: int = 1
    WVK: int = 1
    BM: int = 0
    BC: int = 0
    M: int = 0
    C: int = 0
    n_mtiles: int = 0
    n_ctiles: int = 0
    ragged_m: bool = False
    ragged_c: bool = False
    NP: int = 0                       # pixels per tile (PIX / GATHER)
    NPJ: int = 0                      # pixel slots per tile
    ntiles: int = 0
    last_tile_pixels: int = 0         # PIX / GATHER
    images_per_tile: int = 1          # the most images one pixel tile touches
    span: int = 1                     # what the 2 GiB check multiplies an image by
    npairs: int = 0
    splits: int = 1
    tiles_per_split: int = 0
    last_split: int = 0               # tiles of the last split
    R: int = 0
    XW: int = 0
    XWe: int = 0
    IR: int = 0
    IC: int = 0
    WS: int = 0
    tiles_x: int = 0
    tiles_y: int = 0
    partial_row: bool = False
    partial_col: bool = False
    r_capped: bool = False            # R = HO < NPX / XWe
    r_shrunk: bool = False            # the halo capacity cut R (for (;; --R))
    xw_halved: bool = False           # ... and XW (its XW /= 2 branch)
    lds: int = 0
    facts: dict = field(default_factory=dict)

    @property
    def family(self):
        return self.result

    @property
    def inst(self) -> tuple:
        return (self.kernel, self.args)

    @property
    def pairs_class(self) -> str:
        """npairs against the k-waves' stride of the generic pair loop (s += 2 * WVK, break at s + WVK >= npairs)"""
        if self.npairs % (2 * self.WVK) == 0:
            return "multiple of 2 WVK"
        return "multiple of WVK only" if self.npairs % self.WVK == 0 else "no multiple of WVK"

    @property
    def split_class(self) -> str:
        if self.splits == 1:
            return "one split"
        return "equal splits" if self.last_split == self.tiles_per_split else "short last split"

    @property
    def edges(self) -> frozenset:
        """the run-time edges this launch meets, by name (tests/test_wgrad_dispatch_cpu.py asks for each of them per kernel)"""
        if self.result == "error":
            return frozenset()
        sp = self.mode == WG_SPATIAL
        named = {
            "ragged last m-tile": self.ragged_m,
            "ragged last c-tile": self.ragged_c,
            "M one past a tile": self.BM > 0 and self.M % self.BM == 1,
            "C one past a tile": self.BC > 0 and self.C % self.BC == 1,
            "ragged last pixel tile": not sp and self.last_tile_pixels < self.NP,
            "pixel tile in 1 image": not sp and self.images_per_tile == 1,
            "pixel tile straddles 2 images": self.images_per_tile == 2,
            "pixel tile straddles >= 3 images": self.images_per_tile >= 3,
            "npairs: " + self.pairs_class: True,
            self.split_class: True,
            "partial last tile row": sp and self.partial_row,
            "partial last tile column": sp and self.partial_col,
            "odd XW": sp and self.XWe != self.XW,
            "several x tiles per row": sp and self.tiles_x > 1,
            "R capped by HO": sp and self.r_capped,
            "R cut by the halo capacity": sp and self.r_shrunk,
            "XW halved by the halo capacity": sp and self.xw_halved,
        }
        return frozenset(k for k, v in named.items() if v)


class _P:
    pass


def _images_per_tile(ntot: int, hw: int, np_: int) -> int:
    worst = 1
    for nt in range(cdiv(ntot, np_)):
        worst = max(worst, (min((nt + 1) * np_, ntot) - 1) // hw - (nt * np_) // hw + 1)
        if worst >= 3:
            break
    return worst


def _split_search(ntiles: int, mc: int, slots: int, cost_of) -> tuple:
    """the pixel-split search of launch_q4w / launch_pc2 / launch_wg2; cost_of(rounds, tiles per split) in the launcher's own order"""
    max_splits = cdiv(ntiles, MIN_TILES_PER_SPLIT)
    if max_splits > MAX_SPLITS:
        max_splits = MAX_SPLITS
    if max_splits < 1:
        max_splits = 1
    splits, best = 1, 1e30
    s_hi = min(max_splits, max(1, SPLIT_ROUNDS * slots // mc))
    for sp in range(1, s_hi + 1):
        rounds = float(cdiv(mc * sp, slots))
        cost = cost_of(rounds, float(cdiv(ntiles, sp)))
        if cost < best * BETTER:
            best, splits = cost, sp
    tps = cdiv(ntiles, splits)
    splits = cdiv(ntiles, tps)
    return splits, tps, ntiles - (splits - 1) * tps


def _span(p, NPJ: int, spatial: bool) -> int:
    return 1 if (spatial or p.HWp % NPJ == 0) else min(p.B, (NPJ - 2) // p.HWp + 2)


def _too_big(p, span: int) -> bool:
    return max(p.M * p.HWp, p.C * p.HWq) * 4 * span >= SPAN_LIMIT


def _facts(p, v: Wv, mode, T, BM, BC, WVK, NPJ):
    v.mode, v.T, v.BM, v.BC, v.WVK, v.NPJ, v.M, v.C = mode, T, BM, BC, WVK, NPJ, p.M, p.C
    v.n_mtiles, v.n_ctiles = cdiv(p.M, BM), cdiv(p.C, BC)
    v.ragged_m, v.ragged_c = p.M % BM != 0, p.C % BC != 0
    if mode == WG_SPATIAL:
        v.R, v.XW, v.XWe, v.IR, v.IC, v.WS, v.tiles_x, v.tiles_y = p.R, p.XW, p.XWe, p.IR, p.IC, p.WS, p.tiles_x, p.tiles_y
        v.ntiles = p.ntiles
        v.partial_row, v.partial_col = p.HO % p.R != 0, p.WO % p.XW != 0
        v.npairs = p.R * p.XWe // 2
        v.images_per_tile = 1
    else:
        npix = p.B * p.HWp
        v.NP, v.ntiles = p.NP, p.ntiles
        v.last_tile_pixels = npix - (p.ntiles - 1) * p.NP
        v.images_per_tile = _images_per_tile(npix, p.HWp, p.NP)
        v.npairs = NPJ // 2
    v.span = _span(p, NPJ, mode == WG_SPATIAL)


# ---------------------------------------------------------------------------------------------------------------------------------
# csrc/wgrad_q4.hip
# ---------------------------------------------------------------------------------------------------------------------------------
def _launch_q4(p):
    """a Wv, or the reason launch_wgrad_q4 returns 1"""
    if p.gatep:
        return "a gate on P"
    if p.gateq and (p.proq != PRO_SILU or p.T != 1):
        return "a gate on Q without SiLU / outside 1x1"
    if p.mode != MODE_CONV or p.S != 1 or p.H != p.HO or p.W != p.WO:
        return "not a stride-1 same-size conv"
    if not (p.p_al16 and p.q_al16):
        return "P or Q not 16-byte aligned"
    if p.T != 1:
        return "not 1x1"
    if p.M <= THIN_SIDE or p.C <= THIN_SIDE or (p.HWp & 3) or p.HWq != p.HWp:
        return "a thin side or H * W % 4 != 0"
    if p.B * p.HWp < MIN_PIXELS or p.B * p.HWp > 0x7fffffff:
        return "fewer than 1024 pixels"
    wm, wn = edge(p.M) // 64, edge(p.C) // 64
    if (p.prop, p.proq) not in Q4_PRO:
        return "prologue pair not in launch_q4w_pro"
    p.NP = 64
    p.ntiles = cdiv(p.B * p.HWp, 64)
    span = _span(p, 64, False)
    if _too_big(p, span):
        return Wv("error", "exceed 2 GiB")
    v = Wv(Q4, "", "wgrad_q4_kernel", (wm, wn, p.prop, p.proq))
    _facts(p, v, WG_PIX, 1, wm * 64, wn * 64, 1, 64)
    mc = v.n_mtiles * v.n_ctiles
    v.splits, v.tiles_per_split, v.last_split = _split_search(p.ntiles, mc, 256, lambda rounds, tiles: rounds * (tiles + (2.0 if wm * wn >= 4 else 1.0)))
    v.lds = 2 * (v.BM + v.BC) * (64 + 4) * 4
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# csrc/wgrad_pc.hip
# ---------------------------------------------------------------------------------------------------------------------------------
def _launch_pc2(p, mode, T, wm, wn, wvm, wvn, wvk, npj, r, xwe) -> Wv:
    BM, BC = wm * wvm * 32, wn * wvn * 32
    span = _span(p, npj, mode == WG_SPATIAL)
    if _too_big(p, span):
        return Wv("error", "exceed 2 GiB")
    used = (r + 2) * (xwe + 2) if mode == WG_SPATIAL else npj
    v = Wv(PC, "", "wgrad_pc_kernel", (mode, T, wm, wn, wvm, wvn, wvk, npj, r, xwe, p.prop, p.proq))
    _facts(p, v, mode, T, BM, BC, wvk, npj)
    v.lds = 2 * (npj * (BM + 4) + used * (BC + 4)) * 4
    mc = v.n_mtiles * v.n_ctiles
    v.splits, v.tiles_per_split, v.last_split = _split_search(
        p.ntiles, mc, 256, lambda rounds, tiles: rounds * (tiles + (1.0 if T == 9 else (2.0 if wm * wn >= 4 else 1.0))))
    return v


def _launch_pc(p):
    """a Wv, or the reason launch_wgrad_pc returns 1"""
    npix = p.B * p.HWp
    if p.gatep or p.gateq:
        return "an SE gate"
    if p.mode == MODE_CONV and p.T == 9 and p.S == 1 and p.KH == 3 and p.KW == 3 and p.H == p.HO and p.W == p.WO:
        thin = p.M <= THIN_SIDE or (p.M <= THIN_M2 and p.C <= THIN_C2)
        if thin:
            if p.C > THIN_SIDE or p.WO < PC_THIN_MIN_WO or p.HO < PC_THIN_MIN_HO:
                return "thin 3x3 with C > 32, WO < 64 or HO < 2"
            p.R, p.XW, p.XWe, p.IR, p.IC, p.WS = 2, 64, 64, 4, 66, 66
            p.tiles_x, p.tiles_y = cdiv(p.WO, 64), cdiv(p.HO, 2)
            p.ntiles = p.B * p.tiles_x * p.tiles_y
            p.NP = 0
            if (p.prop, p.proq) not in PC_SPATIAL_PRO:
                return "3x3 prologue pair not in launch_pc_spatial_thin"
            wm, wn, wvm, wvn, wvk = PC_THIN[p.M <= THIN_SIDE]
            return _launch_pc2(p, WG_SPATIAL, 9, wm, wn, wvm, wvn, wvk, 128, 2, 64)
        XW = p.WO if p.WO <= 64 else 64
        XWe = (XW + 1) & ~1
        R = 64 // XWe
        if R > p.HO:
            R = p.HO
        if (R, XWe) not in PC_GEOMS:
            return f"no PC_SPATIAL_CASE({R}, {XWe})"
        p.R, p.XW, p.XWe, p.IR, p.IC, p.WS = R, XW, XWe, R + 2, XWe + 2, XWe + 2
        p.tiles_x, p.tiles_y = cdiv(p.WO, XW), cdiv(p.HO, R)
        p.ntiles = p.B * p.tiles_x * p.tiles_y
        p.NP = 0
        if (p.prop, p.proq) not in PC_SPATIAL_PRO:
            return "3x3 prologue pair not in launch_pc_spatial"
        v = _launch_pc2(p, WG_SPATIAL, 9, 1, 1, 2, 2, 1, 64, R, XWe)
        v.r_capped = R == p.HO and R < 64 // XWe
        return v
    if p.mode == MODE_CONV and p.T == 1 and p.S == 1 and p.H == p.HO and p.W == p.WO:
        if p.M <= THIN_SIDE or p.C <= THIN_SIDE:
            return "a thin side"
        if npix < MIN_PIXELS:
            return "fewer than 1024 pixels"
        p.NP = 64
        p.ntiles = cdiv(npix, 64)
        if (p.prop, p.proq) not in PC_PIX_PRO:
            return "prologue pair not in launch_pc_pix"
        return _launch_pc2(p, WG_PIX, 1, edge(p.M) // 64, edge(p.C) // 64, 2, 2, 1, 64, 1, 64)
    return "not a stride-1 same-size 1x1 / 3x3 conv"


# ---------------------------------------------------------------------------------------------------------------------------------
# csrc/wgrad.hip
# ---------------------------------------------------------------------------------------------------------------------------------
def _launch_wg(p, cfg) -> Wv:
    mode, T, wm, wn, wvm, wvn, wvk, npj, ept = cfg[:9]
    wsc = cfg[9] if len(cfg) > 9 else 0
    pair = (p.prop, p.proq)
    if wsc and pair in G_PRO_WSC:
        args = cfg[:9] + pair + (wsc,)
    elif pair in G_PRO[mode]:
        args = cfg[:9] + pair + (0,)
    else:
        return Wv("error", f"prologue combination (P {p.prop}, Q {p.proq}) is not instantiated for this mode")
    BM, BC = wm * wvm * 32, wn * wvn * 32
    span = _span(p, npj, mode == WG_SPATIAL)
    if _too_big(p, span):
        return Wv("error", "exceed 2 GiB")
    csq = NTHREADS * ept + 1 if mode == WG_SPATIAL else (4 * npj + 1 if mode == WG_GATHER else npj + 1)
    lds = (BM * (npj + 1) + BC * csq + 2 * (BM + BC)) * 4
    if p.gatep or (p.gateq and mode != WG_PIX):
        return Wv("error", "SE gate is only supported on the Q operand of 1x1 convs")
    assert lds <= LDS_MAX
    if mode == WG_SPATIAL:
        assert p.IR * p.WS <= NTHREADS * ept and p.R * p.XWe <= npj      # ("halo exceeds EPT", "tile exceeds pixel slots": the launcher's geometry rules them out)
    v = Wv(GENERIC, "", "wgrad_kernel", args)
    _facts(p, v, mode, T, BM, BC, wvk, npj)
    v.lds = lds
    mc = v.n_mtiles * v.n_ctiles
    slots = 256 if (T == 9 or wm * wn >= 4) else (512 if wm * wn >= 2 else 768)
    v.splits, v.tiles_per_split, v.last_split = _split_search(
        p.ntiles, mc, slots,
        lambda rounds, tiles: rounds * (tiles + (1.5 if T == 9 else (2.0 if wm * wn >= 4 else 0.7))) * (1.0 if T == 9 else 1.0 + 0.15 / rounds))
    v.facts["slots"] = slots
    return v


def _launch_generic(p) -> Wv:
    npix = p.B * p.HWp
    if p.mode == MODE_GATHER2X2:
        if p.T != 4 or p.H != 2 * p.HO or p.W != 2 * p.WO or p.proq != PRO_NONE or p.gateq:
            return Wv("error", "wgrad: gather geometry")
        p.NP = 32
        p.ntiles = cdiv(npix, 32)
        return _launch_wg(p, G_GATHER_THIN if (p.M <= THIN_SIDE or p.C <= THIN_SIDE) else G_GATHER)
    if p.T == 1 and p.S == 1:
        if p.H != p.HO or p.W != p.WO:
            return Wv("error", "wgrad: 1x1 geometry")
        p.NP = 64
        p.ntiles = cdiv(npix, 64)
        if p.M <= THIN_SIDE and p.C <= THIN_SIDE:
            if npix >= THIN_NP_PIXELS:
                p.NP = 256
                p.ntiles = cdiv(npix, 256)
                return _launch_wg(p, G_PIX_THIN256)
            return _launch_wg(p, G_PIX_THIN)
        return _launch_wg(p, G_PIX[(edge(p.M), edge(p.C))])
    if p.T != 9:
        return Wv("error", "only 1x1, 3x3 and 2x2-transpose kernels are on this path")
    thin = p.M <= THIN_SIDE or (p.M <= THIN_M2 and p.C <= THIN_C2)
    NPX = 128 if thin else 64
    XW = p.WO if p.WO <= NPX else NPX
    R = NPX // ((XW + 1) & ~1)
    r_capped = False
    if R > p.HO:
        R, r_capped = p.HO, True
    if R < 1:
        R = 1
    r0, shrunk, halved = R, False, False
    while True:      # for (;; --R)
        p.R, p.XW, p.XWe = R, XW, (XW + 1) & ~1
        p.IR = (R - 1) * p.S + p.KH
        p.IC = (p.XWe - 1) * p.S + p.KW
        p.WS = p.IC
        if p.IR * p.WS <= NTHREADS * WG_EPT_MAX:
            break
        if R == 1:
            if XW > 16:      # { XW /= 2; R = 2; continue; } - and the `continue` of a for (;; --R) runs the --R: the halved tile gets R = 1
                XW //= 2
                R = 2 - 1
                halved = True
                continue
            return Wv("error", "halo tile does not fit")
        R -= 1
        shrunk = True
    p.tiles_x, p.tiles_y = cdiv(p.WO, p.XW), cdiv(p.HO, p.R)
    p.ntiles = p.B * p.tiles_x * p.tiles_y
    p.NP = 0
    if thin and p.M <= THIN_SIDE and p.C <= THIN_SIDE:
        cfg = G_SP_THIN_MC
    elif thin and p.M <= THIN_SIDE:
        cfg = G_SP_THIN_M
    elif thin:
        cfg = G_SP_THIN_C
    elif p.IR * p.WS <= NTHREADS and p.WS == 66 and p.KW == 3:
        cfg = G_SP_WSC
    elif p.IR * p.WS <= NTHREADS:
        cfg = G_SP_EPT1
    else:
        cfg = G_SP_EPT2
    v = _launch_wg(p, cfg)
    v.r_capped, v.r_shrunk, v.xw_halved = r_capped and p.R == r0 and not halved, shrunk, halved
    return v


def dispatch(*, B, M, C, H, W, CTOT=None, KH=1, KW=1, STRIDE=1, PAD_T=0, PAD_L=0, HO=None, WO=None, PROP=PRO_NONE, PROQ=PRO_NONE, MODE=MODE_CONV,
             GATEP=False, GATEQ=False, P_ALIGNED16=True, Q_ALIGNED16=True, P_BF16=0, flags=0) -> Wv:
    """launch_wgrad on an f32 record: the chain q4 -> pc -> generic"""
    if flags & (FLAG_BF16 | FLAG_SPLIT) or P_BF16:
        raise NotImplementedError("FLAG_BF16 / FLAG_SPLIT / P_BF16 stages: tests/b16_dispatch.py")
    p = _P()
    p.B, p.M, p.C, p.CTOT, p.H, p.W, p.KH, p.KW, p.S, p.PT, p.PL = B, M, C, (C if CTOT is None else CTOT), H, W, KH, KW, STRIDE, PAD_T, PAD_L
    p.HO, p.WO = (H if HO is None else HO), (W if WO is None else WO)
    p.prop, p.proq, p.mode, p.gatep, p.gateq, p.p_al16, p.q_al16 = PROP, PROQ, MODE, bool(GATEP), bool(GATEQ), bool(P_ALIGNED16), bool(Q_ALIGNED16)
    p.T, p.HWp, p.HWq = KH * KW, p.HO * p.WO, H * W
    p.NP = p.ntiles = 0
    if B <= 0 or M <= 0 or C <= 0:
        return Wv("error", "missing tensor / bad dims")
    declined = []
    for name, link in (("q4", _launch_q4), ("pc", _launch_pc)):
        v = link(p)
        if isinstance(v, Wv):
            v.declined = tuple(declined)
            return v
        declined.append((name, v))
    v = _launch_generic(p)
    v.declined = tuple(declined)
    return v
