"""Which dense-convolution kernel an f32 CONV stage runs, restated in plain Python from launch_conv (csrc/igemm.hip) and the four
launchers it hands a record to, in the order of the chain - launch_conv_q4 (csrc/conv_q4.hip, FLAG_Q4) or the flagged
launch_conv_dma (csrc/conv_dma.hip, FLAG_DMA), then launch_conv_pc (csrc/igemm_pc.hip), launch_conv_dma again, then the generic
conv_igemm_kernel - at their default tuning (tune_int defaults, listed below) and on a 256-CU device.  Test infrastructure.

    dispatch(B=, C1=, H=, W=, M=, ...) -> Cv

The keyword arguments are the CONV record's fields (opdefs.OPS["CONV"]) that decide the routing; tensors are given as truth values
(GATE, BIAS, RES, STATS, SCRATCH).  `flags` takes FLAG_Q4 / FLAG_DMA / FLAG_RES_GELU_GRAD; FLAG_BF16, FLAG_SPLIT and X1_BF16 belong
to csrc/conv_bf16.hip (tests/b16_dispatch.py restates it) and raise NotImplementedError.  Besides the kernel family (the code the launcher leaves in g_s2k_variant:
0 generic, 1 producer / consumer, 3 LDS-DMA ring, 4 quad reads) and the exact template instantiation, a Cv holds the run-time facts
a test case has to reach: tile counts and ragged edges, the split-K partition, the epilogue form, the K tail, tiles that straddle
images, the 3x3 tiling, the persistent kernels' items per workgroup.  The two cost searches are restated in the launchers' own
floating-point expression order, so that a tie breaks the same way.  tests/test_conv_dispatch_cpu.py parses every constant below
out of the four .hip files and compares."""
from __future__ import annotations

from dataclasses import dataclass

GENERIC, PC, DMA, Q4 = 0, 1, 3, 4     # kernel families (include/s2k.h, s2k_program_profile_variants)

FLAG_BF16, FLAG_DMA, FLAG_Q4, FLAG_RES_GELU_GRAD, FLAG_SPLIT = 4, 8, 16, 32, 64       # plan/opdefs.py
PRO_NONE, PRO_AFFINE, PRO_SILU, PRO_RELU, PRO_GELU = 0, 1, 2, 3, 4
MODE_CONV, MODE_CONVT_SCATTER, MODE_GATHER2X2 = 0, 1, 2
BM_PIX, BM_SPATIAL = 0, 1
NTHREADS = 256
N_CU = 256                            # workgroups of the persistent kernels (one per CU of an MI355X)

# ---- csrc/igemm.hip ---------------------------------------------------------------------------------------------------------------
PICK_BM_WASTE = 0.12                  # pick_bm: largest BM in {128, 64, 32} wasting <= 12 % of the rows
PIX_SMALL_TILES = 400                 # S2K_PIX_SMALL_TILES
PIX_K16_MAX = 192                     # S2K_PIX_K16_MAX
# PIX_CFG(WM, WN, WVM, WVN, KCH, pixels per tile, split-K allowed), in the launcher's order of tests
PIX_SMALL = (1, 1, 2, 2, 64, 64, True)
PIX_128_K16 = (2, 2, 2, 2, 16, 128, False)
PIX_128 = (2, 2, 2, 2, 64, 128, False)
PIX_64 = (2, 2, 1, 4, 16, 256, False)
PIX_32 = (1, 2, 1, 4, 16, 256, False)
SPLITK_MIN_CHUNKS = 4
SPLITK_A = (512, 1024)                # blocks <= 512: splits = cdiv(1024, blocks)
SPLITK_B = (1024, 32, 1536)           # else blocks <= 1024 and nchunks >= 32: splits = cdiv(1536, blocks)
SPLITK_MAX = 8
# launch_cfg<BM_SPATIAL, 9, WM, WN, WVM, WVN, KCH, EPT, MINW>, BN, cap / NTHREADS
SP_128 = (2, 2, 2, 2, 8, 2, 2)
SP_64W = (2, 2, 1, 4, 8, 4, 2)
SP_64 = (1, 1, 2, 2, 8, 2, 2)
SP_THIN512 = (1, 4, 1, 4, 8, 5, 2)
SP_THIN1024 = (1, 8, 1, 4, 8, 7, 1)
SP_32 = (1, 2, 1, 4, 8, 4, 2)
SP_MIN_TILES = 160                    # 128-row and 64 x 256 tiles need this many
SP_THIN_MIN = 200                     # out_px / 512 (or / 1024) >= 200
TEPI_BN = (64, 256)
SPAN_LIMIT = 0x7ffffff0

# ---- csrc/igemm_pc.hip ------------------------------------------------------------------------------------------------------------
PC_PRO = (PRO_NONE, PRO_RELU)
PC_THIN_MAX_M, PC_THIN_MIN_M, PC_THIN_MIN_TILES, PC_THIN_KCH = 32, 20, 512, 4      # S2K_CONV_PC_THIN_KCH
PC_MIN_M = 48
PC_BM_PAD = 1.12
PC_PIX_MIN_TILES = 192
PC_NARROW_MIN_K, PC_NARROW_MIN_TILES = 512, 384
PC_PIX_MIN_K = 256
PC_KCH1 = 32                          # S2K_CONV_PC_KCH1
PC_KCH3, PC_KCH3_WIDE_M = 4, 256      # S2K_CONV_PC_KCH3; M >= 256: 8-channel chunks
PC3_MIN_TILES = 160
# (R, XW) by the map width, in the launcher's order
PC3_GEOMS = (((2, 64), "mult64"), ((4, 32), (32,)), ((8, 16), (16,)), ((2, 56), (56, 112, 224)), ((4, 28), (28,)), ((8, 14), (14,)))

# ---- csrc/conv_dma.hip ------------------------------------------------------------------------------------------------------------
DMA_MIN_M = 40
DMA_RULE = (8192, 512, 768)           # Ntot <= 8192 and (Ctot >= 512 or M >= 768)
DMA_MAX_WM, DMA_MAX_WN = 5, 2
DMA_PRE_MAX_TILES = 5                 # PRE variants: wm * wn <= 5
DMA_SPLIT = (256, 8, 8, 4)            # items < 256 and nchunks >= 8: sp = min(8, nchunks / 4, cdiv(256, items))
DMA_COST = (3.0, 2.0, 0.02, 6, 0.02, 2)
DMA_K32_MIN = 32                      # Ctot > 32: 32-channel stages in a ring of 3

# ---- csrc/conv_q4.hip -------------------------------------------------------------------------------------------------------------
Q4_MIN_M = 24
Q4_RULE_A = (32768, 40, 256)          # Ntot >= 32768 and M >= 40 and Ctot < 256
Q4_RULE_B = (8192, 512, 2048)         # Ntot <= 8192 and M <= 512 and Ctot >= 2048
Q4_CANDS = ((2, 4, 1), (2, 2, 2), (2, 1, 4), (1, 4, 1), (1, 2, 2))      # (wm, wvm, wvn)
Q4_COST = (2.0, 2.0, 1.10)
Q4_K32_MIN = 32


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


@dataclass
class Cv:
    family: int
    kernel: str                       # template name
    args: tuple                       # its exact template arguments, in the template's order
    BM: int = 0
    BN: int = 0
    n_mtiles: int = 0
    n_ntiles: int = 0                 # pixel tiles (3x3: B * tiles_x * tiles_y)
    ragged_m: bool = False            # the last m-tile has rows past M
    ragged_n: bool = False            # 1x1: the last pixel tile has pixels past Ntot
    KCH: int = 0                      # channels per chunk (ring kernels: per stage)
    nchunks: int = 0
    k_tail: int = 0                   # Ctot % KCH
    k_lt_chunk: bool = False          # the whole reduction is shorter than one chunk
    tail_in_src2: bool = False        # concat: the K tail's valid channels end in source 2
    chunk_straddles_sources: bool = False   # concat: some chunk holds channels of both sources
    mixed_pro: bool = False           # concat with pro2 != pro1 (the generic kernel's per-element prologue form)
    splits: int = 1
    chunks_per_split: int = 0         # the longest split, in chunks
    short_last_split: bool = False    # generic rule: the last split is shorter; ring rule: the splits differ in length
    split_rule: str = ""              # generic: "A" (blocks <= 512) or "B"; ring kernels: "ring"
    split_cap8: bool = False          # the rule asked for more than 8 splits
    split_cap_half: bool = False      # ... for more than nchunks / 2
    could_split: bool = False         # the same record with SCRATCH would split (this one has none)
    tepi: bool = False                # transposed (LDS) store of the output tile
    bvec: bool = False                # generic 1x1: the vector stager
    images_per_tile: int = 1          # 1x1: the most images one pixel tile touches
    span: int = 1                     # what the 2 GiB check multiplies an image by
    R: int = 0                        # 3x3 tiling
    XW: int = 0
    tiles_x: int = 0
    tiles_y: int = 0
    partial_row: bool = False         # the last tile row is cut by HO
    partial_col: bool = False         # the last tile column is cut by WO
    r_capped: bool = False            # R = HO < BN / XW
    r_shrunk: bool = False            # the halo capacity cut R (generic)
    items: int = 0                    # ring / quad kernels: work items
    items_per_wg: float = 0.0         # ... per workgroup at 256 CUs
    k32: bool = False                 # ring / quad kernels: 32-channel stages (ring of 3), else 16 (ring of 4)
    PRE: int = 0
    nrep: int = 1
    declined: tuple = ()              # the links that saw the record and passed it on

    @property
    def inst(self) -> tuple:
        return (self.kernel, self.args)

    @property
    def edges(self) -> frozenset:
        """the run-time edges this launch meets, by name (tests/test_conv_dispatch_cpu.py asks for each of them per kernel)"""
        ring = self.family in (DMA, Q4)
        spatial = self.XW > 0
        named = {
            "ragged last m-tile": self.ragged_m,
            "ragged last pixel tile": self.ragged_n,
            "pixel tile straddles 2 images": self.images_per_tile == 2,
            "pixel tile straddles >= 3 images": self.images_per_tile >= 3,
            "K tail": self.k_tail > 0 and not self.k_lt_chunk,
            "K < one chunk": self.k_lt_chunk,
            "K tail in source 2": self.tail_in_src2,
            "a chunk holds channels of both sources": self.chunk_straddles_sources,
            "concat with pro2 != pro1": self.mixed_pro,
            "split-K": self.splits > 1,
            "no split-K": self.splits == 1,
            "split-K: the splits differ in length": self.short_last_split,
            "split-K rule A (blocks <= 512)": self.split_rule == "A",
            "split-K rule B (512 < blocks <= 1024, >= 32 chunks)": self.split_rule == "B",
            "split-K capped at 8": self.split_cap8,
            "split-K capped at nchunks / 2": self.split_cap_half,
            "would split with SCRATCH, has none": self.could_split,
            "transposed epilogue": self.tepi and not ring,
            "scalar epilogue": not self.tepi and self.splits == 1,
            "vector stager": self.family == GENERIC and not spatial and self.bvec,
            "scalar stager": self.family == GENERIC and not spatial and not self.bvec,
            "partial last tile row": self.partial_row,
            "partial last tile column": self.partial_col,
            "several x tiles per row": self.tiles_x > 1,
            "R capped by HO": self.r_capped,
            "R cut by the halo capacity": self.r_shrunk,
            "more items than workgroups, with a remainder": ring and self.items_gt_wgs_with_remainder,
            "fewer items than workgroups": ring and self.items_lt_wgs,
            "32-channel stages": ring and self.k32,
            "16-channel stages": ring and not self.k32,
        }
        return frozenset(k for k, v in named.items() if v)

    @property
    def items_gt_wgs_with_remainder(self) -> bool:
        return self.items > N_CU and self.items % N_CU != 0

    @property
    def items_lt_wgs(self) -> bool:
        return 0 < self.items < N_CU


class _P:
    pass


def pick_bm(M: int) -> int:
    best, best_w = 32, 1e9
    for bm in (128, 64, 32):
        w = float(cdiv(M, bm) * bm) / M - 1.0
        if w <= PICK_BM_WASTE:
            return bm
        if w < best_w - 1e-9:
            best_w, best = w, bm
    return best


def _images_per_tile(p, BN: int) -> int:
    worst = 1
    for nt in range(cdiv(p.Ntot, BN)):
        first = (nt * BN) // p.HW
        last = (min((nt + 1) * BN, p.Ntot) - 1) // p.HW
        worst = max(worst, last - first + 1)
    return worst


def _span(p, BN: int, spatial: bool) -> int:
    return 1 if (spatial or p.HW % BN == 0) else min(p.B, (BN - 2) // p.HW + 2)


def _k_facts(p, KCH: int) -> dict:
    nch = cdiv(p.Ctot, KCH)
    tail = p.Ctot % KCH
    return dict(KCH=KCH, nchunks=nch, k_tail=tail, k_lt_chunk=p.Ctot < KCH, tail_in_src2=p.C2 > 0 and tail > 0,
                chunk_straddles_sources=p.C2 > 0 and p.C1 % KCH != 0, mixed_pro=p.C2 > 0 and p.PRO2 != p.PRO1)


def _pix_facts(p, BM: int, BN: int) -> dict:
    return dict(BM=BM, BN=BN, n_mtiles=cdiv(p.M, BM), n_ntiles=cdiv(p.Ntot, BN), ragged_m=p.M % BM != 0, ragged_n=p.Ntot % BN != 0,
                images_per_tile=_images_per_tile(p, BN), span=_span(p, BN, False), nrep=p.NREP)


def _sp_facts(p, BM: int, BN: int, R: int, XW: int) -> dict:
    tx, ty = cdiv(p.WO, XW), cdiv(p.HO, R)
    return dict(BM=BM, BN=BN, n_mtiles=cdiv(p.M, BM), n_ntiles=p.B * tx * ty, ragged_m=p.M % BM != 0, R=R, XW=XW, tiles_x=tx, tiles_y=ty,
                partial_row=p.HO % R != 0, partial_col=p.WO % XW != 0, nrep=p.NREP)


# ---------------------------------------------------------------------------------------------------------------------------------
# csrc/conv_q4.hip
# ---------------------------------------------------------------------------------------------------------------------------------
def _ring_supported(p) -> bool:
    if p.res_mul:
        return False
    if p.MODE != MODE_CONV or p.KH != 1 or p.KW != 1 or p.S != 1 or p.C2 != 0 or p.GATE or p.PRO1 != PRO_NONE:
        return False
    if (p.HW & 3) or p.HO != p.H or p.WO != p.W:
        return False
    return True


def _ring_split(p, items: int, nchunks16: int) -> int:
    lim, cap, min_chunks, per = DMA_SPLIT
    sp = 1
    if p.SCRATCH and items < lim and nchunks16 >= min_chunks:
        sp = min(cap, min(nchunks16 // per, cdiv(lim, items)))
        if sp < 1:
            sp = 1
    return sp


def _ring_facts(p, BM: int, BN: int, sp: int, k32: bool) -> dict:
    KCH = 32 if k32 else 16
    f = _pix_facts(p, BM, BN)
    f.update(_k_facts(p, KCH))
    nch = f["nchunks"]
    lens = [((ks + 1) * nch) // sp - (ks * nch) // sp for ks in range(sp)]
    items = f["n_mtiles"] * f["n_ntiles"] * sp
    f.update(splits=sp, chunks_per_split=max(lens), short_last_split=min(lens) != max(lens), split_rule="ring" if sp > 1 else "",
             could_split=(not p.SCRATCH) and _ring_split_with_scratch(p, f["n_mtiles"] * f["n_ntiles"]) > 1,
             tepi=True, items=items, items_per_wg=items / N_CU, k32=k32)
    return f


def _ring_split_with_scratch(p, items: int) -> int:
    q = _P()
    q.SCRATCH = True
    return _ring_split(q, items, cdiv(p.Ctot, 16))


def _q4(p):
    if not _ring_supported(p) or p.M < Q4_MIN_M:
        return None
    a, b = Q4_RULE_A, Q4_RULE_B
    if not p.force_dma and not ((p.Ntot >= a[0] and p.M >= a[1] and p.Ctot < a[2]) or (p.Ntot <= b[0] and p.M <= b[1] and p.Ctot >= b[2])):
        return None
    nchunks = cdiv(p.Ctot, 16)
    pre = 2 if (p.RES or p.BETA) else (1 if p.BIAS else 0)
    fixed, split_extra, thin = Q4_COST
    best, best_sp, best_cost = -1, 1, 1e30
    for ci, (wm, wvm, wvn) in enumerate(Q4_CANDS):
        if pre == 2 and wm != 1:
            continue
        bm, bn = 32 * wm * wvm, 128 * wvn
        nmt = cdiv(p.M, bm)
        if nmt * bm > p.W_ST:
            continue
        nnt = cdiv(p.Ntot, bn)
        items = nmt * nnt
        sp = _ring_split(p, items, nchunks)
        rounds = float(cdiv(items * sp, 256))
        per_item = float(bm) * bn * (float(cdiv(nchunks, sp)) + fixed + (split_extra if sp > 1 else 0.0))
        cost = rounds * per_item * (thin if wm == 1 else 1.0)
        if cost < best_cost:
            best_cost, best, best_sp = cost, ci, sp
    if best < 0:
        return None
    wm, wvm, wvn = Q4_CANDS[best]
    bn = 128 * wvn
    if p.C1 * p.HW * 4 * _span(p, bn, False) >= SPAN_LIMIT:
        return None
    wide = wvn == 4
    k32 = (not wide) and p.Ctot > Q4_K32_MIN
    if wide and pre == 2:
        return None
    f = _ring_facts(p, 32 * wm * wvm, bn, best_sp, k32)
    f.update(PRE=pre)
    return Cv(Q4, "conv_q4_kernel", (wm, wvm, wvn, 3 if k32 else 4, pre, 32 if k32 else 16), **f)


# ---------------------------------------------------------------------------------------------------------------------------------
# csrc/conv_dma.hip
# ---------------------------------------------------------------------------------------------------------------------------------
def _dma(p):
    if not _ring_supported(p) or p.M < DMA_MIN_M:
        return None
    n_max, k_min, m_min = DMA_RULE
    if not p.force_dma and not (p.Ntot <= n_max and (p.Ctot >= k_min or p.M >= m_min)):
        return None
    nchunks = cdiv(p.Ctot, 16)
    pre = bool(p.BIAS or p.RES or p.BETA)
    fixed, split_extra, pm, pm0, pn, pn0 = DMA_COST
    best_wm, best_wn, best_sp, best_cost = 0, 0, 1, 1e30
    for wm in range(1, DMA_MAX_WM + 1):
        bm = 64 * wm
        nmt = cdiv(p.M, bm)
        if nmt * bm > p.W_ST:
            continue
        for wn in range(1, DMA_MAX_WN + 1):
            if wm == 5 and wn == 2:
                continue
            if pre and wm * wn > DMA_PRE_MAX_TILES:
                continue
            nnt = cdiv(p.Ntot, 64 * wn)
            items = nmt * nnt
            sp = _ring_split(p, items, nchunks)
            rounds = float(cdiv(items * sp, 256))
            per_item = float(bm) * 64 * wn * (float(cdiv(nchunks, sp)) + fixed + (split_extra if sp > 1 else 0.0))
            cost = rounds * per_item * (1.0 + pm * (pm0 - wm) + pn * (pn0 - wn))
            if cost < best_cost:
                best_cost, best_wm, best_wn, best_sp = cost, wm, wn, sp
    if not best_wm:
        return None
    bn = 64 * best_wn
    if p.C1 * p.HW * 4 * _span(p, bn, False) >= SPAN_LIMIT:
        return None
    big = best_wm == 5 or (best_wm == 4 and best_wn == 2)
    k32 = (not big) and p.Ctot > DMA_K32_MIN
    if pre and (best_wm, best_wn) in ((3, 2), (4, 2)):
        return None
    f = _ring_facts(p, 64 * best_wm, bn, best_sp, k32)
    f.update(PRE=int(pre))
    return Cv(DMA, "conv_dma_kernel", (best_wm, best_wn, 3 if k32 else 4, pre, 32 if k32 else 16), **f)


# ---------------------------------------------------------------------------------------------------------------------------------
# csrc/igemm_pc.hip
# ---------------------------------------------------------------------------------------------------------------------------------
def _pc_cv(p, bmode, wm, kch, r, xw, thin=False, narrow=False) -> Cv:
    BM = 32 if thin else wm * 64
    BN = 256 if thin else (64 if narrow else 128)
    args = (bmode, wm, kch, r, xw, p.PRO1, thin, narrow)
    f = _k_facts(p, kch)
    if bmode == BM_PIX:
        f.update(_pix_facts(p, BM, BN))
        f.update(tepi=True)
    else:
        f.update(_sp_facts(p, BM, BN, r, xw))
        f.update(tepi=xw % 4 == 0, r_capped=False)
    f.update(chunks_per_split=f["nchunks"])
    return Cv(PC, "conv_pc_kernel", args, **f)


def _pc(p):
    if p.MODE != MODE_CONV or p.S != 1 or p.GATE:
        return None
    if p.PRO1 not in PC_PRO:
        return None
    if p.C2 > 0 and p.PRO2 != p.PRO1:
        return None
    if p.M <= PC_THIN_MAX_M and p.KH == 3 and p.KW == 3:
        if p.HO != p.H or p.WO != p.W or p.PT != 1 or p.PL != 1 or p.WO % 64 != 0 or p.M < PC_THIN_MIN_M:
            return None
        n = p.B * (p.WO // 64) * cdiv(p.HO, 4)
        if n < PC_THIN_MIN_TILES:
            return None
        return _pc_cv(p, BM_SPATIAL, 1, PC_THIN_KCH, 4, 64, thin=True)
    if p.M < PC_MIN_M:
        return None
    bm = 128 if float(cdiv(p.M, 128) * 128) / p.M <= PC_BM_PAD else 64
    T = p.KH * p.KW
    if T == 1:
        if p.C2 != 0 or (p.HW & 3) or p.HO != p.H or p.WO != p.W:
            return None
        n_ntiles = cdiv(p.Ntot, 128)
        if cdiv(p.M, bm) * n_ntiles < PC_PIX_MIN_TILES:
            n64 = cdiv(p.Ntot, 64)
            if p.Ctot < PC_NARROW_MIN_K or cdiv(p.M, 64) * n64 < PC_NARROW_MIN_TILES:
                return None
            return _pc_cv(p, BM_PIX, 1, 32, 1, 64, narrow=True)
        if p.Ctot < PC_PIX_MIN_K:
            return None
        return _pc_cv(p, BM_PIX, 2 if bm == 128 else 1, PC_KCH1, 1, 64)
    if T != 9 or p.KH != 3 or p.HO != p.H or p.WO != p.W or p.PT != 1 or p.PL != 1:
        return None
    for (r, xw), widths in PC3_GEOMS:
        if (p.WO >= 64 and p.WO % 64 == 0) if widths == "mult64" else (p.WO in widths):
            n = p.B * cdiv(p.WO, xw) * cdiv(p.HO, r)
            if cdiv(p.M, bm) * n < PC3_MIN_TILES:
                return None
            kch = 8 if (PC_KCH3 == 8 or (PC_KCH3 == 4 and p.M >= PC_KCH3_WIDE_M)) else 4
            return _pc_cv(p, BM_SPATIAL, 2 if bm == 128 else 1, kch, r, xw)
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# csrc/igemm.hip
# ---------------------------------------------------------------------------------------------------------------------------------
def _generic_split(p, blocks: int, nchunks: int, scratch: bool) -> dict:
    out = dict(splits=1, chunks_per_split=nchunks)
    if not (scratch and p.MODE == MODE_CONV and nchunks >= SPLITK_MIN_CHUNKS):
        return out
    splits, rule = 1, ""
    if blocks <= SPLITK_A[0]:
        splits, rule = cdiv(SPLITK_A[1], blocks), "A"
    elif blocks <= SPLITK_B[0] and nchunks >= SPLITK_B[1]:
        splits, rule = cdiv(SPLITK_B[2], blocks), "B"
    cap8 = splits > SPLITK_MAX
    if cap8:
        splits = SPLITK_MAX
    cap_half = splits > nchunks // 2
    if cap_half:
        splits = nchunks // 2
    if splits > 1:
        cps = cdiv(nchunks, splits)
        n = cdiv(nchunks, cps)
        out.update(splits=n, chunks_per_split=cps, short_last_split=nchunks % cps != 0, split_rule=rule, split_cap8=cap8, split_cap_half=cap_half)
    return out


def _spatial_tiling(p, BN: int, cap: int):
    XW = p.WO if p.WO <= BN else BN
    R = BN // XW
    r_capped = R > p.HO
    if R > p.HO:
        R = p.HO
    if R < 1:
        R = 1
    r0 = R
    while True:
        IR = (R - 1) * p.S + p.KH
        IC = (XW - 1) * p.S + p.KW
        if IR * IC <= cap:
            break
        if R == 1:
            return None
        R -= 1
    return R, XW, r_capped, R < r0


def _generic_cv(p, bmode, tt, cfg, n_ntiles: int, allow_splitk: bool, bvec=False, tiling=None, declined=()) -> Cv:
    if bmode == BM_PIX:
        wm, wn, wvm, wvn, kch = cfg[:5]
        ept, minw = 1, 2
    else:
        wm, wn, wvm, wvn, kch, ept, minw = cfg
    BM, BN = wm * wvm * 32, wn * wvn * 32
    if bmode == BM_SPATIAL and p.GATE:
        raise ValueError("conv: SE gate is only supported on 1x1 convs")
    f = _k_facts(p, kch)
    if bmode == BM_PIX:
        f.update(_pix_facts(p, BM, BN))
    else:
        R, XW, r_capped, r_shrunk = tiling
        f.update(_sp_facts(p, BM, BN, R, XW))
        f.update(r_capped=r_capped, r_shrunk=r_shrunk)
    assert f["n_ntiles"] == n_ntiles, (f["n_ntiles"], n_ntiles)
    span = _span(p, BN, bmode == BM_SPATIAL)
    if max(p.C1, p.C2) * p.H * p.W * 4 * span >= SPAN_LIMIT:
        raise ValueError("conv: the image(s) one tile touches exceed 2 GiB")
    blocks = f["n_mtiles"] * n_ntiles
    f.update(_generic_split(p, blocks, f["nchunks"], bool(p.SCRATCH) and allow_splitk))
    if allow_splitk and not p.SCRATCH:
        f["could_split"] = _generic_split(p, blocks, f["nchunks"], True)["splits"] > 1
    tepi = (TEPI_BN[0] <= BN <= TEPI_BN[1] and f["splits"] == 1 and p.MODE != MODE_CONVT_SCATTER and
            ((bmode == BM_PIX and (p.HW & 3) == 0) or (bmode == BM_SPATIAL and (f["XW"] & 3) == 0 and (p.WO & 3) == 0)))
    f.update(tepi=tepi, bvec=bvec, span=span, declined=declined)
    return Cv(GENERIC, "conv_igemm_kernel", (bmode, tt, wm, wn, wvm, wvn, kch, ept, minw, bvec), **f)


def _generic(p, declined) -> Cv:
    T = p.KH * p.KW
    bm = pick_bm(p.M)
    if p.pix:
        tiles_big = cdiv(p.M, bm) * cdiv(p.Ntot, 128 if bm == 128 else 256)
        bvec = p.MODE != MODE_GATHER2X2 and (p.HW & 3) == 0
        if bm >= 64 and tiles_big < PIX_SMALL_TILES:
            cfg = PIX_SMALL
        elif bm == 128 and p.Ctot <= PIX_K16_MAX:
            cfg = PIX_128_K16
        elif bm == 128:
            cfg = PIX_128
        elif bm == 64:
            cfg = PIX_64
        else:
            cfg = PIX_32
        return _generic_cv(p, BM_PIX, 1, cfg, cdiv(p.Ntot, cfg[5]), cfg[6], bvec=bvec, declined=declined)
    if T != 9 or p.S > 2:
        raise ValueError(f"conv: unsupported kernel {p.KH}x{p.KW} stride {p.S}")
    out_px = p.B * p.HO * p.WO

    def go(cfg, BN):
        t = _spatial_tiling(p, BN, cfg[5] * NTHREADS)
        if t is None:
            return None
        n = p.B * cdiv(p.WO, t[1]) * cdiv(p.HO, t[0])
        return t, n

    if bm == 128:
        g = go(SP_128, 128)
        if g is None:
            raise ValueError("conv: halo tile does not fit")
        if g[1] * cdiv(p.M, 128) >= SP_MIN_TILES:
            return _generic_cv(p, BM_SPATIAL, 9, SP_128, g[1], False, tiling=g[0], declined=declined)
    if bm >= 64:
        if cdiv(p.M, 64) * cdiv(out_px, 256) >= SP_MIN_TILES:
            g = go(SP_64W, 256)
            if g is not None:
                return _generic_cv(p, BM_SPATIAL, 9, SP_64W, g[1], False, tiling=g[0], declined=declined)
        g = go(SP_64, 64)
        if g is None:
            raise ValueError("conv: halo tile does not fit")
        return _generic_cv(p, BM_SPATIAL, 9, SP_64, g[1], False, tiling=g[0], declined=declined)
    if p.S == 1 and cdiv(out_px, 512) >= SP_THIN_MIN:
        g = go(SP_THIN512, 512)
        if g is not None:
            return _generic_cv(p, BM_SPATIAL, 9, SP_THIN512, g[1], False, tiling=g[0], declined=declined)
    if p.S == 1 and cdiv(out_px, 1024) >= SP_THIN_MIN:
        g = go(SP_THIN1024, 1024)
        if g is not None:
            return _generic_cv(p, BM_SPATIAL, 9, SP_THIN1024, g[1], False, tiling=g[0], declined=declined)
    g = go(SP_32, 256)
    if g is None:
        raise ValueError("conv: halo tile does not fit")
    return _generic_cv(p, BM_SPATIAL, 9, SP_32, g[1], False, tiling=g[0], declined=declined)


# ---------------------------------------------------------------------------------------------------------------------------------
def dispatch(*, B, C1, H, W, M, C2=0, KH=1, KW=1, STRIDE=1, PAD_T=0, PAD_L=0, HO=None, WO=None, PRO1=PRO_NONE, PRO2=PRO_NONE,
             MODE=MODE_CONV, GATE=False, BIAS=False, RES=False, STATS=False, SCRATCH=False, BETA=0, YC=None, NREP=1, W_ST=None,
             X1_BF16=0, flags=0) -> Cv:
    """launch_conv (csrc/igemm.hip) on one CONV record.  ValueError where the launcher reports S2K_EINVAL."""
    if flags & (FLAG_BF16 | FLAG_SPLIT) or X1_BF16:
        raise NotImplementedError("FLAG_BF16 / FLAG_SPLIT / X1_BF16 stages belong to csrc/conv_bf16.hip: tests/b16_dispatch.conv restates its launchers")
    p = _P()
    p.B, p.C1, p.C2, p.H, p.W, p.M, p.KH, p.KW, p.S, p.PT, p.PL = B, C1, C2, H, W, M, KH, KW, STRIDE, PAD_T, PAD_L
    p.HO, p.WO = (H if HO is None else HO), (W if WO is None else WO)
    p.PRO1, p.PRO2, p.MODE, p.GATE, p.BIAS, p.RES, p.STATS, p.SCRATCH, p.BETA = PRO1, PRO2, MODE, bool(GATE), bool(BIAS), bool(RES), bool(STATS), bool(SCRATCH), BETA
    p.NREP = NREP if NREP > 0 else 1
    p.W_ST = (M + 127) // 128 * 128 if W_ST is None else W_ST
    p.YC = YC or M
    p.force_dma = bool(flags & FLAG_DMA)
    p.res_mul = bool(flags & FLAG_RES_GELU_GRAD)
    if p.res_mul and not p.RES:
        raise ValueError("conv: S2K_FLAG_RES_GELU_GRAD needs RES and an f32 stage")
    T = KH * KW
    p.Ctot, p.HW = C1 + C2, H * W
    if B <= 0 or C1 <= 0 or M <= 0 or H <= 0 or W <= 0:
        raise ValueError("conv: missing tensor or non-positive dimension")
    p.pix = (T == 1 and STRIDE == 1) or MODE != MODE_CONV
    if MODE != MODE_CONV:
        if T != 1 or STRIDE != 1 or C2 != 0 or p.HO != H or p.WO != W:
            raise ValueError("conv: scatter/gather modes are 1x1 over the low-resolution grid")
        if MODE == MODE_CONVT_SCATTER and ((M & 3) or BETA or STATS or RES):
            raise ValueError("conv: scatter needs M = 4*Cout, beta = 0, no stats, no residual")
        if MODE == MODE_GATHER2X2 and ((C1 & 3) or PRO1 != PRO_NONE or GATE):
            raise ValueError("conv: gather needs C1 = 4*Cout and no prologue")
    if p.pix and (p.HO != H or p.WO != W or PAD_T or PAD_L):
        raise ValueError("conv: 1x1 geometry mismatch")
    p.Ntot = B * p.HW
    if p.Ntot > 0x7fffffff:
        raise ValueError("conv: too many pixels")
    declined = []
    if flags & FLAG_Q4:
        cv = _q4(p)
        if cv is not None:
            return cv
        declined.append("q4")
    elif p.force_dma:
        cv = _dma(p)
        if cv is not None:
            return cv
        declined.append("dma (flagged)")
    cv = _pc(p)
    if cv is not None:
        cv.declined = tuple(declined)
        return cv
    declined.append("pc")
    cv = _dma(p)
    if cv is not None:
        cv.declined = tuple(declined)
        return cv
    declined.append("dma")
    return _generic(p, tuple(declined))
