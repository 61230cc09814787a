"""TEST INFRASTRUCTURE ONLY - the layouts that WEIGHT_PACK, WGRAD_FINALIZE, SPACE_TO_DEPTH and IM2COL write, stated once more
without a GPU and without the kernels' index arithmetic.

Every function works from what the kernels receive - the table rows {src_off, dst_off, M, K, T, s_m, s_k, s_t, flip, MP, KP, start}
of a WEIGHT_PACK record, {off, M, C, T, start} of a WGRAD_FINALIZE record - and follows the layout COMMENTS of csrc/ew.hip,
csrc/conv_q4.hip, csrc/conv_bf16.hip and csrc/common.h (split_bf16x2): the logical weight is gathered as a (K, T, M) array, and
each layout is a zero-padded reshape / transpose of it.  Values are carried as their 32-bit patterns wherever they are only moved,
so that a comparison with a kernel's output is one of bytes (NaN payloads and signed zeros included).

A WEIGHT_PACK function returns its writes as a list of (byte offset from the record's DST, uint8 array): `apply` puts them into a
byte image of the arena.  The mirrors live at

    bf16   DST + BF16_BASE  + 2 * dst_off bytes   [KP/8][T][MP][8]        bf16, one 16-byte unit = eight consecutive input channels
    quad   DST + Q4_BASE    + 4 * dst_off bytes   [KP/8][MP][8]           f32, channels of a group in the order 0,2,4,6,1,3,5,7;
                                                                          only rows with T == 1 and bit 1 of `flip`
    split  DST + SPLIT_BASE + 6 * dst_off bytes   3 x [KP/8][T][MP][8]    bf16 planes hi / mid / lo, one after the other

bf16 rounding (round to nearest, ties to even) is stated twice - bf16_bits_torch (tensor.to(torch.bfloat16)) and bf16_bits_int
(the integer formula on the bit pattern); tests/test_pack_ref_cpu.py holds the two together."""
from __future__ import annotations

import numpy as np
import torch

Q4_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)      # position j of a quad group holds input channel Q4_ORDER[j]


# ---- bf16 rounding, twice ------------------------------------------------------------------------------------------------------------
def bf16_bits_torch(x: np.ndarray) -> np.ndarray:
    """f32 values -> bf16 bit patterns (uint16) through torch's conversion"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def bf16_bits_int(x: np.ndarray) -> np.ndarray:
    """f32 values -> bf16 bit patterns (uint16) on the bit pattern: add half an ulp of the kept part minus one, plus the kept part's
    last bit (so that a tie goes to the even neighbour), and drop the low 16 bits; a carry out of the significand moves into the
    exponent (0x7f7fffff -> Inf).  NaN: the upper half with the quiet bit set."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7fffffff) > 0x7f800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_value(bits: np.ndarray) -> np.ndarray:
    """bf16 bit patterns -> the f32 values they stand for"""
    return (bits.astype(np.uint32) << 16).view(np.float32)


def tie_vector() -> np.ndarray:
    """f32 values (as uint32 patterns, returned as float32) around the bf16 rounding rule: exact ties whose kept part is even (round
    down) and odd (round up), one f32 ulp either side of each, a carry into the exponent, +-0, +-Inf and +-0x7f7fffff (the largest
    finite f32, which rounds to Inf).  No denormals, and no value whose f32-split mid / lo terms are denormal."""
    pats = []
    for hi16 in (0x3f80, 0x3f81, 0x3fff, 0x4000, 0x4049, 0x42c8, 0x3eaa, 0x3a83, 0x4b7f, 0x3400):
        for low in (0x8000, 0x7fff, 0x8001, 0x0000, 0x0001, 0xffff, 0x4000, 0xc000):
            pats.append((hi16 << 16) | low)
    pats += [p | 0x80000000 for p in pats]
    pats += [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x7f7f0000, 0xff7f0000, 0x7f7f8000, 0x7f7f7fff]
    return np.array(pats, dtype=np.uint32).view(np.float32)


# ---- WEIGHT_PACK ---------------------------------------------------------------------------------------------------------------------
def _u32(a) -> np.ndarray:
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype.itemsize == 4
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def logical_weight(row, src) -> np.ndarray:
    """the (K, T, M) weight a row describes, as bit patterns: element (k, t, m) is float src_off + m*s_m + k*s_k + t*s_t of SRC, the
    taps reversed when bit 0 of `flip` is set"""
    src_off, _, M, K, T, s_m, s_k, s_t, flip = row[:9]
    at = (src_off + np.arange(K, dtype=np.int64)[:, None, None] * s_k + np.arange(T, dtype=np.int64)[None, :, None] * s_t
          + np.arange(M, dtype=np.int64)[None, None, :] * s_m)
    w = _u32(src)[at]
    return w[:, ::-1, :] if flip & 1 else w


def padded(row, src) -> np.ndarray:
    """[KP][T][MP]: the logical weight with rows K .. KP-1 and columns M .. MP-1 exactly +0.0"""
    M, K, T, MP, KP = row[2], row[3], row[4], row[9], row[10]
    p = np.zeros((KP, T, MP), dtype=np.uint32)
    p[:K, :, :M] = logical_weight(row, src)
    return p


def entry_floats(row) -> int:
    return row[10] * row[4] * row[9]


def _bytes(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def f32_pack(rows, src):
    """the f32 packs: [KP][T][MP] per entry at float dst_off of DST"""
    return [(4 * r[1], _bytes(padded(r, src))) for r in rows]


def _fragments(p: np.ndarray) -> np.ndarray:
    """[KP][T][MP] -> [KP/8][T][MP][8]: the eight consecutive input channels of one (tap, output row) side by side"""
    KP, T, MP = p.shape
    return p.reshape(KP // 8, 8, T, MP).transpose(0, 2, 3, 1)


def bf16_addr(base: int, dst_off: int) -> int:
    """byte offset from DST of an entry's bf16 copy: unit dst_off / 8 of the region at BF16_BASE, 16 bytes a unit"""
    assert dst_off % 8 == 0
    return base + 16 * (dst_off // 8)


def bf16_mirror(rows, src, base: int, rounding=bf16_bits_int):
    out = []
    for r in rows:
        frag = _fragments(padded(r, src)).view(np.float32)
        out.append((bf16_addr(base, r[1]), _bytes(rounding(frag))))
    return out


def q4_wanted(row) -> bool:
    return row[4] == 1 and bool(row[8] & 2)


def q4_addr(base: int, dst_off: int) -> int:
    """byte offset from DST of an entry's quad copy: f32 floats at Q4_BASE + 4 * dst_off"""
    return base + 4 * dst_off


def q4_mirror(rows, src, base: int):
    """[KP/8][MP][8] per wanted entry; every other row's mirror area is not written"""
    out = []
    for r in rows:
        if not q4_wanted(r):
            continue
        p = padded(r, src)[:, 0, :]                                             # T == 1: [KP][MP]
        KP, MP = p.shape
        groups = p.reshape(KP // 8, 8, MP)[:, list(Q4_ORDER), :]                 # position j <- channel Q4_ORDER[j]
        out.append((q4_addr(base, r[1]), _bytes(groups.transpose(0, 2, 1))))
    return out


def q4_decode(mirror_u32: np.ndarray, KP: int, MP: int) -> np.ndarray:
    """a quad copy back to [KP][MP]"""
    g = mirror_u32.reshape(KP // 8, MP, 8).transpose(0, 2, 1)                    # [group][position][m]
    back = np.empty_like(g)
    back[:, list(Q4_ORDER), :] = g
    return back.reshape(KP, MP)


def split_terms(x: np.ndarray, rounding=bf16_bits_int):
    """x = hi + mid + lo in three bf16 terms (as bit patterns): hi = bf16(x), mid = bf16(x - hi), lo = bf16((x - hi) - mid), the
    differences in f32; mid = lo = +0 where hi is not finite"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = rounding(x)
    hv = bf16_value(hi)
    fin = np.isfinite(hv)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(fin, x - np.where(fin, hv, np.float32(0)), np.float32(0)).astype(np.float32)
        mid = rounding(r)
        q = (r - bf16_value(mid)).astype(np.float32)
    lo = rounding(q)
    return hi, mid, lo


def split_addr(base: int, dst_off: int, plane: int, floats: int) -> int:
    """byte offset from DST of plane `plane` of an entry of `floats` f32 elements: unit 3 * dst_off / 8 + plane * floats / 8"""
    assert dst_off % 8 == 0 and floats % 8 == 0
    return base + 16 * (3 * dst_off // 8 + plane * floats // 8)


def split_mirror(rows, src, base: int, rounding=bf16_bits_int):
    out = []
    for r in rows:
        frag = _fragments(padded(r, src)).view(np.float32)
        for pl, bits in enumerate(split_terms(frag, rounding)):
            out.append((split_addr(base, r[1], pl, entry_floats(r)), _bytes(bits)))
    return out


def weight_pack_writes(rows, src, bf16_base=0, q4_base=0, split_base=0):
    """everything one WEIGHT_PACK record writes, as (byte offset from DST, bytes)"""
    w = f32_pack(rows, src)
    if bf16_base:
        w += bf16_mirror(rows, src, bf16_base)
    if q4_base:
        w += q4_mirror(rows, src, q4_base)
    if split_base:
        w += split_mirror(rows, src, split_base)
    return w


def apply(image: np.ndarray, dst_byte: int, writes) -> np.ndarray:
    """the writes put into a byte image whose byte `dst_byte` is the record's DST; regions must not overlap each other"""
    seen = np.zeros(image.size, dtype=bool)
    for off, b in writes:
        a = dst_byte + off
        assert 0 <= a and a + b.size <= image.size, "a write falls outside the image"
        assert not seen[a:a + b.size].any(), "two writes overlap"
        seen[a:a + b.size] = True
        image[a:a + b.size] = b
    return image


# ---- WGRAD_FINALIZE ------------------------------------------------------------------------------------------------------------------
def wgrad_fold(rows, wgs, grads) -> np.ndarray:
    """GRADS after the fold: per row {off, M, C, T, start} the scratch [T][M][C] at float `off` of WGS is added, as one f32 add per
    element, to the parameter-shaped [M][C][T] slice at float `off` of GRADS"""
    wgs = np.ascontiguousarray(wgs, dtype=np.float32).reshape(-1)
    out = np.array(grads, dtype=np.float32).reshape(-1).copy()
    for off, M, C, T, _ in rows:
        n = M * C * T
        scratch = wgs[off:off + n].reshape(T, M, C)
        out[off:off + n] = out[off:off + n] + scratch.transpose(1, 2, 0).reshape(-1)
    return out


# ---- SPACE_TO_DEPTH, IM2COL ----------------------------------------------------------------------------------------------------------
def space_to_depth(x: np.ndarray) -> np.ndarray:
    """[B][C][2H][2W] -> [B][4C][H][W]: output channel (c, dy, dx) holds pixel (2y + dy, 2x + dx) of input channel c"""
    B, C, H2, W2 = x.shape
    H, W = H2 // 2, W2 // 2
    return np.ascontiguousarray(x.reshape(B, C, H, 2, W, 2).transpose(0, 1, 3, 5, 2, 4)).reshape(B, 4 * C, H, W)


def im2col(x: np.ndarray, KH: int, KW: int, S: int, PT: int, PL: int, HO: int, WO: int) -> np.ndarray:
    """[B][C][H][W] -> [B][C*KH*KW][HO][WO]: row (c, ky, kx) holds x[c][yo*S + ky - PT][xo*S + kx - PL], +0.0 outside the map"""
    B, C, H, W = x.shape
    hp, wp = max((HO - 1) * S + KH, PT + H), max((WO - 1) * S + KW, PL + W)
    xp = np.zeros((B, C, hp, wp), dtype=x.dtype)
    xp[:, :, PT:PT + H, PL:PL + W] = x
    y = np.zeros((B, C, KH, KW, HO, WO), dtype=x.dtype)
    for ky in range(KH):
        for kx in range(KW):
            y[:, :, ky, kx] = xp[:, :, ky:ky + (HO - 1) * S + 1:S, kx:kx + (WO - 1) * S + 1:S]
    return y.reshape(B, C * KH * KW, HO, WO)


# ---- the stride patterns the planners hand to WEIGHT_PACK (plan/unet_plan.py, plan/vit_plan.py: pack_weight callers) -----------------
# pattern -> (the parameter tensor, does the row reach the LDS-transpose branch of weight_pack_kernel: (k, tap) contiguous in SRC)
PATTERNS = {
    "dense_fwd": ("[M][K][T] conv weight", True),                # (M, Ct, T, Ct*T, T, 1, 0)
    "linear_fwd": ("[M][K] Linear weight", True),                # (M, K, 1, K, 1, 1, 0)
    "linear_dgrad": ("[K][M] Linear weight, transposed", False),                        # (K', M', 1, 1, K', 1, 0)
    "concat_dgrad": ("[K][Ctot][T] conv weight, a channel slice, taps reversed", False),  # (Cs, M', T, T, Ctot*T, 1, 1) + c_off*T
    "convt_fwd": ("[K][M/4][2][2] ConvTranspose weight", False),  # (4*Cout, Cin, 1, 1, 4*Cout, 1, 0)
    "convt_dgrad": ("[M][K/4][2][2] ConvTranspose weight", True),  # (Cin, 4*Cout, 1, 4*Cout, 1, 1, 0)
}

# (pattern, M, K, T): M, K the row's own fields.  M in {24, 128, 130} (ragged / exact / one tile and a bit), K in {13, 64, 65, 200},
# every entry at most ~300k floats
SINGLE_ROWS = [
    ("dense_fwd", 24, 13, 1), ("dense_fwd", 128, 65, 1), ("dense_fwd", 130, 200, 1), ("dense_fwd", 128, 64, 9), ("dense_fwd", 130, 65, 9),
    ("dense_fwd", 24, 200, 9), ("dense_fwd", 24, 13, 25),
    ("linear_fwd", 24, 200, 1), ("linear_fwd", 130, 64, 1), ("linear_fwd", 128, 13, 1),
    ("linear_dgrad", 24, 65, 1), ("linear_dgrad", 130, 200, 1), ("linear_dgrad", 128, 64, 1),
    ("concat_dgrad", 24, 13, 1), ("concat_dgrad", 130, 65, 1), ("concat_dgrad", 128, 64, 9), ("concat_dgrad", 24, 200, 9),
    ("concat_dgrad", 130, 13, 9),
    ("convt_fwd", 24, 13, 1), ("convt_fwd", 128, 200, 1), ("convt_fwd", 128, 65, 1),
    ("convt_dgrad", 24, 64, 1), ("convt_dgrad", 130, 200, 1), ("convt_dgrad", 128, 64, 1),
]


def pattern_row(pattern: str, M: int, K: int, T: int):
    """-> (floats of the parameter tensor, [src_elem_off, M, K, T, s_m, s_k, s_t, flip]) of one planner pattern with row fields M, K"""
    if pattern == "dense_fwd":
        return M * K * T, [0, M, K, T, K * T, T, 1, 0]
    if pattern == "linear_fwd":
        assert T == 1
        return M * K, [0, M, K, 1, K, 1, 1, 0]
    if pattern == "linear_dgrad":          # the Linear is [K][M]: out = K, in = M
        assert T == 1
        return K * M, [0, M, K, 1, 1, M, 1, 0]
    if pattern == "concat_dgrad":          # the conv is [K][Ctot][T]; the slice c_off .. c_off + M of its input channels
        ctot, c_off = M + 11, 7
        return K * ctot * T, [c_off * T, M, K, T, T, ctot * T, 1, 1]
    if pattern == "convt_fwd":             # the ConvTranspose is [K = Cin][M = 4 * Cout]
        assert T == 1 and M % 4 == 0
        return K * M, [0, M, K, 1, 1, M, 1, 0]
    if pattern == "convt_dgrad":           # the ConvTranspose is [M = Cin][K = 4 * Cout]
        assert T == 1 and K % 4 == 0
        return M * K, [0, M, K, 1, K, 1, 1, 0]
    raise KeyError(pattern)


def table_rows(entries, dst_offs):
    """12-int table rows from [src_off, M, K, T, s_m, s_k, s_t, flip] entries and their dst_off: MP, KP and the running `start`"""
    rows, start = [], 0
    for (src_off, M, K, T, s_m, s_k, s_t, flip), d in zip(entries, dst_offs):
        MP, KP = (M + 127) // 128 * 128, (K + 63) // 64 * 64
        rows.append([src_off, d, M, K, T, s_m, s_k, s_t, flip, MP, KP, start])
        start += KP * T * MP
    return rows, start
