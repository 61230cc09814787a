"""Which depthwise kernel a DWCONV_{FWD,DGRAD,WGRAD} stage runs, restated in plain Python from the three launchers of
csrc/dwconv.hip (launch_dwconv_fwd / _dgrad / _wgrad) at their default tuning (tune_int defaults: S2K_DW_TARGET 4096,
S2K_DW_PLANE_WAVES 6144, S2K_DW_WGP_SPLIT_MAX 48, every S2K_DW_* switch on) - test infrastructure.

    dispatch(op, B, C, H, W, K, S) -> Dw

`op` is "fwd", "dgrad" or "wgrad"; the padding is TF-SAME (what every planned stage carries).  Besides the kernel family (the code
the launcher leaves in g_s2k_variant: 0 band kernels, 6 wave-per-channel plane kernels, 7 the weight gradient's image loop) and
the exact template instantiation, a Dw holds the run-time facts a test case has to reach: the row bands of the band kernels,
the chunk of (image, band) items a plane-kernel wave walks, the weight-gradient split cap, the image loop's images per
workgroup, the parity bodies of dwconv_dgrad_s2_kernel and whether a stager takes its plain (multi-pass) loop for wide rows."""
from __future__ import annotations

from dataclasses import dataclass, field

TARGET = 4096            # S2K_DW_TARGET
PLANE_WAVES = 6144       # S2K_DW_PLANE_WAVES
WGP_SPLIT_MAX = 48       # S2K_DW_WGP_SPLIT_MAX
LDS_BAND = 26 * 1024     # tile_rows: LDS bytes per band workgroup
LDS_MAX = 64 * 1024

BAND, PLANE, IMAGE_LOOP = 0, 6, 7     # kernel families (include/s2k.h, s2k_program_profile_variants)


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def same_pads(size: int, k: int, s: int) -> tuple[int, int]:
    """TF 'SAME': (output size, padding before) - plan/unet_plan.same_pads."""
    out = cdiv(size, s)
    return out, max((out - 1) * s + k - size, 0) // 2


def _pow2ceil(v: int) -> int:
    r = 1
    while r < v:
        r <<= 1
    return r


@dataclass
class Dw:
    op: str
    family: int
    kernel: str                       # template name in csrc/dwconv.hip
    args: tuple                       # its template arguments without PRO (dwconv_dgrad_s2_kernel: (K,))
    bands: int = 1                    # band kernels: row bands per plane; plane kernels: bands per image (W / R)
    rt: int = 0                       # band kernels: rows per band
    bchunk: int = 0                   # plane kernels: (image, band) items per wave
    spans: bool = False               # plane kernels, band form: some wave's chunk holds items of two images
    capped: bool = False              # plane weight gradient: the split hit WGP_SPLIT_MAX
    bloop: int = 0                    # image loop: images per workgroup
    ragged: bool = False              # image loop: the last workgroup has fewer than bloop images
    cgroups: int = 0                  # image loop: channel groups
    ppb: int = 0                      # band kernels / image loop: planes (channels) per workgroup
    parities: frozenset = field(default_factory=frozenset)   # dwconv_dgrad_s2_kernel: the (qy, qx) bodies its bands run
    wide: bool = False                # a band kernel's stager takes its plain loop for wide rows

    @property
    def inst(self) -> tuple:
        """(op, family, kernel, args): one template instantiation (the PRO argument aside) as the launcher reaches it."""
        return (self.op, self.family, self.kernel, self.args)


def _tile_rows(ho: int, wo: int, irt, lw: int, K: int, with_w: bool, vec: bool) -> dict:
    """launcher's tile_rows(): planes per workgroup, rows per band, LDS layout."""
    LW = (lw + 3) & ~3 if vec else lw | 1
    hw = ho * wo
    target = TARGET
    while True:
        if hw <= target:
            ppb, rt = min(target // hw, 32), ho
        else:
            ppb, rt = 1, max(target // wo, 1)
        irt_ = irt(rt)
        lds = (ppb * irt_ * LW + (ppb * K * K if with_w else 4 * K * K)) * 4
        if lds <= LDS_BAND or (ppb == 1 and rt == 1):
            break
        target >>= 1
    items = rt * cdiv(wo, 4)
    lpp = 64 if items >= 64 else _pow2ceil(items)
    # vector stager (LW % 4 == 0): a tile row is LW / 4 float4 slots, one pass of a lane group holds at most 64;
    # scalar stager (dgrad stride 2): LW floats, at most 64 per pass
    wide = (LW >> 2) > 64 if vec else LW > 64
    return dict(LW=LW, PPB=ppb, RT=rt, IRt=irt_, lds=lds, bands=cdiv(ho, rt), LPP=lpp, wide=wide)


def _chunks(n_items: int, bsplit: int, pw: int) -> tuple[int, int]:
    bchunk = cdiv(cdiv(n_items, bsplit), pw) * pw
    return bchunk, cdiv(n_items, bchunk)


def _spans(n_items: int, bchunk: int, nb: int) -> bool:
    """does some chunk [j * bchunk, (j + 1) * bchunk) of (image, band) items hold items of two images?"""
    return nb > 1 and any(lo // nb != (min(n_items, lo + bchunk) - 1) // nb for lo in range(0, n_items, bchunk))


def _plane(op: str, kernel: str, B: int, C: int, W: int, K: int, cap: bool) -> Dw:
    """stride 1, square W x W plane: dwconv_{fwd,dgrad,wgrad}_plane_kernel<K, PRO, W, R>"""
    pw = 4 if W == 8 else 1
    rows = 16 if W == 64 else 8 if W == 128 else W
    nb = W // rows
    n_items = B * nb
    bsplit = max(1, min(cdiv(n_items, 2 * pw), cdiv(PLANE_WAVES, C)))
    capped = cap and bsplit > WGP_SPLIT_MAX
    if cap:
        bsplit = min(bsplit, WGP_SPLIT_MAX)
    bchunk, _ = _chunks(n_items, bsplit, pw)
    return Dw(op, PLANE, kernel, (K, W, rows), bands=nb, bchunk=bchunk, spans=_spans(n_items, bchunk, nb), capped=capped)


def _plane_s2(op: str, kernel: str, B: int, C: int, WO: int, K: int) -> Dw:
    """stride 2, even square plane (2 WO)^2: dwconv_{fwd,dgrad}_plane_s2_kernel<K, PRO, WO, RO>"""
    pw = 4 if WO == 8 else 1
    ro = 4 if WO == 64 else 8 if WO == 32 else WO
    nb = WO // ro
    n_items = B * nb
    bsplit = max(1, min(cdiv(n_items, 2 * pw), cdiv(PLANE_WAVES, C)))
    bchunk, _ = _chunks(n_items, bsplit, pw)
    return Dw(op, PLANE, kernel, (K, WO, ro), bands=nb, bchunk=bchunk, spans=_spans(n_items, bchunk, nb))


def dispatch(op: str, B: int, C: int, H: int, W: int, K: int, S: int) -> Dw:
    HO, PT = same_pads(H, K, S)
    WO, PL = same_pads(W, K, S)
    sq = H == W
    if op in ("fwd", "dgrad", "wgrad") and S == 1 and sq and PT == PL == (K - 1) // 2 and (W in (8, 16, 32, 64) or (W == 128 and K == 3)):
        return _plane(op, f"dwconv_{op}_plane_kernel", B, C, W, K, cap=op == "wgrad")
    if op in ("fwd", "dgrad") and S == 2 and sq and H == 2 * HO and WO in (8, 16, 32, 64) and PT == PL == (K - 2) // 2:
        return _plane_s2(op, f"dwconv_{op}_plane_s2_kernel", B, C, WO, K)
    if op == "fwd":
        lw = 4 - PL + (cdiv(WO, 4) * 4 - 1) * S + K
        t = _tile_rows(HO, WO, lambda rt: (rt - 1) * S + K, lw, K, True, True)
        return Dw(op, BAND, "dwconv_fwd_kernel", (K, S, PL), bands=t["bands"], rt=t["RT"], ppb=t["PPB"], wide=t["wide"])
    if op == "wgrad":
        lw = 4 - PL + (cdiv(WO, 4) * 4 - 1) * S + K
        t = _tile_rows(HO, WO, lambda rt: (rt - 1) * S + K, lw, K, False, True)
        if t["bands"] == 1 and HO * WO <= 1024 and B > 1:
            ppb = 4 * (64 // t["LPP"])
            if (ppb * t["IRt"] * t["LW"] + ppb * K * K) * 4 <= LDS_MAX:
                cgroups = cdiv(C, ppb)
                bsplits = min(cdiv(768, cgroups), B)
                bloop = cdiv(B, max(bsplits, 1))
                return Dw(op, IMAGE_LOOP, "dwconv_wgrad_kernel", (K, S, PL), bands=1, rt=t["RT"], bloop=bloop, ragged=B % bloop != 0,
                          cgroups=cgroups, ppb=ppb, wide=t["wide"])
        return Dw(op, BAND, "dwconv_wgrad_kernel", (K, S, PL), bands=t["bands"], rt=t["RT"], ppb=t["PPB"], wide=t["wide"])
    if S == 1:
        pr = K - 1 - PL
        lw = 4 - pr + cdiv(W, 4) * 4 + K - 1
        t = _tile_rows(H, W, lambda rt: rt + K - 1, lw, K, True, True)
        return Dw(op, BAND, "dwconv_dgrad_s1_kernel", (K, pr), bands=t["bands"], rt=t["RT"], ppb=t["PPB"], wide=t["wide"])
    t = _tile_rows(H, W, lambda rt: (rt + K - 2) // 2 + 3, WO + 2, K, True, False)
    par = frozenset(((b * t["RT"] + PT) & 1, PL & 1) for b in range(t["bands"]))
    return Dw(op, BAND, "dwconv_dgrad_s2_kernel", (K,), bands=t["bands"], rt=t["RT"], ppb=t["PPB"], parities=par, wide=t["wide"])
