"""Which kernel a CHAN_LN_FWD or MAE_LOSS_{FWD,BWD} stage runs in the product build, and how far the grid-stride kernels of
csrc/vit.hip reach in one trip, restated in plain Python from the launchers - test infrastructure.

    ln_rows(B, C, HW, aligned=True) -> LnRows or None      (ln_rows_geometry; None: the tile kernel runs)
    mae_vec(P, W, aligned=True) -> bool                    (mae_vec: the float4 form of mae_loss_rows_kernel)

In the product build tune_int() returns its default, so S2K_LN_ROWS is 1: the row kernel is taken only for HW % 4 == 0,
32 <= HW <= 64, C >= 64, B < 128 and 16-byte-aligned X / Y / MR.  The family codes are the ones the launchers leave in
g_s2k_variant (include/s2k.h): CHAN_LN_FWD 0 tile / 8 rows, MAE_LOSS_* 0 float4 / 9 scalar.
tests/test_vit_dispatch_cpu.py parses csrc/vit.hip for every constant used here and fails when one drifts."""
from __future__ import annotations

from dataclasses import dataclass

LN_TILE, LN_ROWS = 0, 8          # CHAN_LN_FWD families
MAE_VEC, MAE_SCALAR = 0, 9       # MAE_LOSS_FWD / _BWD families

LNR_NW = 16                      # waves per workgroup of the row kernel
LNR_US = 8                       # rows in flight per lane when summing over all channels
LN_ROWS_DEFAULT = 1              # tune_int("S2K_LN_ROWS", 1)
HW_MIN, HW_MAX = 32, 64          # row kernel: HW % 4 == 0 and HW in [HW_MIN, HW_MAX]
C_MIN = 64                       # ... C >= C_MIN
B_LIMIT = 128                    # ... B < B_LIMIT
WG_TARGET = 256                  # workgroups the channel split aims at: csplit = cdiv(WG_TARGET, B * pgroups), capped
CSPLIT_MAX = 8

# workgroups of one launch (the grid-stride kernels loop beyond) and work items per workgroup
GRID_CAP = {"chan_ln_fwd": 8192, "chan_ln_bwd": 1024, "act_bwd": 8192, "act_fwd": 8192, "token_gather": 8192, "token_scatter": 4096,
            "patchify": 16384, "ids_to_dec_idx": 4096}
PER_WG = {"chan_ln_fwd": 1, "chan_ln_bwd": 1, "act_bwd": 256, "act_fwd": 256, "token_gather": 256, "token_scatter": 4, "patchify": 256,
          "ids_to_dec_idx": 256}
MASK_INDEX_L_MAX = 12288         # mae_mask_index: one workgroup holds a sample's noise in LDS


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


@dataclass(frozen=True)
class LnRows:
    qw: int          # 16-byte columns of a row = lanes per row slot
    rw: int          # rows side by side in a wave
    pgroups: int     # position groups
    csplit: int      # channel splits of a sample
    rows_cs: int     # channels per split (the last one may be short)
    grid: int
    uneven: bool     # the last channel split is shorter than the others


def ln_rows(B: int, C: int, HW: int, aligned: bool = True) -> LnRows | None:
    if not LN_ROWS_DEFAULT or HW % 4 or HW < HW_MIN or HW > HW_MAX or C < C_MIN or B >= B_LIMIT or not aligned:
        return None
    ncol = HW // 4
    pgroups = cdiv(ncol, 64)
    qw = cdiv(ncol, pgroups)            # (the two-group form for qw > 32 needs HW > 128: not reachable in the product build)
    rw = 64 // qw
    rpi = LNR_NW * rw
    cs = cdiv(WG_TARGET, B * pgroups)
    cs = max(1, min(cs, min(CSPLIT_MAX, C // (rpi * 2))))
    return LnRows(qw, rw, pgroups, cs, cdiv(C, cs), 8 * pgroups * cs * cdiv(B, 8), cs > 1 and C % cs != 0)


def ln_family(B: int, C: int, HW: int, aligned: bool = True) -> int:
    return LN_ROWS if ln_rows(B, C, HW, aligned) is not None else LN_TILE


def mae_vec(P: int, W: int, aligned: bool = True) -> bool:
    return P % 4 == 0 and W % 4 == 0 and aligned


def mae_family(P: int, W: int, aligned: bool = True) -> int:
    return MAE_VEC if mae_vec(P, W, aligned) else MAE_SCALAR


def trips(kernel: str, items: int) -> int:
    """trips of the busiest workgroup's grid-stride loop over `items` work items (tiles, elements or rows)"""
    wgs = cdiv(items, PER_WG[kernel])
    return cdiv(wgs, min(wgs, GRID_CAP[kernel]))
