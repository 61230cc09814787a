"""The BatchNorm / squeeze-excitation / residual / reduction stages of csrc/ew.hip, pinned to the kernel that runs and taken through
every routing boundary and loop edge of their launchers: the wave-per-channel small-plane kernels (family 11) at every lanes-per-
plane count, with short, empty and single batch chunks and partial unrolled passes; the workgroup-per-plane kernels (12) with and
without their tail loop; channel_sum_rows_kernel (13) at batch sizes where only some waves take the unrolled loop; the SE backward
and parameter-gradient routes (14, 15) on both sides of Q = 64 and Q = 224; the generic kernels (0) in their float4, scalar and
chunked bodies; every prologue, the folded BN_FINALIZE, EVAL, OUT_BF16 and every recomputing form of BN_BWD_APPLY; UPSAMPLE_ZERO.

Every row states its kernel family (Case.run want_variant), is compared with oracle/ops_ref.py in f32 AND in float64, over the
whole output and per channel / per column against that part's own max |ref| (channel c of the inputs an output is linear in, and
of the BatchNorm shift, is scaled by 2^-(c mod 8), so a small channel really is small beside its neighbours), and must leave every
byte of the arena outside its outputs as uploaded (Case.run untouched).  Bars are the ones tests/test_ops_gpu.py has for the stage.
tests/ew_dispatch.py restates the launchers; tests/test_ew_dispatch_cpu.py checks the tables below against it without a GPU and
holds the f32 oracle alone to a quarter of each bar against float64 on every row's data."""
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import ops_ref
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan.program import Program
from tests.test_ops_gpu import WS, Case, _fold_fields

pytestmark = pytest.mark.gpu

NONE, AFF, SILU, RELU, GELU = D.PRO_NONE, D.PRO_AFFINE, D.PRO_SILU, D.PRO_RELU, D.PRO_GELU
KEEP = 0.5          # drop-connect keep rate of the rows with NOISE: floor(KEEP + noise) / KEEP is 0 or 2, exact in f32

# bars, as in tests/test_ops_gpu.py (of the output's max |ref|; here also per channel / column and against float64)
BAR = {"SE_POOL": 1e-5, "SE_BWD_REDUCE": 1e-4, "CHANNEL_SUM": 1e-4, "SE_BN_SUMS": 2e-4, "SE_BN_COMBINE": 1e-6, "BN_BWD_REDUCE": 1e-4,
       "BN_BWD_FINALIZE": 1e-5, "BN_BWD_APPLY": 1e-5, "BN_BWD_APPLY:recompute": 2e-5,
       # dY rounded to bf16 on store: an element within an ulp of a rounding boundary may land on the other neighbour (2^-8 relative)
       "BN_BWD_APPLY:bf16": 8e-3,
       "BN_RESIDUAL": 1e-6, "BN_RESIDUAL:fold": 1e-5, "BN_FINALIZE": 1e-5, "SE_FC": 1e-5, "SE_FC_BWD": 1e-4, "SE_FC_WGRAD": 1e-4,
       "UPSAMPLE_ZERO": 1e-30}


# ---------------------------------------------------------------------------------------------------------------
# tables: (fields, family).  The LARGE row (UPSAMPLE_ZERO's 68 MB output) runs without the float64 oracle.
# ---------------------------------------------------------------------------------------------------------------
def _pool(B, C, HW, PRO=SILU, FOLD=0, LARGE=False):
    return dict(B=B, C=C, HW=HW, PRO=PRO, FOLD=FOLD, LARGE=LARGE)


SE_POOL = [
    # family 11: lanes per plane 1 (HW 4), 4, 16 with idle lanes (36), 16, 64 with idle lanes (196), 64
    (_pool(2, 9, 4), 11), (_pool(70, 6, 4, NONE), 11), (_pool(9, 12, 16, AFF), 11), (_pool(5, 7, 36, RELU), 11),
    (_pool(25, 400, 64), 11),                    # bsplit 6, bper 5: the last batch chunk starts at B
    (_pool(3, 2052, 64), 11),                    # C >= 2048: one batch chunk
    (_pool(3, 10, 196), 11), (_pool(2, 24, 256, RELU), 11),
    (_pool(6, 20, 64, SILU, 3), 11), (_pool(4, 5, 16, SILU, 20), 11),        # folded BN_FINALIZE: replicas as scalar loads / wave sum
    # family 12: main loop only, a one-float4 tail for thread 0, a whole tail trip; B * C > 4
    (_pool(1, 3, 4096), 12), (_pool(2, 3, 4100, NONE), 12), (_pool(1, 2, 5120, RELU), 12), (_pool(2, 4, 4096, SILU, 9), 12),
    # family 0, float4 body
    (_pool(2, 5, 260), 0), (_pool(2, 6, 1024), 0), (_pool(2, 6, 1024, SILU, 10), 0), (_pool(1, 3, 4092, AFF), 0), (_pool(1, 11, 64), 0),
    # family 0, scalar body
    (_pool(3, 5, 49), 0), (_pool(2, 4, 63, RELU), 0), (_pool(3, 5, 49, SILU, 3), 0),
    # the plane bound of the workgroup-per-plane kernel: B * C = 8192 | 8193 (134 MB each; the float64 oracle of such a row takes
    # 0.3 s on 8 CPU threads, so these rows keep ref64)
    (_pool(1, 8192, 4096), 12), (_pool(1, 8193, 4096), 0),
]


def _sbr(B, C, HW, PRO=SILU):
    return dict(B=B, C=C, HW=HW, PRO=PRO)


SE_BWD_REDUCE = [(_sbr(2, 5, 4), 0), (_sbr(3, 1, 252, NONE), 0), (_sbr(2, 6, 1024, RELU), 0), (_sbr(1, 10, 1024), 0), (_sbr(3, 7, 49), 0),
                 (_sbr(2, 3, 49, NONE), 0), (_sbr(2, 5, 49, RELU), 0)]


def _cs(B, C, HW):
    return dict(B=B, C=C, HW=HW)


CHANNEL_SUM = ([(_cs(B, 256, 1), 13) for B in (1, 3, 4, 29, 32, 33, 36, 64, 67)] + [(_cs(B, 300, 65), 13) for B in (3, 29, 33, 67)]
               + [(_cs(B, 256, 512), 13) for B in (1, 4, 36)]
               + [(_cs(2, 255, 512), 0), (_cs(2, 256, 513), 0), (_cs(2, 3, 4096), 0), (_cs(2, 3, 4097), 0), (_cs(1, 5, 8196), 0)])

SE_BN_SUMS = [
    (_cs(2, 9, 4), 11), (_cs(64, 5, 16), 11), (_cs(65, 5, 16), 11), (_cs(5, 7, 36), 11), (_cs(25, 400, 64), 11), (_cs(2, 6, 64), 11),
    (_cs(16, 5, 64), 11), (_cs(17, 5, 64), 11),
    (_cs(16, 2052, 64), 11), (_cs(17, 2052, 64), 11),       # one batch chunk (C >= 2048): exactly four passes, four plus one
    (_cs(1, 3, 4096), 12), (_cs(2, 3, 4100), 12),
    (_cs(2, 5, 68), 0), (_cs(2, 6, 256), 0), (_cs(3, 5, 49), 0), (_cs(1, 11, 64), 0),
]


def _cmb(B, C, MUL, ADD):
    return dict(B=B, C=C, MUL=MUL, ADD=ADD)


SE_BN_COMBINE = [(_cmb(1, 5, True, True), 0), (_cmb(63, 6, True, False), 0), (_cmb(64, 7, False, True), 0), (_cmb(65, 5, False, False), 0),
                 (_cmb(65, 9, True, True), 0)]


def _red(B, C, HW, ACT, MUL, ADD, NOISE, NREP):
    return dict(B=B, C=C, HW=HW, ACT=ACT, MUL=MUL, ADD=ADD, NOISE=NOISE, NREP=NREP)


BN_BWD_REDUCE = [
    (_red(2, 5, 4, NONE, False, False, False, 1), 0), (_red(3, 6, 49, SILU, True, True, False, 8), 0),
    (_red(2, 3, 4096, RELU, False, False, True, 9), 0), (_red(2, 3, 4100, SILU, True, False, False, 64), 0),
    (_red(2, 2, 8193, NONE, False, True, True, 9), 0),             # scalar body, three chunks per plane
    (_red(2, 5, 49, GELU, True, True, False, 1), 0), (_red(2, 7, 16, RELU, True, False, False, 64), 0),
    (_red(4, 6, 64, NONE, False, False, True, 8), 0),
]

BN_BWD_FINALIZE = [(dict(C=C, NREP=n), 0) for C, n in ((1, 1), (5, 8), (70, 9), (5, 64), (70, 64))]


def _app(B, C, HW, FORM="fused", NREP=1, ACT=NONE, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=False):
    return dict(B=B, C=C, HW=HW, FORM=FORM, NREP=NREP, ACT=ACT, MUL=MUL, ADD=ADD, PS=PS, EVAL=EVAL, BF16=BF16, INPLACE=INPLACE)


def _rec(B, C, HW, MUL, ADD, PS, INPLACE, EVAL=0):
    return _app(B, C, HW, "fused", 1, SILU, MUL, ADD, PS, EVAL, 0, INPLACE)


BN_BWD_APPLY = [
    # COEF-table form: float4, scalar, chunked float4, chunked scalar
    (_app(2, 5, 16, "coef"), 0), (_app(3, 5, 49, "coef"), 0), (_app(2, 3, 4100, "coef"), 0), (_app(1, 2, 8193, "coef"), 0),
    # fused form, family 11: B = 2, 4 x planes per pass, that plus 1, the empty last chunk; NREP 1, 8, 9, 64
    (_app(2, 9, 4, NREP=1), 11), (_app(64, 5, 16, NREP=8), 11), (_app(65, 5, 16, NREP=9), 11), (_app(5, 7, 36, NREP=64), 11),
    (_app(25, 400, 64, NREP=10), 11), (_app(16, 5, 64, NREP=1), 11), (_app(17, 5, 64, NREP=9), 11),
    (_app(16, 2052, 64, NREP=1), 11), (_app(17, 2052, 64, NREP=2), 11),     # one batch chunk: exactly four passes, four plus one
    # fused form, family 0 (chunked rows: DGAMMA / DBETA must be added exactly once)
    (_app(2, 5, 68, NREP=1), 0), (_app(3, 5, 49, NREP=8), 0), (_app(2, 3, 4100, NREP=9), 0), (_app(1, 11, 64, NREP=64), 0),
    (_app(1, 2, 8193, NREP=2), 0),
    # 2048 planes of three chunks, more waves than the device holds at once: the chunks of one plane fall into neighbouring
    # workgroups that start at different times.  A second wave adding DGAMMA / DBETA is invisible where the chunks run side by
    # side - their non-atomic `+=` read the same old value and store the same sum - and shows here as doubled channels.
    (_app(1, 2048, 8196, NREP=2), 0),
    # EVAL: dY = A * g' only, DGAMMA / DBETA still added
    (_app(6, 5, 64, NREP=3, EVAL=1), 11), (_app(2, 5, 1024, NREP=9, EVAL=1), 0), (_rec(6, 5, 16, True, True, True, True, 1), 11),
    (_rec(2, 5, 256, True, True, True, True, 1), 0),
    # OUT_BF16
    (_app(6, 8, 64, NREP=2, BF16=1), 11), (_app(2, 5, 1024, NREP=16, BF16=1), 0), (_app(2, 3, 4100, NREP=3, BF16=1), 0),
    # recomputing (SiLU) form: STATS2 or PS; MULBC only, ADDBC only, both, neither; in place and out of place; B = 65 with PS
    (_rec(6, 5, 64, True, True, False, True), 11), (_rec(5, 7, 36, True, False, True, False), 11), (_rec(65, 5, 16, True, True, True, True), 11),
    (_rec(3, 6, 4, False, True, False, False), 11), (_rec(4, 5, 64, False, False, False, False), 11),
    (_rec(2, 5, 256, True, True, True, True), 0), (_rec(3, 5, 49, True, False, False, False), 0), (_rec(2, 3, 4100, False, True, True, True), 0),
    (_rec(65, 3, 68, True, True, True, False), 0), (_rec(2, 5, 68, False, False, False, True), 0),
]


def _res(B, C, HW, IDENT, NOISE, FOLD=0):
    return dict(B=B, C=C, HW=HW, IDENT=IDENT, NOISE=NOISE, FOLD=FOLD)


BN_RESIDUAL = [
    (_res(2, 9, 4, True, True), 11), (_res(5, 7, 36, False, False), 11), (_res(3, 10, 196, True, False), 11), (_res(2, 6, 256, False, True), 11),
    (_res(7, 5, 64, True, True), 11),                      # chunks of 4 and 3 samples
    (_res(6, 20, 64, True, True, 3), 11), (_res(25, 400, 64, True, True, 10), 11),
    (_res(2, 5, 260, True, True), 0), (_res(3, 5, 49, False, False), 0), (_res(2, 3, 4100, True, False), 0), (_res(1, 11, 64, True, False), 0),
    (_res(2, 6, 1024, True, True, 64), 0), (_res(3, 5, 49, False, True, 3), 0),
]


def _fin(C, NREP, TRAIN=1, COUNT=5000, NEG=False):
    return dict(C=C, NREP=NREP, TRAIN=TRAIN, COUNT=COUNT, NEG=NEG)


BN_FINALIZE = [(_fin(1, 1), 0), (_fin(5, 63), 0), (_fin(70, 64), 0), (_fin(5, 1, 0), 0), (_fin(70, 3, 0), 0),
               (_fin(5, 3, 1, 1), 0),                        # COUNT = 1: the unbiased factor count / max(count - 1, 1)
               (_fin(5, 2, 1, 5000, True), 0)]               # one channel whose q / n - mean^2 is negative by rounding

# (B, C, Q): Q 64 | 65 (se_fc_bwd_small_kernel), 224 | 225 (se_fc_wgrad_tile_kernel), Q = 1, Q % 4 != 0; sample chunks of 32
SE_FC = [(1, 3, 1), (32, 20, 6), (33, 100, 64), (64, 300, 65), (65, 12, 224), (2, 50, 225), (2, 3840, 160), (5, 257, 10)]


def _ups(B, C, H, W, S, HO, WO, LARGE=False):
    return dict(B=B, C=C, H=H, W=W, S=S, HO=HO, WO=WO, LARGE=LARGE)


UPSAMPLE_ZERO = [(_ups(2, 3, 8, 8, 2, 16, 16), 0), (_ups(2, 3, 8, 8, 2, 15, 15), 0),
                 (_ups(2, 5, 4, 6, 2, 10, 13), 0),           # rows / columns beyond S * H, S * W stay zero (the ys < H guard)
                 (_ups(1, 4, 5, 7, 3, 15, 21), 0), (_ups(1, 3, 5, 7, 3, 14, 20), 0),
                 (_ups(2, 64, 182, 182, 2, 364, 364, True), 0)]     # 16.96 M outputs > 65536 x 256: a second grid-stride trip (68 MB)

# ---------------------------------------------------------------------------------------------------------------
# Every (stage, family, form) of the b5 13x256^2 bs 32 and b0 224^2 bs 8 training plans, the eval-mode input-gradient plan and
# the Prithvi plans at that plan's own HW (Q for the SE stages), B and C cut down so that tests/ew_dispatch.py still returns the
# same family and loop facts (tests/test_ew_dispatch_cpu.py).  (stage, fields, family)
# ---------------------------------------------------------------------------------------------------------------
PROD = [
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=1024, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=12544, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=16384, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=196, FORM='fused', NREP=8, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=196, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=256, FORM='fused', NREP=8, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=256, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=3136, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=4096, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=49, FORM='fused', NREP=3, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=49, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=50176, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=64, FORM='fused', NREP=2, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 11),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=64, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 11),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=65536, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=784, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=1024, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=12544, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=16384, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=196, FORM='fused', NREP=8, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=196, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=256, FORM='fused', NREP=8, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=256, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=3136, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=4096, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=49, FORM='fused', NREP=3, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=49, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=50176, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=64, FORM='fused', NREP=2, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 11),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=64, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 11),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=65536, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=784, FORM='fused', NREP=9, ACT=0, MUL=False, ADD=False, PS=False, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=1024, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=12544, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=16384, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=196, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=3136, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=4096, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=49, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=64, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=1, BF16=0, INPLACE=True), 11),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=784, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=1, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=1024, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=12544, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=3, HW=16384, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=196, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=3136, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=4096, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=49, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=64, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=0, BF16=0, INPLACE=True), 11),
    ("BN_BWD_APPLY", dict(B=2, C=5, HW=784, FORM='fused', NREP=1, ACT=2, MUL=True, ADD=True, PS=True, EVAL=0, BF16=0, INPLACE=True), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=1024, ACT=0, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=3, HW=12544, ACT=0, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=3, HW=16384, ACT=0, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=196, ACT=0, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=256, ACT=0, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=3136, ACT=0, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=4096, ACT=0, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=49, ACT=0, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=64, ACT=0, MUL=False, ADD=False, NOISE=False, NREP=8), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=784, ACT=0, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=1024, ACT=0, MUL=False, ADD=False, NOISE=True, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=3, HW=16384, ACT=0, MUL=False, ADD=False, NOISE=True, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=196, ACT=0, MUL=False, ADD=False, NOISE=True, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=256, ACT=0, MUL=False, ADD=False, NOISE=True, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=3136, ACT=0, MUL=False, ADD=False, NOISE=True, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=4096, ACT=0, MUL=False, ADD=False, NOISE=True, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=49, ACT=0, MUL=False, ADD=False, NOISE=True, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=64, ACT=0, MUL=False, ADD=False, NOISE=True, NREP=8), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=784, ACT=0, MUL=False, ADD=False, NOISE=True, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=49, ACT=2, MUL=False, ADD=False, NOISE=False, NREP=3), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=64, ACT=2, MUL=False, ADD=False, NOISE=False, NREP=2), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=1024, ACT=3, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=3, HW=12544, ACT=3, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=3, HW=16384, ACT=3, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=196, ACT=3, MUL=False, ADD=False, NOISE=False, NREP=8), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=256, ACT=3, MUL=False, ADD=False, NOISE=False, NREP=8), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=3136, ACT=3, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=4096, ACT=3, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=3, HW=50176, ACT=3, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=3, HW=65536, ACT=3, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=5, HW=784, ACT=3, MUL=False, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_BWD_REDUCE", dict(B=2, C=3, HW=50176, ACT=3, MUL=True, ADD=False, NOISE=False, NREP=9), 0),
    ("BN_FINALIZE", dict(C=5, NREP=3, TRAIN=0, COUNT=5000, NEG=False), 0),
    ("BN_FINALIZE", dict(C=5, NREP=2, TRAIN=1, COUNT=5000, NEG=False), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=1024, IDENT=False, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=3, HW=12544, IDENT=False, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=3, HW=16384, IDENT=False, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=196, IDENT=False, NOISE=False, FOLD=0), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=256, IDENT=False, NOISE=False, FOLD=0), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=3136, IDENT=False, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=4096, IDENT=False, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=49, IDENT=False, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=64, IDENT=False, NOISE=False, FOLD=0), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=784, IDENT=False, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=1024, IDENT=False, NOISE=False, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=3, HW=12544, IDENT=False, NOISE=False, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=3, HW=16384, IDENT=False, NOISE=False, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=196, IDENT=False, NOISE=False, FOLD=9), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=256, IDENT=False, NOISE=False, FOLD=9), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=3136, IDENT=False, NOISE=False, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=4096, IDENT=False, NOISE=False, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=49, IDENT=False, NOISE=False, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=64, IDENT=False, NOISE=False, FOLD=8), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=64, IDENT=False, NOISE=False, FOLD=9), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=784, IDENT=False, NOISE=False, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=1024, IDENT=True, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=3, HW=16384, IDENT=True, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=196, IDENT=True, NOISE=False, FOLD=0), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=256, IDENT=True, NOISE=False, FOLD=0), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=3136, IDENT=True, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=4096, IDENT=True, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=49, IDENT=True, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=64, IDENT=True, NOISE=False, FOLD=0), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=784, IDENT=True, NOISE=False, FOLD=0), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=1024, IDENT=True, NOISE=True, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=3, HW=16384, IDENT=True, NOISE=True, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=196, IDENT=True, NOISE=True, FOLD=9), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=256, IDENT=True, NOISE=True, FOLD=9), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=3136, IDENT=True, NOISE=True, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=4096, IDENT=True, NOISE=True, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=49, IDENT=True, NOISE=True, FOLD=9), 0),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=64, IDENT=True, NOISE=True, FOLD=8), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=64, IDENT=True, NOISE=True, FOLD=9), 11),
    ("BN_RESIDUAL", dict(B=2, C=5, HW=784, IDENT=True, NOISE=True, FOLD=9), 0),
    ("CHANNEL_SUM", dict(B=2, C=5, HW=1024), 0),
    ("CHANNEL_SUM", dict(B=2, C=3, HW=12544), 0),
    ("CHANNEL_SUM", dict(B=2, C=3, HW=16384), 0),
    ("CHANNEL_SUM", dict(B=8, C=256, HW=196), 13),
    ("CHANNEL_SUM", dict(B=16, C=256, HW=196), 13),
    ("CHANNEL_SUM", dict(B=64, C=256, HW=196), 13),
    ("CHANNEL_SUM", dict(B=16, C=256, HW=200), 13),
    ("CHANNEL_SUM", dict(B=64, C=256, HW=200), 13),
    ("CHANNEL_SUM", dict(B=32, C=256, HW=256), 13),
    ("CHANNEL_SUM", dict(B=2, C=5, HW=3136), 0),
    ("CHANNEL_SUM", dict(B=2, C=5, HW=4096), 0),
    ("CHANNEL_SUM", dict(B=2, C=3, HW=50176), 0),
    ("CHANNEL_SUM", dict(B=64, C=256, HW=52), 13),
    ("CHANNEL_SUM", dict(B=2, C=3, HW=65536), 0),
    ("CHANNEL_SUM", dict(B=2, C=5, HW=784), 0),
    ("SE_BN_SUMS", dict(B=2, C=5, HW=1024), 0),
    ("SE_BN_SUMS", dict(B=2, C=3, HW=12544), 12),
    ("SE_BN_SUMS", dict(B=2, C=3, HW=16384), 12),
    ("SE_BN_SUMS", dict(B=2, C=5, HW=196), 0),
    ("SE_BN_SUMS", dict(B=2, C=5, HW=256), 0),
    ("SE_BN_SUMS", dict(B=2, C=5, HW=3136), 0),
    ("SE_BN_SUMS", dict(B=2, C=5, HW=4096), 12),
    ("SE_BN_SUMS", dict(B=2, C=5, HW=49), 0),
    ("SE_BN_SUMS", dict(B=2, C=5, HW=64), 11),
    ("SE_BN_SUMS", dict(B=2, C=5, HW=784), 0),
    ("SE_FC", dict(B=32, C=16, Q=10), 0),
    ("SE_FC", dict(B=32, C=16, Q=12), 0),
    ("SE_FC", dict(B=32, C=16, Q=128), 0),
    ("SE_FC", dict(B=32, C=16, Q=16), 0),
    ("SE_FC", dict(B=8, C=16, Q=20), 0),
    ("SE_FC", dict(B=8, C=16, Q=28), 0),
    ("SE_FC", dict(B=32, C=16, Q=32), 0),
    ("SE_FC", dict(B=8, C=16, Q=4), 0),
    ("SE_FC", dict(B=32, C=16, Q=44), 0),
    ("SE_FC", dict(B=8, C=16, Q=48), 0),
    ("SE_FC", dict(B=32, C=16, Q=6), 0),
    ("SE_FC", dict(B=32, C=16, Q=76), 0),
    ("SE_FC", dict(B=8, C=16, Q=8), 0),
    ("SE_FC_BWD", dict(B=32, C=16, Q=10, PARAMS=False), 14),
    ("SE_FC_BWD", dict(B=32, C=16, Q=12, PARAMS=False), 14),
    ("SE_FC_BWD", dict(B=32, C=16, Q=128, PARAMS=False), 0),
    ("SE_FC_BWD", dict(B=32, C=16, Q=16, PARAMS=False), 14),
    ("SE_FC_BWD", dict(B=8, C=16, Q=20, PARAMS=False), 14),
    ("SE_FC_BWD", dict(B=8, C=16, Q=28, PARAMS=False), 14),
    ("SE_FC_BWD", dict(B=32, C=16, Q=32, PARAMS=False), 14),
    ("SE_FC_BWD", dict(B=8, C=16, Q=4, PARAMS=False), 14),
    ("SE_FC_BWD", dict(B=32, C=16, Q=44, PARAMS=False), 14),
    ("SE_FC_BWD", dict(B=8, C=16, Q=48, PARAMS=False), 14),
    ("SE_FC_BWD", dict(B=32, C=16, Q=6, PARAMS=False), 14),
    ("SE_FC_BWD", dict(B=32, C=16, Q=76, PARAMS=False), 0),
    ("SE_FC_BWD", dict(B=8, C=16, Q=8, PARAMS=False), 14),
    ("SE_FC_WGRAD", dict(B=32, C=16, Q=10), 15),
    ("SE_FC_WGRAD", dict(B=32, C=16, Q=12), 15),
    ("SE_FC_WGRAD", dict(B=32, C=16, Q=128), 15),
    ("SE_FC_WGRAD", dict(B=32, C=16, Q=16), 15),
    ("SE_FC_WGRAD", dict(B=8, C=16, Q=20), 15),
    ("SE_FC_WGRAD", dict(B=8, C=16, Q=28), 15),
    ("SE_FC_WGRAD", dict(B=32, C=16, Q=32), 15),
    ("SE_FC_WGRAD", dict(B=8, C=16, Q=4), 15),
    ("SE_FC_WGRAD", dict(B=32, C=16, Q=44), 15),
    ("SE_FC_WGRAD", dict(B=8, C=16, Q=48), 15),
    ("SE_FC_WGRAD", dict(B=32, C=16, Q=6), 15),
    ("SE_FC_WGRAD", dict(B=32, C=16, Q=76), 15),
    ("SE_FC_WGRAD", dict(B=8, C=16, Q=8), 15),
    ("SE_POOL", dict(B=2, C=5, HW=1024, PRO=2, FOLD=0, LARGE=False), 0),
    ("SE_POOL", dict(B=2, C=3, HW=12544, PRO=2, FOLD=0, LARGE=False), 12),
    ("SE_POOL", dict(B=2, C=3, HW=16384, PRO=2, FOLD=0, LARGE=False), 12),
    ("SE_POOL", dict(B=2, C=5, HW=196, PRO=2, FOLD=0, LARGE=False), 11),
    ("SE_POOL", dict(B=2, C=5, HW=256, PRO=2, FOLD=0, LARGE=False), 11),
    ("SE_POOL", dict(B=2, C=5, HW=3136, PRO=2, FOLD=0, LARGE=False), 0),
    ("SE_POOL", dict(B=2, C=5, HW=4096, PRO=2, FOLD=0, LARGE=False), 12),
    ("SE_POOL", dict(B=2, C=5, HW=49, PRO=2, FOLD=0, LARGE=False), 0),
    ("SE_POOL", dict(B=2, C=5, HW=64, PRO=2, FOLD=0, LARGE=False), 11),
    ("SE_POOL", dict(B=2, C=5, HW=784, PRO=2, FOLD=0, LARGE=False), 0),
    ("SE_POOL", dict(B=2, C=5, HW=1024, PRO=2, FOLD=9, LARGE=False), 0),
    ("SE_POOL", dict(B=2, C=3, HW=12544, PRO=2, FOLD=9, LARGE=False), 12),
    ("SE_POOL", dict(B=2, C=3, HW=16384, PRO=2, FOLD=9, LARGE=False), 12),
    ("SE_POOL", dict(B=2, C=5, HW=196, PRO=2, FOLD=8, LARGE=False), 11),
    ("SE_POOL", dict(B=2, C=5, HW=196, PRO=2, FOLD=9, LARGE=False), 11),
    ("SE_POOL", dict(B=2, C=5, HW=256, PRO=2, FOLD=5, LARGE=False), 11),
    ("SE_POOL", dict(B=2, C=5, HW=256, PRO=2, FOLD=9, LARGE=False), 11),
    ("SE_POOL", dict(B=2, C=5, HW=3136, PRO=2, FOLD=9, LARGE=False), 0),
    ("SE_POOL", dict(B=2, C=5, HW=4096, PRO=2, FOLD=9, LARGE=False), 12),
    ("SE_POOL", dict(B=2, C=5, HW=49, PRO=2, FOLD=6, LARGE=False), 0),
    ("SE_POOL", dict(B=2, C=5, HW=64, PRO=2, FOLD=3, LARGE=False), 11),
    ("SE_POOL", dict(B=2, C=5, HW=784, PRO=2, FOLD=9, LARGE=False), 0),
    ("UPSAMPLE_ZERO", dict(B=1, C=2, H=112, W=112, S=2, HO=224, WO=224, LARGE=False), 0),
    ("UPSAMPLE_ZERO", dict(B=1, C=2, H=128, W=128, S=2, HO=256, WO=256, LARGE=False), 0),
]

TABLES = {"SE_POOL": SE_POOL, "SE_BWD_REDUCE": SE_BWD_REDUCE, "CHANNEL_SUM": CHANNEL_SUM, "SE_BN_SUMS": SE_BN_SUMS, "SE_BN_COMBINE": SE_BN_COMBINE,
          "BN_BWD_REDUCE": BN_BWD_REDUCE, "BN_BWD_FINALIZE": BN_BWD_FINALIZE, "BN_BWD_APPLY": BN_BWD_APPLY, "BN_RESIDUAL": BN_RESIDUAL,
          "BN_FINALIZE": BN_FINALIZE, "UPSAMPLE_ZERO": UPSAMPLE_ZERO}


def all_rows():
    """(stage, fields, family) of every table row; the SE_FC shapes as their three stages"""
    for kind, tab in TABLES.items():
        for kw, fam in tab:
            yield kind, kw, fam
    for B, C, Q in SE_FC:
        yield "SE_FC", dict(B=B, C=C, Q=Q), 0
        yield "SE_FC_BWD", dict(B=B, C=C, Q=Q, PARAMS=True), 14 if Q <= 64 else 0
        yield "SE_FC_BWD", dict(B=B, C=C, Q=Q, PARAMS=False), 14 if Q <= 64 else 0
        yield "SE_FC_WGRAD", dict(B=B, C=C, Q=Q), 15 if Q <= 224 else 0
    yield from PROD


def record_fields(kind, kw):
    """the row as the stage record names its fields (tensor fields: True where given), for tests/ew_dispatch.py"""
    f = {k: v for k, v in kw.items() if k in ("B", "C", "HW", "PRO", "ACT", "NREP", "EVAL", "H", "W", "S", "HO", "WO", "TRAIN")}
    t = lambda k: True if kw.get(k) else None      # noqa: E731
    if kind in ("SE_POOL", "BN_RESIDUAL"):
        f.update(FSTATS=t("FOLD"), FNREP=kw.get("FOLD", 0), IDENT=t("IDENT"), NOISE=t("NOISE"))
    if kind in ("BN_BWD_REDUCE", "SE_BN_COMBINE"):
        f.update(MULBC=t("MUL"), ADDBC=t("ADD"), NOISE=t("NOISE"))
    if kind == "BN_BWD_APPLY":
        f.update(COEF=True if kw["FORM"] == "coef" else None, MULBC=t("MUL"), ADDBC=t("ADD"), PS=t("PS"), OUT_BF16=kw["BF16"])
    if kind.startswith("SE_FC"):
        f.update(CSQ=kw["Q"], DW1=True if kw.get("PARAMS", True) else None)
    return f


# ---------------------------------------------------------------------------------------------------------------
# builders: a Case holding the row's tensors + what to run and compare
# ---------------------------------------------------------------------------------------------------------------
def colscale(C):
    return 0.5 ** (torch.arange(C) % 8).float()


def _noise(c, B):
    """alternating dropped / kept samples: floor(KEEP + 0.2) = 0, floor(KEEP + 0.8) = 1"""
    nz = torch.tensor([0.2 if b % 2 == 0 else 0.8 for b in range(B)])
    dcs = torch.floor(KEEP + nz)
    assert (dcs == 0).any() and (dcs == 1).any(), "a NOISE row needs a dropped and a kept sample"
    return c.t("noise", (B,), nz)


def _bnv(c, C, cs):
    ref = c.bnv("bnv", C)
    c.items["bnv"][1][1] *= cs          # the shift: u = scale * y + shift scales with its channel
    return ref


def _fold(c, C, n, nrep, cs):
    """_fold_fields with channel c's batch mean and FBETA scaled by cs[c]: shift = beta - mean * scale scales with its channel"""
    fold, bnv = _fold_fields(c, C, n, nrep)
    parts = c.items["fstats"][1]
    full = parts.sum(0)
    mean = full[0] / n
    var = full[1] / n - mean * mean
    new = torch.stack([mean * cs.double() * n, (var + (mean * cs.double()) ** 2) * n])
    parts *= (new / full).unsqueeze(0)
    c.items["fbeta"][1].mul_(cs)
    c.items["frm"][1].mul_(cs)
    return fold, bnv


def _st2(c, name, nrep, C, cs, positive=True):
    """STATS2 replicas with channel magnitudes 2^-(c mod 8); positive: no cancellation against the (positive) DGAMMA / DBETA they
    are added to, so that a per-element comparison of those is a statement about the sums"""
    v = torch.rand(nrep, 2, C, dtype=torch.float64, generator=c.gen) + 0.5 if positive else torch.randn(nrep, 2, C, dtype=torch.float64, generator=c.gen)
    return c.t(name, (nrep, 2, C), v * 3 * cs.double().view(1, 1, C), "f64")


def _scaled(c, name, shape, cs, axis=1, fill="randn", scale=1.0):
    """tensor `name` with index i of `axis` scaled by cs[i]"""
    g = (torch.rand if fill in ("rand", "pos") else torch.randn)(shape, generator=c.gen)
    if fill == "pos":
        g = g + 0.5
    elif fill == "off1":        # mixed signs around 1: sums over it do not cancel to nothing
        g = g + 1.0
    g = g * scale
    view = [1] * len(shape)
    view[axis] = shape[axis]
    return c.t(name, shape, g * cs.view(view))


def build(kind, kw, seed=0):
    """-> (Case, dict(outputs, tol, sum0, per_column, per_channel, pre, fields, kind, ref64)) for one table row"""
    c = Case(seed)
    s = dict(kind=kind, sum0=(), per_column=(), per_channel=(), pre=[], ref64=not kw.get("LARGE", False))
    B, C, HW = kw.get("B"), kw.get("C"), kw.get("HW")
    cs = colscale(C) if C else None
    if kind == "SE_POOL":
        y = _scaled(c, "y", (B, C, HW), cs)
        pool = c.t("pool", (B, C), "nan")
        if kw["FOLD"]:
            fold, bnv = _fold(c, C, B * HW, kw["FOLD"], cs)
            s.update(outputs=["pool", "bnv", "frm", "frv"], per_column=("pool", "bnv", "frm", "frv"))
        else:
            fold, bnv = {}, (_bnv(c, C, cs) if kw["PRO"] else None)
            if bnv is not None:     # a positive shift: a plane's mean must not cancel to nothing (POOL is compared per column over B rows, B = 1 included)
                c.items["bnv"][1][1] = c.items["bnv"][1][1].abs() + 0.5 * cs
            s.update(outputs=["pool"], per_column=("pool",))
        s.update(tol=BAR[kind], fields=dict(Y=y, BNV=bnv, POOL=pool, B=B, C=C, HW=HW, PRO=kw["PRO"], **fold))
    elif kind == "SE_BWD_REDUCE":
        g, y = _scaled(c, "g", (B, C, HW), cs), c.t("y", (B, C, HW))
        bnv = c.bnv("bnv", C) if kw["PRO"] else None
        s.update(outputs=["dgate"], per_column=("dgate",), tol=BAR[kind],
                 fields=dict(G=g, Y=y, BNV=bnv, DGATE=c.t("dgate", (B, C), "nan"), B=B, C=C, HW=HW, PRO=kw["PRO"]))
    elif kind == "CHANNEL_SUM":
        # (OUT [C] is compared element by element: values around +1 keep a sum of a few terms from cancelling to nothing, where the
        # f32 oracle's own rounding would be all that is left to compare)
        g = _scaled(c, "g", (B, C, HW), cs, fill="off1")
        out = _scaled(c, "out", (C,), cs, axis=0, fill="pos")          # OUT starts non-zero: the stage accumulates
        s.update(outputs=["out"], per_column=("out",), tol=BAR[kind], fields=dict(G=g, OUT=out, B=B, C=C, HW=HW))
    elif kind == "SE_BN_SUMS":
        g, y = _scaled(c, "g", (B, C, HW), cs), c.t("y", (B, C, HW))
        bnv = c.bnv("bnv", C)
        s.update(outputs=["dgate", "ps"], per_column=("dgate", "ps"), tol=BAR[kind],
                 fields=dict(G=g, Y=y, BNV=bnv, DGATE=c.t("dgate", (B, C), "nan"), PS=c.t("ps", (4, B, C), "nan"), B=B, C=C, HW=HW, ACT=D.ACT_SILU))
    elif kind == "SE_BN_COMBINE":
        ps = c.t("ps", (4, B, C), torch.randn(4, B, C, generator=c.gen) * 5 * torch.stack([cs, torch.ones(C), cs, torch.ones(C)]).view(4, 1, C))
        mul = c.t("mul", (B, C), "rand") if kw["MUL"] else None
        add = _scaled(c, "add", (B, C), cs) if kw["ADD"] else None
        s.update(outputs=["st2"], per_column=("st2",), tol=BAR[kind],
                 fields=dict(PS=ps, MULBC=mul, ADDBC=add, STATS2=c.t("st2", (2, C), "nan", "f64"), B=B, C=C, ADDSCALE=1.0 / 49))
    elif kind == "BN_BWD_REDUCE":
        g, y = _scaled(c, "g", (B, C, HW), cs), c.t("y", (B, C, HW))
        bnv = c.bnv("bnv", C)
        mul = c.t("mul", (B, C), "rand") if kw["MUL"] else None
        add = _scaled(c, "add", (B, C), cs, scale=float(HW)) if kw["ADD"] else None
        nz = _noise(c, B) if kw["NOISE"] else None
        nrep = kw["NREP"]
        s.update(outputs=["gout", "stats2"], sum0=("stats2",), per_column=("stats2",), per_channel=("gout",), tol=BAR[kind],
                 fields=dict(G=g, Y=y, BNV=bnv, MULBC=mul, ADDBC=add, NOISE=nz, GOUT=c.t("gout", (B, C, HW), "nan"),
                             STATS2=c.t("stats2", (nrep, 2, C), "zeros", "f64"), B=B, C=C, HW=HW, ACT=kw["ACT"], NREP=nrep, KEEP=KEEP,
                             ADDSCALE=1.0 / HW))
    elif kind == "BN_BWD_FINALIZE":
        nrep = kw["NREP"]
        st2, gam, bnv = _st2(c, "stats2", nrep, C, cs), c.t("gamma", (C,), "pos"), c.bnv("bnv", C)
        dg, db = _scaled(c, "dgamma", (C,), cs, 0, "pos"), _scaled(c, "dbeta", (C,), cs, 0, "pos")
        s.update(outputs=["dgamma", "dbeta", "coef"], per_column=("dgamma", "dbeta", "coef"), tol=BAR[kind],
                 fields=dict(STATS2=st2, GAMMA=gam, BNV=bnv, DGAMMA=dg, DBETA=db, COEF=c.t("coef", (3, C), "nan"), COUNT=777, C=C, NREP=nrep))
    elif kind == "BN_BWD_APPLY":
        gp, y = _scaled(c, "gp", (B, C, HW), cs, scale=0.3), c.t("y", (B, C, HW))
        bnv = c.bnv("bnv", C)
        if kw["FORM"] == "coef":
            coef = c.t("coef", (3, C), torch.randn(3, C, generator=c.gen) * torch.stack([torch.ones(C), cs, cs]))
            s.update(outputs=["dy"], per_channel=("dy",), tol=BAR[kind],
                     fields=dict(GP=gp, Y=y, BNV=bnv, COEF=coef, DY=c.t("dy", (B, C, HW), "nan"), B=B, C=C, HW=HW))
        else:
            rec = bool(kw["ACT"]) or kw["MUL"] or kw["ADD"]
            gam = c.t("gamma", (C,), "pos")
            dg, db = _scaled(c, "dgamma", (C,), cs, 0, "pos"), _scaled(c, "dbeta", (C,), cs, 0, "pos")      # start non-zero
            mul = c.t("mul", (B, C), "rand") if kw["MUL"] else None
            add = _scaled(c, "add", (B, C), cs, fill="rand", scale=float(HW)) if kw["ADD"] else None
            if kw["PS"]:
                ps = c.t("ps", (4, B, C), (torch.rand(4, B, C, generator=c.gen) + 0.5) * 3 * torch.stack([cs, torch.ones(C), cs, torch.ones(C)]).view(4, 1, C))
                st2 = None
            else:
                ps, st2 = None, _st2(c, "stats2", kw["NREP"], C, cs)
            dyname = "gp" if kw["INPLACE"] else "dy"
            dy = gp if kw["INPLACE"] else c.t("dy", (B, C, HW), "nan", "bf16" if kw["BF16"] else "f32")
            bar = BAR["BN_BWD_APPLY:bf16"] if kw["BF16"] else BAR["BN_BWD_APPLY:recompute"] if rec else BAR[kind]
            s.update(outputs=[dyname, "dgamma", "dbeta"], per_column=("dgamma", "dbeta"), per_channel=(dyname,), tol=bar,
                     fields=dict(GP=gp, Y=y, BNV=bnv, COEF=None, DY=dy, STATS2=st2, GAMMA=gam, DGAMMA=dg, DBETA=db, MULBC=mul, ADDBC=add, PS=ps,
                                 COUNT=B * HW, B=B, C=C, HW=HW, NREP=kw["NREP"], ACT=kw["ACT"], EVAL=kw["EVAL"], OUT_BF16=kw["BF16"],
                                 ADDSCALE=1.0 / HW))
    elif kind == "BN_RESIDUAL":
        y = _scaled(c, "y", (B, C, HW), cs)
        idt = _scaled(c, "ident", (B, C, HW), cs) if kw["IDENT"] else None
        nz = _noise(c, B) if kw["NOISE"] else None
        out = c.t("xout", (B, C, HW), "nan")
        if kw["FOLD"]:
            fold, bnv = _fold(c, C, B * HW, kw["FOLD"], cs)
            s.update(outputs=["xout", "bnv", "frm", "frv"], per_column=("bnv", "frm", "frv"), tol=BAR["BN_RESIDUAL:fold"])
        else:
            fold, bnv = {}, _bnv(c, C, cs)
            s.update(outputs=["xout"], tol=BAR[kind])
        s.update(per_channel=("xout",), fields=dict(Y=y, BNV=bnv, IDENT=idt, NOISE=nz, XOUT=out, B=B, C=C, HW=HW, KEEP=KEEP, **fold))
    elif kind == "BN_FINALIZE":
        n, nrep, eps = kw["COUNT"], kw["NREP"], 1e-5 if kw["NEG"] else 1e-3
        mean = torch.randn(C, dtype=torch.float64, generator=c.gen) * cs.double()
        var = torch.rand(C, dtype=torch.float64, generator=c.gen) + 0.1
        full = torch.stack([mean * n, (var + mean * mean) * n])
        if kw["NEG"]:
            # a constant plane of 1e6: n * mean^2 = 5e15, and q eight ulps below it; var comes out as -1e-3 .. -2e-3, beyond EPS = 1e-5
            m = 1.0e6
            full[0, 2], full[1, 2] = m * n, (n * m * m) * (1.0 - 8 * 2.0 ** -52)
            assert full[1, 2].item() / n - (full[0, 2].item() / n) ** 2 < -eps, "the float64 variance of channel 2 is not negative"
            parts = full.unsqueeze(0).repeat(nrep, 1, 1) / nrep          # (nrep = 2: halving is exact)
        else:
            parts = torch.rand(nrep, 2, C, dtype=torch.float64, generator=c.gen) + 0.5
            parts = parts / parts.sum(0, keepdim=True) * full
        train = kw["TRAIN"]
        stats = c.t("stats", (nrep, 2, C), parts, "f64") if train else None
        gam, bet = c.t("gamma", (C,), "pos"), _scaled(c, "beta", (C,), cs, 0)
        rm, rv = _scaled(c, "rm", (C,), cs, 0), c.t("rv", (C,), "pos")
        s.update(outputs=["bnv", "rm", "rv"], per_column=("bnv", "rm", "rv"), tol=BAR[kind],
                 fields=dict(STATS=stats, GAMMA=gam, BETA=bet, RM=rm, RV=rv, BNV=c.t("bnv", (4, C), "nan"), COUNT=n, C=C, TRAIN=train, NREP=nrep,
                             EPS=eps, MOM=0.01))
    elif kind == "SE_FC":
        Q = kw["Q"]
        qs = colscale(Q)
        pool = c.t("pool", (B, C), "rand")
        # (W1 / B1 positive: a column of HPRE holds B values, one at B = 1 - a dot product that cancels would leave the f32 oracle's
        # own rounding as the yardstick)
        w1, b1 = _scaled(c, "w1", (Q, C), qs, 0, "rand", scale=2.0 / C), _scaled(c, "b1", (Q,), qs, 0, "rand")
        w2, b2 = c.t("w2", (C, Q), scale=Q ** -0.5), c.t("b2", (C,))
        s.update(outputs=["hpre", "gate"], per_column=("hpre", "gate"), tol=BAR[kind],
                 fields=dict(POOL=pool, W1=w1, B1=b1, W2=w2, B2=b2, HPRE=c.t("hpre", (B, Q), "nan"), GATE=c.t("gate", (B, C), "nan"), B=B, C=C, CSQ=Q))
    elif kind in ("SE_FC_BWD", "SE_FC_WGRAD"):
        Q = kw["Q"]
        # (DGATE, W1, W2 and the bias gradients positive: the [C] / [Q] outputs are compared element by element or over B = 1, 2 rows,
        # and sums of a few signed terms that cancel would be compared with their own rounding noise)
        dgate, gate = _scaled(c, "dgate", (B, C), cs, fill="pos"), c.t("gate", (B, C), "rand")
        hpre, pool = c.t("hpre", (B, Q)), _scaled(c, "pool", (B, C), cs, fill="rand")
        w1, w2 = _scaled(c, "w1", (Q, C), cs, fill="rand", scale=C ** -0.5), c.t("w2", (C, Q), "rand", scale=Q ** -0.5)
        dw1, db1, dw2, db2 = _scaled(c, "dw1", (Q, C), cs), c.t("db1", (Q,), "pos"), c.t("dw2", (C, Q)), _scaled(c, "db2", (C,), cs, 0, "pos")
        dpool, hs = c.t("dpool", (B, C), "nan"), c.t("hs", (B, Q), "nan")
        bwd = dict(DGATE=dgate, GATE=gate, HPRE=hpre, POOL=pool, W1=w1, W2=w2, DW1=dw1, DB1=db1, DW2=dw2, DB2=db2, DPOOL=dpool, HS=hs, B=B, C=C, CSQ=Q)
        cols = ("dw1", "db1", "dw2", "db2", "dpool", "hs", "dgate", "hpre")
        if kind == "SE_FC_BWD" and kw.get("PARAMS", True):
            s.update(outputs=list(cols), per_column=cols, tol=BAR[kind], fields=bwd)
        elif kind == "SE_FC_BWD":
            bwd.update(DW1=None, DB1=None, DW2=None, DB2=None)
            s.update(outputs=["dpool", "hs", "dgate", "hpre"], per_column=("dpool", "hs", "dgate", "hpre"), tol=BAR[kind], fields=bwd)
        else:   # the split form the planner emits: data gradient first, parameter gradients as a stage of their own
            bwd.update(DW1=None, DB1=None, DW2=None, DB2=None)
            s.update(outputs=list(cols), per_column=cols, tol=BAR[kind], pre=[("SE_FC_BWD", bwd)],
                     fields=dict(DGP=dgate, HS=hs, DHP=hpre, POOL=pool, DW1=dw1, DB1=db1, DW2=dw2, DB2=db2, B=B, C=C, CSQ=Q))
    elif kind == "UPSAMPLE_ZERO":
        H, W, S, HO, WO = kw["H"], kw["W"], kw["S"], kw["HO"], kw["WO"]
        x = c.t("x", (B, C, H, W))
        s.update(outputs=["y"], tol=BAR[kind], fields=dict(X=x, Y=c.t("y", (B, C, HO, WO), "nan"), B=B, C=C, H=H, W=W, S=S, HO=HO, WO=WO))
    else:
        raise KeyError(kind)
    return c, s


def row_seed(kind, kw):
    """a seed per row (stable across runs and processes); SEEDS overrides it where the f32 oracle alone came too close to a bar"""
    key = (kind,) + tuple(sorted((k, v) for k, v in kw.items()))
    return SEEDS.get(key, 1 + sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key))) % 9973)


SEEDS: dict = {}


def row_id(kind, kw):
    parts = []
    for k, v in kw.items():
        if isinstance(v, bool):
            if v:
                parts.append(k)
        elif v is not None and (v != 0 or k in ("PRO", "ACT")):
            parts.append(f"{k}{v}")
    return kind + ":" + "-".join(parts)


def program_of(s):
    prog = Program()
    for k, f in s["pre"]:
        prog.add(k, **f)
    prog.add(s["kind"], **s["fields"])
    return prog


def cpu_images(c: Case, packed):
    """byte images of the f32 oracle and the float64 oracle over the case's arena (what Case.execute builds, without a GPU)"""
    cpu = torch.zeros(c.arena.top + 256, dtype=torch.uint8)
    wide = torch.zeros(2 * cpu.numel(), dtype=torch.uint8)
    for name, (ref, data) in c.items.items():
        cpu[ref.off:ref.off + ref.nbytes] = data.contiguous().reshape(-1).view(torch.uint8)
        wdt = {"f32": torch.float64, "bf16": torch.float32}.get(ref.dtype)
        b = (data.to(wdt) if wdt is not None else data).contiguous().reshape(-1).view(torch.uint8)
        wide[2 * ref.off:2 * ref.off + b.numel()] = b
    ops_ref.run_program(packed, {WS: wide}, D, wide=True)
    ops_ref.run_program(packed, {WS: cpu}, D)
    return cpu, wide


def oracle_alone(c: Case, s):
    """{output: worst figure} of the f32 oracle against the float64 oracle under the norms the GPU row is held to: the whole
    tensor and, where the row asks for them, per column / per channel"""
    cpu, wide = cpu_images(c, program_of(s).pack())
    out = {}
    for name in s["outputs"]:
        ref, _ = c.items[name]
        a, t = c.read(cpu, name).double(), c.read(wide, name, wide=True)
        if ref.dtype == "bf16":     # a value the stage rounds on store: the wide image holds it unrounded (as f32) - round it the same way
            t = t.to(torch.bfloat16)
        t = t.double()
        if name in s["sum0"]:
            a, t = a.sum(0), t.sum(0)
        fig = [((a - t).abs().max() / t.abs().max().clamp_min(1e-20)).item()]
        if name in s["per_column"] or name in s["per_channel"]:
            if name in s["per_column"]:
                pa, pt = a.reshape(-1, ref.shape[-1]), t.reshape(-1, ref.shape[-1])
            else:
                n = ref.shape[1]
                pa, pt = (v.reshape(ref.shape[0], n, -1).transpose(0, 1).reshape(n, -1).t() for v in (a, t))
            fig.append(((pa - pt).abs().amax(0) / pt.abs().amax(0).clamp_min(1e-20)).max().item())
        out[name] = max(fig)
    return out


WORST: dict = {}       # (stage, output) -> worst (f32 oracle, float64) figure over the rows run so far, whole tensor and parts


def run_row(kind, kw, fam):
    c, s = build(kind, kw, row_seed(kind, kw))
    fams = fam
    if s["pre"]:       # SE_FC_WGRAD behind its SE_FC_BWD
        fams = [14 if kw["Q"] <= 64 else 0, fam]
    errs = c.run(kind, s["outputs"], s["tol"], sum0=s["sum0"], pre=s["pre"], want_variant=fams, per_column=s["per_column"], ref64=s["ref64"],
                 per_channel=s["per_channel"], untouched=True, **s["fields"])
    for name, (e32, e64) in errs.items():
        p32, p64 = c.parts.get(name, (0.0, None))
        w = WORST.setdefault((kind + (" bf16" if kw.get("BF16") else ""), name), [0.0, 0.0])
        w[0], w[1] = max(w[0], e32, p32 or 0.0), max(w[1], e64 or 0.0, p64 or 0.0)
        print(f"{row_id(kind, kw)} {name}: whole {e32:.2e} / {e64 if e64 is None else format(e64, '.2e')}, parts {p32:.2e} / {p64 if p64 is None else format(p64, '.2e')}"
              f" (bar {s['tol']:.0e})")
    return c, s


def _params(rows):
    rows = list(rows)
    return dict(argnames="kind,kw,fam", argvalues=rows, ids=[row_id(k, kw) for k, kw, _ in rows])


# every row of all_rows() - hand tables and PROD - belongs to exactly one of the three row tests (tests/test_ew_dispatch_cpu.py checks it)
OWN_TEST = {"BN_FINALIZE": "test_bn_finalize_row", "UPSAMPLE_ZERO": "test_upsample_zero_exact"}       # every other stage: test_stage_row


def rows_of(test):
    return [(k, kw, f) for k, kw, f in all_rows() if OWN_TEST.get(k, "test_stage_row") == test]


@pytest.mark.parametrize(**_params(rows_of("test_stage_row")))
def test_stage_row(kind, kw, fam):
    run_row(kind, kw, fam)


@pytest.mark.parametrize(**_params(rows_of("test_bn_finalize_row")))
def test_bn_finalize_row(kind, kw, fam):
    c, s = run_row(kind, kw, fam)
    if kw["NEG"]:       # the clamped channel: var = 0, invstd = 1 / sqrt(eps)
        bnv = c.read(c.got, "bnv")
        want = torch.tensor(1.0 / (float(torch.tensor(1e-5, dtype=torch.float32)) ** 0.5), dtype=torch.float32)
        assert abs(bnv[3, 2].item() - want.item()) <= 2.0 ** -23 * want.item(), (bnv[3, 2].item(), want.item())


@pytest.mark.parametrize(**_params(rows_of("test_upsample_zero_exact")))
def test_upsample_zero_exact(kind, kw, fam):
    """bit-exact (tolerance as in test_ops_gpu.py::test_im2col_exact): data movement and zeros"""
    c, s = run_row(kind, kw, fam)


def test_chunked_apply_adds_the_parameter_gradients_once():
    """HW > 4096: several waves per plane form the same coefficients; only the one of chunk 0, sample 0 may add DGAMMA / DBETA"""
    kw = _app(2, 3, 4100 * 3, NREP=9)
    c, s = build("BN_BWD_APPLY", kw, 5)
    dg0, db0 = c.items["dgamma"][1].clone().double(), c.items["dbeta"][1].clone().double()
    st = c.items["stats2"][1].sum(0)
    c.run("BN_BWD_APPLY", s["outputs"], s["tol"], per_column=s["per_column"], per_channel=s["per_channel"], ref64=True, want_variant=0,
          untouched=True, **s["fields"])
    got = c.got
    for name, before, add in (("dgamma", dg0, st[1]), ("dbeta", db0, st[0])):
        inc = c.read(got, name).double() - before
        assert ((inc - add).abs() <= 1e-6 * add.abs()).all(), f"{name}: added {inc / add} times the sum"


# ---------------------------------------------------------------------------------------------------------------
# BN_FINALIZE folded into SE_POOL / BN_RESIDUAL against the stand-alone stage, on the same statistics
# ---------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """|a - b| in units of the f32 spacing at b"""
    _, e = torch.frexp(b.double().abs().clamp_min(1e-300))
    return ((a.double() - b.double()).abs() / torch.pow(2.0, (e - 24).double())).max().item()


@pytest.mark.parametrize("C,nrep,B,HW", [(21, 3, 4, 64), (9, 20, 3, 1024)], ids=["nrep3-small", "nrep20-generic"])
def test_folded_bn_finalize_agrees_with_the_stage(C, nrep, B, HW):
    """mean and invstd within 1 f32 ulp (both round a float64 value accurate to ~1e-14), scale within 2 (one more f32 product),
    shift within 4 * 2^-24 * (|beta| + |mean * scale|), RM / RV within 2 ulp.  Channel 2 is a constant plane of 1e6 whose float64
    variance is negative by rounding: clamped to 0 by all three."""
    n, eps = B * HW, 1e-5
    res = {}
    for which in ("BN_FINALIZE", "SE_POOL", "BN_RESIDUAL"):
        c = Case(77)
        fold, bnv = _fold_fields(c, C, n, nrep)
        parts = c.items["fstats"][1]
        m = 1.0e6
        parts[:, 0, 2], parts[:, 1, 2] = m * n / nrep, (n * m * m) * (1.0 - 8 * 2.0 ** -52) / nrep
        q, s_ = parts[:, 1, 2].sum().item(), parts[:, 0, 2].sum().item()
        assert q / n - (s_ / n) ** 2 < -eps, "the float64 variance of channel 2 is not negative"
        fold["FEPS"] = eps
        y = c.t("y", (B, C, HW))
        if which == "BN_FINALIZE":
            prog = ("BN_FINALIZE", dict(STATS=fold["FSTATS"], GAMMA=fold["FGAMMA"], BETA=fold["FBETA"], RM=fold["FRM"], RV=fold["FRV"], BNV=bnv,
                                        COUNT=n, C=C, TRAIN=1, NREP=nrep, EPS=eps, MOM=fold["FMOM"]))
        elif which == "SE_POOL":
            prog = ("SE_POOL", dict(Y=y, BNV=bnv, POOL=c.t("pool", (B, C), "nan"), B=B, C=C, HW=HW, PRO=SILU, **fold))
        else:
            prog = ("BN_RESIDUAL", dict(Y=y, BNV=bnv, IDENT=None, NOISE=None, XOUT=c.t("xout", (B, C, HW), "nan"), B=B, C=C, HW=HW, KEEP=1.0, **fold))
        p = Program()
        p.add(prog[0], **prog[1])
        got, _, _ = c.execute(p.pack(), oracle=False)
        res[which] = {k: c.read(got, k).clone() for k in ("bnv", "frm", "frv")}
        res[which]["beta"] = c.items["fbeta"][1].clone()
    ref = res["BN_FINALIZE"]
    assert torch.isfinite(ref["bnv"]).all()
    assert abs(ref["bnv"][3, 2].item() - eps ** -0.5) <= 1e-6 * eps ** -0.5, "channel 2: invstd is not 1 / sqrt(eps)"
    for which in ("SE_POOL", "BN_RESIDUAL"):
        got = res[which]
        assert torch.isfinite(got["bnv"]).all(), which
        assert _ulps(got["bnv"][2], ref["bnv"][2]) <= 1 and _ulps(got["bnv"][3], ref["bnv"][3]) <= 1, which
        assert _ulps(got["bnv"][0], ref["bnv"][0]) <= 2, which
        lim = 4 * 2.0 ** -24 * (ref["beta"].double().abs() + (ref["bnv"][2].double() * ref["bnv"][0].double()).abs())
        assert ((got["bnv"][1].double() - ref["bnv"][1].double()).abs() <= lim).all(), which
        assert _ulps(got["frm"], ref["frm"]) <= 2 and _ulps(got["frv"], ref["frv"]) <= 2, which


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    """after the module's rows: the worst figure per (stage, output), whole tensor and parts (shown with pytest -s)"""
    yield
    for (kind, name), (e32, e64) in sorted(WORST.items()):
        print(f"WORST {kind} {name}: {e32:.2e} (f32 oracle) / {e64:.2e} (float64)")
