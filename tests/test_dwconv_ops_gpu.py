"""Depthwise convolution (csrc/dwconv.hip), kernel by kernel: every template instantiation the three launchers reach, each case
pinned to the kernel family it must run on (s2k_program_profile_variants: 0 band kernels, 6 wave-per-channel plane kernels,
7 the weight gradient's image loop) and compared with the f32 oracle AND with a float64 run of it (Case.run ref64) at the bars of
tests/test_ops_gpu.py (1e-4; 2e-4 for the atomically summed weight gradient).

Each table row is (B, C, H, W, K, S, family); TF-SAME padding as the planner emits it.  tests/dw_dispatch.py restates the
launchers' arithmetic: which instantiation a row reaches and the run-time facts it exercises (row bands, chunks of (image, band)
items that span two images, the 48-wave cap of the plane weight gradient, images per workgroup of the image loop, the parity
bodies of dwconv_dgrad_s2_kernel, the stagers' wide-row loops).  tests/test_dwconv_dispatch_cpu.py checks, without a GPU, that
these tables reach every instantiation of the launch macros, every required edge, and every (op, instantiation) of the b5 256²
bs 32 and b0 224² bs 8 training plans at that plan's own geometry (the PROD_* tables)."""
import pytest

from s2lc_amd.plan import opdefs as D
from tests.dw_dispatch import BAND, IMAGE_LOOP, PLANE, dispatch
from tests.test_ops_gpu import Case, _dw_geo, _fold_fields, _shape_ids

pytestmark = pytest.mark.gpu

P, L = PLANE, IMAGE_LOOP

# ---- forward: dwconv_fwd_plane_kernel<K, PRO, W, R>, dwconv_fwd_plane_s2_kernel<K, PRO, WO, RO>, dwconv_fwd_kernel<K, S, PL, PRO>
FWD = [
    (9, 6, 8, 8, 3, 1, P),              # <3, 8, 8>: four planes per wave pass, the last pass partial; C % 4 != 0
    (13, 7, 8, 8, 5, 1, P),             # <5, 8, 8>
    (3, 7, 16, 16, 3, 1, P),            # <3, 16, 16>
    (4, 6, 16, 16, 5, 1, P),            # <5, 16, 16>
    (3, 5, 32, 32, 3, 1, P),            # <3, 32, 32>
    (2, 6, 32, 32, 5, 1, P),            # <5, 32, 32>
    (16, 201, 64, 64, 3, 1, P),         # <3, 64, 16>: bchunk 3 over 4 bands, chunks span two images
    (16, 201, 64, 64, 5, 1, P),         # <5, 64, 16>: likewise
    (2, 5, 128, 128, 3, 1, P),          # <3, 128, 8>: 16 bands, bchunk 2
    (18, 43, 128, 128, 3, 1, P),        # <3, 128, 8>: bchunk 3 over 16 bands
    (6, 5, 16, 16, 3, 2, P),            # s2 <3, 8, 8>
    (5, 6, 16, 16, 5, 2, P),            # s2 <5, 8, 8>
    (4, 7, 32, 32, 3, 2, P),            # s2 <3, 16, 16>
    (3, 6, 32, 32, 5, 2, P),            # s2 <5, 16, 16>
    (16, 201, 64, 64, 3, 2, P),         # s2 <3, 32, 8>: bchunk 3 over 2 bands
    (16, 201, 64, 64, 5, 2, P),         # s2 <5, 32, 8>: likewise
    (2, 6, 128, 128, 5, 2, P),          # s2 <5, 64, 4>
    (18, 43, 128, 128, 3, 2, P),        # s2 <3, 64, 4>: bchunk 3 over 16 bands
    (18, 43, 128, 128, 5, 2, P),        # s2 <5, 64, 4>: likewise
    (3, 7, 7, 7, 3, 1, BAND),           # <3, 1, 1>: 7 x 7 planes, several per workgroup
    (1, 3, 130, 70, 3, 1, BAND),        # <3, 1, 1>: 3 bands
    (1, 4, 300, 20, 3, 1, BAND),        # <3, 1, 1>: a tall plane, 2 bands
    (1, 4, 20, 300, 3, 1, BAND),        # <3, 1, 1>: rows of 300: the vector stager's plain loop
    (2, 8, 40, 40, 3, 2, BAND),         # <3, 2, 0>
    (1, 5, 200, 200, 3, 2, BAND),       # <3, 2, 0>: 10 bands
    (2, 6, 14, 15, 3, 2, BAND),         # <3, 2, 1>: odd width
    (1, 3, 161, 161, 3, 2, BAND),       # <3, 2, 1>: 7 bands
    (3, 16, 7, 7, 5, 1, BAND),          # <5, 1, 2>
    (1, 3, 130, 70, 5, 1, BAND),        # <5, 1, 2>: 3 bands
    (2, 3, 128, 128, 5, 1, BAND),       # <5, 1, 2>: 128² at k 5 has no plane kernel
    (1, 4, 20, 300, 5, 1, BAND),        # <5, 1, 2>: wide rows
    (2, 8, 56, 56, 5, 2, BAND),         # <5, 2, 1>: the b0 224² layer at 56 -> 28
    (1, 3, 200, 200, 5, 2, BAND),       # <5, 2, 1>: 10 bands
    (1, 6, 15, 13, 5, 2, BAND),         # <5, 2, 2>
    (1, 3, 161, 161, 5, 2, BAND),       # <5, 2, 2>: 7 bands
]

# ---- data gradient: dwconv_dgrad_plane_kernel, dwconv_dgrad_plane_s2_kernel, dwconv_dgrad_s1_kernel<K, PR, PRO>,
# dwconv_dgrad_s2_kernel<K> with its four (qy, qx) parity bodies
DGRAD = [
    (9, 6, 8, 8, 3, 1, P), (13, 7, 8, 8, 5, 1, P), (3, 7, 16, 16, 3, 1, P), (4, 6, 16, 16, 5, 1, P), (3, 5, 32, 32, 3, 1, P),
    (2, 6, 32, 32, 5, 1, P),
    (16, 201, 64, 64, 3, 1, P),         # <3, 64, 16>: chunks span two images
    (16, 201, 64, 64, 5, 1, P),         # <5, 64, 16>
    (18, 43, 128, 128, 3, 1, P),        # <3, 128, 8>
    (6, 5, 16, 16, 3, 2, P), (5, 6, 16, 16, 5, 2, P), (4, 7, 32, 32, 3, 2, P), (3, 6, 32, 32, 5, 2, P),
    (16, 201, 64, 64, 3, 2, P),         # s2 <3, 32, 8>: chunks span two images
    (16, 201, 64, 64, 5, 2, P),         # s2 <5, 32, 8>
    (2, 6, 128, 128, 5, 2, P),          # s2 <5, 64, 4>
    (18, 43, 128, 128, 3, 2, P),        # s2 <3, 64, 4>: chunks span two images
    (18, 43, 128, 128, 5, 2, P),        # s2 <5, 64, 4>
    (3, 7, 7, 7, 3, 1, BAND),           # s1 <3, 1>
    (1, 3, 130, 70, 3, 1, BAND),        # s1 <3, 1>: 3 bands
    (1, 4, 20, 300, 3, 1, BAND),        # s1 <3, 1>: wide rows
    (3, 16, 7, 7, 5, 1, BAND),          # s1 <5, 2>
    (1, 3, 130, 70, 5, 1, BAND),        # s1 <5, 2>: 3 bands
    (2, 3, 128, 128, 5, 1, BAND),       # s1 <5, 2>: 4 bands
    (2, 8, 40, 40, 3, 2, BAND),         # s2 <3>: parity (0, 0)
    (2, 6, 15, 14, 3, 2, BAND),         # s2 <3>: (1, 0)
    (2, 6, 14, 15, 3, 2, BAND),         # s2 <3>: (0, 1)
    (2, 6, 15, 15, 3, 2, BAND),         # s2 <3>: (1, 1)
    (1, 3, 130, 130, 3, 2, BAND),       # s2 <3>: 5 bands of 31 rows: (0, 0) and (1, 0) alternate; WO 65: the scalar stager's passes
    (1, 3, 130, 131, 3, 2, BAND),       # s2 <3>: (0, 1) and (1, 1) alternate
    (1, 3, 20, 300, 3, 2, BAND),        # s2 <3>: 2 bands of 13 rows, WO 150
    (2, 6, 15, 15, 5, 2, BAND),         # s2 <5>: (0, 0)
    (2, 6, 14, 15, 5, 2, BAND),         # s2 <5>: (1, 0)
    (2, 6, 15, 14, 5, 2, BAND),         # s2 <5>: (0, 1)
    (2, 8, 56, 56, 5, 2, BAND),         # s2 <5>: (1, 1), the b0 224² layer at 56 -> 28
    (1, 3, 130, 130, 5, 2, BAND),       # s2 <5>: (0, 1) and (1, 1) alternate
    (1, 3, 130, 131, 5, 2, BAND),       # s2 <5>: (0, 0) and (1, 0) alternate
]

# ---- weight gradient: dwconv_wgrad_plane_kernel, dwconv_wgrad_kernel<K, S, PL, PRO> per band and in its image loop
WGRAD = [
    (9, 6, 8, 8, 3, 1, P), (13, 7, 8, 8, 5, 1, P), (3, 7, 16, 16, 3, 1, P), (4, 6, 16, 16, 5, 1, P), (3, 5, 32, 32, 3, 1, P),
    (2, 6, 32, 32, 5, 1, P),
    (3, 6, 64, 64, 3, 1, P),            # <3, 64, 16>: bchunk 2
    (25, 3, 64, 64, 3, 1, P),           # <3, 64, 16>: the split capped at 48 waves, bchunk 3 over 4 bands
    (25, 3, 64, 64, 5, 1, P),           # <5, 64, 16>: likewise
    (2, 5, 128, 128, 3, 1, P),          # <3, 128, 8>
    (7, 5, 128, 128, 3, 1, P),          # <3, 128, 8>: capped, bchunk 3 over 16 bands
    (9, 2001, 7, 7, 3, 1, L),           # loop <3, 1, 1>: 2 images per workgroup, 9 images (ragged), 2001 % 16 channels
    (200, 41, 14, 14, 3, 1, L),         # loop <3, 1, 1>: 3 per workgroup, 200 images (ragged), 41 % 4 channels
    (9, 2001, 7, 7, 5, 1, L),           # loop <5, 1, 2>: 2, ragged
    (151, 41, 28, 28, 3, 2, L),         # loop <3, 2, 0>: 3, ragged
    (151, 41, 27, 27, 3, 2, L),         # loop <3, 2, 1>: 3, ragged
    (151, 41, 28, 28, 5, 2, L),         # loop <5, 2, 1>: 3, ragged
    (151, 41, 27, 27, 5, 2, L),         # loop <5, 2, 2>: 3, ragged
    (4, 6, 32, 32, 5, 2, L),            # loop <5, 2, 1>: one image per workgroup
    (1, 3, 130, 70, 3, 1, BAND),        # <3, 1, 1>: 3 bands
    (1, 4, 20, 300, 3, 1, BAND),        # <3, 1, 1>: wide rows
    (3, 6, 128, 128, 3, 2, BAND),       # <3, 2, 0>: 4 bands
    (1, 3, 131, 131, 3, 2, BAND),       # <3, 2, 1>: 5 bands
    (1, 3, 130, 70, 5, 1, BAND),        # <5, 1, 2>: 3 bands
    (2, 3, 128, 128, 5, 1, BAND),       # <5, 1, 2>: 4 bands
    (5, 7, 64, 64, 5, 2, BAND),         # <5, 2, 1>
    (1, 4, 20, 300, 5, 2, BAND),        # <5, 2, 1>: wide rows
    (1, 6, 15, 13, 5, 2, BAND),         # <5, 2, 2>
    (1, 3, 131, 131, 5, 2, BAND),       # <5, 2, 2>: 5 bands
]

# ---- the b5 256² bs 32 and b0 224² bs 8 training plans: one row per (op, instantiation) they run, at the plan's geometry and with
# the plan's own prologue (forward: SiLU with the input's BatchNorm finalize folded in wherever the plan folds it)
PROD_FWD = [   # (..., family, PRO, folded BN)
    (32, 24, 128, 128, 3, 1, P, 0, False),      # b5 <3, 128, 8>: bchunk 11 over 16 bands
    (32, 48, 128, 128, 3, 1, P, 2, True),
    (32, 144, 128, 128, 3, 2, P, 2, True),      # b5 s2 <3, 64, 4>: bchunk 12 over 16 bands
    (32, 240, 64, 64, 3, 1, P, 2, True),        # b5 <3, 64, 16>: bchunk 5 over 4 bands
    (32, 240, 64, 64, 5, 2, P, 2, True),        # b5 s2 <5, 32, 8>
    (32, 384, 32, 32, 3, 2, P, 2, True),        # b5 s2 <3, 16, 16>
    (32, 384, 32, 32, 5, 1, P, 2, True),        # b5 <5, 32, 32>
    (32, 768, 16, 16, 3, 1, P, 2, True),        # b5 <3, 16, 16>
    (32, 1056, 16, 16, 5, 1, P, 2, True),       # b5 <5, 16, 16>
    (32, 1056, 16, 16, 5, 2, P, 2, True),       # b5 s2 <5, 8, 8>
    (32, 3072, 8, 8, 3, 1, P, 2, True),         # b5 <3, 8, 8>
    (32, 1824, 8, 8, 5, 1, P, 2, True),         # b5 <5, 8, 8>
    (8, 32, 112, 112, 3, 1, BAND, 2, True),     # b0 <3, 1, 1>
    (8, 96, 112, 112, 3, 2, BAND, 2, True),     # b0 <3, 2, 0>
    (8, 144, 56, 56, 5, 2, BAND, 2, True),      # b0 <5, 2, 1>
    (8, 240, 28, 28, 5, 1, BAND, 2, True),      # b0 <5, 1, 2>
]
PROD_DGRAD = [   # (..., family, PRO, BETA)
    (32, 24, 128, 128, 3, 1, P, 0, 1),          # b5 <3, 128, 8>
    (32, 144, 128, 128, 3, 2, P, 2, 0),         # b5 s2 <3, 64, 4>
    (32, 240, 64, 64, 3, 1, P, 2, 0),           # b5 <3, 64, 16>
    (32, 240, 64, 64, 5, 2, P, 2, 0),           # b5 s2 <5, 32, 8>
    (32, 384, 32, 32, 3, 2, P, 2, 0),           # b5 s2 <3, 16, 16>
    (32, 384, 32, 32, 5, 1, P, 2, 0),           # b5 <5, 32, 32>
    (32, 768, 16, 16, 3, 1, P, 2, 0),           # b5 <3, 16, 16>
    (32, 1056, 16, 16, 5, 1, P, 2, 0),          # b5 <5, 16, 16>
    (32, 1056, 16, 16, 5, 2, P, 2, 0),          # b5 s2 <5, 8, 8>
    (32, 3072, 8, 8, 3, 1, P, 2, 0),            # b5 <3, 8, 8>
    (32, 1824, 8, 8, 5, 1, P, 2, 0),            # b5 <5, 8, 8>
    (8, 32, 112, 112, 3, 1, BAND, 2, 0),        # b0 s1 <3, 1>
    (8, 240, 28, 28, 5, 1, BAND, 2, 0),         # b0 s1 <5, 2>
    (8, 96, 112, 112, 3, 2, BAND, 2, 0),        # b0 s2 <3>: 4 bands of 36 rows, parity (0, 0)
    (8, 144, 56, 56, 5, 2, BAND, 2, 0),         # b0 s2 <5>: (1, 1)
    (8, 672, 14, 14, 5, 2, BAND, 2, 0),         # b0 s2 <5>: (1, 1), 7 -> 14
]
PROD_WGRAD = [   # (..., family, PRO)
    (32, 24, 128, 128, 3, 1, P, 0),             # b5 <3, 128, 8>: capped at 48 waves, bchunk 11 over 16 bands
    (32, 48, 128, 128, 3, 1, P, 2),
    (32, 240, 64, 64, 3, 1, P, 2),              # b5 <3, 64, 16>
    (32, 384, 32, 32, 5, 1, P, 2),              # b5 <5, 32, 32>
    (32, 768, 16, 16, 3, 1, P, 2),              # b5 <3, 16, 16>
    (32, 1056, 16, 16, 5, 1, P, 2),             # b5 <5, 16, 16>
    (32, 3072, 8, 8, 3, 1, P, 2),               # b5 <3, 8, 8>
    (32, 1824, 8, 8, 5, 1, P, 2),               # b5 <5, 8, 8>
    (32, 144, 128, 128, 3, 2, BAND, 2),         # b5 band <3, 2, 0>
    (32, 240, 64, 64, 5, 2, BAND, 2),           # b5 band <5, 2, 1> (the image loop's tile would not fit)
    (32, 384, 32, 32, 3, 2, L, 2),              # b5 loop <3, 2, 0>: 4 images per workgroup
    (32, 1056, 16, 16, 5, 2, L, 2),             # b5 loop <5, 2, 1>: 3 per workgroup, ragged
    (8, 32, 112, 112, 3, 1, BAND, 2),           # b0 band <3, 1, 1>
    (8, 240, 28, 28, 5, 1, L, 2),               # b0 loop <5, 1, 2>
    (8, 480, 14, 14, 3, 1, L, 2),               # b0 loop <3, 1, 1>: 2 images per workgroup
    (8, 96, 112, 112, 3, 2, BAND, 2),           # b0 band <3, 2, 0>
    (8, 240, 28, 28, 3, 2, L, 2),               # b0 loop <3, 2, 0>
    (8, 144, 56, 56, 5, 2, L, 2),               # b0 loop <5, 2, 1>
]

# ---- SiLU arguments past the fast exp's range: the input BatchNorm's scale x 100 drives u to hundreds; e^-u overflows for u < -88
SILU_RANGE = [
    ("fwd", (3, 7, 16, 16, 3, 1, P)), ("fwd", (2, 6, 14, 15, 3, 2, BAND)), ("fwd", (6, 5, 16, 16, 3, 2, P)),
    ("dgrad", (3, 7, 16, 16, 3, 1, P)), ("dgrad", (2, 6, 15, 15, 5, 2, BAND)), ("dgrad", (4, 7, 32, 32, 3, 2, P)),
    ("dgrad", (3, 16, 7, 7, 5, 1, BAND)),
    ("wgrad", (3, 7, 16, 16, 3, 1, P)), ("wgrad", (9, 2001, 7, 7, 3, 1, L)), ("wgrad", (1, 3, 131, 131, 3, 2, BAND)),
]


def _check_family(op, geo, fam):
    d = dispatch(op, *geo)
    assert d.family == fam, f"{op} {geo}: tests/dw_dispatch.py predicts family {d.family} ({d.kernel}{d.args}), the table says {fam}"
    return d


def _report(op, geo, d, errs):
    """one line per case (pytest -s): the measured errors against the f32 oracle and against float64"""
    print(f"\nDWERR {op} fam={d.family} {d.kernel}{d.args} {geo} " + " ".join(f"{k}={e32:.2e}/{e64:.2e}" for k, (e32, e64) in errs.items()))


def _bnv(c, C, mult):
    ref = c.bnv("bnv", C)
    if mult != 1.0:
        c.items["bnv"][1][0] *= mult
    return ref


def run_fwd(geo, fam, pro, fold=False, mult=1.0, seed=41):
    B, C, H, W, K, S = geo
    d = _check_family("fwd", geo, fam)
    g, Ho, Wo = _dw_geo(*geo)
    c = Case(seed)
    x = c.t("x", (B, C, H, W))
    w = c.t("w", (C, K, K), scale=0.3)
    y = c.t("y", (B, C, Ho, Wo), "nan")
    nrep = D.stats_replicas(C)
    st = c.t("stats", (nrep, 2, C), "zeros", "f64")
    outs, extra = ["y", "stats"], {}
    if fold:
        extra, bnv = _fold_fields(c, C, B * H * W, nrep)
        outs += ["bnv", "frm", "frv"]
    else:
        bnv = _bnv(c, C, mult) if pro else None
    errs = c.run("DWCONV_FWD", outs, 1e-4, sum0=("stats",), want_variant=fam, ref64=True, X=x, BNV=bnv, WT=w, Y=y, STATS=st, PRO=pro,
                 NREP=nrep, **extra, **g)
    _report("fwd", geo, d, errs)


def run_dgrad(geo, fam, pro, beta, mult=1.0, seed=42):
    B, C, H, W, K, S = geo
    d = _check_family("dgrad", geo, fam)
    g, Ho, Wo = _dw_geo(*geo)
    c = Case(seed)
    dy = c.t("dy", (B, C, Ho, Wo))
    w = c.t("w", (C, K, K), scale=0.3)
    xr = c.t("xraw", (B, C, H, W)) if pro else None
    bnv = _bnv(c, C, mult) if pro else None
    gg = c.t("g", (B, C, H, W), "randn" if beta else "nan")
    nrep = D.stats_replicas(C)
    st = c.t("stats2", (nrep, 2, C), "zeros", "f64") if pro else None
    outs = ["g"] + (["stats2"] if pro else [])
    errs = c.run("DWCONV_DGRAD", outs, 1e-4, sum0=("stats2",), want_variant=fam, ref64=True, DY=dy, WT=w, XRAW=xr, BNV=bnv, G=gg,
                 STATS2=st, PRO=pro, BETA=beta, NREP=nrep, **g)
    _report("dgrad", geo, d, errs)


def run_wgrad(geo, fam, pro, mult=1.0, seed=43):
    B, C, H, W, K, S = geo
    d = _check_family("wgrad", geo, fam)
    g, Ho, Wo = _dw_geo(*geo)
    c = Case(seed)
    dy = c.t("dy", (B, C, Ho, Wo))
    x = c.t("x", (B, C, H, W))
    bnv = _bnv(c, C, mult) if pro else None
    dw = c.t("dw", (C, K, K), "randn")
    errs = c.run("DWCONV_WGRAD", ["dw"], 2e-4, want_variant=fam, ref64=True, DY=dy, X=x, BNV=bnv, DW=dw, PRO=pro, **g)
    _report("wgrad", geo, d, errs)


@pytest.mark.parametrize("case", FWD, ids=_shape_ids(FWD, 6))
@pytest.mark.parametrize("pro", [D.PRO_NONE, D.PRO_SILU])
def test_dw_fwd(case, pro):
    run_fwd(case[:6], case[6], pro)


@pytest.mark.parametrize("case", FWD, ids=_shape_ids(FWD, 6))
def test_dw_fwd_folded_bn(case):
    run_fwd(case[:6], case[6], D.PRO_SILU, fold=True, seed=44)


@pytest.mark.parametrize("case", DGRAD, ids=_shape_ids(DGRAD, 6))
@pytest.mark.parametrize("pro,beta", [(D.PRO_NONE, 0), (D.PRO_NONE, 1), (D.PRO_SILU, 0), (D.PRO_SILU, 1)])
def test_dw_dgrad(case, pro, beta):
    run_dgrad(case[:6], case[6], pro, beta)


@pytest.mark.parametrize("case", WGRAD, ids=_shape_ids(WGRAD, 6))
@pytest.mark.parametrize("pro", [D.PRO_NONE, D.PRO_SILU])
def test_dw_wgrad(case, pro):
    run_wgrad(case[:6], case[6], pro)


@pytest.mark.parametrize("case", PROD_FWD, ids=_shape_ids(PROD_FWD, 6))
def test_dw_fwd_production(case):
    run_fwd(case[:6], case[6], case[7], fold=case[8], seed=45)


@pytest.mark.parametrize("case", PROD_DGRAD, ids=_shape_ids(PROD_DGRAD, 6))
def test_dw_dgrad_production(case):
    run_dgrad(case[:6], case[6], case[7], case[8], seed=46)


@pytest.mark.parametrize("case", PROD_WGRAD, ids=_shape_ids(PROD_WGRAD, 6))
def test_dw_wgrad_production(case):
    run_wgrad(case[:6], case[6], case[7], seed=47)


@pytest.mark.parametrize("op,case", SILU_RANGE, ids=[f"{op}-" + "-".join(map(str, case[:6])) for op, case in SILU_RANGE])
def test_dw_silu_beyond_exp_range(op, case):
    """1 / (1 + e^-u) with e^-u = inf must give SiLU 0 and a SiLU' of 0, not NaN"""
    if op == "fwd":
        run_fwd(case[:6], case[6], D.PRO_SILU, mult=100.0, seed=48)
    elif op == "dgrad":
        run_dgrad(case[:6], case[6], D.PRO_SILU, 1, mult=100.0, seed=48)
    else:
        run_wgrad(case[:6], case[6], D.PRO_SILU, mult=100.0, seed=48)
