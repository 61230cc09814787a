"""GPU: the small-plane depthwise backward chain as one kernel (csrc/dwconv.hip, dw_bwd_chain_kernel; opdefs.FLAG_CHAIN).

A four-record program - BN_BWD_APPLY (depthwise BatchNorm, g' recomputed from the SE backward's plane sums), DWCONV_WGRAD, DWCONV_DGRAD
(SiLU, statistics), BN_BWD_APPLY (expand BatchNorm) - runs through `s2k_program_run` with the flag on its first record and must report
kernel family 10 on all four records; the same program without the flag, and flagged programs the executor has to decline, must run on
the kernels of the single stages.  Either way G, the depthwise BatchNorm's dY (written in place over d), dw and both dgamma / dbeta
pairs are compared with the emulator's record-by-record run in f32 and in f64, at the bars of tests/test_ops_gpu.py and
tests/test_dwconv_ops_gpu.py (1e-4 of the tensor's max; 2e-4 for dw).  The emulator's own f32 run is within 6e-7 of its f64 run on
these shapes, so the bars hide nothing."""
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan.program import Program
from tests.test_ops_gpu import Case, _dw_geo

pytestmark = pytest.mark.gpu

FUSED = [10, 10, 10, 10]
BARS = {"g": 1e-4, "d": 1e-4, "dw": 2e-4, "dgamma1": 1e-4, "dbeta1": 1e-4, "dgamma2": 1e-4, "dbeta2": 1e-4, "stats2": 1e-4}


def _chain(B, C, W, K, S=1, beta=0, flag=True, nrec=4, seed=41):
    """The chain over an expanded tensor [B][C][W][W] (stride S: the depthwise output is W / S wide).  Returns (case, packed records)."""
    geo, Ho, Wo = _dw_geo(B, C, W, W, K, S)
    c = Case(seed)
    d = c.t("d", (B, C, Ho, Wo))                                   # upstream gradient; dY of the depthwise BatchNorm in place
    ydw = c.t("ydw", (B, C, Ho, Wo))
    bnv1, gam1 = c.bnv("bnv1", C), c.t("gamma1", (C,), "pos")
    mul, add = c.t("mul", (B, C), "rand"), c.t("add", (B, C))
    ps = c.t("ps", (4, B, C), scale=3.0)
    dg1, db1 = c.t("dgamma1", (C,)), c.t("dbeta1", (C,))           # random: a missing += shows
    x = c.t("x", (B, C, W, W))
    bnv2, gam2 = c.bnv("bnv2", C), c.t("gamma2", (C,), "pos")
    w = c.t("w", (C, K, K), scale=0.3)
    dw = c.t("dw", (C, K, K))
    g = c.t("g", (B, C, W, W), "randn" if beta else "nan")
    nrep = D.stats_replicas(C)
    st2 = c.t("stats2", (nrep, 2, C), "zeros", "f64")
    dg2, db2 = c.t("dgamma2", (C,)), c.t("dbeta2", (C,))
    prog = Program()
    prog.add("BN_BWD_APPLY", GP=d, Y=ydw, BNV=bnv1, COEF=None, DY=d, STATS2=None, GAMMA=gam1, DGAMMA=dg1, DBETA=db1, MULBC=mul, ADDBC=add,
             PS=ps, COUNT=B * Ho * Wo, B=B, C=C, HW=Ho * Wo, NREP=1, ACT=D.ACT_SILU, ADDSCALE=1.0 / (Ho * Wo), EVAL=0,
             _flags=D.FLAG_CHAIN if flag else 0)
    prog.add("DWCONV_WGRAD", DY=d, X=x, BNV=bnv2, DW=dw, PRO=D.PRO_SILU, **geo)
    prog.add("DWCONV_DGRAD", DY=d, WT=w, XRAW=x, BNV=bnv2, G=g, STATS2=st2, PRO=D.PRO_SILU, BETA=beta, NREP=nrep, **geo)
    prog.add("BN_BWD_APPLY", GP=g, Y=x, BNV=bnv2, COEF=None, DY=g, STATS2=st2, GAMMA=gam2, DGAMMA=dg2, DBETA=db2, COUNT=B * W * W, B=B, C=C,
             HW=W * W, NREP=nrep, EVAL=0)
    prog.ops = prog.ops[:nrec]
    return c, prog.pack()


def _families(c, packed):
    """kernel family per record (a profiled run on its own copy of the inputs)"""
    from s2lc_amd import _lib

    cpu = torch.zeros(c.arena.top + 256, dtype=torch.uint8)
    for ref, data in c.items.values():
        cpu[ref.off:ref.off + ref.nbytes] = data.contiguous().reshape(-1).view(torch.uint8)
    _, var = _lib.profile_variants(packed, _lib.Bases().set("WS", cpu.cuda()), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [int(v) for v in var]


def _compare(c, got, cpu, wide, outputs, sum0=()):
    for name in outputs:
        ref, _ = c.items[name]
        a = c.read(got, name).double()
        for image, is_wide, label in ((cpu, False, "f32"), (wide, True, "f64")):
            b = c.read(image, name, wide=is_wide).double()
            aa = a
            if name in sum0:
                aa, b = a.sum(0), b.sum(0)
            assert torch.isfinite(b).all(), f"{name}: the {label} emulator produced non-finite values"
            assert torch.isfinite(aa).all(), f"{name}: the GPU produced non-finite values"
            denom = max(b.abs().max().item(), 1e-20)
            err = (aa - b).abs().max().item() / denom
            print(f"{name}: rel err {err:.3e} against the {label} emulator (max |ref| {denom:.3e})")
            assert err < BARS[name], f"{name}: rel err {err:.3e} against the {label} emulator (max |ref| {denom:.3e})"


OUTS = ["g", "d", "dw", "dgamma1", "dbeta1", "dgamma2", "dbeta2"]

# (9, 6, 8, 3): C % 4 != 0 and a partial last pass; (33, 5, ...): more images than one round of the workgroup; (1, 4, 8, 3): B = 1
SHAPES = [(9, 6, 8, 3), (13, 7, 8, 5), (33, 5, 8, 5), (1, 4, 8, 3), (3, 7, 16, 3), (4, 6, 16, 5), (33, 5, 16, 5)]


@pytest.mark.parametrize("B,C,W,K", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_chain_runs_as_one_kernel(B, C, W, K):
    c, packed = _chain(B, C, W, K)
    got, cpu, wide = c.execute(packed, ref64=True, want_variant=FUSED, kind="dw chain")
    _compare(c, got, cpu, wide, OUTS)


@pytest.mark.parametrize("B,C,W,K", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_flag_off_runs_the_single_stages(B, C, W, K):
    c, packed = _chain(B, C, W, K, flag=False)
    fam = _families(c, packed)
    assert 10 not in fam and fam[1] == 6 and fam[2] == 6, fam           # the plane kernels of the depthwise stages, as before
    got, cpu, wide = c.execute(packed, ref64=True)
    _compare(c, got, cpu, wide, OUTS + ["stats2"], sum0=("stats2",))


@pytest.mark.parametrize("what,args", [("beta", dict(B=5, C=6, W=8, K=3, beta=1)), ("w32", dict(B=3, C=5, W=32, K=3)),
                                       ("stride2", dict(B=5, C=6, W=16, K=5, S=2)), ("three_records", dict(B=5, C=6, W=16, K=3, nrec=3))])
def test_declined_chains_run_unfused(what, args):
    """a flag the executor cannot honour is never an error: BETA = 1, a 32 x 32 plane, stride 2, a program that ends after the third record"""
    c, packed = _chain(**args)
    assert packed[0]["flags"] & D.FLAG_CHAIN
    fam = _families(c, packed)
    assert len(fam) == len(packed) and 10 not in fam, fam
    got, cpu, wide = c.execute(packed, ref64=True)
    outs = ["g", "d", "dw", "dgamma1", "dbeta1", "stats2"] if what == "three_records" else OUTS + ["stats2"]
    _compare(c, got, cpu, wide, outs, sum0=("stats2",))
