"""The f32-SPLIT kernels stage by stage (S2K_FLAG_SPLIT: conv_bf16_kernel / wgrad_bf16_kernel with SPLIT, kernel family 5).  Each
case runs one stage record on identical seeded bytes three ways - split, the exact-f32 kernels (the same record without the flag)
and the float64 emulator (oracle/ops_ref.py, wide) - and checks that
  * family 5 ran (s2k_program_profile_variants);
  * the split result is within the f32 op tests' tolerance of the fp32 oracle (tests/test_ops_gpu.py: 1e-4 of the largest value);
  * its max error against float64 is at most 2x the exact-f32 kernel's on the same inputs, above a floor of 2^-22 of the largest value.
The shape tables mirror the bf16-mixed op tests, without their stored-bf16 forms (every operand stays f32 in this mode)."""
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import ops_ref
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan.program import Arena, Program

pytestmark = pytest.mark.gpu

WS = D.BASE["WS"]
_DT = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32}
FLOOR = 2.0 ** -22


class Case:
    def __init__(self, seed=0):
        self.arena = Arena(WS)
        self.items = {}
        self.gen = torch.Generator().manual_seed(seed)

    def t(self, name, shape, fill="randn", dtype="f32", scale=1.0):
        ref = self.arena.alloc(name, shape, dtype)
        if isinstance(fill, torch.Tensor):
            data = fill.reshape(shape).clone()
        elif fill == "randn":
            data = torch.randn(shape, generator=self.gen) * scale
        elif fill == "rand":
            data = torch.rand(shape, generator=self.gen) * scale
        elif fill == "zeros":
            data = torch.zeros(shape)
        elif fill == "nan":
            data = torch.full(shape, float("nan"))
        else:
            raise ValueError(fill)
        self.items[name] = (ref, data.to(_DT[dtype]))
        return ref

    def bnv(self, name, C):
        scale = torch.rand(C, generator=self.gen) + 0.5
        shift = torch.randn(C, generator=self.gen) * 0.3
        return self.t(name, (4, C), torch.stack([scale, shift, torch.randn(C, generator=self.gen) * 0.3, torch.rand(C, generator=self.gen) + 0.7]))

    def pack(self, wt, M, K, T, s_m, s_k, s_t, src_elem_off=0):
        """WEIGHT_PACK of one weight with its hi / mid / lo planes (SPLIT_BASE: the entry's planes start at DST bytes + SPLIT_BASE +
        6 * dst_off); returns (pre-op, packed ref, MP, split ref)"""
        MP, KP = (M + 127) // 128 * 128, (K + 63) // 64 * 64
        dst = self.t(f"packed{len(self.items)}", (KP * T, MP), "nan")
        row = [wt.off // 4 + src_elem_off, dst.off // 4, M, K, T, s_m, s_k, s_t, 0, MP, KP, 0]
        tab = self.t(f"packtab{len(self.items)}", (1, 12), torch.tensor([row], dtype=torch.int32), "i32")
        self.arena.alloc("gap", (dst.off // 8 + 64,))      # the split region must lie beyond 1.5 x dst.off
        dsts = self.t(f"packeds{len(self.items)}", (3 * KP * T * MP // 2,), "nan")
        zero = self.arena.alloc("zero", (1,))
        fields = dict(TABLE=tab, SRC=zero.at(-(zero.off // 4)), DST=zero.at(-(zero.off // 4)), TOTAL=KP * T * MP, N_ENTRIES=1,
                      SPLIT_BASE=dsts.off - 3 * dst.off // 2)
        assert fields["SPLIT_BASE"] > 0 and fields["SPLIT_BASE"] % 16 == 0
        return ("WEIGHT_PACK", fields), dst, MP, dsts

    def _bytes(self, wide):
        k = 2 if wide else 1
        buf = torch.zeros(k * (self.arena.top + 256), dtype=torch.uint8)
        for ref, data in self.items.values():
            d = data.double() if (wide and data.dtype == torch.float32) else data
            b = d.contiguous().reshape(-1).view(torch.uint8)
            buf[k * ref.off:k * ref.off + b.numel()] = b
        return buf

    def run(self, kind, out, tol=1e-4, pre=(), wtb=None, **fields):
        """out: the output tensor's name.  Returns (split error, f32-kernel error) against float64, relative to max |ref|."""
        from s2lc_amd import _lib

        def program(split):
            prog = Program()
            for k, f in pre:
                prog.add(k, **f)
            extra = dict(_flags=D.FLAG_SPLIT, **({"WTB": wtb} if wtb is not None else {})) if split else {}
            prog.add(kind, **fields, **extra)
            return prog.pack()

        st = torch.cuda.current_stream().cuda_stream
        ps, pf = program(True), program(False)
        cpu = self._bytes(False)
        results = {}
        for name, packed in (("split", ps), ("f32", pf)):
            gpu = cpu.cuda()
            _lib.run(packed, _lib.Bases().set("WS", gpu), st)
            torch.cuda.synchronize()
            results[name] = gpu.cpu()
        _, var = _lib.profile_variants(ps, _lib.Bases().set("WS", cpu.cuda()), st)
        assert int(var[-1]) == 5, f"{kind}: kernel family {int(var[-1])}, expected 5 (f32-split)"
        ref32 = cpu.clone()
        ops_ref.run_program(ps, {WS: ref32}, D)                    # the flag is exact f32 to the emulator
        wide = self._bytes(True)
        ops_ref.run_program(ps, {WS: wide}, D, wide=True)
        ref, _ = self.items[out]
        n = ref.nbytes // 4
        view = lambda buf: buf[ref.off:ref.off + ref.nbytes].view(torch.float32).double()    # noqa: E731
        r64 = wide[2 * ref.off:2 * ref.off + 2 * ref.nbytes].view(torch.float64)[:n]
        s, f, r32 = view(results["split"]), view(results["f32"]), view(ref32)
        assert torch.isfinite(s).all() and torch.isfinite(f).all() and torch.isfinite(r64).all(), f"{kind}: non-finite output"
        scale = max(r64.abs().max().item(), 1e-30)
        e32 = (s - r32).abs().max().item() / max(r32.abs().max().item(), 1e-30)
        assert e32 < tol, f"{kind}: split vs fp32 oracle rel err {e32:.3e}"
        es = (s - r64).abs().max().item() / scale
        ef = (f - r64).abs().max().item() / scale
        print(f"{kind} {out}: max error vs float64 / max|ref|: split {es:.3e}, f32 kernel {ef:.3e}")
        assert es <= 2 * ef + FLOOR, f"{kind}: split error {es:.3e} > 2 x the f32 kernel's {ef:.3e} (+ {FLOOR:.1e})"
        return es, ef


def _conv(B, C1, C2, H, W, M, k, pro1, pro2=0, gate=False, bias=True, stats=True, beta=0, mode=0, strides=None, seed=0, x_fill=None,
          w_fill=None):
    c = Case(seed)
    T = k * k
    Ct = C1 + C2
    x1 = c.t("x1", (B, C1, H, W), x_fill if x_fill is not None else "randn")
    x2 = c.t("x2", (B, C2, H, W)) if C2 else None
    bnv1 = c.bnv("bnv1", C1) if pro1 else None
    bnv2 = c.bnv("bnv2", C2) if (C2 and pro2) else None
    g1 = c.t("gate1", (B, C1), "rand") if gate else None
    if strides is None:
        wt = c.t("wt", (M, Ct, T), w_fill if w_fill is not None else "randn", scale=(1.0 / (Ct * T)) ** 0.5)
        sm, sk, st = Ct * T, T, 1
    else:
        wshape, (sm, sk, st) = strides
        wt = c.t("wt", wshape, scale=(1.0 / (Ct * T)) ** 0.5)
    scatter = mode == D.MODE_CONVT_SCATTER
    bs = c.t("bias", (M // 4 if scatter else M,)) if bias else None
    YC = M // 4 if scatter else M
    y = c.t("y", (B, YC, 2 * H, 2 * W) if scatter else (B, YC, H, W), "randn" if beta else "nan")
    nrep = D.stats_replicas(M)
    st_ref = c.t("stats", (nrep, 2, M), "zeros", "f64") if stats else None
    pre, wp, MP, wps = c.pack(wt, M, Ct, T, sm, sk, st)
    pad = 1 if k == 3 else 0
    return c.run("CONV", "y", pre=[pre], wtb=wps, NREP=nrep, X1=x1, BNV1=bnv1, GATE1=g1, X2=x2, BNV2=bnv2, WT=wp, BIAS=bs, Y=y,
                 STATS=st_ref, B=B, C1=C1, C2=C2, H=H, W=W, M=M, KH=k, KW=k, STRIDE=1, PAD_T=pad, PAD_L=pad, HO=H, WO=W, PRO1=pro1,
                 PRO2=pro2, MODE=mode, W_SM=1, W_SK=T * MP, W_ST=MP, FLIP=0, BETA=beta, YC=YC)


def _wgrad(B, M, C, CT, c_off, H, W, k, prop, proq, gateq, seed=0):
    c = Case(seed)
    T = k * k
    P = c.t("p", (B, M, H, W))
    Q = c.t("q", (B, C, H, W))
    bp = c.bnv("bnvp", M) if prop else None
    bq = c.bnv("bnvq", C) if proq else None
    gq = c.t("gateq", (B, C), "rand") if gateq else None
    wgs = c.t("wgs", (T, M, CT), "randn")
    pad = 1 if k == 3 else 0
    return c.run("WGRAD", "wgs", 2e-4, P=P, BNVP=bp, GATEP=None, Q=Q, BNVQ=bq, GATEQ=gq, WGS=wgs.at(c_off), B=B, M=M, C=C, CTOT=CT,
                 H=H, W=W, KH=k, KW=k, STRIDE=1, PAD_T=pad, PAD_L=pad, HO=H, WO=W, PROP=prop, PROQ=proq, MODE=D.MODE_CONV)


@pytest.mark.parametrize("B,C1,H,W,M,pro,gate,bias,stats,beta", [
    (3, 24, 16, 16, 144, 0, False, False, True, 0),     # short K (24 of a 32-channel chunk); 64 x 64 tiles (fewer than 200 tiles of 128 x 128)
    (2, 144, 16, 16, 40, 2, True, False, True, 0),      # project conv: BatchNorm + SiLU + SE gate prologue, 64-row tiles
    (2, 40, 12, 20, 240, 0, False, False, True, 0),
    (2, 1824, 8, 8, 304, 2, True, False, True, 0),      # deep project conv: 64-channel chunks, few pixels
    (2, 32, 24, 24, 24, 3, False, True, False, 0),      # thin (M <= 32), ReLU prologue, bias
    (1, 13, 8, 8, 48, 0, False, False, True, 0),        # K tail (13 channels)
    (4, 264, 64, 64, 200, 3, False, True, True, 0),     # K tail, ReLU prologue, bias
    (6, 288, 1, 200, 320, 0, False, True, False, 1),    # a Linear over feature-major tokens (H = 1), accumulate into Y
    (3, 256, 100, 100, 176, 1, False, False, True, 0),  # AFFINE prologue; tiles straddle images, ragged last tile
    (2, 576, 16, 16, 200, 0, False, True, True, 0),     # deep reduction, no prologue: packed K = 9 x 64
    (2, 1056, 16, 16, 176, 2, True, False, False, 1),   # deep project conv, ragged K, accumulate
])
def test_conv1x1_split(B, C1, H, W, M, pro, gate, bias, stats, beta):
    _conv(B, C1, 0, H, W, M, 1, pro, gate=gate, bias=bias, stats=stats, beta=beta, seed=C1 + M)


@pytest.mark.parametrize("B,C1,C2,H,W,M,pro,beta", [
    (4, 32, 24, 64, 128, 64, 0, 0),      # (R, XW) = (2, 64): decoder concat conv, two x tiles per row
    (8, 64, 0, 32, 32, 128, 3, 0),       # (4, 32): BatchNorm + ReLU prologue, zero padding after the activation
    (20, 72, 0, 16, 16, 192, 3, 1),      # (8, 16): K tail, accumulate
    (4, 24, 0, 30, 56, 72, 0, 0),        # (2, 56): 15 whole tile rows, K tail
    (12, 32, 0, 28, 28, 64, 3, 0),       # (4, 28)
    (40, 64, 0, 14, 14, 128, 0, 0),      # (8, 14)
    (8, 32, 13, 64, 64, 32, 0, 0),       # thin (M <= 32): concat with the raw 13-band input
    (8, 32, 0, 64, 64, 32, 3, 0),        # thin, BatchNorm + ReLU prologue
    (6, 64, 0, 62, 128, 24, 0, 1),       # thin, M = 24, ragged last tile row, accumulate
])
def test_conv3x3_split(B, C1, C2, H, W, M, pro, beta):
    _conv(B, C1, C2, H, W, M, 3, pro, pro if C2 else 0, bias=True, stats=(beta == 0), beta=beta, seed=B + M)


@pytest.mark.parametrize("B,Cin,Cout,H,W,pro", [(2, 24, 16, 8, 8, 3), (2, 2048, 512, 4, 4, 2), (2, 64, 32, 16, 24, 3)])
def test_conv_transpose_scatter_split(B, Cin, Cout, H, W, pro):
    _conv(B, Cin, 0, H, W, 4 * Cout, 1, pro, bias=True, stats=False, mode=D.MODE_CONVT_SCATTER,
          strides=((Cin, Cout, 4), (1, 4 * Cout, 1)), seed=Cin)


@pytest.mark.parametrize("beta", [0, 1])
def test_conv_dgrad_3x3_flip_split(beta):
    """the data gradient of a 3x3 conv: A = the flipped, transposed weight slice of a concat conv (WEIGHT_PACK flip)"""
    B, Mout, Ctot, c_off, Cs, H, W = 2, 64, 40, 16, 24, 12, 64
    c = Case(3)
    dy = c.t("x1", (B, Mout, H, W))
    wfull = c.t("wt_full", (Mout, Ctot, 9), scale=0.1)
    y = c.t("y", (B, Cs, H, W), "randn" if beta else "nan")
    MP, KP = 128, 64
    dst = c.t("packed", (KP * 9, MP), "nan")
    row = [wfull.off // 4 + c_off * 9, dst.off // 4, Cs, Mout, 9, 9, Ctot * 9, 1, 1, MP, KP, 0]
    tab = c.t("packtab", (1, 12), torch.tensor([row], dtype=torch.int32), "i32")
    c.arena.alloc("gap", (dst.off // 8 + 64,))
    dsts = c.t("packeds", (3 * KP * 9 * MP // 2,), "nan")
    zero = c.arena.alloc("zero", (1,))
    pre = ("WEIGHT_PACK", dict(TABLE=tab, SRC=zero.at(-(zero.off // 4)), DST=zero.at(-(zero.off // 4)), TOTAL=KP * 9 * MP, N_ENTRIES=1,
                               SPLIT_BASE=dsts.off - 3 * dst.off // 2))
    c.run("CONV", "y", pre=[pre], wtb=dsts, X1=dy, BNV1=None, GATE1=None, X2=None, BNV2=None, WT=dst, BIAS=None, Y=y, STATS=None, B=B,
          C1=Mout, C2=0, H=H, W=W, M=Cs, KH=3, KW=3, STRIDE=1, PAD_T=1, PAD_L=1, HO=H, WO=W, PRO1=0, PRO2=0, MODE=0, W_SM=1,
          W_SK=9 * MP, W_ST=MP, FLIP=0, BETA=beta, YC=Cs, NREP=1)


@pytest.mark.parametrize("B,M,C,H,W,prop,proq,gate", [
    (5, 240, 250, 16, 16, 0, 0, False),      # 128 x 128 tiles, ragged on both sides
    (8, 240, 72, 8, 8, 0, 2, True),          # 128 x 64, SiLU + SE gate on Q
    (4, 40, 144, 16, 20, 0, 3, False),       # 64 x 64 (three c tiles), ReLU on Q
    (3, 64, 64, 20, 20, 2, 0, False),        # SiLU prologue on P
    (2, 768, 384, 1, 520, 0, 0, False),      # a Linear over feature-major tokens; tiles straddle images
    (4, 130, 130, 16, 16, 3, 0, False),      # ReLU on P
    (2, 24, 4, 64, 64, 0, 3, False),         # thin on both sides
    (2, 24, 144, 32, 32, 0, 2, True),        # thin M, SiLU + gate on Q
    (3, 144, 24, 20, 20, 0, 0, False),       # thin C; tiles straddle images
])
def test_wgrad_1x1_split(B, M, C, H, W, prop, proq, gate):
    _wgrad(B, M, C, C, 0, H, W, 1, prop, proq, gate, seed=M + C)


@pytest.mark.parametrize("B,M,C,CT,c_off,H,W,proq", [
    (2, 64, 64, 64, 0, 6, 64, 3),        # BatchNorm + ReLU on Q: zero padding after the activation
    (1, 128, 88, 88, 0, 10, 128, 0),     # four x tiles per row (2 x 32 pixel tiles), ragged c tile
    (2, 72, 40, 104, 64, 12, 32, 3),     # channel slice of a concat conv (CTOT > C), ragged m / c tiles
    (2, 256, 64, 64, 0, 16, 16, 0),      # 16-wide maps: 4 m-tiles
    (3, 64, 128, 128, 0, 10, 16, 3),     # H not a multiple of the tile height
    (1, 32, 13, 45, 32, 10, 128, 0),     # 32 x 32 tile: 13 of 32 columns used
    (2, 24, 32, 32, 0, 5, 64, 3),        # 32 x 32 tile, odd height
    (2, 64, 24, 24, 0, 9, 128, 0),       # 64 x 32 tiles
    (2, 32, 64, 64, 0, 8, 64, 3),        # 32 x 64 tiles
])
def test_wgrad_3x3_split(B, M, C, CT, c_off, H, W, proq):
    _wgrad(B, M, C, CT, c_off, H, W, 3, 0, proq, False, seed=M + C + H)


def _spread(shape, seed):
    """values over 2^-20 .. 2^20 with random signs and all 23 stored significand bits random: bf16 keeps 8 of them"""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-20, 21, shape, generator=g).double()
    mant = 1.0 + torch.rand(shape, generator=g, dtype=torch.float64)
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return (sign * mant * torch.pow(2.0, e)).float()


def test_adversarial_operands_stay_f32_accurate():
    """operands spread over 2^-20 .. 2^20 with their low significand bits set: one bf16 term would lose 2^-9 of each, the split keeps
    the f32 kernel's accuracy (the f64 comparison of Case.run: within 2x)"""
    B, C, H, W, M = 2, 96, 16, 16, 128
    es, ef = _conv(B, C, 0, H, W, M, 1, 0, bias=False, stats=False, seed=5, x_fill=_spread((B, C, H, W), 1),
                   w_fill=_spread((M, C, 1), 2))
    assert es < 1e-5, es
    es3, _ = _conv(B, C, 0, H, 64, M, 3, 0, bias=False, stats=False, seed=6, x_fill=_spread((B, C, H, 64), 3),
                   w_fill=_spread((M, C, 9), 4))
    assert es3 < 1e-5, es3

