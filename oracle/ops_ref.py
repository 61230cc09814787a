"""TEST INFRASTRUCTURE ONLY — CPU semantics of every s2k stage, and a program emulator.

Each function below states, with plain torch CPU ops, what one stage record
(`sentinel2-landcover-classification_amd/plan/opdefs.py`) must compute.  Two uses:
  * tests/test_plan_cpu.py runs whole planned programs through `run_program` and compares with
    oracle autograd — this validates the planner (the hand-derived backward) without a GPU;
  * tests/test_ops_gpu.py runs single-stage programs through the HIP C-ABI and compares with
    the same functions.
The arithmetic mirrors the reference's torch calls (F.conv2d / F.batch_norm / ... as used in
/root/reference/src/modules/efficientnet_unet.py and losses.py); nothing here is product code.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

_DT = {"f32": torch.float32, "f64": torch.float64, "i64": torch.int64, "i32": torch.int32, "i16": torch.int16, "u8": torch.uint8,
       "bf16": torch.bfloat16}


class Mem:
    """Byte-addressed bases (one flat uint8 CPU tensor each).

    wide=True: every f32 tensor is held as float64 at twice its byte offset (the bases must be
    allocated twice as large).  Running a planned program this way against a float64 oracle
    checks the planner's algebra to ~1e-12, free of the fp32 noise that small-batch BatchNorm
    and ReLU masks amplify to ~1e-2 in the gradients."""

    def __init__(self, bases: dict[int, torch.Tensor], wide: bool = False, narrow_bases=(), b16_operands: bool = False):
        self.bases = bases
        self.wide = wide
        self.b16 = bool(b16_operands)     # wide only: FLAG_BF16 stages round their operands as the kernels do (see _bf16_operands)
        self.narrow = set(narrow_bases)
        self.fdtype = torch.float64 if wide else torch.float32

    def addr(self, ref: int, elem_off: int = 0) -> int:
        """ref advanced by elem_off f32 elements."""
        return ref + elem_off * 4

    def view(self, ref: int, shape, dtype="f32", strides=None) -> torch.Tensor | None:
        if ref < 0:
            return None
        base, off = ref >> 56, ref & ((1 << 56) - 1)
        if self.wide and base not in self.narrow:
            off *= 2
            if dtype == "f32":
                dtype = "f64"
            elif dtype == "bf16":      # (a 2-byte slot doubled holds an f32: the float64 emulation does not round operands)
                dtype = "f32"
        dt = _DT[dtype]
        isz = torch.empty((), dtype=dt).element_size()
        buf = self.bases[base]
        assert off % isz == 0
        flat = buf.view(torch.uint8)[off:].view(dt) if off else buf.view(torch.uint8).view(dt)
        n = int(np.prod(shape)) if strides is None else None
        if strides is None:
            return flat[:n].view(*shape)
        return torch.as_strided(flat, tuple(shape), tuple(strides))


def _pro(x, bnv, gate, pro, C):
    """prologue: act(scale*x+shift) * gate[b][c]; bnv rows = scale, shift, mean, invstd."""
    if pro != 0:
        x = x * bnv[0].view(1, C, 1, 1) + bnv[1].view(1, C, 1, 1)
        if pro == 2:
            x = F.silu(x)
        elif pro == 3:
            x = F.relu(x)
        elif pro == 4:
            x = F.gelu(x)
    if gate is not None:
        x = x * gate.view(gate.shape[0], C, 1, 1)
    return x


def _act_grad(u, act):
    if act == 2:
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    if act == 3:
        return (u > 0).to(u.dtype)
    if act == 4:   # d/du [u * Phi(u)] = Phi(u) + u * phi(u)
        return 0.5 * (1 + torch.erf(u * 0.7071067811865476)) + u * torch.exp(-0.5 * u * u) * 0.3989422804014327
    return torch.ones_like(u)


def _unshuffle2(x):  # [B,C,2H,2W] -> [B,C*4,H,W] with k = (c,dy,dx)
    B, C, H2, W2 = x.shape
    return x.view(B, C, H2 // 2, 2, W2 // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, C * 4, H2 // 2, W2 // 2)


def _shuffle2(z, Cout):  # [B,4*Cout,H,W] rows (co,dy,dx) -> [B,Cout,2H,2W]
    B, _, H, W = z.shape
    return z.view(B, Cout, 2, 2, H, W).permute(0, 1, 4, 2, 5, 3).reshape(B, Cout, 2 * H, 2 * W)


def _pad_to(x, pt, pl, k_h, k_w, s, Ho, Wo):
    H, W = x.shape[-2:]
    pb = (Ho - 1) * s + k_h - H - pt
    pr = (Wo - 1) * s + k_w - W - pl
    return F.pad(x, [pl, pr, pt, pb])


def op_memset(m: Mem, o):
    base, off = o["DST"] >> 56, o["DST"] & ((1 << 56) - 1)
    k = 2 if (m.wide and base not in m.narrow) else 1
    m.bases[base].view(torch.uint8)[off * k:(off + o["BYTES"]) * k].zero_()


def op_axpy(m: Mem, o):
    m.view(o["Y"], (o["COUNT"],)).add_(m.view(o["X"], (o["COUNT"],)))


def op_weight_pack(m: Mem, o):
    tab = m.view(o["TABLE"], (o["N_ENTRIES"], 12), "i32")
    for src_off, dst_off, M, K, T, s_m, s_k, s_t, flip, MP, KP, _ in tab.tolist():
        src = m.view(m.addr(o["SRC"], src_off), (M, K, T), strides=(s_m, s_k, s_t))
        if flip & 1:        # (bit 1: a quad copy of the entry is wanted - a layout for csrc/conv_q4.hip, no arithmetic: not modelled)
            src = src.flip(2)
        dst = m.view(m.addr(o["DST"], dst_off), (KP, T, MP))
        dst.zero_()
        dst[:K, :, :M] = src.permute(1, 2, 0)


def _bf16_operands(m: Mem, o) -> bool:
    """bf16-MIXED stage (S2kOp.flags & FLAG_BF16): the two MFMA operands - the activated inputs and the weights - are rounded to
    bf16 (round-to-nearest-even), products and sums stay f32.  Not applied in `wide` (float64) emulation: that mode checks the
    planner's algebra, not the arithmetic - unless run_program is given b16_operands=True, the float64 reference OF the bf16
    operation: the prologue is evaluated in f32 as the kernels do (_pro_b16), the activated operand and the weight are rounded to
    bf16, and the products, the sums, the epilogue terms and the statistics are float64."""
    return bool(o.get("_flags", 0) & 4) and (not m.wide or m.b16)


def _pro_b16(m: Mem, o, x, bnv, gate, pro, C):
    """_pro; in the float64 reference of a bf16 stage (wide + b16_operands) evaluated in f32, as the kernels evaluate it"""
    if m.wide and _bf16_operands(m, o):
        f = lambda t: None if t is None else t.float()     # noqa: E731  (the tensors hold f32 values: exact)
        return _pro(f(x), f(bnv), f(gate), pro, C).double()
    return _pro(x, bnv, gate, pro, C)


def _r16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def op_conv(m: Mem, o):
    B, C1, C2, H, W, M = o["B"], o["C1"], o["C2"], o["H"], o["W"], o["M"]
    KH, KW, S, Ho, Wo, mode = o["KH"], o["KW"], o["STRIDE"], o["HO"], o["WO"], o["MODE"]
    T = KH * KW
    Ct = C1 + C2
    if mode == 2:
        co = C1 // 4
        x1 = _unshuffle2(m.view(o["X1"], (B, co, 2 * H, 2 * W)))
    else:
        x1 = m.view(o["X1"], (B, C1, H, W), "bf16" if o.get("X1_BF16", 0) else "f32").to(m.fdtype)
    x = _pro_b16(m, o, x1, m.view(o["BNV1"], (4, C1)), m.view(o["GATE1"], (B, C1)), o["PRO1"], C1)
    if C2:
        x2 = _pro_b16(m, o, m.view(o["X2"], (B, C2, H, W)), m.view(o["BNV2"], (4, C2)), None, o["PRO2"], C2)
        x = torch.cat([x, x2], 1)
    wv = m.view(o["WT"], (M, Ct, T), strides=(o["W_SM"], o["W_SK"], o["W_ST"]))
    if o["FLIP"]:
        wv = wv.flip(2)
    wv = wv.reshape(M, Ct, KH, KW)
    if _bf16_operands(m, o):
        x, wv = _r16(x), _r16(wv)
    y = F.conv2d(_pad_to(x, o["PAD_T"], o["PAD_L"], KH, KW, S, Ho, Wo), wv, None, S)
    bias = m.view(o["BIAS"], (M // 4 if mode == 1 else M,))
    YC = o["YC"]
    if mode == 1:
        y = _shuffle2(y, M // 4)
        if bias is not None:
            y = y + bias.view(1, -1, 1, 1)
        dst = m.view(o["Y"], (B, M // 4, 2 * Ho, 2 * Wo), strides=(YC * 4 * Ho * Wo, 4 * Ho * Wo, 2 * Wo, 1))
    else:
        if bias is not None:
            y = y + bias.view(1, -1, 1, 1)
        dst = m.view(o["Y"], (B, M, Ho, Wo), strides=(YC * Ho * Wo, Ho * Wo, Wo, 1))
    if o.get("RES", -1) >= 0:
        res = m.view(o["RES"], tuple(dst.shape), strides=tuple(dst.stride()))
        # FLAG_RES_GELU_GRAD: the backward of "GELU, then this Linear's transpose" in one stage - times gelu'(RES) instead of + RES
        y = y * _act_grad(res, 4) if (o.get("_flags", 0) & 32) else y + res       # 32 = opdefs.FLAG_RES_GELU_GRAD
    if o["BETA"]:
        dst.add_(y)
    else:
        dst.copy_(y)
    if o["STATS"] >= 0:
        # the statistics of the FINISHED rows - what Y holds now, residual and accumulate included - as every CONV kernel and the
        # split-K tail take them (csrc/igemm.hip: "BatchNorm statistics of the finished rows"); no planned stage has STATS with
        # RES or BETA, so only stage-level tests see the order
        fin = dst.double()
        st = m.view(o["STATS"], (max(o["NREP"], 1), 2, M), "f64")[0]   # any replica: finalize sums them all
        st[0] += fin.sum((0, 2, 3))
        st[1] += (fin ** 2).sum((0, 2, 3))


def op_wgrad(m: Mem, o):
    B, M, C, CT, H, W = o["B"], o["M"], o["C"], o["CTOT"], o["H"], o["W"]
    KH, KW, S, Ho, Wo, mode = o["KH"], o["KW"], o["STRIDE"], o["HO"], o["WO"], o["MODE"]
    T = KH * KW
    P = _pro_b16(m, o, m.view(o["P"], (B, M, Ho, Wo), "bf16" if o.get("P_BF16", 0) else "f32").to(m.fdtype), m.view(o["BNVP"], (4, M)), m.view(o["GATEP"], (B, M)), o["PROP"], M)
    Q = _pro_b16(m, o, m.view(o["Q"], (B, C, H, W)), m.view(o["BNVQ"], (4, C)), m.view(o["GATEQ"], (B, C)), o["PROQ"], C)
    if _bf16_operands(m, o):
        P, Q = _r16(P), _r16(Q)
    if mode == 2:
        Qg = _unshuffle2(Q).view(B, C, 4, Ho * Wo)
        dW = torch.einsum("bmp,bctp->tmc", P.reshape(B, M, Ho * Wo).double(), Qg.double())
    else:
        Qp = _pad_to(Q, o["PAD_T"], o["PAD_L"], KH, KW, S, Ho, Wo)
        cols = F.unfold(Qp, (KH, KW), stride=S).view(B, C, T, Ho * Wo)
        dW = torch.einsum("bmp,bctp->tmc", P.reshape(B, M, Ho * Wo).double(), cols.double())
    m.view(o["WGS"], (T, M, C), strides=(M * CT, CT, 1)).add_(dW.to(m.fdtype))


def op_wgrad_finalize(m: Mem, o):
    tab = m.view(o["TABLE"], (o["N_ENTRIES"], 5), "i32")
    for off, M, C, T, _ in tab.tolist():
        src = m.view(m.addr(o["WGS"], off), (T, M, C))
        dst = m.view(m.addr(o["GRADS"], off), (M, C, T))
        dst.add_(src.permute(1, 2, 0))


def _dw_geo(o):
    return (o["B"], o["C"], o["H"], o["W"], o["K"], o["STRIDE"], o["PAD_T"], o["PAD_L"], o["HO"], o["WO"])


def op_dwconv_fwd(m: Mem, o):
    _fold(m, o)
    B, C, H, W, K, S, pt, pl, Ho, Wo = _dw_geo(o)
    x = _pro(m.view(o["X"], (B, C, H, W)), m.view(o["BNV"], (4, C)), None, o["PRO"], C)
    w = m.view(o["WT"], (C, 1, K, K))
    y = F.conv2d(_pad_to(x, pt, pl, K, K, S, Ho, Wo), w, None, S, 0, 1, C)
    m.view(o["Y"], (B, C, Ho, Wo)).copy_(y)
    if o["STATS"] >= 0:
        st = m.view(o["STATS"], (max(o["NREP"], 1), 2, C), "f64")[-1]
        st[0] += y.double().sum((0, 2, 3))
        st[1] += (y.double() ** 2).sum((0, 2, 3))


def op_dwconv_dgrad(m: Mem, o):
    B, C, H, W, K, S, pt, pl, Ho, Wo = _dw_geo(o)
    dy = m.view(o["DY"], (B, C, Ho, Wo))
    w = m.view(o["WT"], (C, 1, K, K))
    xd = torch.zeros(B, C, H, W, requires_grad=True, dtype=dy.dtype)
    y = F.conv2d(_pad_to(xd, pt, pl, K, K, S, Ho, Wo), w, None, S, 0, 1, C)
    (gx,) = torch.autograd.grad(y, xd, dy)
    if o["PRO"] != 0:
        bnv = m.view(o["BNV"], (4, C))
        xr = m.view(o["XRAW"], (B, C, H, W))
        u = xr * bnv[0].view(1, C, 1, 1) + bnv[1].view(1, C, 1, 1)
        gx = gx * _act_grad(u, o["PRO"])
        if o["STATS2"] >= 0:
            xhat = (xr - bnv[2].view(1, C, 1, 1)) * bnv[3].view(1, C, 1, 1)
            st = m.view(o["STATS2"], (max(o["NREP"], 1), 2, C), "f64")[0]
            st[0] += gx.double().sum((0, 2, 3))
            st[1] += (gx.double() * xhat.double()).sum((0, 2, 3))
    g = m.view(o["G"], (B, C, H, W))
    if o["BETA"]:
        g.add_(gx)
    else:
        g.copy_(gx)


def op_dwconv_wgrad(m: Mem, o):
    B, C, H, W, K, S, pt, pl, Ho, Wo = _dw_geo(o)
    dy = m.view(o["DY"], (B, C, Ho, Wo))
    x = _pro(m.view(o["X"], (B, C, H, W)), m.view(o["BNV"], (4, C)), None, o["PRO"], C)
    wd = torch.zeros(C, 1, K, K, requires_grad=True, dtype=dy.dtype)
    y = F.conv2d(_pad_to(x, pt, pl, K, K, S, Ho, Wo), wd, None, S, 0, 1, C)
    (gw,) = torch.autograd.grad(y, wd, dy)
    m.view(o["DW"], (C, 1, K, K)).add_(gw)


def op_bn_finalize(m: Mem, o):
    C = o["C"]
    gamma, beta = m.view(o["GAMMA"], (C,)), m.view(o["BETA"], (C,))
    rm, rv = m.view(o["RM"], (C,)), m.view(o["RV"], (C,))
    bnv = m.view(o["BNV"], (4, C))
    if o["TRAIN"]:
        n = float(o["COUNT"])
        st = m.view(o["STATS"], (max(o["NREP"], 1), 2, C), "f64").sum(0)
        mean = st[0] / n
        var = (st[1] / n - mean * mean).clamp_min(0.0)
        invstd = 1.0 / torch.sqrt(var + float(np.float32(o["EPS"])))
        mom = float(np.float32(o["MOM"]))
        rm.mul_(1 - mom).add_((mom * mean).to(m.fdtype))
        rv.mul_(1 - mom).add_((mom * var * (n / max(n - 1.0, 1.0))).to(m.fdtype))
        mean, invstd = mean.to(m.fdtype), invstd.to(m.fdtype)
    else:
        mean = rm.clone()
        invstd = 1.0 / torch.sqrt(rv + o["EPS"])
    scale = gamma * invstd
    bnv[0] = scale
    bnv[1] = beta - mean * scale
    bnv[2] = mean
    bnv[3] = invstd


def _fold(m: Mem, o):
    """BN_FINALIZE folded into the first consumer of its {scale, shift} (plan/opdefs.py FOLD_*): run it first."""
    if o.get("FSTATS", -1) >= 0:
        op_bn_finalize(m, {"STATS": o["FSTATS"], "GAMMA": o["FGAMMA"], "BETA": o["FBETA"], "RM": o["FRM"], "RV": o["FRV"], "BNV": o["BNV"],
                           "COUNT": o["FCOUNT"], "C": o["C"], "TRAIN": 1, "NREP": o["FNREP"], "EPS": o["FEPS"], "MOM": o["FMOM"]})


def op_se_pool(m: Mem, o):
    _fold(m, o)
    B, C, HW = o["B"], o["C"], o["HW"]
    a = _pro(m.view(o["Y"], (B, C, HW, 1)), m.view(o["BNV"], (4, C)), None, o["PRO"], C)
    m.view(o["POOL"], (B, C)).copy_(a.view(B, C, HW).mean(2))


def op_se_fc(m: Mem, o):
    B, C, Q = o["B"], o["C"], o["CSQ"]
    pool = m.view(o["POOL"], (B, C))
    hpre = pool @ m.view(o["W1"], (Q, C)).t() + m.view(o["B1"], (Q,))
    g = F.silu(hpre) @ m.view(o["W2"], (C, Q)).t() + m.view(o["B2"], (C,))
    m.view(o["HPRE"], (B, Q)).copy_(hpre)
    m.view(o["GATE"], (B, C)).copy_(torch.sigmoid(g))


def op_se_fc_bwd(m: Mem, o):
    B, C, Q = o["B"], o["C"], o["CSQ"]
    dgate, gate = m.view(o["DGATE"], (B, C)), m.view(o["GATE"], (B, C))
    hpre, pool = m.view(o["HPRE"], (B, Q)), m.view(o["POOL"], (B, C))
    W1, W2 = m.view(o["W1"], (Q, C)), m.view(o["W2"], (C, Q))
    dgp = dgate * gate * (1 - gate)
    h = F.silu(hpre)
    dhp = (dgp @ W2) * _act_grad(hpre, 2)
    if o["DW1"] >= 0:
        m.view(o["DW2"], (C, Q)).add_(dgp.t() @ h)
        m.view(o["DB2"], (C,)).add_(dgp.sum(0))
        m.view(o["DW1"], (Q, C)).add_(dhp.t() @ pool)
        m.view(o["DB1"], (Q,)).add_(dhp.sum(0))
    m.view(o["DPOOL"], (B, C)).copy_(dhp @ W1)
    # what the kernels leave behind for SE_FC_WGRAD
    m.view(o["HS"], (B, Q)).copy_(h)
    dgate.copy_(dgp)
    hpre.copy_(dhp)


def op_se_fc_wgrad(m: Mem, o):
    B, C, Q = o["B"], o["C"], o["CSQ"]
    dgp, hs = m.view(o["DGP"], (B, C)), m.view(o["HS"], (B, Q))
    dhp, pool = m.view(o["DHP"], (B, Q)), m.view(o["POOL"], (B, C))
    m.view(o["DW2"], (C, Q)).add_(dgp.t() @ hs)
    m.view(o["DB2"], (C,)).add_(dgp.sum(0))
    m.view(o["DW1"], (Q, C)).add_(dhp.t() @ pool)
    m.view(o["DB1"], (Q,)).add_(dhp.sum(0))


def op_se_bwd_reduce(m: Mem, o):
    B, C, HW = o["B"], o["C"], o["HW"]
    a = _pro(m.view(o["Y"], (B, C, HW, 1)), m.view(o["BNV"], (4, C)), None, o["PRO"], C).view(B, C, HW)
    m.view(o["DGATE"], (B, C)).copy_((m.view(o["G"], (B, C, HW)) * a).sum(2))


def _dcs(m, o, B):
    noise = m.view(o["NOISE"], (B,))
    if noise is None:
        return None
    keep = np.float32(o["KEEP"])
    return torch.floor(float(keep) + noise) / float(keep)


def op_bn_bwd_reduce(m: Mem, o):
    B, C, HW, act = o["B"], o["C"], o["HW"], o["ACT"]
    g = m.view(o["G"], (B, C, HW)).clone()
    y = m.view(o["Y"], (B, C, HW))
    bnv = m.view(o["BNV"], (4, C))
    mul, add = m.view(o["MULBC"], (B, C)), m.view(o["ADDBC"], (B, C))
    if mul is not None:
        g = g * mul.view(B, C, 1)
    dcs = _dcs(m, o, B)
    if dcs is not None:
        g = g * dcs.view(B, 1, 1)
    if add is not None:
        g = g + add.view(B, C, 1) * float(np.float32(o["ADDSCALE"]))
    u = y * bnv[0].view(1, C, 1) + bnv[1].view(1, C, 1)
    g = g * _act_grad(u, act)
    xhat = (y - bnv[2].view(1, C, 1)) * bnv[3].view(1, C, 1)
    st = m.view(o["STATS2"], (max(o["NREP"], 1), 2, C), "f64")[0]
    st[0] += g.double().sum((0, 2))
    st[1] += (g.double() * xhat.double()).sum((0, 2))
    m.view(o["GOUT"], (B, C, HW)).copy_(g)


def op_bn_bwd_finalize(m: Mem, o):
    C, n = o["C"], float(o["COUNT"])
    st = m.view(o["STATS2"], (max(o["NREP"], 1), 2, C), "f64").sum(0)
    gamma, bnv = m.view(o["GAMMA"], (C,)), m.view(o["BNV"], (4, C))
    m.view(o["DGAMMA"], (C,)).add_(st[1].to(m.fdtype))
    m.view(o["DBETA"], (C,)).add_(st[0].to(m.fdtype))
    coef = m.view(o["COEF"], (3, C))
    a = (gamma * bnv[3]).double()
    coef[0] = a.to(m.fdtype)
    coef[1] = (-a * st[1] / n).to(m.fdtype)
    coef[2] = (-a * st[0] / n).to(m.fdtype)


def op_bn_bwd_apply(m: Mem, o):
    B, C, HW = o["B"], o["C"], o["HW"]
    gp, y = m.view(o["GP"], (B, C, HW)), m.view(o["Y"], (B, C, HW))
    bnv = m.view(o["BNV"], (4, C))
    if o["COEF"] >= 0:
        coef = m.view(o["COEF"], (3, C))
    else:   # fused form: BN_BWD_FINALIZE's arithmetic
        n = float("inf") if o.get("EVAL", 0) else float(o["COUNT"])   # eval-mode BatchNorm: statistics are constants
        if o.get("PS", -1) >= 0:   # SE_BN_COMBINE folded in
            ps = m.view(o["PS"], (4, B, C)).double()
            mul, add = m.view(o["MULBC"], (B, C)), m.view(o["ADDBC"], (B, C))
            mul = mul.double() if mul is not None else torch.ones(B, C, dtype=torch.float64)
            add = add.double() * o["ADDSCALE"] if add is not None else torch.zeros(B, C, dtype=torch.float64)
            st = torch.stack([(mul * ps[0] + add * ps[1]).sum(0), (mul * ps[2] + add * ps[3]).sum(0)])
        else:
            st = m.view(o["STATS2"], (max(o["NREP"], 1), 2, C), "f64").sum(0)
        m.view(o["DGAMMA"], (C,)).add_(st[1].to(m.fdtype))
        m.view(o["DBETA"], (C,)).add_(st[0].to(m.fdtype))
        a = (m.view(o["GAMMA"], (C,)) * bnv[3]).double()
        coef = torch.stack([a, -a * st[1] / n, -a * st[0] / n]).to(m.fdtype)
    xhat = (y - bnv[2].view(1, C, 1)) * bnv[3].view(1, C, 1)
    if o["COEF"] < 0 and (o.get("ACT", 0) or o.get("MULBC", -1) >= 0 or o.get("ADDBC", -1) >= 0):   # recompute g' from the raw gradient
        mul, add = m.view(o["MULBC"], (B, C)), m.view(o["ADDBC"], (B, C))
        g = gp * (mul.view(B, C, 1) if mul is not None else 1.0)
        if add is not None:
            g = g + add.view(B, C, 1) * o["ADDSCALE"]
        gp = g * _act_grad(y * bnv[0].view(1, C, 1) + bnv[1].view(1, C, 1), o["ACT"])
    dy = coef[0].view(1, C, 1) * gp + coef[1].view(1, C, 1) * xhat + coef[2].view(1, C, 1)
    m.view(o["DY"], (B, C, HW), "bf16" if o.get("OUT_BF16", 0) else "f32").copy_(dy)       # (copy_ rounds to nearest even)


def op_bn_residual(m: Mem, o):
    _fold(m, o)
    B, C, HW = o["B"], o["C"], o["HW"]
    bnv = m.view(o["BNV"], (4, C))
    v = m.view(o["Y"], (B, C, HW)) * bnv[0].view(1, C, 1) + bnv[1].view(1, C, 1)
    dcs = _dcs(m, o, B)
    if dcs is not None:
        v = v * dcs.view(B, 1, 1)
    ident = m.view(o["IDENT"], (B, C, HW))
    if ident is not None:
        v = v + ident
    m.view(o["XOUT"], (B, C, HW)).copy_(v)


def op_channel_sum(m: Mem, o):
    B, C, HW = o["B"], o["C"], o["HW"]
    m.view(o["OUT"], (C,)).add_(m.view(o["G"], (B, C, HW)).double().sum((0, 2)).to(m.fdtype))


def _loss_value(lg, y, alpha, o):
    from . import losses_ref

    ign = o["IGNORE"]
    if alpha is None and o["MODE"] != 0:
        alpha = torch.ones(lg.shape[1], dtype=lg.dtype)
    if o["MODE"] == 0:
        return losses_ref.cross_entropy(lg, y, alpha, float(np.float32(o["SMOOTH"])), ign)
    return losses_ref.focal(lg, y, alpha, float(np.float32(o["GAMMA"])), float(np.float32(o["SMOOTH"])), ign,
                            "sum" if o["REDUCE_SUM"] else "mean")


def op_loss_fwd(m: Mem, o):
    B, C, HW = o["B"], o["C"], o["HW"]
    lg = m.view(o["LOGITS"], (B, C, HW, 1))
    y = m.view(o["LABELS"], (B, HW, 1), "i64")
    alpha = m.view(o["ALPHA"], (C,))
    m.view(o["LOSS"], (1,)).copy_(_loss_value(lg, y, alpha, o).reshape(1))
    acc = m.view(o["ACC"], (2,), "f64")
    if acc is not None:     # [numerator, denominator] as LOSS_BWD reads them: per-pixel terms in the working precision, summed in f64
        from . import losses_ref

        smooth = float(np.float32(o["SMOOTH"]))
        if o["MODE"] == 0:
            ce, w_y, _ = losses_ref._per_pixel_ce(lg, y, alpha, smooth, o["IGNORE"])
            acc[0], acc[1] = ce.double().sum(), w_y.double().sum()
        else:
            a = torch.ones(C, dtype=lg.dtype) if alpha is None else alpha
            acc[0] = losses_ref.focal(lg, y, a, float(np.float32(o["GAMMA"])), smooth, o["IGNORE"], "none").double().sum()
            acc[1] = 0.0


def op_loss_bwd(m: Mem, o):
    B, C, HW = o["B"], o["C"], o["HW"]
    lg = m.view(o["LOGITS"], (B, C, HW, 1)).clone().requires_grad_(True)
    y = m.view(o["LABELS"], (B, HW, 1), "i64")
    alpha = m.view(o["ALPHA"], (C,))
    v = _loss_value(lg, y, alpha, o)
    (g,) = torch.autograd.grad(v, lg)
    m.view(o["DLOGITS"], (B, C, HW, 1)).copy_(g * m.view(o["GOUT"], (1,)))


def op_argmax(m: Mem, o):
    from . import losses_ref

    B, C, HW = o["B"], o["C"], o["HW"]
    m.view(o["MASK"], (B, HW, 1), "i64").copy_(losses_ref.class_mask(m.view(o["LOGITS"], (B, C, HW, 1))))


# ---- Prithvi MAE-ViT / segmentation stages (feature-major [B][C][L] activations) -----------------------
# arithmetic follows the reference's torch calls: nn.LayerNorm (prithvi.py via timm Block, prithvi_segmentation.py:11-20),
# softmax attention (timm Attention, parity unpinned), random_masking (prithvi.py:258-283), forward_loss (:333-350)
def op_chan_ln_fwd(m: Mem, o):
    B, C, HW = o["B"], o["C"], o["HW"]
    x = m.view(o["X"], (B, C, HW))
    mean = x.mean(1, keepdim=True)
    var = x.var(1, unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + o["EPS"])
    g, b = m.view(o["GAMMA"], (C,)), m.view(o["BETA"], (C,))
    m.view(o["Y"], (B, C, HW)).copy_((x - mean) * rstd * g.view(1, C, 1) + b.view(1, C, 1))
    mr = m.view(o["MR"], (B, HW, 2))
    mr[..., 0] = mean[:, 0]
    mr[..., 1] = rstd[:, 0]


def op_chan_ln_bwd(m: Mem, o):
    B, C, HW = o["B"], o["C"], o["HW"]
    dy, x = m.view(o["DY"], (B, C, HW)), m.view(o["X"], (B, C, HW))
    mr = m.view(o["MR"], (B, HW, 2))
    mean, rstd = mr[..., 0].unsqueeze(1), mr[..., 1].unsqueeze(1)
    xhat = (x - mean) * rstd
    g = dy * m.view(o["GAMMA"], (C,)).view(1, C, 1)
    dx = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    dst = m.view(o["DX"], (B, C, HW))
    if o["ACCUM"]:
        if o.get("DXIN", -1) >= 0:
            dst.copy_(m.view(o["DXIN"], (B, C, HW)) + dx)
        else:
            dst.add_(dx)
    else:
        dst.copy_(dx)
    if o.get("DSUM", -1) >= 0:
        m.view(o["DSUM"], (C,)).add_(dst.double().sum((0, 2)).to(m.fdtype))
    if o["DGAMMA"] >= 0:
        m.view(o["DGAMMA"], (C,)).add_((dy * xhat).double().sum((0, 2)).to(m.fdtype))
        m.view(o["DBETA"], (C,)).add_(dy.double().sum((0, 2)).to(m.fdtype))


def op_act_bwd(m: Mem, o):
    n = o["COUNT"]
    g = m.view(o["G"], (n,))
    x = m.view(o["X"], (n,))
    g.mul_(x if o["ACT"] == 5 else _act_grad(x, o["ACT"]))


def op_act_fwd(m: Mem, o):
    n = o["COUNT"]
    x = m.view(o["X"], (n,))
    act = o["ACT"]
    if o.get("BNV", -1) >= 0:
        C, HW = o["C"], o["HW"]
        bnv = m.view(o["BNV"], (4, C))
        x = (x.view(-1, C, HW) * bnv[0].view(1, C, 1) + bnv[1].view(1, C, 1)).reshape(-1)
    y = F.gelu(x) if act == 4 else (F.silu(x) if act == 2 else (F.relu(x) if act == 3 else x))
    if o.get("GATE", -1) >= 0:
        C, HW = o["C"], o["HW"]
        B = n // (C * HW)
        y = (y.view(B, C, HW) * m.view(o["GATE"], (B, C)).view(B, C, 1)).reshape(-1)
    m.view(o["Y"], (n,)).copy_(y)


def _split_qkv(t, B, H, HD, L):   # [B][3*H*HD][L] -> q, k, v each [B,H,L,HD]
    t = t.reshape(B, 3, H, HD, L).permute(1, 0, 2, 4, 3)
    return t[0], t[1], t[2]


def _attn_ls(o):
    return o["LS"] if o.get("LS", 0) else o["L"]


def op_attn_fwd(m: Mem, o):
    B, H, HD, L, LS = o["B"], o["HEADS"], o["HD"], o["L"], _attn_ls(o)
    q, k, v = _split_qkv(m.view(o["QKV"], (B, 3 * H * HD, LS))[..., :L], B, H, HD, L)
    s = (q @ k.transpose(-2, -1)) * o["SCALE"]
    p = torch.softmax(s, dim=-1)
    out = p @ v                                              # [B,H,L,HD]
    dst = m.view(o["O"], (B, H, HD, LS))
    dst.zero_()
    dst[..., :L].copy_(out.permute(0, 1, 3, 2))
    lse = m.view(o["LSE"], (B, H, LS))
    lse.zero_()
    lse[..., :L].copy_(torch.logsumexp(s, dim=-1))


def op_attn_bwd(m: Mem, o):
    B, H, HD, L, LS = o["B"], o["HEADS"], o["HD"], o["L"], _attn_ls(o)
    q, k, v = _split_qkv(m.view(o["QKV"], (B, 3 * H * HD, LS))[..., :L], B, H, HD, L)
    do = m.view(o["DO"], (B, H, HD, LS))[..., :L].permute(0, 1, 3, 2)  # [B,H,L,HD]
    p = torch.softmax((q @ k.transpose(-2, -1)) * o["SCALE"], dim=-1)
    dv = p.transpose(-2, -1) @ do
    dp = do @ v.transpose(-2, -1)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True)) * o["SCALE"]
    dq = ds @ k
    dk = ds.transpose(-2, -1) @ q
    dst = m.view(o["DQKV"], (B, 3, H, HD, LS))
    dst.zero_()
    dst[:, 0, ..., :L].copy_(dq.permute(0, 1, 3, 2))
    dst[:, 1, ..., :L].copy_(dk.permute(0, 1, 3, 2))
    dst[:, 2, ..., :L].copy_(dv.permute(0, 1, 3, 2))
    if o.get("DELTA", -1) >= 0 and o.get("O", -1) >= 0:      # delta[b][h][i] = sum_d dO[d][i] O[d][i] of the O handed in; row padding := 0
        out = m.view(o["O"], (B, H, HD, LS))[..., :L].permute(0, 1, 3, 2)
        delta = m.view(o["DELTA"], (B, H, LS))
        delta.zero_()
        delta[..., :L].copy_((do * out).sum(-1))


def op_mae_mask_index(m: Mem, o):
    B, L, keep = o["B"], o["L"], o["KEEP"]
    noise = m.view(o["NOISE"], (B, L))
    ids_shuffle = torch.argsort(noise, dim=1, stable=True)
    rank = torch.argsort(ids_shuffle, dim=1)
    m.view(o["IDS_RESTORE"], (B, L), "i64").copy_(rank)
    m.view(o["MASK"], (B, L)).copy_((rank >= keep).to(m.fdtype))
    enc = m.view(o["ENC_IDX"], (B, 1 + keep), "i32")
    enc[:, 0] = -1
    enc[:, 1:] = ids_shuffle[:, :keep].to(torch.int32)
    dec = m.view(o["DEC_IDX"], (B, 1 + L), "i32")
    dec[:, 0] = 0
    dec[:, 1:] = torch.where(rank < keep, rank + 1, torch.full_like(rank, -1)).to(torch.int32)


def op_token_gather(m: Mem, o):
    B, C, Lin, Lout = o["B"], o["C"], o["LIN"], o["LOUT"]
    LinS, LoutS = o.get("LIN_S", 0) or Lin, o.get("LOUT_S", 0) or Lout   # row strides; padding columns of OUT := 0
    src = m.view(o["IN"], (B, C, LinS))[..., :Lin]
    idx = m.view(o["IDX"], (B, Lout), "i32").long()
    fill = m.view(o["FILL"], (C,))
    got = torch.gather(src, 2, idx.clamp(min=0).unsqueeze(1).expand(-1, C, -1))
    # idx < 0 takes FILL[c]; without FILL it is 0, as the kernel writes it (plan_random_masking's absent cls slot)
    fill = fill.view(1, C, 1).expand(B, C, Lout) if fill is not None else torch.zeros_like(got)
    got = torch.where((idx >= 0).unsqueeze(1), got, fill)
    if o["POS"] >= 0:
        prow = (idx + o["POS_OFF"]) if o["POS_BY_SRC"] else torch.arange(Lout).unsqueeze(0).expand(B, -1)
        nrows = int(prow.max().item()) + 1
        pos = m.view(o["POS"], (nrows, C))
        got = got + pos[prow].permute(0, 2, 1)
    out = m.view(o["OUT"], (B, C, LoutS))
    out.zero_()
    out[..., :Lout].copy_(got)


def op_token_scatter(m: Mem, o):
    B, C, Lin, Lout = o["B"], o["C"], o["LIN"], o["LOUT"]
    LinS, LoutS = o.get("LIN_S", 0) or Lin, o.get("LOUT_S", 0) or Lout
    dout = m.view(o["DOUT"], (B, C, LoutS))[..., :Lout]
    idx = m.view(o["IDX"], (B, Lout), "i32").long()
    din = m.view(o["DIN"], (B, C, LinS))
    din.zero_()
    valid = idx >= 0
    for b in range(B):
        jj = torch.nonzero(valid[b]).flatten()
        din[b][:, idx[b, jj]] = dout[b][:, jj]
    if o["DFILL"] >= 0:
        w = (~valid).to(dout.dtype).unsqueeze(1)
        m.view(o["DFILL"], (C,)).add_((dout * w).double().sum((0, 2)).to(m.fdtype))


def _patch_cols(x, P, TUB, order):
    """x [B,C,T,H,W] -> [B, F, L]; order 'conv': f = (c,tt,py,px); 'mae': f = (tt,py,px,c)."""
    B, C, T, H, W = x.shape
    v = x.reshape(B, C, T // TUB, TUB, H // P, P, W // P, P)          # b c t tt h py w px
    if order == "conv":
        v = v.permute(0, 1, 3, 5, 7, 2, 4, 6)                           # b c tt py px t h w
    else:
        v = v.permute(0, 3, 5, 7, 1, 2, 4, 6)                           # b tt py px c t h w
    return v.reshape(B, C * TUB * P * P, (T // TUB) * (H // P) * (W // P))


def op_patchify(m: Mem, o):
    B, C, T, H, W, P, TUB = (o[k] for k in ("B", "C", "T", "H", "W", "P", "TUB"))
    x = m.view(o["X"], (B, C, T, H, W))
    inv, order = o.get("INVERSE", 0), "mae" if o.get("ORDER", 0) else "conv"
    L = (T // TUB) * (H // P) * (W // P)
    ls = o.get("LS", 0) or L
    lo = o.get("L_OFF", 0)
    out = m.view(o["OUT"], (B, C * TUB * P * P, ls))[:, :, lo:lo + L]
    if inv == 0:
        out.copy_(_patch_cols(x, P, TUB, order))
        return
    if inv == 4:             # gradient through the standardised target (opdefs.PATCHIFY)
        tgt = _patch_cols(m.view(o["IMGS"], (B, C, T, H, W)), P, TUB, "mae")      # [B, PD, L]
        n = tgt.shape[1]
        mu = tgt.mean(1, keepdim=True)
        sdev = (tgt.var(1, keepdim=True) + 1.0e-6) ** 0.5
        g = -out
        xc = tgt - mu
        out = (g - g.mean(1, keepdim=True)) / sdev - xc * (g * xc).sum(1, keepdim=True) / (sdev ** 3 * (n - 1))
        inv = 1
    if order == "conv":      # rows (c, tt, py, px)
        v = out.reshape(B, C, TUB, P, P, T // TUB, H // P, W // P).permute(0, 1, 5, 2, 6, 3, 7, 4)      # b c t tt h py w px
    else:                    # rows (tt, py, px, c)
        v = out.reshape(B, TUB, P, P, C, T // TUB, H // P, W // P).permute(0, 4, 5, 1, 6, 2, 7, 3)
    v = v.reshape(B, C, T, H, W)
    if inv == 1:
        x.copy_(v)
    elif inv == 2:
        x.copy_(-v)
    else:
        x.add_(v)


def _mae_loss_terms(m: Mem, o):
    B, C, T, H, W, P, TUB, LP, LO = (o[k] for k in ("B", "C", "T", "H", "W", "P", "TUB", "LP", "L_OFF"))
    x = m.view(o["IMGS"], (B, C, T, H, W))
    target = _patch_cols(x, P, TUB, "mae")                               # [B, PD, L]
    PD, L = target.shape[1], target.shape[2]
    if o["NORM_PIX"]:
        mean = target.mean(1, keepdim=True)
        var = target.var(1, keepdim=True)                                # unbiased, as torch.var default
        target = (target - mean) / (var + 1.0e-6) ** 0.5
    pred = m.view(o["PRED"], (B, PD, LP))[:, :, LO:LO + L]
    mask = m.view(o["MASK"], (B, L))
    return pred, target, mask, PD, L


def op_mae_loss_fwd(m: Mem, o):
    pred, target, mask, PD, L = _mae_loss_terms(m, o)
    per = ((pred - target) ** 2).mean(1)
    acc = m.view(o["ACC"], (2,), "f64")
    acc[0] = (per * mask).double().sum()
    acc[1] = mask.double().sum()
    m.view(o["LOSS"], (1,)).copy_((acc[0] / acc[1]).to(m.fdtype).reshape(1))


def op_mae_loss_bwd(m: Mem, o):
    pred, target, mask, PD, L = _mae_loss_terms(m, o)
    acc = m.view(o["ACC"], (2,), "f64")
    go = m.view(o["GOUT"], (1,)) if o["GOUT"] >= 0 else torch.ones(1, dtype=m.fdtype)
    d = 2.0 * (pred - target) * mask.unsqueeze(1) * (go[0] / (PD * acc[1].to(m.fdtype)))
    dst = m.view(o["DPRED"], (o["B"], PD, o["LP"]))
    dst.zero_()
    dst[:, :, o["L_OFF"]:o["L_OFF"] + L] = d


def op_transpose_cl(m: Mem, o):
    B, C, L, LO, Lout = o["B"], o["C"], o["L"], o["L_OFF"], o["LOUT"]
    x = m.view(o["X"], (B, C, L))
    ys, yo = o.get("YS", 0), o.get("Y_OFF", 0)
    if ys <= 0:
        ys, yo = C, 0
    y = m.view(o["Y"], (B, Lout, ys))
    y.zero_()
    y[:, :, yo:yo + C] = x[:, :, LO:LO + Lout].permute(0, 2, 1)


def op_upsample_zero(m: Mem, o):
    B, C, H, W, S, HO, WO = o["B"], o["C"], o["H"], o["W"], o["S"], o["HO"], o["WO"]
    x = m.view(o["X"], (B, C, H, W))
    y = m.view(o["Y"], (B, C, HO, WO))
    y.zero_()
    hh, ww = min(H, (HO + S - 1) // S), min(W, (WO + S - 1) // S)
    y[:, :, 0:hh * S:S, 0:ww * S:S] = x[:, :, :hh, :ww]


def op_ids_to_dec_idx(m: Mem, o):
    B, L, keep = o["B"], o["L"], o["KEEP"]
    ids = m.view(o["IDS"], (B, L), "i64")
    dec = m.view(o["DEC_IDX"], (B, 1 + L), "i32")
    dec[:, 0] = 0
    dec[:, 1:] = torch.where((ids >= 0) & (ids < keep), ids + 1, torch.full_like(ids, -1)).to(torch.int32)


def op_confusion(m: Mem, o):
    n, C = o["COUNT"], o["C"]
    pred = m.view(o["PRED"], (n,), "i64")
    lab = m.view(o["LABELS"], (n,), "i64")
    ok = (pred >= 0) & (pred < C) & (lab >= 0) & (lab < C)
    idx = lab[ok] * C + pred[ok]
    m.view(o["HIST"], (C * C,), "i64").add_(torch.bincount(idx, minlength=C * C))


def op_se_bn_sums(m: Mem, o):
    B, C, HW = o["B"], o["C"], o["HW"]
    g, y, bnv = m.view(o["G"], (B, C, HW)), m.view(o["Y"], (B, C, HW)), m.view(o["BNV"], (4, C))
    u = y * bnv[0].view(1, C, 1) + bnv[1].view(1, C, 1)
    ap = _act_grad(u, o["ACT"])
    xhat = (y - bnv[2].view(1, C, 1)) * bnv[3].view(1, C, 1)
    m.view(o["DGATE"], (B, C)).copy_((g * F.silu(u)).sum(-1))
    ps = m.view(o["PS"], (4, B, C))
    ps[0] = (g * ap).sum(-1)
    ps[1] = ap.sum(-1)
    ps[2] = (g * ap * xhat).sum(-1)
    ps[3] = (ap * xhat).sum(-1)


def op_se_bn_combine(m: Mem, o):
    B, C = o["B"], o["C"]
    ps = m.view(o["PS"], (4, B, C)).double()
    mul, add = m.view(o["MULBC"], (B, C)), m.view(o["ADDBC"], (B, C))
    mul = mul.double() if mul is not None else torch.ones(B, C, dtype=torch.float64)
    add = add.double() * o["ADDSCALE"] if add is not None else torch.zeros(B, C, dtype=torch.float64)
    st = m.view(o["STATS2"], (2, C), "f64")
    st[0] = (mul * ps[0] + add * ps[1]).sum(0)
    st[1] = (mul * ps[2] + add * ps[3]).sum(0)


def op_space_to_depth(m: Mem, o):
    B, C, H, W = o["B"], o["C"], o["H"], o["W"]
    m.view(o["Y"], (B, 4 * C, H, W)).copy_(_unshuffle2(m.view(o["X"], (B, C, 2 * H, 2 * W))))


def op_im2col(m: Mem, o):
    B, C, H, W, KH, KW, S, PT, PL, HO, WO = (o[k] for k in ("B", "C", "H", "W", "KH", "KW", "STRIDE", "PAD_T", "PAD_L", "HO", "WO"))
    x = m.view(o["X"], (B, C, H, W))
    pb, pr = (HO - 1) * S + KH - H - PT, (WO - 1) * S + KW - W - PL
    xp = F.pad(x, (PL, max(pr, 0), PT, max(pb, 0)))[:, :, :(HO - 1) * S + KH, :(WO - 1) * S + KW]
    cols = F.unfold(xp, (KH, KW), stride=S)                      # [B, C*KH*KW, HO*WO], rows ordered (c, ky, kx)
    m.view(o["Y"], (B, C * KH * KW, HO * WO)).copy_(cols)


def op_tile_prep(m: Mem, o):
    """crop -> flips -> normalise (two separately rounded fp32 steps, as numpy's `img -= mean; img *= denominator`) + label LUT"""
    B, C, H, W, S, N = o["B"], o["C"], o["H"], o["W"], o["S"], o["NSRC"]
    raw = m.view(o["RAW"], (N, C, H, W), "i16")
    par = m.view(o["PARAMS"], (B, 4), "i32")
    norm = m.view(o["NORM"], (2, C)).to(torch.float32)
    x = m.view(o["X"], (B, C, S, S))
    y = m.view(o["Y"], (B, S, S), "i64")
    lab = m.view(o["LABELS"], (N, H, W), "u8")
    lut = m.view(o["LUT"], (256,), "i32")
    for b in range(B):
        src, y0, x0, fl = (int(v) for v in par[b])
        img = raw[src, :, y0:y0 + S, x0:x0 + S].to(torch.float32)
        msk = lab[src, y0:y0 + S, x0:x0 + S].long() if y is not None else None
        if fl & 1:
            img = img.flip(-1)
            msk = msk.flip(-1) if msk is not None else None
        if fl & 2:
            img = img.flip(-2)
            msk = msk.flip(-2) if msk is not None else None
        img = img - norm[0].view(C, 1, 1)
        img = img * norm[1].view(C, 1, 1)
        x[b].copy_(img)
        if y is not None:
            y[b].copy_(lut[msk].long())


def op_drop_gate(m: Mem, o):
    n = o["COUNT"]
    u = m.view(o["U"], (n,))
    m.view(o["GATE"], (n,)).copy_((u >= o["P"]).to(m.fdtype) / (1.0 - o["P"]))


DISPATCH = {
    "MEMSET": op_memset, "AXPY": op_axpy, "WEIGHT_PACK": op_weight_pack, "CONV": op_conv, "WGRAD": op_wgrad, "WGRAD_FINALIZE": op_wgrad_finalize,
    "DWCONV_FWD": op_dwconv_fwd, "DWCONV_DGRAD": op_dwconv_dgrad, "DWCONV_WGRAD": op_dwconv_wgrad,
    "BN_FINALIZE": op_bn_finalize, "SE_POOL": op_se_pool, "SE_FC": op_se_fc, "SE_FC_BWD": op_se_fc_bwd,
    "SE_BWD_REDUCE": op_se_bwd_reduce, "BN_BWD_REDUCE": op_bn_bwd_reduce, "BN_BWD_FINALIZE": op_bn_bwd_finalize,
    "BN_BWD_APPLY": op_bn_bwd_apply, "BN_RESIDUAL": op_bn_residual, "CHANNEL_SUM": op_channel_sum,
    "LOSS_FWD": op_loss_fwd, "LOSS_BWD": op_loss_bwd, "ARGMAX": op_argmax,
    "CHAN_LN_FWD": op_chan_ln_fwd, "CHAN_LN_BWD": op_chan_ln_bwd, "ACT_BWD": op_act_bwd, "ACT_FWD": op_act_fwd, "ATTN_FWD": op_attn_fwd,
    "ATTN_BWD": op_attn_bwd, "TILE_PREP": op_tile_prep, "SPACE_TO_DEPTH": op_space_to_depth, "SE_FC_WGRAD": op_se_fc_wgrad, "SE_BN_SUMS": op_se_bn_sums, "SE_BN_COMBINE": op_se_bn_combine, "MAE_MASK_INDEX": op_mae_mask_index, "TOKEN_GATHER": op_token_gather,
    "TOKEN_SCATTER": op_token_scatter, "PATCHIFY": op_patchify, "MAE_LOSS_FWD": op_mae_loss_fwd,
    "MAE_LOSS_BWD": op_mae_loss_bwd, "TRANSPOSE_CL": op_transpose_cl, "IDS_TO_DEC_IDX": op_ids_to_dec_idx, "UPSAMPLE_ZERO": op_upsample_zero, "DROP_GATE": op_drop_gate, "CONFUSION": op_confusion, "IM2COL": op_im2col,
}


def unpack(packed: np.ndarray, opdefs) -> list[tuple[str, dict]]:
    """Decode packed S2kOp records back to (kind, fields) — the emulator consumes exactly what
    the native executor would."""
    names = {v: k for k, v in opdefs.KIND.items()}
    out = []
    for rec in packed:
        kind = names[int(rec["kind"])]
        t, n, d, f = opdefs.OPS[kind]
        o = {}
        for j, k in enumerate(t):
            o[k] = int(rec["t"][j])
        for j, k in enumerate(n):
            o[k] = int(rec["n"][j])
        for j, k in enumerate(d):
            o[k] = int(rec["d"][j])
        for j, k in enumerate(f):
            o[k] = float(rec["f"][j])
        o["_flags"] = int(rec["flags"])
        out.append((kind, o))
    return out


def run_program(packed: np.ndarray, bases: dict[int, torch.Tensor], opdefs, wide: bool = False,
                narrow_bases=(), b16_operands: bool = False) -> None:
    """b16_operands (with wide; no existing caller passes it): FLAG_BF16 stages become the float64 reference of the bf16 operation
    (_bf16_operands) instead of the unrounded float64 emulation; every other stage, and every call without it, is unchanged."""
    assert wide or not b16_operands
    m = Mem(bases, wide, narrow_bases, b16_operands)
    with torch.no_grad():
        for kind, o in unpack(packed, opdefs):
            if kind in ("DWCONV_DGRAD", "DWCONV_WGRAD", "LOSS_BWD"):
                with torch.enable_grad():
                    DISPATCH[kind](m, o)
            else:
                DISPATCH[kind](m, o)
