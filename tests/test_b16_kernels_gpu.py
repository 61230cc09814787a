"""The bf16 matrix-core kernels, instantiation by instantiation: conv_bf16_kernel (csrc/conv_bf16.hip) and wgrad_bf16_kernel
(csrc/wgrad_bf16.hip) in both of their modes - bf16-mixed (FLAG_BF16, kernel family 2) and f32-split (FLAG_SPLIT, family 5) -
launched as one CONV / WGRAD record through the C ABI (CONV behind a WEIGHT_PACK record, as a plan does).

One table per kernel and mode (CONV_BF16, CONV_SPLIT, WGRAD_BF16, WGRAD_SPLIT) plus the records the launchers must decline or refuse
(DECLINED).  Which template instantiation a row reaches, and which loop edges, is tests/b16_dispatch.py's restatement of the
launchers; tests/test_b16_dispatch_cpu.py checks without a GPU that the tables reach every instantiation the launch sites can
produce at default tuning and every edge it lists.  Output channel c (CONV) / column c (WGRAD) is scaled by 2^-(c mod 8), so that a
value in the wrong channel, or an error in one row of a tile, shows against that channel's own max |ref|.  Every row is held

  * to the kernel family the launcher must take: 2, 5, or on a decline the f32 family tests/conv_dispatch.py (CONV) or
    tests/wgrad_dispatch.py (WGRAD) restates;
  * to leaving every byte of the arena outside the stage's outputs as uploaded (Y is NaN-filled or, with YC > M, a channel slice of
    a wider tensor whose other channels must stay bit-identical; WGS columns outside the stage's slice likewise).

Family 2, random data: the project's bars (tests/test_ops_gpu._conv_case / _wgrad_case: CONV 1e-4 without a prologue, 1e-3 with one
- an activated value next to a bf16 rounding boundary may round the other way on the GPU; WGRAD 1e-3), applied to the whole tensor
AND to every channel / column, against the f32 oracle on bf16-rounded operands AND against the float64 reference of the bf16
operation (oracle/ops_ref.run_program(wide=True, b16_operands=True): prologue in f32, operands rounded to bf16, products, sums,
epilogue and statistics in float64); statistics alike.

Family 2, exact data: every row also runs on lattice data - inputs, BatchNorm scale / shift, SE gate and weights small integers
times powers of two, chosen so that an activated operand has at most 8 significant bits (bf16 rounding is the identity: asserted on
the CPU) and a whole reduction fewer than 24: every product and every partial sum is exact in f32 in any order, split-K partials and
atomics included.  ReLU and AFFINE are exact by construction; SiLU and GELU arguments lie at |u| >= 100, where the activation
returns u or 0 exactly.  Bias, residual and old Y are lattice values too, so at most three epilogue adds round: the bar is 1e-6 of
each channel's max |ref| against the float64 reference, and a WGRAD row (which accumulates into a lattice WGS) must be bit-equal.

Family 5: the three-way scheme of tests/test_f32_split_ops_gpu.py - split vs the f32 oracle at 1e-4 (WGRAD 2e-4); error against
float64 at most 2 x the exact-f32 kernel's on the same bytes + 2^-22 - for the whole tensor and for every channel / column; rows
tagged spread use operands with all 23 significand bits random over 2^-20 .. 2^20.  A split stage never falls back: every DECLINED
split row must raise S2kError with the launcher's message.

Random data of a family-2 row avoids bf16 rounding boundaries (settle): an element whose activated value lies within 1/64 bf16 ulp of
one is drawn again, so that the GPU's fma / v_exp + v_rcp prologue and the oracle's round every operand to the same neighbour and
the bars hold per channel on short reductions too (without it single flips reach 1.7e-3 of a channel's max at K = 72 .. 520).

Rows: 431 (CONV_BF16 89, CONV_SPLIT 69, WGRAD_BF16 41, WGRAD_SPLIT 20, DECLINED 23, PROD 189); they reach all 76 + 56 reachable
instantiations of conv_bf16_kernel (parsed: 76 + 58) and all 28 + 12 of wgrad_bf16_kernel (tests/test_b16_dispatch_cpu.py).
Worst on an MI355X (f32 oracle / float64 reference), whole tensor | per channel or column:
  CONV_BF16   Y 5.3e-7 / 3.3e-7 | 9.4e-7 / 5.3e-7; STATS 6.2e-8 / 6.0e-8 | 1.5e-6 / 4.4e-6; lattice rows 0 (bit-equal)
  WGRAD_BF16  WGS 4.3e-7 / 4.4e-7 | 7.3e-7 / 7.3e-7; lattice rows bit-equal
  CONV_SPLIT  Y 1.0e-6 / 8.7e-7 | 1.4e-6 / 1.2e-6; STATS 8.6e-8 | 6.1e-6; against float64 split 8.7e-7 | 1.2e-6, the f32 kernels 1.4e-6 | 1.7e-6
  WGRAD_SPLIT WGS 5.5e-7 / 5.5e-7 | 9.2e-7 / 9.3e-7; against float64 split 5.5e-7 | 9.3e-7, the f32 kernels 4.7e-7 | 7.9e-7
  PROD        Y 8.0e-6 | 1.9e-5, WGS 1.3e-5 | 4.2e-5 (the 2048- and 3072-channel reductions), STATS 1.5e-7 | 7.9e-6; lattice rows bit-equal
431 cases in 35 s; the slowest row (a 3x3 weight gradient at 224 x 224, 5.5 G multiply-adds) 1.5 s."""
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import ops_ref
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan.program import Program
from tests import b16_dispatch as BD
from tests import conv_dispatch as CD
from tests import wgrad_dispatch as WD
from tests.test_ops_gpu import WS, Case

NO, AF, SI, RE, GE = D.PRO_NONE, D.PRO_AFFINE, D.PRO_SILU, D.PRO_RELU, D.PRO_GELU
FLOOR = 2.0 ** -22
EXACT_TOL = 1e-6


class B16Case(Case):
    """Case whose float64 oracle is the float64 reference OF the bf16 operation, and which lays out the bf16 / split weight copies"""
    oracle_packed = None      # a declined stage: the oracles run this program (the record without its flag) instead

    def oracles(self, packed, ref64=False):
        if self.oracle_packed is not None:
            packed = self.oracle_packed
        cpu = self.image()
        wide = None
        if ref64:
            wide = torch.zeros(2 * cpu.numel(), dtype=torch.uint8)
            for name, (ref, data) in self.items.items():
                wdt = {"f32": torch.float64, "bf16": torch.float32}.get(ref.dtype)
                b = (data.to(wdt) if wdt is not None else data).contiguous().reshape(-1).view(torch.uint8)
                wide[2 * ref.off:2 * ref.off + b.numel()] = b
            ops_ref.run_program(packed, {WS: wide}, D, wide=True, b16_operands=True)
        ops_ref.run_program(packed, {WS: cpu}, D)
        self.wide = wide
        return cpu, wide

    def pack_split(self, wt, M, K, T, s_m, s_k, s_t):
        """WEIGHT_PACK of one weight with its hi / mid / lo planes (tests/test_f32_split_ops_gpu.Case.pack)"""
        MP, KP = (M + 127) // 128 * 128, (K + 63) // 64 * 64
        dst = self.t(f"packed{len(self.items)}", (KP * T, MP), "nan")
        row = [wt.off // 4, dst.off // 4, M, K, T, s_m, s_k, s_t, 0, MP, KP, 0]
        tab = self.t(f"packtab{len(self.items)}", (1, 12), torch.tensor([row], dtype=torch.int32), "i32")
        self.arena.alloc("gap", (dst.off // 8 + 64,))      # the split region must lie beyond 1.5 x dst.off
        dsts = self.t(f"packeds{len(self.items)}", (3 * KP * T * MP // 2,), "nan")
        zero = self.arena.alloc("zero", (1,))
        fields = dict(TABLE=tab, SRC=zero.at(-(zero.off // 4)), DST=zero.at(-(zero.off // 4)), TOTAL=KP * T * MP, N_ENTRIES=1,
                      SPLIT_BASE=dsts.off - 3 * dst.off // 2)
        assert fields["SPLIT_BASE"] > 0 and fields["SPLIT_BASE"] % 16 == 0
        self.packed += [dst, dsts]
        return ("WEIGHT_PACK", fields), dst, MP, dsts


def spread(shape, gen):
    """values over 2^-20 .. 2^20 with random signs and all 23 stored significand bits random: bf16 keeps 8 of them"""
    e = torch.randint(-20, 21, shape, generator=gen).double()
    mant = 1.0 + torch.rand(shape, generator=gen, dtype=torch.float64)
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (sign * mant * torch.pow(2.0, e)).float()


def ints(gen, shape, lo, hi, nonzero=False):
    v = torch.randint(lo, hi + 1, shape, generator=gen).float()
    if nonzero:
        v = torch.where(v == 0, torch.ones_like(v), v)
    return v


def pick(gen, shape, values):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=gen)]


def lattice_bnv(c, name, C, pro):
    """BatchNorm {scale, shift, -, -} on the lattice: AFFINE / ReLU: u = scale * x + shift is a multiple of 1/2 with |u| <= 6;
    SiLU / GELU: |u| >= 112 in multiples of 16 (the activation returns u or 0 exactly), |u| <= 272"""
    if pro in (SI, GE):
        scale, shift = pick(c.gen, (C,), [128.0, -128.0]), pick(c.gen, (C,), [-16.0, 0.0, 16.0])
    else:
        scale, shift = pick(c.gen, (C,), [0.5, 1.0, 2.0, -1.0]), ints(c.gen, (C,), -2, 2)
    return c.t(name, (4, C), torch.stack([scale, shift, torch.zeros(C), torch.ones(C)]))


def lattice_x(c, pro, shape):
    """inputs on the lattice: integers in -2 .. 2 (SiLU / GELU: +-1, +-2, so that no argument is near 0)"""
    return ints(c.gen, shape, -2, 2, nonzero=pro in (SI, GE))


def settle(c, name, bnv, gate, pro, C, scale=None):
    """Random data of a family-2 row: re-draw every input element whose ACTIVATED value lies within 1/64 bf16 ulp (512 f32 ulps) of a
    bf16 rounding boundary, until none does.  The kernels evaluate the prologue with one fma and SiLU with v_exp + v_rcp, the oracle
    with a multiply, an add and exp: a few f32 ulps apart, so such an element could round to the other bf16 neighbour on the GPU -
    2^-8 of one operand, which over a short reduction is more than the bar of a single channel.  With these elements gone both
    sides round every operand alike and the bars are left to the kernel's products and sums."""
    if not pro and gate is None:
        return
    x = c.items[name][1]
    if x.dtype != torch.float32:        # (a stored-bf16 operand has no prologue: such a record is refused)
        return
    item = lambda n: None if n is None else c.items[n][1]       # noqa: E731
    for _ in range(64):
        a = ops_ref._pro(x, item(bnv), item(gate), pro, C)
        r = a.to(torch.bfloat16).float()
        ulp = torch.pow(2.0, torch.frexp(r)[1].float() - 8.0)
        bad = ((a - r).abs() / ulp > 0.5 - 1.0 / 64) & (r != 0)
        if not bad.any():
            return
        fresh = torch.randn(x.shape, generator=c.gen) * (1.0 if scale is None else scale)
        x[bad] = fresh[bad]
    raise AssertionError(f"{name}: activated values stay near bf16 rounding boundaries")


# ---------------------------------------------------------------------------------------------------------------------------------
# CONV rows
# ---------------------------------------------------------------------------------------------------------------------------------
def R(B, C1, H, W, M, C2=0, k=1, s=1, pro=0, pro2=None, gate=False, x16=False, bias=False, stats=False, beta=0, res=False, scratch=False,
      yc=None, mode=0, nrep=None, split=False, spread=False, seed=0, raises=None, prod=False):
    """One CONV case.  C2: channels of a second (concat) source; k, s: kernel size and stride (3x3 pads 1); pro / pro2: prologue
    codes (pro2 defaults to pro); gate / bias / stats / res / scratch: the record carries GATE1 / BIAS / STATS / RES / SCRATCH; x16: X1
    is stored as bf16 (X1_BF16); beta: accumulate into Y; yc: channel stride of Y (> M: Y is a channel slice of a wider tensor);
    mode: opdefs.MODE_*; nrep: statistics replicas (default opdefs.stats_replicas); split: FLAG_SPLIT instead of FLAG_BF16; spread:
    operands with 23 random significand bits over 2^-20 .. 2^20; raises: a declined record the f32 launcher refuses with this message."""
    return dict(prod=prod, raises=raises, kind="CONV", B=B, C1=C1, H=H, W=W, M=M, C2=C2, k=k, s=s, pro=pro, pro2=(pro if pro2 is None else pro2) if C2 else 0, gate=gate,
                x16=x16, bias=bias, stats=stats, beta=beta, res=res, scratch=scratch, yc=yc, mode=mode, nrep=nrep, split=split, spread=spread,
                seed=seed)


def RW(B, M, C, H, W, k=1, prop=0, proq=0, gateq=False, gatep=False, p16=False, ct=None, coff=0, s=1, split=False, spread=False, seed=0, raises=None, prod=False):
    """One WGRAD case: dW[tap][m][c] += sum_pix Ppro[m][pix] * Qpro[c][pix + tap].  prop / proq: prologues on P / Q; gateq: SE gate on Q;
    p16: P is stored as bf16 (P_BF16); ct, coff: WGS is the column slice [coff, coff + C) of a [T][M][ct] tensor."""
    return dict(prod=prod, raises=raises, kind="WGRAD", B=B, M=M, C=C, H=H, W=W, k=k, s=s, prop=prop, proq=proq, gateq=gateq, gatep=gatep, p16=p16, ct=ct or C, coff=coff,
                split=split, spread=spread, seed=seed)


def rid(r) -> str:
    if r["kind"] == "CONV":
        o = [f"{r['B']}x{r['C1']}" + (f"+{r['C2']}" if r["C2"] else "") + f"x{r['H']}x{r['W']}-M{r['M']}"]
        if r["k"] != 1 or r["s"] != 1:
            o.append(f"k{r['k']}s{r['s']}")
        if r["pro"] or r["pro2"]:
            o.append(f"pro{r['pro']}" + (f"{r['pro2']}" if r["C2"] else ""))
        o += [n for n in ("gate", "x16", "bias", "stats", "beta", "res", "scratch", "split", "spread") if r[n]]
        if r["yc"]:
            o.append(f"yc{r['yc']}")
        if r["mode"]:
            o.append(f"mode{r['mode']}")
        if r["nrep"]:
            o.append(f"nrep{r['nrep']}")
    else:
        o = [f"w{r['B']}x{r['M']}x{r['C']}x{r['H']}x{r['W']}"]
        if r["k"] != 1 or r["s"] != 1:
            o.append(f"k{r['k']}s{r['s']}")
        if r["prop"] or r["proq"]:
            o.append(f"pro{r['prop']}{r['proq']}")
        o += [n for n in ("gateq", "gatep", "p16", "split", "spread") if r[n]]
        if r["ct"] != r["C"]:
            o.append(f"ct{r['ct']}+{r['coff']}")
    if r["seed"]:
        o.append(f"s{r['seed']}")
    if r["prod"]:
        o.append("prod")
    return "-".join(o)


def geometry(r):
    """(HO, WO, PAD) of a row"""
    if r["k"] == 1:
        return r["H"], r["W"], 0
    if r["s"] == 1:
        return r["H"], r["W"], 1
    return -(-r["H"] // 2), -(-r["W"] // 2), 1      # (H, W even in the tables: TF-SAME pads 0 before, the f32 kernels' business)


def nrep_of(r) -> int:
    return (r["nrep"] or D.stats_replicas(r["M"])) if r["stats"] else 1


def record(r) -> dict:
    """the row as tests/b16_dispatch.conv's / wgrad's keyword arguments"""
    ho, wo, pad = geometry(r)
    flags = BD.FLAG_SPLIT if r["split"] else BD.FLAG_BF16
    if r["kind"] == "CONV":
        pad = pad if r["s"] == 1 else 0
        return dict(B=r["B"], C1=r["C1"], C2=r["C2"], H=r["H"], W=r["W"], M=r["M"], KH=r["k"], KW=r["k"], STRIDE=r["s"], PAD_T=pad, PAD_L=pad, HO=ho,
                    WO=wo, PRO1=r["pro"], PRO2=r["pro2"], MODE=r["mode"], GATE=r["gate"], BIAS=r["bias"], RES=r["res"], STATS=r["stats"],
                    SCRATCH=r["scratch"], BETA=r["beta"], YC=r["yc"], NREP=nrep_of(r), X1_BF16=int(r["x16"]), flags=flags)
    pad = pad if r["s"] == 1 else 0
    return dict(B=r["B"], M=r["M"], C=r["C"], CTOT=r["ct"], H=r["H"], W=r["W"], KH=r["k"], KW=r["k"], STRIDE=r["s"], PAD_T=pad, PAD_L=pad, HO=ho, WO=wo,
                PROP=r["prop"], PROQ=r["proq"], GATEP=r["gatep"], GATEQ=r["gateq"], P_BF16=int(r["p16"]), flags=flags)


def launch(r):
    """the restated launcher's verdict on a row: a Cv / Wv"""
    return BD.conv(**record(r)) if r["kind"] == "CONV" else BD.wgrad(**record(r))


def f32_launch(r):
    """the f32 launchers' verdict on a row without its flag: tests/conv_dispatch.py (CONV) / tests/wgrad_dispatch.py (WGRAD; every
    allocation of a Case is 16-byte aligned)"""
    rec = record(r)
    rec.pop("X1_BF16" if r["kind"] == "CONV" else "P_BF16")
    rec["flags"] = 0
    return CD.dispatch(**rec) if r["kind"] == "CONV" else WD.dispatch(**rec)


def f32_family(r):
    """the kernel family that takes a declined row (tests/conv_dispatch.py, tests/wgrad_dispatch.py)"""
    return f32_launch(r).family


def f32_has(r) -> bool:
    """the exact-f32 kernels take the row (tests/wgrad_dispatch.py: launch_wg instantiates a prologue on one side at most, never AFFINE;
    3x3: none or ReLU on Q), so that the f32-split scheme has its third leg"""
    if r["kind"] == "CONV":
        return True
    return f32_launch(r).result != "error"


def row_edges(r) -> frozenset:
    """the launch's edges (Cv.edges / Wv.edges) + what the record itself asks of the kernel"""
    v = launch(r)
    e = set(v.edges) if v.result in (2, 5) else set()
    if r["kind"] == "CONV":
        used = min(v.nrep, max(v.n_mtiles * v.n_ntiles, 1)) if r["stats"] else 0
        e.add(f"prologue {r['pro']}")
        named = (("SE gate", r["gate"]), ("bias", r["bias"]), ("statistics", r["stats"]), ("beta", r["beta"]), ("residual", r["res"]),
                 ("concat", r["C2"] > 0), ("YC > M", bool(r["yc"]) and r["mode"] == 0 and r["yc"] > r["M"]), ("X16", r["x16"]),
                 ("M one past a tile", v.BM > 0 and r["M"] % v.BM == 1), ("statistics: several replicas", used > 1),
                 ("statistics: one replica", used == 1), (f"statistics: reduction width {v.G}", r["stats"] and v.G > 0 and v.splits == 1),
                 ("spread operands", r["spread"]))
    else:
        e |= {f"P prologue {r['prop']}", f"Q prologue {r['proq']}"}
        named = (("gate on Q", r["gateq"]), ("P16", r["p16"]), ("C < 8", r["C"] < 8), ("CTOT > C with a column offset", r["ct"] > r["C"] and r["coff"] > 0),
                 ("gate on Q over a tile that straddles images", r["gateq"] and v.images_per_tile >= 2), ("spread operands", r["spread"]))
    e |= {n for n, on in named if on}
    if r["kind"] == "CONV" and v.splits > 1:
        e |= {f"reduce tail: {n}" for n in ("bias", "statistics", "beta", "residual") if n in e}
    return frozenset(e)


def build_conv(r, data="random"):
    """(Case, outputs, the WEIGHT_PACK record, the CONV record's fields) of a row; data: "random", "exact" (the lattice) or "spread" """
    B, C1, C2, H, W, M, k, mode = r["B"], r["C1"], r["C2"], r["H"], r["W"], r["M"], r["k"], r["mode"]
    Ho, Wo, pad = geometry(r)
    pad = pad if r["s"] == 1 else 0
    c = B16Case(r["seed"])
    g = c.gen
    T, Ct = k * k, C1 + C2
    exact = data == "exact"
    xdt = "bf16" if r["x16"] else "f32"
    fill = (lambda sh, pro: lattice_x(c, pro, sh)) if exact else ((lambda sh, pro: spread(sh, g)) if data == "spread" else (lambda sh, pro: torch.randn(sh, generator=g)))
    x1 = c.t("x1", (B, C1, H, W), fill((B, C1, H, W), r["pro"]), xdt)
    x2 = c.t("x2", (B, C2, H, W), fill((B, C2, H, W), r["pro2"])) if C2 else None
    bnv1 = (lattice_bnv(c, "bnv1", C1, r["pro"]) if exact else c.bnv("bnv1", C1)) if r["pro"] else None
    bnv2 = (lattice_bnv(c, "bnv2", C2, r["pro2"]) if exact else c.bnv("bnv2", C2)) if (C2 and r["pro2"]) else None
    g1 = None
    if r["gate"]:
        g1 = c.t("gate1", (B, C1), pick(g, (B, C1), [0.5, 1.0, 2.0, 0.25])) if exact else c.t("gate1", (B, C1), "rand")
    if data == "random" and not r["split"]:
        settle(c, "x1", "bnv1" if r["pro"] else None, "gate1" if r["gate"] else None, r["pro"], C1)
        if C2:
            settle(c, "x2", "bnv2" if r["pro2"] else None, None, r["pro2"], C2)
    # output channel c is scaled by 2^-(c mod 8) - weights, bias, residual and the old content of Y alike (an exact scaling)
    nch = M // 4 if mode == D.MODE_CONVT_SCATTER else M
    YC = r["yc"] or nch
    chs = 0.5 ** (torch.arange(YC) % 8)

    def val(shape, scale=1.0):      # epilogue terms: lattice integers (exact) or normal deviates
        return ints(g, shape, -8, 8) if exact else torch.randn(shape, generator=g) * scale
    if mode == D.MODE_CONVT_SCATTER:     # ConvTranspose weights [Cin][Cout][2x2]: row m = (co, dy, dx)
        w0 = ints(g, (C1, nch, 4), -4, 4) if exact else (spread((C1, nch, 4), g) if data == "spread" else torch.randn(C1, nch, 4, generator=g) * (1.0 / Ct) ** 0.5)
        wt, (sm, sk, st) = c.t("wt", (C1, nch, 4), w0 * chs[:nch].view(1, nch, 1)), (1, M, 1)
    else:
        w0 = ints(g, (M, Ct, T), -4, 4) if exact else (spread((M, Ct, T), g) if data == "spread" else torch.randn(M, Ct, T, generator=g) * (1.0 / (Ct * T)) ** 0.5)
        wt, (sm, sk, st) = c.t("wt", (M, Ct, T), w0 * chs[:M].view(M, 1, 1)), (Ct * T, T, 1)
    bs = c.t("bias", (nch,), val((nch,)) * chs[:nch]) if r["bias"] else None
    yshape = (B, YC, 2 * Ho, 2 * Wo) if mode == D.MODE_CONVT_SCATTER else (B, YC, Ho, Wo)
    y = c.t("y", yshape, val(yshape) * chs.view(1, YC, 1, 1) if (r["beta"] or YC > M) else "nan")
    nrep = nrep_of(r)
    st_ref = c.t("stats", (nrep, 2, M), "zeros", "f64") if r["stats"] else None
    extra = {}
    if r["res"]:
        extra["RES"] = c.t("res", yshape, val(yshape, 1.5) * chs.view(1, YC, 1, 1))
    if r["scratch"]:
        extra["SCRATCH"] = c.t("scratch", (8 * B * YC * Ho * Wo,), "nan")
    if r["split"]:
        pre, wp, MP, wtb = c.pack_split(wt, M, Ct, T, sm, sk, st)
    else:
        pre, wp, MP, wtb = c.pack(wt, M, Ct, T, sm, sk, st, 0, bf16=True)
    fields = dict(NREP=nrep, X1=x1, BNV1=bnv1, GATE1=g1, X2=x2, BNV2=bnv2, WT=wp, BIAS=bs, Y=y, STATS=st_ref, B=B, C1=C1, C2=C2, H=H, W=W, M=M, KH=k,
                  KW=k, STRIDE=r["s"], PAD_T=pad, PAD_L=pad, HO=Ho, WO=Wo, PRO1=r["pro"], PRO2=r["pro2"], MODE=mode, W_SM=1, W_SK=T * MP, W_ST=MP,
                  FLIP=0, BETA=r["beta"], YC=YC, X1_BF16=int(r["x16"]), WTB=wtb, _flags=D.FLAG_SPLIT if r["split"] else D.FLAG_BF16, **extra)
    return c, ["y"] + (["stats"] if r["stats"] else []), [pre], fields


def build_wgrad(r, data="random"):
    """(Case, outputs, no pre-records, the WGRAD record's fields) of a row"""
    B, M, C, CT, H, W, k = r["B"], r["M"], r["C"], r["ct"], r["H"], r["W"], r["k"]
    Ho, Wo, pad = geometry(r)
    pad = pad if r["s"] == 1 else 0
    c = B16Case(r["seed"])
    g = c.gen
    T = k * k
    exact = data == "exact"
    fill = (lambda sh, pro: lattice_x(c, pro, sh)) if exact else ((lambda sh, pro: spread(sh, g)) if data == "spread" else (lambda sh, pro: torch.randn(sh, generator=g)))
    P = c.t("p", (B, M, Ho, Wo), fill((B, M, Ho, Wo), r["prop"]), "bf16" if r["p16"] else "f32")
    # column c of WGS is scaled by 2^-(c mod 8): Q channel c and its BatchNorm shift (u = scale * q + shift scales with its channel -
    # AFFINE and ReLU exactly), and the old content of WGS
    cols = 0.5 ** (torch.arange(CT) % 8)
    qs = cols[r["coff"]:r["coff"] + C]
    big = exact and r["proq"] in (SI, GE)       # (the SiLU / GELU lattice keeps |u| >= 112: no channel scaling of Q there)
    Q = c.t("q", (B, C, H, W), fill((B, C, H, W), r["proq"]) * (1.0 if big else qs.view(1, C, 1, 1)))
    bp = (lattice_bnv(c, "bnvp", M, r["prop"]) if exact else c.bnv("bnvp", M)) if r["prop"] else None
    bq = (lattice_bnv(c, "bnvq", C, r["proq"]) if exact else c.bnv("bnvq", C)) if r["proq"] else None
    if r["proq"] and not big:
        c.items["bnvq"][1][1] *= qs
    mk_gate = lambda n: pick(g, (B, n), [0.5, 1.0, 2.0, 0.25]) if exact else torch.rand(B, n, generator=g)       # noqa: E731
    gq = c.t("gateq", (B, C), mk_gate(C)) if r["gateq"] else None
    gp = c.t("gatep", (B, M), mk_gate(M)) if r["gatep"] else None
    # (the lattice WGS: integers in the unit of the products or coarser - 16 per side with a SiLU / GELU prologue -, in the column's scale)
    if data == "random" and not r["split"]:
        settle(c, "p", "bnvp" if r["prop"] else None, "gatep" if r["gatep"] else None, r["prop"], M)
        settle(c, "q", "bnvq" if r["proq"] else None, "gateq" if r["gateq"] else None, r["proq"], C, qs.view(1, C, 1, 1))
    old = ints(g, (T, M, CT), -8, 8) * (16.0 if r["prop"] in (SI, GE) else 1.0) * (16.0 if big else 1.0) if exact else torch.randn(T, M, CT, generator=g)
    wgs = c.t("wgs", (T, M, CT), old * (1.0 if big else cols.view(1, 1, CT)))      # (WGS non-zero before the stage: it accumulates)
    fields = dict(P=P, BNVP=bp, GATEP=gp, Q=Q, BNVQ=bq, GATEQ=gq, WGS=wgs.at(r["coff"]), B=B, M=M, C=C, CTOT=CT, H=H, W=W, KH=k, KW=k, STRIDE=r["s"],
                  PAD_T=pad, PAD_L=pad, HO=Ho, WO=Wo, PROP=r["prop"], PROQ=r["proq"], MODE=D.MODE_CONV, P_BF16=int(r["p16"]),
                  _flags=D.FLAG_SPLIT if r["split"] else D.FLAG_BF16)
    return c, ["wgs"], [], fields


def build(r, data="random"):
    return build_conv(r, data) if r["kind"] == "CONV" else build_wgrad(r, data)


def bars(r, family):
    """the bar of a row by the family that runs it (module docstring)"""
    if r["kind"] == "CONV":
        if family == 2:
            return 1e-3 if (r["pro"] or r["pro2"]) else 1e-4
        return 1e-4
    return {2: 1e-3, 5: 2e-4}.get(family, 2e-4)


def program(pre, kind, fields, flags=None):
    prog = Program()
    for k, f in pre:
        prog.add(k, **f)
    f = dict(fields)
    if flags is not None:
        f["_flags"] = flags
        f.pop("WTB", None)
    prog.add(kind, **f)
    return prog.pack()


def by_part(r, v):
    """a flat output as (rows, channels / columns): CONV's Y per channel, WGRAD's WGS per column"""
    if r["kind"] == "CONV":
        n = v.shape[1]
        return v.reshape(v.shape[0], n, -1).transpose(0, 1).reshape(n, -1).t()
    return v.reshape(-1, v.shape[-1])


def rel(a, b):
    """(whole-tensor, worst per-part) error of a against b, relative to max |b| / the part's max |b|"""
    whole = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
    part = ((a - b).abs().amax(0) / b.abs().amax(0).clamp_min(1e-30)).max().item()
    return whole, part


def outside_unchanged(r, c, fields):
    """the parts of the output tensor the stage does not own, bit for bit (`untouched` takes the whole tensor as written)"""
    if r["kind"] == "CONV":
        M, YC = r["M"], fields["YC"]
        if r["mode"] == D.MODE_CONV and YC > M:
            sent, back = c.items["y"][1][:, M:].contiguous().view(torch.int32), c.read(c.got, "y")[:, M:].contiguous().view(torch.int32)
            assert torch.equal(sent, back), f"channels >= M of Y changed: {(sent != back).sum().item()} words"
    elif r["ct"] > r["C"]:
        keep = torch.ones(r["ct"], dtype=torch.bool)
        keep[r["coff"]:r["coff"] + r["C"]] = False
        sent, back = c.items["wgs"][1][..., keep].contiguous().view(torch.int32), c.read(c.got, "wgs")[..., keep].contiguous().view(torch.int32)
        assert torch.equal(sent, back), f"columns of WGS outside the stage's slice changed: {(sent != back).sum().item()} words"


def run_pass(r, data, family, tol):
    c, outs, pre, fields = build(r, data)
    kind = r["kind"]
    opts = dict(per_channel=("y",), per_column=("stats",) if r.get("stats") else (), sum0=("stats",)) if kind == "CONV" else dict(per_column=("wgs",))
    errs = c.run(kind, outs, tol, pre=pre, want_variant=family, ref64=True, untouched=True, **opts, **fields)
    outside_unchanged(r, c, fields)
    print(f"{rid(r)} [{data}] family {family}: " + ", ".join(f"{n} {e[0]:.2e} / f64 {e[1]:.2e} (per part {c.parts[n][0]:.2e} / {c.parts[n][1]:.2e})"
                                                          for n, e in errs.items()))
    return c, outs, pre, fields


def run_row(r):
    from s2lc_amd import _lib

    v = launch(r)
    kind = r["kind"]
    if v.result == "error":
        c, outs, pre, fields = build(r)
        with pytest.raises(_lib.S2kError, match=v.message.replace("(", r"\(").replace(")", r"\)").replace("*", r"\*")):
            c.run(kind, outs, 1.0, pre=pre, **fields)
        return
    if v.result == "declined" and r["raises"]:       # the f32 launcher's own refusal
        c, outs, pre, fields = build(r)
        with pytest.raises(_lib.S2kError, match=r["raises"]):
            c.run(kind, outs, 1.0, pre=pre, **fields)
        return
    if v.result == "declined":
        # the f32 kernels take the stage: held to their bar against the oracles of the record WITHOUT the flag (no operand is rounded)
        c, outs, pre, fields = build(r)
        c.oracle_packed = program(pre, kind, fields, flags=0)
        opts = dict(per_channel=("y",), per_column=("stats",) if r.get("stats") else (), sum0=("stats",)) if kind == "CONV" else dict(per_column=("wgs",))
        c.run(kind, outs, bars(r, 0), pre=pre, want_variant=f32_family(r), ref64=True, untouched=True, **opts, **fields)
        fam = int(_lib.profile_variants(program(pre, kind, fields), _lib.Bases().set("WS", c.image().cuda()), torch.cuda.current_stream().cuda_stream)[1][-1])
        assert fam not in (2, 5), f"a declined stage ran on kernel family {fam}"
        outside_unchanged(r, c, fields)
        return
    family = v.result
    tol = bars(r, family)
    c, outs, pre, fields = run_pass(r, "spread" if r["spread"] else "random", family, tol)
    if family == 5:
        # against float64 (the unrounded emulation: FLAG_SPLIT is exact f32 to the oracle) at most 2 x the exact-f32 kernel's error on
        # the same bytes + 2^-22, for the whole tensor and for every channel / column
        if not f32_has(r):       # no exact-f32 kernel has this prologue pair (csrc/wgrad.hip launch_wg): the first two parts of the scheme only
            with pytest.raises(_lib.S2kError, match="prologue combination"):
                c.execute(program(pre, kind, fields, flags=0), oracle=False)
            return
        got32, _, _ = c.execute(program(pre, kind, fields, flags=0), oracle=False)
        out = outs[0]
        r64 = c.read(c.wide, out, wide=True).double()
        s, f = by_part(r, c.read(c.got, out).double()), by_part(r, c.read(got32, out).double())
        assert torch.isfinite(f).all(), "the f32 kernels produced non-finite values"
        t = by_part(r, r64)
        (es, esp), (ef, efp) = rel(s, t), rel(f, t)
        print(f"{rid(r)}: error vs float64: split {es:.3e} (per part {esp:.3e}), f32 kernel {ef:.3e} (per part {efp:.3e})")
        assert es <= 2 * ef + FLOOR, f"split error {es:.3e} > 2 x the f32 kernel's {ef:.3e} (+ {FLOOR:.1e})"
        # ... and per channel / column: every part's split error, relative to that part's max |ref|, against the f32 kernel's worst
        # part.  (Not against the f32 kernel's error in the SAME part: that is the maximum of a rounding random walk over as few as
        # T x M = 32 values - a draw, not a bound; the parts of a row share one reduction length and one distribution up to the exact
        # scaling 2^-(c mod 8), so the f32 kernel's accuracy per part is what it reaches over all of them.)
        scale = t.abs().amax(0).clamp_min(1e-30)
        ps = (s - t).abs().amax(0) / scale
        bad = torch.nonzero(ps > 2 * efp + FLOOR).reshape(-1)
        assert not bad.numel(), f"part {int(bad[0])}: split error {ps[bad[0]]:.3e} > 2 x the f32 kernel's worst part {efp:.3e} (+ {FLOOR:.1e})"
        return
    # family 2 on the lattice: every product and partial sum exact, at most three epilogue roundings
    c, outs, pre, fields = run_pass(r, "exact", family, tol)
    out = outs[0]
    a, t = by_part(r, c.read(c.got, out).double()), by_part(r, c.read(c.wide, out, wide=True).double())
    whole, part = rel(a, t)
    print(f"{rid(r)} [exact]: {whole:.3e} of max |ref|, worst channel / column {part:.3e}")
    if kind == "WGRAD":
        assert torch.equal(a, t), f"WGS on the lattice is not bit-equal to the float64 reference: {(a != t).sum().item()} elements, worst column {part:.3e}"
    assert part <= EXACT_TOL, f"lattice data: channel / column error {part:.3e} of its max |ref| against the float64 reference (bar {EXACT_TOL:.0e})"


# ---------------------------------------------------------------------------------------------------------------------------------
# tables.  The 1x1 CONV geometries depend on the tile counts (n128 = cdiv(B H W, 128), mt = cdiv(M, 128)): thin 32 x 256 tiles for
# M <= 32; 64 x 64 tiles while n128 * mt < 200; else 128 x 128 (M padded by <= 12 %) or 64 x 128; 128-channel (split: 64) chunks for
# Ctot >= 512 while n128 * mt <= 1024.  The smallest maps that reach the large tiles: 2 x 80 x 80 with M = 240 / 136 (exactly 200 tiles),
# 3 x 66 x 66 (x16: 3 x 72 x 72) for a ragged last tile and tiles over two images, 800 x 4 x 4 for tiles over eight.
# ---------------------------------------------------------------------------------------------------------------------------------
_EPI = [dict(stats=True), dict(bias=True, stats=True), dict(beta=1, res=True, yc=8), dict(bias=True, stats=True, res=True), dict(stats=True, beta=1),
        dict(bias=True, yc=8)]        # (yc: channels added to M)
_THIN = [(2, 12, 12, 24), (40, 4, 4, 32), (3, 16, 16, 8)]
_S64 = [(2, 16, 16, 40), (9, 4, 4, 65), (2, 16, 16, 144)]
_B128 = [(2, 80, 80, 240), (3, 66, 66, 240), (800, 4, 4, 240)]
_M64 = [(2, 80, 80, 136), (3, 66, 66, 129), (800, 4, 4, 136)]


def _conv_1x1(split):
    rows, i = [], 0
    k1 = BD.K1[split]
    shallow = [k1 - 8, k1 + 8, 2 * k1 + 6, k1]                     # K < one chunk; K tail; Ctot % 8 != 0; whole chunks
    # deep reductions (Ctot >= 512: 128-channel chunks, split 64): 576 and 517 end in the lower half of a 128-channel chunk (the upper
    # half lies past the packed K; 517 also has Ctot % 8 != 0), 600 ends in the upper half, 1056 has a ragged packed K
    deep = [576, 517, 600, 1056] if not split else [576, 517, 600]
    sites = [(NO, False, False), (RE, False, False), (SI, False, False), (AF, False, False), (SI, True, False)] + ([] if split else [(NO, False, True)])
    # one row per launch site x tile geometry; the shape, the channel count and the epilogue terms cycle through their lists, so that
    # every edge meets several sites (tests/test_b16_dispatch_cpu.py checks which: REQUIRED, test_combined_edges)
    for pro, gate, x16 in sites:
        forms = [((_THIN, _S64, _B128, _M64), shallow)]
        if pro == NO or gate:               # the sites with a deep form (the thin tile has none: deep needs M > 32)
            forms.append(((_S64, _B128, _M64), deep))
        for geoms, depth in forms:
            for gi, geom in enumerate(geoms):
                B, H, W, M = geom[i % 3]
                if x16 and H * W % 8:
                    H = W = 72
                C = depth[(i + gi) % len(depth)]
                if depth is deep and B * H * W > 2048:
                    C = depth[i % 2]                                # (the 1.8 G multiply-add rows: Ctot 576 and 517 only)
                epi = dict(_EPI[i % len(_EPI)])
                if "yc" in epi:
                    epi["yc"] += M
                rows.append(R(B, C, H, W, M, pro=pro, gate=gate, x16=x16, split=split, spread=split and pro == NO and depth is shallow, seed=i, **epi))
                i += 1
    return rows


def _conv_3x3(split):
    rows, i = [], 0
    maps = {(2, 64): [(7, 64), (5, 128)], (4, 32): [(10, 32)], (8, 16): [(12, 16)], (2, 56): [(7, 56), (5, 112), (3, 224)], (4, 28): [(10, 28)], (8, 14): [(12, 14)]}
    chans = [(16, 0), (24, 0), (13, 0), (16, 13), (32, 24)]           # whole chunk; K tail; K < one chunk, Ctot % 8 != 0; concat with the tail in source 2
    for (rr, xw), hw in maps.items():
        for pro, x16 in [(NO, False), (RE, False)] + ([] if split else [(NO, True)]):
            for M in (240, 72 if i % 2 else 129):
                H, W = hw[i % len(hw)]
                C1, C2 = chans[i % len(chans)] if not x16 else (chans[i % 3][0], 0)
                epi = dict(_EPI[i % len(_EPI)])
                if "yc" in epi:
                    epi["yc"] += M
                rows.append(R(2, C1, H, W, M, C2=C2, k=3, pro=pro, x16=x16, split=split, spread=split and pro == NO and C2 == 0, seed=i, **epi))
                i += 1
    # thin: M <= 32 on maps a multiple of 64 wide (R 4: H = 6 leaves a partial last tile row)
    rows.append(R(2, 16, 6, 64, 32, C2=13, k=3, bias=True, stats=True, split=split, spread=split, seed=i))                # concat with the raw 13-band input: the K tail in source 2
    rows.append(R(2, 24, 6, 128, 24, k=3, pro=RE, bias=True, stats=True, split=split, seed=i + 1))            # two x tiles per row; M = 24 of 32 rows
    if not split:
        rows.append(R(2, 16, 6, 64, 32, k=3, x16=True, beta=1, split=split, seed=i + 2))
    return rows


def _conv_edges(split):
    """rows for the edges the products above do not meet"""
    f = dict(split=split)
    rows = [
        # split-K (SCRATCH, <= 512 blocks, >= 8 chunks), the tail applying bias, statistics, accumulate and residual
        R(2, 1056, 16, 16, 40, pro=SI, gate=True, bias=True, stats=True, beta=1, res=True, scratch=True, **f),      # bf16: 9 chunks of 128 = 5 + 4 under the nchunks / 4 cap; split: 17 of 64 -> 4 splits of 5, 5, 5, 2
        R(2, 1056, 16, 16, 40, pro=SI, gate=True, bias=True, stats=True, beta=1, res=True, **f),                    # the same record without SCRATCH must not split
        R(2, 2048, 8, 8, 48, pro=NO if split else RE, bias=True, stats=True, beta=1, res=True, scratch=True, **f),   # 32 chunks of 64 over 2 tiles: 8 splits of 4
        R(2, 576, 16, 16, 144, bias=True, stats=True, scratch=True, yc=150, **f),                                      # few chunks (bf16: 5 < 8): SCRATCH given, no split (split mode: 9 chunks, 2 splits)
        R(40, 520, 16, 16, 136, pro=RE, stats=True, scratch=True, **f),                                                # 480 blocks of 64 x 64: 2 splits asked (bf16: 9 chunks = 5 + 4; split: 17 = 9 + 8), no cap binds
        R(2, 200, 16, 16, 144, bias=True, stats=True, scratch=True, **f),                                              # 4 / 7 chunks: SCRATCH given, no split in either mode
        # statistics at each reduction width with one replica (NREP 1) - the products above use several
        R(3, 16, 16, 16, 24, stats=True, nrep=1, **f), R(2, 24, 16, 16, 40, pro=AF, stats=True, nrep=1, **f), R(2, 16, 80, 80, 240, stats=True, nrep=1, **f),
        R(2, 16, 12, 14, 72, k=3, pro=RE, stats=True, nrep=1, **f),                                                     # ... on the scalar store's LDS rows
        R(2, 16, 12, 14, 72, k=3, stats=True, beta=1, res=True, **f),                                                   # scalar store: statistics after residual + accumulate
        # a pixel tile over >= 3 images with the SE gate, on each pixel tile width
        R(40, 40, 4, 4, 24, pro=SI, gate=True, stats=True, **f), R(800, 24, 4, 4, 240, pro=SI, gate=True, bias=True, **f),
        # ConvTranspose2d(k2, s2): rows (co, dy, dx) scattered as 2 x 2 patches
        R(2, 24, 8, 8, 64, pro=RE, bias=True, mode=D.MODE_CONVT_SCATTER, **f), R(2, 70, 6, 10, 240, pro=RE, bias=True, mode=D.MODE_CONVT_SCATTER, **f),
        R(3, 40, 8, 8, 72, pro=SI, bias=True, mode=D.MODE_CONVT_SCATTER, **f), R(2, 24, 4, 6, 232, pro=SI, mode=D.MODE_CONVT_SCATTER, **f),
    ]
    return rows


CONV_BF16 = _conv_1x1(False) + _conv_3x3(False) + _conv_edges(False)
CONV_SPLIT = _conv_1x1(True) + _conv_3x3(True) + _conv_edges(True)


def _wgrad_rows(split):
    f = dict(split=split)
    p16s = (False,) if split else (False, True)
    rows, i = [], 0
    # 1x1: tile edges by side length (32 | 33 64 65 114 | 115 129(64) 229), all five prologues on P and on Q
    sides = [(32, 5, 70, 2, 4), (24, 33, 3, 16, 16), (32, 115, 2, 16, 20), (33, 32, 9, 8, 8), (229, 24, 4, 16, 16), (115, 229, 2, 16, 24), (229, 65, 5, 8, 16),
             (114, 115, 4, 12, 12), (64, 129, 70, 2, 4), (65, 64, 3, 16, 16)]
    pros = [(NO, NO), (NO, SI), (RE, NO), (NO, RE), (SI, AF), (AF, GE), (GE, SI), (NO, AF), (NO, GE), (SI, RE)]
    if split:       # (a prologue on one side at most wherever it can be: the exact-f32 kernels of the comparison have no other form - f32_has)
        pros = [(NO, NO), (NO, SI), (RE, NO), (NO, RE), (SI, NO), (GE, NO), (NO, GE), (AF, NO), (NO, AF), (NO, SI)]
    for p16 in p16s:
        for (M, C, B, H, W), (pp, pq) in zip(sides, pros):
            gate = pq == SI or (i % 4 == 0)
            rows.append(RW(B, M, C, H, W, prop=NO if p16 else pp, proq=pq, gateq=gate, p16=p16, spread=split and pp == NO and pq == NO, seed=i, **f))
            i += 1
    # 3x3 (Q prologue NONE / ReLU only meets the zero padding after the activation; P has none)
    if split:
        shapes = [(24, 13, 2, 6, 64), (32, 40, 2, 6, 64), (72, 32, 1, 5, 128), (72, 40, 2, 6, 64), (129, 229, 1, 5, 128), (40, 72, 2, 10, 32), (72, 40, 3, 10, 16)]
    else:
        shapes = [(24, 13, 2, 6, 64), (32, 40, 2, 6, 64), (72, 32, 1, 5, 128), (72, 40, 2, 6, 64), (129, 229, 1, 5, 128), (40, 72, 2, 5, 112), (72, 40, 2, 7, 56),
                  (40, 72, 2, 10, 32), (72, 40, 3, 10, 16)]
    for p16 in p16s:
        for j, (M, C, B, H, W) in enumerate(shapes):
            sl = dict(ct=C + 24, coff=16) if j % 3 == 1 else {}
            rows.append(RW(B, M, C, H, W, k=3, proq=((NO, RE, RE, AF)[j % 4] if not split else (NO, RE, RE, NO, RE, AF, RE)[j]), p16=p16, spread=split and j == 0, seed=i, **sl, **f))
            i += 1
    # one split / several / a shorter last one; >= 3 images per 256-pixel tile with a ragged last tile
    rows += [RW(4, 24, 16, 8, 16, proq=RE, **f), RW(33, 40, 48, 8, 8, proq=SI, gateq=True, **f), RW(2, 40, 48, 16, 64, k=3, proq=RE, **f)]
    return rows


WGRAD_BF16 = _wgrad_rows(False)
WGRAD_SPLIT = _wgrad_rows(True)

# records the launchers must decline (bf16-mixed: the f32 kernels take the stage) or refuse (f32-split, X1_BF16, P_BF16: S2kError)
_DECL_CONV = [
    dict(B=2, C1=16, H=16, W=16, M=64, k=3, s=2, stats=True),         # stride 2
    dict(B=2, C1=24, H=7, W=7, M=48, bias=True),                      # HW % 4 != 0
    dict(B=2, C1=24, H=8, W=8, M=48, C2=8, stats=True),               # 1x1 with a concat
    dict(B=2, C1=24, H=8, W=8, M=48, gate=True, pro=RE),              # gate without SiLU
    dict(B=2, C1=16, H=8, W=48, M=64, k=3, stats=True),               # WO = 48
    dict(B=2, C1=24, H=8, W=64, M=64, C2=8, k=3),                     # concat with C1 % 16 != 0
    dict(B=2, C1=16, H=8, W=64, M=64, C2=16, k=3, pro=RE, pro2=NO),   # concat with pro2 != pro1
    dict(B=2, C1=16, H=8, W=32, M=24, k=3, bias=True),                # thin 3x3 with WO % 64 != 0
]
_DECL_WGRAD = [
    dict(B=1, M=40, C=48, H=16, W=16),                                # B * HW < 512
    dict(B=12, M=40, C=48, H=6, W=10),                                # HW % 8 != 0
    dict(B=2, M=40, C=48, H=8, W=64, k=3, prop=RE, raises="prologue combination"),              # 3x3 with a prologue on P: declined, and no f32 kernel has such a form either (the
                                                                                                 # producer / consumer launcher used to run it WITHOUT the prologue: csrc/wgrad_pc.hip)
    dict(B=2, M=40, C=48, H=8, W=64, k=3, gateq=True, raises="SE gate is only supported"),       # 3x3 with a gate on Q: likewise
    dict(B=4, M=40, C=48, H=10, W=28, k=3, proq=RE),                  # WO = 28
    dict(B=8, M=40, C=48, H=14, W=14, k=3),                           # WO = 14
]
DECLINED = ([R(**d) for d in _DECL_CONV] + [R(**d, split=True) for d in _DECL_CONV[:3]] + [RW(**d) for d in _DECL_WGRAD] +
            [RW(**d, split=True) for d in _DECL_WGRAD[:2]] + [
    R(2, 24, 8, 8, 48, x16=True, pro=RE),                             # X1_BF16 with a prologue
    R(2, 24, 8, 8, 48, x16=True, pro=SI, gate=True),                  # ... with the gated SiLU prologue (which has a kernel of its own)
    R(2, 24, 6, 6, 48, x16=True),                                     # X1_BF16 with HW % 8 != 0
    RW(4, 40, 48, 16, 16, prop=RE, p16=True),                         # P_BF16 with a prologue on P
])
# ---------------------------------------------------------------------------------------------------------------------------------
# every distinct (instantiation, edges) among the FLAG_BF16 / FLAG_SPLIT CONV and WGRAD records of the production plans - the b5 U-Net
# at 13 x 256 x 256 bs 32, the Prithvi-100M MAE step at bs 64 and the segmentation steps at bs 16 (frozen and unfrozen backbone), built
# with precision "bf16-mixed" and "f32-split" - at the plan's own map size, B and the channel counts cut down as far as both stay the
# same (comments: the template arguments, multiply-adds)
# ---------------------------------------------------------------------------------------------------------------------------------
PROD = [
    R(32, 512, 1, 56, 1920, bias=True, scratch=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 1.76 GMAC
    R(32, 512, 1, 56, 1920, scratch=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 1.76 GMAC
    R(8, 512, 1, 56, 64, bias=True, res=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, False, False) 0.01 GMAC
    R(8, 512, 1, 56, 64, bias=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, False, False) 0.01 GMAC
    R(8, 512, 1, 56, 64, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, False, False) 0.01 GMAC
    R(18, 512, 8, 8, 2944, stats=True, scratch=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 1.74 GMAC
    R(18, 512, 8, 8, 2944, x16=True, scratch=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, True, False) 1.74 GMAC
    R(1, 1032, 8, 8, 72, pro=2, gate=True, stats=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 2, True, False, False, False) 0.00 GMAC
    R(1, 72, 8, 8, 33, x16=True, scratch=True, prod=True),   # (0, 2, 1, 1, 64, 1, 64, 0, False, False, True, False) 0.00 GMAC
    R(1, 904, 8, 8, 128, pro=2, gate=True, stats=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 2, True, False, False, False) 0.01 GMAC
    R(1, 904, 8, 8, 33, x16=True, beta=1, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, True, False) 0.00 GMAC
    R(1, 904, 8, 8, 33, x16=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, True, False) 0.00 GMAC
    R(1, 904, 8, 8, 72, pro=2, gate=True, stats=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 2, True, False, False, False) 0.00 GMAC
    R(22, 3072, 8, 8, 512, pro=2, gate=True, stats=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 2, True, False, False, False) 2.21 GMAC
    R(22, 3072, 8, 8, 512, x16=True, beta=1, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, True, False) 2.21 GMAC
    R(26, 512, 8, 8, 2048, stats=True, scratch=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 1.74 GMAC
    R(28, 512, 8, 8, 1800, x16=True, scratch=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, True, False) 1.65 GMAC
    R(28, 72, 8, 8, 1800, stats=True, scratch=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.23 GMAC
    R(28, 72, 8, 8, 1800, x16=True, scratch=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, True, False) 0.23 GMAC
    R(2, 64, 8, 8, 128, pro=2, bias=True, mode=1, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 2, False, True, False, False) 0.00 GMAC
    R(32, 2048, 8, 8, 2048, scratch=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 8.59 GMAC
    R(32, 2048, 8, 8, 512, x16=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, True, False) 2.15 GMAC
    R(16, 512, 14, 14, 64, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, False, False) 0.10 GMAC
    R(16, 512, 1, 196, 64, bias=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, False, False) 0.10 GMAC
    R(64, 512, 1, 196, 384, bias=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 2.47 GMAC
    R(16, 512, 1, 200, 1024, bias=True, scratch=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 1.68 GMAC
    R(32, 1024, 1, 200, 512, bias=True, res=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 3.36 GMAC
    R(32, 1024, 1, 200, 512, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 3.36 GMAC
    R(32, 512, 1, 200, 512, bias=True, res=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 1.68 GMAC
    R(32, 512, 1, 200, 512, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 1.68 GMAC
    R(48, 64, 1, 200, 384, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.24 GMAC
    R(64, 64, 1, 200, 256, bias=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.21 GMAC
    R(8, 512, 1, 200, 64, bias=True, res=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, False, False) 0.05 GMAC
    R(8, 512, 1, 200, 64, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, False, False) 0.05 GMAC
    R(12, 72, 16, 16, 1032, stats=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.23 GMAC
    R(12, 72, 16, 16, 1032, x16=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, True, False) 0.23 GMAC
    R(17, 64, 16, 16, 768, stats=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.21 GMAC
    R(17, 64, 16, 16, 768, x16=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, True, False) 0.21 GMAC
    R(17, 72, 16, 16, 768, x16=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, True, False) 0.24 GMAC
    R(1, 1032, 16, 16, 33, pro=2, gate=True, stats=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 2, True, False, False, False) 0.01 GMAC
    R(1, 1032, 16, 16, 33, x16=True, beta=1, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, True, False) 0.01 GMAC
    R(1, 1032, 16, 16, 33, x16=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, True, False) 0.01 GMAC
    R(1, 512, 16, 16, 33, pro=2, gate=True, stats=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 2, True, False, False, False) 0.00 GMAC
    R(1, 512, 16, 16, 64, pro=2, gate=True, stats=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 2, True, False, False, False) 0.01 GMAC
    R(1, 512, 16, 16, 64, x16=True, beta=1, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, True, False) 0.01 GMAC
    R(1, 512, 16, 16, 64, x16=True, scratch=True, prod=True),   # (0, 2, 1, 1, 128, 1, 64, 0, False, False, True, False) 0.01 GMAC
    R(1, 64, 16, 16, 128, pro=3, bias=True, mode=1, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 3, False, True, False, False) 0.00 GMAC
    R(1, 64, 16, 16, 64, pro=2, gate=True, stats=True, scratch=True, prod=True),   # (0, 2, 1, 1, 64, 1, 64, 2, True, False, False, False) 0.00 GMAC
    R(1, 64, 16, 16, 64, x16=True, prod=True),   # (0, 2, 1, 1, 64, 1, 64, 0, False, False, True, False) 0.00 GMAC
    R(25, 1024, 16, 16, 512, scratch=True, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 3.36 GMAC
    R(16, 512, 28, 28, 384, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 2.47 GMAC
    R(13, 512, 32, 32, 256, prod=True),   # (0, 2, 2, 2, 128, 1, 64, 0, False, False, False, False) 1.74 GMAC
    R(13, 64, 32, 32, 232, x16=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, True, False) 0.20 GMAC
    R(1, 64, 32, 32, 128, pro=3, bias=True, mode=1, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 3, False, True, False, False) 0.01 GMAC
    R(25, 64, 32, 32, 64, pro=2, gate=True, stats=True, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 2, True, False, False, False) 0.10 GMAC
    R(25, 64, 32, 32, 64, x16=True, beta=1, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 0, False, False, True, False) 0.10 GMAC
    R(25, 64, 32, 32, 64, x16=True, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 0, False, False, True, False) 0.10 GMAC
    R(25, 72, 32, 32, 64, pro=2, gate=True, stats=True, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 2, True, False, False, False) 0.12 GMAC
    R(9, 64, 32, 32, 384, stats=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.23 GMAC
    R(9, 64, 32, 32, 384, x16=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, True, False) 0.23 GMAC
    R(8, 64, 56, 56, 256, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.41 GMAC
    R(1, 64, 64, 64, 128, pro=3, bias=True, mode=1, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 3, False, True, False, False) 0.03 GMAC
    R(4, 8, 64, 64, 136, x16=True, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 0, False, False, True, False) 0.02 GMAC
    R(4, 8, 64, 64, 232, stats=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.03 GMAC
    R(4, 8, 64, 64, 232, x16=True, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, True, False) 0.03 GMAC
    R(7, 64, 64, 64, 128, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.23 GMAC
    R(7, 72, 64, 64, 33, pro=2, gate=True, stats=True, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 2, True, False, False, False) 0.07 GMAC
    R(7, 72, 64, 64, 33, x16=True, beta=1, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 0, False, False, True, False) 0.07 GMAC
    R(7, 72, 64, 64, 33, x16=True, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 0, False, False, True, False) 0.07 GMAC
    R(2, 64, 112, 112, 256, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.41 GMAC
    R(1, 64, 128, 128, 128, pro=3, bias=True, mode=1, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 3, False, True, False, False) 0.13 GMAC
    R(1, 72, 128, 128, 2, x16=True, prod=True),   # (0, 1, 1, 2, 64, 1, 64, 0, False, False, True, False) 0.00 GMAC
    R(1, 8, 128, 128, 136, stats=True, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 0, False, False, False, False) 0.02 GMAC
    R(1, 8, 128, 128, 2, pro=2, gate=True, stats=True, prod=True),   # (0, 1, 1, 2, 64, 1, 64, 2, True, False, False, False) 0.00 GMAC
    R(1, 8, 128, 128, 2, x16=True, prod=True),   # (0, 1, 1, 2, 64, 1, 64, 0, False, False, True, False) 0.00 GMAC
    R(2, 64, 128, 128, 64, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 0, False, False, False, False) 0.13 GMAC
    R(2, 69, 128, 128, 33, stats=True, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 0, False, False, False, False) 0.07 GMAC
    R(2, 8, 128, 128, 33, x16=True, prod=True),   # (0, 2, 1, 2, 64, 1, 64, 0, False, False, True, False) 0.01 GMAC
    R(1, 1, 224, 224, 128, prod=True),   # (0, 2, 2, 2, 64, 1, 64, 0, False, False, False, False) 0.01 GMAC
    R(1, 1, 256, 256, 32, prod=True),   # (0, 1, 1, 2, 64, 1, 64, 0, False, False, False, False) 0.00 GMAC
    R(1, 8, 256, 256, 2, pro=3, bias=True, prod=True),   # (0, 1, 1, 2, 64, 1, 64, 3, False, False, False, False) 0.00 GMAC
    R(1, 16, 16, 16, 128, C2=16, k=3, bias=True, stats=True, prod=True),   # (1, 2, 2, 2, 16, 8, 16, 0, False, False, False, False) 0.01 GMAC
    R(1, 16, 16, 16, 128, k=3, pro=3, bias=True, stats=True, prod=True),   # (1, 2, 2, 2, 16, 8, 16, 3, False, False, False, False) 0.00 GMAC
    R(1, 16, 16, 16, 128, k=3, x16=True, prod=True),   # (1, 2, 2, 2, 16, 8, 16, 0, False, False, True, False) 0.00 GMAC
    R(1, 16, 32, 32, 128, C2=16, k=3, bias=True, stats=True, prod=True),   # (1, 2, 2, 2, 16, 4, 32, 0, False, False, False, False) 0.04 GMAC
    R(1, 16, 32, 32, 128, k=3, pro=3, bias=True, stats=True, prod=True),   # (1, 2, 2, 2, 16, 4, 32, 3, False, False, False, False) 0.02 GMAC
    R(1, 16, 32, 32, 128, k=3, x16=True, prod=True),   # (1, 2, 2, 2, 16, 4, 32, 0, False, False, True, False) 0.02 GMAC
    R(1, 16, 32, 32, 64, k=3, x16=True, prod=True),   # (1, 2, 1, 2, 16, 4, 32, 0, False, False, True, False) 0.01 GMAC
    R(1, 16, 64, 64, 128, C2=8, k=3, bias=True, stats=True, prod=True),   # (1, 2, 2, 2, 16, 2, 64, 0, False, False, False, False) 0.11 GMAC
    R(1, 16, 64, 64, 128, k=3, pro=3, bias=True, stats=True, prod=True),   # (1, 2, 2, 2, 16, 2, 64, 3, False, False, False, False) 0.08 GMAC
    R(1, 16, 64, 64, 128, k=3, x16=True, prod=True),   # (1, 2, 2, 2, 16, 2, 64, 0, False, False, True, False) 0.08 GMAC
    R(1, 16, 64, 64, 33, k=3, x16=True, prod=True),   # (1, 2, 1, 2, 16, 2, 64, 0, False, False, True, False) 0.02 GMAC
    R(1, 16, 128, 128, 64, C2=8, k=3, bias=True, stats=True, prod=True),   # (1, 2, 1, 2, 16, 2, 64, 0, False, False, False, False) 0.23 GMAC
    R(1, 16, 128, 128, 2, k=3, x16=True, prod=True),   # (1, 1, 1, 2, 16, 4, 64, 0, False, False, True, False) 0.00 GMAC
    R(1, 16, 128, 128, 64, k=3, pro=3, bias=True, stats=True, prod=True),   # (1, 2, 1, 2, 16, 2, 64, 3, False, False, False, False) 0.15 GMAC
    R(1, 16, 128, 128, 64, k=3, x16=True, prod=True),   # (1, 2, 1, 2, 16, 2, 64, 0, False, False, True, False) 0.15 GMAC
    R(1, 16, 224, 224, 128, k=3, bias=True, stats=True, prod=True),   # (1, 2, 2, 2, 16, 2, 56, 0, False, False, False, False) 0.92 GMAC
    R(1, 16, 224, 224, 128, k=3, x16=True, prod=True),   # (1, 2, 2, 2, 16, 2, 56, 0, False, False, True, False) 0.92 GMAC
    R(1, 16, 256, 256, 32, C2=1, k=3, bias=True, stats=True, prod=True),   # (1, 1, 1, 2, 16, 4, 64, 0, False, False, False, False) 0.32 GMAC
    R(1, 16, 256, 256, 32, k=3, pro=3, bias=True, stats=True, prod=True),   # (1, 1, 1, 2, 16, 4, 64, 3, False, False, False, False) 0.30 GMAC
    R(1, 16, 256, 256, 32, k=3, x16=True, prod=True),   # (1, 1, 1, 2, 16, 4, 64, 0, False, False, True, False) 0.30 GMAC
    R(2, 32, 8, 8, 128, pro=2, bias=True, mode=1, split=True, prod=True),   # (0, 2, 2, 2, 32, 1, 64, 2, False, True, False, True) 0.00 GMAC
    R(1, 32, 16, 16, 128, pro=3, bias=True, mode=1, split=True, prod=True),   # (0, 2, 2, 2, 32, 1, 64, 3, False, True, False, True) 0.00 GMAC
    R(1, 32, 32, 32, 128, pro=3, bias=True, mode=1, split=True, prod=True),   # (0, 2, 2, 2, 32, 1, 64, 3, False, True, False, True) 0.00 GMAC
    R(1, 32, 64, 64, 128, pro=3, bias=True, mode=1, split=True, prod=True),   # (0, 2, 2, 2, 32, 1, 64, 3, False, True, False, True) 0.02 GMAC
    R(1, 32, 128, 128, 128, pro=3, bias=True, mode=1, split=True, prod=True),   # (0, 2, 2, 2, 32, 1, 64, 3, False, True, False, True) 0.07 GMAC
    R(1, 16, 16, 16, 128, C2=16, k=3, bias=True, stats=True, split=True, prod=True),   # (1, 2, 2, 2, 16, 8, 16, 0, False, False, False, True) 0.01 GMAC
    R(1, 16, 16, 16, 128, k=3, pro=3, bias=True, stats=True, split=True, prod=True),   # (1, 2, 2, 2, 16, 8, 16, 3, False, False, False, True) 0.00 GMAC
    R(1, 16, 16, 16, 128, k=3, split=True, prod=True),   # (1, 2, 2, 2, 16, 8, 16, 0, False, False, False, True) 0.00 GMAC
    R(1, 16, 32, 32, 128, C2=16, k=3, bias=True, stats=True, split=True, prod=True),   # (1, 2, 2, 2, 16, 4, 32, 0, False, False, False, True) 0.04 GMAC
    R(1, 16, 32, 32, 128, k=3, pro=3, bias=True, stats=True, split=True, prod=True),   # (1, 2, 2, 2, 16, 4, 32, 3, False, False, False, True) 0.02 GMAC
    R(1, 16, 32, 32, 128, k=3, split=True, prod=True),   # (1, 2, 2, 2, 16, 4, 32, 0, False, False, False, True) 0.02 GMAC
    R(1, 16, 32, 32, 64, k=3, split=True, prod=True),   # (1, 2, 1, 2, 16, 4, 32, 0, False, False, False, True) 0.01 GMAC
    R(1, 16, 64, 64, 128, C2=8, k=3, bias=True, stats=True, split=True, prod=True),   # (1, 2, 2, 2, 16, 2, 64, 0, False, False, False, True) 0.11 GMAC
    R(1, 16, 64, 64, 128, k=3, pro=3, bias=True, stats=True, split=True, prod=True),   # (1, 2, 2, 2, 16, 2, 64, 3, False, False, False, True) 0.08 GMAC
    R(1, 16, 64, 64, 128, k=3, split=True, prod=True),   # (1, 2, 2, 2, 16, 2, 64, 0, False, False, False, True) 0.08 GMAC
    R(1, 16, 64, 64, 33, k=3, split=True, prod=True),   # (1, 2, 1, 2, 16, 2, 64, 0, False, False, False, True) 0.02 GMAC
    R(1, 16, 128, 128, 64, C2=8, k=3, bias=True, stats=True, split=True, prod=True),   # (1, 2, 1, 2, 16, 2, 64, 0, False, False, False, True) 0.23 GMAC
    R(1, 16, 128, 128, 2, k=3, split=True, prod=True),   # (1, 1, 1, 2, 16, 4, 64, 0, False, False, False, True) 0.00 GMAC
    R(1, 16, 128, 128, 64, k=3, pro=3, bias=True, stats=True, split=True, prod=True),   # (1, 2, 1, 2, 16, 2, 64, 3, False, False, False, True) 0.15 GMAC
    R(1, 16, 128, 128, 64, k=3, split=True, prod=True),   # (1, 2, 1, 2, 16, 2, 64, 0, False, False, False, True) 0.15 GMAC
    R(1, 16, 224, 224, 128, k=3, bias=True, stats=True, split=True, prod=True),   # (1, 2, 2, 2, 16, 2, 56, 0, False, False, False, True) 0.92 GMAC
    R(1, 16, 224, 224, 128, k=3, split=True, prod=True),   # (1, 2, 2, 2, 16, 2, 56, 0, False, False, False, True) 0.92 GMAC
    R(1, 16, 256, 256, 32, C2=1, k=3, bias=True, stats=True, split=True, prod=True),   # (1, 1, 1, 2, 16, 4, 64, 0, False, False, False, True) 0.32 GMAC
    R(1, 16, 256, 256, 32, k=3, pro=3, bias=True, stats=True, split=True, prod=True),   # (1, 1, 1, 2, 16, 4, 64, 3, False, False, False, True) 0.30 GMAC
    R(1, 16, 256, 256, 32, k=3, split=True, prod=True),   # (1, 1, 1, 2, 16, 4, 64, 0, False, False, False, True) 0.30 GMAC
    RW(16, 128, 128, 1, 56, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 0.01 GMAC
    RW(32, 128, 128, 1, 56, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 0.03 GMAC
    RW(8, 128, 120, 8, 8, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 2, 2, 1, 64, True, False) 0.01 GMAC
    RW(8, 128, 128, 8, 8, p16=True, prod=True),   # (0, 2, 2, 2, 2, 1, 64, True, False) 0.01 GMAC
    RW(8, 128, 128, 8, 8, prop=2, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 0.01 GMAC
    RW(8, 33, 120, 8, 8, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 1, 2, 1, 64, True, False) 0.00 GMAC
    RW(9, 120, 33, 8, 8, p16=True, prod=True),   # (0, 2, 2, 2, 1, 1, 64, True, False) 0.00 GMAC
    RW(9, 128, 128, 8, 8, p16=True, prod=True),   # (0, 2, 2, 2, 2, 1, 64, True, False) 0.01 GMAC
    RW(9, 128, 128, 8, 8, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 2, 2, 1, 64, True, False) 0.01 GMAC
    RW(9, 33, 120, 8, 8, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 1, 2, 1, 64, True, False) 0.00 GMAC
    RW(56, 512, 512, 1, 200, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 2.94 GMAC
    RW(8, 128, 128, 1, 200, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 0.03 GMAC
    RW(29, 136, 768, 16, 16, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 1, 2, 1, 64, True, False) 0.78 GMAC
    RW(2, 120, 33, 16, 16, p16=True, prod=True),   # (0, 2, 2, 2, 1, 1, 64, True, False) 0.00 GMAC
    RW(2, 128, 128, 16, 16, p16=True, prod=True),   # (0, 2, 2, 2, 2, 1, 64, True, False) 0.01 GMAC
    RW(2, 128, 128, 16, 16, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 2, 2, 1, 64, True, False) 0.01 GMAC
    RW(2, 128, 128, 16, 16, prop=3, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 0.01 GMAC
    RW(2, 33, 120, 16, 16, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 1, 2, 1, 64, True, False) 0.00 GMAC
    RW(4, 128, 128, 28, 28, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 0.05 GMAC
    RW(1, 128, 128, 32, 32, prop=3, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 0.02 GMAC
    RW(1, 128, 64, 32, 32, p16=True, prod=True),   # (0, 2, 2, 2, 1, 1, 64, True, False) 0.01 GMAC
    RW(1, 64, 120, 32, 32, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 1, 2, 1, 64, True, False) 0.01 GMAC
    RW(1, 64, 128, 32, 32, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 1, 2, 1, 64, True, False) 0.01 GMAC
    RW(1, 128, 128, 56, 56, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 0.05 GMAC
    RW(11, 33, 136, 64, 64, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 1, 1, 1, 64, True, False) 0.20 GMAC
    RW(1, 120, 33, 64, 64, p16=True, prod=True),   # (0, 2, 2, 2, 1, 1, 64, True, False) 0.02 GMAC
    RW(1, 128, 128, 64, 64, prop=3, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 0.07 GMAC
    RW(1, 33, 120, 64, 64, proq=2, gateq=True, p16=True, prod=True),   # (0, 2, 2, 1, 2, 1, 64, True, False) 0.02 GMAC
    RW(1, 128, 1408, 112, 112, prod=True),   # (0, 2, 2, 2, 2, 1, 64, False, False) 2.26 GMAC
    RW(1, 1, 33, 128, 128, proq=2, gateq=True, p16=True, prod=True),   # (0, 1, 2, 1, 1, 1, 128, True, False) 0.00 GMAC
    RW(1, 1, 8, 128, 128, proq=2, gateq=True, p16=True, prod=True),   # (0, 1, 1, 1, 1, 1, 256, True, False) 0.00 GMAC
    RW(1, 33, 117, 128, 128, p16=True, prod=True),   # (0, 2, 2, 1, 2, 1, 64, True, False) 0.06 GMAC
    RW(1, 64, 128, 128, 128, prop=3, prod=True),   # (0, 2, 2, 1, 2, 1, 64, False, False) 0.13 GMAC
    RW(6, 136, 8, 128, 128, p16=True, prod=True),   # (0, 2, 1, 1, 1, 1, 128, True, False) 0.11 GMAC
    RW(1, 1, 64, 224, 224, proq=3, gateq=True, prod=True),   # (0, 1, 2, 1, 1, 1, 128, False, False) 0.00 GMAC
    RW(1, 1, 32, 256, 256, proq=3, prod=True),   # (0, 1, 1, 1, 1, 1, 256, False, False) 0.00 GMAC
    RW(4, 64, 64, 16, 16, k=3, p16=True, ct=576, coff=16, prod=True),   # (1, 2, 2, 1, 1, 8, 16, True, False) 0.04 GMAC
    RW(4, 64, 64, 16, 16, k=3, proq=3, p16=True, prod=True),   # (1, 2, 2, 1, 1, 8, 16, True, False) 0.04 GMAC
    RW(1, 64, 64, 32, 32, k=3, p16=True, ct=320, coff=16, prod=True),   # (1, 2, 2, 1, 1, 4, 32, True, False) 0.04 GMAC
    RW(1, 64, 64, 32, 32, k=3, proq=3, p16=True, prod=True),   # (1, 2, 2, 1, 1, 4, 32, True, False) 0.04 GMAC
    RW(1, 64, 33, 64, 64, k=3, p16=True, ct=161, coff=16, prod=True),   # (1, 2, 2, 1, 1, 4, 64, True, False) 0.08 GMAC
    RW(1, 64, 64, 64, 64, k=3, p16=True, ct=104, coff=16, prod=True),   # (1, 2, 2, 1, 1, 4, 64, True, False) 0.15 GMAC
    RW(1, 64, 64, 64, 64, k=3, proq=3, p16=True, prod=True),   # (1, 2, 2, 1, 1, 4, 64, True, False) 0.15 GMAC
    RW(1, 64, 64, 128, 128, k=3, p16=True, ct=88, coff=16, prod=True),   # (1, 2, 2, 1, 1, 4, 64, True, False) 0.60 GMAC
    RW(1, 64, 64, 128, 128, k=3, proq=3, p16=True, prod=True),   # (1, 2, 2, 1, 1, 4, 64, True, False) 0.60 GMAC
    RW(1, 64, 8, 128, 128, k=3, p16=True, ct=72, coff=16, prod=True),   # (1, 2, 1, 1, 1, 4, 64, True, False) 0.08 GMAC
    RW(1, 64, 192, 224, 224, k=3, p16=True, prod=True),   # (1, 2, 2, 1, 1, 2, 56, True, False) 5.55 GMAC
    RW(1, 32, 32, 256, 256, k=3, p16=True, ct=45, prod=True),   # (1, 1, 1, 1, 1, 4, 64, True, False) 0.60 GMAC
    RW(1, 32, 32, 256, 256, k=3, proq=3, p16=True, prod=True),   # (1, 1, 1, 1, 1, 4, 64, True, False) 0.60 GMAC
    RW(1, 32, 8, 256, 256, k=3, p16=True, ct=40, coff=16, prod=True),   # (1, 1, 1, 1, 1, 4, 64, True, False) 0.15 GMAC
    RW(2, 64, 64, 16, 16, k=3, proq=3, split=True, prod=True),   # (1, 2, 2, 1, 1, 4, 16, False, True) 0.02 GMAC
    RW(2, 64, 64, 16, 16, k=3, ct=576, coff=16, split=True, prod=True),   # (1, 2, 2, 1, 1, 4, 16, False, True) 0.02 GMAC
    RW(1, 64, 64, 32, 32, k=3, proq=3, split=True, prod=True),   # (1, 2, 2, 1, 1, 2, 32, False, True) 0.04 GMAC
    RW(1, 64, 64, 32, 32, k=3, ct=320, coff=16, split=True, prod=True),   # (1, 2, 2, 1, 1, 2, 32, False, True) 0.04 GMAC
    RW(1, 64, 33, 64, 64, k=3, ct=161, coff=16, split=True, prod=True),   # (1, 2, 2, 1, 1, 2, 32, False, True) 0.08 GMAC
    RW(1, 64, 64, 64, 64, k=3, proq=3, split=True, prod=True),   # (1, 2, 2, 1, 1, 2, 32, False, True) 0.15 GMAC
    RW(1, 64, 64, 64, 64, k=3, ct=104, coff=16, split=True, prod=True),   # (1, 2, 2, 1, 1, 2, 32, False, True) 0.15 GMAC
    RW(1, 64, 64, 128, 128, k=3, proq=3, split=True, prod=True),   # (1, 2, 2, 1, 1, 2, 32, False, True) 0.60 GMAC
    RW(1, 64, 64, 128, 128, k=3, ct=88, coff=16, split=True, prod=True),   # (1, 2, 2, 1, 1, 2, 32, False, True) 0.60 GMAC
    RW(1, 64, 8, 128, 128, k=3, ct=72, coff=16, split=True, prod=True),   # (1, 2, 1, 1, 1, 2, 64, False, True) 0.08 GMAC
    RW(1, 32, 32, 256, 256, k=3, proq=3, split=True, prod=True),   # (1, 1, 1, 1, 1, 4, 64, False, True) 0.60 GMAC
    RW(1, 32, 32, 256, 256, k=3, ct=45, split=True, prod=True),   # (1, 1, 1, 1, 1, 4, 64, False, True) 0.60 GMAC
    RW(1, 32, 8, 256, 256, k=3, ct=40, coff=16, split=True, prod=True),   # (1, 1, 1, 1, 1, 4, 64, False, True) 0.15 GMAC
]
TABLES = {"CONV_BF16": CONV_BF16, "CONV_SPLIT": CONV_SPLIT, "WGRAD_BF16": WGRAD_BF16, "WGRAD_SPLIT": WGRAD_SPLIT, "DECLINED": DECLINED, "PROD": PROD}

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("r", CONV_BF16, ids=rid)
def test_conv_bf16_mixed(r):
    run_row(r)


@pytest.mark.parametrize("r", CONV_SPLIT, ids=rid)
def test_conv_f32_split(r):
    run_row(r)


@pytest.mark.parametrize("r", WGRAD_BF16, ids=rid)
def test_wgrad_bf16_mixed(r):
    run_row(r)


@pytest.mark.parametrize("r", WGRAD_SPLIT, ids=rid)
def test_wgrad_f32_split(r):
    run_row(r)


@pytest.mark.parametrize("r", DECLINED, ids=rid)
def test_declined_and_refused_records(r):
    run_row(r)


@pytest.mark.parametrize("r", PROD, ids=rid)
def test_production_records(r):
    run_row(r)
