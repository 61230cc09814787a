"""The f32 dense weight-gradient kernels, instantiation by instantiation: wgrad_kernel (csrc/wgrad.hip: 1x1 pixel mode, 3x3 spatial
mode, the ConvTranspose gather mode), wgrad_pc_kernel (csrc/wgrad_pc.hip) and wgrad_q4_kernel (csrc/wgrad_q4.hip), launched as one
WGRAD record through the C ABI.

One table per kernel and mode plus the records the launcher refuses and the production rows.  Which template instantiation a row
reaches, and which loop edges, is tests/wgrad_dispatch.py's restatement of launch_wgrad and its three launchers;
tests/test_wgrad_dispatch_cpu.py checks without a GPU that the tables reach every instantiation the launch sites can produce at
default tuning, every edge it lists per kernel, and the instantiation and edges of every WGRAD record of the production plans (rows
tagged PROD: the plan's own map size, B and channels cut down where the instantiation and the edges stay the same).  Here every row
is held

  * to the kernel family the launcher must take (want_variant);
  * to 2e-4 of max |ref| - the project's bar for the f32 weight gradients (tests/test_ops_gpu._wgrad_case) - for the whole of WGS and
    for every column on its own, against the f32 oracle (oracle/ops_ref.py) and against a float64 run of it; Q channel c, its
    BatchNorm shift and the old content of WGS are scaled by 2^-(c mod 8), an exact scaling, so a sum that lands in the wrong
    column, or an error in one column of a c-tile, shows against that column's own max |ref|;
  * rows marked by_row, in a second pass, to the same bar for every output row m: P channel m (and its BatchNorm shift where P
    has a prologue) is scaled by 2^-(m mod 8) instead - the P rows past M of a ragged m-tile are clamped loads (min(row, M - 1)),
    and a row computed from the wrong one would hide under the whole tensor's max;
  * WGS is non-zero before the stage (it accumulates), and every byte of the arena outside WGS must stay as uploaded; for CTOT > C
    the columns outside the stage's slice bit-identical.

The combine of the pixel splits is float atomics in no fixed order: repeats are not bit-identical and nothing here asks for it.
The one exception the project makes to the bar is the thin 1x1 kernel on >= 262144 pixels (256-pixel tiles): see TOL_NP256.

Row = R(B, M, C, H, W, family, options): see R below.  Each row prints its errors (whole / per column / per row, f32 oracle and
float64).

Rows: 257 (GENERIC_PIX 55, GENERIC_SPATIAL 23, GENERIC_GATHER 8, PC_SPATIAL 18, PC_PIX 22, QUAD 33, REFUSED 12, PROD 86 for the 296 WGRAD
records of the five production plans); they reach all 60 reachable instantiations of wgrad_kernel (parsed: 64), all 30 of
wgrad_pc_kernel and all 16 of wgrad_q4_kernel - the older rows of tests/test_ops_gpu.py reach 63 of these 106.
Worst on an MI355X (f32 oracle / float64): whole 1.2e-6 / 1.2e-6 (the MAE plan's 2304 x 768 Linear), per column 3.8e-6 / 4.3e-6,
per row 8.5e-7.  257 cases in 9 s; the slowest row (13 x 2 x 32 on 256 x 256, 109 MB of Q) 1.0 s."""
import re

import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd.plan import opdefs as D
from tests import wgrad_dispatch as WD
from tests.test_ops_gpu import Case
from tests.wgrad_dispatch import GENERIC, PC, Q4

TOL = 2e-4
# The thin 1x1 kernel on >= 262144 pixels: tests/test_ops_gpu.test_wgrad_1x1_thin_large_map holds it to 3e-4.  On zero-mean data (P is a
# normal deviate whatever Q's prologue makes of Q, so every product has mean 0) the rows below meet 2e-4 and carry it.  Measured on
# an MI355X, worst of the eleven 256-pixel rows (f32 oracle / float64): whole 9.6e-7 / 9.0e-7, per column 3.8e-6 / 4.3e-6 (the b0
# plan's 6 x 4 x 32 record at 224 x 224), per row 6.2e-7 / 6.4e-7.
TOL_NP256 = 2e-4

NO, AF, SI, RE, GE = D.PRO_NONE, D.PRO_AFFINE, D.PRO_SILU, D.PRO_RELU, D.PRO_GELU
GATHER = D.MODE_GATHER2X2


class WCase(Case):
    """Case that keeps the float64 oracle's image (per-row errors of the by_row pass)"""

    def oracles(self, packed, ref64=False):
        cpu, wide = super().oracles(packed, ref64)
        self.wide = wide
        return cpu, wide


def same_pads(size: int, k: int, s: int):
    """TF 'SAME': (output size, padding before) - plan/unet_plan.same_pads"""
    out = -(-size // s)
    return out, max((out - 1) * s + k - size, 0) // 2


def R(B, M, C, H, W, fam, k=1, s=1, prop=0, proq=0, gate=False, ct=None, coff=0, mode=0, poff=0, silu_big=False, by_row=False, seed=0,
      raises=None, gatep=False, geo=None, prod=False):
    """One case: dW[tap][m][c] += sum_pix Ppro[m][pix] * Qpro[c][pix + tap].  fam: the kernel family the launcher must take.  H, W:
    the map of Q (mode GATHER: of P - Q is the 2H x 2W gradient of a ConvTranspose k2 s2); k, s: kernel size and stride (3x3 stride 1
    pads 1, stride 2 pads TF-SAME); prop / proq: prologue codes of P / Q; gate: SE gate on Q; ct, coff: WGS is the column slice
    [coff, coff + C) of a [T][M][ct] tensor; poff: P starts this many floats into its allocation (1: 4-byte aligned only); silu_big:
    Q's BatchNorm scale x 100, SiLU arguments far beyond the range of exp; by_row: the second pass with P scaled per row.
    REFUSED rows: raises = a fragment of the launcher's message; gatep: a gate on P; geo: record fields that replace the table's
    conventions (KH, KW, STRIDE, HO, WO, ...)."""
    return dict(B=B, M=M, C=C, H=H, W=W, fam=fam, k=k, s=s, prop=prop, proq=proq, gate=gate, ct=ct or C, coff=coff, mode=mode, poff=poff,
                silu_big=silu_big, by_row=by_row, seed=seed, raises=raises, gatep=gatep, geo=geo or {}, prod=prod)


def rid(r) -> str:
    o = [f"{r['B']}x{r['M']}x{r['C']}x{r['H']}x{r['W']}"]
    if r["k"] != 1 or r["s"] != 1:
        o.append(f"k{r['k']}s{r['s']}")
    if r["prop"] or r["proq"]:
        o.append(f"pro{r['prop']}{r['proq']}")
    o += [n for n in ("gate", "gatep", "silu_big", "by_row") if r[n]]
    if r["ct"] != r["C"]:
        o.append(f"ct{r['ct']}+{r['coff']}")
    if r["mode"]:
        o.append(f"mode{r['mode']}")
    if r["poff"]:
        o.append(f"poff{r['poff']}")
    if r["geo"]:
        o.append("geo" + "".join(f"{k}{v}" for k, v in sorted(r["geo"].items())))
    if r["seed"]:
        o.append(f"s{r['seed']}")
    if r["prod"]:
        o.append("prod")
    return "-".join(o)


def geometry(r) -> dict:
    """the geometry fields of a row's record"""
    H, W, k, s = r["H"], r["W"], r["k"], r["s"]
    if r["mode"] == GATHER:
        g = dict(H=2 * H, W=2 * W, KH=2, KW=2, STRIDE=2, PAD_T=0, PAD_L=0, HO=H, WO=W)
    elif k == 1:
        g = dict(H=H, W=W, KH=1, KW=1, STRIDE=1, PAD_T=0, PAD_L=0, HO=H, WO=W)
    elif s == 1:
        g = dict(H=H, W=W, KH=k, KW=k, STRIDE=1, PAD_T=1, PAD_L=1, HO=H, WO=W)
    else:
        (ho, pt), (wo, pl) = same_pads(H, k, s), same_pads(W, k, s)
        g = dict(H=H, W=W, KH=k, KW=k, STRIDE=s, PAD_T=pt, PAD_L=pl, HO=ho, WO=wo)
    g.update(r["geo"])
    return g


def record(r) -> dict:
    """the row as tests/wgrad_dispatch.dispatch's keyword arguments (every allocation of a Case is 256-byte aligned)"""
    return dict(B=r["B"], M=r["M"], C=r["C"], CTOT=r["ct"], PROP=r["prop"], PROQ=r["proq"], MODE=r["mode"], GATEP=r["gatep"], GATEQ=r["gate"],
                P_ALIGNED16=r["poff"] % 4 == 0, Q_ALIGNED16=True, **geometry(r))


def launch(r) -> WD.Wv:
    return WD.dispatch(**record(r))


def row_edges(r) -> frozenset:
    """the launch's edges (Wv.edges) + what the record itself asks of the kernel"""
    v = launch(r)
    e = set(v.edges)
    e |= {f"P prologue {r['prop']}", f"Q prologue {r['proq']}"}
    for name, on in (("SE gate", r["gate"]), ("SE gate over a tile that straddles 2 images", r["gate"] and v.images_per_tile == 2),
                     ("SE gate over a tile that straddles >= 3 images", r["gate"] and v.images_per_tile >= 3),
                     ("CTOT > C with a column offset", r["ct"] > r["C"] and r["coff"] > 0), ("stride 2", r["s"] == 2 and r["mode"] == 0),
                     ("ReLU on Q under zero padding", r["k"] == 3 and r["proq"] == RE), ("SiLU beyond the exp range", r["silu_big"]),
                     ("P 4-byte aligned only", r["poff"] % 4 != 0), ("per output row", r["by_row"])):
        if on:
            e.add(name)
    return frozenset(e)


def build(r, scale="column"):
    """(Case, the WGRAD record's fields) of a row; scale: "column" (Q channel c, its BatchNorm shift and WGS column c times
    2^-(c mod 8)) or "row" (P channel m, its BatchNorm shift and WGS row m times 2^-(m mod 8))"""
    B, M, C, CT = r["B"], r["M"], r["C"], r["ct"]
    g = geometry(r)
    H, W, Ho, Wo, T = g["H"], g["W"], g["HO"], g["WO"], g["KH"] * g["KW"]
    c = WCase(r["seed"])
    cols = 0.5 ** (torch.arange(CT) % 8) if scale == "column" else torch.ones(CT)
    rows = 0.5 ** (torch.arange(M) % 8) if scale == "row" else torch.ones(M)
    qs = cols[r["coff"]:r["coff"] + C]
    pdata = torch.randn(B, M, Ho, Wo, generator=c.gen) * rows.view(1, M, 1, 1)
    if r["poff"]:
        P = c.t("p", (B * M * Ho * Wo + r["poff"],), torch.cat([torch.zeros(r["poff"]), pdata.reshape(-1)])).at(r["poff"], (B, M, Ho, Wo))
    else:
        P = c.t("p", (B, M, Ho, Wo), pdata)
    Q = c.t("q", (B, C, H, W), torch.randn(B, C, H, W, generator=c.gen) * qs.view(1, C, 1, 1))
    bp = c.bnv("bnvp", M) if r["prop"] else None
    bq = c.bnv("bnvq", C) if r["proq"] else None
    if r["prop"]:
        c.items["bnvp"][1][1] *= rows         # the BatchNorm shift too: u = scale * p + shift scales with its channel (ReLU exactly)
    if r["proq"]:
        c.items["bnvq"][1][1] *= qs
        if r["silu_big"]:
            c.items["bnvq"][1][0] *= 100.0
    gq = c.t("gateq", (B, C), "rand") if r["gate"] else None
    gp = c.t("gatep", (B, M), "rand") if r["gatep"] else None
    wgs = c.t("wgs", (T, M, CT), torch.randn(T, M, CT, generator=c.gen) * cols.view(1, 1, CT) * rows.view(1, M, 1))      # non-zero: the stage accumulates
    fields = dict(P=P, BNVP=bp, GATEP=gp, Q=Q, BNVQ=bq, GATEQ=gq, WGS=wgs.at(r["coff"]), B=B, M=M, C=C, CTOT=CT, PROP=r["prop"], PROQ=r["proq"],
                  MODE=r["mode"], **g)
    return c, fields


def outside_unchanged(r, c):
    """the columns of WGS the stage does not own, bit for bit (`untouched` takes the whole tensor as written)"""
    if r["ct"] > r["C"]:
        keep = torch.ones(r["ct"], dtype=torch.bool)
        keep[r["coff"]:r["coff"] + r["C"]] = False
        sent, back = c.items["wgs"][1][..., keep].contiguous().view(torch.int32), c.read(c.got, "wgs")[..., keep].contiguous().view(torch.int32)
        assert torch.equal(sent, back), f"columns of WGS outside the stage's slice changed: {(sent != back).sum().item()} words"


def tol_of(r) -> float:
    return TOL_NP256 if launch(r).NPJ == 256 else TOL


def per_row_errors(r, c):
    """worst error of one output row m of WGS against that row's own max |ref|: (f32 oracle, float64)"""
    M = r["M"]
    got = c.read(c.got, "wgs").double().transpose(0, 1).reshape(M, -1)
    out = []
    for ref in (c.read(c.ref, "wgs").double(), c.read(c.wide, "wgs", wide=True).double()):
        ref = ref.transpose(0, 1).reshape(M, -1)
        out.append(((got - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-20)))
    return out


def run_row(r):
    v = launch(r)
    assert v.result == r["fam"], f"family column {r['fam']}, the restated launcher takes {v.inst} ({v.result} {v.message}) after {v.declined}"
    tol = tol_of(r)
    c, fields = build(r)
    errs = c.run("WGRAD", ["wgs"], tol, want_variant=r["fam"], ref64=True, per_column=("wgs",), untouched=True, **fields)
    outside_unchanged(r, c)
    line = f"{rid(r)} {v.args}: whole {errs['wgs'][0]:.2e} / f64 {errs['wgs'][1]:.2e}, per column {c.parts['wgs'][0]:.2e} / {c.parts['wgs'][1]:.2e}"
    if r["by_row"]:
        c, fields = build(r, "row")
        errs = c.run("WGRAD", ["wgs"], tol, want_variant=r["fam"], ref64=True, untouched=True, **fields)
        outside_unchanged(r, c)
        e32, e64 = per_row_errors(r, c)
        line += f"; by row: whole {errs['wgs'][0]:.2e} / {errs['wgs'][1]:.2e}, per row {e32.max().item():.2e} / {e64.max().item():.2e}"
        print(line)
        for e, against in ((e32, ""), (e64, " against float64")):
            m = int(e.argmax())
            assert e[m] < tol, f"WGRAD:wgs: row {m} of {r['M']}: rel err {e[m]:.3e}{against}"
    else:
        print(line)


def run_refused(r):
    """the launcher refuses the record with its message and leaves the arena as uploaded"""
    from s2lc_amd import _lib
    from s2lc_amd.plan.program import Program

    v = launch(r)
    assert v.result == "error" and r["raises"] in v.message, (v.result, v.message)
    c, fields = build(r)
    prog = Program()
    prog.add("WGRAD", **fields)
    sent = c.image()
    gpu = sent.cuda()
    with pytest.raises(_lib.S2kError, match=re.escape(r["raises"])):
        _lib.run(prog.pack(), _lib.Bases().set("WS", gpu), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(gpu.cpu(), sent), "a refused record changed the arena"


def older(fn_or_table, conv):
    """rows of tests/test_ops_gpu.py, converted: the table is imported, not copied"""
    from tests import test_ops_gpu as O

    t = getattr(O, fn_or_table)
    if not isinstance(t, list):
        (mark,) = [m for m in t.pytestmark if m.name == "parametrize"]
        t = mark.args[1]
    return [conv(*case) for case in t]


# ---------------------------------------------------------------------------------------------------------------------------------
# wgrad_kernel<WG_PIX, 1, WM, WN, WVM, WVN, WVK, NPJ, 1, PROP, PROQ> (csrc/wgrad.hip): what wgrad_q4 and wgrad_pc decline - an SE gate
# without SiLU or off the quad kernel's maps, SiLU / GELU prologues, a thin side, fewer than 1024 pixels.  (WM, WN, WVM, WVN, WVK, NPJ)
# ---------------------------------------------------------------------------------------------------------------------------------
GENERIC_PIX = [
    # ---- (1,1,1,1,4,256): M, C <= 32 on >= 262144 pixels; the four waves split the 128 pixel pairs of a tile ----
    R(1, 8, 8, 512, 512, GENERIC),                                            # 1024 whole tiles in 256 equal splits
    R(1, 4, 8, 511, 514, GENERIC, proq=RE),                                   # 262654 pixels: ragged last tile (254 of 256); short last split
    R(2, 8, 5, 362, 363, GENERIC, proq=SI, gate=True),                        # the b5 plan's thin project conv: SiLU + SE gate; a tile straddles the two images
    R(1, 8, 8, 512, 512, GENERIC, proq=SI, silu_big=True),                    # SiLU beyond the exp range
    R(1, 8, 8, 512, 512, GENERIC, proq=GE),
    R(1, 8, 8, 512, 512, GENERIC, prop=RE, by_row=True),                      # ragged m-tile (8 of 32 rows): per output row
    R(1, 7, 8, 512, 512, GENERIC, prop=SI),
    R(1, 8, 6, 512, 512, GENERIC, prop=GE, ct=16, coff=5),                    # a column slice of a wider WGS
    # ---- (1,1,1,1,4,64): M, C <= 32 ----
    R(3, 24, 24, 7, 7, GENERIC, by_row=True),                                 # 147 pixels: tiles straddle 2 - 3 images; one split of 3 tiles
    R(8, 4, 32, 16, 16, GENERIC, proq=RE),                                    # C = 32: whole c-tile; 32 tiles in equal splits
    R(20, 32, 13, 3, 3, GENERIC, proq=SI, gate=True),                         # 3x3 maps: a 64-pixel tile holds 8 images, the gate's row changes 7 times inside it
    R(5, 24, 17, 9, 11, GENERIC, proq=GE, gate=True),                         # GELU + gate
    R(9, 32, 32, 10, 10, GENERIC, prop=RE),                                   # 900 pixels: 15 tiles, a short last split
    R(3, 24, 24, 8, 8, GENERIC, prop=SI),
    R(3, 1, 24, 8, 8, GENERIC, prop=GE, by_row=True),                         # M = 1: one past (zero) tiles, 31 clamped rows
    R(3, 24, 1, 8, 8, GENERIC, proq=RE, gate=True),                           # C = 1; ReLU + gate
    R(3, 24, 24, 8, 8, GENERIC, gate=True),                                   # the gate alone
    R(3, 24, 24, 8, 8, GENERIC, proq=SI, silu_big=True),
    # ---- (1,1,2,2,1,64): 64 x 64 tiles ----
    R(5, 64, 64, 12, 17, GENERIC),                                            # 1020 pixels: below both faster kernels' 1024
    R(3, 40, 65, 7, 7, GENERIC, proq=RE, by_row=True),                        # C = 65 one past a tile; ragged m-tile per row
    R(22, 40, 72, 7, 7, GENERIC, proq=SI, gate=True),                         # SiLU + gate, H * W = 49: tiles straddle 2 - 3 images
    R(3, 65, 40, 6, 6, GENERIC, proq=GE, by_row=True),                        # M = 65 one past a tile
    R(3, 40, 40, 8, 8, GENERIC, prop=RE),
    R(3, 64, 64, 20, 20, GENERIC, prop=SI),                                   # ConvTranspose weight gradient as a 1x1: SiLU on P; >= 1024 pixels
    R(3, 40, 40, 8, 8, GENERIC, prop=GE, ct=100, coff=33),
    R(4, 32, 144, 16, 16, GENERIC, proq=RE),                                  # M = 32 thin, C not: 64-row tile half empty
    R(4, 144, 24, 12, 12, GENERIC, by_row=True),                              # C thin: 64 x 64 tiles, three m-tiles, the last ragged
    R(3, 40, 40, 8, 8, GENERIC, proq=GE, gate=True),
    R(3, 40, 40, 8, 8, GENERIC, proq=RE, gate=True),
    R(3, 40, 40, 8, 8, GENERIC, gate=True),
    R(3, 40, 40, 8, 8, GENERIC, proq=SI),
    R(6, 40, 40, 13, 13, GENERIC, proq=SI, silu_big=True, gate=True),         # SiLU beyond the exp range under the gate; H * W = 169: tiles straddle images
    # ---- (1,2,2,2,1,64): 64 x 128 ----
    R(3, 40, 250, 8, 8, GENERIC, by_row=True),                                # ragged on both sides
    R(3, 40, 120, 7, 9, GENERIC, proq=RE),
    R(7, 64, 240, 7, 7, GENERIC, proq=SI, gate=True),                         # the b0 plan's 7x7 maps: SiLU + SE gate on 64 x 128 tiles
    R(3, 40, 120, 8, 8, GENERIC, proq=GE),
    R(3, 40, 120, 8, 8, GENERIC, prop=RE),
    R(3, 40, 120, 8, 8, GENERIC, prop=SI),
    R(3, 40, 120, 8, 8, GENERIC, prop=GE),
    # ---- (2,1,2,2,1,64): 128 x 64 ----
    R(3, 250, 40, 8, 8, GENERIC, by_row=True),
    R(3, 120, 40, 7, 9, GENERIC, proq=RE),
    R(8, 240, 72, 7, 7, GENERIC, proq=SI, gate=True),
    R(3, 120, 40, 8, 8, GENERIC, proq=GE, gate=True),
    R(3, 120, 40, 8, 8, GENERIC, prop=RE),
    R(3, 120, 40, 8, 8, GENERIC, prop=SI),
    R(3, 120, 40, 8, 8, GENERIC, prop=GE),
    # ---- (2,2,2,2,1,64): 128 x 128 ----
    R(3, 250, 240, 8, 8, GENERIC, by_row=True),
    R(3, 120, 120, 7, 9, GENERIC, proq=RE),
    R(22, 240, 250, 7, 7, GENERIC, proq=SI, gate=True),                       # 1078 pixels, 4 output tiles
    R(3, 120, 120, 8, 8, GENERIC, proq=GE),
    R(3, 120, 120, 8, 8, GENERIC, prop=RE),
    R(1, 256, 256, 8, 8, GENERIC, prop=SI),                                   # the b5 plan's ConvTranspose gradient as a 1x1 on 8 x 8 (2048 x 2048 there): whole tiles, one pixel tile
    R(3, 120, 120, 8, 8, GENERIC, prop=GE),
    R(1, 1153, 40, 8, 8, GENERIC, by_row=True),                               # M = 1153 one past nine 128-row tiles (the smallest such M that edge() gives 128 rows)
    R(1, 40, 1153, 8, 8, GENERIC),                                            # C = 1153 one past a tile
]

# ---------------------------------------------------------------------------------------------------------------------------------
# wgrad_kernel<WG_SPATIAL, 9, 1, 1, WVM, WVN, WVK, NPJ, EPT, NONE, PROQ>: thin layers off wgrad_pc's 64-wide maps, stride 2, odd tilings
# ---------------------------------------------------------------------------------------------------------------------------------
GENERIC_SPATIAL = [
    # ---- (1,1,4,128,2): M, C <= 32; npairs = R * XWe / 2 against the four k-waves' stride of 8 ----
    R(2, 24, 13, 20, 32, GENERIC, k=3, by_row=True),                          # XW 32, R 4: 64 pairs (8 | 64)
    R(2, 32, 32, 24, 20, GENERIC, k=3, proq=RE),                              # XW 20, R 6: 60 pairs (4 | 60 only): the break in the middle of the pair loop
    R(2, 8, 8, 13, 21, GENERIC, k=3, proq=RE),                                # XW 21 odd (XWe 22), R 5: 55 pairs, no multiple of 4: the waves' pair counts differ; partial last tile row
    R(1, 32, 13, 32, 40, GENERIC, k=3, ct=45, coff=32),                       # XW 40, R 3; a column slice of a concat conv's gradient
    R(3, 16, 16, 3, 22, GENERIC, k=3),                                        # R capped by HO = 3 with XWe 22: 33 pairs
    # ---- (1,2,2,128,2): M <= 32 < C; two k-waves, stride 4 ----
    R(2, 32, 64, 8, 64, GENERIC, k=3, proq=RE),                               # wgrad_pc declines C > 32: XW 64, R 2: 64 pairs
    R(2, 24, 40, 9, 36, GENERIC, k=3, by_row=True),                           # XW 36, R 3: 54 pairs (2 | 54 only)
    R(2, 32, 65, 14, 18, GENERIC, k=3, proq=RE),                              # XW 18, R 7: 63 pairs (odd); C = 65 one past a tile
    R(1, 8, 40, 6, 130, GENERIC, k=3),                                        # WO = 130: two x tiles per row, the last 2 columns wide
    # ---- (2,1,2,128,2): 32 < M <= 64, C <= 32 ----
    R(2, 64, 24, 20, 20, GENERIC, k=3, ct=64, coff=40),                       # XW 20, R 6: 60 pairs (4 | 60)
    R(2, 48, 13, 9, 36, GENERIC, k=3, proq=RE, by_row=True),                  # 54 pairs
    R(2, 33, 32, 14, 18, GENERIC, k=3),                                       # 63 pairs; M = 33: the smallest M of this form, 31 rows of its 64 empty
    R(2, 48, 13, 32, 40, GENERIC, k=3, s=2),                                  # the stem's form: stride 2, TF-SAME; HO 16, WO 20: the 6 x 20 tile needs a 13 x 41 halo, R cut to 5
    R(1, 48, 13, 33, 171, GENERIC, k=3, s=2, proq=RE),                        # odd sizes (pad 1 before); WO = 86: a 1 x 86 tile's halo does not fit, XW halved to 43 (XWe 44)
    R(1, 40, 3, 10, 256, GENERIC, k=3, s=2),                                  # the stem at 256 pixels: WO = 128 halved to 64; even width (pad 0 before)
    # ---- (2,2,1,64,1): neither side thin, halo <= 256 elements: widths without a wgrad_pc tile ----
    R(2, 40, 40, 9, 20, GENERIC, k=3, by_row=True),                           # XW 20, R 3; ragged tiles on both sides
    R(2, 65, 64, 7, 10, GENERIC, k=3, proq=RE, by_row=True),                  # XW 10, R 6: partial last row; M = 65 one past a tile
    R(3, 40, 40, 3, 10, GENERIC, k=3, proq=RE),                               # R capped by HO = 3: 15 pairs, odd: the pair loop breaks after its first half
    R(4, 64, 64, 4, 8, GENERIC, k=3, proq=RE),                                # R capped by HO (4 rows of the 8 x 8 tile): no (4, 8) form in wgrad_pc
    R(2, 48, 40, 8, 16, GENERIC, k=3, s=2),                                   # stride 2 with R capped (HO 4, WO 8): the halo fits one element per thread
    # ---- (2,2,1,64,2): stride 2 on a layer that is not thin ----
    R(2, 48, 40, 30, 30, GENERIC, k=3, s=2, by_row=True),                     # HO = WO = 15: XWe 16, R 4, halo 9 x 33
    R(2, 72, 40, 29, 31, GENERIC, k=3, s=2, proq=RE, ct=104, coff=64),        # odd sizes; ReLU under TF-SAME padding; a column slice
    R(8, 64, 65, 16, 128, GENERIC, k=3, s=2),                                 # WO = 64: 1 x 64 tiles, 64 tiles; C = 65 one past a tile
]

# ---------------------------------------------------------------------------------------------------------------------------------
# wgrad_kernel<WG_GATHER, 4, 1, WN, 2, WVN, WVK, 32, 1, PROP, NONE>: ConvTranspose k2 s2; H, W = the layer input's map (P)
# ---------------------------------------------------------------------------------------------------------------------------------
GENERIC_GATHER = [
    # ---- (1,1,2,1,2,32): M <= 32 or C <= 32 ----
    R(2, 64, 32, 8, 8, GENERIC, mode=GATHER, prop=RE),                        # whole tiles, 2 per image
    R(3, 24, 33, 5, 6, GENERIC, mode=GATHER, by_row=True),                    # no prologue; 30 pixels per image: a 32-pixel tile straddles two (the brel term of qbase); ragged last tile; C = 33 one past a tile
    R(2, 65, 24, 4, 6, GENERIC, mode=GATHER, prop=SI, by_row=True),           # M = 65 one past a tile
    R(9, 72, 13, 3, 3, GENERIC, mode=GATHER, prop=GE),                        # 9 pixels per image: a tile holds 4 - 5 images
    # ---- (1,2,2,2,1,32): 64 x 128 tiles ----
    R(1, 200, 72, 4, 6, GENERIC, mode=GATHER, prop=SI),
    R(3, 40, 129, 5, 7, GENERIC, mode=GATHER, by_row=True),                   # no prologue; 35 pixels per image: tiles straddle two; C = 129 one past a tile
    R(2, 64, 64, 16, 24, GENERIC, mode=GATHER, prop=RE),                      # 24 tiles in equal splits
    R(5, 40, 40, 8, 8, GENERIC, mode=GATHER, prop=GE, ct=80, coff=24),        # 10 tiles in splits of 4, 4 and 2
]

# ---------------------------------------------------------------------------------------------------------------------------------
# wgrad_pc_kernel<WG_SPATIAL, 9, 1, 1, WVM, WVN, WVK, NPJ, R, XWE, NONE, PROQ> (csrc/wgrad_pc.hip): 3x3 stride 1
# ---------------------------------------------------------------------------------------------------------------------------------
PC_SPATIAL = [
    # ---- 64 x 64 tiles (2,2,1,64) x the seven (R, XWE) ----
    R(2, 64, 64, 6, 64, PC, k=3, proq=RE),                                    # (1, 64)
    R(1, 65, 88, 5, 130, PC, k=3, by_row=True),                               # (1, 64): three x tiles per row, the last 2 columns wide; M = 65 one past a tile; ragged c-tile
    R(2, 72, 40, 12, 32, PC, k=3, proq=RE, ct=104, coff=64),                  # (2, 32): a column slice of a concat conv's gradient
    R(2, 40, 65, 7, 31, PC, k=3),                                             # (2, 32): XW 31 odd; partial last tile row; C = 65 one past a tile
    R(2, 256, 64, 16, 16, PC, k=3),                                           # (4, 16): 4 m-tiles
    R(3, 64, 128, 10, 15, PC, k=3, proq=RE),                                  # (4, 16): 15 valid columns, H no multiple of R
    R(4, 64, 64, 8, 8, PC, k=3, proq=RE),                                     # (8, 8)
    R(3, 40, 40, 12, 7, PC, k=3, by_row=True),                                # (8, 8): XW 7, partial last row
    R(1, 64, 96, 9, 56, PC, k=3),                                             # (1, 56)
    R(2, 64, 40, 5, 55, PC, k=3, proq=RE),                                    # (1, 56): XW 55
    R(2, 96, 64, 28, 28, PC, k=3, proq=RE),                                   # (2, 28)
    R(2, 40, 40, 9, 27, PC, k=3),                                             # (2, 28): XW 27
    R(3, 512, 64, 14, 14, PC, k=3, proq=RE),                                  # (4, 14): pixel splits over 8 m-tiles
    R(2, 128, 88, 14, 13, PC, k=3),                                           # (4, 14): XW 13
    # ---- thin: 128-pixel tiles (2 x 64) on maps >= 64 wide, C <= 32 ----
    R(2, 32, 32, 6, 64, PC, k=3, proq=RE),                                    # (1,1,1,1,4): the four consumer waves split the pixel pairs
    R(1, 24, 13, 5, 130, PC, k=3, ct=45, coff=32, by_row=True),               # the same form ragged on both sides, a column slice, three x tiles per row, odd height
    R(2, 64, 24, 5, 128, PC, k=3),                                            # (1,1,2,1,2): 64-row tiles, two k-waves
    R(2, 48, 32, 9, 64, PC, k=3, proq=RE, by_row=True),                       # the same form with a ragged m-tile (48 of 64)
]


def _pc_pix(B, M, C, H, W, prop, proq, gate, p_offset, want):
    return R(B, M, C, H, W, want, prop=prop, proq=proq, gate=gate, poff=p_offset)


def _percol(B, M, C, H, W, prop, proq, gate, want):
    return R(B, M, C, H, W, want, prop=prop, proq=proq, gate=gate, seed=39)


# ---------------------------------------------------------------------------------------------------------------------------------
# wgrad_pc_kernel<WG_PIX, 1, WM, WN, 2, 2, 1, 64, 1, 64, PROP, PROQ>: the rows of tests/test_ops_gpu.py that run on it (imported),
# under this file's checks, + what they leave out
# ---------------------------------------------------------------------------------------------------------------------------------
PC_PIX = [r for r in older("WGRAD_1X1_PC", _pc_pix) if r["fam"] == PC] + [
    R(22, 65, 129, 7, 7, PC, proq=RE, by_row=True),                           # (1, 1): M = 65 one past a tile, C = 129 one past a tile
    R(9, 250, 40, 15, 15, PC, by_row=True),                                   # (2, 1): ragged 128-row tile per output row
    R(44, 40, 40, 5, 5, PC, prop=RE, ct=64, coff=24),                         # 25-pixel maps: a tile straddles 3 - 4 images; a column slice
    R(16, 64, 64, 63, 65, PC),                                                # one output tile: 1024 pixel tiles in 256 equal splits
    R(5, 2048, 2048, 15, 15, PC),                                             # 256 output tiles fill the CUs: one split of 18 pixel tiles
]

# ---------------------------------------------------------------------------------------------------------------------------------
# wgrad_q4_kernel<WM, WN, PROP, PROQ> (csrc/wgrad_q4.hip): likewise
# ---------------------------------------------------------------------------------------------------------------------------------
QUAD = older("test_wgrad_1x1_quad", lambda B, M, C, H, W, prop, proq, gate: R(B, M, C, H, W, Q4, prop=prop, proq=proq, gate=gate)) + [
    R(11, 240, 250, 10, 10, Q4, proq=SI, gate=True, silu_big=True, seed=38),  # SiLU beyond the exp range (test_wgrad_1x1_quad_silu_beyond_exp_range)
    R(6, 65, 129, 14, 14, Q4, proq=RE, by_row=True),                          # M = 65 and C = 129 one past a tile
    R(5, 250, 40, 16, 16, Q4, prop=RE, by_row=True),                          # (2, 1) ragged 128-row tile per output row
    R(5, 250, 250, 16, 16, Q4, by_row=True),                                  # (2, 2)
    R(4, 2048, 2048, 16, 16, Q4),                                             # 256 output tiles fill the CUs: one split of 16 pixel tiles
    R(64, 40, 40, 4, 4, Q4, proq=SI, gate=True, ct=64, coff=24),              # 16-pixel maps: a tile holds 4 images, the gate's row changes inside it; a column slice
]

# ---------------------------------------------------------------------------------------------------------------------------------
# records launch_wgrad refuses: the launcher's message, and the arena as uploaded.  (The 2 GiB span check needs operands above 2 GiB:
# tests/test_ops_gpu.py has those records where they are legal, tests/test_wgrad_dispatch_cpu.py restates the refusal.)
# ---------------------------------------------------------------------------------------------------------------------------------
REFUSED = [
    R(3, 40, 40, 8, 8, None, prop=RE, proq=RE, raises="prologue combination (P 3, Q 3) is not instantiated for this mode"),
    R(3, 40, 40, 8, 8, None, proq=AF, raises="prologue combination (P 0, Q 1) is not instantiated for this mode"),
    R(2, 40, 40, 9, 20, None, k=3, proq=SI, raises="prologue combination (P 0, Q 2) is not instantiated for this mode"),
    R(2, 64, 64, 6, 64, None, k=3, proq=GE, raises="prologue combination (P 0, Q 4) is not instantiated for this mode"),      # wgrad_pc's (1, 64) declines GELU; the WSC = 66 form has none either
    R(2, 64, 32, 8, 8, None, mode=GATHER, prop=AF, raises="prologue combination (P 1, Q 0) is not instantiated for this mode"),
    R(3, 40, 40, 8, 8, None, gatep=True, raises="SE gate is only supported on the Q operand of 1x1 convs"),
    R(2, 40, 40, 9, 20, None, k=3, gate=True, raises="SE gate is only supported on the Q operand of 1x1 convs"),
    R(2, 64, 32, 8, 8, None, mode=GATHER, proq=RE, raises="gather geometry"),
    R(2, 64, 32, 8, 8, None, mode=GATHER, gate=True, raises="gather geometry"),
    R(2, 40, 40, 8, 8, None, geo=dict(HO=4, WO=4, STRIDE=1), raises="1x1 geometry"),
    R(2, 40, 40, 8, 8, None, geo=dict(KH=2, KW=2, HO=7, WO=7), raises="only 1x1, 3x3 and 2x2-transpose kernels are on this path"),
    R(1, 8, 8, 9, 64, None, geo=dict(KH=9, KW=1, STRIDE=4, HO=1, WO=16), raises="halo tile does not fit"),
]

# ---------------------------------------------------------------------------------------------------------------------------------
# every distinct (instantiation, edges, map size) among the WGRAD records of the production plans - the b5 U-Net at 13 x 256 x 256
# bs 32, the b0 U-Net at 224 x 224 bs 8, the Prithvi-100M MAE step at bs 64 and the segmentation steps at bs 16 (frozen and unfrozen
# backbone) - at the plan's own map size, B and the channel counts cut down as far as both stay the same (comments: a plan and
# record the row stands for as B x M x C, the kernel and its template arguments).  A column slice stands as the last of its tensor.
# ---------------------------------------------------------------------------------------------------------------------------------
PROD = [
    R(16, 2, 2, 128, 128, GENERIC, proq=SI, gate=True, prod=True),   # unet 32x24x24: wgrad_kernel (0, 1, 1, 1, 1, 1, 4, 256, 1, 0, 2, 0)
    R(6, 2, 32, 224, 224, GENERIC, proq=RE, prod=True),   # unet_b0 8x4x32: wgrad_kernel (0, 1, 1, 1, 1, 1, 4, 256, 1, 0, 3, 0)
    R(13, 2, 32, 256, 256, GENERIC, proq=RE, prod=True),   # unet 32x4x32: wgrad_kernel (0, 1, 1, 1, 1, 1, 4, 256, 1, 0, 3, 0)
    R(1, 2, 32, 112, 112, GENERIC, proq=SI, gate=True, prod=True),   # unet_b0 8x16x32: wgrad_kernel (0, 1, 1, 1, 1, 1, 4, 64, 1, 0, 2, 0)
    R(4, 33, 2, 56, 56, GENERIC, prod=True),   # unet_b0 8x144x24: wgrad_kernel (0, 1, 1, 1, 2, 2, 1, 64, 1, 0, 0, 0)
    R(8, 66, 2, 112, 112, GENERIC, prod=True),   # unet_b0 8x96x16: wgrad_kernel (0, 1, 1, 1, 2, 2, 1, 64, 1, 0, 0, 0)
    R(1, 33, 2, 128, 128, GENERIC, prod=True),   # unet 32x144x24: wgrad_kernel (0, 1, 1, 1, 2, 2, 1, 64, 1, 0, 0, 0)
    R(6, 64, 2, 7, 7, GENERIC, proq=SI, gate=True, prod=True),   # unet_b0 8x192x672: wgrad_kernel (0, 1, 1, 1, 2, 2, 1, 64, 1, 0, 2, 0)
    R(4, 2, 33, 56, 56, GENERIC, proq=SI, gate=True, prod=True),   # unet_b0 8x24x144: wgrad_kernel (0, 1, 1, 1, 2, 2, 1, 64, 1, 0, 2, 0)
    R(13, 2, 33, 128, 128, GENERIC, proq=SI, gate=True, prod=True),   # unet 32x24x48: wgrad_kernel (0, 1, 1, 1, 2, 2, 1, 64, 1, 0, 2, 0)
    R(1, 2, 115, 112, 112, GENERIC, prod=True),   # unet_b0 8x32x117: wgrad_kernel (0, 1, 1, 2, 2, 2, 1, 64, 1, 0, 0, 0)
    R(6, 64, 128, 7, 7, GENERIC, proq=SI, gate=True, prod=True),   # unet_b0 8x320x1152: wgrad_kernel (0, 1, 1, 2, 2, 2, 1, 64, 1, 0, 2, 0)
    R(3, 2, 128, 224, 224, GENERIC, proq=RE, gate=True, prod=True),   # seg_frozen 16x4x256: wgrad_kernel (0, 1, 1, 2, 2, 2, 1, 64, 1, 0, 3, 0)
    R(6, 128, 64, 7, 7, GENERIC, prod=True),   # unet_b0 8x1280x320: wgrad_kernel (0, 1, 2, 1, 2, 2, 1, 64, 1, 0, 0, 0)
    R(6, 1152, 1920, 7, 7, GENERIC, prop=SI, prod=True),   # unet_b0 8x1280x2048: wgrad_kernel (0, 1, 2, 2, 2, 2, 1, 64, 1, 2, 0, 0)
    R(28, 128, 128, 8, 8, GENERIC, prop=SI, prod=True),   # unet 32x2048x2048: wgrad_kernel (0, 1, 2, 2, 2, 2, 1, 64, 1, 2, 0, 0)
    R(1, 32, 32, 224, 224, PC, k=3, ct=40, coff=8, prod=True),   # unet_b0 8x32x32: wgrad_pc_kernel (1, 9, 1, 1, 1, 1, 4, 128, 2, 64, 0, 0)
    R(1, 32, 2, 224, 224, PC, k=3, ct=10, coff=8, prod=True),   # unet_b0 8x32x13: wgrad_pc_kernel (1, 9, 1, 1, 1, 1, 4, 128, 2, 64, 0, 0)
    R(1, 32, 32, 256, 256, PC, k=3, ct=40, coff=8, prod=True),   # unet 32x32x32: wgrad_pc_kernel (1, 9, 1, 1, 1, 1, 4, 128, 2, 64, 0, 0)
    R(1, 32, 2, 256, 256, PC, k=3, ct=10, coff=8, prod=True),   # unet 32x32x13: wgrad_pc_kernel (1, 9, 1, 1, 1, 1, 4, 128, 2, 64, 0, 0)
    R(1, 32, 32, 224, 224, PC, k=3, proq=RE, prod=True),   # unet_b0 8x32x32: wgrad_pc_kernel (1, 9, 1, 1, 1, 1, 4, 128, 2, 64, 0, 3)
    R(1, 32, 32, 256, 256, PC, k=3, proq=RE, prod=True),   # unet 32x32x32: wgrad_pc_kernel (1, 9, 1, 1, 1, 1, 4, 128, 2, 64, 0, 3)
    R(1, 64, 2, 112, 112, PC, k=3, ct=10, coff=8, prod=True),   # unet_b0 8x64x16: wgrad_pc_kernel (1, 9, 1, 1, 2, 1, 2, 128, 2, 64, 0, 0)
    R(1, 64, 2, 128, 128, PC, k=3, ct=10, coff=8, prod=True),   # unet 32x64x24: wgrad_pc_kernel (1, 9, 1, 1, 2, 1, 2, 128, 2, 64, 0, 0)
    R(1, 64, 64, 56, 56, PC, k=3, ct=72, coff=8, prod=True),   # unet_b0 8x128x128: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 56, 0, 0)
    R(1, 128, 2, 56, 56, PC, k=3, ct=10, coff=8, prod=True),   # unet_b0 8x128x24: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 56, 0, 0)
    R(1, 64, 64, 56, 56, PC, k=3, proq=RE, prod=True),   # unet_b0 8x128x128: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 56, 0, 3)
    R(1, 64, 64, 64, 64, PC, k=3, ct=72, coff=8, prod=True),   # unet 32x128x128: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 64, 0, 0)
    R(1, 64, 33, 64, 64, PC, k=3, ct=41, coff=8, prod=True),   # unet 32x128x40: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 64, 0, 0)
    R(1, 64, 64, 112, 112, PC, k=3, ct=72, coff=8, prod=True),   # unet_b0 8x64x64: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 64, 0, 0)
    R(1, 64, 64, 128, 128, PC, k=3, ct=72, coff=8, prod=True),   # unet 32x64x64: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 64, 0, 0)
    R(1, 128, 64, 224, 224, PC, k=3, prod=True),   # seg_frozen 16x256x768: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 64, 0, 0)
    R(1, 64, 64, 64, 64, PC, k=3, proq=RE, prod=True),   # unet 32x128x128: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 64, 0, 3)
    R(1, 64, 64, 112, 112, PC, k=3, proq=RE, prod=True),   # unet_b0 8x64x64: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 64, 0, 3)
    R(1, 64, 64, 128, 128, PC, k=3, proq=RE, prod=True),   # unet 32x64x64: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 1, 64, 0, 3)
    R(2, 64, 64, 28, 28, PC, k=3, ct=72, coff=8, prod=True),   # unet_b0 8x256x256: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 2, 28, 0, 0)
    R(2, 64, 33, 28, 28, PC, k=3, ct=41, coff=8, prod=True),   # unet_b0 8x256x40: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 2, 28, 0, 0)
    R(2, 64, 64, 28, 28, PC, k=3, proq=RE, prod=True),   # unet_b0 8x256x256: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 2, 28, 0, 3)
    R(1, 64, 64, 32, 32, PC, k=3, ct=72, coff=8, prod=True),   # unet 32x256x256: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 2, 32, 0, 0)
    R(1, 64, 64, 32, 32, PC, k=3, proq=RE, prod=True),   # unet 32x256x256: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 2, 32, 0, 3)
    R(2, 64, 64, 14, 14, PC, k=3, ct=72, coff=8, prod=True),   # unet_b0 8x512x512: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 4, 14, 0, 0)
    R(2, 64, 33, 14, 14, PC, k=3, ct=41, coff=8, prod=True),   # unet_b0 8x512x80: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 4, 14, 0, 0)
    R(2, 64, 64, 14, 14, PC, k=3, proq=RE, prod=True),   # unet_b0 8x512x512: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 4, 14, 0, 3)
    R(2, 64, 64, 16, 16, PC, k=3, ct=72, coff=8, prod=True),   # unet 32x512x512: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 4, 16, 0, 0)
    R(2, 64, 64, 16, 16, PC, k=3, proq=RE, prod=True),   # unet 32x512x512: wgrad_pc_kernel (1, 9, 1, 1, 2, 2, 1, 64, 4, 16, 0, 3)
    R(6, 33, 33, 14, 14, Q4, prod=True),   # unet_b0 8x672x112: wgrad_q4_kernel (1, 1, 0, 0)
    R(6, 33, 33, 14, 14, Q4, proq=SI, gate=True, prod=True),   # unet_b0 8x112x672: wgrad_q4_kernel (1, 1, 0, 2)
    R(4, 33, 33, 28, 28, Q4, proq=SI, gate=True, prod=True),   # unet_b0 8x40x144: wgrad_q4_kernel (1, 1, 0, 2)
    R(6, 33, 130, 64, 64, Q4, proq=SI, gate=True, prod=True),   # unet 32x40x144: wgrad_q4_kernel (1, 1, 0, 2)
    R(1, 33, 115, 128, 128, Q4, prod=True),   # unet 32x48x117: wgrad_q4_kernel (1, 2, 0, 0)
    R(16, 258, 1538, 8, 8, Q4, proq=SI, gate=True, prod=True),   # unet 32x304x1824: wgrad_q4_kernel (1, 2, 0, 2)
    R(6, 33, 115, 14, 14, Q4, proq=SI, gate=True, prod=True),   # unet_b0 8x112x480: wgrad_q4_kernel (1, 2, 0, 2)
    R(11, 130, 915, 16, 16, Q4, proq=SI, gate=True, prod=True),   # unet 32x176x1056: wgrad_q4_kernel (1, 2, 0, 2)
    R(16, 130, 768, 16, 16, Q4, proq=SI, gate=True, prod=True),   # unet 32x176x768: wgrad_q4_kernel (1, 2, 0, 2)
    R(4, 33, 115, 28, 28, Q4, proq=SI, gate=True, prod=True),   # unet_b0 8x40x240: wgrad_q4_kernel (1, 2, 0, 2)
    R(22, 64, 384, 32, 32, Q4, proq=SI, gate=True, prod=True),   # unet 32x64x384: wgrad_q4_kernel (1, 2, 0, 2)
    R(1, 64, 115, 32, 32, Q4, proq=SI, gate=True, prod=True),   # unet 32x64x240: wgrad_q4_kernel (1, 2, 0, 2)
    R(1, 33, 115, 64, 64, Q4, proq=SI, gate=True, prod=True),   # unet 32x40x240: wgrad_q4_kernel (1, 2, 0, 2)
    R(1, 64, 128, 112, 112, Q4, prop=RE, prod=True),   # unet_b0 8x64x128: wgrad_q4_kernel (1, 2, 3, 0)
    R(1, 64, 128, 128, 128, Q4, prop=RE, prod=True),   # unet 32x64x128: wgrad_q4_kernel (1, 2, 3, 0)
    R(16, 1538, 258, 8, 8, Q4, prod=True),   # unet 32x1824x304: wgrad_q4_kernel (2, 1, 0, 0)
    R(6, 115, 33, 14, 14, Q4, prod=True),   # unet_b0 8x480x80: wgrad_q4_kernel (2, 1, 0, 0)
    R(11, 915, 130, 16, 16, Q4, prod=True),   # unet 32x1056x176: wgrad_q4_kernel (2, 1, 0, 0)
    R(4, 115, 33, 28, 28, Q4, prod=True),   # unet_b0 8x240x40: wgrad_q4_kernel (2, 1, 0, 0)
    R(22, 384, 64, 32, 32, Q4, prod=True),   # unet 32x384x64: wgrad_q4_kernel (2, 1, 0, 0)
    R(1, 115, 33, 64, 64, Q4, prod=True),   # unet 32x240x40: wgrad_q4_kernel (2, 1, 0, 0)
    R(32, 128, 128, 1, 52, Q4, prod=True),   # mae 64x512x768: wgrad_q4_kernel (2, 2, 0, 0)
    R(32, 1920, 768, 1, 52, Q4, prod=True),   # mae 64x2304x768: wgrad_q4_kernel (2, 2, 0, 0)
    R(16, 384, 1280, 1, 196, Q4, prod=True),   # mae 64x768x1536: wgrad_q4_kernel (2, 2, 0, 0)
    R(8, 1280, 512, 1, 200, Q4, prod=True),   # mae 64x1536x512: wgrad_q4_kernel (2, 2, 0, 0)
    R(8, 128, 128, 1, 200, Q4, prod=True),   # mae 64x512x512: wgrad_q4_kernel (2, 2, 0, 0)
    R(16, 128, 128, 8, 8, Q4, prod=True),   # unet 32x2048x512: wgrad_q4_kernel (2, 2, 0, 0)
    R(16, 128, 128, 14, 14, Q4, prod=True),   # seg_frozen 16x768x3072: wgrad_q4_kernel (2, 2, 0, 0)
    R(4, 128, 128, 16, 16, Q4, prod=True),   # unet 32x768x128: wgrad_q4_kernel (2, 2, 0, 0)
    R(8, 384, 768, 28, 28, Q4, prod=True),   # seg_frozen 16x768x3072: wgrad_q4_kernel (2, 2, 0, 0)
    R(2, 384, 768, 56, 56, Q4, prod=True),   # seg_frozen 16x768x3072: wgrad_q4_kernel (2, 2, 0, 0)
    R(1, 384, 128, 112, 112, Q4, prod=True),   # seg_frozen 16x768x3072: wgrad_q4_kernel (2, 2, 0, 0)
    R(16, 128, 128, 8, 8, Q4, proq=SI, gate=True, prod=True),   # unet 32x512x3072: wgrad_q4_kernel (2, 2, 0, 2)
    R(16, 128, 115, 8, 8, Q4, proq=SI, gate=True, prod=True),   # unet 32x512x1824: wgrad_q4_kernel (2, 2, 0, 2)
    R(4, 128, 128, 16, 16, Q4, proq=SI, gate=True, prod=True),   # unet 32x128x768: wgrad_q4_kernel (2, 2, 0, 2)
    R(6, 128, 128, 14, 14, Q4, prop=RE, prod=True),   # unet_b0 8x512x1024: wgrad_q4_kernel (2, 2, 3, 0)
    R(4, 128, 128, 16, 16, Q4, prop=RE, prod=True),   # unet 32x512x1024: wgrad_q4_kernel (2, 2, 3, 0)
    R(4, 128, 128, 28, 28, Q4, prop=RE, prod=True),   # unet_b0 8x256x512: wgrad_q4_kernel (2, 2, 3, 0)
    R(1, 128, 128, 32, 32, Q4, prop=RE, prod=True),   # unet 32x256x512: wgrad_q4_kernel (2, 2, 3, 0)
    R(4, 128, 128, 56, 56, Q4, prop=RE, prod=True),   # unet_b0 8x128x256: wgrad_q4_kernel (2, 2, 3, 0)
    R(1, 128, 128, 64, 64, Q4, prop=RE, prod=True),   # unet 32x128x256: wgrad_q4_kernel (2, 2, 3, 0)
]

TABLES = {"GENERIC_PIX": GENERIC_PIX, "GENERIC_SPATIAL": GENERIC_SPATIAL, "GENERIC_GATHER": GENERIC_GATHER, "PC_SPATIAL": PC_SPATIAL,
          "PC_PIX": PC_PIX, "QUAD": QUAD, "REFUSED": REFUSED, "PROD": PROD}

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("r", GENERIC_PIX, ids=rid)
def test_generic_1x1_kernel(r):
    run_row(r)


@pytest.mark.parametrize("r", GENERIC_SPATIAL, ids=rid)
def test_generic_3x3_kernel(r):
    run_row(r)


@pytest.mark.parametrize("r", GENERIC_GATHER, ids=rid)
def test_generic_gather_kernel(r):
    run_row(r)


@pytest.mark.parametrize("r", PC_SPATIAL, ids=rid)
def test_producer_consumer_3x3_kernel(r):
    run_row(r)


@pytest.mark.parametrize("r", PC_PIX, ids=rid)
def test_producer_consumer_1x1_kernel(r):
    run_row(r)


@pytest.mark.parametrize("r", QUAD, ids=rid)
def test_quad_kernel(r):
    run_row(r)


@pytest.mark.parametrize("r", REFUSED, ids=rid)
def test_refused_records(r):
    run_refused(r)


@pytest.mark.parametrize("r", PROD, ids=rid)
def test_production_records(r):
    run_row(r)
