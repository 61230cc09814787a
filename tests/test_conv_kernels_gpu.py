"""The f32 dense-convolution kernels, instantiation by instantiation: csrc/igemm.hip (conv_igemm_kernel + the split-K tail),
csrc/igemm_pc.hip (conv_pc_kernel), csrc/conv_dma.hip (conv_dma_kernel) and csrc/conv_q4.hip (conv_q4_kernel), launched as one CONV
record through the C ABI behind a WEIGHT_PACK record, as a plan does.

One table per kernel family plus the production rows.  Which template instantiation a row reaches, and which loop edges, is
tests/conv_dispatch.py's restatement of launch_conv and the four launchers; tests/test_conv_dispatch_cpu.py checks without a GPU
that the tables reach every instantiation the launch macros can produce at default tuning, every edge named in the row comments,
and the instantiation and edges of every CONV record of the production plans (rows tagged PROD: the plan's own map size, B and
channels cut down where the instantiation and the edges stay the same).  Here every row is held

  * to the kernel family the launcher must take (want_variant);
  * to 1e-4 of max |ref| - the project's bar for these f32 kernels - for the whole of Y and for every output channel on its own,
    against the f32 oracle (oracle/ops_ref.py) and against a float64 run of it;
  * where the record has STATS, to the same bar for the replica-summed statistics, whole tensor and per column;
  * to leaving every byte of the arena outside Y / STATS / SCRATCH and the weight packs as uploaded;
  * for YC > M, to leaving the channels >= M of Y bit-identical.

Row = R(B, C1, H, W, M, family, options): see R below."""
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd.plan import opdefs as D
from tests import conv_dispatch as CD
from tests.conv_dispatch import DMA, GENERIC, PC, Q4
from tests.test_ops_gpu import Case

TOL = 1e-4


def same_pads(size: int, k: int, s: int):
    """TF 'SAME': (output size, padding before) - plan/unet_plan.same_pads"""
    out = -(-size // s)
    return out, max((out - 1) * s + k - size, 0) // 2


def R(B, C1, H, W, M, fam, C2=0, k=1, s=1, pro=0, pro2=None, gate=False, bias=False, stats=False, beta=0, res=False, resg=False,
      scratch=False, yc=None, mode=0, dma=False, q4=False, silu_big=False, seed=0, prod=False):
    """One case.  fam: the kernel family the launcher must take.  C2: channels of a second (concat) source; k, s: kernel size and
    stride (3x3 stride 1 pads 1, stride 2 pads TF-SAME); pro / pro2: prologue codes (pro2 defaults to pro); gate / bias / stats /
    res / scratch: the record carries GATE1 / BIAS / STATS / RES / SCRATCH; resg: RES with FLAG_RES_GELU_GRAD; beta: accumulate
    into Y; yc: channel stride of Y (> M: Y is a channel slice of a wider tensor); mode: opdefs.MODE_*; dma / q4: FLAG_DMA /
    FLAG_Q4 (+ the quad weight copy); silu_big: BatchNorm scales x 300, SiLU arguments far beyond the range of exp."""
    return dict(B=B, C1=C1, H=H, W=W, M=M, fam=fam, C2=C2, k=k, s=s, pro=pro, pro2=(pro if pro2 is None else pro2) if C2 else 0, gate=gate,
                bias=bias, stats=stats, beta=beta, res=res or resg, resg=resg, scratch=scratch, yc=yc, mode=mode, dma=dma, q4=q4,
                silu_big=silu_big, seed=seed, prod=prod)


def rid(r) -> str:
    o = [f"{r['B']}x{r['C1']}" + (f"+{r['C2']}" if r["C2"] else "") + f"x{r['H']}x{r['W']}-M{r['M']}"]
    if r["k"] != 1 or r["s"] != 1:
        o.append(f"k{r['k']}s{r['s']}")
    if r["pro"] or r["pro2"]:
        o.append(f"pro{r['pro']}" + (f"{r['pro2']}" if r["C2"] else ""))
    o += [n for n in ("gate", "bias", "stats", "beta", "resg", "scratch", "dma", "q4", "silu_big", "prod") if r[n]]
    if r["res"] and not r["resg"]:
        o.append("res")
    if r["yc"]:
        o.append(f"yc{r['yc']}")
    if r["mode"]:
        o.append(f"mode{r['mode']}")
    return "-".join(o)


def geometry(r):
    """(HO, WO, PAD_T, PAD_L) of a row"""
    if r["k"] == 1:
        return r["H"], r["W"], 0, 0
    if r["s"] == 1:
        return r["H"], r["W"], 1, 1
    (ho, pt), (wo, pl) = same_pads(r["H"], r["k"], r["s"]), same_pads(r["W"], r["k"], r["s"])
    return ho, wo, pt, pl


def record(r) -> dict:
    """the row as tests/conv_dispatch.dispatch's keyword arguments"""
    ho, wo, pt, pl = geometry(r)
    flags = (CD.FLAG_DMA if r["dma"] else 0) | (CD.FLAG_Q4 if r["q4"] else 0) | (CD.FLAG_RES_GELU_GRAD if r["resg"] else 0)
    return dict(B=r["B"], C1=r["C1"], C2=r["C2"], H=r["H"], W=r["W"], M=r["M"], KH=r["k"], KW=r["k"], STRIDE=r["s"], PAD_T=pt, PAD_L=pl, HO=ho,
                WO=wo, PRO1=r["pro"], PRO2=r["pro2"], MODE=r["mode"], GATE=r["gate"], BIAS=r["bias"], RES=r["res"], STATS=r["stats"],
                SCRATCH=r["scratch"], BETA=r["beta"], YC=r["yc"], NREP=D.stats_replicas(r["M"]) if r["stats"] else 1, flags=flags)


def row_edges(r) -> frozenset:
    """the launch's edges (Cv.edges) + what the record itself asks of the kernel"""
    cv = CD.dispatch(**record(r))
    e = set(cv.edges)
    e.add(f"prologue {r['pro']}")
    for name, on in (("SE gate", r["gate"]), ("bias", r["bias"]), ("statistics", r["stats"]), ("beta", r["beta"]), ("residual", r["res"] and not r["resg"]),
                     ("residual x gelu'", r["resg"]), ("concat", r["C2"] > 0), ("YC > M", bool(r["yc"]) and r["mode"] == 0 and r["yc"] > r["M"]),
                     ("scatter mode", r["mode"] == D.MODE_CONVT_SCATTER), ("gather mode", r["mode"] == D.MODE_GATHER2X2), ("stride 2", r["s"] == 2),
                     ("SiLU beyond the exp range", r["silu_big"]), ("M = 4", r["M"] == 4), ("M one past a tile", cv.BM > 0 and r["M"] % cv.BM == 1),
                     ("statistics replicas > 1", r["stats"] and min(cv.nrep, cv.n_mtiles * cv.n_ntiles) > 1),
                     ("one statistics replica", r["stats"] and cv.nrep == 1)):
        if on:
            e.add(name)
    if cv.splits > 1:
        e |= {f"reduce tail: {n}" for n in ("bias", "statistics", "beta", "residual") if n in e}
    return frozenset(e)


def build(r):
    """(Case, outputs, the WEIGHT_PACK record, the CONV record's fields) of a row"""
    B, C1, C2, H, W, M, k, mode = r["B"], r["C1"], r["C2"], r["H"], r["W"], r["M"], r["k"], r["mode"]
    Ho, Wo, pt, pl = geometry(r)
    c = Case(r["seed"])
    T, Ct = k * k, C1 + C2
    x1 = c.t("x1", (B, C1 // 4, 2 * H, 2 * W) if mode == D.MODE_GATHER2X2 else (B, C1, H, W))
    x2 = c.t("x2", (B, C2, H, W)) if C2 else None
    bnv1 = c.bnv("bnv1", C1) if r["pro"] else None
    bnv2 = c.bnv("bnv2", C2) if (C2 and r["pro2"]) else None
    if r["silu_big"]:
        c.items["bnv1"][1][0] *= 300.0
    g1 = c.t("gate1", (B, C1), "rand") if r["gate"] else None
    # Output channel c is scaled by 2^-(c mod 8) - weights, bias, residual and the old content of Y alike, an exact scaling, so the
    # channel's sums and their rounding errors scale with it: a value that lands in the wrong channel, or an error in one row of
    # an m-tile, shows against that channel's own max |ref| where the whole tensor's max would hide it
    nch = M // 4 if mode == D.MODE_CONVT_SCATTER else M
    YC = r["yc"] or nch
    chs = 0.5 ** (torch.arange(YC) % 8)
    if mode == D.MODE_CONVT_SCATTER:     # ConvTranspose weights [Cin][Cout][2x2]: row m = (co, dy, dx)
        wt, (sm, sk, st) = c.t("wt", (C1, nch, 4), torch.randn(C1, nch, 4, generator=c.gen) * (1.0 / Ct) ** 0.5 * chs[:nch].view(1, nch, 1)), (1, M, 1)
    else:
        wt, (sm, sk, st) = c.t("wt", (M, Ct, T), torch.randn(M, Ct, T, generator=c.gen) * (1.0 / (Ct * T)) ** 0.5 * chs[:M].view(M, 1, 1)), (Ct * T, T, 1)
    bs = c.t("bias", (nch,), torch.randn(nch, generator=c.gen) * chs[:nch]) if r["bias"] else None
    yshape = (B, YC, 2 * Ho, 2 * Wo) if mode == D.MODE_CONVT_SCATTER else (B, YC, Ho, Wo)
    y = c.t("y", yshape, torch.randn(yshape, generator=c.gen) * chs.view(1, YC, 1, 1) if (r["beta"] or YC > M) else "nan")
    nrep = D.stats_replicas(M) if r["stats"] else 1
    st_ref = c.t("stats", (nrep, 2, M), "zeros", "f64") if r["stats"] else None
    extra = {}
    if r["res"]:
        # (FLAG_RES_GELU_GRAD multiplies by gelu'(RES): the output scales with the weights alone, RES keeps its range)
        extra["RES"] = c.t("res", yshape, torch.randn(yshape, generator=c.gen) * 1.5 * (1.0 if r["resg"] else chs.view(1, YC, 1, 1)))
    if r["scratch"]:
        extra["SCRATCH"] = c.t("scratch", (8 * B * YC * Ho * Wo,), "nan")
    flags = (D.FLAG_DMA if r["dma"] else 0) | (D.FLAG_Q4 if r["q4"] else 0) | (D.FLAG_RES_GELU_GRAD if r["resg"] else 0)
    if flags:
        extra["_flags"] = flags
    if r["q4"]:
        pre, wp, MP, wpq = c.pack(wt, M, Ct, T, sm, sk, st, 0, q4=True)
        extra["WTB"] = wpq
    else:
        pre, wp, MP = c.pack(wt, M, Ct, T, sm, sk, st, 0)
    fields = dict(NREP=nrep, X1=x1, BNV1=bnv1, GATE1=g1, X2=x2, BNV2=bnv2, WT=wp, BIAS=bs, Y=y, STATS=st_ref, B=B, C1=C1, C2=C2, H=H, W=W, M=M, KH=k,
                  KW=k, STRIDE=r["s"], PAD_T=pt, PAD_L=pl, HO=Ho, WO=Wo, PRO1=r["pro"], PRO2=r["pro2"], MODE=mode, W_SM=1, W_SK=T * MP, W_ST=MP,
                  FLIP=0, BETA=r["beta"], YC=YC, **extra)
    return c, ["y"] + (["stats"] if r["stats"] else []), pre, fields


def run_row(r):
    c, outs, pre, fields = build(r)
    c.run("CONV", outs, TOL, sum0=("stats",), pre=[pre], want_variant=r["fam"], ref64=True, per_channel=("y",),
          per_column=("stats",) if r["stats"] else (), untouched=True, **fields)
    # `untouched` takes the weight packs as written by the WEIGHT_PACK record: a CONV kernel must leave them as that record made
    # them - the f32 pack as the oracle's, bit for bit, the quad copy as its regrouping [K / 8][MP][8], channel k of a group at
    # (k & 1) * 4 + (k >> 1)
    pack = c.read(c.got, c.packed[0].name)
    assert torch.equal(pack.view(torch.int32), c.read(c.ref, c.packed[0].name).view(torch.int32)), "the f32 weight pack changed under the CONV stage"
    if r["q4"]:
        KP, MP = pack.shape
        if r["k"] == 1:
            quad = pack.view(KP // 8, 4, 2, MP).permute(0, 3, 2, 1).reshape(KP // 8, MP, 8)      # [kg][m][(k & 1) * 4 + (k >> 1)]
        else:           # WEIGHT_PACK writes the quad copy of 1x1 entries only: still what was uploaded
            quad = c.items[c.packed[1].name][1]
        assert torch.equal(c.read(c.got, c.packed[1].name).reshape(-1).view(torch.int32), quad.contiguous().reshape(-1).view(torch.int32)), \
            "the quad weight copy changed under the CONV stage"
    M, YC = r["M"], fields["YC"]
    if r["mode"] == D.MODE_CONV and YC > M:        # `untouched` takes all of Y as written: the channels the stage does not own, bit for bit
        sent = c.items["y"][1][:, M:].contiguous().view(torch.int32)
        back = c.read(c.got, "y")[:, M:].contiguous().view(torch.int32)
        assert torch.equal(sent, back), f"channels >= M of Y changed: {(sent != back).sum().item()} words"


PRO_NONE, PRO_AFFINE, PRO_SILU, PRO_RELU, PRO_GELU = D.PRO_NONE, D.PRO_AFFINE, D.PRO_SILU, D.PRO_RELU, D.PRO_GELU

NO, AF, SI, RE, GE = PRO_NONE, PRO_AFFINE, PRO_SILU, PRO_RELU, PRO_GELU

# ---------------------------------------------------------------------------------------------------------------------------------
# conv_igemm_kernel<BMODE, TT, WM, WN, WVM, WVN, KCH, EPT, MINW, BVEC> (csrc/igemm.hip): what the three other launchers decline
# ---------------------------------------------------------------------------------------------------------------------------------
GENERIC_ROWS = [
    # ---- 1x1, 64 x 64 tiles (1,1,2,2, KCH 64): bm >= 64 and fewer than 400 large tiles; the only form that may split K ----
    R(2, 24, 8, 8, 48, GENERIC, stats=True),                                   # vector stager, transposed store; K < one chunk; ragged m-tile (48 of 64); 2 replicas used
    R(3, 70, 7, 7, 120, GENERIC, pro=RE, stats=True, bias=True),                # HW = 49: scalar stager + scalar epilogue; tiles straddle 2 images, ragged last pixel tile; K tail (70 = 64 + 6); ragged m-tile (120 = 64 + 56)
    R(5, 130, 5, 5, 33, GENERIC, pro=SI, gate=True, stats=True),               # HW = 25: a 64-pixel tile touches 3 - 4 images (scalar stager); M = 33 one past 32: 64-row tile, 31 rows empty
    R(9, 40, 4, 4, 100, GENERIC, pro=AF, gate=True, beta=1),                   # 4x4 maps: 4 images per tile on the vector stager; AFFINE prologue + gate; accumulate
    R(2, 96, 12, 12, 64, GENERIC, pro=GE, bias=True, res=True, yc=80),         # GELU prologue; bias + residual; Y is a 64-channel slice of an 80-channel tensor
    R(2, 96, 11, 13, 64, GENERIC, pro=GE, gate=True, res=True, yc=70),         # ... on the scalar stager / scalar epilogue (HW = 143), with the gate
    R(2, 48, 8, 8, 64, GENERIC, gate=True, stats=True),                         # the SE gate alone (no BatchNorm prologue)
    R(2, 64, 8, 8, 64, GENERIC, pro=SI, silu_big=True, stats=True),            # SiLU arguments of +-1000: exp overflows, the quotient must not
    R(3, 64, 7, 9, 64, GENERIC, pro=SI, gate=True, silu_big=True),             # ... scalar stager
    R(2, 40, 6, 6, 120, GENERIC, C2=24, pro=RE, pro2=NO, stats=True),           # concat of a ReLU source and a raw one (pro2 != pro1: per-element prologue form), vector stager; the chunk holds both sources
    R(2, 40, 5, 7, 120, GENERIC, C2=30, pro=NO, pro2=SI, bias=True),            # ... raw + SiLU, scalar stager; K tail (70) ends in source 2
    R(2, 64, 8, 8, 120, GENERIC, C2=70, pro=AF, stats=True),                    # concat, both AFFINE: K tail (134 = 2 x 64 + 6) in source 2
    # split-K (SCRATCH given, >= 4 chunks): rule A = blocks <= 512
    R(2, 264, 8, 8, 120, GENERIC, pro=SI, gate=True, stats=True, scratch=True),            # 4 blocks: 256 splits asked, capped at 8, then at nchunks / 2 = 2; 5 chunks = 3 + 2 (shorter last split); statistics in the reduce tail
    R(2, 264, 8, 8, 120, GENERIC, pro=SI, gate=True, stats=True),                          # the same record without SCRATCH must not split
    R(1, 1030, 8, 8, 64, GENERIC, pro=SI, bias=True, beta=1, res=True, scratch=True),     # 1 block, 17 chunks (tail 6): capped at 8 -> 6 splits of 3, the last 2; bias + residual + accumulate in the reduce tail
    R(1, 1030, 6, 6, 64, GENERIC, bias=True, resg=True, scratch=True, yc=96),             # HW = 36; the tail multiplies by gelu'(RES); Y a channel slice; nothing but K split decides the stores
    R(342, 384, 8, 8, 64, GENERIC, bias=True, stats=True, scratch=True),                  # 342 blocks: 3 splits, no cap, 6 chunks = 2 + 2 + 2; bias + statistics in the reduce tail, 64 replicas
    # rule B: 512 < blocks <= 1024 and >= 32 chunks - 8 m-tiles x 65 pixel tiles x 32 chunks is the smallest such problem (7.9 GFLOP)
    R(65, 1985, 8, 8, 481, GENERIC, pro=SI, stats=True, scratch=True),                    # 520 blocks: 3 splits of 11 chunks, the last 10 (its last chunk holds one channel); ragged m-tile (481 = 7 x 64 + 33)
    # ---- 1x1, 128 x 128 tiles, 16-channel chunks (2,2,2,2, KCH 16): bm = 128, K <= 192, >= 400 tiles ----
    R(13, 8, 64, 64, 120, GENERIC, stats=True),                                # vector stager; K < one chunk; ragged m-tile (120 of 128); 416 tiles over 34 replicas
    R(1, 24, 227, 227, 128, GENERIC, pro=RE, bias=True),                       # HW odd: scalar stager + scalar epilogue; K tail (24 = 16 + 8); ragged last pixel tile
    # ---- 1x1, 128 x 128 tiles, 64-channel chunks (2,2,2,2, KCH 64): bm = 128, K > 192 (193 .. 255 or a prologue the pc kernel lacks) ----
    R(13, 200, 64, 64, 120, GENERIC, pro=SI, gate=True, stats=True),           # vector stager, SiLU + gate (the project conv's form); K tail (200 = 3 x 64 + 8)
    R(1, 200, 227, 227, 128, GENERIC, pro=AF, beta=1),                         # scalar stager + scalar epilogue, AFFINE prologue, accumulate
    # ---- 1x1, 64 x 256 tiles (2,2,1,4, KCH 16): bm = 64, >= 400 tiles ----
    R(9, 20, 62, 62, 180, GENERIC, pro=AF, stats=True),                        # vector stager; the 64-lane transposed store; ragged m-tile (180 = 2 x 64 + 52); K tail (20 = 16 + 4); tiles straddle images (HW = 3844)
    R(9, 20, 63, 61, 180, GENERIC, pro=SI, gate=True, bias=True),              # scalar stager + scalar epilogue
    # ---- 1x1, 32 x 256 tiles (1,2,1,4, KCH 16): bm = 32 ----
    R(2, 32, 24, 24, 4, GENERIC, pro=RE, gate=True, bias=True),                # M = 4 (the output conv; the segmentation head gates it with its dropout mask): 28 of 32 rows empty
    R(2, 13, 9, 9, 65, GENERIC, stats=True),                                   # M = 65 one past a tile (3 m-tiles, the last holds one row); scalar stager; K < one chunk
    R(2, 144, 10, 10, 24, GENERIC, beta=1, yc=40),                             # an expand conv's data gradient: accumulate into a channel slice
    R(3, 24, 16, 16, 96, GENERIC, stats=True, bias=True),                      # M = 96 = 3 x 32 exactly (128- and 64-row tiles would waste a third)
    R(1, 8, 4, 4, 2100, GENERIC, pro=AF, stats=True),                          # M > 2048: one statistics replica; 64 x 64 tiles (bm = 128 but one pixel tile), the last m-tile ragged
    # statistics of the FINISHED rows: with a residual and / or an accumulate they are taken after both (no plan combines them)
    R(2, 48, 8, 8, 64, GENERIC, gate=True, bias=True, stats=True, res=True),               # transposed store
    R(3, 70, 7, 7, 120, GENERIC, pro=RE, stats=True, beta=1),                              # scalar epilogue
    R(2, 264, 8, 8, 120, GENERIC, pro=SI, gate=True, stats=True, res=True, beta=1, scratch=True),      # the split-K reduce tail
    R(2, 16, 20, 20, 64, GENERIC, k=3, pro=RE, stats=True, res=True),                      # 3x3, transposed store
    # scatter / gather modes (generic only)
    R(2, 24, 8, 8, 64, GENERIC, pro=RE, bias=True, mode=D.MODE_CONVT_SCATTER),            # ConvTranspose k2 s2: rows (co, dy, dx) scattered as 2x2 patches; never the transposed store
    R(1, 200, 5, 6, 516, GENERIC, pro=SI, bias=True, mode=D.MODE_CONVT_SCATTER),          # scalar stager (HW = 30), ragged m-tile on 64-row tiles, K tail
    R(2, 64, 6, 10, 24, GENERIC, beta=1, mode=D.MODE_GATHER2X2),                          # ConvTranspose data gradient: pseudo-channels (co, dy, dx) gathered from the 2x map; scalar stager with HW % 4 == 0
    R(2, 72, 7, 5, 80, GENERIC, bias=True, mode=D.MODE_GATHER2X2),                        # ... HW = 35, K tail (72 = 64 + 8), 64-row tiles
    # ---- 3x3, 128 x 128 tiles (2,2,2,2, KCH 8, EPT 2) ----
    R(20, 8, 20, 20, 240, GENERIC, k=3, pro=AF, bias=True, stats=True),        # XW 20, R 6: partial last tile row (20 = 3 x 6 + 2); AFFINE prologue: the halo at all four borders is zero AFTER the prologue; transposed store
    R(30, 12, 18, 18, 250, GENERIC, k=3, pro=SI, silu_big=True, beta=1),       # W = 18: scalar epilogue; K tail (12 = 8 + 4); SiLU beyond the exp range under zero padding
    # ---- 3x3, 64 x 256 tiles (2,2,1,4, KCH 8, EPT 4) ----
    R(26, 4, 40, 40, 64, GENERIC, k=3, pro=GE, stats=True),                    # XW 40, R 6 (partial last row: 40 = 6 x 6 + 4); K < one chunk; GELU prologue
    R(7, 13, 160, 161, 48, GENERIC, k=3, s=2, stats=True),                     # stride 2, TF-SAME (pad 0 at the top, 1 at the left for the odd width): the stem conv's form; WO = 81: scalar epilogue
    # ---- 3x3, 64 x 64 tiles (1,1,2,2, KCH 8, EPT 2) ----
    R(2, 40, 20, 20, 64, GENERIC, C2=24, k=3, bias=True, stats=True),          # decoder concat; XW 20, R 3: partial last row
    R(2, 16, 30, 26, 48, GENERIC, C2=5, k=3, pro=RE, pro2=NO, bias=True),      # ReLU source + raw source (per-element prologue form); K tail (21) in source 2; W = 26: scalar epilogue
    R(3, 16, 4, 8, 64, GENERIC, k=3, pro=RE, stats=True),                      # R capped by HO (4 rows of an 8-row tile)
    R(2, 6, 30, 26, 48, GENERIC, k=3, s=2, bias=True, stats=True),             # stride 2 on 64-pixel tiles, K < one chunk
    R(1, 9, 12, 70, 100, GENERIC, k=3, pro=AF),                                # WO = 70 > 64: two x tiles per row, partial last tile column; ragged m-tile
    # ---- 3x3 thin (M <= 32) ----
    R(7, 4, 122, 122, 24, GENERIC, k=3, pro=RE, bias=True, stats=True),        # 32 x 512 tiles (1,4,1,4, EPT 5): >= 200 tiles of 512 pixels, XW 122, R 4 (partial last row); scalar epilogue by design
    R(1, 2, 456, 450, 8, GENERIC, k=3, bias=True, stats=True),                 # 32 x 1024 tiles (1,8,1,4, EPT 7, MINW 1): rows of 450 do not fit the 512-tile's halo; R cut from 2 to 1 by this tile's halo capacity
    R(1, 16, 40, 300, 32, GENERIC, C2=8, k=3, bias=True, stats=True),          # 32 x 256 tiles (1,2,1,4, EPT 4): XW 256 of 300: two x tiles per row, partial column; R 1
    R(2, 5, 9, 12, 4, GENERIC, k=3, pro=SI, bias=True),                        # M = 4, K < one chunk, XW 12, R 9 capped by HO; transposed store
    R(2, 32, 13, 13, 17, GENERIC, k=3, s=2, beta=1),                           # thin + stride 2 + accumulate
    R(1, 8, 32, 32, 17, GENERIC, k=3, s=2, stats=True),                        # stride 2: a 16 x 16 output tile needs a 33 x 33 halo, one row more than the capacity: R cut to 15, partial last tile row
]

# ---------------------------------------------------------------------------------------------------------------------------------
# conv_pc_kernel<BMODE, WM, KCH, R, XW, PRO, THIN, NARROW> (csrc/igemm_pc.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
PC_ROWS = [
    # ---- 1x1, 128-pixel tiles, 32-channel chunks: >= 192 tiles and K >= 256 ----
    R(6, 256, 64, 64, 128, PC, stats=True),                                    # WM 2: 192 tiles exactly; whole chunks; statistics over 32 replicas
    R(3, 264, 100, 100, 120, PC, pro=RE, bias=True),                           # WM 2, ReLU; K tail (264 = 8 x 32 + 8); ragged m-tile; HW = 10000: tiles straddle images, ragged last tile
    R(24, 256, 32, 32, 64, PC, beta=1, res=True),                              # WM 1 (M = 64 pads a 128-row tile by half)
    R(9, 280, 26, 26, 193, PC, pro=RE, stats=True, yc=200),                    # WM 1, ReLU; M = 193 one past a tile (4 m-tiles); K tail 24; HW = 676; Y a channel slice
    R(24, 256, 32, 32, 64, PC, bias=True, resg=True),                          # fc2's data gradient times gelu'(fc1 output): the residual multiplies
    R(6, 256, 16, 16, 2100, PC, stats=True),                                   # M > 2048: one statistics replica (17 m-tiles x 12)
    # ---- 1x1, narrow 64 x 64 tiles: < 192 tiles of 128 pixels, K >= 512, >= 384 narrow tiles ----
    R(12, 512, 32, 32, 128, PC, bias=True, stats=True),                        # 2 x 192 narrow tiles
    R(5, 520, 26, 26, 500, PC, pro=RE, beta=1),                                # ReLU; K tail (520 = 16 x 32 + 8); ragged m-tile (500 = 7 x 64 + 52); tiles straddle images, ragged last tile
    # ---- 3x3 thin (20 <= M <= 32): 32 x (4 x 64) tiles, 4-channel chunks, >= 512 tiles ----
    R(4, 4, 128, 256, 32, PC, C2=5, k=3, bias=True, stats=True),               # four x tiles per row; concat: the K tail (9 = 2 x 4 + 1) is source 2's last channel
    R(8, 6, 254, 64, 24, PC, k=3, pro=RE, beta=1),                             # ReLU under zero padding; M = 24: ragged m-tile; partial last tile row (254 = 63 x 4 + 2); K tail 2
    # ---- 3x3, (R, XW) by the map width x KCH {4 (M < 256), 8} x WM {1, 2} x {NONE, ReLU}: m-tiles x pixel tiles >= 160 ----
    # (2, 64): WO a multiple of 64
    R(2, 8, 54, 64, 192, PC, k=3, stats=True),                                 # KCH 4, WM 1 (3 m-tiles x 54)
    R(2, 6, 54, 64, 160, PC, k=3, pro=RE, bias=True, stats=True),              # ... ReLU; K tail (6 = 4 + 2); ragged m-tile
    R(2, 8, 40, 128, 240, PC, k=3, bias=True),                                 # KCH 4, WM 2 (2 x 80): two x tiles per row; ragged m-tile
    R(2, 3, 40, 128, 230, PC, k=3, pro=RE, beta=1),                            # ... ReLU; K < one chunk
    R(1, 12, 63, 64, 264, PC, k=3, stats=True),                                # KCH 8, WM 1 (5 x 32): partial last tile row; K tail (12 = 8 + 4)
    R(1, 8, 63, 64, 257, PC, k=3, pro=RE, res=True),                           # ... ReLU; M = 257 one past a tile
    R(2, 8, 79, 64, 256, PC, k=3, bias=True, stats=True),                      # KCH 8, WM 2 (2 x 80)
    R(2, 5, 79, 64, 256, PC, C2=6, k=3, pro=RE, stats=True),                   # ... ReLU on both sources of a concat; K tail (11 = 8 + 3) in source 2, the first chunk holds both
    R(2, 8, 54, 64, 192, PC, k=3, bias=True, stats=True, res=True),            # statistics of the finished rows: after the residual (transposed store)
    R(2, 8, 54, 64, 192, PC, k=3, pro=RE, stats=True, beta=1),                 # ... after the accumulate
    # (4, 32): WO = 32
    R(6, 8, 36, 32, 192, PC, k=3, beta=1),
    R(6, 7, 34, 32, 192, PC, k=3, pro=RE, stats=True),                         # partial last tile row (34 = 8 x 4 + 2); K tail 3
    R(8, 8, 40, 32, 240, PC, k=3, stats=True, bias=True),
    R(8, 4, 40, 32, 240, PC, C2=4, k=3, pro=RE, bias=True),                    # concat, whole chunks: chunk 1 is source 2
    R(4, 8, 30, 32, 264, PC, k=3, bias=True),
    R(4, 16, 30, 32, 264, PC, k=3, pro=RE, stats=True),
    R(10, 8, 32, 32, 256, PC, k=3, stats=True),
    R(10, 12, 32, 32, 256, PC, k=3, pro=RE, bias=True, yc=300),                # Y a channel slice
    # (8, 16): WO = 16
    R(27, 8, 16, 16, 192, PC, k=3, bias=True, stats=True),
    R(27, 4, 16, 16, 192, PC, k=3, pro=RE, beta=1),
    R(40, 8, 16, 16, 240, PC, k=3, res=True),
    R(40, 6, 12, 16, 240, PC, k=3, pro=RE, stats=True),                        # partial last tile row (12 = 8 + 4)
    R(16, 8, 16, 16, 264, PC, k=3, stats=True),
    R(16, 8, 16, 16, 320, PC, k=3, pro=RE, bias=True),
    R(40, 6, 12, 16, 256, PC, k=3, beta=1),                                    # K < one 8-channel chunk; partial last tile row
    R(40, 9, 16, 16, 256, PC, k=3, pro=RE, stats=True),                        # K tail (9 = 8 + 1)
    # (2, 56): WO = 56, 112, 224 (224-pixel inputs)
    R(2, 8, 54, 56, 192, PC, k=3, stats=True),                                 # 112-pixel tiles: 16 columns of the 128 idle
    R(2, 8, 53, 56, 192, PC, k=3, pro=RE, bias=True),                          # partial last tile row
    R(2, 8, 40, 112, 240, PC, k=3, stats=True),                                # two x tiles per row
    R(2, 8, 40, 112, 240, PC, k=3, pro=RE, beta=1),
    R(1, 8, 16, 224, 264, PC, k=3, bias=True),                                 # four x tiles per row
    R(1, 8, 15, 224, 264, PC, k=3, pro=RE, stats=True),
    R(2, 8, 79, 56, 256, PC, k=3, stats=True),
    R(2, 8, 79, 56, 256, PC, k=3, pro=RE, res=True),
    # (4, 28): WO = 28
    R(6, 8, 36, 28, 192, PC, k=3, bias=True),
    R(6, 8, 36, 28, 192, PC, k=3, pro=RE, stats=True),
    R(8, 8, 40, 28, 240, PC, k=3, stats=True),
    R(8, 8, 38, 28, 240, PC, k=3, pro=RE, bias=True),                          # partial last tile row
    R(4, 8, 30, 28, 264, PC, k=3, stats=True),
    R(4, 8, 30, 28, 264, PC, k=3, pro=RE, beta=1),
    R(10, 8, 32, 28, 256, PC, k=3, bias=True),
    R(10, 8, 32, 28, 256, PC, k=3, pro=RE, stats=True),
    # (8, 14): WO = 14 - XW % 4 != 0: the only geometry with the scalar epilogue and the LDS statistics rows
    R(27, 8, 14, 14, 192, PC, k=3, bias=True, stats=True),                     # partial last tile row (14 = 8 + 6)
    R(27, 8, 14, 14, 192, PC, k=3, pro=RE, beta=1, res=True),
    R(27, 8, 14, 14, 192, PC, k=3, stats=True, beta=1, res=True),              # statistics after residual + accumulate on the scalar epilogue
    R(40, 8, 14, 14, 240, PC, k=3, stats=True),
    R(40, 8, 14, 14, 240, PC, k=3, pro=RE, bias=True, yc=256),
    R(16, 8, 14, 14, 264, PC, k=3, bias=True, stats=True),
    R(16, 8, 14, 14, 264, PC, k=3, pro=RE, resg=True),
    R(40, 8, 14, 14, 256, PC, k=3, stats=True),
    R(40, 8, 14, 14, 256, PC, k=3, pro=RE, bias=True, stats=True),
]

# ---------------------------------------------------------------------------------------------------------------------------------
# conv_dma_kernel<WM, WN, NST, PRE, KCH> (csrc/conv_dma.hip): FLAG_DMA = every shape the kernel supports; the tile and the K split
# come out of the launcher's cost search (comments: WM x WN, stage depth)
# ---------------------------------------------------------------------------------------------------------------------------------
DMA_ROWS = [
    R(1, 40, 4, 4, 40, DMA, dma=True),                                         # 1 x 1, 32-channel stages: one item for 256 workgroups; K = 40: a stage + a half stage of 8; ragged m-tile and pixel tile
    R(5, 100, 10, 10, 72, DMA, bias=True, stats=True, dma=True),               # 1 x 1 PRE: HW = 100: tiles straddle 2 images, ragged last tile; K tail of 4 channels; bias prefetched, statistics
    R(6, 17, 4, 4, 48, DMA, stats=True, dma=True),                             # 1 x 1, 16-channel stages (K <= 32): 4 images per tile; K = 17 = a stage + 1 channel
    R(1, 8, 4, 4, 65, DMA, bias=True, res=True, beta=1, dma=True, yc=70),      # 1 x 1 PRE 16: K < one stage; M = 65 one past a tile; bias + residual + accumulate prefetched; Y a channel slice
    R(5, 40, 36, 36, 129, DMA, stats=True, dma=True),                          # 1 x 2: 153 items; M = 129 one past a tile; 31 replicas
    R(5, 40, 36, 36, 129, DMA, beta=1, dma=True),                              # 1 x 2 PRE
    R(5, 8, 36, 36, 129, DMA, dma=True),                                       # 1 x 2, 16-channel stages
    R(5, 8, 36, 36, 129, DMA, bias=True, dma=True),                            # 1 x 2 PRE 16
    R(8, 136, 32, 32, 129, DMA, scratch=True, dma=True),                       # 2 x 1: 256 items exactly, so SCRATCH or not nothing is cut; K tail 8 of a 32 stage
    R(8, 136, 32, 32, 129, DMA, bias=True, scratch=True, dma=True),            # 2 x 1 PRE
    R(5, 8, 32, 34, 384, DMA, stats=True, dma=True),                           # 2 x 1, 16-channel stages: 255 items where the equally priced 1 x 2 tile has 258 (two rounds)
    R(5, 24, 32, 34, 384, DMA, res=True, dma=True),                            # 2 x 1 PRE 16; K = 24: a stage + a half stage
    R(5, 40, 36, 36, 640, DMA, stats=True, dma=True),                          # 2 x 2: 255 items
    R(5, 40, 36, 36, 640, DMA, bias=True, dma=True),                           # 2 x 2 PRE
    R(5, 8, 36, 36, 640, DMA, dma=True),                                       # 2 x 2, 16
    R(5, 8, 36, 36, 640, DMA, beta=1, dma=True),                               # 2 x 2 PRE 16
    R(4, 40, 64, 64, 129, DMA, dma=True),                                      # 3 x 1: M = 129 on a 192-row tile
    R(4, 40, 64, 64, 129, DMA, res=True, dma=True),                            # 3 x 1 PRE
    R(4, 8, 64, 64, 129, DMA, stats=True, dma=True),                           # 3 x 1, 16
    R(4, 8, 64, 64, 129, DMA, bias=True, stats=True, dma=True),                # 3 x 1 PRE 16
    R(4, 40, 64, 64, 384, DMA, stats=True, dma=True),                          # 3 x 2 (no PRE form: 6 accumulator tiles)
    R(4, 8, 64, 64, 384, DMA, dma=True),                                       # 3 x 2, 16
    R(4, 40, 64, 64, 200, DMA, dma=True),                                      # 4 x 1: M = 200 on a 256-row tile
    R(4, 40, 64, 64, 200, DMA, beta=1, dma=True),                              # 4 x 1 PRE
    R(4, 8, 64, 64, 200, DMA, stats=True, dma=True),                           # 4 x 1, 16
    R(4, 8, 64, 64, 200, DMA, bias=True, dma=True),                            # 4 x 1 PRE 16
    R(4, 8, 64, 64, 512, DMA, stats=True, dma=True),                           # 4 x 2 (16-channel stages only, no PRE form)
    R(4, 8, 64, 64, 300, DMA, dma=True),                                       # 5 x 1 (16-channel stages only): M = 300 on a 320-row tile
    R(4, 8, 64, 64, 300, DMA, bias=True, dma=True),                            # 5 x 1 PRE
    # the persistent loop and the K split
    R(9, 40, 64, 64, 40, DMA, stats=True, dma=True),                           # 576 items on 256 workgroups: 2 or 3 items each (a skipped last item loses a pixel tile)
    R(9, 8, 64, 64, 40, DMA, beta=1, dma=True),                                # ... PRE, 16-channel stages: the prefetch of the next item's bias / old value
    R(1, 136, 4, 4, 40, DMA, bias=True, stats=True, scratch=True, dma=True),   # 2 splits of 2 and 3 stages (balanced partition); bias + statistics in the reduce tail
    R(1, 136, 4, 4, 40, DMA, bias=True, stats=True, dma=True),                 # the same record without SCRATCH must not split
    R(2, 520, 8, 8, 304, DMA, beta=1, res=True, scratch=True, dma=True),       # 8 splits; residual + accumulate in the reduce tail, the PRE kernel must not add them to the partials
    R(5, 100, 10, 10, 72, DMA, bias=True, stats=True, res=True, dma=True),     # statistics of the finished rows: after the prefetched residual
    R(1, 40, 4, 4, 40, DMA, stats=True, beta=1, dma=True),                     # ... after the accumulate
    R(1, 136, 4, 4, 40, DMA, stats=True, res=True, beta=1, scratch=True, dma=True),        # ... in the reduce tail
    R(1, 32, 4, 4, 40, DMA, stats=True, dma=True),                             # K = 32: the last K with 16-channel stages (two whole stages)
    R(1, 33, 4, 4, 40, DMA, stats=True, dma=True),                             # K = 33: the first K with 32-channel stages (a stage + 1 channel)
    R(1, 8, 4, 4, 2100, DMA, stats=True, dma=True),                            # M > 2048: one statistics replica
    R(4, 512, 8, 8, 64, DMA, stats=True),                                      # unflagged: the routing rule (Ntot <= 8192, K >= 512) after the pc kernel declines (2 tiles)
    R(4, 512, 8, 8, 64, DMA, stats=True, q4=True),                             # FLAG_Q4 alone: the quad kernel's rule declines (K < 2048), the pc kernel declines, the ring kernel's rule takes it
]

# ---------------------------------------------------------------------------------------------------------------------------------
# conv_q4_kernel<WM, WVM, WVN, NST, PRE, KCH> (csrc/conv_q4.hip): FLAG_Q4 + FLAG_DMA = every shape the kernel supports
# (comments: tile rows x pixels; PRE 0 plain, 1 bias, 2 residual / accumulate)
# ---------------------------------------------------------------------------------------------------------------------------------
QUAD_ROWS = [
    R(1, 8, 4, 4, 24, Q4, stats=True, dma=True, q4=True),                      # 128 x 128 (1,4,1), 16-channel stages: M = 24 (the smallest), K < one stage, one item
    R(6, 17, 4, 4, 48, Q4, bias=True, stats=True, dma=True, q4=True),          # ... PRE 1: 4x4 maps, a tile holds 6 images; K = 17
    R(1, 8, 4, 4, 129, Q4, res=True, beta=1, dma=True, q4=True, yc=140),       # ... PRE 2: M = 129 one past a tile; Y a channel slice
    R(1, 40, 4, 4, 24, Q4, dma=True, q4=True),                                 # 128 x 128, 32-channel stages: K = 40 = a stage + one k-group of 8
    R(5, 100, 10, 10, 72, Q4, bias=True, stats=True, dma=True, q4=True),       # ... PRE 1: HW = 100: tiles straddle images, ragged last tile; K tail of 4 channels
    R(3, 52, 1, 52, 96, Q4, bias=True, res=True, beta=1, dma=True, q4=True),   # ... PRE 2: a Linear over 52-token rows
    R(26, 8, 36, 36, 24, Q4, dma=True, q4=True),                               # 64 x 256 (1,2,2), 16
    R(26, 8, 36, 36, 24, Q4, bias=True, stats=True, dma=True, q4=True),        # ... PRE 1
    R(26, 8, 36, 36, 24, Q4, res=True, dma=True, q4=True),                     # ... PRE 2
    R(26, 40, 36, 36, 24, Q4, stats=True, dma=True, q4=True),                  # 64 x 256, 32
    R(26, 40, 36, 36, 24, Q4, bias=True, dma=True, q4=True),                   # ... PRE 1
    R(26, 40, 36, 36, 24, Q4, beta=1, dma=True, q4=True),                      # ... PRE 2
    R(17, 40, 64, 64, 24, Q4, stats=True, dma=True, q4=True),                  # 64 x 512 (2,1,4): 16-channel stages whatever K; K = 40: two stages + a k-group
    R(17, 8, 64, 64, 24, Q4, bias=True, dma=True, q4=True),                    # ... PRE 1
    R(4, 40, 64, 64, 300, Q4, stats=True, dma=True, q4=True),                  # 128 x 256 (2,2,2), 32
    R(4, 40, 64, 64, 300, Q4, bias=True, dma=True, q4=True),                   # ... PRE 1
    R(4, 8, 64, 64, 300, Q4, dma=True, q4=True),                               # 128 x 256, 16
    R(4, 8, 64, 64, 300, Q4, bias=True, stats=True, dma=True, q4=True),        # ... PRE 1
    R(8, 36, 64, 64, 176, Q4, stats=True, dma=True, q4=True),                  # 256 x 128 (2,4,1), 32: M = 176 on a 256-row tile; K tail 4
    R(8, 36, 64, 64, 176, Q4, bias=True, dma=True, q4=True),                   # ... PRE 1
    R(4, 8, 64, 64, 512, Q4, stats=True, dma=True, q4=True),                   # 256 x 128, 16
    R(4, 8, 64, 64, 512, Q4, bias=True, dma=True, q4=True),                    # ... PRE 1
    # the persistent loop and the K split
    R(9, 8, 64, 64, 65, Q4, res=True, dma=True, q4=True),                      # 288 items on 256 workgroups
    R(9, 40, 64, 64, 65, Q4, stats=True, dma=True, q4=True),                   # ... 32-channel stages, statistics
    R(1, 136, 4, 4, 24, Q4, bias=True, stats=True, scratch=True, dma=True, q4=True),     # 2 splits of 2 and 3 stages; bias + statistics in the reduce tail
    R(1, 136, 4, 4, 24, Q4, bias=True, stats=True, dma=True, q4=True),                   # the same record without SCRATCH must not split
    R(2, 520, 8, 8, 304, Q4, beta=1, res=True, scratch=True, dma=True, q4=True),         # 8 splits; residual + accumulate in the reduce tail only
    R(5, 100, 10, 10, 72, Q4, bias=True, stats=True, res=True, dma=True, q4=True),         # statistics of the finished rows: after the residual (PRE 2)
    R(26, 8, 36, 36, 24, Q4, stats=True, beta=1, dma=True, q4=True),                       # ... after the accumulate
    R(1, 136, 4, 4, 24, Q4, stats=True, res=True, scratch=True, dma=True, q4=True),        # ... in the reduce tail
    R(1, 32, 4, 4, 24, Q4, stats=True, dma=True, q4=True),                     # K = 32: the last K with 16-channel stages
    R(1, 33, 4, 4, 24, Q4, stats=True, dma=True, q4=True),                     # K = 33: the first K with 32-channel stages
    R(1, 8, 4, 4, 2100, Q4, stats=True, dma=True, q4=True),                    # M > 2048: one statistics replica
]

# ---------------------------------------------------------------------------------------------------------------------------------
# flagged records a link of the chain must decline, pinned to the family that finally takes them
# ---------------------------------------------------------------------------------------------------------------------------------
DECLINED_ROWS = [
    R(2, 64, 8, 8, 64, GENERIC, pro=SI, gate=True, stats=True, dma=True),      # FLAG_DMA with a gated SiLU operand: the ring and pc kernels have no prologue
    R(2, 64, 7, 7, 64, GENERIC, bias=True, dma=True),                          # FLAG_DMA with HW % 4 != 0
    R(2, 64, 8, 8, 24, GENERIC, stats=True, dma=True),                         # FLAG_DMA with M < 40
    R(2, 64, 8, 8, 16, GENERIC, beta=1, dma=True, q4=True),                    # FLAG_Q4 | FLAG_DMA with M < 24: the flagged ring launch comes after the pc kernel, and declines too
    R(2, 40, 8, 8, 64, GENERIC, C2=24, dma=True, q4=True),                     # ... with a concat
    R(24, 256, 32, 32, 64, PC, bias=True, resg=True, dma=True, q4=True),       # ... with FLAG_RES_GELU_GRAD: neither ring kernel multiplies by gelu'(RES)
    R(2, 256, 6, 6, 64, GENERIC, bias=True, resg=True, scratch=True, dma=True),          # ... few tokens: the generic kernel's split-K tail
    R(5, 8, 64, 64, 64, PC, k=3, stats=True, dma=True, q4=True),               # a 3x3 record with both flags set: the pc kernel (160 tiles)
]

# ---------------------------------------------------------------------------------------------------------------------------------
# every distinct (instantiation, edges) among the CONV records of the production plans - the b5 U-Net at 13 x 256 x 256 bs 32, the
# Prithvi-100M MAE step at bs 64 and the segmentation steps at bs 16 (frozen and unfrozen backbone) - at the plan's own map size and
# flags (FLAG_Q4 where the planner sets it, never FLAG_DMA), B and the channel counts cut down as far as both stay the same
# (comments: the template arguments, GFLOP)
# ---------------------------------------------------------------------------------------------------------------------------------
PROD_ROWS = [
    R(20, 136, 8, 8, 800, DMA, scratch=True, prod=True),   # (1, 1, 3, False, 32) 0.28 GF
    R(32, 512, 16, 16, 128, DMA, scratch=True, prod=True),   # (1, 1, 3, False, 32) 1.07 GF
    R(32, 512, 16, 16, 128, DMA, beta=1, scratch=True, prod=True),   # (1, 1, 3, True, 32) 1.07 GF
    R(32, 36, 16, 16, 1056, DMA, prod=True),   # (3, 1, 3, False, 32) 0.62 GF
    R(32, 36, 16, 16, 1056, DMA, stats=True, prod=True),   # (3, 1, 3, False, 32) 0.62 GF
    R(32, 36, 16, 16, 768, DMA, prod=True),   # (3, 2, 3, False, 32) 0.45 GF
    R(32, 64, 16, 16, 768, DMA, prod=True),   # (3, 2, 3, False, 32) 0.81 GF
    R(32, 64, 16, 16, 768, DMA, stats=True, prod=True),   # (3, 2, 3, False, 32) 0.81 GF
    R(32, 992, 8, 8, 304, DMA, scratch=True, prod=True),   # (5, 1, 4, False, 16) 1.24 GF
    R(32, 992, 8, 8, 304, DMA, beta=1, scratch=True, prod=True),   # (5, 1, 4, True, 16) 1.24 GF
    R(1, 200, 32, 32, 64, GENERIC, pro=SI, gate=True, stats=True, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 0.03 GF
    R(1, 256, 32, 32, 64, GENERIC, pro=SI, gate=True, stats=True, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 0.03 GF
    R(1, 64, 16, 16, 64, GENERIC, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 0.00 GF
    R(1, 64, 8, 8, 64, GENERIC, pro=SI, bias=True, mode=D.MODE_CONVT_SCATTER, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 0.00 GF
    R(29, 384, 16, 16, 176, GENERIC, pro=SI, gate=True, stats=True, scratch=True, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 1.00 GF
    R(29, 416, 16, 16, 176, GENERIC, pro=SI, gate=True, stats=True, scratch=True, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 1.09 GF
    R(30, 992, 8, 8, 304, GENERIC, pro=SI, gate=True, stats=True, scratch=True, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 1.16 GF
    R(32, 256, 16, 16, 64, GENERIC, pro=SI, gate=True, stats=True, scratch=True, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 0.27 GF
    R(32, 512, 16, 16, 128, GENERIC, pro=SI, gate=True, stats=True, scratch=True, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 1.07 GF
    R(32, 512, 8, 8, 512, GENERIC, pro=SI, gate=True, stats=True, scratch=True, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 1.07 GF
    R(32, 608, 8, 8, 512, GENERIC, pro=SI, gate=True, stats=True, scratch=True, prod=True),   # (0, 1, 1, 1, 2, 2, 64, 1, 2, True) 1.28 GF
    R(1, 16, 128, 128, 24, GENERIC, pro=SI, gate=True, stats=True, prod=True),   # (0, 1, 1, 2, 1, 4, 16, 1, 2, True) 0.01 GF
    R(1, 16, 128, 128, 24, GENERIC, prod=True),   # (0, 1, 1, 2, 1, 4, 16, 1, 2, True) 0.01 GF
    R(1, 16, 224, 224, 4, GENERIC, pro=RE, gate=True, bias=True, prod=True),   # (0, 1, 1, 2, 1, 4, 16, 1, 2, True) 0.01 GF
    R(1, 16, 256, 256, 4, GENERIC, pro=RE, bias=True, prod=True),   # (0, 1, 1, 2, 1, 4, 16, 1, 2, True) 0.01 GF
    R(1, 20, 128, 128, 24, GENERIC, pro=SI, gate=True, stats=True, prod=True),   # (0, 1, 1, 2, 1, 4, 16, 1, 2, True) 0.02 GF
    R(1, 20, 128, 128, 24, GENERIC, prod=True),   # (0, 1, 1, 2, 1, 4, 16, 1, 2, True) 0.02 GF
    R(1, 4, 256, 256, 32, GENERIC, prod=True),   # (0, 1, 1, 2, 1, 4, 16, 1, 2, True) 0.02 GF
    R(25, 16, 64, 64, 40, GENERIC, pro=SI, gate=True, stats=True, prod=True),   # (0, 1, 2, 2, 1, 4, 16, 1, 2, True) 0.13 GF
    R(13, 16, 64, 64, 128, GENERIC, pro=RE, bias=True, mode=D.MODE_CONVT_SCATTER, prod=True),   # (0, 1, 2, 2, 2, 2, 16, 1, 2, True) 0.22 GF
    R(4, 16, 128, 128, 128, GENERIC, pro=RE, bias=True, mode=D.MODE_CONVT_SCATTER, prod=True),   # (0, 1, 2, 2, 2, 2, 16, 1, 2, True) 0.27 GF
    R(10, 256, 56, 56, 256, GENERIC, bias=True, mode=D.MODE_CONVT_SCATTER, prod=True),   # (0, 1, 2, 2, 2, 2, 64, 1, 2, True) 4.11 GF
    R(16, 256, 14, 14, 2048, GENERIC, bias=True, mode=D.MODE_CONVT_SCATTER, prod=True),   # (0, 1, 2, 2, 2, 2, 64, 1, 2, True) 3.29 GF
    R(16, 256, 28, 28, 640, GENERIC, bias=True, mode=D.MODE_CONVT_SCATTER, prod=True),   # (0, 1, 2, 2, 2, 2, 64, 1, 2, True) 4.11 GF
    R(25, 256, 32, 32, 256, GENERIC, pro=RE, bias=True, mode=D.MODE_CONVT_SCATTER, prod=True),   # (0, 1, 2, 2, 2, 2, 64, 1, 2, True) 3.36 GF
    R(29, 256, 16, 16, 896, GENERIC, pro=RE, bias=True, mode=D.MODE_CONVT_SCATTER, prod=True),   # (0, 1, 2, 2, 2, 2, 64, 1, 2, True) 3.41 GF
    R(5, 256, 112, 112, 128, GENERIC, bias=True, mode=D.MODE_CONVT_SCATTER, prod=True),   # (0, 1, 2, 2, 2, 2, 64, 1, 2, True) 4.11 GF
    R(1, 8, 16, 16, 64, GENERIC, k=3, prod=True),   # (1, 9, 1, 1, 2, 2, 8, 2, 2, False) 0.00 GF
    R(10, 8, 64, 64, 40, GENERIC, k=3, prod=True),   # (1, 9, 2, 2, 1, 4, 8, 4, 2, False) 0.24 GF
    R(24, 256, 32, 32, 64, PC, beta=1, prod=True),   # (0, 1, 32, 1, 64, 0, False, False) 0.81 GF
    R(24, 256, 32, 32, 64, PC, prod=True),   # (0, 1, 32, 1, 64, 0, False, False) 0.81 GF
    R(32, 256, 16, 16, 176, PC, beta=1, scratch=True, prod=True),   # (0, 1, 32, 1, 64, 0, False, False) 0.74 GF
    R(32, 256, 16, 16, 176, PC, scratch=True, prod=True),   # (0, 1, 32, 1, 64, 0, False, False) 0.74 GF
    R(16, 512, 14, 14, 512, PC, scratch=True, prod=True),   # (0, 1, 32, 1, 64, 0, False, True) 1.64 GF
    R(16, 512, 1, 196, 512, PC, bias=True, scratch=True, prod=True),   # (0, 1, 32, 1, 64, 0, False, True) 1.64 GF
    R(16, 512, 1, 200, 512, PC, bias=True, res=True, scratch=True, prod=True),   # (0, 1, 32, 1, 64, 0, False, True) 1.68 GF
    R(16, 512, 1, 200, 512, PC, scratch=True, prod=True),   # (0, 1, 32, 1, 64, 0, False, True) 1.68 GF
    R(64, 512, 1, 52, 512, PC, bias=True, scratch=True, prod=True),   # (0, 1, 32, 1, 64, 0, False, True) 1.74 GF
    R(64, 512, 1, 52, 512, PC, bias=True, res=True, scratch=True, prod=True),   # (0, 1, 32, 1, 64, 0, False, True) 1.74 GF
    R(64, 512, 1, 52, 512, PC, scratch=True, prod=True),   # (0, 1, 32, 1, 64, 0, False, True) 1.74 GF
    R(16, 256, 28, 28, 256, PC, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.64 GF
    R(24, 256, 32, 32, 128, PC, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.61 GF
    R(24, 256, 8, 8, 2176, PC, stats=True, scratch=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.71 GF
    R(2, 256, 112, 112, 128, PC, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.64 GF
    R(32, 256, 16, 16, 384, PC, scratch=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.61 GF
    R(32, 256, 8, 8, 1440, PC, scratch=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.51 GF
    R(32, 256, 8, 8, 1536, PC, scratch=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.61 GF
    R(32, 256, 8, 8, 1536, PC, stats=True, scratch=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.61 GF
    R(32, 264, 8, 8, 1440, PC, scratch=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.56 GF
    R(32, 264, 8, 8, 1440, PC, stats=True, scratch=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.56 GF
    R(64, 256, 1, 196, 256, PC, bias=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.64 GF
    R(64, 256, 1, 200, 256, PC, bias=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.68 GF
    R(64, 256, 1, 200, 256, PC, bias=True, res=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.68 GF
    R(64, 256, 1, 200, 256, PC, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.68 GF
    R(64, 256, 1, 52, 1024, PC, bias=True, scratch=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.74 GF
    R(64, 256, 1, 52, 1024, PC, scratch=True, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.74 GF
    R(6, 256, 64, 64, 128, PC, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.61 GF
    R(8, 256, 56, 56, 128, PC, prod=True),   # (0, 2, 32, 1, 64, 0, False, False) 1.64 GF
    R(2, 4, 128, 128, 64, PC, C2=4, k=3, bias=True, stats=True, prod=True),   # (1, 1, 4, 2, 64, 0, False, False) 0.30 GF
    R(2, 4, 128, 128, 64, PC, k=3, prod=True),   # (1, 1, 4, 2, 64, 0, False, False) 0.15 GF
    R(2, 4, 128, 128, 64, PC, k=3, pro=RE, bias=True, stats=True, prod=True),   # (1, 1, 4, 2, 64, 3, False, False) 0.15 GF
    R(20, 4, 32, 32, 64, PC, k=3, prod=True),   # (1, 1, 4, 4, 32, 0, False, False) 0.09 GF
    R(2, 4, 256, 256, 32, PC, C2=5, k=3, bias=True, stats=True, prod=True),   # (1, 1, 4, 4, 64, 0, True, False) 0.68 GF
    R(2, 4, 256, 256, 32, PC, k=3, prod=True),   # (1, 1, 4, 4, 64, 0, True, False) 0.30 GF
    R(8, 4, 128, 128, 24, PC, k=3, prod=True),   # (1, 1, 4, 4, 64, 0, True, False) 0.23 GF
    R(2, 4, 256, 256, 32, PC, k=3, pro=RE, bias=True, stats=True, prod=True),   # (1, 1, 4, 4, 64, 3, True, False) 0.30 GF
    R(5, 4, 64, 64, 128, PC, C2=4, k=3, bias=True, stats=True, prod=True),   # (1, 2, 4, 2, 64, 0, False, False) 0.38 GF
    R(5, 4, 64, 64, 128, PC, k=3, prod=True),   # (1, 2, 4, 2, 64, 0, False, False) 0.19 GF
    R(5, 4, 64, 64, 128, PC, k=3, pro=RE, bias=True, stats=True, prod=True),   # (1, 2, 4, 2, 64, 3, False, False) 0.19 GF
    R(1, 8, 224, 224, 256, PC, k=3, bias=True, stats=True, prod=True),   # (1, 2, 8, 2, 56, 0, False, False) 1.85 GF
    R(1, 8, 224, 224, 256, PC, k=3, prod=True),   # (1, 2, 8, 2, 56, 0, False, False) 1.85 GF
    R(10, 8, 32, 32, 256, PC, C2=8, k=3, bias=True, stats=True, prod=True),   # (1, 2, 8, 4, 32, 0, False, False) 0.75 GF
    R(10, 8, 32, 32, 256, PC, k=3, prod=True),   # (1, 2, 8, 4, 32, 0, False, False) 0.38 GF
    R(10, 8, 32, 32, 256, PC, k=3, pro=RE, bias=True, stats=True, prod=True),   # (1, 2, 8, 4, 32, 3, False, False) 0.38 GF
    R(27, 8, 16, 16, 384, PC, C2=8, k=3, bias=True, stats=True, prod=True),   # (1, 2, 8, 8, 16, 0, False, False) 0.76 GF
    R(27, 8, 16, 16, 384, PC, k=3, prod=True),   # (1, 2, 8, 8, 16, 0, False, False) 0.38 GF
    R(27, 8, 16, 16, 384, PC, k=3, pro=RE, bias=True, stats=True, prod=True),   # (1, 2, 8, 8, 16, 3, False, False) 0.38 GF
    R(16, 36, 64, 64, 40, Q4, beta=1, q4=True, prod=True),   # (1, 2, 2, 3, 2, 32) 0.19 GF
    R(32, 2048, 8, 8, 256, Q4, scratch=True, q4=True, prod=True),   # (1, 4, 1, 3, 0, 32) 2.15 GF
    R(32, 64, 32, 32, 128, Q4, q4=True, prod=True),   # (1, 4, 1, 3, 0, 32) 0.54 GF
    R(32, 64, 32, 32, 128, Q4, stats=True, q4=True, prod=True),   # (1, 4, 1, 3, 0, 32) 0.54 GF
    R(32, 2048, 8, 8, 256, Q4, beta=1, scratch=True, q4=True, prod=True),   # (1, 4, 1, 3, 2, 32) 2.15 GF
    R(32, 16, 64, 64, 40, Q4, q4=True, prod=True),   # (2, 1, 4, 4, 0, 16) 0.17 GF
    R(32, 20, 64, 64, 144, Q4, q4=True, prod=True),   # (2, 1, 4, 4, 0, 16) 0.75 GF
    R(8, 16, 128, 128, 64, Q4, q4=True, prod=True),   # (2, 1, 4, 4, 0, 16) 0.27 GF
    R(8, 20, 128, 128, 48, Q4, q4=True, prod=True),   # (2, 1, 4, 4, 0, 16) 0.25 GF
    R(8, 20, 128, 128, 48, Q4, stats=True, q4=True, prod=True),   # (2, 1, 4, 4, 0, 16) 0.25 GF
    R(32, 64, 32, 32, 176, Q4, q4=True, prod=True),   # (2, 4, 1, 3, 0, 32) 0.74 GF
    R(8, 36, 64, 64, 176, Q4, q4=True, prod=True),   # (2, 4, 1, 3, 0, 32) 0.42 GF
    R(8, 36, 64, 64, 176, Q4, stats=True, q4=True, prod=True),   # (2, 4, 1, 3, 0, 32) 0.42 GF
    R(1, 4, 224, 224, 256, Q4, q4=True, prod=True),   # (2, 4, 1, 4, 0, 16) 0.10 GF
]
TABLES = {"GENERIC": GENERIC_ROWS, "PC": PC_ROWS, "DMA_RING": DMA_ROWS, "QUAD": QUAD_ROWS, "DECLINED": DECLINED_ROWS, "PROD": PROD_ROWS}

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("r", GENERIC_ROWS, ids=rid)
def test_generic_kernel(r):
    run_row(r)


@pytest.mark.parametrize("r", PC_ROWS, ids=rid)
def test_producer_consumer_kernel(r):
    run_row(r)


@pytest.mark.parametrize("r", DMA_ROWS, ids=rid)
def test_dma_ring_kernel(r):
    run_row(r)


@pytest.mark.parametrize("r", QUAD_ROWS, ids=rid)
def test_quad_kernel(r):
    run_row(r)


@pytest.mark.parametrize("r", DECLINED_ROWS, ids=rid)
def test_declined_flags_reach_the_family_that_takes_the_record(r):
    run_row(r)


@pytest.mark.parametrize("r", PROD_ROWS, ids=rid)
def test_production_records(r):
    run_row(r)

