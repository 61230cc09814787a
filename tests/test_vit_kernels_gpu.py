"""The Prithvi MAE-ViT stages of csrc/vit.hip and csrc/attn.hip, pinned to the kernel that runs and taken through every dispatch
path, loop trip and edge the plans of plan/vit_plan.py reach: the LayerNorm row kernel at every rows-per-wave count and channel
split (even, uneven, 8) and on both sides of each of its boundaries, the second trip of every grid-stride loop, the attention
kernels at head dims that do not fill their tiles, at every wave-group edge, with row padding full of NaN and with logits that
stress the online softmax, the scalar MAE-loss kernel, and the options of PATCHIFY / TRANSPOSE_CL / TOKEN_GATHER / IDS_TO_DEC_IDX
no op test passed before.

Every case compares with oracle/ops_ref.py in f32 AND in float64.  Bars are the project's (tests/test_vit_ops_gpu.py): LayerNorm
forward 2e-5, backward 1e-4, attention 1e-4 forward / 2e-4 backward, MAE loss 2e-5, activations 1e-5, of the output's max |ref| -
applied to the whole output and to each part a wrong range could hide in (channel, (batch, head), q / k / v third, feature row,
patch) against that part's own max.  Index outputs and pure data movement are bit-exact.  tests/vit_dispatch.py restates the
dispatch; tests/test_vit_dispatch_cpu.py checks the tables below against it without a GPU."""
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import ops_ref
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan.program import Program
from tests.test_ops_gpu import Case, _shape_ids
from tests.test_vit_ops_gpu import ATTN, LN_SHAPES

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _execute(c: Case, records, want_variant=None):
    """the records as one program: byte images of the GPU run, the f32 oracle and the float64 oracle"""
    prog = Program()
    for kind, fields in records:
        prog.add(kind, **fields)
    return c.execute(prog.pack(), ref64=True, want_variant=want_variant, kind="+".join(k for k, _ in records))


def _rel(a, b, dims=None, each=False):
    """max |a - b| / max |b|, over everything or (dims: the axes reduced) per slice of the other axes; each: the tensor of the
    slices' figures instead of their maximum"""
    a, b = a.double(), b.double()
    if dims is None:
        return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
    e = (a - b).abs().amax(dims) / b.abs().amax(dims).clamp_min(1e-30)
    return e if each else e.max().item()


def _check(c, bufs, name, bar, parts=(), what="", view=None, stress=False):
    """output `name` of the GPU image against both oracles at `bar`: over the whole tensor and, for each (label, dims) of `parts`,
    per slice against the slice's own max |ref|.  view: a function reshaping the tensor first.  stress: the bar of each figure -
    the whole tensor's, and EACH slice's own - becomes max(bar, 8 E), E = the f32 oracle's own error against float64 in that
    figure (the factor 8 covers the kernel's fast exp and its different summation order)."""
    f = view or (lambda t: t)
    got, w32, w64 = f(c.read(bufs[0], name)), f(c.read(bufs[1], name)), f(c.read(bufs[2], name, wide=True))
    assert torch.isfinite(got).all(), f"{what}:{name}: GPU produced non-finite values"
    assert torch.isfinite(w32).all() and torch.isfinite(w64).all(), f"{what}:{name}: oracle produced non-finite values"
    out = {}
    for label, dims in (("whole", None),) + tuple(parts):
        e32, e64 = _rel(got, w32, dims), _rel(got, w64, dims)
        if dims is None or not stress:
            lim = max(bar, 8 * _rel(w32, w64)) if stress else bar
            ok = e32 < lim and e64 < lim
        else:       # every slice against its own limit
            lims = (8 * _rel(w32, w64, dims, each=True)).clamp_min(bar)
            ok = bool((_rel(got, w32, dims, each=True) < lims).all() and (_rel(got, w64, dims, each=True) < lims).all())
            lim = lims.max().item()
        print(f"{what} {name} [{label}]: rel err {e32:.2e} (f32 oracle) {e64:.2e} (float64), bar {lim:.1e}")
        assert ok, f"{what}:{name} [{label}]: rel err {e32:.3e} (f32 oracle) {e64:.3e} (float64), bar {lim:.1e}"
        out[label] = (e32, e64)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _check_exact(c, bufs, name, what="", rounded=False):
    """bit-exact against the f32 oracle, NaN sentinels included (what the op does not write must stay as it was); against float64
    the same values and the same untouched positions (rounded: the op adds once - each value within one f32 rounding, 2^-23 of it)"""
    got, w32, w64 = c.read(bufs[0], name), c.read(bufs[1], name), c.read(bufs[2], name, wide=True)
    assert torch.equal(_bits(got), _bits(w32)), f"{what}:{name}: differs from the f32 oracle"
    if got.dtype == torch.float32:
        a, b = got.double().nan_to_num(0.0), w64.nan_to_num(0.0)
        assert torch.equal(torch.isnan(got), torch.isnan(w64)), f"{what}:{name}: untouched positions differ from the float64 oracle"
        assert ((a - b).abs() <= 2.0 ** -23 * b.abs()).all() if rounded else torch.equal(a, b), f"{what}:{name}: differs from the float64 oracle"
    else:
        assert torch.equal(got, w64), f"{what}:{name}: differs from the float64 oracle"
    return got


# ---------------------------------------------------------------------------------------------------------------
# CHAN_LN_FWD: row kernel (8) and tile kernel (0)
# ---------------------------------------------------------------------------------------------------------------
# (B, C, HW): rows per wave 6, 5, 5 (the shuffle tree over a non-power-of-two count); an uneven 7-way channel split whose
# all-channel sums wrap; 8 splits; 5 splits; the last batch size the row kernel takes; then the shapes the older table reaches
LN_ROWS = [(5, 300, 40), (4, 260, 44), (3, 200, 48), (2, 1000, 52), (1, 1024, 64), (2, 700, 60), (127, 64, 56)] \
    + [s[:3] for s in LN_SHAPES if s[3] == 8]
# (B, C, HW, misaligned X): B = 128; an X that is not 16-byte aligned; HW just outside 32..64; C = 63; the long-row shapes
LN_TILE = [(128, 64, 56, False), (3, 768, 52, True), (2, 64, 28, False), (2, 64, 68, False), (2, 63, 52, False)] \
    + [(*s[:3], False) for s in LN_SHAPES if s[3] == 0]


def _ln_fwd(B, C, HW, want, misaligned=False, seed=21):
    c = Case(seed)
    if misaligned:      # X one element past a 16-byte boundary
        xbuf = c.t("xbuf", (B * C * HW + 4,), scale=2.0)
        x = xbuf.at(1, (B, C, HW))
    else:
        x = c.t("x", (B, C, HW), scale=2.0)
    # a distinct gamma per channel (a ramp in shuffled order would do as well: a shifted channel range must not cancel)
    g = c.t("gamma", (C,), 0.5 + 1.5 * torch.arange(C) / C)
    b = c.t("beta", (C,))
    y, mr = c.t("y", (B, C, HW), "nan"), c.t("mr", (B, HW, 2), "nan")
    bufs = _execute(c, [("CHAN_LN_FWD", dict(X=x, GAMMA=g, BETA=b, Y=y, MR=mr, B=B, C=C, HW=HW, EPS=1e-6))], want_variant=want)
    what = f"chan_ln_fwd family {want} ({B},{C},{HW})"
    _check(c, bufs, "y", 2e-5, parts=(("channel", (0, 2)),), what=what)
    _check(c, bufs, "mr", 2e-5, what=what)


@pytest.mark.parametrize("B,C,HW", LN_ROWS, ids=_shape_ids(LN_ROWS, 3))
def test_chan_ln_fwd_row_kernel(B, C, HW):
    _ln_fwd(B, C, HW, 8)


@pytest.mark.parametrize("B,C,HW,misaligned", LN_TILE, ids=_shape_ids(LN_TILE, 4))
def test_chan_ln_fwd_tile_kernel(B, C, HW, misaligned):
    _ln_fwd(B, C, HW, 0, misaligned)


LN_FWD_STRIDE = (8200, 3, 5)          # 8200 tiles on a grid of 8192


def test_chan_ln_fwd_grid_stride_second_trip():
    _ln_fwd(*LN_FWD_STRIDE, 0)


LN_BWD_STRIDE = (1030, 6, 70)         # 2060 tiles on a grid of 1024: two or three tiles per workgroup


@pytest.mark.parametrize("mode", ["accum", "dxin"])
def test_chan_ln_bwd_partials_over_several_tiles(mode):
    """The parameter and DSUM partials of a workgroup collect in LDS over all of its tiles.  dy carries a per-channel share of xhat
    and a per-channel offset, DX's accumulate source a per-channel offset: every entry of dgamma / dbeta / dsum is then a sum of
    72,100 terms that do not cancel (|entry| > 1e4, asserted), and is checked against its own value at the backward bar 1e-4."""
    B, C, HW = LN_BWD_STRIDE
    c = Case(22)
    xd = torch.randn(B, C, HW, generator=c.gen) * 2
    mean = xd.mean(1)
    rstd = torch.rsqrt(xd.var(1, unbiased=False) + 1e-5)
    xhat = (xd - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    ch = torch.arange(C).view(1, C, 1)
    sign = 1.0 - 2.0 * (ch % 2)
    x = c.t("x", (B, C, HW), xd)
    mr = c.t("mr", (B, HW, 2), torch.stack([mean, rstd], -1))
    dy = c.t("dy", (B, C, HW), torch.randn(B, C, HW, generator=c.gen) + sign * (0.3 + 0.1 * ch) * xhat - sign * (0.35 + 0.08 * ch))
    g = c.t("gamma", (C,), 0.5 + 1.5 * torch.arange(C) / C)
    src = torch.randn(B, C, HW, generator=c.gen) + sign * (1.0 + 0.2 * ch)
    dx = c.t("dx", (B, C, HW), src if mode == "accum" else "nan")
    dxin = c.t("dxin", (B, C, HW), src) if mode == "dxin" else None
    dg, db, ds = c.t("dgamma", (C,)), c.t("dbeta", (C,)), c.t("dsum", (C,))
    bufs = _execute(c, [("CHAN_LN_BWD", dict(DY=dy, X=x, MR=mr, GAMMA=g, DX=dx, DGAMMA=dg, DBETA=db, DXIN=dxin, DSUM=ds, B=B, C=C, HW=HW,
                                             ACCUM=1))])
    what = f"chan_ln_bwd {mode}"
    _check(c, bufs, "dx", 1e-4, parts=(("channel", (0, 2)),), what=what)
    for name in ("dgamma", "dbeta", "dsum"):
        assert c.read(bufs[2], name, wide=True).abs().min() > 1e4, f"{name}: an entry cancels, the per-channel check would be vacuous"
        _check(c, bufs, name, 1e-4, parts=(("channel", (1,)),), what=what, view=lambda t: t.reshape(C, 1))


# ---------------------------------------------------------------------------------------------------------------
# ATTN_FWD / ATTN_BWD
# ---------------------------------------------------------------------------------------------------------------
def _attn_ref64(qd, B, H, HD, L, scale):
    t = qd[..., :L].double().reshape(B, 3, H, HD, L).permute(1, 0, 2, 4, 3)
    s = (t[0] @ t[1].transpose(-2, -1)) * scale
    return (torch.softmax(s, -1) @ t[2]).permute(0, 1, 3, 2), torch.logsumexp(s, -1), s       # [B,H,HD,L], [B,H,L], [B,H,L,L]


def _attn(B, H, HD, L, LS, scale=None, qd=None, nan_pad=False, stress=False, chained=False, seed=23, what=""):
    """forward and backward of one case as two records of one program; the backward reads an O / log-sum-exp of its own (the
    float64 attention of the same QKV rounded to f32), so that row padding can be poisoned.  nan_pad: columns L..LS-1 of QKV, DO
    and of the backward's O and LSE hold NaN - the kernels must never read them.  chained: the backward reads the O and LSE its
    forward wrote, as every plan does."""
    c = Case(seed)
    S = LS or L
    scale = HD ** -0.5 if scale is None else scale
    if qd is None:
        qd = torch.randn(B, 3 * H * HD, S, generator=c.gen)
    dod = torch.randn(B, H * HD, S, generator=c.gen)
    od, ld, _ = _attn_ref64(qd, B, H, HD, L, scale)
    pad = NAN if nan_pad else 0.0
    o_in, l_in = torch.full((B, H, HD, S), pad), torch.full((B, H, S), pad)
    o_in[..., :L], l_in[..., :L] = od.float(), ld.float()
    if nan_pad:
        assert S > L
        qd, dod = qd.clone(), dod.clone()
        qd[..., L:] = NAN
        dod[..., L:] = NAN
    qkv = c.t("qkv", (B, 3 * H * HD, S), qd)
    o, lse = c.t("o", (B, H * HD, S), "nan"), c.t("lse", (B, H, S), "nan")
    oi, li = c.t("o_in", (B, H * HD, S), o_in), c.t("lse_in", (B, H, S), l_in)
    do = c.t("do", (B, H * HD, S), dod)
    dqkv, delta = c.t("dqkv", (B, 3 * H * HD, S), "nan"), c.t("delta", (B, H, S), "nan")
    geo = dict(B=B, HEADS=H, HD=HD, L=L, LS=LS, SCALE=scale)
    bufs = _execute(c, [("ATTN_FWD", dict(QKV=qkv, O=o, LSE=lse, **geo)),
                        ("ATTN_BWD", dict(QKV=qkv, DO=do, DQKV=dqkv, O=o if chained else oi, LSE=lse if chained else li, DELTA=delta, **geo))])
    what = f"attn {what} ({B},{H},{HD},{L},{LS}) scale {scale:.3g}{' NaN padding' if nan_pad else ''}"
    errs = {}
    errs["o"] = _check(c, bufs, "o", 1e-4, parts=(("(b,h)", (2, 3)),), what=what, view=lambda t: t.reshape(B, H, HD, S), stress=stress)
    errs["lse"] = _check(c, bufs, "lse", 1e-4, parts=(("(b,h)", (2,)),), what=what, stress=stress)
    errs["delta"] = _check(c, bufs, "delta", 1e-4, parts=(("(b,h)", (2,)),), what=what, stress=stress)
    for i, third in enumerate("qkv"):
        if L == 1 and i < 2:      # one token: dQ = dK = 0, a part without a scale of its own - held to the bar of the whole of dQKV
            ref = c.read(bufs[2], "dqkv", wide=True).reshape(B, 3, H, HD, S)
            assert (ref[:, i] == 0).all() and c.read(bufs[0], "dqkv").reshape(B, 3, H, HD, S)[:, i].abs().max() < 2e-4 * ref.abs().max()
            continue
        errs["d" + third] = _check(c, bufs, "dqkv", 2e-4, parts=(("(b,h)", (2, 3)),), what=f"{what} d{third}",
                                   view=lambda t, i=i: t.reshape(B, 3, H, HD, S)[:, i], stress=stress)
    for name in ("o", "lse", "delta", "dqkv"):        # row padding comes out as exact zeros
        assert (c.read(bufs[0], name)[..., L:] == 0).all(), f"{what}: padding columns of {name} are not zero"
    return errs


_ATTN_IDS = _shape_ids(ATTN, 5)
ATTN_PADDED = [r for r in ATTN if r[4]]


@pytest.mark.parametrize("B,H,HD,L,LS", ATTN, ids=_ATTN_IDS)
def test_attn_per_head_and_per_part(B, H, HD, L, LS):
    _attn(B, H, HD, L, LS)


@pytest.mark.parametrize("B,H,HD,L,LS", ATTN, ids=_ATTN_IDS)
def test_attn_scale_is_not_head_dim_rsqrt(B, H, HD, L, LS):
    """with SCALE = HD^-0.5 a scale applied in the wrong place can cancel against the reference's own; 0.37 is no power of any HD"""
    _attn(B, H, HD, L, LS, scale=0.37, seed=24)


@pytest.mark.parametrize("B,H,HD,L,LS", ATTN_PADDED, ids=_shape_ids(ATTN_PADDED, 5))
def test_attn_never_reads_row_padding(B, H, HD, L, LS):
    _attn(B, H, HD, L, LS, nan_pad=True, seed=25)


ATTN_STRESS = [(1, 2, 64, 197, 200), (1, 2, 32, 70, 72)]


def _stress_qkv(kind, B, H, HD, L, S, gen):
    """(a) 'large': q and k scaled by 4, scores ~ 16 N(0,1).  (b) 'last': every query's largest score is at key L - 1, in the ragged
    last key tile.  (c) 'rising' / (d) 'falling': scores strictly monotonic in the key index by 0.5 per key, so the running
    maximum rises on every key tile (the accumulator is rescaled every time) or never after the first.
    (b)-(d): every q gets the SAME component 4 along the unit direction u = 1/sqrt(HD) and key j the component r_j along u; the
    parts orthogonal to u are 0.2 N(0,1), so score[i][j] = HD^-0.5 (q_i' k_j' + 4 r_j) with |HD^-0.5 q' k'| < 0.25."""
    qkv = torch.randn(B, 3, H, HD, S, generator=gen)
    if kind == "large":
        qkv[:, :2] *= 4.0
        return qkv.reshape(B, 3 * H * HD, S)
    u = torch.full((HD,), HD ** -0.5).view(1, 1, 1, HD, 1)
    qk = qkv[:, :2] * 0.2
    qk = qk - (qk * u).sum(3, keepdim=True) * u
    j = torch.arange(S, dtype=torch.float32)
    want = {"last": 3.0 * (j == L - 1), "rising": 0.5 * j, "falling": 0.5 * (L - 1 - j)}[kind]       # score share of key j
    r = want / (HD ** -0.5 * 4.0)
    qkv[:, 0] = qk[:, 0] + 4.0 * u
    qkv[:, 1] = qk[:, 1] + r.view(1, 1, 1, S) * u
    return qkv.reshape(B, 3 * H * HD, S)


@pytest.mark.parametrize("kind", ["large", "last", "rising", "falling"])
@pytest.mark.parametrize("B,H,HD,L,LS", ATTN_STRESS, ids=_shape_ids(ATTN_STRESS, 5))
def test_attn_online_softmax_under_stress(B, H, HD, L, LS, kind):
    """Bars: max(the attention bar, 8 E) per figure (see _check).  On the CPU E is 5e-6..9e-6 for 'large' inputs and <= 7e-7 for
    plain ones, so the attention bars are not expected to move.

    The backward reads the O and log-sum-exp its own forward wrote, as in every plan.  With scores near 100 an f32 score carries
    ~1e-5 of absolute rounding; the backward recomputes the scores in the forward's own order, so exp(s - lse) still sums to 1 over
    a row and sum_j dS[i][j] = 0 holds to rounding.  Handing it the log-sum-exp of a float64 forward instead breaks that by the
    ~1e-5, and dQ = dS K multiplies the residue by the key component all keys share (up to 196 here): measured on an MI355X,
    dQ 6.6e-4 / 7.9e-4 of its max at (1, 2, 64, 197, 200) falling / rising, every other part <= 7e-5 - a property of the
    inconsistent input, which no plan produces, not of the kernel."""
    gen = torch.Generator().manual_seed(26)
    qd = _stress_qkv(kind, B, H, HD, L, LS, gen)
    s = _attn_ref64(qd, B, H, HD, L, HD ** -0.5)[2]
    if kind == "large":
        assert s.abs().max() > 50, f"max |score| {s.abs().max():.1f}"
    elif kind == "last":
        assert (s.argmax(-1) == L - 1).all()
    elif kind == "rising":
        assert (s.diff(dim=-1) > 0).all() and s.max() - s.min() > 0.45 * (L - 1)
    else:
        assert (s.diff(dim=-1) < 0).all() and s.max() - s.min() > 0.45 * (L - 1)
    _attn(B, H, HD, L, LS, qd=qd, stress=True, chained=True, seed=27, what=kind)


# ---------------------------------------------------------------------------------------------------------------
# MAE_LOSS_FWD / MAE_LOSS_BWD
# ---------------------------------------------------------------------------------------------------------------
# (B, C, T, H, P, TUB, LP, L_OFF, IMGS off by one element, family)
MAE = [(2, 3, 1, 16, 2, 1, 65, 1, False, 9),        # P = 2: scalar kernel
       (2, 2, 4, 24, 6, 2, 33, 1, False, 9),        # P = 6, two frames per patch
       (2, 3, 1, 16, 4, 1, 17, 1, True, 9),         # P = 4 but the images are not 16-byte aligned
       (2, 2, 1, 64, 4, 1, 260, 1, False, 0),       # float4 kernel: two column workgroups, a padded tail behind the 256 patches
       (2, 2, 1, 64, 4, 1, 256, 0, False, 0)]       # no cls column: L_OFF = 0 and LP = L


@pytest.mark.parametrize("norm_pix", [0, 1])
@pytest.mark.parametrize("B,C,T,H,P,TUB,LP,L_OFF,misaligned,want", MAE, ids=_shape_ids(MAE, 9))
def test_mae_loss_kernels_and_options(B, C, T, H, P, TUB, LP, L_OFF, misaligned, want, norm_pix):
    """forward, then the backward on the ACC the forward left.  ACC holds garbage before the forward (which must clear it itself);
    sample 0 has no masked patch; every other case passes GOUT = None (an upstream gradient of 1)."""
    c = Case(28 + norm_pix)
    L = (T // TUB) * (H // P) ** 2
    PD = TUB * P * P * C
    assert LP >= L + L_OFF
    pred = c.t("pred", (B, PD, LP))
    n = B * C * T * H * H
    if misaligned:
        xbuf = c.t("imgbuf", (n + 4,))
        x = xbuf.at(1, (B, C, T, H, H))
    else:
        x = c.t("imgs", (B, C, T, H, H))
    mk = (torch.rand(B, L, generator=c.gen) < 0.75).float()
    mk[0] = 0.0
    mk[1, 0], mk[1, L - 1] = 1.0, 1.0
    mask = c.t("mask", (B, L), mk)
    loss = c.t("loss", (1,), "nan")
    acc = c.t("acc", (2,), torch.tensor([123.0, -7.0], dtype=torch.float64), "f64")
    with_gout = (MAE.index((B, C, T, H, P, TUB, LP, L_OFF, misaligned, want)) + norm_pix) % 2 == 0
    gout = c.t("gout", (1,), torch.tensor([0.7])) if with_gout else None
    dpred = c.t("dpred", (B, PD, LP), "nan")
    geo = dict(B=B, C=C, T=T, H=H, W=H, P=P, TUB=TUB, LP=LP, L_OFF=L_OFF, NORM_PIX=norm_pix)
    bufs = _execute(c, [("MAE_LOSS_FWD", dict(PRED=pred, IMGS=x, MASK=mask, LOSS=loss, ACC=acc, **geo)),
                        ("MAE_LOSS_BWD", dict(PRED=pred, IMGS=x, MASK=mask, ACC=acc, GOUT=gout, DPRED=dpred, **geo))], want_variant=[want, want])
    what = f"mae_loss family {want} P {P} LP {LP} L_OFF {L_OFF} norm_pix {norm_pix} gout {with_gout}"
    _check(c, bufs, "loss", 2e-5, what=what)
    _check(c, bufs, "acc", 2e-5, parts=(("entry", (1,)),), what=what, view=lambda t: t.reshape(2, 1))
    _check(c, bufs, "dpred", 2e-5, parts=(("feature row", (0, 2)),), what=what)
    got = c.read(bufs[0], "dpred")
    live = torch.zeros(B, LP, dtype=torch.bool)
    live[:, L_OFF:L_OFF + L] = mk > 0
    assert (got.permute(0, 2, 1)[~live] == 0).all(), "DPRED is not exactly 0 in padding columns / unmasked patches"
    assert (got.permute(0, 2, 1)[live].abs().amax(1) > 0).all()


# ---------------------------------------------------------------------------------------------------------------
# PATCHIFY
# ---------------------------------------------------------------------------------------------------------------
PATCH_GEO = [(2, 3, 3, 32, 8, 1), (1, 2, 4, 16, 4, 2)]          # (B, C, T, H, P, TUB)
GUARD = 64


def _patch_case(c, B, C, T, H, P, TUB, x_fill, out_fill):
    """X inside a NaN guard band, OUT with row stride L + 4 and the patches from column 1 (as the plans pass them); the columns
    of OUT the op does not own hold NaN"""
    L = (T // TUB) * (H // P) ** 2
    PD = C * TUB * P * P
    n = B * C * T * H * H
    xb = torch.full((n + 2 * GUARD,), NAN)
    if x_fill is not None:
        xb[GUARD:GUARD + n] = x_fill.reshape(-1)
    xbuf = c.t("xbuf", (n + 2 * GUARD,), xb)
    ob = torch.full((B, PD, L + 4), NAN)
    if out_fill is not None:
        ob[:, :, 1:1 + L] = out_fill
    out = c.t("out", (B, PD, L + 4), ob)
    return xbuf.at(GUARD, (B, C, T, H, H)), out, L, PD, dict(B=B, C=C, T=T, H=H, W=H, P=P, TUB=TUB, LS=L + 4, L_OFF=1)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("inverse", [0, 1, 2, 3])
@pytest.mark.parametrize("B,C,T,H,P,TUB", PATCH_GEO)
def test_patchify_modes_orders_and_strides(B, C, T, H, P, TUB, inverse, order):
    c = Case(30)
    L, PD = (T // TUB) * (H // P) ** 2, C * TUB * P * P
    xf = torch.randn(B, C, T, H, H, generator=c.gen) if inverse in (0, 3) else None          # INVERSE 3 adds to a pre-filled X
    of = torch.randn(B, PD, L, generator=c.gen) if inverse else None
    x, out, L, PD, geo = _patch_case(c, B, C, T, H, P, TUB, xf, of)
    bufs = _execute(c, [("PATCHIFY", dict(X=x, OUT=out, INVERSE=inverse, ORDER=order, **geo))])
    what = f"patchify inverse {inverse} order {order}"
    xg = _check_exact(c, bufs, "xbuf", what, rounded=inverse == 3)
    og = _check_exact(c, bufs, "out", what)
    n = B * C * T * H * H
    assert torch.isnan(xg[:GUARD]).all() and torch.isnan(xg[GUARD + n:]).all() and torch.isfinite(xg[GUARD:GUARD + n]).all()
    assert torch.isnan(og[:, :, 0]).all() and torch.isnan(og[:, :, 1 + L:]).all() and torch.isfinite(og[:, :, 1:1 + L]).all()


@pytest.mark.parametrize("B,C,T,H,P,TUB", PATCH_GEO + [(2, 3, 1, 8, 2, 1)])       # the last: PD = 12, no multiple of the 64 lanes
def test_patchify_gradient_through_the_standardised_target(B, C, T, H, P, TUB):
    """INVERSE 4 (patch_norm_target_grad_kernel): DX against the float64 oracle at 2e-5 of its max, whole and per patch"""
    c = Case(31)
    L, PD = (T // TUB) * (H // P) ** 2, C * TUB * P * P
    x, out, L, PD, geo = _patch_case(c, B, C, T, H, P, TUB, None, torch.randn(B, PD, L, generator=c.gen))
    imgs = c.t("imgs", (B, C, T, H, H), scale=2.0)
    bufs = _execute(c, [("PATCHIFY", dict(X=x, OUT=out, IMGS=imgs, INVERSE=4, ORDER=1, **geo))])
    n = B * C * T * H * H
    cols = lambda t: ops_ref._patch_cols(t[GUARD:GUARD + n].reshape(B, C, T, H, H), P, TUB, "mae")      # noqa: E731  [B, PD, L]
    _check(c, bufs, "xbuf", 2e-5, parts=(("patch", (1,)),), what=f"patchify inverse 4 PD {PD}", view=cols)
    xg = c.read(bufs[0], "xbuf")
    assert torch.isnan(xg[:GUARD]).all() and torch.isnan(xg[GUARD + n:]).all()
    _check_exact(c, bufs, "out", "patchify inverse 4 (OUT is read only)")


PATCH_STRIDE = (3, 6, 1, 512, 16, 1)        # 4,718,592 elements on a grid of 16384 x 256


def test_patchify_grid_stride_second_trip():
    B, C, T, H, P, TUB = PATCH_STRIDE
    c = Case(32)
    L, PD = (T // TUB) * (H // P) ** 2, C * TUB * P * P
    x = c.t("x", (B, C, T, H, H))
    out = c.t("out", (B, PD, L), "nan")
    bufs = _execute(c, [("PATCHIFY", dict(X=x, OUT=out, B=B, C=C, T=T, H=H, W=H, P=P, TUB=TUB))])
    assert torch.isfinite(_check_exact(c, bufs, "out", "patchify grid-stride")).all()


# ---------------------------------------------------------------------------------------------------------------
# TRANSPOSE_CL with an output row stride and column offset
# ---------------------------------------------------------------------------------------------------------------
# (B, C, L, L_OFF, LOUT, YS, Y_OFF): the plans pass (Y_OFF 1, YS = C + 4) and (Y_OFF 0, YS = C + 3); C and LOUT on both sides of 64
TRANSPOSE = [(2, 50, 70, 0, 70, 54, 1), (2, 100, 40, 0, 40, 103, 0), (1, 64, 64, 0, 64, 68, 1), (2, 63, 66, 1, 65, 66, 0),
             (1, 65, 63, 0, 63, 69, 1), (1, 60, 30, 0, 30, 61, 1), (1, 130, 5, 0, 5, 133, 0)]        # (60, .., 61, 1): Y_OFF + C = YS


@pytest.mark.parametrize("B,C,L,off,Lout,YS,Y_OFF", TRANSPOSE)
def test_transpose_cl_into_strided_rows(B, C, L, off, Lout, YS, Y_OFF):
    c = Case(33)
    x = c.t("x", (B, C, L))
    y = c.t("y", (B, Lout, YS), "nan")
    bufs = _execute(c, [("TRANSPOSE_CL", dict(X=x, Y=y, B=B, C=C, L=L, L_OFF=off, LOUT=Lout, YS=YS, Y_OFF=Y_OFF))])
    got = _check_exact(c, bufs, "y", "transpose_cl")
    assert (got[:, :, :Y_OFF] == 0).all() and (got[:, :, Y_OFF + C:] == 0).all()
    assert torch.equal(got[:, :, Y_OFF:Y_OFF + C], c.items["x"][1][:, :, off:off + Lout].permute(0, 2, 1))


# ---------------------------------------------------------------------------------------------------------------
# IDS_TO_DEC_IDX
# ---------------------------------------------------------------------------------------------------------------
IDS = [(3, 196, 49, "perm"), (2, 50, 20, "wild"), (2, 33, 0, "perm"), (2, 33, 33, "perm"), (1100, 1000, 250, "perm")]    # the last: 1,101,100 > 4096 x 256


@pytest.mark.parametrize("B,L,keep,kind", IDS)
def test_ids_to_dec_idx_exact(B, L, keep, kind):
    c = Case(34)
    if kind == "perm":
        v = torch.rand(B, L, generator=c.gen).argsort(1)
    else:       # values >= keep, >= L and negative ones
        v = torch.randint(-5, L + 6, (B, L), generator=c.gen)
        v[0, 0], v[0, 1], v[1, 0] = -1, keep, keep - 1
    ids = c.t("ids", (B, L), v, "i64")
    dec = c.t("dec", (B, 1 + L), torch.full((B, 1 + L), -9), "i32")
    bufs = _execute(c, [("IDS_TO_DEC_IDX", dict(IDS=ids, DEC_IDX=dec, B=B, L=L, KEEP=keep))])
    got = _check_exact(c, bufs, "dec", "ids_to_dec_idx")
    assert (got[:, 0] == 0).all() and ((got[:, 1:] >= 1) == ((v >= 0) & (v < keep))).all()


# ---------------------------------------------------------------------------------------------------------------
# TOKEN_GATHER / TOKEN_SCATTER
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LinS,LoutS", [(0, 0), (32, 28)])
def test_token_gather_without_fill_and_pos(LinS, LoutS):
    """FILL = None and POS = None, no -1 index: the plain gathers of the plans' method paths"""
    c = Case(35)
    B, C, Lin, Lout = 3, 40, 30, 23
    src = c.t("in", (B, C, LinS or Lin))
    idx = c.t("idx", (B, Lout), torch.stack([torch.randperm(Lin, generator=c.gen)[:Lout] for _ in range(B)]), "i32")
    out = c.t("out", (B, C, LoutS or Lout), "nan")
    bufs = _execute(c, [("TOKEN_GATHER", dict(IN=src, IDX=idx, FILL=None, POS=None, OUT=out, B=B, C=C, LIN=Lin, LOUT=Lout, POS_BY_SRC=0,
                                              POS_OFF=0, LIN_S=LinS, LOUT_S=LoutS))])
    got = _check_exact(c, bufs, "out", "token_gather")
    assert (got[..., Lout:] == 0).all()


def test_token_gather_without_fill_takes_zero_for_a_negative_index():
    """FILL = None with a -1 index: plan_random_masking gathers through ENC_IDX, whose column 0 is the absent cls slot.  The stage
    writes 0 there (opdefs.py, TOKEN_GATHER); the emulator used to copy token 0 instead (found by tests/test_vit_stages_gpu.py)."""
    c = Case(38)
    B, C, Lin, Lout = 2, 12, 16, 9
    src = c.t("in", (B, C, Lin))
    idxv = torch.stack([torch.randperm(Lin, generator=c.gen)[:Lout] for _ in range(B)])
    idxv[:, 0] = -1
    idxv[1, 5] = -1
    idx = c.t("idx", (B, Lout), idxv, "i32")
    out = c.t("out", (B, C, Lout), "nan")
    bufs = _execute(c, [("TOKEN_GATHER", dict(IN=src, IDX=idx, FILL=None, POS=None, OUT=out, B=B, C=C, LIN=Lin, LOUT=Lout, POS_BY_SRC=0,
                                              POS_OFF=0, LIN_S=0, LOUT_S=0))])
    got = _check_exact(c, bufs, "out", "token_gather without fill")
    assert (got[:, :, 0] == 0).all() and (got[1, :, 5] == 0).all() and (got[0, :, 1:] != 0).all()


GATHER_STRIDE = (3, 700, 1100, 1001)        # 2,102,100 output elements on a grid of 8192 x 256
SCATTER_STRIDE = (5, 3300, 9, 7)            # 16,500 rows on a grid of 4096 x 4 rows


def test_token_gather_grid_stride_second_trip():
    B, C, Lin, Lout = GATHER_STRIDE
    c = Case(36)
    src = c.t("in", (B, C, Lin))
    idxv = torch.stack([torch.randperm(Lin, generator=c.gen)[:Lout] for _ in range(B)])
    idxv[:, 0] = -1
    idxv[2, Lout - 1] = -1
    idx = c.t("idx", (B, Lout), idxv, "i32")
    fill, pos = c.t("fill", (C,)), c.t("pos", (Lout, C))
    out = c.t("out", (B, C, Lout), "nan")
    bufs = _execute(c, [("TOKEN_GATHER", dict(IN=src, IDX=idx, FILL=fill, POS=pos, OUT=out, B=B, C=C, LIN=Lin, LOUT=Lout, POS_BY_SRC=0,
                                              POS_OFF=0, LIN_S=0, LOUT_S=0))])
    _check(c, bufs, "out", 1e-6, parts=(("sample", (1, 2)), ("token", (0, 1))), what="token_gather grid-stride")


def test_token_scatter_grid_stride_second_trip():
    """DFILL per channel: each entry is its start value plus the <= 10 gradient values of the tokens that came from the fill
    token, summed in f32 in an order of the kernel's own; the error of such a sum is bounded by (terms) 2^-24 sum |term|, so every
    channel is held to the scatter bar 1e-5 of ITS sum of |terms|"""
    B, C, Lin, Lout = SCATTER_STRIDE
    c = Case(37)
    doutd = torch.randn(B, C, Lout, generator=c.gen)
    dout = c.t("dout", (B, C, Lout), doutd)
    idxv = torch.stack([torch.randperm(Lin, generator=c.gen)[:Lout] for _ in range(B)])
    idxv[:, 0] = -1
    idxv[3, 4] = -1
    idx = c.t("idx", (B, Lout), idxv, "i32")
    din = c.t("din", (B, C, Lin), "nan")
    df0 = torch.randn(C, generator=c.gen)
    dfill = c.t("dfill", (C,), df0)
    bufs = _execute(c, [("TOKEN_SCATTER", dict(DOUT=dout, IDX=idx, DIN=din, DFILL=dfill, B=B, C=C, LIN=Lin, LOUT=Lout, LIN_S=0, LOUT_S=0))])
    _check_exact(c, bufs, "din", "token_scatter grid-stride")
    _check(c, bufs, "dfill", 1e-5, what="token_scatter grid-stride")
    terms = df0.double().abs() + (doutd.double().abs() * (idxv < 0).unsqueeze(1)).sum((0, 2))
    got = c.read(bufs[0], "dfill").double()
    for ref, wide in ((bufs[1], False), (bufs[2], True)):
        e = ((got - c.read(ref, "dfill", wide).double()).abs() / terms).max().item()
        print(f"token_scatter dfill per channel: {e:.2e} of the channel's sum of |terms| ({'float64' if wide else 'f32 oracle'})")
        assert e < 1e-5


# ---------------------------------------------------------------------------------------------------------------
# ACT_FWD / ACT_BWD
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [D.ACT_SILU, D.ACT_GELU, D.ACT_RELU])
@pytest.mark.parametrize("HW", [50, 64])
def test_act_fwd_affine_without_gate(HW, act):
    """BNV without GATE: the generic kernel's per-channel affine branch, at a plane size that is and is not a multiple of 4"""
    c = Case(38)
    B, C = 3, 7
    x, y = c.t("x", (B, C, HW), scale=2.0), c.t("y", (B, C, HW), "nan")
    bnv = c.bnv("bnv", C)
    bufs = _execute(c, [("ACT_FWD", dict(X=x, Y=y, BNV=bnv, GATE=None, COUNT=B * C * HW, ACT=act, C=C, HW=HW))])
    _check(c, bufs, "y", 1e-5, parts=(("channel", (0, 2)),), what=f"act_fwd affine act {act} HW {HW}")


ACT_STRIDE = 8192 * 256 + 4099


def _act_input(c, n):
    """N(0, 2^2) values, and at both ends of the buffer (the first and the second trip) a sweep over [-30, 30]"""
    v = torch.randn(n, generator=c.gen) * 2.0
    sweep = torch.linspace(-30.0, 30.0, 2001)
    v[:2001] = sweep
    v[n - 2001:] = sweep.flip(0)
    return v


@pytest.mark.parametrize("act", [D.ACT_GELU, D.ACT_SILU, D.ACT_RELU])
def test_act_fwd_grid_stride_and_wide_inputs(act):
    c = Case(39)
    n = ACT_STRIDE
    x, y = c.t("x", (n,), _act_input(c, n)), c.t("y", (n,), "nan")
    bufs = _execute(c, [("ACT_FWD", dict(X=x, Y=y, COUNT=n, ACT=act))])
    # whole, and the second trip on its own (elements from 8192 x 256 on)
    _check(c, bufs, "y", 1e-5, what=f"act_fwd act {act}")
    _check(c, bufs, "y", 1e-5, what=f"act_fwd act {act} second trip", view=lambda t: t[8192 * 256:])
    # |x| <= 5 on its own: a relative-to-max bar of the whole tensor is set by y(30) = 30
    small = c.items["x"][1].abs() <= 5.0
    _check(c, bufs, "y", 1e-5, what=f"act_fwd act {act} |x| <= 5", view=lambda t: t[small])


@pytest.mark.parametrize("act", [D.ACT_GELU, D.ACT_SILU, D.ACT_RELU])
def test_act_bwd_grid_stride_and_wide_inputs(act):
    c = Case(40)
    n = ACT_STRIDE
    g, x = c.t("g", (n,)), c.t("x", (n,), _act_input(c, n))
    bufs = _execute(c, [("ACT_BWD", dict(G=g, X=x, COUNT=n, ACT=act))])
    _check(c, bufs, "g", 1e-5, what=f"act_bwd act {act}")
    _check(c, bufs, "g", 1e-5, what=f"act_bwd act {act} second trip", view=lambda t: t[8192 * 256:])


# ---------------------------------------------------------------------------------------------------------------
# MAE_MASK_INDEX
# ---------------------------------------------------------------------------------------------------------------
MASK_INDEX = [(1, 12288, 3072, 0), (2, 600, 150, 8)]       # (B, L, keep, noise levels; 0 = continuous): the limit L; heavy ties


@pytest.mark.parametrize("B,L,keep,levels", MASK_INDEX)
def test_mae_mask_index_at_its_limit_and_with_heavy_ties(B, L, keep, levels):
    c = Case(41)
    nz = torch.rand(B, L, generator=c.gen)
    if levels:
        nz = (nz * levels).floor() / levels
    noise = c.t("noise", (B, L), nz)
    ids = c.t("ids", (B, L), torch.full((B, L), -7), "i64")
    mask = c.t("mask", (B, L), "nan")
    enc = c.t("enc", (B, 1 + keep), torch.full((B, 1 + keep), -9), "i32")
    dec = c.t("dec", (B, 1 + L), torch.full((B, 1 + L), -9), "i32")
    bufs = _execute(c, [("MAE_MASK_INDEX", dict(NOISE=noise, IDS_RESTORE=ids, MASK=mask, ENC_IDX=enc, DEC_IDX=dec, B=B, L=L, KEEP=keep))])
    for name in ("ids", "mask", "enc", "dec"):
        _check_exact(c, bufs, name, f"mae_mask_index L {L}")
    got = c.read(bufs[0], "ids")
    assert torch.equal(got.sort(1).values, torch.arange(L).expand(B, L))          # a permutation of 0..L-1
    assert c.read(bufs[0], "mask").sum().item() == B * (L - keep)
