"""The layout reference of tests/pack_ref.py against itself and the oracle, and the planners' real WEIGHT_PACK / WGRAD_FINALIZE /
AXPY tables against what the kernels of csrc/ew.hip silently rely on.  No GPU: tests/test_pack_kernels_gpu.py compares the same
reference with the kernels, byte for byte."""
import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import detgen, ops_ref
from oracle import efficientnet_unet_ref as R
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan import vit_plan as V
from s2lc_amd.plan.program import TRef
from s2lc_amd.plan.unet_plan import plan_unet
from tests import pack_ref as PR
from tests.helpers import mae_inputs, seg_inputs

WS = D.BASE["WS"]


def _distinct(n, seed):
    """n distinct, exactly representable, non-zero floats in a seeded order"""
    v = np.arange(1, n + 1, dtype=np.float32) * np.float32(0.25)
    return v[np.random.default_rng(seed).permutation(n)]


def _spread(n, seed):
    """2^-20 .. 2^20, random signs, all 23 stored significand bits random (tests/test_b16_kernels_gpu.spread)"""
    g = np.random.default_rng(seed)
    return (g.choice([-1.0, 1.0], n) * (1.0 + g.random(n)) * 2.0 ** g.integers(-20, 21, n)).astype(np.float32)


# ---- the reference against itself and the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,M,K,T", PR.SINGLE_ROWS, ids=["-".join(str(v) for v in r) for r in PR.SINGLE_ROWS])
def test_f32_pack_equals_the_oracle_and_the_mirrors_decode_to_it(pattern, M, K, T):
    n_src, entry = PR.pattern_row(pattern, M, K, T)
    src = _distinct(n_src, M + K + T)
    entry[7] |= 2 if T == 1 else 0
    rows, total = PR.table_rows([entry], [64 * ((n_src + 63) // 64) + 64])
    row = rows[0]
    MP, KP, dst_off = row[9], row[10], row[1]
    # one image: SRC at float 0, the pack at float dst_off (NaN-filled), the table behind it
    image = np.full(dst_off + total + 64, np.nan, dtype=np.float32)
    image[:n_src] = src
    mine = PR.apply(image.copy().view(np.uint8), 0, PR.f32_pack(rows, image))
    theirs = torch.from_numpy(np.concatenate([image, np.array(row + [0] * 4, dtype=np.int32).view(np.float32)]).view(np.uint8).copy())
    ops_ref.op_weight_pack(ops_ref.Mem({WS: theirs}), dict(TABLE=(WS << 56) | 4 * image.size, N_ENTRIES=1, SRC=WS << 56, DST=WS << 56))
    assert np.array_equal(mine, theirs.numpy()[:mine.size]), "f32_pack and ops_ref.op_weight_pack disagree"

    pack = mine.view(np.uint32)[dst_off:dst_off + total].reshape(KP, T, MP)
    assert not pack[K:].any() and not pack[:, :, M:].any()                      # padding is +0.0, bit for bit
    assert np.array_equal(np.sort(pack[:K, :, :M].reshape(-1).view(np.float32)),
                          np.sort(PR.logical_weight(row, image).reshape(-1).view(np.float32)))
    assert np.unique(pack[:K, :, :M]).size == K * T * M                         # distinct values: nothing copied twice
    # quad copy -> the pack exactly
    q = PR.q4_mirror(rows, image, 1 << 20)
    if T == 1:
        (addr, b), = q
        assert addr == (1 << 20) + 4 * dst_off
        assert np.array_equal(PR.q4_decode(b.view(np.uint32), KP, MP), pack[:, 0, :])
    else:
        assert q == []
    # bf16 copy -> the pack rounded
    (addr, b), = PR.bf16_mirror(rows, image, 1 << 20)
    assert addr == (1 << 20) + 2 * dst_off
    back = b.view(np.uint16).reshape(KP // 8, T, MP, 8).transpose(0, 3, 1, 2).reshape(KP, T, MP)
    assert np.array_equal(back, PR.bf16_bits_torch(pack.view(np.float32)))
    # the three planes lie one behind the other at 6 bytes per f32 element
    planes = PR.split_mirror(rows, image, 1 << 20)
    assert [a for a, _ in planes] == [(1 << 20) + 6 * dst_off + p * 2 * total for p in range(3)]
    assert np.array_equal(planes[0][1], b)                                       # hi is the bf16 copy


def test_split_planes_sum_to_the_pack():
    """hi + mid + lo, summed in f32, give back every finite value of 2^-20 .. 2^20 exactly"""
    M, K = 130, 65
    n_src, entry = PR.pattern_row("dense_fwd", M, K, 1)
    src = _spread(n_src, 3)
    rows, total = PR.table_rows([entry], [0])
    pack = PR.padded(rows[0], src).view(np.float32)
    hi, mid, lo = (PR.bf16_value(b.view(np.uint16)) for _, b in PR.split_mirror(rows, src, 0))
    s = ((hi + mid).astype(np.float32) + lo).astype(np.float32)
    frag = pack.reshape(rows[0][10] // 8, 8, 1, rows[0][9]).transpose(0, 2, 3, 1).reshape(-1)
    assert np.array_equal(s.view(np.uint32), frag.view(np.uint32))
    assert (mid != 0).any() and (lo != 0).any()


def test_the_two_bf16_roundings_agree():
    v = PR.tie_vector()
    u = v.view(np.uint32)
    a, b = PR.bf16_bits_int(v), PR.bf16_bits_torch(v)
    assert np.array_equal(a, b)
    at = {int(p): int(r) for p, r in zip(u, a)}
    assert at[0x3f808000] == 0x3f80 and at[0x3f818000] == 0x3f82             # ties: to the even neighbour, down and up
    assert at[0x3f807fff] == 0x3f80 and at[0x3f808001] == 0x3f81             # one ulp either side of a tie
    assert at[0x3f817fff] == 0x3f81 and at[0x3f818001] == 0x3f82
    assert at[0x3fff8000] == 0x4000                                           # the carry moves into the exponent
    assert at[0x00000000] == 0x0000 and at[0x80000000] == 0x8000
    assert at[0x7f800000] == 0x7f80 and at[0xff800000] == 0xff80
    assert at[0x7f7fffff] == 0x7f80 and at[0xff7fffff] == 0xff80             # the largest finite f32 rounds to Inf
    wide = np.concatenate([_spread(100000, 1), np.random.default_rng(2).standard_normal(100000).astype(np.float32)])
    assert np.array_equal(PR.bf16_bits_int(wide), PR.bf16_bits_torch(wide))
    # f32-split: a non-finite hi keeps mid = lo = +0
    hi, mid, lo = PR.split_terms(v)
    nf = ~np.isfinite(PR.bf16_value(hi))
    assert nf.sum() == 5 and not mid[nf].any() and not lo[nf].any()         # +-Inf, +-0x7f7fffff and the tie 0x7f7f8000
    for x, y in zip((hi, mid, lo), PR.split_terms(v, PR.bf16_bits_torch)):
        assert np.array_equal(x, y)


def test_wgrad_fold_equals_the_oracle():
    g = np.random.default_rng(4)
    rows, start = [], 0
    for off, M, C, T in [(640, 7, 5, 9), (0, 3, 11, 4), (1500, 9, 3, 1), (2000, 5, 7, 25)]:
        rows.append([off, M, C, T, start])
        start += M * C * T
    wgs, grads = g.standard_normal(3000).astype(np.float32), g.standard_normal(3000).astype(np.float32)
    mine = PR.wgrad_fold(rows, wgs, grads)
    image = torch.from_numpy(np.concatenate([wgs, grads, np.array(rows, dtype=np.int32).reshape(-1).view(np.float32)]).view(np.uint8).copy())
    ops_ref.op_wgrad_finalize(ops_ref.Mem({WS: image}), dict(TABLE=(WS << 56) | 24000, N_ENTRIES=len(rows), WGS=WS << 56, GRADS=(WS << 56) | 12000))
    assert np.array_equal(mine.view(np.uint32), image.numpy().view(np.uint32)[3000:6000])
    touched = np.zeros(3000, dtype=bool)
    for off, M, C, T, _ in rows:
        touched[off:off + M * C * T] = True
    assert np.array_equal(mine[~touched], grads[~touched]) and (mine[touched] != grads[touched]).all()


def test_space_to_depth_and_im2col_equal_the_oracle():
    g = np.random.default_rng(5)
    x = g.standard_normal((2, 3, 6, 10)).astype(np.float32)
    y = torch.full((2 * 12 * 3 * 5,), float("nan"))
    image = torch.cat([torch.from_numpy(x).reshape(-1), y]).view(torch.uint8)
    ops_ref.op_space_to_depth(ops_ref.Mem({WS: image}), dict(X=WS << 56, Y=(WS << 56) | 4 * x.size, B=2, C=3, H=3, W=5))
    assert np.array_equal(PR.space_to_depth(x).reshape(-1), image.view(torch.float32).numpy()[x.size:])
    for (H, W, k, s, pt, pl, HO, WO) in [(7, 9, 3, 2, 0, 0, 4, 5), (6, 6, 3, 1, 1, 1, 6, 6), (9, 7, 5, 1, 2, 2, 9, 7), (8, 11, 3, 3, 0, 0, 3, 4)]:
        x = g.standard_normal((2, 3, H, W)).astype(np.float32)
        n = 2 * 3 * k * k * HO * WO
        image = torch.cat([torch.from_numpy(x).reshape(-1), torch.full((n,), float("nan"))]).view(torch.uint8)
        ops_ref.op_im2col(ops_ref.Mem({WS: image}), dict(X=WS << 56, Y=(WS << 56) | 4 * x.size, B=2, C=3, H=H, W=W, KH=k, KW=k, STRIDE=s,
                                                         PAD_T=pt, PAD_L=pl, HO=HO, WO=WO))
        assert np.array_equal(PR.im2col(x, k, k, s, pt, pl, HO, WO).reshape(-1).view(np.uint32),
                              image.view(torch.float32).numpy()[x.size:].view(np.uint32))


# ---- the planners' real tables --------------------------------------------------------------------------------------------------------
def _mae_spec(cfg, decoder=True):
    return V.MaeSpec(cfg.img_size, cfg.patch_size, cfg.num_frames, cfg.tubelet_size, cfg.in_chans, cfg.embed_dim, cfg.depth,
                     cfg.num_heads, cfg.decoder_embed_dim, cfg.decoder_depth, cfg.decoder_num_heads, cfg.mlp_ratio,
                     cfg.norm_pix_loss, decoder)


def _unet_model():
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet

    return EfficientnetUnet(EfficientNetConfig("b0", 4, 4, class_distribution=[0.25] * 4))


_PLANS = {}


def _plan(model, precision):
    """U-Net b0 (4 channels, 64 x 64, batch 2), and the smallest Prithvi MAE / segmentation plans of tests/test_vit_plan_cpu.py"""
    key = (model, precision)
    if key not in _PLANS:
        kw = dict(bf16=precision == "bf16-mixed", split=precision == "f32-split")
        if model in ("unet", "unet256"):       # (256 x 256: the smallest b0 plan whose f32 form has quad rows)
            m = _unet_model()
            hw = 64 if model == "unet" else 256
            _PLANS[key] = plan_unet(m.spec, 2, hw, hw, True, m._layout, **kw)
        elif model == "mae":
            cfg, sd, x, noise, ratio = mae_inputs("small_bs2")
            _PLANS[key] = V.plan_mae(_mae_spec(cfg), x.shape[0], ratio, True, **kw)
        else:
            cfg, sd, x, y, noise, drop_u, train = seg_inputs("small_train_unfrozen")
            spec = V.SegSpec(_mae_spec(cfg.mae, decoder=False), cfg.num_classes, cfg.fcn_out_channels, cfg.fcn_num_convs, cfg.fcn_dropout,
                             cfg.frozen_backbone)
            _PLANS[key] = V.plan_seg(spec, x.shape[0], train, **kw)
    return _PLANS[key]


PLAN_IDS = [(m, p) for m in ("unet", "mae", "seg") for p in ("f32", "bf16-mixed", "f32-split")] + [("unet256", "f32"), ("unet256", "f32-split")]


def _table(plan, ref: TRef, width):
    assert ref.base == D.BASE["CONST"] and ref.off % 4 == 0
    n = ref.shape[0]
    words = plan.const_table[ref.off // 4:ref.off // 4 + n * width]
    assert len(words) == n * width
    return [list(words[i * width:(i + 1) * width]) for i in range(n)]


def _ops(plan):
    return list(plan.fwd.ops) + (list(plan.bwd.ops) if plan.bwd is not None else [])


def _span_disjoint(spans, what):
    spans = sorted(spans)
    for (a0, a1, na), (b0, b1, nb) in zip(spans, spans[1:]):
        assert a1 <= b0, f"{what}: {na} [{a0}, {a1}) overlaps {nb} [{b0}, {b1})"


@pytest.mark.parametrize("model,precision", PLAN_IDS)
def test_planned_weight_pack_tables(model, precision):
    plan = _plan(model, precision)
    packs = [f for k, f in _ops(plan) if k == "WEIGHT_PACK"]
    assert packs
    f32_spans, mirror_spans, where = [], [], {}
    for pi, f in enumerate(packs):
        rows = _table(plan, f["TABLE"], 12)
        assert f["N_ENTRIES"] == len(rows) and f["DST"].base == D.BASE["WPACK"] and f["DST"].off == 0
        bases = {k: f.get(k, 0) for k in ("BF16_BASE", "Q4_BASE", "SPLIT_BASE")}
        assert all(b % 16 == 0 and b >= 0 for b in bases.values())
        assert {"f32": (0, 0), "bf16-mixed": (1, 0), "f32-split": (0, None)}[precision][0] == (bases["BF16_BASE"] > 0)
        if precision == "bf16-mixed":
            assert not bases["Q4_BASE"] and not bases["SPLIT_BASE"]
        start = 0
        for ri, r in enumerate(rows):
            src_off, dst_off, M, K, T, s_m, s_k, s_t, flip, MP, KP, st = r
            n = PR.entry_floats(r)
            assert st == start, "start is not the running sum of KP * T * MP"
            start += n
            assert MP % 128 == 0 and KP % 64 == 0 and dst_off % 8 == 0 and MP >= M and KP >= K and MP - M < 128 and KP - K < 64
            assert not (flip & 2) or T == 1, "the quad flag on a row that is no 1x1 entry"
            assert not (flip & ~3)
            # the source stays inside the parameter buffer
            assert 0 <= src_off and src_off + (M - 1) * s_m + (K - 1) * s_k + (T - 1) * s_t < plan.layout.n_params
            name = f"pack {pi} row {ri}"
            f32_spans.append((4 * dst_off, 4 * (dst_off + n), name))
            assert dst_off not in where, "two rows write one entry"
            where[dst_off] = (r, bases)
            if bases["BF16_BASE"]:
                a = PR.bf16_addr(bases["BF16_BASE"], dst_off)
                mirror_spans.append((a, a + 2 * n, name + " bf16"))
            if bases["Q4_BASE"] and PR.q4_wanted(r):
                a = PR.q4_addr(bases["Q4_BASE"], dst_off)
                mirror_spans.append((a, a + 4 * n, name + " quad"))
            if bases["SPLIT_BASE"]:
                a = PR.split_addr(bases["SPLIT_BASE"], dst_off, 0, n)
                assert [PR.split_addr(bases["SPLIT_BASE"], dst_off, p, n) for p in (1, 2)] == [a + 2 * n, a + 4 * n]
                mirror_spans.append((a, a + 6 * n, name + " split"))
        assert f["TOTAL"] == start and start % 4096 == 0
    _span_disjoint(f32_spans, "f32 packs")
    _span_disjoint(mirror_spans, "mirrors")
    packs_end = max(e for _, e, _ in f32_spans)
    assert all(a >= packs_end for a, _, _ in mirror_spans), "a mirror region starts inside the f32 packs"
    assert max(e for _, e, _ in f32_spans + mirror_spans) <= plan.wpack_bytes
    # every CONV weight reference into WPACK is exactly one row's entry, and WTB the copy of the SAME row the flag stands for
    n_wt = n_wtb = 0
    for k, f in _ops(plan):
        if k != "CONV":
            continue
        wt, wtb, flags = f.get("WT"), f.get("WTB"), f.get("_flags", 0)
        if not (isinstance(wt, TRef) and wt.base == D.BASE["WPACK"]):
            assert wtb is None
            continue
        n_wt += 1
        assert wt.off % 4 == 0 and wt.off // 4 in where, "WT is no row's entry"
        r, bases = where[wt.off // 4]
        n = PR.entry_floats(r)
        assert f["M"] == r[2] and f["C1"] + f["C2"] == r[3] and f["KH"] * f["KW"] == r[4]
        assert (f["W_SM"], f["W_SK"], f["W_ST"], f["FLIP"]) == (1, r[4] * r[9], r[9], 0)
        if wtb is None:
            assert not flags & (D.FLAG_BF16 | D.FLAG_Q4 | D.FLAG_SPLIT)
            continue
        n_wtb += 1
        assert wtb.base == D.BASE["WPACK"]
        kinds = [b for b in (D.FLAG_BF16, D.FLAG_Q4, D.FLAG_SPLIT) if flags & b]
        assert len(kinds) == 1
        if flags & D.FLAG_BF16:
            assert bases["BF16_BASE"] and wtb.off == PR.bf16_addr(bases["BF16_BASE"], r[1])
        elif flags & D.FLAG_Q4:
            assert bases["Q4_BASE"] and PR.q4_wanted(r) and wtb.off == PR.q4_addr(bases["Q4_BASE"], r[1])
        else:
            assert bases["SPLIT_BASE"] and wtb.off == PR.split_addr(bases["SPLIT_BASE"], r[1], 0, n)
    assert n_wt > 0
    if model == "unet256" or (model == "unet" and precision != "f32"):
        assert n_wtb > 0


def test_the_f32_unet_plan_has_quad_rows_and_unflagged_1x1_rows():
    """what the multi-row GPU cases mix - quad-flagged and unflagged T = 1 rows in one table - is what a real plan holds"""
    plan = _plan("unet256", "f32")
    rows = [r for k, f in _ops(plan) if k == "WEIGHT_PACK" and f.get("Q4_BASE") for r in _table(plan, f["TABLE"], 12)]
    assert any(PR.q4_wanted(r) for r in rows) and any(r[4] == 1 and not r[8] & 2 for r in rows) and any(r[4] == 9 for r in rows)


@pytest.mark.parametrize("model,precision", PLAN_IDS)
def test_planned_wgrad_finalize_tables(model, precision):
    plan = _plan(model, precision)
    params = {off: (name, shape) for name, (off, shape) in plan.layout.params.items()}
    folded = []
    for k, f in _ops(plan):
        if k != "WGRAD_FINALIZE":
            continue
        rows = _table(plan, f["TABLE"], 5)
        assert f["N_ENTRIES"] == len(rows)
        assert f["WGS"].base == D.BASE["WGS"] and f["GRADS"].base == D.BASE["GRADS"] and f["WGS"].off == 0 and f["GRADS"].off == 0
        start = 0
        for off, M, C, T, st in rows:
            assert st == start
            start += M * C * T
            name, shape = params[off]                 # the entry's slice IS a parameter's slice
            assert shape[0] == M and shape[1] == C and int(np.prod(shape[2:])) == T, (name, shape, (M, C, T))
            folded.append(off)
        assert f["TOTAL"] == start and 0 < start < 2 ** 31
    assert len(folded) == len(set(folded)), "a conv weight is folded twice"
    starts = sorted(params)
    owners = set()
    for k, f in _ops(plan):
        if k == "WGRAD" and f["WGS"].base == D.BASE["WGS"]:
            fo = f["WGS"].off // 4
            owners.add(max(s for s in starts if s <= fo))
    assert owners == set(folded), "the weights whose gradient goes through the scratch are not the weights that are folded"
    if model != "mae":
        assert folded


@pytest.mark.parametrize("model,precision", PLAN_IDS)
def test_planned_axpy_operands_are_16_byte_aligned(model, precision):
    """axpy_kernel casts X and Y to float4 unconditionally"""
    plan = _plan(model, precision)
    n = 0
    for k, f in _ops(plan):
        if k == "AXPY":
            n += 1
            assert f["X"].off % 16 == 0 and f["Y"].off % 16 == 0 and f["COUNT"] > 0
        if k == "MEMSET":
            assert f["BYTES"] > 0
    if model.startswith("unet"):
        assert n > 0


# ---- wiring: the planned table through the reference gives back the parameters ------------------------------------------------------------
def test_b0_forward_pack_table_slices_back_to_the_parameters():
    m = _unet_model()
    net = R.build("b0", 4, 4)
    sd = detgen.fill_state(R.state_shapes(net), seed=5)
    m.load_state_dict(sd)
    plan = _plan("unet", "f32")
    flat = m._flat_params.detach().cpu().numpy()
    by_off = {}
    for k, f in plan.fwd.ops:
        if k == "WEIGHT_PACK" and not f.get("_flags", 0) & D.FLAG_SIDE:      # the forward's own table (the backward's rides the side stream)
            rows = _table(plan, f["TABLE"], 12)
            for r, (addr, b) in zip(rows, PR.f32_pack(rows, flat)):
                assert addr == 4 * r[1]
                by_off.setdefault(r[0], []).append((r, b.view(np.float32)))
    assert by_off

    def entry(name, M, K, T):
        off, shape = plan.layout.params[name]
        (r, w), = [(r, w) for r, w in by_off[off] if (r[2], r[3], r[4]) == (M, K, T)]
        return w.reshape(r[10], T, r[9])[:K, :, :M], sd[name].detach().numpy()

    # a 3x3 conv [M][C][3][3] -> [C][tap][M]
    got, w = entry("double_convs.0.3.weight", 512, 512, 9)
    assert np.array_equal(got, w.reshape(512, 512, 9).transpose(1, 2, 0))
    # a 1x1 conv [M][C][1][1] -> [C][1][M]
    got, w = entry("out_conv1x1.weight", 4, 32, 1)
    assert np.array_equal(got, w.reshape(4, 32, 1).transpose(1, 2, 0))
    # a ConvTranspose [Cin][Cout][2][2] -> [Cin][1][(co, dy, dx)]
    cin = sd["up_convs.1.weight"].shape[0]
    got, w = entry("up_convs.1.weight", 4 * 256, cin, 1)
    assert np.array_equal(got, w.reshape(cin, 1, 4 * 256))
