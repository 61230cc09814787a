"""CPU: the f32-SPLIT precision mode's public switch and its plans (plan/split.py, unet_plan.mark_split).  A split plan is the f32 plan
plus FLAG_SPLIT on the stages plan/split.py routes, their split weight copies (WEIGHT_PACK SPLIT_BASE) and nothing else; the
emulator computes a flagged stage in exact f32, so the emulated split plan is the emulated f32 plan."""
import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import detgen
from oracle import efficientnet_unet_ref as R
from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan import split as SP
from s2lc_amd.plan.program import TRef
from tests.helpers import rel_err
from tests.plan_harness import emulate, fview, make_bases


def _model(version, C, ncls=4):
    return EfficientnetUnet(EfficientNetConfig(version, C, ncls, class_distribution=[1.0 / ncls] * ncls))


def test_precision_accepts_f32_split():
    m = _model("b0", 4)
    m.precision = "f32-split"
    assert m.precision == "f32-split"
    with pytest.raises(ValueError, match="f32-split"):
        m.precision = "tf32"


@pytest.mark.parametrize("version,C,H,B", [("b0", 4, 64, 4), ("b5", 13, 256, 8)])
def test_split_plan_flags_exactly_what_plan_split_routes(version, C, H, B):
    m = _model(version, C)
    ref = m._make_plan(B, H, H, True)
    m.precision = "f32-split"
    plan = m._make_plan(B, H, H, True)
    n = 0
    for p32, ps in ((ref.fwd, plan.fwd), (ref.bwd, plan.bwd)):
        assert [k for k, _ in p32.ops] == [k for k, _ in ps.ops]
        for (kind, f32), (_, f) in zip(p32.ops, ps.ops):
            flags = f.get("_flags", 0)
            assert not flags & D.FLAG_BF16 and not f.get("X1_BF16", 0) and not f.get("P_BF16", 0)
            assert flags & ~D.FLAG_SPLIT == f32.get("_flags", 0)          # the f32 plan's own flags are untouched
            if kind not in ("CONV", "WGRAD"):
                continue
            dedicated = f32.get("_flags", 0) & (D.FLAG_Q4 | D.FLAG_RES_GELU_GRAD | D.FLAG_DMA)
            want = SP.routed(kind, f) and not dedicated and (kind == "WGRAD" or f["WT"].base == D.BASE["WPACK"])
            assert bool(flags & D.FLAG_SPLIT) == want, (kind, {k: f[k] for k in ("B", "H", "W") if k in f})
            n += want
            if flags & D.FLAG_SPLIT and kind == "CONV":
                assert f["WTB"].base == D.BASE["WPACK"] and f["WTB"].name.startswith("split:")
            # every field but the flag and the split weight copy is the f32 plan's
            assert {k: v for k, v in f.items() if k not in ("_flags", "WTB")} == \
                   {k: v for k, v in f32.items() if k not in ("_flags", "WTB")} or kind == "WEIGHT_PACK"
    assert n >= (20 if version == "b0" else 40), n


@pytest.mark.parametrize("version,C,H,B", [("b0", 4, 64, 2), ("b5", 13, 128, 2)])
def test_split_weight_region_lies_beyond_the_packs(version, C, H, B):
    m = _model(version, C)
    m.precision = "f32-split"
    plan = m._make_plan(B, H, H, True)
    packs = [f for prog in (plan.fwd, plan.bwd) for k, f in prog.ops if k == "WEIGHT_PACK"]
    assert packs and all(f["SPLIT_BASE"] > 0 and f["SPLIT_BASE"] % 256 == 0 for f in packs)
    base = packs[0]["SPLIT_BASE"]
    f32_end, q4_lo, q4_hi = 0, None, 0
    for prog in (plan.fwd, plan.bwd):
        for k, f in prog.ops:
            if k != "CONV" or not isinstance(f.get("WT"), TRef) or f["WT"].base != D.BASE["WPACK"]:
                continue
            f32_end = max(f32_end, f["WT"].off + f["WT"].nbytes)
            if f.get("_flags", 0) & D.FLAG_Q4:
                q4_lo = f["WTB"].off if q4_lo is None else min(q4_lo, f["WTB"].off)
                q4_hi = max(q4_hi, f["WTB"].off + f["WTB"].nbytes)
    assert base >= f32_end and base >= q4_hi
    for prog in (plan.fwd, plan.bwd):
        for k, f in prog.ops:
            if k == "CONV" and f.get("_flags", 0) & D.FLAG_SPLIT:
                wt, wtb = f["WT"], f["WTB"]
                assert wtb.off == base + 3 * wt.off // 2                  # the entry's three planes: 6 bytes per packed f32 element
                assert wtb.off + 3 * wt.nbytes // 2 <= plan.wpack_bytes


def test_emulated_split_plan_equals_the_f32_plan_float64():
    """oracle/ops_ref.py reads FLAG_SPLIT (64) as exact f32: in the float64 emulation the split training plan reproduces the f32
    plan's logits and gradients"""
    version, C, H, B, ncls = "b0", 6, 64, 2, 4
    net = R.build(version, C, ncls)
    sd = detgen.fill_state(R.state_shapes(net), seed=31)
    x = detgen.normal("split.x", (B, C, H, H), seed=31)
    noise = detgen.uniform("split.dc", (len(net.blocks), B), 0.0, 1.0, seed=31)
    dl = detgen.normal("split.dl", (B, ncls, H, H), seed=31).double()
    out = {}
    for prec in ("f32", "f32-split"):
        m = _model(version, C, ncls)
        m.load_state_dict(sd)
        m.precision = prec
        plan = m._make_plan(B, H, H, True)
        if prec == "f32-split":
            assert sum(1 for k, f in plan.bwd.ops if f.get("_flags", 0) & D.FLAG_SPLIT) >= 10
        bases = make_bases(plan, m._flat_params, m._flat_bufs, x, noise, B * ncls * H * H, True)
        emulate(plan.fwd.pack(), bases, True)
        logits = fview(bases, "OUT", True).clone()
        fview(bases, "DOUT", True).copy_(dl.reshape(-1))
        emulate(plan.bwd.pack(), bases, True)
        out[prec] = (logits, fview(bases, "GRADS", True).clone())
    (l0, g0), (l1, g1) = out["f32"], out["f32-split"]
    assert rel_err(l1.numpy(), l0.numpy()) < 1e-5
    assert rel_err(g1.numpy(), g0.numpy()) < 1e-5
    assert np.isfinite(g1.numpy()).all()
