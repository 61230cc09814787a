"""The f32-SPLIT mode at model level (module.precision = "f32-split"): f32-accurate, so it is held to the f32 path's own bars -
against the fp32 reference fixtures and against the f32 path - not to a mode tolerance of its own."""
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import detgen
from oracle import efficientnet_unet_ref as R
from s2lc_amd.plan import opdefs as D
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(version, C, ncls, seed):
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet

    net = R.build(version, C, ncls)
    sd = detgen.fill_state(R.state_shapes(net), seed=seed)
    model = EfficientnetUnet(EfficientNetConfig(version, C, ncls, class_distribution=[1.0 / ncls] * ncls))
    model.load_state_dict(sd)
    return model, net, sd


def _step(model, x, y, noise):
    from s2lc_amd.losses import FocalLoss

    model.drop_connect_noise = noise
    for p in model.parameters():
        p.grad = None
    logits = model(x)
    loss = FocalLoss(torch.ones(logits.shape[1]), 2.0, 0.0, ignore_index=0)(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), float(loss), model._grad_buffer().detach().clone()


@pytest.mark.parametrize("version,C,H,B", [("b0", 4, 64, 4), ("b5", 13, 256, 8)])
def test_every_flagged_stage_runs_on_the_split_kernels(version, C, H, B):
    """plan/split.py and the native split launchers agree: flagged <=> kernel family 5, at a toy size and at the benchmark's tile
    shape (a flagged stage the launchers did not take would have failed the run: there is no fall-back)"""
    from s2lc_amd import _lib

    model, net, sd = _model(version, C, 4, seed=61)
    model.to(DEV).train()
    model.precision = "f32-split"
    x = detgen.normal("split.x", (B, C, H, H), seed=61).to(DEV)
    model(x)
    eng = next(iter(model._engines.values()))
    st = torch.cuda.current_stream().cuda_stream
    noise = torch.rand(eng.n_noise_rows, B, device=DEV)
    out = torch.empty(eng.plan.logits_shape, device=DEV)
    dout = torch.zeros(eng.plan.logits_shape, device=DEV)
    scratch = torch.zeros_like(model._flat_params)
    n_flag = 0
    for prog, bases in ((eng.fwd, eng.bases(model, x, out, noise=noise)), (eng.bwd, eng.bases(model, x, None, dout=dout, noise=noise, grads=scratch))):
        _, var = _lib.profile_variants(prog, bases, st)
        for i, (rec, v) in enumerate(zip(prog, var)):
            kind = D.NAME_OF[int(rec["kind"])]
            if kind in ("CONV", "WGRAD"):
                flagged = bool(int(rec["flags"]) & D.FLAG_SPLIT)
                n_flag += flagged
                assert flagged == (int(v) == 5), (kind, i, flagged, int(v), [int(d) for d in rec["d"][:16]])
    assert n_flag >= 1, n_flag


def test_unet_b5_256x13_evalgrad_bs4_split_matches_reference(monkeypatch):
    """the f32 path's eval-mode gradient fixture at the benchmark's tile shape (logits 1e-3, class masks, gradients 1e-3 of the
    reference's own), run in the f32-split mode"""
    from s2lc_amd.modules.efficientnet_unet import EfficientnetUnet
    from tests.test_parity_r2_gpu import test_eval_mode_gradients_match_reference as check

    monkeypatch.setattr(EfficientnetUnet, "_precision", "f32-split", raising=False)      # the default of every instance
    check("b5_256x13_evalgrad_bs4", "b5", 13, 256, 4, 33)


@pytest.mark.parametrize("version,C,H,B,seed,training", [("b0", 4, 128, 2, 6, False), ("b5", 13, 128, 2, 8, False), ("b0", 4, 128, 2, 6, True)])
def test_split_against_the_f32_path(version, C, H, B, seed, training):
    """the same step in "f32" and "f32-split": two f32-accurate computations that differ in summation order only"""
    ncls = 4
    x = detgen.normal(f"splf.{seed}.x", (B, C, H, H), seed=seed)
    y = detgen.labels(f"splf.{seed}.y", (B, H, H), ncls, seed=seed)
    m32, net, sd = _model(version, C, ncls, seed)
    noise = detgen.uniform(f"splf.{seed}.dc", (len(net.blocks), B), 0.0, 1.0, seed=seed) if training else None
    m32.to(DEV).train(training)
    l32, s32, g32 = _step(m32, x.to(DEV), y.to(DEV), noise)
    ms, _, _ = _model(version, C, ncls, seed)
    ms.to(DEV).train(training)
    ms.precision = "f32-split"
    ls, ss, gs = _step(ms, x.to(DEV), y.to(DEV), noise)
    e = rel_err(ls.cpu().numpy(), l32.cpu().numpy())
    cos = float((gs.double() * g32.double()).sum() / (gs.double().norm() * g32.double().norm()))
    print(f"{version} {'train' if training else 'eval'}: f32-split vs f32 path: logits {e:.2e}, loss {ss:.7f} vs {s32:.7f}, gradient cosine {cos:.8f}")
    assert e < 1e-3 and abs(ss - s32) <= 1e-4 * abs(s32)
    assert cos > (0.999 if training else 0.99999)


def test_split_bs32_plan_equals_the_replicated_bs8_step():
    """b5, 13 x 256 x 256, bs 32 in the split mode against the bs-8 step on 4 copies of its batch (eval-mode BatchNorm)"""
    model, net, sd = _model("b5", 13, 4, seed=9)
    model.to(DEV).eval()
    model.precision = "f32-split"
    B, rep = 8, 4
    x = detgen.normal("splrep.x", (B, 13, 256, 256), seed=9).to(DEV)
    y = detgen.labels("splrep.y", (B, 256, 256), 4, seed=9).to(DEV)
    lg8, loss8, g8 = _step(model, x, y, None)
    lg32, loss32, g32 = _step(model, x.repeat(rep, 1, 1, 1), y.repeat(rep, 1, 1), None)
    scale = lg8.abs().max().item()
    worst = max((lg32[B * r:B * r + B] - lg8).abs().max().item() / scale for r in range(rep))
    n2 = (g32.double() - g8.double()).norm().item() / g8.double().norm().item()
    print(f"f32-split bs 32 vs bs 8: logits {worst:.2e}, loss {loss32:.7f} vs {loss8:.7f}, |g32 - g8| / |g8| = {n2:.2e}")
    assert worst < 1e-3 and abs(loss32 - loss8) < 1e-5 * abs(loss8)
    assert n2 < 1e-3


def test_prithvi_mae_split_gradients_match_the_f32_path():
    """MaskedAutoencoderViT bs 2 in "f32-split" (the routed Linears and their weight gradients on split operands) against the f32 path"""
    from s2lc_amd.modules.prithvi import MaskedAutoencoderViT
    from tests.helpers import PRITHVI_SMALL

    x = detgen.normal("spl.mae.x", (2, 3, 1, 32, 32), seed=81).to(DEV)
    noise = detgen.uniform("spl.mae.n", (2, 16), 0.0, 1.0, seed=81)
    res = {}
    for prec in ("f32", "f32-split"):
        torch.manual_seed(7)
        m = MaskedAutoencoderViT(**PRITHVI_SMALL).to(DEV)
        m.precision = prec
        m.masking_noise = noise
        loss, pred, mask = m(x, mask_ratio=0.75)
        loss.backward()
        torch.cuda.synchronize()
        res[prec] = (float(loss), pred.detach().clone(), mask.clone(), m._grad_buffer().detach().clone())
        if prec == "f32-split":
            eng = next(e for e in m._engines.values() if e.bwd is not None)
            flagged = sum(1 for prog in (eng.plan.fwd, eng.plan.bwd) for k, f in prog.ops if k in ("CONV", "WGRAD") and f.get("_flags", 0) & D.FLAG_SPLIT)
            print(f"MAE split plan: {flagged} flagged stages")
    (l0, p0, k0, g0), (l1, p1, k1, g1) = res["f32"], res["f32-split"]
    assert torch.equal(k0, k1)
    e = rel_err(p1.cpu().numpy(), p0.cpu().numpy())
    eg = rel_err(g1.cpu().numpy(), g0.cpu().numpy())
    print(f"MAE f32-split vs f32: loss {l1:.7f} vs {l0:.7f}, pred {e:.2e}, gradients {eg:.2e}")
    assert abs(l1 - l0) <= 1e-4 * abs(l0) and e < 1e-3 and eg < 1e-3
