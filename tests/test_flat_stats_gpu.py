"""GPU: the SEG_STATS / SEG_HIST / GRAD_CLIP stages (csrc/flat_stats.hip) as programs through the C ABI against their float64 numpy
restatement (tests/flat_stats_ref.py; the ops have no entry in oracle/ops_ref.py), and `flat_stats.FlatStats` / `clip_grad_norm_` /
`grad_norm` end to end on the smoke() configurations of the U-Net and the MAE.

Bars.
* SEG_STATS: min, max and COUNTS exact; sum within n * 2^-53 * sum|x| and sumsq within n * 2^-53 * sum x^2 of the restatement - the
  worst-case bound of ANY f64 summation order (the restatement's order is numpy's pairwise one, not the kernel's); a NaN / Inf sumsq
  as in the restatement; two runs on the same bytes bit-identical.
* SEG_HIST: exact equality with the restatement, which evaluates the same f64 expression (f64 subtraction, division, multiplication
  and floor are correctly rounded on the device).
* GRAD_CLIP: elements within 2 * 2^-23 relative of float32(x * coef) - one rounding of coef, whose f64 input may differ in the last bit,
  and one of the product; NORM within 2^-23 relative; without clipping, and outside the segments always, bit-identical.
* End to end: the bars above per tensor; after `clip_grad_norm_` + one `FlatAdam.step()` the parameters equal a twin's (clipped with
  `torch.nn.utils.clip_grad_norm_`, stepped with the same FlatAdam) to 8 * 2^-23 of the update's magnitude.  The step runs with lr = 1
  so that the update (|lr * m / (sqrt(v) + eps)| = 1 on the first Adam step) is not smaller than the parameters themselves: the bar
  is 9.5e-7, and the f32 rounding of the stored parameter (an ulp of a value below 8: 4.8e-7) stays inside it.  With the
  default lr = 1e-3 the bar (9.5e-10) would lie below the rounding of the parameter and no implementation could meet it.

Measured on an MI355X: histograms 0 counts off in all eight cases; clipped elements 0.000 * 2^-23 from float32(x * coef) (the device's
coef equals the restatement's), NORM 9.5e-9 relative; end to end the clipped gradients are at most 0.67 * 2^-23 relative from torch's
and the stepped parameters at most 2.45 (U-Net) / 2.00 (MAE) * 2^-23 of the update from the twin's."""
import functools

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import flat_stats as FS
from tests.flat_stats_ref import grad_clip_ref, probe, seg_hist_ref, seg_stats_ref
from tests.test_ops_gpu import Case
from tests.test_predict_gpu import run_records

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = FS.CHUNK
LAYOUTS = {"aligned": (0, 0), "unaligned": (1, 3)}        # starts on 64-float boundaries / at offsets 1 and 3 mod 4


@functools.lru_cache(maxsize=None)
def layout(name, nan_segments=True, pad=float("nan")):
    """(x, segs, names, SEGS, CHUNKS, reference STATS, reference COUNTS) - computed once, shared, never written"""
    x, segs, names = probe(CHUNK, special=True, nan_segments=nan_segments, shifts=LAYOUTS[name], pad=pad)
    if name == "unaligned":
        assert {first % 4 for first, _ in segs} == {1, 3}
    else:
        assert all(first % 64 == 0 for first, _ in segs)
    S, C = FS.build_tables(segs)
    FS.check_tables(S, C, x.size)
    stats, counts = seg_stats_ref(x, segs)
    return x, segs, names, S, C, stats, counts


def make_case(name, nan_segments=True, pad=float("nan")):
    x, segs, names, S, C, _, _ = layout(name, nan_segments, pad)
    c = Case(3)
    P, NC = len(S), len(C)
    f = dict(X=c.t("x", (x.size,), torch.from_numpy(x.copy())), SEGS=c.t("segs", (P, 2), torch.from_numpy(S), "i32"),
             CHUNKS=c.t("chunks", (NC, 2), torch.from_numpy(C), "i32"), STATS=c.t("stats", (P, 4), "nan", "f64"), P=P, NC=NC)
    stats_rec = ("SEG_STATS", dict(f, PART=c.t("part", (NC, 6), "nan", "f64"), COUNTS=c.t("counts", (P, 2), torch.full((P, 2), -1), "i64")))
    return c, f, stats_rec


# ---- SEG_STATS ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_seg_stats_matches_the_float64_reference(name):
    x, segs, names, _, _, want, want_counts = layout(name)
    c, _, rec = make_case(name)
    img = run_records(c, [rec])
    got, counts = c.read(img, "stats").numpy(), c.read(img, "counts").numpy()
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(got[:, 2], want[:, 2]) and np.array_equal(got[:, 3], want[:, 3])           # min / max exact (+-inf: none finite)
    for p, ((first, n), nm) in enumerate(zip(segs, names)):
        v = x[first:first + n].astype(np.float64)
        fin = v[np.isfinite(v)]
        bar_s, bar_q = n * 2.0 ** -53 * np.abs(fin).sum(), n * 2.0 ** -53 * (fin * fin).sum()
        err_s = abs(got[p, 0] - want[p, 0])
        print(f"{name} {nm}: sum err {err_s:.3e} (bar {bar_s:.3e}), sumsq {got[p, 1]!r} (ref {want[p, 1]!r}, bar {bar_q:.3e})")
        assert err_s <= bar_s
        if np.isfinite(want[p, 1]):
            assert abs(got[p, 1] - want[p, 1]) <= bar_q
        else:
            assert np.isnan(got[p, 1]) if np.isnan(want[p, 1]) else got[p, 1] == want[p, 1]
    assert np.isnan(want[names.index("mixed"), 1]) and want[names.index("infs"), 1] == np.inf and np.isnan(want[names.index("nonfinite"), 1])
    assert want[names.index("nonfinite"), 2] == np.inf and want[names.index("nonfinite"), 3] == -np.inf
    # the same record on the same bytes again: bit-identical
    img2 = run_records(c, [rec])
    assert torch.equal(c.read(img, "stats").view(torch.int64), c.read(img2, "stats").view(torch.int64))
    assert torch.equal(c.read(img, "counts"), c.read(img2, "counts"))
    assert torch.equal(c.read(img, "x").view(torch.int32), torch.from_numpy(x.copy()).view(torch.int32))      # X is only read


# ---- SEG_HIST -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NB", [64, 1, 7, 256])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_seg_hist_equals_the_reference_and_accumulates(name, NB):
    x, segs, names, _, _, want_stats, want_counts = layout(name)
    c, f, rec = make_case(name)
    P = len(segs)
    hist_rec = ("SEG_HIST", dict(f, HIST=c.t("hist", (P, NB), torch.zeros(P, NB), "i64"), NB=NB))
    img = run_records(c, [rec, hist_rec])
    got = c.read(img, "hist").numpy()
    want = seg_hist_ref(x, segs, want_stats, NB)       # min / max are exact (tested above), so the reference's own range is the stage's
    diff = int(np.abs(got - want).sum())
    print(f"{name} NB={NB}: {diff} counts differ")
    assert np.array_equal(got, want)
    finite = np.array([n for _, n in segs]) - want_counts.sum(axis=1)
    assert np.array_equal(got.sum(axis=1), finite)
    assert got[names.index("nonfinite")].sum() == 0
    assert got[names.index("constant"), NB // 2] == segs[names.index("constant")][1]
    assert got[names.index("zero"), NB // 2] == segs[names.index("zero")][1]
    img2 = run_records(c, [rec, hist_rec, hist_rec])       # a second record into the same HIST doubles it
    assert np.array_equal(c.read(img2, "hist").numpy(), 2 * want)


# ---- GRAD_CLIP ----------------------------------------------------------------------------------------------------------------------
def _outside(x, segs):
    m = np.ones(x.size, dtype=bool)
    for first, n in segs:
        m[first:first + n] = False
    return m


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_grad_clip_scales_the_segments_only(name):
    x, segs, names, _, _, want_stats, _ = layout(name, False, 3.0)       # finite padding: a stray multiply would show
    norm, _, _ = grad_clip_ref(x, segs, want_stats[:, 1], 1.0)
    max_norm = float(np.float32(0.5 * norm))
    norm, coef, _ = grad_clip_ref(x, segs, want_stats[:, 1], max_norm)
    assert coef < 1.0
    c, f, rec = make_case(name, False, 3.0)
    clip = ("GRAD_CLIP", dict(f, NORM=c.t("norm", (1,), "nan"), APPLY=1, MAX_NORM=max_norm))
    img = run_records(c, [rec, clip])
    got, got_norm = c.read(img, "x").numpy(), float(c.read(img, "norm")[0])
    out = _outside(x, segs)
    assert np.array_equal(got.view(np.uint32)[out], x.view(np.uint32)[out])          # padding and decoy regions bit-identical
    want = (x.astype(np.float64) * coef).astype(np.float32).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)[~out]
    rel = float(np.max(err[want[~out] != 0] / np.abs(want[~out][want[~out] != 0])))
    print(f"{name}: elements rel {rel / 2.0 ** -23:.3f} * 2^-23, NORM rel {abs(got_norm - norm) / norm:.3e}")
    assert np.all(err <= 2 * 2.0 ** -23 * np.abs(want[~out]))
    assert abs(got_norm - norm) <= 2.0 ** -23 * norm
    before = run_records(c, [rec])          # the arena as SEG_STATS leaves it (bit-identical from run to run)
    for name_ in ("segs", "chunks", "stats", "part", "counts"):          # nothing but X and NORM is written by the clipping pass
        assert torch.equal(c.read(img, name_).contiguous().view(torch.uint8), c.read(before, name_).contiguous().view(torch.uint8))
    # MAX_NORM at twice the norm: nothing is written
    clip2 = ("GRAD_CLIP", dict(f, NORM=f_norm(c), APPLY=1, MAX_NORM=float(np.float32(2.0 * norm))))
    img = run_records(c, [rec, clip2])
    assert np.array_equal(c.read(img, "x").numpy().view(np.uint32), x.view(np.uint32))
    assert abs(float(c.read(img, "norm")[0]) - norm) <= 2.0 ** -23 * norm
    # the WHOLE arena - X, SEGS, CHUNKS, PART, STATS, COUNTS, every alignment gap - is what it was before GRAD_CLIP, NORM excepted
    keep = torch.ones(before.numel(), dtype=torch.bool)
    keep[f_norm(c).off:f_norm(c).off + 4] = False
    assert torch.equal(before[keep], img[keep])
    # APPLY = 0: the norm alone, X untouched even with a MAX_NORM far below the norm
    clip3 = ("GRAD_CLIP", dict(STATS=f["STATS"], NORM=f_norm(c), P=f["P"], NC=f["NC"], APPLY=0, MAX_NORM=1e-3))
    img = run_records(c, [rec, clip3])
    assert np.array_equal(c.read(img, "x").numpy().view(np.uint32), x.view(np.uint32))
    assert abs(float(c.read(img, "norm")[0]) - norm) <= 2.0 ** -23 * norm


def f_norm(c):
    return c.items["norm"][0]


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_grad_clip_with_a_nan_segment(name):
    x, segs, names, _, _, _, _ = layout(name, True, 3.0)
    c, f, rec = make_case(name, True, 3.0)
    clip = ("GRAD_CLIP", dict(f, NORM=c.t("norm", (1,), torch.zeros(1)), APPLY=1, MAX_NORM=1.0))
    img = run_records(c, [rec, clip])
    got = c.read(img, "x").numpy()
    out = _outside(x, segs)
    assert np.isnan(got[~out]).all() and np.isnan(float(c.read(img, "norm")[0]))
    assert np.array_equal(got.view(np.uint32)[out], x.view(np.uint32)[out])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _unet_pair():
    from oracle import detgen
    from oracle import efficientnet_unet_ref as R
    from s2lc_amd.losses import FocalLoss
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet

    version, C, H, B, ncls = "b0", 4, 64, 2, 4
    net = R.build(version, C, ncls)
    sd = detgen.fill_state(R.state_shapes(net), seed=5)
    x = detgen.normal("smoke.x", (B, C, H, H), seed=5).to(DEV)
    y = detgen.labels("smoke.y", (B, H, H), ncls, seed=5).to(DEV)
    noise = detgen.uniform("smoke.dc", (len(net.blocks), B), 0.0, 1.0, seed=5)
    loss_fn = FocalLoss(torch.ones(ncls), 2.0, 0.0, ignore_index=0)

    def make():
        m = EfficientnetUnet(EfficientNetConfig(version, C, ncls, class_distribution=[0.25] * 4))
        m.load_state_dict(sd)
        m.to(DEV).train()
        m.drop_connect_noise = noise
        return m

    def backward(m):
        loss_fn(m(x), y).backward()

    return make, backward, "encoder.fc.3.weight"


def _mae_pair():
    from oracle import detgen
    from oracle import prithvi_ref as P
    from s2lc_amd.modules.prithvi import MaskedAutoencoderViT

    args = dict(img_size=32, patch_size=8, num_frames=1, tubelet_size=1, in_chans=3, embed_dim=32, depth=2, num_heads=2,
                decoder_embed_dim=16, decoder_depth=1, decoder_num_heads=2)
    cfg = P.MaeCfg(**args)
    sd = detgen.fill_state(P.mae_state_shapes(cfg), seed=9)
    sd["pos_embed"] = P.sincos_pos_embed(cfg.embed_dim, cfg.grid)
    sd["decoder_pos_embed"] = P.sincos_pos_embed(cfg.decoder_embed_dim, cfg.grid)
    x = detgen.normal("smoke.mae.x", (2, 3, 1, 32, 32), seed=9).to(DEV)
    noise = detgen.uniform("smoke.mae.noise", (2, cfg.num_patches), 0.0, 1.0, seed=9)

    def make():
        m = MaskedAutoencoderViT(**args)
        m.load_state_dict(sd)
        m.to(DEV)
        m.masking_noise = noise
        return m

    def backward(m):
        m(x, mask_ratio=0.75)[0].backward()

    return make, backward, "pos_embed"


def _check_against_numpy(result, tensors, bins):
    """a SegmentStats against per-tensor float64 numpy on the tensors' host copies: the stage bars, per tensor"""
    host = result.cpu()
    assert list(host) == result.names == list(tensors) and result.numel == [t.numel() for t in tensors.values()]
    st, ct = result.stats.cpu().numpy(), result.counts.cpu().numpy()
    assert not ct.any()
    for i, (name, t) in enumerate(tensors.items()):
        v32 = t.detach().cpu().numpy().reshape(-1)
        v = v32.astype(np.float64)
        n = v.size
        assert st[i, 2] == v.min() and st[i, 3] == v.max()
        assert abs(st[i, 0] - v.sum()) <= n * 2.0 ** -53 * np.abs(v).sum()
        assert abs(st[i, 1] - (v * v).sum()) <= n * 2.0 ** -53 * (v * v).sum()
        h = host[name]
        assert h["min"] == st[i, 2] and h["max"] == st[i, 3] and h["nan"] == 0 and h["inf"] == 0
        assert h["norm"] == np.sqrt(st[i, 1]) and h["mean"] == st[i, 0] / n
        if bins is None:
            assert result.hist is None and h["hist"] is None and h["edges"] is None
        else:
            want = seg_hist_ref(v32, [(0, n)], st[i:i + 1], bins)[0]
            assert np.array_equal(h["hist"], want), name
            assert h["hist"].sum() == n and h["edges"].shape == (bins + 1,)
            lo, hi = (st[i, 2] - 1, st[i, 3] + 1) if st[i, 2] == st[i, 3] else (st[i, 2], st[i, 3])
            assert h["edges"][0] == lo and h["edges"][-1] == hi


@pytest.mark.parametrize("pair", [_unet_pair, _mae_pair], ids=["unet_b0", "mae_small"])
def test_end_to_end(pair):
    from s2lc_amd.optim import FlatAdam

    make, backward, unused = pair()
    model, twin = make(), make()
    backward(model)
    backward(twin)
    named = dict(model.named_parameters())
    with_grad = {n: p.grad for n, p in named.items() if n not in model._no_grad_params and p.requires_grad and p.grad is not None}
    assert unused in named and unused not in with_grad and 0 < len(with_grad) < len(named)

    stats = FS.FlatStats(model, bins=64)
    _check_against_numpy(stats.gradients(), with_grad, 64)
    _check_against_numpy(stats.parameters(hist=False), {n: p.data for n, p in named.items()}, None)
    _check_against_numpy(FS.FlatStats(model, bins=7).parameters(), {n: p.data for n, p in named.items()}, 7)
    tables = stats._tables[True][1]
    assert stats.gradients().names == list(with_grad) and stats._tables[True][1] is tables          # cached: not rebuilt

    # freeze one parameter: after the next backward the selection follows and the tables are rebuilt
    frozen = list(with_grad)[-1]
    named[frozen].requires_grad_(False)
    backward(model)
    g2 = stats.gradients()
    assert g2.names == [n for n in with_grad if n != frozen] and stats._tables[True][1] is not tables
    _check_against_numpy(g2, {n: named[n].grad for n in g2.names}, 64)
    assert stats.parameters(hist=False).names == list(named)
    named[frozen].requires_grad_(True)          # unfrozen again: it still holds its gradient view, so the selection is the full one
    assert stats.gradients(hist=False).names == list(with_grad)
    twin._grad_buffer().copy_(model._grad_buffer())          # the same gradients bit for bit (weight-gradient sums vary from run to run)
    tables = stats._tables[True][1]

    # the norm: float64 numpy over the same tensors, and torch's own on the twin
    want_norm = float(np.sqrt(sum((g.detach().cpu().numpy().astype(np.float64) ** 2).sum() for g in with_grad.values())))
    before = model._grad_buffer().clone()
    got_norm = FS.grad_norm(model)
    assert got_norm.shape == () and got_norm.dtype == torch.float32 and got_norm.is_cuda
    assert abs(float(got_norm) - want_norm) <= 2.0 ** -23 * want_norm
    assert torch.equal(model._grad_buffer().view(torch.int32), before.view(torch.int32))
    # a max_norm above the norm leaves the buffer bit-identical
    assert abs(float(FS.clip_grad_norm_(model, 2.0 * want_norm)) - want_norm) <= 2.0 ** -23 * want_norm
    assert torch.equal(model._grad_buffer().view(torch.int32), before.view(torch.int32))

    # clip below the norm, then one Adam step, against the twin clipped by torch
    max_norm = 0.5 * want_norm
    total = FS.clip_grad_norm_(model, max_norm, error_if_nonfinite=True)
    total_twin = torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm)
    assert abs(float(total) - want_norm) <= 2.0 ** -23 * want_norm and abs(float(total_twin) - want_norm) <= 1e-6 * want_norm
    # floats outside the selected tensors (padding, unused parameters) were not touched
    out = torch.ones(before.numel(), dtype=torch.bool)
    for first, n in zip((s[0] for s in tables.segs.tolist()), tables.numel):
        out[first:first + n] = False
    assert torch.equal(model._grad_buffer().cpu().view(torch.int32)[out], before.cpu().view(torch.int32)[out])
    g_rel = max(float(((a.double() - b.double()).abs() / b.double().abs().clamp_min(1e-300)).max())
                for a, b in ((named[n].grad, dict(twin.named_parameters())[n].grad) for n in with_grad))
    print(f"clipped gradients differ from torch's by at most {g_rel / 2.0 ** -23:.2f} * 2^-23 relative")
    assert g_rel <= 8 * 2.0 ** -23          # the bar of the CPU comparison with torch: the clipping itself, which Adam's first step barely sees
    old = {n: p.detach().clone() for n, p in named.items()}
    FlatAdam(model, lr=1.0).step()
    FlatAdam(twin, lr=1.0).step()
    worst = 0.0
    for (n, a), b in zip(model.named_parameters(), twin.parameters()):
        upd = float((a.detach() - old[n]).abs().max())
        d = float((a.detach().double() - b.detach().double()).abs().max())
        if n not in with_grad or upd == 0.0:          # not stepped, or an all-zero gradient: both sides left it where it was
            assert upd == 0.0 and d == 0.0, n
            continue
        worst = max(worst, d / upd)
        assert d <= 8 * 2.0 ** -23 * upd, (n, d, upd)
    print(f"parameters after the step differ by at most {worst / 2.0 ** -23:.2f} * 2^-23 of the update")
