"""The kernels at the end of the step, csrc/loss.hip: LOSS_FWD, LOSS_BWD and ARGMAX at every class count they are compiled
for (loss_{fwd,bwd}_kernel<2..8> and the run-time form <0> for 9..64 classes, which indexes lp[64] / sm[64] dynamically), with
the grid-stride loop taking a second trip, through every branch of pow_gamma and of the saturated focal backward, and with
labels outside [0, C).

Every case compares with oracle/ops_ref.py in f32 AND in float64.  Bars (the project's, tests/test_ops_gpu.py::test_loss_fwd_bwd):
loss and each entry of ACC (the f64 {numerator, denominator} the forward leaves for the backward) 1e-5 relative; dlogits 1e-4 of
its max, over the whole tensor and per class plane (b, c) against that plane's own max.  The f32 oracle itself stays under 2e-6
(value) / 2e-5 (gradient, whole and per plane) of float64 on these inputs.  The backward runs as the second record of a
two-record program, on the ACC its forward wrote - as losses._PixelLoss does; one case keeps a test-supplied ACC."""
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import losses_ref
from s2lc_amd import _lib
from s2lc_amd.plan.program import Program
from tests.test_ops_gpu import Case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAR_VALUE, BAR_GRAD = 1e-5, 1e-4


def _execute(c: Case, records, oracle=True):
    """the records as one program through Case.execute: byte images of the GPU run, the f32 oracle and the float64 oracle"""
    prog = Program()
    for kind, fields in records:
        prog.add(kind, **fields)
    return c.execute(prog.pack(), ref64=True, oracle=oracle)


def _read(c: Case, image, name, wide=False):
    return c.read(image, name, wide)


def _rel(a, b, dims=None):
    """max |a - b| / max |b|, over everything or (dims) per slice of the leading axes"""
    a, b = a.double(), b.double()
    if dims is None:
        return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
    return ((a - b).abs().amax(dims) / b.abs().amax(dims).clamp_min(1e-30)).max().item()


def _form(C):
    return f"<{C}>" if C <= 8 else "<0>"


def _check_value(c, bufs, C, mode, what=""):
    errs = []
    for ref_buf, wide in ((bufs[1], False), (bufs[2], True)):
        loss, want = _read(c, bufs[0], "loss").double(), _read(c, ref_buf, "loss", wide).double()
        acc, wacc = _read(c, bufs[0], "acc"), _read(c, ref_buf, "acc", wide)
        assert torch.isfinite(want).all() and torch.isfinite(wacc).all(), "oracle produced non-finite values"
        e = [_rel(loss, want), _rel(acc[0], wacc[0])]
        if mode == 0:
            e.append(_rel(acc[1], wacc[1]))
        else:
            assert acc[1].item() == 0.0 and wacc[1].item() == 0.0      # focal keeps no denominator
        errs.append(max(e))
    print(f"loss_fwd_kernel{_form(C)} {what}: loss / ACC rel err {errs[0]:.2e} (f32 oracle) {errs[1]:.2e} (float64)")
    assert max(errs) < BAR_VALUE, f"loss / ACC rel err {errs}"
    return errs


def _check_grad(c, bufs, C, what=""):
    got = _read(c, bufs[0], "dlogits")
    assert torch.isfinite(got).all(), "GPU produced non-finite gradients"
    errs = []
    for ref_buf, wide in ((bufs[1], False), (bufs[2], True)):
        want = _read(c, ref_buf, "dlogits", wide)
        assert torch.isfinite(want).all(), "oracle produced non-finite gradients"
        errs += [_rel(got, want), _rel(got, want, dims=2)]
    print(f"loss_bwd_kernel{_form(C)} {what}: dlogits rel err {errs[0]:.2e} whole / {errs[1]:.2e} worst plane (f32 oracle) "
          f"{errs[2]:.2e} / {errs[3]:.2e} (float64)")
    assert max(errs) < BAR_GRAD, f"dlogits rel err (whole, plane) x (f32, float64): {errs}"
    return errs


def _distinct_alpha(C, gen):
    """class weights in [0.3, 1.7], every entry different, in no order: a weight read from the wrong slot, or a denominator that
    counts pixels instead of weights, changes ACC and the gradient.  (The kernels index alpha directly; `pick` is applied to the
    log-probabilities only, so a wrong pick shows in the loss value and the gradient, whatever alpha is.)"""
    return torch.linspace(0.3, 1.7, C)[torch.randperm(C, generator=gen)]


def _labels(B, C, HW, mode, ignore, gen):
    """labels over every class; classes 0, C - 1 and C // 2 are present whatever the draw.  With ignore -100 a tenth of the pixels
    carries it in CE mode (in focal mode the reference indexes alpha with the raw label: -100 must not occur,
    oracle/losses_ref.py::focal)."""
    y = torch.randint(0, C, (B, HW), generator=gen)
    if ignore < 0 and mode == 0:
        y[torch.rand((B, HW), generator=gen) < 0.1] = ignore
    flat = y.view(-1)
    n = flat.numel()
    if n >= 4:
        flat[0], flat[n // 2], flat[n - 1] = 0, C - 1, C // 2
    flat[min(1, n - 1)] = 1            # (at least one valid pixel when 0 is the ignore index)
    return y


def _setup(B, C, HW, mode, ignore, gamma, smooth, alpha, rsum, scale=2.0, seed=0, labels=None, logits=None):
    c = Case(seed)
    lg = c.t("logits", (B, C, HW), scale=scale) if logits is None else c.t("logits", (B, C, HW), logits)
    y = _labels(B, C, HW, mode, ignore, c.gen) if labels is None else labels
    lab = c.t("labels", (B, HW), y, "i64")
    al = c.t("alpha", (C,), _distinct_alpha(C, c.gen)) if alpha else None
    acc = c.t("acc", (2,), torch.tensor([float("nan"), float("nan")], dtype=torch.float64), "f64")      # (the forward must set both)
    loss = c.t("loss", (1,), "nan")
    gout = c.t("gout", (1,), torch.tensor([1.7]))
    dl = c.t("dlogits", (B, C, HW), "nan")
    common = dict(B=B, C=C, HW=HW, MODE=mode, IGNORE=ignore, REDUCE_SUM=rsum, GAMMA=gamma, SMOOTH=smooth)
    fwd = ("LOSS_FWD", dict(LOGITS=lg, LABELS=lab, ALPHA=al, LOSS=loss, ACC=acc, **common))
    bwd = ("LOSS_BWD", dict(LOGITS=lg, LABELS=lab, ALPHA=al, ACC=acc, GOUT=gout, DLOGITS=dl, **common))
    return c, fwd, bwd


def _fwd_bwd(B, C, HW, mode, ignore, gamma, smooth, alpha, rsum, what="", **kw):
    """forward, then the backward on the ACC the forward left; both against both oracles"""
    c, fwd, bwd = _setup(B, C, HW, mode, ignore, gamma, smooth, alpha, rsum, **kw)
    bufs = _execute(c, [fwd, bwd])
    _check_value(c, bufs, C, mode, what)
    _check_grad(c, bufs, C, what)
    return c, bufs


# ---------------------------------------------------------------------------------------------------------------
# class counts: loss_{fwd,bwd}_kernel<2..8> and the run-time form <0> at 9, 13, 23 (the cnes-full label map) and 64
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["ce", "focal"])
@pytest.mark.parametrize("C", [2, 3, 4, 5, 6, 7, 8, 9, 13, 23, 64])
def test_every_class_count(C, mode):
    _fwd_bwd(2, C, 561, mode, 0, 2.0, 0.1, True, 0, what="ce" if mode == 0 else "focal", seed=100 + C)


@pytest.mark.parametrize("kind", ["LOSS_FWD", "LOSS_BWD"])
@pytest.mark.parametrize("C", [1, 65])
def test_class_count_outside_2_to_64_is_refused(C, kind):
    c, fwd, bwd = _setup(2, C, 16, 1, 0, 2.0, 0.0, False, 0, labels=torch.zeros(2, 16, dtype=torch.int64))
    with pytest.raises(_lib.S2kError, match=rf"s2k error -22: op 0 \({kind}\): loss: unsupported shape C={C}$"):     # S2K_EINVAL: nothing is launched
        _execute(c, [fwd if kind == "LOSS_FWD" else bwd], oracle=False)


# ---------------------------------------------------------------------------------------------------------------
# options, by pairs: every value of every option meets every value of every other one at least once (gamma and the sum
# reduction are focal options; in CE mode the kernel must ignore them, as the oracle does)
# ---------------------------------------------------------------------------------------------------------------
OPTIONS = [  # mode, ignore, gamma, smoothing, alpha, reduce-sum
    (1, 0, 0.0, 0.0, False, 0), (1, -100, 0.0, 0.1, True, 1), (1, 0, 0.5, 0.1, True, 0), (1, -100, 0.5, 0.0, False, 1),
    (1, 0, 1.0, 0.0, True, 1), (1, -100, 1.0, 0.1, False, 0), (1, 0, 2.0, 0.1, False, 1), (1, -100, 2.0, 0.0, True, 0),
    (1, 0, 3.0, 0.0, True, 0), (1, -100, 3.0, 0.1, False, 1),
    (0, 0, 0.0, 0.0, False, 0), (0, -100, 2.0, 0.1, True, 1), (0, 0, 1.0, 0.1, True, 0), (0, -100, 0.5, 0.0, False, 1),
    (0, 0, 3.0, 0.0, True, 1), (0, -100, 0.0, 0.1, False, 0)]


def test_option_table_covers_every_pair():
    values = [(0, 1), (0, -100), (0.0, 0.5, 1.0, 2.0, 3.0), (0.0, 0.1), (False, True), (0, 1)]
    for i in range(6):
        for j in range(i + 1, 6):
            seen = {(row[i], row[j]) for row in OPTIONS}
            assert seen == {(a, b) for a in values[i] for b in values[j]}, (i, j)


@pytest.mark.parametrize("C", [4, 23])
@pytest.mark.parametrize("mode,ignore,gamma,smooth,alpha,rsum", OPTIONS)
def test_option_pairs(mode, ignore, gamma, smooth, alpha, rsum, C):
    _fwd_bwd(2, C, 561, mode, ignore, gamma, smooth, alpha, rsum, what=f"options {(mode, ignore, gamma, smooth, alpha, rsum)}", seed=200 + C)


def test_backward_on_a_supplied_acc():
    """the earlier form of the backward test: ACC[1] is the true weight sum, computed here, not the forward's"""
    B, C, HW = 2, 23, 561
    c, fwd, bwd = _setup(B, C, HW, 0, 0, 0.0, 0.1, True, 0, seed=31)
    y, w = c.items["labels"][1], c.items["alpha"][1]
    c.items["acc"] = (c.items["acc"][0], torch.tensor([0.0, float(w[y][y != 0].double().sum())], dtype=torch.float64))
    _check_grad(c, _execute(c, [bwd]), C, "supplied ACC")


# ---------------------------------------------------------------------------------------------------------------
# the grid-stride loop: pixel_blocks() caps the grid at cdiv(1024, B) blocks of 256 threads per sample
# ---------------------------------------------------------------------------------------------------------------
STRIDE_SHAPES = [(600, 3, 700),      # 2 blocks per sample: 512 threads, the second trip covers 188 of them
                 (1100, 2, 300),     # 1 block per sample, two trips
                 (3, 5, 100000)]     # 342 blocks: 87,552 threads, a partial second trip


@pytest.mark.parametrize("mode", [0, 1], ids=["ce", "focal"])
@pytest.mark.parametrize("B,C,HW", STRIDE_SHAPES)
def test_grid_stride_second_trip(B, C, HW, mode):
    _fwd_bwd(B, C, HW, mode, 0, 2.0, 0.1, True, 0, what=f"grid-stride {(B, C, HW)}", seed=300)


@pytest.mark.parametrize("mode", [0, 1], ids=["ce", "focal"])
@pytest.mark.parametrize("HW", [1, 63, 64, 65, 255, 257])
def test_small_and_ragged_planes(HW, mode):
    _fwd_bwd(3, 6, HW, mode, 0, 2.0, 0.1, True, 0, what=f"HW={HW}", seed=400 + HW)


# ---------------------------------------------------------------------------------------------------------------
# saturated pixels: in f32 a pixel whose winning logit leads by more than ~17 has ce == 0 and pt == 1 exactly (om <= 0 in the
# backward); one whose label lost by more than 20 has pt < 2^-28 and om == 1
# ---------------------------------------------------------------------------------------------------------------
def _saturated_inputs(C, seed):
    """logits at scale 30; 70 % of the pixels carry the winning class as their label, the others a random one"""
    gen = torch.Generator().manual_seed(seed)
    B, HW = 2, 561
    lg = torch.randn((B, C, HW), generator=gen) * 30.0
    y = torch.randint(0, C, (B, HW), generator=gen)
    win = torch.rand((B, HW), generator=gen) < 0.7
    y = torch.where(win, lg.argmax(1), y)
    # the unsmoothed ce is what saturates (smoothing adds eps / C * sum_c -logp[c], far from 0 at this scale)
    ce, _, valid = losses_ref._per_pixel_ce(lg.unsqueeze(-1), y.unsqueeze(-1), None, 0.0, 0)
    n = int(valid.sum())
    assert int(((ce == 0) & valid).sum()) >= n // 10, "too few pixels with ce == 0 in f32: the saturated branch is not reached"
    assert int((ce > 20).sum()) >= n // 10, "too few pixels with ce > 20"
    return B, HW, lg, y


# gamma 0.5 without smoothing is left out at this scale: the reference's own f32 gradient is NaN there (autograd forms
# 0.5 * om^-0.5 * 0 with om == 0) while the kernel returns 0 for such a pixel (parity notes).  With smoothing 0.1 the
# same gamma is finite (ce > 0 everywhere) and stays in.
SATURATED = [(g, s) for g in (0.0, 1.0, 2.0, 3.0) for s in (0.0, 0.1)] + [(0.5, 0.1)]


@pytest.mark.parametrize("C", [4, 23])
@pytest.mark.parametrize("gamma,smooth", SATURATED)
def test_saturated_pixels(gamma, smooth, C):
    B, HW, lg, y = _saturated_inputs(C, 500 + C)
    _fwd_bwd(B, C, HW, 1, 0, gamma, smooth, True, 0, what=f"saturated gamma={gamma} smoothing={smooth}", seed=500 + C, logits=lg, labels=y)


@pytest.mark.parametrize("C", [4, 23])
def test_saturated_pixel_with_gamma_0_keeps_its_cross_entropy_gradient(C):
    """With gamma = 0 the focal term is alpha[y] * ce, so a saturated pixel still has d/dx[c] = alpha[y] * softmax[c] for the classes
    that lost - values below 4e-8 of the tensor's max, which no bar relative to a max can see.  They are compared element by
    element with float64 instead.  Bound: softmax[c] = expf(x[c] - lse); lse and the difference are each rounded once at a
    magnitude below 256 (logits at scale 30), i.e. by at most 2^-16 = 1.5e-5 each, which is the relative error of the
    exponential; expf adds ~1e-7.  3.1e-5 in all; the bar is 1e-4.  The winning class itself is left out (its softmax - 1 is
    exactly 0 in f32 and -sum of the others in float64), so are values that f32 cannot hold as normal numbers."""
    B, HW, lg, y = _saturated_inputs(C, 500 + C)
    assert lg.abs().max() < 200      # (so that |x[c] - lse| < 256 as the bound assumes)
    c, fwd, bwd = _setup(B, C, HW, 1, 0, 0.0, 0.0, True, 1, seed=500 + C, logits=lg, labels=y)
    bufs = _execute(c, [fwd, bwd])
    got, want = _read(c, bufs[0], "dlogits").double(), _read(c, bufs[2], "dlogits", wide=True)
    ce, _, valid = losses_ref._per_pixel_ce(lg.unsqueeze(-1), y.unsqueeze(-1), None, 0.0, 0)
    sat = ((ce == 0) & valid).squeeze(-1).unsqueeze(1).expand(B, C, HW)
    lost = torch.ones(B, C, HW, dtype=torch.bool).scatter_(1, y.unsqueeze(1), False)
    sel = sat & lost & (want.abs() > 1e-30)
    assert int(sel.sum()) > 100
    err = ((got[sel] - want[sel]).abs() / want[sel].abs()).max().item()
    print(f"loss_bwd_kernel{_form(C)} saturated, gamma 0: losing classes' gradient, worst element-wise rel err {err:.2e} (float64)")
    assert err < 1e-4, err


# ---------------------------------------------------------------------------------------------------------------
# whole-sample ignore, labels outside [0, C)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["ce", "focal"])
@pytest.mark.parametrize("C", [4, 23])
def test_whole_sample_ignored(C, mode):
    B, HW = 2, 561
    gen = torch.Generator().manual_seed(600 + C)
    y = _labels(B, C, HW, mode, 0, gen)
    y[0] = 0
    c, bufs = _fwd_bwd(B, C, HW, mode, 0, 2.0, 0.1, True, 0, what="sample 0 ignored", seed=600 + C, labels=y)
    got = _read(c, bufs[0], "dlogits")
    assert torch.equal(got[0], torch.zeros_like(got[0])) and got[1].abs().max() > 0


@pytest.mark.parametrize("ignore", [0, -100])
@pytest.mark.parametrize("C", [4, 23])
def test_labels_outside_the_classes_are_skipped(C, ignore):
    """labels 255, -1 and C contribute nothing and get a zero gradient, exactly as if they carried the ignore index (focal mode: no
    denominator that could differ between the two runs)"""
    B, HW = 2, 561
    gen = torch.Generator().manual_seed(700 + C)
    y = torch.randint(0, C, (B, HW), generator=gen)
    out = torch.rand((B, HW), generator=gen) < 0.1
    bad = torch.tensor([255, -1, C])[torch.randint(0, 3, (B, HW), generator=gen)]
    assert all(int((out & (bad == v)).sum()) > 0 for v in (255, -1, C))
    res = []
    for labels in (torch.where(out, bad, y), torch.where(out, torch.full_like(y, ignore), y)):
        c, fwd, bwd = _setup(B, C, HW, 1, ignore, 2.0, 0.1, True, 0, seed=700 + C, labels=labels)
        got = _execute(c, [fwd, bwd], oracle=False)[0]
        res.append((_read(c, got, "loss").clone(), _read(c, got, "dlogits").clone()))
    (loss_a, d_a), (loss_b, d_b) = res
    assert torch.isfinite(d_a).all() and d_a.abs().max() > 0
    assert torch.equal(d_a.view(torch.int32), d_b.view(torch.int32)), "dlogits differ from the run with the ignore index in their place"
    assert torch.equal(d_a.transpose(1, 2)[out], torch.zeros(int(out.sum()), C))
    assert abs(loss_a.item() - loss_b.item()) <= 1e-6 * abs(loss_b.item()), (loss_a.item(), loss_b.item())


# ---------------------------------------------------------------------------------------------------------------
# ARGMAX
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,HW", [(2, 2, 777), (2, 23, 777), (2, 64, 777)] + STRIDE_SHAPES)
def test_argmax_exact(B, C, HW):
    """rounded logits: exact ties in more than a tenth of the pixels, the first maximum must win; sample 0's first 50 pixels are -inf in every class
    (class 0 wins), and class plane C - 1 of the last sample is -inf as a whole (never wins)"""
    c = Case(800 + C)
    lg = torch.randn(B, C, HW, generator=c.gen).round()
    lg[0, :, :min(50, HW)] = float("-inf")
    lg[B - 1, C - 1] = float("-inf")
    lt = c.t("logits", (B, C, HW), lg)
    mask = c.t("mask", (B, HW), torch.full((B, HW), -1), "i64")
    got, want, _ = _execute(c, [("ARGMAX", dict(LOGITS=lt, MASK=mask, B=B, C=C, HW=HW))])
    got, want = _read(c, got, "mask"), _read(c, want, "mask")
    top = lg.max(1, keepdim=True).values
    assert int(((lg == top).sum(1) > 1).sum()) > B * HW // 10, "ties are not common in this draw"
    assert torch.equal(got, want)
    assert int(got[0, :min(50, HW)].abs().max()) == 0 and int((got[B - 1] == C - 1).sum()) == 0


# ---------------------------------------------------------------------------------------------------------------
# the product surface at 23 classes
# ---------------------------------------------------------------------------------------------------------------
def _product_inputs():
    gen = torch.Generator().manual_seed(900)
    B, C, H, W = 2, 23, 24, 40
    lg = (torch.randn((B, C, H, W), generator=gen) * 2.0)
    y = torch.randint(0, C, (B, H, W), generator=gen)
    w = _distinct_alpha(C, gen)
    return lg, y, w


@pytest.mark.parametrize("name", ["focal_masked_weighted_smoothed", "focal_plain_sum", "ce_masked_weighted_smoothed", "ce_plain"])
def test_product_losses_at_23_classes(name):
    from s2lc_amd.losses import CrossEntropyLoss, FocalLoss

    lg, y, w = _product_inputs()
    fn, ref = {
        "focal_masked_weighted_smoothed": (FocalLoss(w, 2.0, 0.1, ignore_index=0), lambda l: losses_ref.focal(l, y, w, 2.0, 0.1, 0)),
        "focal_plain_sum": (FocalLoss(torch.ones(23), 0.5, 0.0, ignore_index=-100, reduce_type="sum"),
                            lambda l: losses_ref.focal(l, y, torch.ones(23), 0.5, 0.0, -100, "sum")),
        "ce_masked_weighted_smoothed": (CrossEntropyLoss(weight=w, label_smoothing=0.1, ignore_index=0),
                                        lambda l: losses_ref.cross_entropy(l, y, w, 0.1, 0)),
        "ce_plain": (CrossEntropyLoss(ignore_index=-100), lambda l: losses_ref.cross_entropy(l, y, None, 0.0, -100)),
    }[name]
    l = lg.to(DEV).requires_grad_(True)
    v = fn(l, y.to(DEV))
    (v * 1.7).backward()
    l64 = lg.double().requires_grad_(True)
    v64 = ref(l64)
    (g64,) = torch.autograd.grad(v64 * 1.7, l64)
    got = l.grad.cpu().reshape(2, 23, -1)
    ev = abs(v.item() - v64.item()) / abs(v64.item())
    eg, ep = _rel(got, g64.reshape(2, 23, -1)), _rel(got, g64.reshape(2, 23, -1), dims=2)
    print(f"{name} at 23 classes: value rel err {ev:.2e}, gradient {eg:.2e} whole / {ep:.2e} worst plane (float64)")
    assert ev < BAR_VALUE and eg < BAR_GRAD and ep < BAR_GRAD, (ev, eg, ep)


def test_class_mask_and_metrics_at_23_classes():
    from s2lc_amd.losses import class_mask
    from s2lc_amd.metrics import SegMetrics

    lg, y, _ = _product_inputs()
    lg = lg.round()                                 # ties
    pred = class_mask(lg.to(DEV))
    assert torch.equal(pred.cpu(), losses_ref.class_mask(lg))
    m = SegMetrics(23, ignore_index=0, device=DEV)
    m.update(pred, y.to(DEV))
    m.update(pred, y.to(DEV))
    torch.cuda.synchronize()
    want = 2 * torch.bincount((y * 23 + pred.cpu()).reshape(-1), minlength=23 * 23)
    assert torch.equal(m.hist.cpu(), want)
    assert len(set(pred.cpu().reshape(-1).tolist())) == 23 and len(set(y.reshape(-1).tolist())) == 23
