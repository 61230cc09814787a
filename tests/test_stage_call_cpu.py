"""CPU: the standalone stage calls (stage_call.StageCall) bind what the tensors say.  The product's own call builders are fed CPU
tensors, their packed records are interpreted by oracle/ops_ref.py over {slot: that tensor's bytes} and compared with plain torch;
then the binding rules, the packed constants / scratch, `rebind`, and where base names may still be spelled out.  No GPU and no built
library is needed: only `run()` refuses CPU tensors.

Float tolerance of the loss cases: interpreter and torch both work in float32 but order the operations differently; 16 pixels x 3
classes, a handful of roundings and two transcendentals per term bound the difference by a few tens of ulps (1.2e-7 each): 1e-5."""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import s2lc_amd  # noqa: F401
from oracle import ops_ref
from s2lc_amd import losses, metrics
from s2lc_amd.data.gpu_pipeline import tile_prep_call
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan.program import ALIGN, NULL
from s2lc_amd.stage_call import StageCall, cached

PKG = Path(s2lc_amd.__file__).resolve().parent


def interpret(call: StageCall) -> None:
    """run the call's packed records on the host, every base slot being the bytes of the tensor bound to it"""
    ops_ref.run_program(call.pack(), {i: t.view(-1).view(torch.uint8) for i, t in enumerate(call.tensors)}, D)


def field(call: StageCall, kind: str, name: str, rec: int = 0) -> int:
    return int(call.pack()[rec]["t"][D.slot(kind, name)[1]])


# ---- 1. records built through the binder mean what the tensors say -----------------------------------------------------------------
@pytest.mark.parametrize("with_labels", [True, False])
def test_tile_prep_call_is_crop_flip_normalise(with_labels):
    N, C, H, W, S = 3, 2, 8, 12, 4
    g = torch.Generator().manual_seed(1)
    raw = torch.randint(-2000, 9000, (N, C, H, W), generator=g, dtype=torch.int32).to(torch.int16)
    labels = torch.randint(0, 24, (N, H, W), generator=g, dtype=torch.int32).to(torch.uint8) if with_labels else None
    par = torch.tensor([[0, 0, 0, 0], [2, H - S, W - S, 1], [1, 2, 3, 2], [2, 0, W - S, 3], [0, H - S, 0, 1]], dtype=torch.int32)
    norm = torch.tensor([[1234.5, 987.25], [1 / 611.0, 1 / 377.0]], dtype=torch.float32)
    lut = (torch.arange(256, dtype=torch.int32) * 7) % 5
    x = torch.full((len(par), C, S, S), float("nan"))
    y = torch.full((len(par), S, S), -7, dtype=torch.int64) if with_labels else None
    call = tile_prep_call(raw, labels, par, norm, lut, x, y)
    interpret(call)
    assert len(call.tensors) == (7 if with_labels else 4) <= len(D.BASES)
    for name in ("LABELS", "LUT", "Y"):
        assert (field(call, "TILE_PREP", name) == NULL) == (not with_labels)
    for b, (tile, y0, x0, fl) in enumerate(par.tolist()):
        dims = [d for d, bit in ((-1, 1), (-2, 2)) if fl & bit]
        img = raw[tile, :, y0:y0 + S, x0:x0 + S].to(torch.float32).flip(dims) - norm[0].view(C, 1, 1)      # two separately rounded steps
        assert torch.equal(x[b], img * norm[1].view(C, 1, 1))
        if with_labels:
            assert torch.equal(y[b], lut[labels[tile, y0:y0 + S, x0:x0 + S].long()].long().flip(dims))


def torch_loss(logits, y, alpha, mode, ignore, gamma, smooth):
    if mode == 0:
        return F.cross_entropy(logits, y, weight=alpha, ignore_index=ignore, label_smoothing=smooth)
    ce = F.cross_entropy(logits, y, ignore_index=ignore, label_smoothing=smooth, reduction="none")
    a = torch.ones(logits.shape[1]) if alpha is None else alpha
    return (a[y] * (1.0 - torch.exp(-ce)) ** gamma * ce).mean()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("with_alpha", [True, False])
def test_loss_calls_match_torch(mode, with_alpha):
    B, C, H, W = 2, 3, 2, 4
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(B, C, H, W, generator=g) * 2
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[0, 0, 0], y[1, 1, 2] = 0, 0                       # IGNORE = 0 occurs
    alpha = torch.tensor([0.2, 0.5, 0.3]) if with_alpha else None
    gamma, smooth = (0.0, 0.1) if mode == 0 else (2.0, 0.0)
    common = dict(B=B, C=C, HW=H * W, MODE=mode, IGNORE=0, REDUCE_SUM=0, GAMMA=gamma, SMOOTH=smooth)
    scratch = torch.zeros(32, dtype=torch.uint8)        # {f64 num, f64 den, f32 loss}
    fwd = losses.loss_call(logits, y, alpha, scratch, **common)
    interpret(fwd)
    # one uint8 tensor, one slot, three typed refs into it
    assert field(fwd, "LOSS_FWD", "ACC") >> 56 == field(fwd, "LOSS_FWD", "LOSS") >> 56 and field(fwd, "LOSS_FWD", "LOSS") & 0xFF == 16
    assert (field(fwd, "LOSS_FWD", "ALPHA") == NULL) == (not with_alpha)
    lg = logits.clone().requires_grad_(True)
    want = torch_loss(lg, y, alpha, mode, 0, gamma, smooth)
    got = scratch[16:20].view(torch.float32)
    assert torch.allclose(got, want.detach().reshape(1), rtol=1e-5, atol=0)
    gout, dlogits = torch.tensor([0.5]), torch.full_like(logits, float("nan"))
    bwd = losses.loss_call(logits, y, alpha, scratch, gout, dlogits, **common)
    assert field(bwd, "LOSS_BWD", "ACC") & 0xFF == 0
    interpret(bwd)
    (grad,) = torch.autograd.grad(want, lg)
    assert torch.allclose(dlogits, 0.5 * grad, rtol=1e-5, atol=1e-5 * float(grad.abs().max()))


def test_argmax_and_confusion_calls_match_torch():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2, 3, 2, 4, generator=g)
    logits[0, 1, 0, 0] = logits[0, 2, 0, 0] = 9.0       # a tie: the first maximum wins, as torch's argmax
    mask = torch.full((2, 2, 4), -1, dtype=torch.int64)
    interpret(losses.argmax_call(logits, mask))
    assert torch.equal(mask, logits.argmax(dim=1))
    labels = torch.randint(0, 3, (2, 2, 4), generator=g)
    hist = torch.arange(9, dtype=torch.int64)           # CONFUSION accumulates
    interpret(metrics.confusion_call(mask, labels, hist, 3))
    assert torch.equal(hist, torch.arange(9) + torch.bincount((labels * 3 + mask).reshape(-1), minlength=9))


# ---- 2. binding rules ----------------------------------------------------------------------------------------------------------------
def test_binding_rules():
    call = StageCall()
    a, b = torch.zeros(4, 6), torch.zeros(10, dtype=torch.int64)
    ra, rb = call.t(a), call.t(b, (2, 5))
    assert (ra.base, ra.off, ra.shape, ra.dtype) == (0, 0, (4, 6), "f32") and (rb.base, rb.shape, rb.dtype) == (1, (2, 5), "i64")
    assert call.t(a, (24,)).base == 0 and len(call.tensors) == 2                    # the same tensor: the same slot
    assert call.t(None) is None
    piece = a[1:3]                                                                   # a slice binds at its own address
    rp = call.t(piece)
    assert (rp.base, rp.off, rp.shape) == (2, 0, (2, 6)) and call.bases.arr[2] == a.data_ptr() + 24 and call.bases.arr[0] == a.data_ptr()
    raw = torch.zeros(32, dtype=torch.uint8)                                         # raw bytes: any dtype, at a byte offset
    assert (call.t(raw, (2,), "f64").off, call.t(raw, (1,), "f32", 16).off, call.t(raw, (1,), "f32", 16).base) == (0, 16, 3)
    assert all(t is u for t, u in zip(call.tensors, (a, b, piece, raw)))             # kept alive, in slot order


def test_binding_errors_are_raised_on_the_host():
    call = StageCall()
    a = torch.zeros(4, 6)
    call.t(a)
    with pytest.raises(ValueError, match="contiguous"):
        call.t(a.t())
    with pytest.raises(ValueError, match="different devices"):                      # decided before any data_ptr(): a meta tensor has none
        call.t(torch.zeros(4, device="meta"))
    with pytest.raises(ValueError, match="dtype"):
        call.t(torch.zeros(4, dtype=torch.float16))
    with pytest.raises(ValueError, match="dtype"):
        call.t(torch.zeros(8, dtype=torch.uint8), (1,), "f16")
    with pytest.raises(ValueError, match="dtype"):
        call.t(a, dtype="i32")                                                      # only uint8 is raw bytes
    raw = torch.zeros(32, dtype=torch.uint8)
    for shape, dtype, off in (((25,), None, 0), ((5,), "f64", 0), ((4,), "f64", 8), ((1,), "f64", 12), ((1,), "f32", -4)):
        with pytest.raises(ValueError, match="does not fit"):
            call.t(raw, shape, dtype, off) if dtype else call.t(a, shape)
    assert len(call.tensors) == 1                                                    # a refused tensor takes no slot
    for _ in range(len(D.BASES) - 1):
        call.t(torch.zeros(1))
    with pytest.raises(ValueError, match=f"at most {len(D.BASES)}"):
        call.t(torch.zeros(1))
    with pytest.raises(RuntimeError, match="GPU"):                                   # packing worked; launching needs the GPU
        call.run()


# ---- 3. packed constants and scratch -------------------------------------------------------------------------------------------------
def test_constants_and_scratch():
    assert len(StageCall().image()) == ALIGN and not StageCall().image().any()       # nothing allocated: still ALIGN bytes
    call = StageCall()
    ints, wide = call.const([3, 1, 4, 1, 5], "i32"), call.const(np.array([[1.5, -2.0]]), "f64")
    grid = call.const(range(6), "i64", (2, 3))
    s0, s1 = call.scratch((3, 100), "i64"), call.scratch((2,), "f32")
    refs = (ints, wide, grid, s0, s1)
    assert all(r.off % ALIGN == 0 for r in refs) and [r.off for r in refs] == [0, 256, 512, 0, 2560]
    assert ints.base == wide.base == grid.base != s0.base == s1.base and (grid.shape, s0.shape) == ((2, 3), (3, 100))
    with pytest.raises(ValueError, match="values for a constant"):
        call.const([1, 2, 3], "i32", (2, 2))
    assert len(call.image()) == 3 * ALIGN
    assert call.view(ints).tolist() == [3, 1, 4, 1, 5] and call.view(wide).tolist() == [[1.5, -2.0]]
    assert torch.equal(call.view(grid), torch.arange(6).view(2, 3)) and call.view(grid).dtype == torch.int64
    assert call.view(s0).shape == (3, 100) and not call.view(s0).any() and call.view(s1).dtype == torch.float32
    assert call.tensors[s0.base].numel() == 2560 + ALIGN
    call.view(s1)[0] = 2.5                                                           # a view of the scratch, not a copy
    assert call.tensors[s1.base][2560:2564].view(torch.float32).item() == 2.5
    with pytest.raises(RuntimeError, match="packed"):
        call.const([1], "i32")


# ---- 4. rebind -----------------------------------------------------------------------------------------------------------------------
def test_rebind_swaps_the_tensor_and_keeps_the_records():
    call = StageCall()
    logits, mask = torch.zeros(2, 3, 8), torch.zeros(2, 8, dtype=torch.int64)
    call.add("ARGMAX", LOGITS=call.t(logits), MASK=(ref := call.t(mask)), B=2, C=3, HW=8)
    with pytest.raises(ValueError, match="packed call"):
        call.rebind(ref, torch.zeros(2, 8, dtype=torch.int64))
    before = call.pack().tobytes()
    other = torch.zeros(3, 8, dtype=torch.int64)                                     # more bytes than needed: accepted
    call.rebind(ref, other)
    assert call.pack().tobytes() == before
    assert call.bases.arr[ref.base] == other.data_ptr() != mask.data_ptr() and call.tensors[ref.base] is other
    with pytest.raises(RuntimeError, match="packed"):                                # a packed call takes no further tensor or record
        call.t(torch.zeros(1))
    with pytest.raises(RuntimeError, match="packed"):
        call.add("ARGMAX", B=1)
    with pytest.raises(ValueError, match="rebind"):
        call.rebind(ref, torch.zeros(3, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="rebind"):
        call.rebind(ref, torch.zeros(2, 7, dtype=torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        call.rebind(ref, torch.zeros(8, 4, dtype=torch.int64).t())


def test_cached_call_is_built_once_and_keeps_no_tensor():
    g = torch.Generator().manual_seed(4)
    cache = {}
    first = None
    for _ in range(3):                                                               # every use: its own tensors, the right result
        logits, mask = torch.randn(2, 3, 2, 4, generator=g), torch.full((2, 2, 4), -1, dtype=torch.int64)
        call = cached(cache, losses.argmax_call, logits, mask)
        first = first or (call, call.pack().tobytes())
        assert call is first[0] and call.pack().tobytes() == first[1] and len(cache) == 1
        assert call.tensors[:2] == [logits, mask] and call.bases.arr[1] == mask.data_ptr()
        interpret(call)
        assert torch.equal(mask, logits.argmax(dim=1))
        with pytest.raises(RuntimeError, match="GPU"):
            call.run()
        assert call.tensors == [None, None]                                          # let go of after the launch, or the refusal
    assert cached(cache, losses.argmax_call, torch.zeros(2, 3, 2, 5), torch.zeros(2, 2, 5, dtype=torch.int64)) is not call      # other shapes
    assert len(cache) == 2
    with pytest.raises(ValueError, match="rebind"):                                  # same shapes, another dtype: refused, not misread
        cached(cache, losses.argmax_call, logits, mask.to(torch.int32))
    # a tensor given twice shares one slot: that call is right for this use and must not serve a later one with two tensors
    both = torch.randint(0, 3, (2, 2, 4), generator=g)
    hist, cache = torch.zeros(9, dtype=torch.int64), {}
    interpret(cached(cache, metrics.confusion_call, both, both, hist, C=3))
    assert not cache and torch.equal(hist, torch.bincount(both.reshape(-1) * 4, minlength=9))
    pred = (both + 1) % 3
    call = cached(cache, metrics.confusion_call, pred, both, hist.zero_(), C=3)
    assert len(cache) == 1 and cached(cache, metrics.confusion_call, both, both, hist, C=3) is call      # the other way round is fine
    assert call.bases.arr[0] == call.bases.arr[1] == both.data_ptr()
    interpret(call)
    assert torch.equal(hist, torch.bincount(both.reshape(-1) * 4, minlength=9))


# ---- 5. base names are the engines' vocabulary -----------------------------------------------------------------------------------------
def test_only_the_engines_and_the_binder_spell_out_bases():
    """plan/ is the planner, whose names the engines bind; every other module launches through StageCall"""
    allowed = {"engine.py", "vit_engine.py", "_lib.py", "stage_call.py"}
    found = {str(p.relative_to(PKG)) for p in PKG.rglob("*.py") if p.relative_to(PKG).parts[0] != "plan"
             and any(s in p.read_text() for s in ("D.BASE[", "Bases()"))}
    assert found and found <= allowed, sorted(found - allowed)
