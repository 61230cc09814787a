"""s2k_adam_step (csrc/ew.hip: adam_kernel, adam_scalar_kernel) called directly, on every path it has: the float4 kernel with
each tail length, fewer than four elements, its grid-stride loop (n > 8192 * 256 * 4), and the scalar kernel that takes over
when one of the four pointers is not 16-byte aligned (a slice handed out by ddp.FlatGradReducer.owned() in sharded mode can be),
with its own stride loop (n > 8192 * 256).

Reference: the kernel's formula (adam_one) in float64 from the same f32 inputs, with the bias corrections in double:
  g' = g + wd * p;  m' = m + (1 - b1) (g' - m);  v' = b2 v + (1 - b2) g'^2;  p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps).
m, v and p must agree to 1e-6 of their max (the bar of tests/test_parity_r2_gpu.py).  That bar barely sees the update - it is
about lr of |p| - so the update itself, dp = p_after - p_before formed in float64, is compared with the reference's:
  |dp - dp_ref| <= 2^-23 max|p|   (max over p before and after),
which is what two roundings of p to f32 may cost.  The issue's recipe for a relative term on top - the error that
torch.optim.Adam(foreach=False) in f32 on the CPU leaves beyond that rounding term against the same float64 formula, times 4 -
was measured on these inputs, over every hyper-parameter set below at n = 4099 and n = 1_000_003: torch's whole error is 8e-7
to 3e-6 of max|dp_ref| at lr 1e-2 and step >= 2 (2e-7 to 3e-7 absolute) and stays inside the rounding term (>= 4.7e-7)
everywhere, so the measured excess, and with it the relative term, is 0.
Headroom of the bound that is left: the kernel stores p once (fmaf), at most 2^-24 |p'|; the other 2^-24 max|p| is there for
the arithmetic of the update - m', v', sqrtf, two divisions, the f32 constants: about 7 roundings of 6e-8, 4e-7 relative - on
an update that is at most 0.28 here, i.e. 1.1e-7 absolute against 2.2e-7 to 2.7e-7 available.  Measured on an MI355X: the worst
error is 0.45 of the bound, for both kernels.
What the bound can see is limited by f32 p itself, not by the test: at lr 1e-2 it is 1e-5 of the largest update, at lr 1e-5
0.2 % of it (6 % at step 1, where every update is lr): an update wrong by less than that cannot be told from a rounding of p."""
import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B1, B2, EPS = 0.9, 0.999, 1e-8
GUARD = 64                       # floats before and after each array (256 bytes: keeps the array 16-byte aligned)
STRIDE_N = 8192 * 256 * 4        # elements one pass of adam_kernel's grid covers


def make_inputs(n, step, seed):
    """p ~ N(0, 1).  Gradients: a quarter zeros, a quarter +-1e-6, a quarter +-1e2, a quarter N(0, 1); the first and the last
    element carry -+1e2, so that an element the kernel skipped shows whatever the draw.  m = v = 0 at step 1.  Later steps:
    m ~ 0.1 N(0, 1), v in [1e-4, 2e-2], and wherever the gradient is zero every eighth such element has v = 0 and |m| = 1e-9:
    eps alone is the denominator there."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    kind = rng.integers(0, 4, n)
    sign = rng.choice(np.float32([-1.0, 1.0]), n)
    g = np.select([kind == 0, kind == 1, kind == 2], [np.float32(0.0), sign * np.float32(1e-6), sign * np.float32(1e2)],
                  rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    g[0], g[-1] = -1e2, 1e2
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (0.1 * rng.standard_normal(n)).astype(np.float32)
        v = (1e-4 + 2e-2 * rng.random(n)).astype(np.float32)
        bare = (g == 0) & (rng.integers(0, 8, n) == 0)
        v[bare] = 0.0
        m[bare] = sign[bare] * np.float32(1e-9)
    return p, g, m, v


def reference(p, g, m, v, lr, wd, step):
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    if wd != 0.0:
        g = g + wd * p
    m = m + (1.0 - B1) * (g - m)
    v = B2 * v + (1.0 - B2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - B2 ** step) + EPS
    return p - lr / (1.0 - B1 ** step) * m / denom, m, v


def _rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def _step(n, step, lr, wd, offsets=(0, 0, 0, 0), seed=0):
    """One s2k_adam_step over arrays that start `offsets` floats past a 16-byte boundary, each between two guard bands."""
    host = make_inputs(n, step, seed)
    rng = np.random.default_rng(seed + 1)
    bufs, views = [], []
    for a, off in zip(host, offsets):
        full = rng.integers(0, 2 ** 31 - 1, GUARD + off + n + GUARD, dtype=np.int32).view(np.float32)      # (guards: arbitrary bit patterns)
        full[GUARD + off:GUARD + off + n] = a
        t = torch.from_numpy(full.copy()).to(DEV)
        assert t.data_ptr() % 16 == 0
        bufs.append((full, t))
        views.append(t[GUARD + off:GUARD + off + n])
    assert [v.data_ptr() % 16 for v in views] == [4 * o % 16 for o in offsets]
    L = _lib.lib()
    _lib.check(L.s2k_adam_step(*(v.data_ptr() for v in views), n, lr, B1, B2, EPS, wd, step, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = []
    for (full, t), off in zip(bufs, offsets):
        after = t.cpu().numpy()
        lo, hi = GUARD + off, GUARD + off + n
        assert np.array_equal(after[:lo].view(np.int32), full[:lo].view(np.int32)), "wrote before the array"
        assert np.array_equal(after[hi:].view(np.int32), full[hi:].view(np.int32)), "wrote past the array"
        out.append(after[lo:hi])
    p1, g1, m1, v1 = out
    p0, g0, m0, v0 = host
    assert np.array_equal(g1.view(np.int32), g0.view(np.int32)), "the gradient was modified"
    pr, mr, vr = reference(p0, g0, m0, v0, lr, wd, step)
    errs = {"m": _rel(m1, mr), "v": _rel(v1, vr), "p": _rel(p1, pr)}
    dp, dpr = p1.astype(np.float64) - p0.astype(np.float64), pr - p0.astype(np.float64)
    bound = 2.0 ** -23 * float(max(np.abs(p0).max(), np.abs(pr).max()))      # (max |p| over before and after: with a handful of elements lr can be of |p|'s size)
    errs["dp"] = float(np.abs(dp - dpr).max())
    kernel = "adam_kernel" if not any(offsets) else "adam_scalar_kernel"
    print(f"{kernel} n={n} step={step} lr={lr} wd={wd} offsets={offsets}: rel err m {errs['m']:.2e} v {errs['v']:.2e} p {errs['p']:.2e}; "
          f"update: abs err {errs['dp']:.2e} = {errs['dp'] / np.abs(dpr).max():.2e} of max |dp|, bound {bound:.2e}")
    assert np.isfinite(p1).all() and np.isfinite(m1).all() and np.isfinite(v1).all()
    assert max(errs["m"], errs["v"], errs["p"]) < 1e-6, errs
    assert errs["dp"] <= bound, (errs, bound)
    return errs


HYPER = [(step, lr, wd) for step in (1, 2, 1000, 100000) for lr in (1e-2, 1e-5) for wd in (0.0, 0.05)]


@pytest.mark.parametrize("step,lr,wd", HYPER)
def test_hyper_parameters(step, lr, wd):
    _step(4099, step, lr, wd, seed=step)                       # float4 kernel, 5 blocks, tail of 3
    _step(4099, step, lr, wd, offsets=(1, 1, 1, 1), seed=step)      # scalar kernel


@pytest.mark.parametrize("n", [1, 2, 3, 4, 1024, 1025, 1026, 1027, 70001, 70002, 70003])
@pytest.mark.parametrize("step,lr,wd", [(1, 1e-2, 0.05), (1000, 1e-5, 0.0)])
def test_float4_kernel_tails_and_fewer_than_four_elements(n, step, lr, wd):
    _step(n, step, lr, wd, seed=n)


def test_float4_kernel_stride_loop():
    _step(STRIDE_N + 1027, 2, 1e-2, 0.05, seed=5)


@pytest.mark.parametrize("offsets", [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1), (1, 2, 3, 1)],
                         ids=["p", "g", "m", "v", "all", "all-differently"])
@pytest.mark.parametrize("step,lr,wd", [(1, 1e-2, 0.05), (1000, 1e-5, 0.0)])
def test_scalar_kernel_when_a_pointer_is_not_16_byte_aligned(offsets, step, lr, wd):
    _step(1000, step, lr, wd, offsets=offsets, seed=11)
    _step(3, step, lr, wd, offsets=offsets, seed=12)


def test_scalar_kernel_stride_loop():
    _step(2_200_003, 2, 1e-2, 0.05, offsets=(1, 1, 1, 1), seed=6)


@pytest.mark.parametrize("n,step", [(0, 1), (16, 0), (0, 0), (16, -1)])
def test_bad_arguments_are_refused(n, step):
    t = [torch.ones(16, device=DEV) for _ in range(4)]
    with pytest.raises(_lib.S2kError, match="s2k error -22: adam: bad args"):      # S2K_EINVAL: nothing is launched
        _lib.check(_lib.lib().s2k_adam_step(*(a.data_ptr() for a in t), n, 1e-2, B1, B2, EPS, 0.0, step, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert all(bool((a == 1).all()) for a in t)
