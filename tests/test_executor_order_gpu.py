"""GPU: the fork / join behaviour of `s2k_program_run` itself (csrc/s2k_api.hip), on multi-record programs over two streams.

Single-record tests never run the side stream, and model-level bars pass a stale read of 1e-4.  Here every scenario is correct only
if one named wait exists: a PRODUCER - a run of AXPY records over one large tensor - is still running when the CONSUMER, one AXPY
that reads it, could start on the other stream.  AXPY and MEMSET are one rounding per element, so the arena the GPU leaves is
compared BIT FOR BIT with the emulator's record-by-record run on the same bytes (oracle/ops_ref.py).

Sizing is measured, not assumed (`sizing`): the producer run must last at least RATIO = 50 times a 64-float AXPY record, both timed
with `_lib.profile_ops`, so that a dropped wait shows as a stale read instead of hiding behind launch latency.  DESIGN.md (stream
ordering) records the measured times and what a join left off on purpose did.  No test here asserts that a race is observed."""
import math

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import detgen, losses_ref, ops_ref
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan.program import Program
from tests.plan_harness import emulate, make_bases
from tests.test_dw_chain_gpu import FUSED, OUTS, _chain, _compare, _families
from tests.test_ops_gpu import WS, Case

pytestmark = pytest.mark.gpu

S, J = D.FLAG_SIDE, D.FLAG_JOIN
RATIO = 50                  # producer run / one 64-float AXPY record
N_START = 1 << 24           # floats per large tensor, doubled while the producer would need more than K_MAX records
N_MAX = 1 << 25             # four large tensors: 512 MiB, the arena stays under 1 GiB
K_MAX = 24


def _axpy_ms(n_floats: int, records: int) -> float:
    """median device time of one AXPY record over n_floats (after a warm-up run of the same program)"""
    from s2lc_amd import _lib

    c = Case(1)
    a, b = c.t("a", (n_floats,), "zeros"), c.t("b", (n_floats,), "zeros")
    prog = Program()
    for _ in range(records):
        prog.add("AXPY", X=a, Y=b, COUNT=n_floats)
    packed = prog.pack()
    bases = _lib.Bases().set("WS", c.image().cuda())
    st = torch.cuda.current_stream().cuda_stream
    _lib.profile_ops(packed, bases, st)
    ms = _lib.profile_ops(packed, bases, st)
    torch.cuda.synchronize()
    return float(np.median(ms))


def measure_sizing():
    """-> dict(n, k, small_ms, big_ms, producer_ms): tensor length, producer records and the measured times"""
    small = _axpy_ms(64, 9)
    n = N_START
    while True:
        big = _axpy_ms(n, 5)
        k = max(2, math.ceil(RATIO * small / big * 1.25))          # a quarter more than the ratio asks for
        if k <= K_MAX or n >= N_MAX:
            break
        n *= 2
    return dict(n=n, k=min(k, K_MAX), small_ms=small, big_ms=big, producer_ms=min(k, K_MAX) * big)


@pytest.fixture(scope="module")
def sizing():
    z = measure_sizing()
    print(f"sizing: 64-float AXPY {z['small_ms'] * 1e3:.1f} us, {z['n']}-float AXPY {z['big_ms'] * 1e3:.1f} us, producer {z['k']} records = "
          f"{z['producer_ms'] * 1e3:.1f} us = {z['producer_ms'] / z['small_ms']:.0f} x the small record")
    assert z["producer_ms"] >= RATIO * z["small_ms"], z
    return z


def scene(n, names, seed=3):
    c = Case(seed)
    return c, {name: c.t(name, (n,)) for name in names}


def axpy(prog, x, y, n, flags=0, times=1):
    for _ in range(times):
        prog.add("AXPY", X=x, Y=y, COUNT=n, _flags=flags)


def run_calls(c, packed, calls=None):
    """the records on the GPU, as the given calls [begin, end) on one stream -> (GPU arena, emulator arena), both as CPU bytes"""
    from s2lc_amd import _lib

    cpu = c.image()
    gpu = cpu.cuda()
    bases = _lib.Bases().set("WS", gpu)
    st = torch.cuda.current_stream().cuda_stream
    for a, b in calls or [(0, len(packed))]:
        _lib.run(packed, bases, st, a, b)
    torch.cuda.synchronize()
    ops_ref.run_program(packed, {WS: cpu}, D)
    return gpu.cpu(), cpu


def mismatches(c, got, ref):
    """{tensor: number of floats that differ}"""
    out = {}
    for name in c.items:
        a, b = c.read(got, name).view(torch.int32), c.read(ref, name).view(torch.int32)
        bad = int((a != b).sum())
        if bad:
            out[name] = bad
    return out


def check_exact(c, packed, calls=None, what=""):
    got, ref = run_calls(c, packed, calls)
    assert torch.equal(got, ref), f"{what}: the arena differs from the emulator's: {mismatches(c, got, ref)}"


def test_fork_waits_for_the_main_producer(sizing):
    n, k = sizing["n"], sizing["k"]
    c, t = scene(n, "abc")
    prog = Program()
    axpy(prog, t["a"], t["b"], n, times=k)
    axpy(prog, t["b"], t["c"], n, S)
    check_exact(c, prog.pack(), what="fork")


def test_join_waits_for_the_side_producer(sizing):
    n, k = sizing["n"], sizing["k"]
    c, t = scene(n, "abc")
    prog = Program()
    axpy(prog, t["a"], t["b"], n, S, times=k)
    axpy(prog, t["b"], t["c"], n, J)
    check_exact(c, prog.pack(), what="join")


def test_join_protects_what_side_records_still_read(sizing):
    """write after read: c must hold the sums of the ORIGINAL b"""
    n, k = sizing["n"], sizing["k"]
    c, t = scene(n, "bc")
    prog = Program()
    axpy(prog, t["b"], t["c"], n, S, times=k)
    prog.add("MEMSET", DST=t["b"], BYTES=4 * n, _flags=J)
    got, ref = run_calls(c, prog.pack())
    assert torch.equal(got, ref), f"write after read: {mismatches(c, got, ref)}"
    assert not c.read(got, "b").any()


def test_fork_is_rearmed_after_later_main_work(sizing):
    """main writes b, side reads b, main writes e, side reads e: the second fork must come after e"""
    n, k = sizing["n"], sizing["k"]
    c, t = scene(n, "abce")
    prog = Program()
    axpy(prog, t["a"], t["b"], n, times=k)
    axpy(prog, t["b"], t["c"], n, S)
    axpy(prog, t["a"], t["e"], n, times=k)
    axpy(prog, t["e"], t["c"], n, S)
    check_exact(c, prog.pack(), what="re-arm")


def test_side_stream_is_serial(sizing):
    n, k = sizing["n"], sizing["k"]
    c, t = scene(n, "abc")
    prog = Program()
    axpy(prog, t["a"], t["b"], n, S, times=k)
    axpy(prog, t["b"], t["c"], n, S)
    check_exact(c, prog.pack(), what="side stream serial")


def test_end_of_call_joins(sizing):
    """a call that ends in a side producer, and a second call on the same stream that consumes it"""
    n, k = sizing["n"], sizing["k"]
    c, t = scene(n, "abc")
    prog = Program()
    axpy(prog, t["a"], t["b"], n, S, times=k)
    axpy(prog, t["b"], t["c"], n)
    check_exact(c, prog.pack(), calls=[(0, k), (k, k + 1)], what="end-of-call join")


@pytest.mark.parametrize("calls", [[(0, 6)], [(0, 2), (2, 5), (5, 6)]], ids=["one-call", "three-calls"])
def test_begin_end_ranges(sizing, calls):
    n = sizing["n"]
    c, t = scene(n, "abce")
    prog = Program()
    axpy(prog, t["a"], t["b"], n, times=2)
    axpy(prog, t["b"], t["c"], n, S)
    axpy(prog, t["a"], t["e"], n)
    axpy(prog, t["e"], t["c"], n, S)
    axpy(prog, t["c"], t["b"], n, J)
    check_exact(c, prog.pack(), calls=calls, what=f"calls {calls}")


def _chain_behind_a_side_producer(sizing, B, C, W, K):
    """a side producer that ends in a small side AXPY into `ps`, which the chain's first record reads; FLAG_JOIN on the chain's third
    record only, FLAG_SIDE on its DWCONV_WGRAD"""
    n, k = sizing["n"], sizing["k"]
    c, chain = _chain(B, C, W, K)
    a, b = c.t("big_a", (n,)), c.t("big_b", (n,))
    ps_add = c.t("ps_add", (4, B, C), scale=3.0)
    pre = Program()
    axpy(pre, a, b, n, S, times=k)
    axpy(pre, ps_add, c.items["ps"][0], 4 * B * C, S)
    packed = np.concatenate([pre.pack(), chain])
    packed["flags"][k + 2] |= S
    packed["flags"][k + 3] |= J
    assert [int(f) & (S | J) for f in packed["flags"][k + 1:]] == [0, S, J, 0] and packed["flags"][k + 1] & D.FLAG_CHAIN
    return c, packed


def test_chain_honours_a_join_asked_for_by_its_third_record(sizing):
    c, packed = _chain_behind_a_side_producer(sizing, 9, 6, 8, 3)
    assert _families(c, packed)[-4:] == FUSED
    got, cpu, wide = c.execute(packed, ref64=True)
    _compare(c, got, cpu, wide, OUTS)
    assert torch.equal(c.read(got, "big_b"), c.read(cpu, "big_b")) and torch.equal(c.read(got, "ps"), c.read(cpu, "ps"))


def test_declined_chain_honours_the_same_flags_record_by_record(sizing):
    c, packed = _chain_behind_a_side_producer(sizing, 3, 5, 32, 3)
    plain_case, plain = _chain(3, 5, 32, 3, flag=False)
    fam = _families(c, packed)[-4:]
    assert 10 not in fam and fam == _families(plain_case, plain), fam
    got, cpu, wide = c.execute(packed, ref64=True)
    _compare(c, got, cpu, wide, OUTS + ["stats2"], sum0=("stats2",))
    assert torch.equal(c.read(got, "big_b"), c.read(cpu, "big_b")) and torch.equal(c.read(got, "ps"), c.read(cpu, "ps"))


def test_side_and_join_flags_are_ordering_only():
    """the b0 2x64x64 backward (weights and inputs of tests/test_unet_gpu.py) as planned, and with FLAG_SIDE / FLAG_JOIN cleared in
    the packed records: both meet that file's gradient bars against the emulator.  Their mutual difference is printed, not asserted:
    the float atomics of WGRAD are not exact from run to run."""
    from s2lc_amd import _lib, engine
    from tests.test_unet_gpu import _model

    version, C, H, W, B, ncls = "b0", 6, 64, 64, 2, 4
    model, net, sd = _model(version, C, ncls, seed=31)
    x = detgen.normal("gpu.x", (B, C, H, W), seed=31)
    y = detgen.labels("gpu.y", (B, H, W), ncls, seed=31)
    noise = detgen.uniform("gpu.dc", (len(net.blocks), B), 0.0, 1.0, seed=31)
    plan = model._make_plan(B, H, W, True)
    bases_cpu = make_bases(plan, model._flat_params, model._flat_bufs, x, noise, B * ncls * H * W)
    emulate(plan.fwd.pack(), bases_cpu)
    dev = torch.device("cuda:0")
    model.to(dev).train()
    eng = engine.UnetEngine(model, B, H, W, True, dev)
    eng.ws.view(torch.float32)[: eng.ws.numel() // 4].fill_(float("nan"))
    out = torch.empty(B, ncls, H, W, device=dev)
    xg, ng = x.to(dev), noise.to(dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.run(eng.fwd, eng.bases(model, xg, out, noise=ng), st)
    torch.cuda.synchronize()
    lg = bases_cpu[D.BASE["OUT"]].view(torch.float32).view(B, ncls, H, W).clone().requires_grad_(True)
    (dlogits,) = torch.autograd.grad(losses_ref.focal(lg, y, torch.ones(ncls), 2.0, 0.0, ignore_index=0), lg)
    bases_cpu[D.BASE["DOUT"]].view(torch.float32).copy_(dlogits.reshape(-1))
    ws0, aux0 = eng.ws.clone(), eng.aux.clone()          # the backward overwrites forward state (SE_FC_BWD: HPRE): restored per run
    bases_cpu[D.BASE["WS"]][: ws0.numel()].copy_(ws0.cpu()[: bases_cpu[D.BASE["WS"]].numel()])
    bases_cpu[D.BASE["AUX"]][: aux0.numel()].copy_(aux0.cpu()[: bases_cpu[D.BASE["AUX"]].numel()])
    emulate(plan.bwd.pack(), bases_cpu)
    gref = bases_cpu[D.BASE["GRADS"]].view(torch.float32)
    scale = gref.abs().max().item()

    cleared = eng.bwd.copy()
    cleared["flags"] &= ~(S | J)
    assert int((eng.bwd["flags"] & S != 0).sum()) > 50 and not (cleared["flags"] & (S | J)).any()
    assert (cleared["flags"] == eng.bwd["flags"] & ~(S | J)).all()
    runs = {}
    for label, packed in (("as planned", eng.bwd), ("flags cleared", cleared)):
        eng.ws.copy_(ws0)
        eng.aux.copy_(aux0)
        grads = torch.zeros_like(model._flat_params)
        _lib.run(packed, eng.bases(model, xg, None, dout=dlogits.to(dev), noise=ng, grads=grads), st)
        torch.cuda.synchronize()
        runs[label] = grads.cpu()
        worst = []
        for name, (off, shape) in plan.layout.params.items():
            cnt = int(np.prod(shape))
            a, b = runs[label][off:off + cnt].double(), gref[off:off + cnt].double()
            if b.abs().max().item() < 1e-7 * scale:
                assert a.abs().max().item() < 1e-5 * scale, (label, name)
                continue
            e = (a - b).abs().max().item() / b.abs().max().item()
            if e > 2e-3:
                worst.append((name, e))
        assert not worst, (label, worst[:8])
    d = (runs["as planned"] - runs["flags cleared"]).abs().max().item()
    print(f"largest difference between the two runs: {d:.3e} ({d / scale:.3e} of the largest gradient)")
