"""CPU: the order `s2k_program_run` leaves between the records of a program, and the byte-level hazards of every plan.

tests/stream_order.py restates the executor's fork / join rules and the bytes every record reads and writes.  Here
  * the rules are held to hand-made programs (the exact set of unordered record pairs of each);
  * the footprints are held to the emulator, one record of every signature (kind, flags, tensor slots present) of four plans: every
    byte a record changes lies in its write footprint, and with every byte outside read + write poisoned (0xFF: a NaN in every float
    format) it writes the same bytes;
  * no unordered pair of any plan the project can build conflicts - a byte one record writes and the other reads or writes -, with
    every depthwise chain accepted and with every chain declined;
  * no record at or behind the end of a backward segment touches that segment's gradient bucket (ddp.FlatGradReducer all-reduces it
    while the later records run);
  * the checker reports each of five planted hazards with the pair of records it was planted on."""
import copy
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import ops_ref
from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, unet_spec
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan import vit_plan as V
from s2lc_amd.plan.program import Program, TRef
from s2lc_amd.plan.unet_plan import plan_unet
from tests import stream_order as SO
from tests.helpers import PRITHVI_FULL, PRITHVI_SEG_SMALL, PRITHVI_SMALL
from tests.plan_harness import NARROW, make_bases, make_bases_vit

S, J, C = D.FLAG_SIDE, D.FLAG_JOIN, D.FLAG_CHAIN


# ---- the model on hand-made programs -------------------------------------------------------------------------------------------------
def _prog(*recs):
    """records as "KIND" or ("KIND", flags)"""
    return [(r, {"_flags": 0}) if isinstance(r, str) else (r[0], {"_flags": r[1]}) for r in recs]


def _chain(f1=0, f2=0, f3=0, f4=0):
    return [("BN_BWD_APPLY", C | f1), ("DWCONV_WGRAD", f2), ("DWCONV_DGRAD", f3), ("BN_BWD_APPLY", f4)]


def test_side_then_main_is_unordered():
    p = _prog(("AXPY", S), "AXPY")
    assert SO.unordered_pairs(p, True) == {(0, 1)}
    o = SO.execute_order(p, True)
    assert o.forks == [0] and o.stream == ["S", "M"] and o.end_join


def test_join_orders_the_main_record():
    p = _prog(("AXPY", S), ("AXPY", J), "AXPY")
    assert SO.unordered_pairs(p, True) == set()
    o = SO.execute_order(p, True)
    assert o.join_before == [False, True, False] and not o.end_join
    # a join with nothing pending does nothing, and the flag on a side record is never looked at
    assert SO.execute_order(_prog(("AXPY", J), ("AXPY", S | J), "AXPY"), True).join_before == [False, False, False]
    assert SO.unordered_pairs(_prog(("AXPY", J), ("AXPY", S | J), "AXPY"), True) == {(1, 2)}


def test_fork_is_rearmed_after_main_work_only():
    p = _prog(("AXPY", S), "AXPY", ("AXPY", S), "AXPY")
    assert SO.unordered_pairs(p, True) == {(0, 1), (0, 3), (2, 3)}
    assert SO.execute_order(p, True).forks == [0, 2]


def test_two_side_records_in_a_row_share_one_fork_and_are_serial():
    p = _prog("AXPY", ("AXPY", S), ("AXPY", S), "AXPY")
    assert SO.unordered_pairs(p, True) == {(1, 3), (2, 3)}
    assert SO.execute_order(p, True).forks == [1]
    assert SO.execute_order(_prog(("AXPY", S), ("AXPY", S)), True).forks == [0]      # the dirty bit starts set


def test_a_side_record_at_the_end_is_joined_by_the_end_of_the_call():
    p = _prog("AXPY", ("AXPY", S))
    assert SO.unordered_pairs(p, True) == set()
    assert SO.execute_order(p, True).end_join
    # call boundaries are joins: the same records as two calls
    q = _prog(("AXPY", S), "AXPY", "AXPY")
    assert SO.unordered_pairs(q, True) == {(0, 1), (0, 2)}
    assert SO.unordered_pairs(q, True, 0, 2) | SO.unordered_pairs(q, True, 2, 3) == {(0, 1)}


@pytest.mark.parametrize("where", [1, 2, 3])
def test_chain_honours_a_join_of_any_record_in_front_of_its_first(where):
    """[side, head, wgrad | SIDE, dgrad, apply, main] with FLAG_JOIN on the chain's 2nd, 3rd or 4th record"""
    fl = [0, S, 0, 0]
    fl[where] |= J
    p = _prog(("WGRAD", S), *_chain(*fl), "AXPY")
    acc = SO.execute_order(p, True)
    assert acc.join_before[1] and acc.chains == [1] and acc.stream == ["S", "M", "M", "M", "M", "M"] and acc.forks == [0]
    assert SO.unordered_pairs(p, True) == set()
    dec = SO.execute_order(p, False)
    assert dec.join_before[1] and dec.chains == [] and dec.stream == ["S", "M", "S", "M", "M", "M"] and dec.forks == [0, 2]
    # declined: the depthwise weight gradient goes to the side stream; its own JOIN bit is not looked at there (where == 1), a JOIN
    # on the 3rd record waits for it at once, one on the 4th leaves the data gradient unordered with it
    want = {1: {(2, 3), (2, 4), (2, 5)}, 2: set(), 3: {(2, 3)}}[where]
    assert SO.unordered_pairs(p, False) == want
    assert dec.join_before[2:] == [False, where == 2, where == 3, False]


def test_chain_consumes_a_side_flagged_wgrad_onto_the_main_stream():
    p = _prog(("WGRAD", S), *_chain(0, S, 0, 0))
    assert SO.unordered_pairs(p, True) == {(0, 1), (0, 2), (0, 3), (0, 4)}
    assert SO.unordered_pairs(p, False) == {(0, 1), (0, 3), (0, 4), (2, 3), (2, 4)}
    # fewer than three records behind the head inside the call: the flag is not looked at
    q = _prog(*_chain(0, S, 0, 0)[:3])
    assert SO.unordered_pairs(q, True) == {(1, 2)} and SO.execute_order(q, True).chains == []
    full = _prog(*_chain(0, S, 0, 0))
    assert SO.unordered_pairs(full, True, 0, 3) == {(1, 2)} and SO.unordered_pairs(full, True) == set()
    # bf16 / split records are never fused
    r = _prog(*_chain(0, S | D.FLAG_BF16, 0, 0))
    assert SO.execute_order(r, True).chains == []


def test_strided_intervals_and_merging():
    lo, hi = SO.strided(100, [(3, 1), (4, 3), (2, 12)])                 # contiguous: one run of 24 floats
    assert lo.tolist() == [100] and hi.tolist() == [196]
    lo, hi = SO.strided(0, [(3, 1), (2, 5), (2, 20)])                   # rows of 3 floats at 0, 5, 20, 25
    assert sorted(zip(lo.tolist(), hi.tolist())) == [(0, 12), (20, 32), (80, 92), (100, 112)]
    m = SO._merge([(np.array([0, 8, 40]), np.array([8, 16, 44])), (30, 41)])
    assert m.tolist() == [[0, 16], [30, 44]]
    assert SO._hit(np.array([[0, 4], [10, 14]]), np.array([[4, 10], [14, 20]])) is None
    assert SO._hit(np.array([[0, 4], [10, 14]]), np.array([[4, 11]])) == (10, 11)


# ---- the plans -----------------------------------------------------------------------------------------------------------------------
def _bench_defaults():
    """the benchmark's own U-Net workload, from its argument defaults"""
    text = (Path(__file__).resolve().parents[1] / "bench.py").read_text()
    get = lambda name: re.search(r'add_argument\("--%s",[^)]*default=("?)([\w.]+)\1' % name, text).group(2)  # noqa: E731
    return get("version"), int(get("bands")), int(get("size")), int(get("batch"))


def _unet_spec(version, bands=4):
    return unet_spec(EfficientNetConfig(version, bands, 4, class_distribution=[0.25] * 4))


def _mae_spec(a, decoder=True):
    return V.MaeSpec(a["img_size"], a["patch_size"], a["num_frames"], a["tubelet_size"], a["in_chans"], a["embed_dim"], a["depth"],
                     a["num_heads"], a["decoder_embed_dim"], a["decoder_depth"], a["decoder_num_heads"], 4.0, False, decoder)


PRECISIONS = {"f32": {}, "bf16": {"bf16": True}, "split": {"split": True}}


def check_plan(name, plan):
    """both programs of a plan: no conflicting unordered pair with every chain accepted and with every chain declined, the segments
    tile, no late touch of a bucket.  Prints one line per program."""
    blob = plan.const_table
    for which, prog in (("fwd", plan.fwd), ("bwd", plan.bwd)):
        if prog is None:
            continue
        fps = SO.footprints(prog.ops, blob)
        hulls = SO.Hulls(fps)
        for accept in (True, False):
            bad, o, pairs = SO.find_conflicts(prog.ops, blob, accept, fps, hulls)
            line = (f"{name} {which} chains {'accepted' if accept else 'declined'}: {len(prog.ops)} records, {o.stream.count('S')} side, "
                    f"{sum(o.join_before)} joins, {len(o.chains)} chains, {pairs} unordered pairs examined, {len(bad)} conflicts")
            print(line)
            assert not bad, (name, which, accept, [(i, prog.ops[i][0], j, prog.ops[j][0], w, b, lo, hi) for i, j, w, b, lo, hi in bad[:4]])
            if not o.chains and accept:
                break               # no chain to decline: the other outcome is the same call
        if which == "bwd":
            segs, n = plan.bwd_param_marks, plan.layout.n_params
            assert SO.segments_tile(segs, len(prog.ops), n), (name, segs[:3], segs[-3:])
            for tlo in {0, getattr(plan, "trainable_lo", 0)}:
                late = SO.bucket_touches(fps, segs, n, tlo)
                assert not late, (name, tlo, [(segs[k], i, prog.ops[i][0], lo, hi) for k, i, lo, hi in late[:4]])


def _unet_sizes():
    _, bands, size, batch = _bench_defaults()
    return [(4, 2, 64), (4, 5, 96), (bands, batch, size)]


@pytest.mark.parametrize("version", ["b0", "b3", "b5"])
def test_no_unordered_pair_of_a_unet_plan_conflicts(version):
    n = 0
    for bands, B, H in _unet_sizes():
        spec = _unet_spec(version, bands)
        for pname, pkw in PRECISIONS.items():
            for defer in (None, False):
                for bucket in (4096, 1 << 16, None):
                    kw = dict(pkw, defer_wgrads=defer, **({} if bucket is None else {"bucket_floats": bucket}))
                    check_plan(f"unet {version} {B}x{bands}x{H}x{H} {pname} defer={defer} bucket={bucket}", plan_unet(spec, B, H, H, True, **kw))
                    n += 1
            for want_dx in (False, True):
                check_plan(f"unet {version} {B}x{bands}x{H}x{H} {pname} eval want_bwd want_dx={want_dx}",
                           plan_unet(spec, B, H, H, False, want_bwd=True, want_dx=want_dx, **pkw))
                n += 1
    assert n == 3 * 3 * (2 * 3 + 2)
    assert _bench_defaults()[0] in ("b0", "b3", "b5")       # the benchmark's own plan is one of those above


# (name, MAE arguments, segmentation arguments, MAE batch, segmentation batch, fcn_out): the fixtures' small models, and Prithvi-100M
# as bench.py's prithvi_workload runs it (6 x 1 x 224 x 224; MAE bs 64 mask 0.75; segmentation bs 16, 4 classes, 256 FCN channels)
VIT = [("small", PRITHVI_SMALL, PRITHVI_SEG_SMALL, 2, 2, 8), ("full", PRITHVI_FULL, PRITHVI_FULL, 64, 16, 256)]


@pytest.mark.parametrize("name,a,sa,B,Bs,fcn", VIT, ids=[v[0] for v in VIT])
def test_no_unordered_pair_of_a_vit_plan_conflicts(name, a, sa, B, Bs, fcn):
    for pname, pkw in PRECISIONS.items():
        for want_dx in (False, True):
            check_plan(f"mae {name} bs{B} {pname} want_dx={want_dx}", V.plan_mae(_mae_spec(a), B, 0.75, True, want_dx=want_dx, **pkw))
        for frozen in (True, False):
            spec = V.SegSpec(_mae_spec(sa, False), 4, fcn, 1, 0.1, frozen)
            check_plan(f"seg {name} bs{Bs} {pname} frozen={frozen}", V.plan_seg(spec, Bs, True, **pkw))
            check_plan(f"seg {name} bs{Bs} {pname} frozen={frozen} eval want_bwd want_dx", V.plan_seg(spec, Bs, False, want_bwd=True, want_dx=True, **pkw))
    s = _mae_spec(a)
    L = V.mae_layout(s)
    keep = int(s.num_patches * 0.25)
    for mname, plan in (("forward_encoder", V.plan_mae_encoder(s, B, 0.75, True, L)),
                        ("forward_encoder want_dx", V.plan_mae_encoder(s, B, 0.75, True, L, want_dx=True)),
                        ("forward_decoder", V.plan_mae_decoder(s, B, 1 + keep, True, L)),
                        ("forward_loss", V.plan_mae_loss(s, B, True, L)),
                        ("random_masking", V.plan_random_masking(s, B, s.num_patches, 12, 0.5, True, L))):
        check_plan(f"method {name} {mname}", plan)


def test_leading_segments_without_stages_stay_empty_behind_a_weight_pack():
    """found by the sweep above: forward_encoder's backward gives the decoder's parameters - the top of the flat buffer - no gradient,
    so its first segments hold no stage; with the WEIGHT_PACK put in front of the program each of them became [0, 1) and a
    segment-by-segment run would have packed the weights once per bucket.  They stay [0, 0); the pack belongs to the first segment
    that runs anything."""
    s = _mae_spec(PRITHVI_FULL)
    plan = V.plan_mae_encoder(s, 64, 0.75, True, V.mae_layout(s))
    segs = plan.bwd_param_marks
    assert plan.bwd.ops[0][0] == "WEIGHT_PACK" and segs[0][:2] == (0, 0) and SO.segments_tile(segs, len(plan.bwd.ops), plan.layout.n_params)
    first = next(k for k, (a, b, _, _) in enumerate(segs) if b > a)
    assert first >= 1 and segs[first][0] == 0 and all(b == 0 for _, b, _, _ in segs[:first])
    covered = [i for a, b, _, _ in segs for i in range(a, b)]
    assert covered == list(range(len(plan.bwd.ops)))            # every record in exactly one segment


# ---- the footprints against the emulator ---------------------------------------------------------------------------------------------
def _signature(kind, f):
    return kind, int(f.get("_flags", 0)), tuple(isinstance(f.get(s), TRef) for s in D.OPS[kind][0])


def _validate_program(name, prog, blob, bases, seen):
    """run `prog` record by record through the emulator; at the first record of every new signature check the footprint.  A shadow
    copy of the bases follows the run through the WRITE footprints alone, so a byte changed outside one shows as a difference."""
    packed = prog.pack()
    run = lambda i, b: ops_ref.run_program(packed[i:i + 1], b, D, narrow_bases=NARROW)  # noqa: E731
    shadow = {b: t.clone() for b, t in bases.items()}
    checked = 0

    def same(what, i, kind):
        for b, t in bases.items():
            if not torch.equal(shadow[b], t):
                at = int(torch.nonzero(shadow[b] != t).reshape(-1)[0])
                raise AssertionError(f"{name} record {i} ({kind}): {what}: bytes of {D.BASES[b]} changed outside the write footprints, first {at}")

    for i, (kind, f) in enumerate(prog.ops):
        fp = SO.footprint(kind, f, blob)
        sig = _signature(kind, f)
        poisoned = None
        if sig not in seen:
            seen.add(sig)
            checked += 1
            poisoned = {b: torch.full_like(t, 0xFF) for b, t in shadow.items()}        # NaN in every float format
            for b, p in poisoned.items():
                for lo, hi in fp.touched(b).tolist():
                    p[lo:hi] = shadow[b][lo:hi]
        run(i, bases)
        for b, iv in fp.writes.items():
            for lo, hi in iv.tolist():
                shadow[b][lo:hi] = bases[b][lo:hi]
        if poisoned is None:
            continue
        same("(a)", i, kind)
        run(i, poisoned)
        for b, iv in fp.writes.items():
            for lo, hi in iv.tolist():
                assert torch.equal(poisoned[b][lo:hi], bases[b][lo:hi]), \
                    f"{name} record {i} ({kind}): written bytes [{lo}, {hi}) of {D.BASES[b]} depend on bytes outside the read footprint"
    same("at the end of the program", len(prog.ops), "-")
    return checked


def _fill(bases, seed):
    """finite random values in every float base (the emulator's own poison of WS stays: a read of never-written memory must not happen)"""
    g = torch.Generator().manual_seed(seed)
    for name, scale in (("PARAMS", 0.2), ("X", 1.0), ("DOUT", 1e-3), ("BUFS", None)):
        v = bases[D.BASE[name]].view(torch.float32)
        v.copy_(torch.rand(v.shape, generator=g) + 0.5 if scale is None else torch.randn(v.shape, generator=g) * scale)


def test_footprints_hold_against_the_emulator_for_every_record_signature():
    seen: set = set()
    total = 0
    spec = _unet_spec("b0")
    g = torch.Generator().manual_seed(5)
    for pname, pkw in PRECISIONS.items():
        plan = plan_unet(spec, 2, 64, 64, True, **pkw)
        x = torch.randn(2, 4, 64, 64, generator=g)
        noise = torch.rand(plan.n_noise_rows, 2, generator=g)
        bases = make_bases(plan, torch.zeros(plan.layout.n_params), torch.zeros(max(plan.layout.n_bufs, 1)), x, noise, 2 * 4 * 64 * 64)
        _fill(bases, 6)
        for which, prog in (("fwd", plan.fwd), ("bwd", plan.bwd)):
            n = _validate_program(f"unet b0 {pname} {which}", prog, plan.const_table, bases, seen)
            print(f"unet b0 2x4x64x64 {pname} {which}: {n} new record signatures checked")
            total += n
    s = _mae_spec(PRITHVI_SMALL)
    plan = V.plan_mae(s, 2, 0.75, True, want_dx=True)
    x = torch.randn(2, s.in_chans, s.num_frames, s.img_size, s.img_size, generator=g)
    bases = make_bases_vit(plan, torch.zeros(plan.layout.n_params), torch.zeros(1), x, torch.rand(2, s.num_patches, generator=g))
    _fill(bases, 7)
    for which, prog in (("fwd", plan.fwd), ("bwd", plan.bwd)):
        n = _validate_program(f"mae small {which}", prog, plan.const_table, bases, seen)
        print(f"mae small bs2 {which}: {n} new record signatures checked")
        total += n
    kinds = {k for k, _, _ in seen}
    assert {"WEIGHT_PACK", "WGRAD_FINALIZE", "WGRAD", "CONV", "MEMSET", "BN_BWD_APPLY", "CHAN_LN_BWD", "PATCHIFY", "ATTN_BWD"} <= kinds
    assert any(k == "CONV" and fl & D.FLAG_SPLIT for k, fl, _ in seen) and any(k == "CONV" and fl & D.FLAG_BF16 for k, fl, _ in seen)
    print(f"{total} signatures of {len(kinds)} kinds")


def test_exact_rows_of_a_concat_wgrad_and_a_strided_conv_output():
    """WGRAD with CTOT > C owns C floats of every [tap][m] row; CONV with YC > M owns M channels of every image"""
    wgs = TRef(D.BASE["WGS"], 4 * 1000, (4, 10, 3, 3))
    f = dict(P=None, Q=None, WGS=wgs.at(4), B=1, M=4, C=6, CTOT=10, KH=3, KW=3, H=4, W=4, HO=4, WO=4)
    w = SO.footprint("WGRAD", f, []).writes[D.BASE["WGS"]]
    assert len(w) == 36 and w[0].tolist() == [4016, 4040] and w[1].tolist() == [4056, 4080] and w[-1, 1] == 4000 + 4 * (35 * 10 + 10)
    y = TRef(D.BASE["WS"], 256, (2, 8, 4, 4))
    f = dict(Y=y.at(3 * 16), B=2, M=5, YC=8, HO=4, WO=4, MODE=D.MODE_CONV, BETA=0)
    fp = SO.footprint("CONV", f, [])
    assert fp.writes[D.BASE["WS"]].tolist() == [[256 + 192, 256 + 192 + 320], [256 + 192 + 512, 256 + 192 + 832]] and not fp.reads
    f["BETA"] = 1
    assert SO.footprint("CONV", f, []).reads[D.BASE["WS"]].tolist() == fp.writes[D.BASE["WS"]].tolist()


# ---- the checker must be able to fail ------------------------------------------------------------------------------------------------
def _b0(**kw):
    return plan_unet(_unet_spec("b0"), 2, 64, 64, True, **kw)


def _conflict_pairs(ops, blob, accept=False):
    bad, _, _ = SO.find_conflicts(ops, blob, accept, limit=10 ** 6)
    return {(i, j) for i, j, *_ in bad}


def test_mutation_side_flag_on_a_producer_is_reported():
    """a BatchNorm backward whose dY the following records read, moved to the side stream: the weight gradient behind it is on the side
    stream too and stays ordered (the side stream is serial); the first main-stream reader - the data-gradient CONV - is not"""
    plan = _b0()
    ops = copy.deepcopy(plan.bwd.ops)

    def reads(j, ref):
        k, f = ops[j]
        return any(isinstance(v, TRef) and v.ref == ref for s, v in f.items() if s not in D.WRITES[k])

    i = next(i for i, (k, f) in enumerate(ops[:-2]) if k == "BN_BWD_APPLY" and not f.get("_flags", 0) and reads(i + 1, f["DY"].ref))
    j = next(j for j in range(i + 1, len(ops)) if not ops[j][1].get("_flags", 0) & S and reads(j, ops[i][1]["DY"].ref))
    assert ops[i + 1][0] == "WGRAD" and ops[j][0] == "CONV" and j <= i + 3
    assert not _conflict_pairs(ops, plan.const_table)
    ops[i][1]["_flags"] = S
    got = _conflict_pairs(ops, plan.const_table)
    assert (i, j) in got and (i, i + 1) not in got


def test_mutation_cleared_join_is_reported():
    """the in-place residual-stream accumulation the docstring of unet_plan.side_stream_hazards describes: a weight gradient on the
    side stream reads g, the LayerNorm backward then adds into g.  The planner's pass adds the join; without it the pair is reported."""
    from s2lc_amd.plan.unet_plan import side_stream_hazards

    ws = D.BASE["WS"]
    t = lambda off, shape: TRef(ws, off, shape)  # noqa: E731
    g, a1, dy, x, mr, gam = t(0, (2, 8, 16)), t(4096, (2, 32, 16)), t(8192, (2, 8, 16)), t(12288, (2, 8, 16)), t(16384, (2, 16, 2)), t(20480, (8,))
    prog = Program()
    prog.add("WGRAD", P=g, BNVP=None, GATEP=None, Q=a1, BNVQ=None, GATEQ=None, WGS=TRef(D.BASE["GRADS"], 0, (8, 32)), B=2, M=8, C=32, CTOT=32,
             H=1, W=16, KH=1, KW=1, STRIDE=1, PAD_T=0, PAD_L=0, HO=1, WO=16, PROP=0, PROQ=0, MODE=D.MODE_CONV, _flags=S)
    prog.add("CHAN_LN_BWD", DY=dy, X=x, MR=mr, GAMMA=gam, DX=g, DGAMMA=None, DBETA=None, DXIN=None, DSUM=None, B=2, C=8, HW=16, ACCUM=1)
    assert side_stream_hazards(prog) == 1 and prog.ops[1][1]["_flags"] & J
    assert not _conflict_pairs(prog.ops, [])
    prog.ops[1][1]["_flags"] &= ~J
    assert _conflict_pairs(prog.ops, []) == {(0, 1)}
    # the out-of-place form the planner emits today (DXIN) needs no join
    prog.ops[1][1].update(DXIN=g, DX=t(24576, (2, 8, 16)))
    assert not _conflict_pairs(prog.ops, [])


def test_mutation_finalize_row_on_a_batchnorm_gamma_is_reported():
    plan = _b0(bucket_floats=4096, defer_wgrads=False)
    ops, blob = plan.bwd.ops, list(plan.const_table)
    fin = next(i for i, (k, f) in enumerate(ops) if k == "WGRAD_FINALIZE" and f["_flags"] & S)
    ap = next(i for i, (k, f) in enumerate(ops) if i > fin and k == "BN_BWD_APPLY" and not f.get("_flags", 0) & (S | C))
    assert not _conflict_pairs(ops, blob)
    row = ops[fin][1]["TABLE"].off // 4
    off, M, Cc, T = blob[row:row + 4]
    gamma = ops[ap][1]["DGAMMA"].off // 4
    blob[row] = gamma
    assert (fin, ap) in _conflict_pairs(ops, blob)


def test_mutation_side_pack_row_on_a_forward_pack_is_reported():
    plan = _b0()
    ops, blob = plan.fwd.ops, list(plan.const_table)
    assert ops[0][0] == "WEIGHT_PACK" and ops[0][1]["_flags"] & S and ops[1][0] == "WEIGHT_PACK"
    conv = next(i for i, (k, f) in enumerate(ops) if k == "CONV")
    assert not _conflict_pairs(ops, blob)
    row = ops[0][1]["TABLE"].off // 4
    blob[row + 1] = ops[conv][1]["WT"].off // 4             # dst_off of the backward's first row := the pack that CONV reads
    got = _conflict_pairs(ops, blob)
    assert (0, conv) in got and (0, 1) in got               # the reader, and the forward's own WEIGHT_PACK that writes the same bytes


def test_mutation_segment_end_in_front_of_its_finalize_is_reported():
    plan = _b0(bucket_floats=4096, defer_wgrads=False)
    ops = plan.bwd.ops
    fps = SO.footprints(ops, plan.const_table)
    segs = list(plan.bwd_param_marks)
    assert not SO.bucket_touches(fps, segs, plan.layout.n_params)
    k = next(k for k, (a, b, lo, hi) in enumerate(segs) if b > a and ops[b - 1][0] == "WGRAD_FINALIZE")
    a, b, lo, hi = segs[k]
    segs[k] = (a, b - 1, lo, hi)
    late = SO.bucket_touches(fps, segs, plan.layout.n_params)
    assert late and all((kk, i) == (k, b - 1) for kk, i, _, _ in late)
