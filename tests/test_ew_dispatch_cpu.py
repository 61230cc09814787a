"""Coverage of the element-wise GPU tables (tests/test_ew_kernels_gpu.py), checked without a GPU.  tests/ew_dispatch.py restates
which kernel each launcher of csrc/ew.hip takes and which loop facts a shape exercises; this file parses csrc/ew.hip (and the
replica paths of csrc/common.h) for every constant and threshold that restatement uses and fails when one drifts, checks that each
`g_s2k_variant = N;` follows the launch it belongs to, that the family column of every table row agrees with the restatement, that
the tables reach every kernel instantiation ew.hip launches for these stages, every required edge, and every (stage, family, form)
of the production plans at the plan's own plane size - and that on every row's data the f32 oracle alone stays within a quarter of
the row's bar of the float64 oracle, under the norms the GPU rows are held to, so that the bar is spent on the kernel."""
import dataclasses
import re
from pathlib import Path

import pytest

from tests import ew_dispatch as E
from tests import test_ew_kernels_gpu as T

CSRC = Path(__file__).resolve().parents[1] / "sentinel2-landcover-classification_amd" / "csrc"
# kernels of csrc/ew.hip that belong to other stage families (AXPY, WGRAD_FINALIZE, WEIGHT_PACK, SPACE_TO_DEPTH, IM2COL, Adam)
OTHER = {"axpy_kernel", "wgrad_finalize_kernel", "weight_pack_kernel", "weight_pack_bf16_kernel", "weight_pack_q4_kernel", "weight_pack_split_kernel",
         "space_to_depth_kernel", "space_to_depth_scalar_kernel", "im2col_kernel", "adam_kernel", "adam_scalar_kernel"}


def _src():
    return (CSRC / "ew.hip").read_text()


def _ints(pattern, src, count=None):
    found = re.findall(pattern, src)
    assert found, f"not in its known form: {pattern}"
    if count is not None:
        assert len(found) == count, f"{pattern}: {len(found)} matches, expected {count}"
    return [tuple(int(v) for v in (m if isinstance(m, tuple) else (m,))) for m in found]


def test_constants_and_thresholds_match_the_source():
    src, common = _src(), (CSRC / "common.h").read_text()
    assert _ints(r"constexpr int NTHREADS = (\d+);", common, 1) == [(E.NTHREADS,)]
    assert _ints(r"constexpr int CHUNK = (\d+);", src, 1) == [(E.CHUNK,)]
    assert _ints(r"constexpr int SEW_CT = (\d+), SEW_BT = (\d+), SEW_QMAX = (\d+),", src, 1) == [(E.SEW_CT, E.SEW_BT, E.SEW_QMAX)]
    # workgroup-per-plane kernels: SE_POOL, SE_BN_SUMS
    assert _ints(r"if \(HW >= (\d+) && \(HW & 3\) == 0 && (?:\(int64_t\)B \* C|nplanes) <= (\d+)\) \{", src, 2) == [(E.BIG_HW, E.BIG_PLANES)] * 2
    assert len(re.findall(r"for \(; i \+ NTHREADS < n4; i \+= 2 \* NTHREADS\)", src)) == 2 and len(re.findall(r"for \(; i < n4; i \+= NTHREADS\)", src)) == 2
    # wave-per-channel kernels: SE_POOL and BN_RESIDUAL at HW <= 256, SE_BN_SUMS and BN_BWD_APPLY at HW <= 64, all with B > 1
    small = _ints(r"if \(HW <= (\d+) && \(HW & 3\) == 0 && B > 1\) \{", src, 3)
    assert sorted(small) == sorted([(E.SMALL_HW["SE_POOL"],), (E.SMALL_HW["SE_BN_SUMS"],), (E.SMALL_HW["BN_RESIDUAL"],)])
    order = [m.start() for m in re.finditer(r"if \(HW <= \d+ && \(HW & 3\) == 0 && B > 1\) \{", src)]
    owners = [src.rfind("int launch_", 0, at) for at in order]
    assert [re.match(r"int (launch_\w+)", src[o:]).group(1) for o in owners] == ["launch_se_pool", "launch_se_bn_sums", "launch_bn_residual"]
    assert [v for (v,) in small] == [E.SMALL_HW["SE_POOL"], E.SMALL_HW["SE_BN_SUMS"], E.SMALL_HW["BN_RESIDUAL"]]
    assert _ints(r"if \(HW > (\d+) \|\| \(HW & 3\) \|\| B < 2\) return false;", src, 1) == [(E.SMALL_HW["BN_BWD_APPLY"],)]
    assert _ints(r"const int bsplit = std::max\(1, std::min\(cdiv\(B, 64 / lpp\), cdiv\((\d+), C\)\)\);", src, 4) == [(E.SMALL_WAVES,)] * 4
    assert len(re.findall(r"int lpp = 1;\s*while \(4 \* lpp < HW\) lpp <<= 1;", src)) == 4
    assert _ints(r"constexpr int U = (\d+);", src, 2) == [(E.SMALL_UNROLL,)] * 2
    # CHANNEL_SUM
    assert _ints(r"if \(B > 0 && C >= (\d+) && HW > 0 && HW <= (\d+)\) \{", src, 1) == [(E.ROWS_C, E.ROWS_HW)]
    assert _ints(r"for \(; b \+ (\d+) < B; b \+= (\d+)\) \{", src, 1) == [(4 * (E.ROWS_UNROLL - 1), 4 * E.ROWS_UNROLL)]
    assert re.search(r"float acc\[%d\];" % E.ROWS_UNROLL, src) and re.search(r"for \(; b < B; b \+= 4\) \{", src)
    # SE backward routes
    assert _ints(r"const bool small = Q <= (\d+);", src, 1) == [(E.FC_SMALL_Q,)]
    assert re.search(r"if \(Q <= SEW_QMAX\) \{", src)
    # replica paths (common.h): bn_fold_wave and bn_fuse_sums
    assert _ints(r"if \(f\.nrep <= (\d+)\) \{", common, 1) == [(E.REP_SCALAR,)]
    assert _ints(r"\} else if \(fz\.nrep <= (\d+)\) \{", common, 1) == [(E.REP_SCALAR,)]
    # the chunked kernels take tasks of CHUNK elements; float4 bodies for HW % 4 == 0
    assert re.search(r"const int chunks = \(HW \+ CHUNK - 1\) / CHUNK;", src)
    assert len(re.findall(r"if \(\(HW & 3\) == 0\)", src)) == 4          # plane_reduce, se_bn_sums, bn_bwd_reduce, plane_map
    # UPSAMPLE_ZERO's grid cap
    assert re.search(r"hipLaunchKernelGGL\(upsample_zero_kernel, dim3\(\(unsigned\)std::min<int64_t>\(cdiv64\(total, 256\), 65536\)\), dim3\(256\)", src)


def test_each_variant_report_follows_its_launch():
    src = _src()
    want = [("se_pool_big_kernel", 12), ("se_pool_small_kernel", 11), ("se_bn_sums_big_kernel", 12), ("se_bn_sums_small_kernel", 11),
            ("channel_sum_rows_kernel", 13), ("se_fc_wgrad_tile_kernel", 15), ("se_fc_bwd_small_kernel", 14),
            (r"\(bn_bwd_apply_small_kernel<MODE, OUT16>\)", 11), ("bn_residual_small_kernel", 11)]
    for kernel, code in want:
        assert re.search(r"hipLaunchKernelGGL\(" + kernel + r",[^;]*;\s*g_s2k_variant = %d;" % code, src), f"{kernel}: no `g_s2k_variant = {code};` behind its launch"
    # SE_FC_BWD ends on its data-gradient route, whatever the parameter gradients took
    assert re.search(r"launch_se_fc_param_grads\(dgate, hs, hpre, pool, dw1, db1, dw2, db2, B, C, Q, c\.stream\);\s*g_s2k_variant = small \? 14 : 0;", src)
    assert len(re.findall(r"g_s2k_variant = ", src)) == len(want) + 1
    api = (CSRC / "s2k_api.hip").read_text()
    # reset before every stage (run and profile): the shared issue step resets first, and both loops issue through it and nothing else
    step = re.search(r"static int issue_step\([^)]*\) \{\n(.*?)\n\}\n", api, re.S).group(1)
    assert step.lstrip().startswith("g_s2k_variant = 0;") and "try_dw_chain(" in step and "check_launch(dispatch(" in step
    run = api[api.index("int s2k_program_run("):api.index("int s2k_op_launch(")]
    prof = api[api.rindex("static int profile_impl("):]
    assert len(re.findall(r"issue_step\(", run)) == 2 and len(re.findall(r"issue_step\(", prof)) == 1          # side / main stream; profile
    for loop in (run, prof):
        assert "dispatch(" not in loop and "try_dw_chain(" not in loop


def launched():
    """every kernel instantiation csrc/ew.hip launches for the stages of this family, template parameters expanded from the callers"""
    src = _src()
    out = set()
    modes = {"plane_reduce_kernel": re.findall(r"launch_plane_reduce<(\d)>\(", src), "plane_map_kernel": re.findall(r"launch_plane_map<(\d)>\(", src)}
    assert sorted(set(modes["plane_reduce_kernel"])) == ["0", "1", "2"] and sorted(set(modes["plane_map_kernel"])) == ["0", "1", "2", "3"]
    small = [re.sub(r"\s+", " ", a) for a in re.findall(r"launch_bn_bwd_apply_small<([^>]*)>\(gp", src)]
    for m in re.finditer(r"hipLaunchKernelGGL\(\(?(\w+)(?:<([^>]*)>)?\)?,", src):
        name, args = m.group(1), m.group(2)
        if name in OTHER:
            continue
        if args is None:
            out.add(name)
        elif "MODE" in args and name == "bn_bwd_apply_small_kernel":
            out.update(f"{name}<{a}>" for a in small)
        elif "MODE" in args:
            out.update(f"{name}<{args.replace('MODE', md)}>" for md in modes[name])
        else:
            out.add(f"{name}<{args}>")
    return out


def _rows():
    for kind, kw, fam in T.all_rows():
        yield kind, kw, fam, E.dispatch(kind, **T.record_fields(kind, kw))


def test_every_row_is_pinned_to_the_family_the_launcher_takes():
    for kind, kw, fam, d in _rows():
        assert d.family == fam, f"{T.row_id(kind, kw)}: family column {fam}, the launcher takes {d.kernels} (family {d.family})"


def test_tables_reach_every_launched_instantiation():
    want = launched()
    assert len(want) == 39, sorted(want)
    got = set()
    for _, _, _, d in _rows():
        got.update(d.kernels)
    assert got == want, f"not reached: {sorted(want - got)}; not launched: {sorted(got - want)}"


def _edges():
    """name -> predicate over (stage, fields, Ew)"""
    big = lambda k, d: k == "SE_POOL" and d.family == 12          # noqa: E731
    sm = lambda k, d, kind: k == kind and d.family == 11          # noqa: E731
    e = {
        "SE_POOL float4 generic at HW 1024": lambda k, w, d: k == "SE_POOL" and d.kernels == ("plane_reduce_kernel<0, true>",) and w["HW"] == 1024,
        "SE_POOL both sides of HW 256": lambda k, w, d: k == "SE_POOL" and w["HW"] == 256 and d.family == 11,
        "... 260": lambda k, w, d: k == "SE_POOL" and w["HW"] == 260 and d.family == 0,
        "SE_POOL HW 4092 generic": lambda k, w, d: k == "SE_POOL" and w["HW"] == 4092 and d.family == 0,
        "SE_POOL big: main loop only": lambda k, w, d: big(k, d) and d.main_trips and not d.tail_threads,
        "SE_POOL big: a tail of one float4 for thread 0": lambda k, w, d: big(k, d) and d.tail_threads == 1 and d.tail_trips == 1,
        "SE_POOL big: a whole tail trip": lambda k, w, d: big(k, d) and d.tail_threads == E.NTHREADS,
        "SE_POOL big: B * C > 4": lambda k, w, d: big(k, d) and d.idle_workgroup_waves,
        "SE_POOL big folded": lambda k, w, d: big(k, d) and w["FOLD"],
        "SE_POOL B = 1 at HW 64": lambda k, w, d: k == "SE_POOL" and w["B"] == 1 and w["HW"] == 64 and d.family == 0,
        "SE_POOL B * C = 8192 -> 12": lambda k, w, d: k == "SE_POOL" and w["B"] * w["C"] == 8192 and d.family == 12,
        "SE_POOL B * C = 8193 -> 0": lambda k, w, d: k == "SE_POOL" and w["B"] * w["C"] == 8193 and w["HW"] >= 4096 and d.family == 0,
        "SE_POOL scalar": lambda k, w, d: k == "SE_POOL" and not d.vec,
        "SE_BN_SUMS both sides of HW 64": lambda k, w, d: k == "SE_BN_SUMS" and w["HW"] == 64 and d.family == 11,
        "... 68": lambda k, w, d: k == "SE_BN_SUMS" and w["HW"] == 68 and d.family == 0,
        "SE_BN_SUMS big with a tail": lambda k, w, d: k == "SE_BN_SUMS" and d.family == 12 and d.tail_threads,
        "SE_BN_SUMS big without": lambda k, w, d: k == "SE_BN_SUMS" and d.family == 12 and not d.tail_threads,
        "SE_BN_SUMS B = 1 at HW 64": lambda k, w, d: k == "SE_BN_SUMS" and w["B"] == 1 and w["HW"] == 64 and d.family == 0,
        "CHANNEL_SUM C 255": lambda k, w, d: k == "CHANNEL_SUM" and w["C"] == 255 and w["HW"] == 512 and d.family == 0,
        "CHANNEL_SUM C 256": lambda k, w, d: k == "CHANNEL_SUM" and w["C"] == 256 and w["HW"] == 512 and d.family == 13,
        "CHANNEL_SUM HW 513": lambda k, w, d: k == "CHANNEL_SUM" and w["C"] == 256 and w["HW"] == 513 and d.family == 0,
        "CHANNEL_SUM rows: some waves unrolled, others only the tail": lambda k, w, d: d.family == 13 and d.mixed_rows,
        "CHANNEL_SUM rows: unrolled loop and tail in one wave": lambda k, w, d: d.family == 13 and any(u and t for u, t in d.rows_waves),
        "CHANNEL_SUM rows: two unrolled trips": lambda k, w, d: d.family == 13 and any(u == 2 for u, t in d.rows_waves),
        "CHANNEL_SUM rows: waves without a row": lambda k, w, d: d.family == 13 and any(u == 0 and t == 0 for u, t in d.rows_waves),
        "CHANNEL_SUM one chunk of 4096": lambda k, w, d: k == "CHANNEL_SUM" and d.family == 0 and d.chunks == 1 and d.last_chunk == E.CHUNK,
        "CHANNEL_SUM scalar, a second chunk of one element": lambda k, w, d: k == "CHANNEL_SUM" and not d.vec and d.chunks == 2 and d.last_chunk == 1,
        "CHANNEL_SUM float4, a third chunk of one float4": lambda k, w, d: k == "CHANNEL_SUM" and d.vec and d.chunks == 3 and d.last_chunk == 4,
        "SE_BN_COMBINE two lane trips": lambda k, w, d: k == "SE_BN_COMBINE" and d.rep_trips == 2,
        "SE_BN_COMBINE B = 64": lambda k, w, d: k == "SE_BN_COMBINE" and w["B"] == 64,
        "BN_BWD_REDUCE scalar, three chunks": lambda k, w, d: k == "BN_BWD_REDUCE" and not d.vec and d.chunks == 3,
        "BN_BWD_REDUCE float4, a second chunk of one float4": lambda k, w, d: k == "BN_BWD_REDUCE" and d.vec and d.chunks == 2 and d.last_chunk == 4,
        "BN_BWD_REDUCE GELU": lambda k, w, d: k == "BN_BWD_REDUCE" and w["ACT"] == T.GELU,
        "BN_BWD_REDUCE NOISE": lambda k, w, d: k == "BN_BWD_REDUCE" and w["NOISE"],
        "BN_BWD_APPLY chunked fused": lambda k, w, d: k == "BN_BWD_APPLY" and w["FORM"] == "fused" and d.chunks > 1,
        "BN_BWD_APPLY chunked COEF": lambda k, w, d: k == "BN_BWD_APPLY" and w["FORM"] == "coef" and d.chunks > 1,
        "BN_BWD_APPLY PS at B = 65": lambda k, w, d: k == "BN_BWD_APPLY" and w["PS"] and d.rep_trips == 2,
        "BN_FINALIZE COUNT = 1": lambda k, w, d: k == "BN_FINALIZE" and w["COUNT"] == 1 and w["TRAIN"],
        "BN_FINALIZE a negative variance": lambda k, w, d: k == "BN_FINALIZE" and w["NEG"],
        "BN_FINALIZE NREP 63": lambda k, w, d: k == "BN_FINALIZE" and w["NREP"] == 63,
        "BN_FINALIZE NREP 64": lambda k, w, d: k == "BN_FINALIZE" and w["NREP"] == 64,
        "SE_FC_WGRAD two sample chunks, the last of one": lambda k, w, d: d.family == 15 and d.sample_chunks == 2 and d.last_samples == 1,
        "SE_FC_WGRAD three sample chunks": lambda k, w, d: d.family == 15 and d.sample_chunks == 3,
        "SE_FC_WGRAD ragged channel tile": lambda k, w, d: d.family == 15 and d.ragged_ctile,
        "SE_FC_WGRAD C = 3": lambda k, w, d: d.family == 15 and w["C"] == 3,
        "SE stages at (C, Q) = (3840, 160), B = 2": lambda k, w, d: k == "SE_FC_BWD" and (w["B"], w["C"], w["Q"]) == (2, 3840, 160),
        "UPSAMPLE_ZERO trailing rows and columns": lambda k, w, d: k == "UPSAMPLE_ZERO" and d.extra["trailing"],
        "UPSAMPLE_ZERO S = 3": lambda k, w, d: k == "UPSAMPLE_ZERO" and w["S"] == 3,
        "UPSAMPLE_ZERO odd output": lambda k, w, d: k == "UPSAMPLE_ZERO" and w["HO"] == 15,
        "UPSAMPLE_ZERO a second grid-stride trip": lambda k, w, d: k == "UPSAMPLE_ZERO" and d.extra["trips"] >= 2,
    }
    for q, fams in ((64, (14, 15)), (65, (0, 15)), (224, (0, 15)), (225, (0, 0)), (1, (14, 15))):
        e[f"SE_FC_BWD at Q = {q}"] = lambda k, w, d, q=q, f=fams[0]: k == "SE_FC_BWD" and w["Q"] == q and d.family == f
        e[f"SE_FC_WGRAD at Q = {q}"] = lambda k, w, d, q=q, f=fams[1]: k == "SE_FC_WGRAD" and w["Q"] == q and d.family == f
    for kind in ("SE_POOL", "SE_BN_SUMS", "BN_BWD_APPLY", "BN_RESIDUAL"):
        hws = {"SE_POOL": (4, 16, 36, 64, 196, 256), "BN_RESIDUAL": (4, 36, 196, 256)}.get(kind, (4, 16, 36, 64))
        for hw in hws:
            e[f"{kind} small at HW {hw}"] = lambda k, w, d, kind=kind, hw=hw: sm(k, d, kind) and w["HW"] == hw
        e[f"{kind} small: B = 2"] = lambda k, w, d, kind=kind: sm(k, d, kind) and w["B"] == 2
        e[f"{kind} small: a short last batch chunk"] = lambda k, w, d, kind=kind: sm(k, d, kind) and d.last_short
        e[f"{kind} small: an empty last batch chunk"] = lambda k, w, d, kind=kind: sm(k, d, kind) and d.last_empty
        e[f"{kind} small: a ragged pass"] = lambda k, w, d, kind=kind: sm(k, d, kind) and d.ragged_pass
        e[f"{kind} small: idle lanes in a group"] = lambda k, w, d, kind=kind: sm(k, d, kind) and d.idle_lanes
        e[f"{kind} B = 1 -> generic"] = lambda k, w, d, kind=kind: k == kind and w["B"] == 1 and w["HW"] == 64 and d.family == 0
    e["SE_POOL small: one batch chunk at C >= 2048"] = lambda k, w, d: sm(k, d, "SE_POOL") and w["C"] >= 2048 and d.bsplit == 1 and w["B"] > 1
    for kind in ("SE_BN_SUMS", "BN_BWD_APPLY"):
        e[f"{kind} small: exactly four passes"] = lambda k, w, d, kind=kind: sm(k, d, kind) and d.full_unroll and not d.partial_unroll
        e[f"{kind} small: four passes plus one"] = lambda k, w, d, kind=kind: sm(k, d, kind) and d.full_unroll and d.partial_unroll
    for kind in ("SE_POOL", "BN_RESIDUAL"):
        for path in ("scalar", "wave"):
            e[f"{kind} folded, replicas by {path}"] = lambda k, w, d, kind=kind, path=path: k == kind and w["FOLD"] and d.rep_path == path
        for fam in (0, 11):
            e[f"{kind} folded on family {fam}"] = lambda k, w, d, kind=kind, fam=fam: k == kind and w["FOLD"] and d.family == fam
    for pro in (T.NONE, T.AFF, T.SILU, T.RELU):
        e[f"SE_POOL prologue {pro}"] = lambda k, w, d, pro=pro: k == "SE_POOL" and w["PRO"] == pro
    for pro in (T.NONE, T.SILU, T.RELU):
        for vec in (True, False):
            e[f"SE_BWD_REDUCE prologue {pro} vec {vec}"] = lambda k, w, d, pro=pro, vec=vec: k == "SE_BWD_REDUCE" and w["PRO"] == pro and d.vec == vec
    e["SE_BWD_REDUCE C = 1"] = lambda k, w, d: k == "SE_BWD_REDUCE" and w["C"] == 1
    for n in (1, 8, 9, 64):
        e[f"BN_BWD_REDUCE NREP {n}"] = lambda k, w, d, n=n: k == "BN_BWD_REDUCE" and w["NREP"] == n
        e[f"BN_BWD_FINALIZE NREP {n}"] = lambda k, w, d, n=n: k == "BN_BWD_FINALIZE" and w["NREP"] == n
        e[f"BN_BWD_APPLY fused NREP {n}"] = lambda k, w, d, n=n: k == "BN_BWD_APPLY" and w["FORM"] == "fused" and not w["PS"] and w["NREP"] == n
    for fam in (0, 11):
        e[f"BN_BWD_APPLY EVAL on family {fam}"] = lambda k, w, d, fam=fam: k == "BN_BWD_APPLY" and w["EVAL"] and d.family == fam
        e[f"BN_BWD_APPLY OUT_BF16 on family {fam}"] = lambda k, w, d, fam=fam: k == "BN_BWD_APPLY" and w["BF16"] and d.family == fam
        for mul, add in ((True, False), (False, True), (True, True), (False, False)):
            e[f"BN_BWD_APPLY recomputing, MULBC {mul} ADDBC {add}, family {fam}"] = (
                lambda k, w, d, fam=fam, mul=mul, add=add: k == "BN_BWD_APPLY" and w["ACT"] == T.SILU and (w["MUL"], w["ADD"]) == (mul, add) and d.family == fam)
        for ps in (True, False):
            for inplace in (True, False):
                e[f"BN_BWD_APPLY recomputing, PS {ps}, in place {inplace}, family {fam}"] = (
                    lambda k, w, d, fam=fam, ps=ps, inplace=inplace: k == "BN_BWD_APPLY" and w["ACT"] == T.SILU and w["PS"] == ps and w["INPLACE"] == inplace
                    and d.family == fam)
        for ident in (True, False):
            e[f"BN_RESIDUAL IDENT {ident} family {fam}"] = lambda k, w, d, fam=fam, ident=ident: k == "BN_RESIDUAL" and w["IDENT"] == ident and d.family == fam
            e[f"BN_RESIDUAL NOISE {ident} family {fam}"] = lambda k, w, d, fam=fam, ident=ident: k == "BN_RESIDUAL" and w["NOISE"] == ident and d.family == fam
    for mul, add in ((True, False), (False, True), (True, True), (False, False)):
        e[f"SE_BN_COMBINE MULBC {mul} ADDBC {add}"] = lambda k, w, d, mul=mul, add=add: k == "SE_BN_COMBINE" and (w["MUL"], w["ADD"]) == (mul, add)
    e["BN_RESIDUAL generic chunked"] = lambda k, w, d: k == "BN_RESIDUAL" and d.family == 0 and d.chunks > 1
    e["BN_RESIDUAL generic scalar"] = lambda k, w, d: k == "BN_RESIDUAL" and d.family == 0 and not d.vec
    e["BN_RESIDUAL HW 260"] = lambda k, w, d: k == "BN_RESIDUAL" and w["HW"] == 260 and d.family == 0
    return e


@pytest.mark.parametrize("edge", list(_edges()))
def test_required_edge_has_a_row(edge):
    pred = _edges()[edge]
    assert any(pred(k, w, d) for k, w, _, d in _rows()), edge


def test_issue_example_shapes():
    """the launchers' arithmetic at shapes worked out by hand"""
    d = E.dispatch("SE_POOL", B=25, C=400, HW=64)
    assert (d.lpp, d.pp, d.bsplit, d.bper, d.last_empty) == (16, 4, 6, 5, True)
    assert E.dispatch("SE_POOL", B=3, C=2052, HW=64).bsplit == 1
    d = E.dispatch("SE_POOL", B=3, C=10, HW=196)
    assert (d.lpp, d.pp, d.idle_lanes) == (64, 1, True)
    assert E.dispatch("SE_POOL", B=2, C=9, HW=4).lpp == 1
    d = E.dispatch("SE_POOL", B=1, C=3, HW=4100)
    assert (d.main_trips, d.tail_trips, d.tail_threads) == (2, 1, 1)
    assert E.dispatch("SE_POOL", B=1, C=3, HW=5120).tail_threads == 256
    assert E.dispatch("SE_BN_SUMS", B=2, C=4097, HW=4096).family == 0 and E.dispatch("SE_BN_SUMS", B=2, C=4096, HW=4096).family == 12      # nplanes <= 8192 (no GPU row)
    assert E.dispatch("CHANNEL_SUM", B=29, C=256, HW=1).rows_waves == ((1, 0), (0, 7), (0, 7), (0, 7))
    assert E.dispatch("CHANNEL_SUM", B=36, C=256, HW=1).rows_waves == ((1, 1),) * 4
    # few channels: the batch is cut into chunks of one pass each; only C >= 2048 keeps B = 16 in one chunk of four passes
    assert E.dispatch("SE_BN_SUMS", B=16, C=5, HW=64).bsplit == 4 and not E.dispatch("SE_BN_SUMS", B=16, C=5, HW=64).full_unroll
    d = E.dispatch("SE_BN_SUMS", B=16, C=2052, HW=64)
    assert d.bsplit == 1 and d.full_unroll and not d.partial_unroll
    d = E.dispatch("BN_BWD_APPLY", B=17, C=2052, HW=64, NREP=2)
    assert d.bsplit == 1 and d.full_unroll and d.partial_unroll


def _plans():
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet
    from s2lc_amd.plan import vit_plan as V
    from s2lc_amd.plan.unet_plan import plan_unet
    from s2lc_amd.utils import _prithvi_model_args

    for version, B, H in (("b5", 32, 256), ("b0", 8, 224)):
        m = EfficientnetUnet(EfficientNetConfig(version, 13, 4, class_distribution=[0.25] * 4))
        yield f"{version} training", plan_unet(m.spec, B, H, H, True, m._layout)
        yield f"{version} eval-mode input gradient", plan_unet(m.spec, B, H, H, False, m._layout, want_bwd=True, want_dx=True)
    a = _prithvi_model_args(1)
    spec = V.MaeSpec(a["img_size"], a["patch_size"], 1, a["tubelet_size"], a["in_chans"], a["embed_dim"], a["depth"], a["num_heads"],
                     a["decoder_embed_dim"], a["decoder_depth"], a["decoder_num_heads"], 4.0, False, True)
    yield "Prithvi MAE bs 64", V.plan_mae(spec, 64, 0.75, True)
    yield "Prithvi segmentation bs 16", V.plan_seg(V.SegSpec(dataclasses.replace(spec, decoder=False), 4, 256, 1, 0.1, False), 16, True)


def _collected_rows():
    """(stage, fields, family) of every parameter set pytest collects for the three row tests of tests/test_ew_kernels_gpu.py"""
    out = []
    for test in ("test_stage_row", "test_bn_finalize_row", "test_upsample_zero_exact"):
        marks = [m for m in getattr(T, test).pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and marks[0].kwargs["argnames"] == "kind,kw,fam", test
        out += [(test, *row) for row in marks[0].kwargs["argvalues"]]
    return [(k, kw, f) for _, k, kw, f in out]


def test_every_row_runs_in_exactly_one_gpu_test():
    """a row that no GPU test takes would still count as coverage in the tests of this file"""
    ran = _collected_rows()
    rows = list(T.all_rows())
    for row in rows:
        assert ran.count(row) == rows.count(row) == 1, f"{T.row_id(row[0], row[1])}: in {ran.count(row)} GPU parameter lists, {rows.count(row)} times in the tables"
    assert len(ran) == len(rows)
    for test in ("test_bn_finalize_row", "test_upsample_zero_exact"):
        kinds = {k for k, _, _ in T.rows_of(test)}
        assert len(kinds) == 1 and T.OWN_TEST[kinds.pop()] == test
    assert any(k == "UPSAMPLE_ZERO" for k, _, _ in T.PROD) and any(k == "BN_FINALIZE" for k, _, _ in T.PROD)


def _size(kind, f):
    if kind.startswith("SE_FC"):
        return f["CSQ"]
    if kind == "UPSAMPLE_ZERO":
        return (f["H"], f["W"], f["S"], f["HO"], f["WO"])
    return None if kind in ("BN_FINALIZE", "BN_BWD_FINALIZE", "SE_BN_COMBINE") else f["HW"]


def _key(kind, f):
    return (kind, E.form(kind, **f), _size(kind, f), E.facts(kind, **f))


def test_every_planned_stage_form_and_geometry_has_a_production_row():
    # rows that a GPU test runs (test_every_row_runs_in_exactly_one_gpu_test), hand tables and PROD alike
    have = {_key(kind, T.record_fields(kind, kw)) for kind, kw, fam in _collected_rows()}
    seen = {"EVAL": False, "UPSAMPLE_ZERO": False, "CHANNEL_SUM rows": False}
    for tag, plan in _plans():
        missing = set()
        for prog in (plan.fwd, plan.bwd):
            for kind, f in (prog.ops if prog is not None else ()):
                if kind not in E.KINDS:
                    continue
                if _key(kind, f) not in have:
                    missing.add(_key(kind, f)[:3])
                seen["EVAL"] |= kind == "BN_BWD_APPLY" and bool(f.get("EVAL"))
                seen["UPSAMPLE_ZERO"] |= kind == "UPSAMPLE_ZERO"
                seen["CHANNEL_SUM rows"] |= kind == "CHANNEL_SUM" and E.dispatch(kind, **f).family == 13 and tag.startswith("Prithvi")
        assert not missing, f"{tag}: (stage, form, plane size) without a production row of the same family and loop facts: {sorted(missing, key=str)}"
    assert all(seen.values()), seen


@pytest.mark.parametrize("kind", sorted({k for k, _, _ in T.all_rows()}))
def test_f32_oracle_alone_is_within_a_quarter_of_the_bar(kind):
    """a condition on the rows' inputs: where a row misses it, its data or seed changes, never the bar.  The 68 MB
    UPSAMPLE_ZERO row is left out (LARGE: it runs without the float64 oracle, and moves data only).  dY of an OUT_BF16 row is a value the stage rounds on store; the
    float64 oracle keeps it unrounded, so it is rounded to bf16 the same way before the comparison (tests/test_ew_kernels_gpu.py
    oracle_alone) - the condition is then the same quarter of the bar as everywhere."""
    worst = 0.0
    for k, kw, fam in T.all_rows():
        if k != kind or kw.get("LARGE"):
            continue
        c, s = T.build(k, kw, T.row_seed(k, kw))
        for name, v in T.oracle_alone(c, s).items():
            lim = 0.25 * s["tol"]
            assert v <= lim, f"{T.row_id(k, kw)}:{name}: the f32 oracle is {v:.2e} from float64, more than {lim:.1e}"
            worst = max(worst, v / s["tol"])
    print(f"{kind}: the f32 oracle alone uses at most {worst:.3f} of a bar")
