"""Coverage of the depthwise GPU tables (tests/test_dwconv_ops_gpu.py), checked without a GPU: the launch macros of
csrc/dwconv.hip are parsed, and the tables must reach every instantiation they launch (crossed with each prologue), every parity
body of dwconv_dgrad_s2_kernel, every required run-time edge, and every (op, instantiation) of the b5 256² bs 32 and b0 224² bs 8
training plans at that plan's own geometry.  Which kernel a row reaches is tests/dw_dispatch.py's restatement of the launchers;
the family column of each row must agree with it (the GPU test then checks the family the launcher reports)."""
import re
from pathlib import Path

import pytest

from tests import test_dwconv_ops_gpu as T
from tests.dw_dispatch import BAND, IMAGE_LOOP, PLANE, dispatch, same_pads

SRC = Path(__file__).resolve().parents[1] / "sentinel2-landcover-classification_amd" / "csrc" / "dwconv.hip"

# macro -> (op, family, kernel); the band macros carry K, S (or K, PR) and pick the padding at run time
MACROS = {
    "DW_PLANE": ("fwd", PLANE, "dwconv_fwd_plane_kernel"), "DW_S2": ("fwd", PLANE, "dwconv_fwd_plane_s2_kernel"),
    "DW_FWD_PL": ("fwd", BAND, "dwconv_fwd_kernel"),
    "DW_DGP": ("dgrad", PLANE, "dwconv_dgrad_plane_kernel"), "DW_DG2": ("dgrad", PLANE, "dwconv_dgrad_plane_s2_kernel"),
    "DW_DG": ("dgrad", BAND, "dwconv_dgrad_s1_kernel"),
    "DW_WGP": ("wgrad", PLANE, "dwconv_wgrad_plane_kernel"), "DW_WGB_PL": ("wgrad", IMAGE_LOOP, "dwconv_wgrad_kernel"),
    "DW_WG_PL": ("wgrad", BAND, "dwconv_wgrad_kernel"),
}
PL_MACRO = {"DW_FWD_PL": "DW_FWD", "DW_WGB_PL": "DW_WGB", "DW_WG_PL": "DW_WG"}     # ..._PL(K, S) -> inner(K, S, PL) per PL

# TF-SAME padding fixes the padding of every band instantiation: left padding (K - 1) // 2 at stride 1, at stride 2 (K - 2) // 2
# for an even width and (K - 1) // 2 for an odd one.  The other PL / PR values the macros instantiate are never launched.
REACHABLE_PL = {(3, 1, 1), (5, 1, 2), (3, 2, 0), (3, 2, 1), (5, 2, 1), (5, 2, 2)}       # band fwd / wgrad <K, S, PL>
REACHABLE_PR = {(3, 1), (5, 2)}                                                        # dwconv_dgrad_s1_kernel<K, PR>: PR = K - 1 - PL


def _src():
    return SRC.read_text()


def _defines(src):
    """name -> body of every DW_* macro (continuation lines joined)"""
    out = {}
    for m in re.finditer(r"#define (DW_\w+)\(([^)]*)\)((?:[^\n]*\\\n)*[^\n]*)", src):
        out[m.group(1)] = m.group(3).replace("\\\n", " ")
    return out


def launched():
    """{(op, family, kernel, args): set of PRO} of every instantiation csrc/dwconv.hip launches"""
    src = _src()
    defs = _defines(src)
    body = re.sub(r"#define [^\n]*(?:\\\n[^\n]*)*", "", src)          # invocations only
    out = {}
    for m in re.finditer(r"\b(DW_\w+)\(\s*(\d+)\s*,\s*(\d+)\s*(?:,\s*(\d+)\s*)?\)", body):
        name, args = m.group(1), tuple(int(a) for a in m.groups()[1:] if a is not None)
        assert name in MACROS, f"csrc/dwconv.hip launches through {name}, which this test does not know: add it to MACROS and the tables"
        op, fam, kern = MACROS[name]
        d = defs[PL_MACRO.get(name, name)]
        pros = {p for p in ("S2K_PRO_NONE", "S2K_PRO_SILU") if p in d}
        if name in PL_MACRO:
            for pl in (int(v) for v in re.findall(r"\w+\(KK, SS, (\d)\)", defs[name])):
                out.setdefault((op, fam, kern, args + (pl,)), set()).update(pros)
        else:
            out.setdefault((op, fam, kern, args), set()).update(pros)
    for k in re.findall(r"dwconv_dgrad_s2_kernel<(\d+)>", body):
        out.setdefault(("dgrad", BAND, "dwconv_dgrad_s2_kernel", (int(k),)), set()).update({"run time"})
    return out


def reachable(inst):
    op, fam, kern, args = inst
    if kern in ("dwconv_fwd_kernel", "dwconv_wgrad_kernel"):
        return args in REACHABLE_PL
    if kern == "dwconv_dgrad_s1_kernel":
        return args in REACHABLE_PR
    return True


def _rows():
    """(op, geometry, family, prologues) of every GPU case"""
    pro2 = {0, 2}
    for r in T.FWD:
        yield "fwd", r[:6], r[6], pro2
    for r in T.DGRAD:
        yield "dgrad", r[:6], r[6], pro2
    for r in T.WGRAD:
        yield "wgrad", r[:6], r[6], pro2
    for r in T.PROD_FWD:
        yield "fwd", r[:6], r[6], {r[7]}
    for r in T.PROD_DGRAD:
        yield "dgrad", r[:6], r[6], {r[7]}
    for r in T.PROD_WGRAD:
        yield "wgrad", r[:6], r[6], {r[7]}
    for op, r in T.SILU_RANGE:
        yield op, r[:6], r[6], {2}


def test_macro_parse_finds_every_launch_site():
    got = launched()
    kernels = {k[2] for k in got}
    assert len(kernels) == 9 and len(got) >= 40, sorted(got)
    assert {k for k in got if not reachable(k)} == {
        ("fwd", BAND, "dwconv_fwd_kernel", a) for a in ((3, 1, 0), (3, 1, 2), (5, 1, 0), (5, 1, 1), (3, 2, 2), (5, 2, 0))} | {
        ("wgrad", f, "dwconv_wgrad_kernel", a) for f in (BAND, IMAGE_LOOP) for a in ((3, 1, 0), (3, 1, 2), (5, 1, 0), (5, 1, 1), (3, 2, 2), (5, 2, 0))} | {
        ("dgrad", BAND, "dwconv_dgrad_s1_kernel", a) for a in ((3, 0), (3, 2), (5, 0), (5, 1))}


@pytest.mark.parametrize("op,geo,fam", [(op, g, f) for op, g, f, _ in _rows()])
def test_table_family_matches_dispatch(op, geo, fam):
    d = dispatch(op, *geo)
    assert d.family == fam, f"{op} {geo}: family column {fam}, the launcher takes {d.kernel}{d.args} (family {d.family})"


def test_tables_reach_every_instantiation_with_each_prologue():
    want = {k: v for k, v in launched().items() if reachable(k)}
    got = {}
    for op, geo, _, pros in _rows():
        got.setdefault(dispatch(op, *geo).inst, set()).update(pros)
    name = {0: "S2K_PRO_NONE", 2: "S2K_PRO_SILU"}
    missing = []
    for inst, pros in sorted(want.items()):
        have = {name[p] for p in got.get(inst, ())} | ({"run time"} if inst in got else set())
        if not pros <= have:
            missing.append((inst, sorted(pros - have)))
    assert not missing, f"instantiations (with prologues) no GPU case reaches: {missing}"
    assert set(got) <= set(want), f"cases reach instantiations the macros do not launch: {sorted(set(got) - set(want))}"


def test_every_dgrad_s2_parity_body_runs_for_k3_and_k5():
    for K in (3, 5):
        par = set()
        multi = set()
        for op, geo, _, _ in _rows():
            d = dispatch(op, *geo)
            if d.kernel == "dwconv_dgrad_s2_kernel" and d.args == (K,):
                par |= d.parities
                if d.bands > 1 and d.rt % 2 == 1:
                    multi |= d.parities
        assert par == {(0, 0), (0, 1), (1, 0), (1, 1)}, (K, par)
        assert len(multi) == 4, f"k{K}: multi-band cases with odd rows per band reach only {sorted(multi)}"


def _edges():
    """name -> predicate over (op, geometry, Dw, prologues)"""
    return {
        "a plane chunk spanning two images, fwd_plane": lambda op, g, d, p: d.kernel == "dwconv_fwd_plane_kernel" and d.spans,
        "... fwd_plane_s2": lambda op, g, d, p: d.kernel == "dwconv_fwd_plane_s2_kernel" and d.spans,
        "... dgrad_plane": lambda op, g, d, p: d.kernel == "dwconv_dgrad_plane_kernel" and d.spans,
        "... dgrad_plane_s2": lambda op, g, d, p: d.kernel == "dwconv_dgrad_plane_s2_kernel" and d.spans,
        "... wgrad_plane": lambda op, g, d, p: d.kernel == "dwconv_wgrad_plane_kernel" and d.spans,
        "the plane wgrad split capped at 48 waves": lambda op, g, d, p: d.capped,
        "image loop: bloop > 1 with a ragged last group": lambda op, g, d, p: d.bloop > 1 and d.ragged,
        "image loop: C not a multiple of its channel group": lambda op, g, d, p: d.bloop > 1 and g[1] % d.ppb != 0,
        "C % 4 != 0 on a plane kernel": lambda op, g, d, p: d.family == PLANE and g[1] % 4 != 0,
        "C % 4 != 0 on a band kernel": lambda op, g, d, p: d.family == BAND and g[1] % 4 != 0,
        "W > 256: the vector stager's plain loop, fwd": lambda op, g, d, p: op == "fwd" and d.wide and g[3] > 256,
        "... dgrad s1": lambda op, g, d, p: d.kernel == "dwconv_dgrad_s1_kernel" and d.wide,
        "... wgrad": lambda op, g, d, p: op == "wgrad" and d.wide,
        "WO >= 62: the scalar stager's passes in dgrad_s2": lambda op, g, d, p: d.kernel == "dwconv_dgrad_s2_kernel" and d.wide,
        "multi-band band forward": lambda op, g, d, p: d.kernel == "dwconv_fwd_kernel" and d.bands > 1,
    }


@pytest.mark.parametrize("edge", list(_edges()))
def test_required_edge_has_a_case(edge):
    pred = _edges()[edge]
    assert any(pred(op, g, dispatch(op, *g), p) for op, g, _, p in _rows()), edge


def test_silu_beyond_exp_range_in_every_op_and_family():
    seen = {(op, f) for op, r in T.SILU_RANGE for f in [r[6]]}
    assert {(op, f) for op in ("fwd", "dgrad") for f in (BAND, PLANE)} | {("wgrad", f) for f in (BAND, PLANE, IMAGE_LOOP)} <= seen


def test_issue_example_shapes():
    """the launchers' arithmetic at shapes worked out by hand (no GPU case needs to run them all)"""
    assert dispatch("dgrad", 2, 6, 15, 14, 3, 2).parities == {(1, 0)}
    assert dispatch("dgrad", 2, 6, 14, 15, 3, 2).parities == {(0, 1)}
    assert dispatch("fwd", 2, 6, 14, 15, 3, 2).inst == ("fwd", BAND, "dwconv_fwd_kernel", (3, 2, 1))
    assert dispatch("dgrad", 2, 8, 56, 56, 5, 2).parities == {(1, 1)}
    assert dispatch("fwd", 2, 8, 56, 56, 5, 2).inst == ("fwd", BAND, "dwconv_fwd_kernel", (5, 2, 1))
    for K in (3, 5):
        d = dispatch("dgrad", 1, 3, 130, 130, K, 2)
        assert d.bands > 1 and d.rt % 2 == 1 and len(d.parities) == 2
    for op in ("fwd", "dgrad"):
        assert dispatch(op, 2, 6, 128, 128, 5, 2).inst[2:] == (f"dwconv_{op}_plane_s2_kernel", (5, 64, 4))
    d = dispatch("wgrad", 7, 5, 128, 128, 3, 1)
    assert d.capped and d.bchunk == 3 and d.spans
    d = dispatch("fwd", 5, 2000, 64, 64, 3, 1)
    assert d.bchunk == 5 and d.bands == 4 and d.spans
    for K in (3, 5):
        d = dispatch("wgrad", 9, 2000, 7, 7, K, 1)
        assert d.family == IMAGE_LOOP and d.bloop == 2 and d.ragged
    d = dispatch("wgrad", 200, 40, 14, 14, 3, 1)
    assert d.family == IMAGE_LOOP and d.bloop == 3 and d.ragged
    # rows of 300 take the plain loop; a 300-row plane of 20 columns is only tall (2 bands)
    assert dispatch("fwd", 1, 4, 20, 300, 3, 1).wide and not dispatch("fwd", 1, 4, 300, 20, 3, 1).wide
    assert dispatch("fwd", 1, 4, 300, 20, 3, 1).bands == 2


def _plan_stages(version, B, H):
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet
    from s2lc_amd.plan.unet_plan import plan_unet

    model = EfficientnetUnet(EfficientNetConfig(version, 13, 4, class_distribution=[0.25] * 4))
    plan = plan_unet(model.spec, B, H, H, True, model._layout)
    ops = {"DWCONV_FWD": "fwd", "DWCONV_DGRAD": "dgrad", "DWCONV_WGRAD": "wgrad"}
    out = set()
    for prog in (plan.fwd, plan.bwd):
        for kind, f in prog.ops:
            if kind in ops:
                geo = (f["B"], f["C"], f["H"], f["W"], f["K"], f["STRIDE"])
                # the planner's padding is TF-SAME, which the tables and tests/dw_dispatch.py assume
                assert (f["HO"], f["PAD_T"]) == same_pads(f["H"], f["K"], f["STRIDE"]) and (f["WO"], f["PAD_L"]) == same_pads(f["W"], f["K"], f["STRIDE"])
                out.add((ops[kind], geo))
    return out


@pytest.mark.parametrize("version,B,H", [("b5", 32, 256), ("b0", 8, 224)])
def test_every_training_plan_instantiation_has_a_production_case(version, B, H):
    stages = _plan_stages(version, B, H)
    assert stages
    prod = {(op, g) for op, tab in (("fwd", T.PROD_FWD), ("dgrad", T.PROD_DGRAD), ("wgrad", T.PROD_WGRAD)) for g in (r[:6] for r in tab)}
    used = {dispatch(op, *g).inst for op, g in stages}
    at_plan_shape = {dispatch(op, *g).inst for op, g in prod & stages}
    assert used <= at_plan_shape, f"{version}: instantiations without a case at the plan's geometry: {sorted(used - at_plan_shape)}"
    every = {dispatch(op, *g).inst for op, g, _, _ in _rows()}
    assert used <= every


def test_pinned_families_of_the_older_depthwise_cases_match_dispatch():
    from tests import test_ops_gpu as O

    for r in O.DW_GEOS:
        assert tuple(dispatch(op, *r[:6]).family for op in ("fwd", "dgrad", "wgrad")) == r[6], r
