"""Coverage of the f32 weight-gradient GPU tables (tests/test_wgrad_kernels_gpu.py), checked without a GPU.

The launch sites of csrc/wgrad.hip, wgrad_pc.hip and wgrad_q4.hip are parsed into the set of template instantiations the chain can
launch at default tuning; every threshold tests/wgrad_dispatch.py restates is looked up in the source text.  The tables must reach
every such instantiation, every required edge per kernel that can meet it, and the instantiation and edges of every WGRAD record of
the production plans; the family column of every row (and of the older f32 WGRAD rows in tests/test_ops_gpu.py) must be what the
restated launcher takes; and on every row's data the f32 oracle alone must stay within a quarter of each bar against the float64
oracle."""
import functools
import itertools
import re
from pathlib import Path

import pytest
import torch

from tests import test_wgrad_kernels_gpu as T
from tests import wgrad_dispatch as WD
from tests.wgrad_dispatch import GENERIC, PC, Q4, WG_GATHER, WG_PIX, WG_SPATIAL

CSRC = Path(__file__).resolve().parents[1] / "sentinel2-landcover-classification_amd" / "csrc"
PRO = {"S2K_PRO_NONE": 0, "S2K_PRO_AFFINE": 1, "S2K_PRO_SILU": 2, "S2K_PRO_RELU": 3, "S2K_PRO_GELU": 4}
MODES = {"WG_PIX": WG_PIX, "WG_SPATIAL": WG_SPATIAL, "WG_GATHER": WG_GATHER}
NO, SI, RE, GE = 0, 2, 3, 4

WIDE_OFF = "S2K_WG_WIDE is 0"
WSC_OFF = ("needs a stride-1 3x3 record with 64-wide tiles and a halo of <= 256 elements: wgrad_pc's (1, 64) form takes it first, and with a "
           "prologue that form lacks the generic ladder has no instantiation either")


def _src(name):
    return (CSRC / name).read_text()


def _ints(m):
    return tuple(int(v) for v in m)


def _body(src, head):
    """the text of the function that starts with `head`, up to the first line that is a lone closing brace"""
    at = src.index(head)
    return src[at:src.index("\n}\n", at)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the instantiations each file can launch: {(kernel, template arguments): reason it cannot be reached at default tuning, or None}
# ---------------------------------------------------------------------------------------------------------------------------------
def generic_ladder():
    """launch_wg's prologue ladder: {mode or "WSC": [(P, Q), ...]} in the launcher's order"""
    body = _body(_src("wgrad.hip"), "static int launch_wg(WgradP& p, hipStream_t st)")
    out = {"WSC": [], WG_GATHER: [], WG_SPATIAL: [], WG_PIX: []}
    where, pix_next, pix_block = None, False, False
    for line in body.split("\n"):
        s = line.strip()
        if s.startswith("if constexpr (WSC != 0) {"):
            where = "WSC"
        elif s.startswith("if constexpr (MODE == WG_GATHER) {"):
            where = WG_GATHER
        elif s == "} else {":
            where = "else"
        elif s == "if constexpr (MODE == WG_PIX)":
            pix_next = True
            continue
        elif s == "if constexpr (MODE == WG_PIX) {":
            pix_block = True
        elif s == "}" and pix_block:
            pix_block = False
        elif s == "}" and where == "WSC":
            where = None
        m = re.search(r"return launch_wg2<MODE, T, WM, WN, WVM, WVN, WVK, NPJ, EPT, (S2K_PRO_\w+), (S2K_PRO_\w+)(, WSC)?>\(p, st\);", s)
        if m:
            cond = re.match(r"if \(p([pq]) == (S2K_PRO_\w+) && p([pq]) == (S2K_PRO_\w+)\)", s)
            assert cond, s
            said = {cond.group(1): cond.group(2), cond.group(3): cond.group(4)}
            assert (said["p"], said["q"]) == (m.group(1), m.group(2)), f"a ladder line tests one pair and launches another: {s}"
            pair = (PRO[m.group(1)], PRO[m.group(2)])
            assert bool(m.group(3)) == (where == "WSC"), s
            if where == "else":
                out[WG_PIX].append(pair)
                if not (pix_next or pix_block):
                    out[WG_SPATIAL].append(pair)
            else:
                out[where].append(pair)
        pix_next = False
    return out


def generic_launches():
    src = _src("wgrad.hip")
    ladder = generic_ladder()
    main = src[src.index("int launch_wgrad(const S2kOp& op, const Ctx& c)"):]
    out, sites = {}, []
    for m in re.finditer(r"launch_wg<(WG_\w+), ([\d, ]+)>\(p, st\)", main):
        cfg = (MODES[m.group(1)],) + _ints(m.group(2).split(","))
        line = main[main.rfind("\n", 0, m.start()):m.start()]
        sites.append(cfg)
        if len(cfg) == 10:
            for pair in ladder["WSC"]:
                out[("wgrad_kernel", cfg[:9] + pair + (cfg[9],))] = WSC_OFF
            continue
        for pair in ladder[cfg[0]]:
            out[("wgrad_kernel", cfg + pair + (0,))] = WIDE_OFF if "if (wide)" in line else None
    for cfg in sites:      # the ladder of a WSC launch falls through to the same arguments without WSC: the EPT 1 form's own instantiations
        assert len(cfg) == 9 or all(("wgrad_kernel", cfg[:9] + pair + (0,)) in out for pair in ladder[cfg[0]])
    return out, sites


def pc_launches():
    src = _src("wgrad_pc.hip")
    out = {}
    main = src[src.index("int launch_wgrad_pc("):]
    body = re.sub(r"#define [^\n]*(?:\\\n[^\n]*)*", "", main)
    geoms = [_ints(m) for m in re.findall(r"PC_SPATIAL_CASE\((\d+), (\d+)\)", body)]
    assert "if (R == RR && XWe == XX) { setup(RR, XX); return launch_pc_spatial<RR, XX>(p, st); }" in main
    sp = [(PRO[a], PRO[b]) for a, b in re.findall(r"launch_pc2<WG_SPATIAL, 9, 1, 1, 2, 2, 1, 64, R, XWE, (S2K_PRO_\w+), (S2K_PRO_\w+)>", src)]
    for (r, xwe), pair in itertools.product(geoms, sp):
        out[("wgrad_pc_kernel", (WG_SPATIAL, 9, 1, 1, 2, 2, 1, 64, r, xwe) + pair)] = None
    thin = [(PRO[a], PRO[b]) for a, b in re.findall(r"launch_pc2<WG_SPATIAL, 9, 1, 1, WVM, 1, 4 / WVM, 128, 2, 64, (S2K_PRO_\w+), (S2K_PRO_\w+)>", src)]
    wvms = _ints(re.findall(r"launch_pc_spatial_thin<(\d)>\(p, st\)", main))
    for wvm, pair in itertools.product(wvms, thin):
        out[("wgrad_pc_kernel", (WG_SPATIAL, 9, 1, 1, wvm, 1, 4 // wvm, 128, 2, 64) + pair)] = None
    pix = [(PRO[a], PRO[b]) for a, b in re.findall(r"launch_pc2<WG_PIX, 1, WM, WN, 2, 2, 1, 64, 1, 64, (S2K_PRO_\w+), (S2K_PRO_\w+)>", src)]
    tiles = [_ints(m) for m in re.findall(r"launch_pc_pix<(\d), (\d)>\(p, st\)", main)]
    for (wm, wn), pair in itertools.product(tiles, pix):
        out[("wgrad_pc_kernel", (WG_PIX, 1, wm, wn, 2, 2, 1, 64, 1, 64) + pair)] = None
    return out, dict(geoms=geoms, sp=sp, thin=thin, wvms=wvms, pix=pix, tiles=tiles)


def q4_launches():
    src = _src("wgrad_q4.hip")
    pairs = [(PRO[a], PRO[b]) for a, b in re.findall(r"return launch_q4w<WM, WN, (S2K_PRO_\w+), (S2K_PRO_\w+)>\(p, st\);", src)]
    tiles = [_ints(m) for m in re.findall(r"return launch_q4w_pro<(\d), (\d)>\(p, st\);", src)]
    return {("wgrad_q4_kernel", t + pair): None for t, pair in itertools.product(tiles, pairs)}, pairs, tiles


@functools.lru_cache(maxsize=None)
def launched():
    out = {}
    for part in (generic_launches()[0], pc_launches()[0], q4_launches()[0]):
        assert not set(part) & set(out)
        out.update(part)
    return out


def reachable():
    return {k for k, why in launched().items() if why is None}


KERNELS = ("wgrad_kernel", "wgrad_pc_kernel", "wgrad_q4_kernel")


def test_parse_finds_every_launch_site():
    got = launched()
    per = {k: sum(1 for i in got if i[0] == k) for k in KERNELS}
    reach = {k: sum(1 for i in reachable() if i[0] == k) for k in KERNELS}
    print("launched", per, "reachable", reach)
    assert per == {"wgrad_kernel": 64, "wgrad_pc_kernel": 30, "wgrad_q4_kernel": 16}, per
    assert reach == {"wgrad_kernel": 60, "wgrad_pc_kernel": 30, "wgrad_q4_kernel": 16}, reach
    # per mode of the generic kernel: 2 gather geometries x 4 P prologues, 6 pixel geometries x 7 pairs, 7 3x3 forms x 2 (one of them
    # with WSC = 66)
    by_mode = {m: sum(1 for k, a in got if k == "wgrad_kernel" and a[0] == m) for m in (WG_PIX, WG_SPATIAL, WG_GATHER)}
    assert by_mode == {WG_PIX: 42, WG_SPATIAL: 14, WG_GATHER: 8}, by_mode
    # what default tuning cannot reach, by name: the 128-pixel 3x3 tile of layers that are not thin (S2K_WG_WIDE = 1), and the form with
    # the compile-time halo stride of 66
    unreachable = {k: why for k, why in got.items() if why is not None}
    assert unreachable == {
        **{("wgrad_kernel", WD.G_SP_WIDE + (NO, q, 0)): WIDE_OFF for q in (NO, RE)},
        **{("wgrad_kernel", WD.G_SP_WSC[:9] + (NO, q, 66)): WSC_OFF for q in (NO, RE)}}, unreachable


def test_the_wsc_form_is_unreachable_for_the_reason_given():
    """WSC = 66 needs WS = XWe + 2 = 66 on the 64-slot kernel at stride 1 (stride 2: WS = 2 XWe + 1 is odd), so XW in (63, 64), R = 1 and
    the record is one wgrad_pc's (1, 64) form takes unless its prologue pair is not (NONE, NONE | ReLU) - and then the generic ladder
    refuses it.  Swept over every such record shape."""
    for WO, HO, M, C, prop, proq in itertools.product((63, 64, 65, 127, 128, 200), (1, 2, 5), (33, 64, 65, 200), (33, 40, 200), (NO, RE, SI), (NO, RE, SI, GE)):
        v = WD.dispatch(B=2, M=M, C=C, H=HO, W=WO, KH=3, KW=3, PAD_T=1, PAD_L=1, PROP=prop, PROQ=proq)
        assert v.result == "error" or v.args[-1] == 0 or v.kernel != "wgrad_kernel", (WO, HO, M, C, prop, proq, v.inst)
        if (prop, proq) in WD.PC_SPATIAL_PRO and not (M <= 64 and C <= 32):
            assert v.inst == ("wgrad_pc_kernel", (WG_SPATIAL, 9, 1, 1, 2, 2, 1, 64, 1, 64, prop, proq)), v.inst


def test_the_ept2_form_needs_stride_2_off_thin_layers():
    """the 64-slot 3x3 kernels: a stride-1 halo (R + 2) x (XWe + 2) with R * XWe <= 64 holds at most 198 elements, one per thread"""
    worst = max((64 // xwe + 2) * (xwe + 2) for xwe in range(2, 65, 2))
    assert worst == 198 and worst <= WD.NTHREADS
    for WO, HO in itertools.product(range(1, 70), (1, 3, 8, 40)):
        v = WD.dispatch(B=1, M=40, C=40, H=HO, W=WO, KH=3, KW=3, PAD_T=1, PAD_L=1)
        assert v.result == PC or v.args[:9] == WD.G_SP_EPT1, (WO, HO, v.inst)


def test_prologue_ladders_and_tiles_of_the_restatement_are_the_parsed_ones():
    ladder = generic_ladder()
    assert tuple(ladder["WSC"]) == WD.G_PRO_WSC
    for mode in (WG_GATHER, WG_SPATIAL, WG_PIX):
        assert tuple(ladder[mode]) == WD.G_PRO[mode], mode
    sites = generic_launches()[1]
    assert sites == [WD.G_GATHER_THIN, WD.G_GATHER, WD.G_PIX_THIN256, WD.G_PIX_THIN, WD.G_PIX[(128, 128)], WD.G_PIX[(128, 64)], WD.G_PIX[(64, 128)],
                     WD.G_PIX[(64, 64)], WD.G_SP_THIN_MC, WD.G_SP_THIN_M, WD.G_SP_THIN_C, WD.G_SP_WIDE, WD.G_SP_WSC, WD.G_SP_EPT1, WD.G_SP_EPT2], sites
    pc = pc_launches()[1]
    assert tuple(pc["geoms"]) == WD.PC_GEOMS and tuple(pc["sp"]) == WD.PC_SPATIAL_PRO == tuple(pc["thin"]) and tuple(pc["pix"]) == WD.PC_PIX_PRO
    assert pc["wvms"] == (1, 2) and sorted(pc["tiles"]) == [(1, 1), (1, 2), (2, 1), (2, 2)]
    assert {w: (1, 1, w, 1, 4 // w) for w in (1, 2)} == {1: WD.PC_THIN[True], 2: WD.PC_THIN[False]}
    _, pairs, tiles = q4_launches()
    assert tuple(pairs) == WD.Q4_PRO and sorted(tiles) == [(1, 1), (1, 2), (2, 1), (2, 2)]


@pytest.mark.parametrize("name", list(WD.TUNE))
def test_every_tuning_default_is_the_one_the_restatement_assumes(name):
    got = {k: int(v) for k, v in re.findall(r'tune_int\("(\w+)", (-?\d+)\)', _src(name))}
    assert got == WD.TUNE[name], f"{name}: a tuning switch changed or was added: restate it in tests/wgrad_dispatch.py"


def _thresholds():
    """file -> source fragments that state the thresholds tests/wgrad_dispatch.py uses, written from its constants"""
    C = WD
    pad = f"{C.EDGE_PAD}"
    edge = f"auto edge = [](int n) {{ return (n > 64 && (double)cdiv(n, 128) * 128 / n <= {pad}) ? 128 : 64; }};"
    search = [f"const int s_hi = std::min(max_splits, std::max(1, {C.SPLIT_ROUNDS} * slots / mc));", "for (int sp = 1; sp <= s_hi; ++sp) {",
              "const double rounds = (double)cdiv(mc * sp, slots);", f"if (cost < best * {C.BETTER}) {{ best = cost; splits = sp; }}",
              "p.tiles_per_split = cdiv(p.ntiles, splits);\n    splits = cdiv(p.ntiles, p.tiles_per_split);", "double best = 1e30;"]
    span = ["(p.HWp % NPJ) == 0) ? 1 : std::min<int64_t>(p.B, (NPJ - 2) / p.HWp + 2);",
            "const int64_t need = std::max((int64_t)p.M * p.HWp, (int64_t)p.C * p.HWq) * 4 * span;", "if (need >= 0x7ffffff0ll)"]
    thin = f"(p.M <= {C.THIN_SIDE}) || (p.M <= {C.THIN_M2} && p.C <= {C.THIN_C2});"

    def site(cfg):
        return "launch_wg<" + ", ".join(["WG_PIX", "WG_SPATIAL", "WG_GATHER"][cfg[0]] if i == 0 else str(a) for i, a in enumerate(cfg)) + ">(p, st);"
    return {
        "wgrad.h": [f"constexpr int WG_EPT_MAX = {C.WG_EPT_MAX};", f"enum {{ WG_PIX = {WG_PIX}, WG_SPATIAL = {WG_SPATIAL}, WG_GATHER = {WG_GATHER} }};"],
        "wgrad_q4.hip": [
            "if (!enabled || p.gatep || p.p_bf16) return 1;", "if (p.gateq && (p.proq != S2K_PRO_SILU || p.T != 1 || !(enabled & 4))) return 1;",
            "if (mode != S2K_MODE_CONV || p.S != 1 || p.H != p.HO || p.W != p.WO) return 1;",
            "if ((reinterpret_cast<uintptr_t>(p.p) | reinterpret_cast<uintptr_t>(p.q)) & 15) return 1;", "if (p.T != 1 || !(enabled & 1)) return 1;",
            f"if (p.M <= {C.THIN_SIDE} || p.C <= {C.THIN_SIDE} || (p.HWp & 3) || p.HWq != p.HWp) return 1;",
            f"if ((int64_t)p.B * p.HWp < {C.MIN_PIXELS} || (int64_t)p.B * p.HWp > 0x7fffffffll) return 1;", edge,
            "constexpr int BM = WM * 64, BC = WN * 64, NPJ = 64;", "const int slots = 256;",
            f"int max_splits = std::max(1, std::min({C.MAX_SPLITS}, cdiv(p.ntiles, {C.MIN_TILES_PER_SPLIT})));",
            "const double cost = rounds * ((double)cdiv(p.ntiles, sp) + (WM * WN >= 4 ? 2.0 : 1.0));", "g_s2k_variant = 4;",
            "(p.HWp % NPJ) == 0 ? 1 : std::min<int64_t>(p.B, (NPJ - 2) / p.HWp + 2);"] + search + span[1:],
        "wgrad_pc.hip": [
            "if (p.gatep || p.gateq) return 1;",
            "if ((enabled & 1) && mode == S2K_MODE_CONV && p.T == 9 && p.S == 1 && p.KH == 3 && p.KW == 3 && p.H == p.HO && p.W == p.WO) {",
            "const bool thin = " + thin, f"if (p.C > {C.THIN_SIDE} || p.WO < {C.PC_THIN_MIN_WO} || p.HO < {C.PC_THIN_MIN_HO}) return 1;",
            "p.R = 2; p.XW = 64; p.XWe = 64; p.IR = 4; p.IC = 66; p.WS = 66;", f"return p.M <= {C.THIN_SIDE} ? launch_pc_spatial_thin<1>(p, st) : launch_pc_spatial_thin<2>(p, st);",
            "const int XW = p.WO <= 64 ? p.WO : 64;", "const int XWe = (XW + 1) & ~1;", "int R = 64 / XWe;", "if (R > p.HO) R = p.HO;",
            *[f"PC_SPATIAL_CASE({r}, {x})" for r, x in C.PC_GEOMS],
            "if ((enabled & 2) && mode == S2K_MODE_CONV && p.T == 1 && p.S == 1 && p.H == p.HO && p.W == p.WO) {",
            f"if (p.M <= {C.THIN_SIDE} || p.C <= {C.THIN_SIDE}) return 1;", f"if (npix < {C.MIN_PIXELS}) return 1;", edge,
            "if (p.prop != S2K_PRO_NONE) return 1;", "const int slots = 256;", f"int max_splits = cdiv(p.ntiles, {C.MIN_TILES_PER_SPLIT});",
            f"if (max_splits > {C.MAX_SPLITS}) max_splits = {C.MAX_SPLITS};",
            "const double cost = rounds * ((double)cdiv(p.ntiles, sp) + (T == 9 ? 1.0 : (WM * WN >= 4 ? 2.0 : 1.0)));", "g_s2k_variant = 1;"] + search + span,
        "wgrad.hip": [
            "if (p.T != 4 || p.H != 2 * p.HO || p.W != 2 * p.WO || p.proq != S2K_PRO_NONE || p.gateq) {", 'set_error("wgrad: gather geometry")',
            f"if (p.M <= {C.THIN_SIDE} || p.C <= {C.THIN_SIDE}) return " + site(C.G_GATHER_THIN), "return " + site(C.G_GATHER),
            "if (p.T == 1 && p.S == 1) {", 'if (p.H != p.HO || p.W != p.WO) { set_error("wgrad: 1x1 geometry"); return S2K_EINVAL; }',
            f"if (p.M <= {C.THIN_SIDE} && p.C <= {C.THIN_SIDE}) {{", f"if (thin_np == 256 && npix >= {C.THIN_NP_PIXELS}) {{",
            "return " + site(C.G_PIX_THIN256), "return " + site(C.G_PIX_THIN), edge,
            "if (em == 128 && ec == 128) return " + site(C.G_PIX[(128, 128)]), "if (em == 128) return " + site(C.G_PIX[(128, 64)]),
            "if (ec == 128) return " + site(C.G_PIX[(64, 128)]), "return " + site(C.G_PIX[(64, 64)]),
            'if (p.T != 9) { set_error("wgrad: only 1x1, 3x3 and 2x2-transpose kernels are on this path"); return S2K_EINVAL; }',
            "const bool thin = " + thin, "const int NPX = (thin || wide) ? 128 : 64;", "int XW = p.WO <= NPX ? p.WO : NPX;", "int R = NPX / ((XW + 1) & ~1);",
            "if (R > p.HO) R = p.HO;", "for (;; --R) {", "p.IR = (R - 1) * p.S + p.KH;", "p.IC = (p.XWe - 1) * p.S + p.KW;",
            "if (p.IR * p.WS <= NTHREADS * WG_EPT_MAX) break;", "if (XW > 16) { XW /= 2; R = 2; continue; }", 'set_error("wgrad: halo tile does not fit")',
            f"if (thin && p.M <= {C.THIN_SIDE} && p.C <= {C.THIN_SIDE}) return " + site(C.G_SP_THIN_MC), f"if (thin && p.M <= {C.THIN_SIDE}) return " + site(C.G_SP_THIN_M),
            "if (thin) return " + site(C.G_SP_THIN_C), "if (wide) return " + site(C.G_SP_WIDE),
            "if (p.IR * p.WS <= NTHREADS && p.WS == 66 && p.KW == 3) return " + site(C.G_SP_WSC), "if (p.IR * p.WS <= NTHREADS) return " + site(C.G_SP_EPT1),
            "return " + site(C.G_SP_EPT2),
            "const int slots = (T == 9 || WM * WN >= 4) ? 256 : (WM * WN >= 2 ? 512 : 768);", f"int max_splits = cdiv(p.ntiles, {C.MIN_TILES_PER_SPLIT});",
            f"if (max_splits > {C.MAX_SPLITS}) max_splits = {C.MAX_SPLITS};",
            "const double cost = rounds * ((double)cdiv(p.ntiles, sp) + (T == 9 ? 1.5 : (WM * WN >= 4 ? 2.0 : 0.7))) * (T == 9 ? 1.0 : 1.0 + 0.15 / rounds);",
            'if (p.gatep || (p.gateq && MODE != WG_PIX)) { set_error("wgrad: SE gate is only supported on the Q operand of 1x1 convs"); return S2K_EINVAL; }',
            'set_error("wgrad: prologue combination (P %d, Q %d) is not instantiated for this mode", pp, pq);', "if (lds > 160 * 1024)",
            "for (int s = wk; s < ((p.exp & 4) ? 0 : npairs); s += 2 * WVK) {", "if (s + WVK >= npairs) break;", "while (xp_run >= half_xw) { xp_run -= half_xw; ++r_run; }",
            "const int rc = launch_wgrad_q4(p, mode, st);", "const int rc = launch_wgrad_pc(p, mode, st);"] + search + span,
    }


@pytest.mark.parametrize("name", ["wgrad.h", "wgrad_q4.hip", "wgrad_pc.hip", "wgrad.hip"])
def test_every_threshold_of_the_restatement_stands_in_the_source(name):
    src = re.sub(r"[ \t]+", " ", _src(name))
    missing = [t for t in _thresholds()[name] if re.sub(r"[ \t]+", " ", t) not in src]
    assert not missing, f"{name} no longer says (tests/wgrad_dispatch.py restates it):\n  " + "\n  ".join(missing)


def test_the_chain_runs_q4_then_pc_then_the_generic_launcher():
    main = _src("wgrad.hip")
    main = main[main.index("int launch_wgrad(const S2kOp& op, const Ctx& c)"):]
    assert main.index("launch_wgrad_q4(p, mode, st)") < main.index("launch_wgrad_pc(p, mode, st)") < main.index("if (mode == S2K_MODE_GATHER2X2) {")


def test_flagged_records_are_not_this_restatements():
    for kw in (dict(flags=WD.FLAG_BF16), dict(flags=WD.FLAG_SPLIT), dict(P_BF16=1)):
        with pytest.raises(NotImplementedError):
            WD.dispatch(B=2, M=64, C=64, H=16, W=16, **kw)


def test_the_span_check_refuses_what_the_older_rows_show_to_be_the_limit():
    """one image of a 3x3 record (or the images one 1x1 pixel tile touches) at 2 GiB: refused by whichever launcher takes the shape"""
    big = dict(B=2, M=40, C=2 ** 17, H=64, W=64)                  # C * H * W * 4 = 2 GiB in one image
    for kw in (dict(), dict(P_ALIGNED16=False), dict(PROQ=GE), dict(KH=3, KW=3, PAD_T=1, PAD_L=1), dict(KH=3, KW=3, PAD_T=1, PAD_L=1, PROQ=SI)):
        v = WD.dispatch(**big, **kw)
        if kw.get("PROQ") == SI:
            assert v.result == "error" and "prologue combination" in v.message
        else:
            assert v.result == "error" and "exceed 2 GiB" in v.message, (kw, v.inst)
    ok = WD.dispatch(B=2, M=40, C=2 ** 17 - 1, H=64, W=64)
    assert ok.result == Q4 and ok.span == 1
    two = WD.dispatch(B=2, M=40, C=2 ** 16 + 64, H=63, W=65)     # H * W % 64 != 0: a tile may touch two images
    assert two.result == "error" and WD.dispatch(B=2, M=40, C=2 ** 16 - 1024, H=63, W=65).span == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------------
RUN = [n for n in T.TABLES if n != "REFUSED"]
FAMILY = {"GENERIC_PIX": (GENERIC, WG_PIX), "GENERIC_SPATIAL": (GENERIC, WG_SPATIAL), "GENERIC_GATHER": (GENERIC, WG_GATHER), "PC_SPATIAL": (PC, WG_SPATIAL),
          "PC_PIX": (PC, WG_PIX), "QUAD": (Q4, WG_PIX)}


def _rows(tables=RUN):
    return [r for n in tables for r in T.TABLES[n]]


def test_every_row_is_in_exactly_one_gpu_test():
    import inspect

    ids = [T.rid(r) for r in _rows(list(T.TABLES))]
    dup = {i for i in ids if ids.count(i) > 1}
    assert not dup, f"rows with the same id: {sorted(dup)}"
    used = []
    for name, fn in inspect.getmembers(T, inspect.isfunction):
        for mark in getattr(fn, "pytestmark", []):
            if mark.name == "parametrize":
                used += [T.rid(r) for r in mark.args[1]]
    assert sorted(used) == sorted(ids)


@pytest.mark.parametrize("r", _rows(), ids=T.rid)
def test_table_family_matches_dispatch(r):
    v = T.launch(r)
    assert v.family == r["fam"], f"family column {r['fam']}, the launcher takes {v.inst} (family {v.family} {v.message}) after {v.declined}"


def test_each_table_holds_its_own_kernel_and_mode():
    for name, (fam, mode) in FAMILY.items():
        assert {(T.launch(r).family, T.launch(r).mode) for r in T.TABLES[name]} == {(fam, mode)}, name


def test_tables_reach_every_reachable_instantiation():
    want = reachable()
    got = {T.launch(r).inst for r in _rows()}
    for k in KERNELS:
        print(f"{k}: {sum(1 for i in launched() if i[0] == k)} launched, {sum(1 for i in want if i[0] == k)} reachable, "
              f"{sum(1 for i in got & want if i[0] == k)} reached")
    missing = sorted(want - got, key=str)
    assert not missing, f"{len(missing)} instantiations no GPU row reaches:\n  " + "\n  ".join(map(str, missing))
    assert got <= want, f"rows reach instantiations the launch sites do not have: {sorted(got - want, key=str)}"


def test_refused_rows_are_refused_by_the_restatement_with_the_message_in_the_source():
    srcs = "".join(_src(n) for n in ("wgrad.hip", "wgrad_pc.hip", "wgrad_q4.hip"))
    seen = set()
    for r in T.TABLES["REFUSED"]:
        v = T.launch(r)
        assert v.result == "error" and r["raises"] in v.message, (T.rid(r), v.result, v.message)
        frag = re.sub(r"\(P \d, Q \d\)", "(P %d, Q %d)", r["raises"])
        assert frag in srcs, frag
        seen.add(frag)
    # every refusal of the generic launcher that a record below 2 GiB can meet (LDS, "halo exceeds EPT" and "tile exceeds pixel slots"
    # are ruled out by the launcher's own geometry: tests/wgrad_dispatch._launch_wg asserts it)
    assert seen == {"prologue combination (P %d, Q %d) is not instantiated for this mode", "SE gate is only supported on the Q operand of 1x1 convs",
                    "gather geometry", "1x1 geometry", "only 1x1, 3x3 and 2x2-transpose kernels are on this path", "halo tile does not fit"}


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's own error: on every row's data the f32 oracle must agree with the float64 oracle to a quarter of each bar
# ---------------------------------------------------------------------------------------------------------------------------------
def _rel(a, b, dim):
    return ((a - b).abs().amax(dim) / b.abs().amax(dim).clamp_min(1e-20)).max().item()


@pytest.mark.parametrize("r", _rows(), ids=T.rid)
def test_f32_oracle_is_within_a_quarter_of_each_bar_of_the_float64_oracle(r):
    from s2lc_amd.plan.program import Program

    worst = {}
    for scale in ("column", "row") if r["by_row"] else ("column",):
        c, fields = T.build(r, scale)
        prog = Program()
        prog.add("WGRAD", **fields)
        cpu, wide = c.oracles(prog.pack(), ref64=True)
        w32, w64 = c.read(cpu, "wgs").double(), c.read(wide, "wgs", wide=True)
        assert torch.isfinite(w64).all()
        old = c.items["wgs"][1].double()
        assert (w64 - old).abs().max() > 0 and (old != 0).all(), "WGS must be non-zero before the stage and change under it"
        worst[f"{scale}: whole"] = (w32 - w64).abs().max().item() / w64.abs().max().item()
        if scale == "column":
            worst["per column"] = _rel(w32.reshape(-1, w32.shape[-1]), w64.reshape(-1, w32.shape[-1]), 0)
        else:
            worst["per row"] = _rel(w32.transpose(0, 1).reshape(r["M"], -1), w64.transpose(0, 1).reshape(r["M"], -1), 1)
    bar = T.tol_of(r) / 4
    bad = {k: v for k, v in worst.items() if not v < bar}
    assert not bad, f"the f32 oracle alone is off by {bad} (a quarter of the bar: {bar:.1e})"


# ---------------------------------------------------------------------------------------------------------------------------------
# edges: every one below needs a row in the table of each kernel that can meet it (Wv.edges + test_wgrad_kernels_gpu.row_edges)
# ---------------------------------------------------------------------------------------------------------------------------------
_TILES = ["ragged last m-tile", "ragged last c-tile", "M one past a tile", "C one past a tile", "per output row"]
_SPLITS = ["one split", "equal splits", "short last split"]
_PIXT = ["ragged last pixel tile", "pixel tile in 1 image", "pixel tile straddles 2 images", "pixel tile straddles >= 3 images"]
_SP = ["partial last tile row", "partial last tile column", "odd XW", "several x tiles per row", "ReLU on Q under zero padding", "CTOT > C with a column offset"]
REQUIRED = {
    "GENERIC_PIX": _TILES + _SPLITS + _PIXT + ["npairs: multiple of 2 WVK", "SE gate", "SE gate over a tile that straddles 2 images",
                                                "SE gate over a tile that straddles >= 3 images", "SiLU beyond the exp range", "CTOT > C with a column offset"]
    + [f"P prologue {p}" for p in (NO, RE, SI, GE)] + [f"Q prologue {p}" for p in (NO, RE, SI, GE)],
    "GENERIC_SPATIAL": _TILES + _SPLITS + _SP + ["R capped by HO", "R cut by the halo capacity", "XW halved by the halo capacity", "stride 2",
                                                  "npairs: multiple of 2 WVK", "npairs: multiple of WVK only", "npairs: no multiple of WVK"],
    "GENERIC_GATHER": _TILES + _SPLITS + _PIXT + ["npairs: multiple of 2 WVK"] + [f"P prologue {p}" for p in (NO, RE, SI, GE)],
    "PC_SPATIAL": _TILES + _SPLITS + _SP,
    "PC_PIX": _TILES + _SPLITS + _PIXT + ["P 4-byte aligned only", "CTOT > C with a column offset"],
    "QUAD": _TILES + _SPLITS + _PIXT + ["SE gate", "SE gate over a tile that straddles 2 images", "SE gate over a tile that straddles >= 3 images",
                                        "SiLU beyond the exp range", "CTOT > C with a column offset"],
}
# What no legal record can meet, and why it is not listed:
#  * npairs of the 1x1 and gather kernels is NPJ / 2 = 32, 128 or 16, a multiple of 2 WVK whatever the record; the producer / consumer
#    kernels unroll their pairs at compile time (static_assert NPAIRS % WVK == 0) and have no such loop.
#  * "R capped by HO" on wgrad_pc: a cap changes (R, XWE) into a pair without a PC_SPATIAL_CASE (each of the seven has R = 64 / XWE), and
#    the thin form fixes R = 2 with HO >= 2; the generic rows have the edge.
#  * "R cut" / "XW halved" need stride 2 (a stride-1 halo of a <= 128-pixel tile holds at most 390 elements of the 512): generic only.
#  * a gate on the gather and 3x3 kernels, a Q prologue on the gather kernel: refused (REFUSED rows).


@pytest.mark.parametrize("table,edge", [(t, e) for t, es in REQUIRED.items() for e in es])
def test_required_edge_has_a_row_in_the_kernels_table(table, edge):
    assert any(edge in T.row_edges(r) for r in T.TABLES[table]), f"no {table} row meets: {edge}"


def _some(table, pred):
    return any(pred(r, T.launch(r), T.row_edges(r)) for r in T.TABLES[table])


def test_combined_edges():
    """edges that only count together; every missing combination is reported"""
    want = []

    def need(what, table, pred):
        want.append((f"{table}: {what}", _some(table, pred)))
    # a ragged last m-tile (checked per output row) and a ragged last c-tile for each (BM, BC) of each kernel
    tiles = {"GENERIC_PIX": [(32, 32), (64, 64), (64, 128), (128, 64), (128, 128)], "GENERIC_SPATIAL": [(32, 32), (32, 64), (64, 32), (64, 64)],
             "GENERIC_GATHER": [(64, 32), (64, 128)], "PC_SPATIAL": [(32, 32), (64, 32), (64, 64)], "PC_PIX": [(64, 64), (64, 128), (128, 64), (128, 128)],
             "QUAD": [(64, 64), (64, 128), (128, 64), (128, 128)]}
    for table, sizes in tiles.items():
        assert {(T.launch(r).BM, T.launch(r).BC) for r in T.TABLES[table]} == set(sizes), table
        for bm, bc in sizes:
            need(f"ragged last m-tile, {bm} x {bc}", table, lambda r, v, e, bm=bm, bc=bc: (v.BM, v.BC) == (bm, bc) and v.ragged_m)
            need(f"ragged last c-tile, {bm} x {bc}", table, lambda r, v, e, bm=bm, bc=bc: (v.BM, v.BC) == (bm, bc) and v.ragged_c)
        for bm in {s[0] for s in sizes}:
            need(f"ragged last m-tile per output row, BM {bm}", table, lambda r, v, e, bm=bm: v.BM == bm and v.ragged_m and r["by_row"])
        for r in T.TABLES[table]:
            if "M one past a tile" in T.row_edges(r):
                want.append((f"{table}: {T.rid(r)} has M one past a tile and is checked per output row", r["by_row"]))
    # the NP-256 and NP-64 thin forms apart
    for npj in (64, 256):
        need(f"ragged last m-tile per output row, NPJ {npj}", "GENERIC_PIX", lambda r, v, e, npj=npj: v.NPJ == npj and v.BM == 32 and r["by_row"])
    # each Q prologue with and without the SE gate on the generic 1x1 kernel; the gate over tiles that straddle 2 and >= 3 images
    for pro, gate in itertools.product((NO, RE, SI, GE), (False, True)):
        need(f"Q prologue {pro}, gate {gate}", "GENERIC_PIX", lambda r, v, e, pro=pro, gate=gate: r["proq"] == pro and r["gate"] == gate)
    # ReLU on Q under zero padding for each 3x3 geometry class
    for cfg in (WD.G_SP_THIN_MC, WD.G_SP_THIN_M, WD.G_SP_THIN_C):
        need(f"ReLU under zero padding, thin {cfg[4:7]}", "GENERIC_SPATIAL", lambda r, v, e, cfg=cfg: v.args[:9] == cfg and r["proq"] == RE)
    need("ReLU under zero padding, not thin", "GENERIC_SPATIAL", lambda r, v, e: v.NPJ == 64 and r["proq"] == RE)
    for wvm in (1, 2):
        need(f"ReLU under zero padding, thin WVM {wvm}", "PC_SPATIAL", lambda r, v, e, wvm=wvm: v.NPJ == 128 and v.args[4] == wvm and r["proq"] == RE)
    need("ReLU under zero padding, not thin", "PC_SPATIAL", lambda r, v, e: v.NPJ == 64 and r["proq"] == RE)
    # stride 2 with TF-SAME pads on an odd and an even width
    for odd in (0, 1):
        need(f"stride 2, W % 2 == {odd}", "GENERIC_SPATIAL", lambda r, v, e, odd=odd: r["s"] == 2 and r["W"] % 2 == odd)
    # a GATHER tile that straddles two images, for both geometries
    for cfg in (WD.G_GATHER_THIN, WD.G_GATHER):
        need(f"tile over 2 images, {cfg[2:7]}", "GENERIC_GATHER", lambda r, v, e, cfg=cfg: v.args[:9] == cfg and v.images_per_tile == 2)
    # npairs in each of the three classes for every WVK > 1 instantiation of the 3x3 kernel (M, C <= 32: WVK 4; one thin side: WVK 2)
    for cfg, cls in itertools.product((WD.G_SP_THIN_MC, WD.G_SP_THIN_M, WD.G_SP_THIN_C), ("multiple of 2 WVK", "multiple of WVK only", "no multiple of WVK")):
        need(f"npairs {cls}, {cfg[4:7]}", "GENERIC_SPATIAL", lambda r, v, e, cfg=cfg, cls=cls: v.args[:9] == cfg and v.pairs_class == cls)
    # ... and an odd npairs on the WVK 1 forms (the break of the pair loop's first half)
    need("npairs odd, WVK 1", "GENERIC_SPATIAL", lambda r, v, e: v.WVK == 1 and v.npairs % 2 == 1)
    # SiLU beyond the range of exp on the generic 1x1 kernel: thin (both tile sizes) and not, with and without the gate
    for what, pred in (("NPJ 256", lambda r, v: v.NPJ == 256), ("thin NPJ 64", lambda r, v: v.NPJ == 64 and v.WVK == 4), ("64-row tiles", lambda r, v: v.WVK == 1),
                       ("with the gate", lambda r, v: r["gate"]), ("without the gate", lambda r, v: not r["gate"])):
        need(f"SiLU beyond the exp range, {what}", "GENERIC_PIX", lambda r, v, e, pred=pred: r["silu_big"] and pred(r, v))
    # a column slice on 1x1 and 3x3, every kernel
    for table in ("GENERIC_PIX", "GENERIC_SPATIAL", "PC_SPATIAL", "PC_PIX", "QUAD"):
        need("CTOT > C with a column offset and a ragged c-tile", table, lambda r, v, e: "CTOT > C with a column offset" in e and v.ragged_c)
    # the halo loop: R cut with and without XW halved; the 3x3 kernels' EPT 1 form under stride 2
    need("R cut, XW kept", "GENERIC_SPATIAL", lambda r, v, e: v.r_shrunk and not v.xw_halved)
    need("EPT 1 under stride 2", "GENERIC_SPATIAL", lambda r, v, e: v.args[:9] == WD.G_SP_EPT1 and r["s"] == 2)
    missing = [w for w, ok in want if not ok]
    assert not missing, missing


# ---------------------------------------------------------------------------------------------------------------------------------
# production plans
# ---------------------------------------------------------------------------------------------------------------------------------
PLANS = ["unet", "unet_b0", "mae", "seg_frozen", "seg_unfrozen"]


@functools.lru_cache(maxsize=None)
def _plan_wgrad_records(which):
    import s2lc_amd  # noqa: F401
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet
    from s2lc_amd.modules.prithvi import MaskedAutoencoderViT
    from s2lc_amd.modules.prithvi_segmentation import PrithviSegmentationNet, PrithviSegmentationNetConfig
    from s2lc_amd.utils import _prithvi_model_args, load_untrained_prithvi

    if which == "unet":         # the b5 U-Net at 13 x 256 x 256, batch 32
        plan = EfficientnetUnet(EfficientNetConfig("b5", 13, 4, class_distribution=[0.25] * 4))._make_plan(32, 256, 256, True)
    elif which == "unet_b0":    # the b0 U-Net at 224 x 224, batch 8
        plan = EfficientnetUnet(EfficientNetConfig("b0", 13, 4, class_distribution=[0.25] * 4))._make_plan(8, 224, 224, True)
    elif which == "mae":        # Prithvi-100M MAE pre-training, batch 64, mask 0.75
        plan = load_untrained_prithvi(1)._make_plan(64, True, 0.75, True)
    else:                       # Prithvi segmentation fine-tuning, batch 16, frozen / unfrozen backbone
        bb = MaskedAutoencoderViT(**_prithvi_model_args(1), _decoder=False, _flat=False)
        plan = PrithviSegmentationNet(PrithviSegmentationNetConfig(1, 4, 256, 1, 0.1, which == "seg_frozen"), backbone=bb)._make_plan(16, True, 0.0, True)
    return tuple(f for prog in (plan.fwd, plan.bwd) for kind, f in prog.ops if kind == "WGRAD")


def _as_row(f):
    """a plan's WGRAD record as a table row (the tables' conventions are asserted: 3x3 stride 1 pads 1, stride 2 pads TF-SAME, ...).
    A record's column offset is not in its fields: a slice (CTOT > C) stands as the last one of its tensor."""
    assert not f.get("_flags", 0) & (WD.FLAG_BF16 | WD.FLAG_SPLIT) and not f.get("P_BF16", 0) and f.get("GATEP") is None
    assert f["P"].off % 16 == 0 and f["Q"].off % 16 == 0 and f["KH"] == f["KW"]
    gather = f["MODE"] == WD.MODE_GATHER2X2
    r = T.R(f["B"], f["M"], f["C"], f["HO"] if gather else f["H"], f["WO"] if gather else f["W"], None, k=1 if gather else f["KH"], s=1 if gather else f["STRIDE"],
            prop=f["PROP"], proq=f["PROQ"], gate=f.get("GATEQ") is not None, ct=f["CTOT"], coff=f["CTOT"] - f["C"], mode=f["MODE"], prod=True)
    rec = T.record(r)
    assert all(rec[k] == f[k] for k in ("H", "W", "KH", "KW", "STRIDE", "HO", "WO", "PAD_T", "PAD_L")), f
    return r


def _prod_key(r):
    """what a PROD row must share with the plan record it stands for: instantiation, edges and the map geometry"""
    return (T.launch(r).inst, T.row_edges(r) - {"per output row"}, r["H"], r["W"], r["k"], r["s"], r["mode"])


@pytest.mark.parametrize("which", PLANS)
def test_every_production_wgrad_record_has_a_prod_row_with_its_instantiation_and_edges(which):
    have = {_prod_key(r) for r in T.TABLES["PROD"]}
    recs = _plan_wgrad_records(which)
    assert recs
    missing = {T.rid(r): (k[0], sorted(k[1])) for r in map(_as_row, recs) for k in [_prod_key(r)] if k not in have}
    assert not missing, f"{which}: {len(missing)} WGRAD records without a PROD row of the same instantiation, edges and map size, e.g. {list(missing.items())[:3]}"


def test_prod_rows_are_all_needed():
    """a PROD row stands for at least one record of a production plan (nothing stale in the table)"""
    used = {_prod_key(_as_row(f)) for which in PLANS for f in _plan_wgrad_records(which)}
    stale = [T.rid(r) for r in T.TABLES["PROD"] if _prod_key(r) not in used]
    assert not stale, stale


def test_where_the_production_plans_run():
    """the issue's count, from the restatement: stages on the generic 1x1 kernel per plan; the MAE plan runs on wgrad_q4 alone"""
    def on(which, pred):
        return sum(1 for f in _plan_wgrad_records(which) if pred(T.launch(_as_row(f))))
    pix = lambda v: v.kernel == "wgrad_kernel" and v.mode == WG_PIX     # noqa: E731
    print({w: (on(w, pix), len(_plan_wgrad_records(w))) for w in PLANS})
    assert on("unet", pix) == 6 and on("unet_b0", pix) == 19
    assert on("mae", lambda v: v.family == Q4) == len(_plan_wgrad_records("mae")) == 83


# ---------------------------------------------------------------------------------------------------------------------------------
# the older f32 WGRAD rows of tests/test_ops_gpu.py: their family pins must be what the restated launcher takes
# ---------------------------------------------------------------------------------------------------------------------------------
def _params(fn):
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize" and not m.args[0].startswith("pro")] or [None]
    return mark.args[1]


def older_wgrad_rows():
    """{test: rows} - the f32 WGRAD cases of tests/test_ops_gpu.py as table rows, as their test functions hand them to _wgrad_case"""
    from tests import test_ops_gpu as O

    out = {}
    out["test_wgrad_1x1"] = [T.R(B, M, C, H, W, 0, proq=proq, gate=gate) for B, M, C, H, W, proq, gate in _params(O.test_wgrad_1x1)]
    out["test_wgrad_1x1_generic_tiles"] = [T.R(B, M, C, H, W, 0, prop=pp, proq=pq, gate=g) for B, M, C, H, W, pp, pq, g in _params(O.test_wgrad_1x1_generic_tiles)]
    out["test_wgrad_1x1_quad"] = [T.R(B, M, C, H, W, 4, prop=pp, proq=pq, gate=g) for B, M, C, H, W, pp, pq, g in _params(O.test_wgrad_1x1_quad)]
    out["test_wgrad_1x1_quad_silu_beyond_exp_range"] = [T.R(B, M, C, H, W, 4, proq=SI, gate=g, silu_big=True) for B, M, C, H, W, g in _params(O.test_wgrad_1x1_quad_silu_beyond_exp_range)]
    out["WGRAD_1X1_PC"] = [T.R(B, M, C, H, W, want, prop=pp, proq=pq, gate=g, poff=off) for B, M, C, H, W, pp, pq, g, off, want in O.WGRAD_1X1_PC]
    out["test_wgrad_1x1_per_column"] = [T.R(B, M, C, H, W, want, prop=pp, proq=pq, gate=g) for B, M, C, H, W, pp, pq, g, want in _params(O.test_wgrad_1x1_per_column)]
    out["WGRAD_3X3"] = [T.R(B, M, C, H, W, want, k=3, proq=pq, ct=CT, coff=off) for B, M, C, CT, off, H, W, pq, want in O.WGRAD_3X3]
    out["test_wgrad_3x3_producer_consumer_tiles"] = [T.R(B, M, C, H, W, 1, k=3, proq=pq, ct=CT, coff=off)
                                                     for B, M, C, CT, off, H, W, pq in _params(O.test_wgrad_3x3_producer_consumer_tiles)]
    out["test_wgrad_stem_stride2"] = [T.R(2, 48, 13, 32, 40, 0, k=3, s=2)]
    out["test_wgrad_conv_transpose"] = [T.R(B, Cin, Cout, H, W, 0, mode=T.GATHER, prop=pp) for B, Cin, Cout, H, W, pp in _params(O.test_wgrad_conv_transpose)]
    B, C, H = O._big()
    out["past 2 GiB"] = [T.R(B, 8, C, H, H, 0, k=3),                             # test_wgrad3x3_reads_past_2gib
                         T.R(15, 8, 768, 220, 222, 0),                           # test_conv1x1_and_wgrad1x1_straddling_tiles_past_2gib
                         T.R(B, 8, C, H // 2, H // 2, 0, mode=T.GATHER)]        # test_convt_wgrad_gather_reads_past_2gib
    out["past 2 GiB"] += [T.R(15, 40, 768, Hh, 222, want) for Hh, want in _params(O.test_wgrad1x1_quad_and_producer_consumer_past_2gib)]
    out["test_wgrad_1x1_with_prologue_on_p"] = [T.R(B, M, C, H, H, 0, prop=pro) for (B, M, C, H), pro in itertools.product(_params(O.test_wgrad_1x1_with_prologue_on_p), (NO, RE, SI, GE))]
    out["test_wgrad_1x1_thin_large_map"] = [T.R(2, M, C, 362, 363, 0, proq=pro) for M, C, pro in _params(O.test_wgrad_1x1_thin_large_map)]
    return out


def test_family_pins_of_the_older_wgrad_rows_match_dispatch():
    from tests import test_ops_gpu as O

    assert [m.args[1] for m in O.test_wgrad_1x1_with_prologue_on_p.pytestmark if m.args[0] == "pro"] == [[NO, RE, SI, GE]]
    tests = older_wgrad_rows()
    rows = [r for rs in tests.values() for r in rs]
    assert len(rows) >= 100
    wrong = [(T.rid(r), r["fam"], T.launch(r).inst) for r in rows if T.launch(r).family != r["fam"]]
    assert not wrong, wrong
    old, new = {T.launch(r).inst for r in rows}, {T.launch(r).inst for r in _rows()}
    print(f"older WGRAD rows: {len(rows)} rows reach {len(old & reachable())} of {len(reachable())} instantiations; the new tables reach {len(new & reachable())}")
    print("without a row before:", *sorted(reachable() - old, key=str), sep="\n  ")
    assert old <= new
    # the claims of the older tests, from the parse: "all 16 instantiations" of wgrad_q4_kernel, "all 12" of wgrad_pc_kernel's pixel mode
    assert {T.launch(r).inst for r in tests["test_wgrad_1x1_quad"]} == set(q4_launches()[0]) and len(q4_launches()[0]) == 16
    pc_pix = {k for k in pc_launches()[0] if k[1][0] == WG_PIX}
    assert {T.launch(r).inst for r in tests["WGRAD_1X1_PC"] if r["fam"] == PC} == pc_pix and len(pc_pix) == 12
    # ... and "one case per compiled tile geometry" of its 3x3 mode: the seven (R, XWE) and the two thin forms
    geoms = {T.launch(r).args[:10] for r in tests["test_wgrad_3x3_producer_consumer_tiles"]}
    assert geoms == {k[1][:10] for k in pc_launches()[0] if k[1][0] == WG_SPATIAL} and len(geoms) == 9
