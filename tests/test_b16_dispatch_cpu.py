"""Coverage of the bf16 / f32-split GPU tables (tests/test_b16_kernels_gpu.py), checked without a GPU.

Every launch site and macro body (B16_3X3, WB16_3X3) of csrc/conv_bf16.hip and csrc/wgrad_bf16.hip is parsed into the set of template
instantiations the launchers can produce; every threshold and default tests/b16_dispatch.py restates is looked up in the source text.
The tables must reach every reachable instantiation and nothing else, and every required edge per table; the table a row stands
in (and the bf16 / split rows of tests/test_ops_gpu.py and tests/test_f32_split_ops_gpu.py) must name the family the restated launcher
takes; on every row's data the f32 oracle must stay within a quarter of each bar of the float64 reference; and on the lattice data of
the exact rows bf16 rounding must be the identity on every activated operand and weight.

Parsed: conv_bf16_kernel 76 (bf16-mixed) + 58 (f32-split; 56 reachable), wgrad_bf16_kernel 28 + 12; 431 rows, of them 189 PROD rows for
the 799 flagged CONV / WGRAD records of the eight production plans.  849 cases in 55 s; the slowest row on 16 CPUs (its two oracle runs,
test_f32_oracle_is_within_a_quarter_of_each_bar_of_the_float64_reference): the 3x3 weight gradient at 224 x 224 of the segmentation
head (5.5 G multiply-adds), 1.5 s; the slowest row of the five kernel tables 0.2 s."""
import functools
import inspect
import re
import time
from pathlib import Path

import pytest
import torch

from tests import b16_dispatch as BD
from tests import test_b16_kernels_gpu as T

CSRC = Path(__file__).resolve().parents[1] / "sentinel2-landcover-classification_amd" / "csrc"
PRO = {"S2K_PRO_NONE": 0, "S2K_PRO_AFFINE": 1, "S2K_PRO_SILU": 2, "S2K_PRO_RELU": 3, "S2K_PRO_GELU": 4}
FAMILY = {"CONV_BF16": 2, "CONV_SPLIT": 5, "WGRAD_BF16": 2, "WGRAD_SPLIT": 5}
DEEP_THIN = "deep chunks need M > 32, the thin tile M <= 32"


def _src(name):
    return (CSRC / name).read_text()


def _between(src, a, b):
    return src[src.index(a):src.index(b)]


def _ev(tok, split, env=()):
    tok = tok.strip()
    table = {"K1": BD.K1[split], "KDEEP": BD.KDEEP[split], "SPLIT": split, "!SPLIT": not split, "true": True, "false": False, "BM_PIX": BD.BM_PIX,
             "BM_SPATIAL": BD.BM_SPATIAL, "WG_PIX": BD.WG_PIX, "WG_SPATIAL": BD.WG_SPATIAL, **PRO, **dict(env)}
    return table[tok] if tok in table else int(tok)


def _sites(text, name):
    """(template argument tokens, only without SPLIT, text of the line before the site) of every `name<...>(` in text"""
    out = []
    for m in re.finditer(r"\b" + name + r"<([^<>]*)>\(", text):
        line = text[text.rfind("\n", 0, m.start()) + 1:m.start()]
        out.append(([t.strip() for t in m.group(1).split(",")], "!SPLIT" in line, line))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the instantiations each file can launch: {(kernel, template arguments): reason it cannot be reached, or None}
# ---------------------------------------------------------------------------------------------------------------------------------
def conv_launches(split):
    src = _src("conv_bf16.hip")
    bm_body = _between(src, "static int launch_b16_bm(", "static int launch_b16_pix(")
    pix_body = _between(src, "static int launch_b16_pix(", "static int conv_b16_route(")
    route = _between(src, "static int conv_b16_route(", "int launch_conv_bf16(")
    bm_forms = [tuple(int(v) for v in m) for m in re.findall(r"launch_b16<BMODE, (\d), (\d), (\d), KCH, R, XW, PRO, GATE, SCATTER, X16, SPLIT>", bm_body)]
    assert bm_forms == [(2, 2, 2), (2, 1, 2)], bm_forms
    assert "if (big) return launch_b16<BMODE, 2, 2, 2," in bm_body
    pix_forms = [tuple(int(v) for v in m) for m in re.findall(r"launch_b16<BM_PIX, (\d), (\d), (\d), KCH, 1, 64, PRO, GATE, false, X16, SPLIT>", pix_body)]
    assert pix_forms == [(1, 1, 2), (2, 1, 1)], pix_forms
    assert "if constexpr (KCH <= 64) {\n        if (p.M <= 32) return launch_b16<BM_PIX, 1, 1, 2," in pix_body
    assert len(re.findall(r"launch_b16_bm<BM_PIX, KCH, 1, 64, PRO, GATE, false, X16, SPLIT>", pix_body)) == 1
    out, counts = {}, {}

    def add(args, why=None):
        key = ("conv_bf16_kernel", args)
        out[key] = why if key not in out else (out[key] and why)

    def via_bm(bmode, kch, r, xw, pro, gate, scatter, x16, sp):
        for f in bm_forms:
            add((bmode,) + f + (kch, r, xw, pro, gate, scatter, x16, sp))
    macro = re.search(r"#define B16_3X3\(RR, XX\)((?:[^\n]*\\\n)*[^\n]*)", route)
    assert macro, "macro B16_3X3 not found"
    body = route.replace(macro.group(0), "")
    pix = _sites(body, "launch_b16_pix")
    counts["launch_b16_pix"] = len(pix)
    for toks, only_plain, _ in pix:
        if only_plain and split:
            continue
        toks = toks + ["false"] * (5 - len(toks))
        kch, pro, gate, x16, sp = (_ev(t, split) for t in toks)
        deep = toks[0] in ("KDEEP", "128")
        if kch <= 64:
            add((BD.BM_PIX,) + pix_forms[0] + (kch, 1, 64, pro, gate, False, x16, sp), DEEP_THIN if deep else None)
        add((BD.BM_PIX,) + pix_forms[1] + (kch, 1, 64, pro, gate, False, x16, sp))
        via_bm(BD.BM_PIX, kch, 1, 64, pro, gate, False, x16, sp)
    bm = _sites(body, "launch_b16_bm")
    counts["launch_b16_bm"] = len(bm)
    for toks, only_plain, _ in bm:
        assert not only_plain
        toks = toks + ["false"] * (9 - len(toks))
        via_bm(*(_ev(t, split) for t in toks))
    thin = _sites(body, "launch_b16")
    counts["launch_b16"] = len(thin)
    for toks, only_plain, _ in thin:
        if only_plain and split:
            continue
        toks = toks + ["false"] * (12 - len(toks))
        add(tuple(_ev(t, split) for t in toks))
    mbody = macro.group(1).replace("\\\n", "\n")
    msites = _sites(mbody, "launch_b16_bm")
    counts["B16_3X3 body"] = len(msites)
    geoms = []
    for cond, r, xw in re.findall(r"if \(([^\n]*?)\) B16_3X3\((\d+), (\d+)\)", body):
        widths = "mult64" if cond == "p.WO >= 64 && p.WO % 64 == 0" else tuple(int(w) for w in re.findall(r"p\.WO == (\d+)", cond))
        assert widths == "mult64" or " || ".join(f"p.WO == {w}" for w in widths) == cond, cond
        geoms.append(((int(r), int(xw)), widths))
        for toks, only_plain, _ in msites:
            if only_plain and split:
                continue
            toks = toks + ["false"] * (9 - len(toks))
            via_bm(*(_ev(t, split, (("RR", int(r)), ("XX", int(xw)))) for t in toks))
    counts["B16_3X3 calls"] = len(geoms)
    return out, counts, tuple(geoms)


def wgrad_launches(split):
    src = _src("wgrad_bf16.hip")
    out, counts = {}, {}
    if split:
        fn = _between(src, "int launch_wgrad_split(", "}  // namespace s2k")
        sites = _sites(fn, "launch_wb16")
        counts["launch_wb16"] = len(sites)
        for toks, _, _ in sites:
            assert toks[-2:] == ["false", "true"], toks
            out[("wgrad_bf16_kernel", tuple(_ev(t, True) for t in toks))] = None
        return out, counts
    fn = _between(src, "int launch_wgrad_bf16(", "// f32-split (S2K_FLAG_SPLIT): S2K_OK = launched, < 0 = error - a split stage never falls back (plan/split.py")
    macro = re.search(r"#define WB16_3X3\(\.\.\.\) ([^\n]*)", fn)
    assert macro and macro.group(1) == "(p.p_bf16 ? launch_wb16<WG_SPATIAL, __VA_ARGS__, true>(p, st) : launch_wb16<WG_SPATIAL, __VA_ARGS__>(p, st))", "macro WB16_3X3"
    body = fn.replace(macro.group(0), "")
    sites = _sites(body, "launch_wb16")
    counts["launch_wb16"] = len(sites)
    for toks, _, _ in sites:
        toks = toks + ["false"] * (9 - len(toks))
        out[("wgrad_bf16_kernel", tuple(_ev(t, False) for t in toks))] = None
    calls = re.findall(r"WB16_3X3\(" + r",\s*".join([r"(\d+)"] * 6) + r"\)", body)
    counts["WB16_3X3 calls"] = len(calls)
    for c in calls:
        for p16 in (False, True):
            out[("wgrad_bf16_kernel", (BD.WG_SPATIAL,) + tuple(int(v) for v in c) + (p16, False))] = None
    return out, counts


def launched():
    out = {}
    for split in (False, True):
        for part in (conv_launches(split)[0], wgrad_launches(split)[0]):
            assert not set(part) & set(out)
            out.update(part)
    return out


def reachable():
    return {k for k, why in launched().items() if why is None}


def _mode(inst):
    return (inst[0], "split" if inst[1][-1] else "bf16")


def test_parse_finds_every_launch_site():
    assert conv_launches(False)[1] == conv_launches(True)[1] == {"launch_b16_pix": 9, "launch_b16_bm": 2, "launch_b16": 3, "B16_3X3 body": 3, "B16_3X3 calls": 6}
    assert wgrad_launches(False)[1] == {"launch_wb16": 14, "WB16_3X3 calls": 7} and wgrad_launches(True)[1] == {"launch_wb16": 13}
    got = launched()
    keys = [("conv_bf16_kernel", "bf16"), ("conv_bf16_kernel", "split"), ("wgrad_bf16_kernel", "bf16"), ("wgrad_bf16_kernel", "split")]
    per = {k: sum(1 for i in got if _mode(i) == k) for k in keys}
    reach = {k: sum(1 for i in reachable() if _mode(i) == k) for k in keys}
    print("launched", per, "reachable", reach)
    assert list(per.values()) == [76, 58, 28, 12], per
    assert list(reach.values()) == [76, 56, 28, 12], reach
    # what no record can reach, by name: the thin 32 x 256 tile with the f32-split mode's deep (64-channel) chunks
    assert {k: why for k, why in got.items() if why} == {
        ("conv_bf16_kernel", (BD.BM_PIX, 1, 1, 2, 64, 1, 64, pro, gate, False, False, True)): DEEP_THIN for pro, gate in ((0, False), (2, True))}
    # by form: 1x1 33 / 26 (+ 2), scatter 4 / 4, 3x3 39 / 26
    for split, want in ((False, (33, 4, 39)), (True, (28, 4, 26))):
        mine = [a for (k, a) in got if k == "conv_bf16_kernel" and a[-1] == split]
        assert (sum(1 for a in mine if a[0] == BD.BM_PIX and not a[9]), sum(1 for a in mine if a[9]), sum(1 for a in mine if a[0] == BD.BM_SPATIAL)) == want


def test_tile_tables_of_the_restatement_are_the_parsed_ones():
    for split in (False, True):
        assert conv_launches(split)[2] == BD.GEOMS_3X3
    for split, tab in ((False, BD.W_3X3_BF16), (True, BD.W_3X3_SPLIT)):
        pix = {a[1:5] + (a[6],) for (k, a) in wgrad_launches(split)[0] if a[0] == BD.WG_PIX}
        assert pix == set(BD.W_PIX.values())
        sp = {a[1:7] for (k, a) in wgrad_launches(split)[0] if a[0] == BD.WG_SPATIAL}
        assert sp == set(tab["mult64"].values()) | {v for k, v in tab.items() if k != "mult64"}


TUNE_DEFAULTS = {"conv_bf16.hip": {"S2K_B16_SPLIT_MAX_BLOCKS": BD.SPLIT_MAX_BLOCKS, "S2K_B16_DEEP_MIN": BD.DEEP_MIN}, "wgrad_bf16.hip": {"S2K_WB16_SLOTS": 0}}


@pytest.mark.parametrize("name", list(TUNE_DEFAULTS))
def test_every_tuning_default_is_the_one_the_restatement_assumes(name):
    got = {k: int(v) for k, v in re.findall(r'tune_int\("(\w+)", (-?\d+)\)', _src(name))}
    assert got == TUNE_DEFAULTS[name], f"{name}: a tuning switch changed or was added: restate it in tests/b16_dispatch.py"


def _thresholds():
    """file -> [(source fragment written from the restatement's constants, how often it stands in the file)]"""
    C = BD
    edge = f"auto edge = [](int n) {{ return n <= 32 ? 32 : ((n > 64 && (double)cdiv(n, 128) * 128 / n <= {C.BM_PAD}) ? 128 : 64); }};"
    widths = {w: f"p.WO == {w}" for _, ws in C.GEOMS_3X3 if ws != "mult64" for w in ws}
    return {
        "conv_bf16.hip": [(t, 1) for t in [
            f"constexpr int K1 = SPLIT ? {C.K1[True]} : {C.K1[False]}, KDEEP = SPLIT ? {C.KDEEP[True]} : {C.KDEEP[False]};",
            f"if (p.M <= {C.THIN_M}) return 1;\n const bool big = p.M > 64 && (double)cdiv(p.M, 128) * 128 / p.M <= {C.BM_PAD};",
            f"if (p.M <= {C.THIN_M}) return launch_b16<BM_PIX, 1, 1, 2, KCH, 1, 64,", "p, cdiv(p.Ntot, 256), st);",
            f"if ((int64_t)n128 * cdiv(p.M, 128) < {C.PIX_SMALL_TILES}) return launch_b16<BM_PIX, 2, 1, 1, KCH, 1, 64, PRO, GATE, false, X16, SPLIT>(p, cdiv(p.Ntot, 64), st);",
            f"const bool deep = p.Ctot >= deep_min && p.M > 32 && (int64_t)cdiv(p.Ntot, 128) * cdiv(p.M, 128) <= {C.DEEP_MAX_TILES};",
            f"if (PIX && !SCATTER && p.scratch && blocks <= split_max_blocks && nchunks >= {C.SPLITK_MIN_CHUNKS}) {{",
            f"int splits = (int)std::min<int64_t>({C.SPLITK_MAX}, cdiv64({C.SPLITK_TARGET}, blocks));", f"splits = std::min(splits, nchunks / {C.SPLITK_PER});",
            "p.chunks_per_split = cdiv(nchunks, splits);\n p.splits = cdiv(nchunks, p.chunks_per_split);",
            "if (lds > 160 * 1024) {", "if (need >= 0x7ffffff0ll)", "const int64_t span = (!PIX || (p.HW % BN) == 0) ? 1 : std::min<int64_t>(p.B, (BN - 2) / p.HW + 2);",
            "constexpr size_t img = (size_t)(NO * TT * BM + NO * USED) * 16 * (SPLIT ? 3 : 1);",
            "constexpr size_t ct_bytes = (!SCATTER && (PIX || XW % 4 == 0)) ? (size_t)WVM * 32 * (BN + 8) * sizeof(float) : 0;",
            "const size_t lds = std::max(img + (PRO != S2K_PRO_NONE ? (size_t)2 * nchunks * KCH * sizeof(float) : 0), ct_bytes);",
            "if constexpr (!SCATTER && (PIX || XW % 4 == 0)) {", "constexpr int G = BN / 4;", "const int kp8 = ((p.Ctot + 63) / 64) * 8;",
            "if (!p.wtb || p.S != 1 || p.HO != p.H || p.WO != p.W) return 1;", "if (p.x1_bf16 && p.mode != S2K_MODE_CONV) return 1;",
            "if (T != 1 || p.C2 != 0 || (p.HW & 3) || p.gate1 || p.M <= 32 || (p.M & 3)) return 1;", "if (p.C2 != 0 || (p.HW & 3) || p.PT || p.PL) return 1;",
            "if (p.gate1 || p.pro1 != S2K_PRO_NONE || (p.HW & 7)) {", "if (T != 9 || p.KH != 3 || p.PT != 1 || p.PL != 1 || p.gate1) return 1;",
            "if (p.pro1 != S2K_PRO_NONE && p.pro1 != S2K_PRO_RELU) return 1;", "if (p.x1_bf16 && (p.pro1 != S2K_PRO_NONE || p.C2 != 0)) return 1;",
            "if (p.C2 > 0 && (p.pro2 != p.pro1 || (p.C1 % 16) != 0)) return 1;", "if (p.WO < 64 || p.WO % 64 != 0) return 1;",
            f"const int n = tiles({C.THIN_3X3[0]}, {C.THIN_3X3[1]});", "if (p.WO >= 64 && p.WO % 64 == 0) B16_3X3(2, 64)",
            f"if ({widths[56]} || {widths[112]} || {widths[224]}) B16_3X3(2, 56)", f"if ({widths[32]}) B16_3X3(4, 32)", f"if ({widths[16]}) B16_3X3(8, 16)",
            f"if ({widths[28]}) B16_3X3(4, 28)", f"if ({widths[14]}) B16_3X3(8, 14)", f"launch_b16_bm<BM_SPATIAL, {C.K3}, RR, XX, S2K_PRO_RELU, false, false, false, SPLIT>",
            "g_s2k_variant = SPLIT ? 5 : 2;",
        ]] + [("if (p.M <= 32) {", 1)],
        "wgrad_bf16.hip": [(edge, 2), (f"(int64_t)p.B * p.HWp < {C.W_MIN_PIXELS}) return 1;", 1), (f"(int64_t)p.B * p.HWp < {C.W_MIN_PIXELS}) return no();", 1),
                           ("if ((p.HWp & 7) ||", 2), (f"const int slots = slots_exp > 0 ? slots_exp : (PIX ? {C.W_SLOTS[True]} : {C.W_SLOTS[False]});", 1),
                           ("int splits = std::max(1, slots / mc);", 1), (f"splits = std::min(splits, std::max(1, p.ntiles / {C.W_MIN_TILES_PER_SPLIT}));", 1),
                           ("if (splits > 65535) splits = 65535;", 1), ("p.tiles_per_split = cdiv(p.ntiles, splits);\n splits = cdiv(p.ntiles, p.tiles_per_split);", 1),
                           ("if (mode != S2K_MODE_CONV || p.S != 1 || p.H != p.HO || p.W != p.WO || p.gatep) return", 2),
                           ("if (p.T != 9 || p.KH != 3 || p.KW != 3 || p.PT != 1 || p.PL != 1 || p.gateq || p.prop != S2K_PRO_NONE) return", 2),
                           ("pro == S2K_PRO_NONE || pro == S2K_PRO_RELU || pro == S2K_PRO_SILU || pro == S2K_PRO_AFFINE || pro == S2K_PRO_GELU; };", 2),
                           ("if (p.WO % 64 == 0) {", 2), ("if (p.WO % 56 == 0) return WB16_3X3(2, 2, 1, 1, 2, 56);", 1), ("if (p.WO == 32) return", 2),
                           ("if (p.WO == 16) return", 2), ("if (em == 32 && ec == 32) return", 5), ("if (em == 128 && ec == 128) return", 3),
                           ("constexpr size_t lds = (size_t)(NPO * BM + QR * QXO * BC) * 16 * (SPLIT ? 3 : 1);", 1), ("if (need >= 0x7ffffff0ll) {", 1),
                           ("p.tiles_x = p.WO / XW;", 1), ("constexpr int WVK = 4 / (WVM * WVC);", 1), ("g_s2k_variant = SPLIT ? 5 : 2;", 1)],
    }


@pytest.mark.parametrize("name", ["conv_bf16.hip", "wgrad_bf16.hip"])
def test_every_threshold_of_the_restatement_stands_in_the_source(name):
    src = re.sub(r"\s+", " ", _src(name))
    wrong = [(t, n, src.count(re.sub(r"\s+", " ", t))) for t, n in _thresholds()[name] if src.count(re.sub(r"\s+", " ", t)) != n]
    assert not wrong, f"{name} no longer says (tests/b16_dispatch.py restates it; fragment, expected count, found):\n  " + "\n  ".join(map(str, wrong))


# ---------------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows(tables=None):
    return [r for name, tab in T.TABLES.items() if tables is None or name in tables for r in tab]


def test_every_row_is_in_exactly_one_gpu_test():
    ids = [T.rid(r) for r in _rows()]
    dup = {i for i in ids if ids.count(i) > 1}
    assert not dup, f"rows with the same id: {sorted(dup)}"
    used = []
    for name, fn in inspect.getmembers(T, inspect.isfunction):
        for mark in getattr(fn, "pytestmark", []):
            if mark.name == "parametrize":
                used += [T.rid(r) for r in mark.args[1]]
    assert sorted(used) == sorted(ids)
    print({name: len(tab) for name, tab in T.TABLES.items()}, len(ids), "rows")


@pytest.mark.parametrize("table", list(FAMILY))
def test_each_table_holds_its_own_kernel_and_family(table):
    for r in T.TABLES[table]:
        v = T.launch(r)
        assert v.result == FAMILY[table], f"{T.rid(r)}: {table} row, the launcher says {v.result} {v.message}"
        assert v.kernel == ("conv_bf16_kernel" if r["kind"] == "CONV" else "wgrad_bf16_kernel") and v.args[-1] == r["split"] == (FAMILY[table] == 5)
        assert v.lds <= BD.LDS_MAX


def test_declined_rows_are_declined_or_refused():
    for r in T.TABLES["DECLINED"]:
        v = T.launch(r)
        assert v.result in ("declined", "error"), T.rid(r)
        if r["split"] or r.get("x16") or r.get("p16"):      # a split stage never falls back; a stored-bf16 operand is never read as floats
            assert v.result == "error" and v.message, T.rid(r)
        if v.result == "declined" and r["kind"] == "CONV":
            assert T.f32_family(r) in (0, 1, 3, 4)
        if v.result == "declined" and r["kind"] == "WGRAD":     # pinned to the f32 family, or refused by the f32 launcher with the row's message
            f = T.f32_launch(r)
            assert (f.result in (0, 1, 4) and not r["raises"]) or (f.result == "error" and r["raises"] and re.search(r["raises"], f.message)), (T.rid(r), f.result, f.message)


def test_f32_has_is_the_prologue_rule_of_the_f32_ladder():
    """f32_has asks tests/wgrad_dispatch.py; on the tables' rows that is launch_wg's rule: a prologue on one side at most, never AFFINE;
    3x3: none or ReLU on Q"""
    NO, SI, RE, GE = BD.PRO_NONE, BD.PRO_SILU, BD.PRO_RELU, BD.PRO_GELU
    rows = [r for tab in T.TABLES.values() for r in tab if r["kind"] == "WGRAD" and not r["p16"] and not r["gatep"] and not r["raises"]]
    assert len(rows) >= 60
    for r in rows:
        if r["k"] == 3:
            rule = r["prop"] == NO and r["proq"] in (NO, RE)
        else:
            rule = (r["prop"] == NO and r["proq"] in (NO, RE, SI, GE)) or (r["proq"] == NO and r["prop"] in (RE, SI, GE))
        assert T.f32_has(r) == rule, T.rid(r)


def test_tables_reach_every_reachable_instantiation():
    want = reachable()
    rows = _rows(FAMILY)
    got = {T.launch(r).inst for r in rows}
    missing = sorted(want - got, key=str)
    for key in sorted({_mode(i) for i in want}):
        print(key, f"{sum(1 for i in want if _mode(i) == key)} reachable, {sum(1 for i in got & want if _mode(i) == key)} reached")
    print(f"{len(want)} reachable instantiations, {len(got & want)} reached by {len(rows)} rows")
    assert not missing, f"{len(missing)} instantiations no GPU row reaches:\n  " + "\n  ".join(map(str, missing))
    assert got <= want, f"rows reach instantiations the launch sites do not produce: {sorted(got - want, key=str)}"


# ---------------------------------------------------------------------------------------------------------------------------------
# edges: every one below needs a row in each table named (Cv.edges / Wv.edges + test_b16_kernels_gpu.row_edges)
# ---------------------------------------------------------------------------------------------------------------------------------
_CONV = ["ragged last m-tile", "M one past a tile", "ragged last pixel tile", "pixel tile over 2 images", "pixel tile over >= 3 images", "K tail",
         "K < one chunk", "Ctot % 8 != 0", "K tail in source 2", "split-K", "no split-K", "split-K: unequal splits", "split-K: 8 splits",
         "split-K: nchunks / 4 cap", "would split, has no SCRATCH", "reduce tail: bias", "reduce tail: statistics", "reduce tail: beta", "reduce tail: residual",
         "transposed store", "scalar store", "scatter store", "statistics: reduction width 16", "statistics: reduction width 32", "statistics: reduction width 64",
         "statistics: several replicas", "statistics: one replica", "partial last tile row", "several x tiles per row", "prologue 0", "prologue 1", "prologue 2",
         "prologue 3", "SE gate", "bias", "beta", "residual", "YC > M", "concat"]
_WGRAD = ["ragged last m-tile", "ragged last c-tile", "C < 8", "ragged last pixel tile", "pixel tile over 2 images", "pixel tile over >= 3 images", "one split",
          "several splits", "shorter last split", "partial last tile row", "two x tiles per row", "k-waves combined", "gate on Q",
          "gate on Q over a tile that straddles images", "CTOT > C with a column offset"] + [f"{s} prologue {p}" for s in "PQ" for p in range(5)]
REQUIRED = {
    "CONV_BF16": _CONV + ["X16", "upper half of the last 128-channel chunk past the packed K", "upper half of the last 128-channel chunk inside the packed K"],
    "CONV_SPLIT": _CONV + ["spread operands"],
    "WGRAD_BF16": _WGRAD + ["P16"],
    "WGRAD_SPLIT": _WGRAD + ["spread operands"],
}


@pytest.mark.parametrize("table,edge", [(t, e) for t, es in REQUIRED.items() for e in es])
def test_required_edge_has_a_row_in_the_kernels_table(table, edge):
    assert any(edge in T.row_edges(r) for r in T.TABLES[table]), f"no {table} row meets: {edge}"


def test_combined_edges():
    """edges that only count together; every missing combination is reported"""
    want = []

    def need(what, table, pred):
        want.append((f"{table}: {what}", any(pred(r, T.launch(r), T.row_edges(r)) for r in T.TABLES[table])))
    for table, split in (("CONV_BF16", False), ("CONV_SPLIT", True)):
        pix = lambda v: v.args[0] == BD.BM_PIX       # noqa: E731
        for bm in (32, 64, 128):
            need(f"ragged last m-tile, BM {bm}", table, lambda r, v, e, bm=bm: v.BM == bm and v.ragged_m)
        need("M one past a tile, BM 64", table, lambda r, v, e: v.BM == 64 and "M one past a tile" in e)
        for bn in (64, 128, 256):
            need(f"ragged last pixel tile, BN {bn}", table, lambda r, v, e, bn=bn: v.BN == bn and v.ragged_n)
        need(">= 3 images per tile with the SE gate", table, lambda r, v, e: v.images_per_tile >= 3 and r["gate"])
        for kch in (BD.K1[split], BD.KDEEP[split], BD.K3):
            need(f"K tail, KCH {kch}", table, lambda r, v, e, kch=kch: v.KCH == kch and "K tail" in e)
            need(f"Ctot % 8 != 0, KCH {kch}", table, lambda r, v, e, kch=kch: v.KCH == kch and v.c_mod8)
        for kch in (BD.K1[split], BD.K3):
            need(f"K < one chunk, KCH {kch}", table, lambda r, v, e, kch=kch: v.KCH == kch and v.k_lt_chunk)
        for c in (576, 517):
            need(f"Ctot {c} on deep chunks", table, lambda r, v, e, c=c: r["C1"] == c and v.deep)
            if not split:
                need(f"Ctot {c} on deep chunks, X16", table, lambda r, v, e, c=c: r["C1"] == c and v.deep and r["x16"])
        need("split-K tail with bias, statistics, accumulate and residual", table,
             lambda r, v, e: {"reduce tail: bias", "reduce tail: statistics", "reduce tail: beta", "reduce tail: residual"} <= e)
        need("SCRATCH given, no split", table, lambda r, v, e: r["scratch"] and v.splits == 1)
        for pro in (0, 1, 2, 3):
            need(f"1x1 prologue {pro}, no gate", table, lambda r, v, e, pro=pro: pix(v) and r["pro"] == pro and not r["gate"])
        need("1x1 SiLU with the gate, deep chunks", table, lambda r, v, e: r["gate"] and v.deep)
        need("statistics + residual, transposed store", table, lambda r, v, e: {"statistics", "residual", "transposed store"} <= e)
        need("statistics + accumulate, transposed store", table, lambda r, v, e: {"statistics", "beta", "transposed store"} <= e)
        need("statistics + residual + accumulate, scalar store", table, lambda r, v, e: {"statistics", "residual", "beta", "scalar store"} <= e)
        for rr in (2, 4, 8):
            need(f"partial last tile row, R {rr}", table, lambda r, v, e, rr=rr: v.R == rr and "partial last tile row" in e)
        for wo in (128, 112):
            need(f"several x tiles per row at WO {wo}", table, lambda r, v, e, wo=wo: r["W"] == wo and "several x tiles per row" in e)
        for wo in (64, 128, 32, 16, 56, 112, 224, 28, 14):
            need(f"3x3 at WO {wo}", table, lambda r, v, e, wo=wo: r["k"] == 3 and r["W"] == wo)
        need("3x3 ReLU prologue (positive shifts on the border)", table, lambda r, v, e: r["k"] == 3 and r["pro"] == 3)
        need("3x3 concat with the K tail in source 2", table, lambda r, v, e: r["k"] == 3 and "K tail in source 2" in e)
        need("3x3 thin tile", table, lambda r, v, e: r["k"] == 3 and v.BM == 32)
        if not split:
            need("X16 on 3x3", table, lambda r, v, e: r["k"] == 3 and r["x16"])
            need("X16 on the thin 3x3 tile", table, lambda r, v, e: r["k"] == 3 and r["x16"] and v.BM == 32)
            need("upper half inside the packed K", table, lambda r, v, e: v.upper_half_in_k)
        if split:
            for geo in {(v.BM, v.BN, v.args[0]) for v in map(T.launch, T.TABLES[table])}:
                need(f"spread operands on geometry {geo}", table, lambda r, v, e, geo=geo: r["spread"] and (v.BM, v.BN, v.args[0]) == geo)
    for table, split in (("WGRAD_BF16", False), ("WGRAD_SPLIT", True)):
        for n in (32, 33, 64, 65, 114, 115, 129, 229):
            need(f"side length {n}", table, lambda r, v, e, n=n: n in (r["M"], r["C"]))
        need("one split", table, lambda r, v, e: v.splits == 1)
        need("3x3: partial last tile row", table, lambda r, v, e: r["k"] == 3 and v.partial_row)
        need("3x3: two x tiles per row", table, lambda r, v, e: r["k"] == 3 and v.tiles_x >= 2)
        need("3x3: ReLU on Q (borders zero after the activation)", table, lambda r, v, e: r["k"] == 3 and r["proq"] == 3)
        need("3x3: CTOT > C with a column offset", table, lambda r, v, e: r["k"] == 3 and "CTOT > C with a column offset" in e)
        need(">= 3 images per 256-pixel tile, ragged last tile", table, lambda r, v, e: v.NPJ == 256 and v.images_per_tile >= 3 and v.ragged_n)
        for geo in {v.args[:7] for v in map(T.launch, T.TABLES[table]) if v.WVK > 1}:
            need(f"k-waves combined on {geo}", table, lambda r, v, e, geo=geo: v.args[:7] == geo)
        if not split:
            for geo in {v.args[:7] for v in map(T.launch, T.TABLES[table])}:
                need(f"P16 on {geo}", table, lambda r, v, e, geo=geo: v.args[:7] == geo and r["p16"])
        if split:
            need("spread operands, 1x1 and 3x3", table, lambda r, v, e: r["spread"] and r["k"] == 3)
            need("spread operands, 1x1", table, lambda r, v, e: r["spread"] and r["k"] == 1)
    missing = [w for w, ok in want if not ok]
    assert not missing, missing


# ---------------------------------------------------------------------------------------------------------------------------------
# production plans: every CONV / WGRAD record that carries FLAG_BF16 or FLAG_SPLIT needs a PROD row with the same instantiation, edges and
# map size
# ---------------------------------------------------------------------------------------------------------------------------------
PLANS = [(which, prec) for prec in ("bf16-mixed", "f32-split") for which in ("unet", "mae", "seg_frozen", "seg_unfrozen")]


@functools.lru_cache(maxsize=None)
def _plan_records(which, precision):
    import s2lc_amd  # noqa: F401
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet
    from s2lc_amd.modules.prithvi import MaskedAutoencoderViT
    from s2lc_amd.modules.prithvi_segmentation import PrithviSegmentationNet, PrithviSegmentationNetConfig
    from s2lc_amd.utils import _prithvi_model_args, load_untrained_prithvi

    if which == "unet":         # the b5 U-Net at 13 x 256 x 256, batch 32
        m = EfficientnetUnet(EfficientNetConfig("b5", 13, 4, class_distribution=[0.25] * 4))
        m.precision = precision
        plan = m._make_plan(32, 256, 256, True)
    elif which == "mae":        # Prithvi-100M MAE pre-training, batch 64, mask 0.75
        m = load_untrained_prithvi(1)
        m.precision = precision
        plan = m._make_plan(64, True, 0.75, True)
    else:                       # Prithvi segmentation fine-tuning, batch 16, frozen / unfrozen backbone
        bb = MaskedAutoencoderViT(**_prithvi_model_args(1), _decoder=False, _flat=False)
        m = PrithviSegmentationNet(PrithviSegmentationNetConfig(1, 4, 256, 1, 0.1, which == "seg_frozen"), backbone=bb)
        m.precision = precision
        plan = m._make_plan(16, True, 0.0, True)
    want = BD.FLAG_SPLIT if precision == "f32-split" else BD.FLAG_BF16
    recs = tuple((kind, f) for prog in (plan.fwd, plan.bwd) for kind, f in prog.ops if kind in ("CONV", "WGRAD") and f.get("_flags", 0) & (BD.FLAG_BF16 | BD.FLAG_SPLIT))
    assert all(f["_flags"] & want for _, f in recs)
    return recs


def _as_row(kind, f):
    """a plan's flagged CONV / WGRAD record as a table row (the tables' conventions are asserted)"""
    from s2lc_amd.plan import opdefs as D

    has = lambda k: f.get(k) is not None     # noqa: E731
    split = bool(f["_flags"] & BD.FLAG_SPLIT)
    if kind == "CONV":
        nrep = max(f.get("NREP", 1), 1)
        r = T.R(f["B"], f["C1"], f["H"], f["W"], f["M"], C2=f["C2"], k=f["KH"], s=f["STRIDE"], pro=f["PRO1"], pro2=f["PRO2"], gate=has("GATE1"),
                x16=bool(f.get("X1_BF16", 0)), bias=has("BIAS"), stats=has("STATS"), beta=f["BETA"], res=has("RES"), scratch=has("SCRATCH"),
                yc=f["YC"] if (f["MODE"] == 0 and f["YC"] != f["M"]) else None, mode=f["MODE"],
                nrep=nrep if (has("STATS") and nrep != D.stats_replicas(f["M"])) else None, split=split, prod=True)
        rec = T.record(r)
        assert f["KH"] == f["KW"] and all(rec[k] == f[k] for k in ("HO", "WO", "PAD_T", "PAD_L", "PRO2", "STRIDE")) and rec["NREP"] == nrep, f
        assert f["W_ST"] == (f["M"] + 127) // 128 * 128 and f["W_SM"] == 1 and f["FLIP"] == 0 and has("WTB")
        return r
    r = T.RW(f["B"], f["M"], f["C"], f["H"], f["W"], k=f["KH"], s=f["STRIDE"], prop=f["PROP"], proq=f["PROQ"], gateq=has("GATEQ"), gatep=has("GATEP"),
             p16=bool(f.get("P_BF16", 0)), ct=f["CTOT"], coff=16 if f["CTOT"] - f["C"] >= 16 else 0, split=split, prod=True)
    rec = T.record(r)
    assert f["KH"] == f["KW"] and all(rec[k] == f[k] for k in ("HO", "WO", "PAD_T", "PAD_L", "STRIDE")) and f["MODE"] == 0, f
    return r


def _prod_key(r):
    """what a PROD row must share with the plan record it stands for: family, instantiation, edges and the map geometry (a WGS column
    slice counts as one with an offset: the plan's own offset is not a record field)"""
    v = T.launch(r)
    return (v.result, v.inst, T.row_edges(r), r["H"], r["W"], r["k"], r.get("mode", 0))


@pytest.mark.parametrize("which,precision", PLANS)
def test_every_flagged_production_record_has_a_prod_row_with_its_instantiation_and_edges(which, precision):
    have = {_prod_key(r) for r in T.TABLES["PROD"]}
    recs = _plan_records(which, precision)
    print(f"{which} {precision}: {len(recs)} flagged CONV / WGRAD records")
    assert recs or (which, precision) == ("mae", "f32-split")         # (the MAE model has no f32-split stages)
    rows = [_as_row(k, f) for k, f in recs]
    off = [T.rid(r) for r in rows if T.launch(r).result != (5 if precision == "f32-split" else 2)]
    assert not off, f"{which}: flagged records the restated launcher does not take: {off[:3]}"
    missing = {T.rid(r): (k[1], sorted(k[2])) for r in rows for k in [_prod_key(r)] if k not in have}
    assert not missing, f"{which}: {len(missing)} flagged records without a PROD row of the same instantiation, edges and map size, e.g. {list(missing.items())[:3]}"


def test_prod_rows_are_all_needed():
    """a PROD row stands for at least one record of a production plan (nothing stale in the table)"""
    used = {_prod_key(_as_row(k, f)) for which, prec in PLANS for k, f in _plan_records(which, prec)}
    stale = [T.rid(r) for r in T.TABLES["PROD"] if _prod_key(r) not in used]
    assert not stale, stale


# ---------------------------------------------------------------------------------------------------------------------------------
# the older bf16 / split rows of tests/test_ops_gpu.py and tests/test_f32_split_ops_gpu.py through the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _params(fn):
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize" and "," in m.args[0]]
    return mark.args[1]


def older_rows(split):
    """the bf16-mixed (split: f32-split) op-test cases as table rows, as their test functions hand them to _conv_case / _wgrad_case"""
    if split:
        from tests import test_f32_split_ops_gpu as O
        names = ("test_conv1x1_split", "test_conv3x3_split", "test_conv_transpose_scatter_split", "test_wgrad_1x1_split", "test_wgrad_3x3_split")
    else:
        from tests import test_ops_gpu as O
        names = ("test_conv1x1_bf16", "test_conv3x3_bf16", "test_conv_transpose_scatter_bf16", "test_wgrad_1x1_bf16", "test_wgrad_3x3_bf16")
    f = dict(split=split)
    rows = []
    for B, C1, H, W, M, pro, gate, bias, stats, beta in _params(getattr(O, names[0])):
        rows.append(T.R(B, C1, H, W, M, pro=pro, gate=gate, bias=bias, stats=stats, beta=beta, **f))
    for B, C1, C2, H, W, M, pro, beta in _params(getattr(O, names[1])):
        rows.append(T.R(B, C1, H, W, M, C2=C2, k=3, pro=pro, bias=True, stats=beta == 0, beta=beta, **f))
    for B, Cin, Cout, H, W, pro in _params(getattr(O, names[2])):
        rows.append(T.R(B, Cin, H, W, 4 * Cout, pro=pro, bias=True, mode=1, **f))
    for B, M, C, H, W, prop, proq, gate in _params(getattr(O, names[3])):
        rows.append(T.RW(B, M, C, H, W, prop=prop, proq=proq, gateq=gate, **f))
    for B, M, C, CT, c_off, H, W, proq in _params(getattr(O, names[4])):
        rows.append(T.RW(B, M, C, H, W, k=3, proq=proq, ct=CT, coff=c_off, **f))
    if not split:
        for B, M, C, H, W in _params(O.test_dy_stored_as_bf16_between_bn_apply_and_its_1x1_readers):
            rows += [T.R(B, M, H, W, C, x16=True, beta=1), T.RW(B, M, C, H, W, proq=2, p16=True)]
        for B, M, C, H, W in _params(O.test_dy_stored_as_bf16_read_by_3x3_stages):
            rows += [T.R(B, M, H, W, C, k=3, x16=True, beta=1), T.RW(B, M, C, H, W, k=3, proq=3, p16=True)]
    return rows


@pytest.mark.parametrize("split", [False, True])
def test_family_pins_of_the_older_rows_match_the_restatement(split):
    rows = older_rows(split)
    assert len(rows) >= (50 if not split else 40)
    fam = 5 if split else 2
    wrong = [(T.rid(r), T.launch(r).result) for r in rows if T.launch(r).result != fam]
    assert not wrong, wrong
    old = {T.launch(r).inst for r in rows}
    mine = {i for i in reachable() if i[1][-1] == split}
    new = {T.launch(r).inst for r in _rows(FAMILY)} & mine
    print(f"older {'f32-split' if split else 'bf16-mixed'} rows: {len(rows)} rows reach {len(old & mine)} of {len(mine)} instantiations; the new tables reach {len(new)}")
    assert old <= new


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference alone: on every row's data the f32 oracle (family 2: on bf16-rounded operands) must agree with the float64 reference
# (family 2: the float64-sum reference of the bf16 operation) to a quarter of each bar the GPU test uses, so that three quarters of
# every bar are left for the kernel (a row that fails this gets other data, not another bar)
# ---------------------------------------------------------------------------------------------------------------------------------
SLOWEST = {}


def _oracles(r, data):
    c, outs, pre, fields = T.build(r, data)
    t0 = time.time()
    cpu, wide = c.oracles(T.program(pre, r["kind"], fields), ref64=True)
    return c, outs, cpu, wide, time.time() - t0


@pytest.mark.parametrize("r", _rows(list(FAMILY) + ["PROD"]), ids=T.rid)
def test_f32_oracle_is_within_a_quarter_of_each_bar_of_the_float64_reference(r):
    fam = T.launch(r).result
    c, outs, cpu, wide, dt = _oracles(r, "spread" if r["spread"] else "random")
    SLOWEST[T.rid(r)] = dt
    out = outs[0]
    a, t = c.read(cpu, out).double(), c.read(wide, out, wide=True).double()
    assert torch.isfinite(t).all()
    whole, part = T.rel(T.by_part(r, a), T.by_part(r, t))
    worst = {out: whole, out + " per part": part}
    if r.get("stats"):
        s32, s64 = c.read(cpu, "stats").sum(0), c.read(wide, "stats", wide=True).sum(0)
        worst["stats"], worst["stats per column"] = T.rel(s32, s64)
    tol = T.bars(r, fam)
    bad = {k: v for k, v in worst.items() if not v < tol / 4}
    assert not bad, f"the f32 oracle alone is off by {bad} (a quarter of the bar: {tol / 4:.1e})"
    print(f"{T.rid(r)}: {dt:.2f} s, worst {max(worst.values()):.2e}")


def test_slowest_row_is_reported():
    if SLOWEST:
        name = max(SLOWEST, key=SLOWEST.get)
        print(f"slowest row (two oracle runs): {name} {SLOWEST[name]:.2f} s")


def _quantum(v):
    """the largest power of two every element of v is an integer multiple of"""
    nz = v[v != 0].double()
    if not nz.numel():
        return 1.0
    m, e = torch.frexp(nz)
    mi = (m.abs() * 2.0 ** 53).long()
    return float(((mi & -mi).double() * torch.pow(2.0, e.double() - 53)).min())


@pytest.mark.parametrize("r", [r for r in _rows(list(FAMILY) + ["PROD"]) if not r["split"]], ids=T.rid)
def test_lattice_data_is_exact_in_bf16_and_in_f32_sums(r):
    """the exact pass of a family-2 row: bf16 rounding is the identity on every activated operand and on the weights, every value of
    the result is a 24-bit multiple of its channel's unit even if every product had the same sign, and the f32 oracle equals float64"""
    from oracle.ops_ref import _pro, _r16

    c, outs, cpu, wide, _ = _oracles(r, "exact")
    item = lambda n: c.items[n][1].float() if n in c.items else None       # noqa: E731
    if r["kind"] == "CONV":
        act = [_pro(item("x1"), item("bnv1"), item("gate1"), r["pro"], r["C1"])]
        if r["C2"]:
            act.append(_pro(item("x2"), item("bnv2"), None, r["pro2"], r["C2"]))
        w = item("wt")
        ops = [(torch.cat(act, 1), "activated X"), (w, "weights")]
        # the channel scaling 2^-(c mod 8) taken back out: what is left is the lattice
        ch = 2.0 ** (torch.arange(w.shape[1 if r["mode"] == 1 else 0]) % 8)
        sides = [ops[0][0], w * (ch.view(1, -1, 1) if r["mode"] == 1 else ch.view(-1, 1, 1))]
        terms, old, old_unit = (r["C1"] + r["C2"]) * r["k"] ** 2, 0, 1.0
    else:
        P = _pro(item("p"), item("bnvp"), item("gatep"), r["prop"], r["M"])
        Q = _pro(item("q"), item("bnvq"), item("gateq"), r["proq"], r["C"])
        ops = [(P, "activated P"), (Q, "activated Q")]
        big = r["proq"] in (2, 4)
        cols = 2.0 ** (torch.arange(r["ct"]) % 8)[r["coff"]:r["coff"] + r["C"]]
        sides = [P, Q if big else Q * cols.view(1, -1, 1, 1)]
        old_unit = (16.0 if r["prop"] in (2, 4) else 1.0) * (16.0 if big else 1.0)     # test_b16_kernels_gpu.build_wgrad: the lattice WGS it accumulates into
        terms, old = r["B"] * r["H"] * r["W"], 8 * old_unit
    for v, what in ops:
        assert torch.isfinite(v).all() and torch.equal(_r16(v), v), f"bf16 rounding changes the {what}"
    steps = [float(v.abs().max()) / _quantum(v) for v in sides]
    unit = _quantum(sides[0]) * _quantum(sides[1])
    assert max(steps) < 2 ** 8, f"an operand of {max(steps):.0f} steps does not fit 8 significant bits"
    bound = (terms * float(sides[0].abs().max()) * float(sides[1].abs().max()) + old) / (min(unit, old_unit) if old else unit)
    assert bound < 2 ** 24, f"{terms} terms of up to {steps[0]:.0f} x {steps[1]:.0f} steps: {bound:.3g} units >= 2^24"
    out = outs[0]
    assert torch.equal(c.read(cpu, out).double(), c.read(wide, out, wide=True).double()), "the f32 oracle and the float64 reference differ on lattice data"
