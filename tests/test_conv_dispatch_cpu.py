"""Coverage of the dense-convolution GPU tables (tests/test_conv_kernels_gpu.py), checked without a GPU.

The launch sites and macros of csrc/igemm.hip, igemm_pc.hip, conv_dma.hip and conv_q4.hip are parsed into the set of template
instantiations the chain can launch at default tuning; every threshold tests/conv_dispatch.py restates is looked up in the source
text.  The tables must reach every such instantiation, every required edge per kernel that can meet it, and the instantiation and
edges of every CONV record of the production plans; the family column of every row (and of the older CONV rows in
tests/test_ops_gpu.py) must be what the restated launcher takes; and on every row's data the f32 oracle alone must stay within a
quarter of each bar against the float64 oracle."""
import functools
import itertools
import re
from pathlib import Path

import pytest
import torch

from tests import conv_dispatch as CD
from tests import test_conv_kernels_gpu as T
from tests.conv_dispatch import DMA, GENERIC, PC, Q4

CSRC = Path(__file__).resolve().parents[1] / "sentinel2-landcover-classification_amd" / "csrc"
PRO = {"S2K_PRO_NONE": 0, "S2K_PRO_RELU": 3}
BOOL = {"true": True, "false": False}


def _src(name):
    return (CSRC / name).read_text()


def _ints(m):
    return tuple(int(v) for v in m)


def _macro(src, name):
    """body of `#define name(...)` with its continuation lines joined"""
    m = re.search(r"#define " + name + r"\([^)]*\)((?:[^\n]*\\\n)*[^\n]*)", src)
    assert m, f"macro {name} not found"
    return m.group(1).replace("\\\n", " ")


def _calls(src, name, n):
    """argument tuples of every invocation of macro `name` with n integer arguments, outside #define lines"""
    body = re.sub(r"#define [^\n]*(?:\\\n[^\n]*)*", "", src)
    return [_ints(m) for m in re.findall(r"\b" + name + r"\(" + r",\s*".join([r"\s*(\d+)"] * n) + r"\s*[,)]", body)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the instantiations each file can launch: {(kernel, template arguments): reason it cannot be reached at default tuning, or None}
# ---------------------------------------------------------------------------------------------------------------------------------
def generic_launches():
    src = _src("igemm.hip")
    out = {}
    forms = re.findall(r"launch_cfg<BM_PIX, 1, WMv, WNv, WVMv, WVNv, KCHv, 1, 2, (true|false)>", _macro(src, "PIX_CFG"))
    assert sorted(forms) == ["false", "true"], forms
    body = re.sub(r"#define [^\n]*(?:\\\n[^\n]*)*", "", src)
    pix = re.findall(r"if \(([^\n]*?)\) return PIX_CFG\((\d+), (\d+), (\d+), (\d+), (\d+), cdiv\(p\.Ntot, (\d+)\), (true|false)\);|"
                     r"^\s*return PIX_CFG\((\d+), (\d+), (\d+), (\d+), (\d+), cdiv\(p\.Ntot, (\d+)\), (true|false)\);", body, flags=re.M)
    cfgs = []
    for m in pix:
        cond, a = (m[0], m[1:8]) if m[1] else ("", m[8:15])
        cfg = _ints(a[:6]) + (BOOL[a[6]],)
        forced = "force_cfg ==" in cond
        if not forced:
            cfgs.append(cfg)
        for bvec in (True, False):
            key = ("conv_igemm_kernel", (CD.BM_PIX, 1) + cfg[:5] + (1, 2, bvec))
            if not forced:
                out[key] = None
            else:
                out.setdefault(key, "S2K_PIX_FORCE is 0")
    sp = re.findall(r"launch_cfg<BM_SPATIAL, 9, (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)(?:, (\d+))?>\(p, \(int\)tiles, st\)", body)
    spc = [_ints(m[:6]) + (int(m[6]) if m[6] else 2,) for m in sp]
    for cfg in spc:
        out[("conv_igemm_kernel", (CD.BM_SPATIAL, 9) + cfg + (False,))] = None
    return out, cfgs, spc


def pc_launches():
    src = _src("igemm_pc.hip")
    out = {}
    bm_body = re.search(r"static int launch_pc_bm\(.*?\n}\n", src, flags=re.S).group(0)
    bm_forms = [(int(wm), PRO[pro]) for wm, pro in re.findall(r"launch_pc<BMODE, (\d), KCH, R, XW, (S2K_PRO_\w+)>", bm_body)]
    assert sorted(set(bm_forms)) == [(1, 0), (1, 3), (2, 0), (2, 3)], bm_forms
    assert "if (bm == 128) return relu ? launch_pc<BMODE, 2," in bm_body

    def via_bm(bmode, kch, r, xw, why):
        for wm, pro in set(bm_forms):
            out[("conv_pc_kernel", (bmode, wm, kch, r, xw, pro, False, False))] = why
    main = src[src.index("int launch_conv_pc("):]
    for m in re.finditer(r"launch_pc<(BM_\w+), (\d+), (\d+), (\d+), (\d+), (S2K_PRO_\w+)(?:, (true|false))?(?:, (true|false))?>", main):
        bmode = CD.BM_PIX if m.group(1) == "BM_PIX" else CD.BM_SPATIAL
        args = (bmode,) + _ints(m.groups()[1:5]) + (PRO[m.group(6)], BOOL[m.group(7) or "false"], BOOL[m.group(8) or "false"])
        line = main[main.rfind("\n", 0, m.start()):m.start()]
        out[("conv_pc_kernel", args)] = "S2K_CONV_PC_THIN_KCH is 4" if "kch == 8" in line else None
    for m in re.finditer(r"(if \(kch1 == 64\) )?return launch_pc_bm<BM_PIX, (\d+), (\d+), (\d+)>", main):
        via_bm(CD.BM_PIX, *_ints(m.groups()[1:]), "S2K_CONV_PC_KCH1 is 32" if m.group(1) else None)
    pc3 = _macro(src, "PC3")
    kchs = _ints(re.findall(r"launch_pc_bm<BM_SPATIAL, (\d+), RR, XX>", pc3))
    assert kchs == (8, 4) and "if (kch3 == 8 || (kch3 == 4 && p.M >= %d))" % CD.PC_KCH3_WIDE_M in pc3
    geoms = []
    for cond, r, xw in re.findall(r"if \(([^\n]*?)\) PC3\((\d+), (\d+)\)", main):
        widths = "mult64" if cond == "p.WO >= 64 && p.WO % 64 == 0" else _ints(re.findall(r"p\.WO == (\d+)", cond))
        assert widths == "mult64" or " || ".join(f"p.WO == {w}" for w in widths) == cond, cond
        geoms.append(((int(r), int(xw)), widths))
        for kch in kchs:
            via_bm(CD.BM_SPATIAL, kch, int(r), int(xw), None)
    return out, geoms


def _ring_go(src, prefix, kernel_launch):
    go = _macro(src, prefix + "_GO")
    m = re.search(r"k32 \? " + kernel_launch + r"<([\w, ]+), 3, PREv, 32>.*? : " + kernel_launch + r"<([\w, ]+), 4, PREv, 16>", go)
    assert m and m.group(1) == m.group(2), go
    return ((3, 32), (4, 16))


def dma_launches():
    src = _src("conv_dma.hip")
    out = {}
    depths = _ring_go(src, "DMA", "launch_dma")
    assert "launch_dma<WMv, WNv, 4, PREv, 16>" in _macro(src, "DMA_BIG")
    assert "return pre ? DMA_GO(WMv, WNv, true) : DMA_GO(WMv, WNv, false);" in _macro(src, "DMA_CFG")
    assert "&& !pre) return DMA_GO(WMv, WNv, false);" in _macro(src, "DMA_CFG_NOPRE")
    main = src[src.index("int launch_conv_dma("):]
    assert "const bool big = best_wm == 5 || (best_wm == 4 && best_wn == 2);" in main and "const bool k32 = !big &&" in main
    for wm, wn in _calls(main, "DMA_CFG", 2):
        for (nst, kch), pre in itertools.product(depths, (True, False)):
            out[("conv_dma_kernel", (wm, wn, nst, pre, kch))] = None
    for wm, wn in _calls(main, "DMA_CFG_NOPRE", 2):
        for nst, kch in depths:
            out[("conv_dma_kernel", (wm, wn, nst, False, kch))] = None
    for wm, wn, pre in re.findall(r"DMA_BIG\((\d), (\d), (true|false)\)", re.sub(r"#define [^\n]*", "", main)):
        assert (int(wm), int(wn)) in ((5, 1), (4, 2))
        out[("conv_dma_kernel", (int(wm), int(wn), 4, BOOL[pre], 16))] = None
    return out


def q4_launches():
    src = _src("conv_q4.hip")
    out = {}
    depths = _ring_go(src, "Q4", "launch_q4")
    main = src[src.index("int launch_conv_q4("):]
    cands = [_ints(c) for c in re.findall(r"\{(\d), (\d), (\d)\}", re.search(r"cands\[5\] = \{(.*?)\};", main).group(1))]
    assert "const bool wide = c.wvn == 4;" in main and "const bool k32 = !wide &&" in main
    for name, pres in (("Q4_CFG2", (0, 1)), ("Q4_CFG1", (0, 1, 2))):
        for i, wm, wvm, wvn in _calls(main, name, 4):
            assert cands[i] == (wm, wvm, wvn), (name, i)
            for (nst, kch), pre in itertools.product(depths, pres):
                out[("conv_q4_kernel", (wm, wvm, wvn, nst, pre, kch))] = None
    for m in re.findall(r"launch_q4<(\d), (\d), (\d), (\d), (\d), (\d+)>", main):
        a = _ints(m)
        assert cands[2] == a[:3] and "if (best == 2) return" in main
        out[("conv_q4_kernel", a)] = None
    return out, cands


def launched():
    out = {}
    for part in (generic_launches()[0], pc_launches()[0], dma_launches(), q4_launches()[0]):
        assert not set(part) & set(out)
        out.update(part)
    return out


def reachable():
    return {k for k, why in launched().items() if why is None}


# ---------------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows():
    return [r for tab in T.TABLES.values() for r in tab]


def _cv(r):
    return CD.dispatch(**T.record(r))


def test_macro_parse_finds_every_launch_site():
    got = launched()
    per = {k: sum(1 for i in got if i[0] == k) for k in ("conv_igemm_kernel", "conv_pc_kernel", "conv_dma_kernel", "conv_q4_kernel")}
    # instantiated by the launch sites / reachable at default tuning: the counts the coverage test below works with
    reach = {k: sum(1 for i in reachable() if i[0] == k) for k in per}
    print("launched", per, "reachable", reach)
    assert per == {"conv_igemm_kernel": 16, "conv_pc_kernel": 62, "conv_dma_kernel": 29, "conv_q4_kernel": 22}, per
    assert reach == {"conv_igemm_kernel": 16, "conv_pc_kernel": 56, "conv_dma_kernel": 29, "conv_q4_kernel": 22}, reach
    # what default tuning cannot reach, by name: the 64-channel chunks of the 1x1 producer / consumer kernel (S2K_CONV_PC_KCH1 = 64)
    # and the thin 3x3 form with 8-channel chunks (S2K_CONV_PC_THIN_KCH = 8)
    unreachable = {k: why for k, why in got.items() if why is not None}
    assert unreachable == {
        **{("conv_pc_kernel", (CD.BM_PIX, wm, 64, 1, 64, pro, False, False)): "S2K_CONV_PC_KCH1 is 32" for wm in (1, 2) for pro in (0, 3)},
        **{("conv_pc_kernel", (CD.BM_SPATIAL, 1, 8, 4, 64, pro, True, False)): "S2K_CONV_PC_THIN_KCH is 4" for pro in (0, 3)}}, unreachable


TUNE_DEFAULTS = {
    "igemm.hip": {"S2K_SPLITS": 0, "S2K_CV_EXP": 0, "S2K_PIX_SMALL_TILES": CD.PIX_SMALL_TILES, "S2K_PIX_K16_MAX": CD.PIX_K16_MAX, "S2K_PIX_NOVEC": 0,
                  "S2K_PIX_FORCE": 0, "S2K_THIN": 1},
    "igemm_pc.hip": {"S2K_CONV_PC": 3, "S2K_CONV_PC_THIN": 1, "S2K_CONV_PC_THIN_KCH": CD.PC_THIN_KCH, "S2K_CONV_PC_NARROW": 1, "S2K_CONV_PC_KCH1": CD.PC_KCH1,
                     "S2K_CONV_PC_KCH3": CD.PC_KCH3},
    "conv_dma.hip": {"S2K_DMA_PER_CU": 1, "S2K_CONV_DMA": 1, "S2K_DMA_WM": 0, "S2K_DMA_WN": 0, "S2K_DMA_SPLITS": 0, "S2K_DMA_KCH": 0},
    "conv_q4.hip": {"S2K_Q4_PER_CU": 1, "S2K_CONV_Q4": 1, "S2K_Q4_TILE": -1, "S2K_Q4_SPLITS": 0, "S2K_Q4_KCH": 0},
}


@pytest.mark.parametrize("name", list(TUNE_DEFAULTS))
def test_every_tuning_default_is_the_one_the_restatement_assumes(name):
    got = {k: int(v) for k, v in re.findall(r'tune_int\("(\w+)", (-?\d+)\)', _src(name))}
    assert got == TUNE_DEFAULTS[name], f"{name}: a tuning switch changed or was added: restate it in tests/conv_dispatch.py"


def _thresholds():
    """file -> source fragments that state the thresholds tests/conv_dispatch.py uses, written from its constants"""
    C = CD
    a, b = C.SPLITK_A, C.SPLITK_B
    ps, pk, p128, p64, p32 = C.PIX_SMALL, C.PIX_128_K16, C.PIX_128, C.PIX_64, C.PIX_32

    def pix(c):
        return f"PIX_CFG({c[0]}, {c[1]}, {c[2]}, {c[3]}, {c[4]}, cdiv(p.Ntot, {c[5]}), {'true' if c[6] else 'false'});"

    def sp(c):
        return f"launch_cfg<BM_SPATIAL, 9, {c[0]}, {c[1]}, {c[2]}, {c[3]}, {c[4]}, {c[5]}" + (f", {c[6]}" if c[6] != 2 else "") + ">(p, (int)tiles, st);"
    dn, dk, dm = C.DMA_RULE
    lim, cap, minch, per = C.DMA_SPLIT
    f3, f2, pm, pm0, pn, pn0 = C.DMA_COST
    qa, qb = C.Q4_RULE_A, C.Q4_RULE_B
    qf, qs, qt = C.Q4_COST
    split_rule = (f"if (p.scratch && items < {lim} && nchunks >= {minch}) {{\n"
                  f"                sp = (int)std::min<int64_t>({cap}, std::min<int64_t>(nchunks / {per}, cdiv64({lim}, items)));")
    return {
        "igemm.hip": [
            "const int cands[3] = {128, 64, 32};", f"if (w <= {C.PICK_BM_WASTE}) return bm;", "if (w < best_w - 1e-9) { best_w = w; best = bm; }",
            "const int64_t tiles_big = (int64_t)cdiv(p.M, bm) * cdiv(p.Ntot, bm == 128 ? 128 : 256);",
            "const bool bvec = !novec && p.mode != S2K_MODE_GATHER2X2 && (p.HW & 3) == 0;",
            "if (bm >= 64 && tiles_big < small_max) return " + pix(ps), "if (bm == 128 && p.Ctot <= k16_max) return " + pix(pk),
            "if (bm == 128) return " + pix(p128), "if (bm == 64) return " + pix(p64), "        return " + pix(p32),
            f"force_splits == 0 && allow_splitk && p.scratch && p.mode == S2K_MODE_CONV && nchunks >= {C.SPLITK_MIN_CHUNKS}",
            f"if (blocks <= {a[0]}) splits = (int)cdiv64({a[1]}, blocks);",
            f"else if (blocks <= {b[0]} && nchunks >= {b[1]}) splits = (int)cdiv64({b[2]}, blocks);",
            f"if (splits > {C.SPLITK_MAX}) splits = {C.SPLITK_MAX};", "if (splits > nchunks / 2) splits = nchunks / 2;",
            "p.chunks_per_split = cdiv(nchunks, splits);\n            p.splits = cdiv(nchunks, p.chunks_per_split);",
            f"if (BN >= {C.TEPI_BN[0]} && BN <= {C.TEPI_BN[1]} && p.splits == 1 && p.mode != S2K_MODE_CONVT_SCATTER &&",
            "((BMODE == BM_PIX && (p.HW & 3) == 0) || (BMODE == BM_SPATIAL && (p.XW & 3) == 0 && (p.WO & 3) == 0))",
            "(BMODE == BM_SPATIAL || (p.HW % BN) == 0) ? 1 : std::min<int64_t>(p.B, (BN - 2) / p.HW + 2);", "if (need >= 0x7ffffff0ll)",
            f"if (!geom(128, {C.SP_128[5]} * NTHREADS))", f"if (tiles * cdiv(p.M, 128) >= {C.SP_MIN_TILES}) return " + sp(C.SP_128),
            f"if ((int64_t)cdiv(p.M, 64) * cdiv64(out_px, 256) >= {C.SP_MIN_TILES} && geom(256, {C.SP_64W[5]} * NTHREADS))", "return " + sp(C.SP_64W),
            f"if (!geom(64, {C.SP_64[5]} * NTHREADS))", "return " + sp(C.SP_64),
            f"if (thin_mode == 1 && p.S == 1 && cdiv64(out_px, 512) >= {C.SP_THIN_MIN} && geom(512, {C.SP_THIN512[5]} * NTHREADS))", "return " + sp(C.SP_THIN512),
            f"if (p.S == 1 && cdiv64(out_px, 1024) >= {C.SP_THIN_MIN} && geom(1024, {C.SP_THIN1024[5]} * NTHREADS))", "return " + sp(C.SP_THIN1024),
            f"if (!geom(256, {C.SP_32[5]} * NTHREADS))", "return " + sp(C.SP_32),
            "p.XW = p.WO <= BN ? p.WO : BN;", "if (R > p.HO) R = p.HO;", "if (p.IR * p.WS <= cap) break;",
            "if (p.wtq) {", "} else if (p.force_dma) {", "if (T != 9 || p.S > 2)",
        ],
        "igemm_pc.hip": [
            "if (p.mode != S2K_MODE_CONV || p.S != 1 || p.gate1) return 1;", "if (p.pro1 != S2K_PRO_NONE && p.pro1 != S2K_PRO_RELU) return 1;",
            "if (p.C2 > 0 && p.pro2 != p.pro1) return 1;", f"if (p.M <= {C.PC_THIN_MAX_M} && p.KH == 3 && p.KW == 3) {{",
            f"p.PT != 1 || p.PL != 1 || p.WO % 64 != 0 || p.M < {C.PC_THIN_MIN_M}) return 1;", f"if (n < {C.PC_THIN_MIN_TILES}) return 1;",
            f"if (p.M < {C.PC_MIN_M}) return 1;", f"const int bm = ((double)cdiv(p.M, 128) * 128 / p.M <= {C.PC_BM_PAD}) ? 128 : 64;",
            "if (!(enabled & 1) || p.C2 != 0 || (p.HW & 3) || p.HO != p.H || p.WO != p.W) return 1;",
            f"if ((int64_t)cdiv(p.M, bm) * n_ntiles < {C.PC_PIX_MIN_TILES}) {{",
            f"if (!narrow || p.Ctot < {C.PC_NARROW_MIN_K} || (int64_t)cdiv(p.M, 64) * n64 < {C.PC_NARROW_MIN_TILES}) return 1;",
            f"if (p.Ctot < {C.PC_PIX_MIN_K}) return 1;", f"if ((int64_t)cdiv(p.M, bm) * n < {C.PC3_MIN_TILES}) return 1;",
            "if (!(enabled & 2) || T != 9 || p.KH != 3 || p.HO != p.H || p.WO != p.W || p.PT != 1 || p.PL != 1) return 1;",
            "constexpr bool TEPI = BMODE == BM_PIX || XW % 4 == 0;",
        ],
        "conv_dma.hip": [
            "if (!enabled || p.res_mul) return 1;",
            "if (p.mode != S2K_MODE_CONV || p.KH != 1 || p.KW != 1 || p.S != 1 || p.C2 != 0 || p.gate1 || p.pro1 != S2K_PRO_NONE || p.x1_bf16) return 1;",
            "if ((p.HW & 3) || p.HO != p.H || p.WO != p.W) return 1;", f"if (p.M < {C.DMA_MIN_M}) return 1;",
            f"if (enabled != 2 && !p.force_dma && !(p.Ntot <= {dn} && (p.Ctot >= {dk} || p.M >= {dm}))) return 1;",
            "const int nchunks = cdiv(p.Ctot, 16);", "const bool pre = p.bias || p.res || p.beta;",
            f"for (int wm = 1; wm <= {C.DMA_MAX_WM}; ++wm) {{", f"for (int wn = 1; wn <= {C.DMA_MAX_WN}; ++wn) {{", "if (wm == 5 && wn == 2) continue;",
            f"if (pre && wm * wn > {C.DMA_PRE_MAX_TILES}) continue;", "if (nmt * bm > p.w_st) continue;", split_rule,
            "const double rounds = (double)cdiv64(items * sp, 256);",
            f"const double per_item = (double)bm * 64 * wn * ((double)cdiv(nchunks, sp) + {f3} + (sp > 1 ? {f2} : 0.0));",
            f"const double cost = rounds * per_item * (1.0 + {pm} * ({pm0} - wm) + {pn} * ({pn0} - wn));",
            "if (cost < best_cost) { best_cost = cost; best_wm = wm; best_wn = wn; best_sp = sp; }", f"(force_kch ? force_kch == 32 : p.Ctot > {C.DMA_K32_MIN});",
            "cb = __builtin_amdgcn_readfirstlane((ks * nchunks) / p.splits);", "const int grid = (int)std::min<int64_t>(items, n_slots[dev]);",
        ],
        "conv_q4.hip": [
            "if (!enabled || !p.wtq || p.res_mul) return 1;",
            "if (p.mode != S2K_MODE_CONV || p.KH != 1 || p.KW != 1 || p.S != 1 || p.C2 != 0 || p.gate1 || p.pro1 != S2K_PRO_NONE || p.x1_bf16) return 1;",
            "if ((p.HW & 3) || p.HO != p.H || p.WO != p.W) return 1;", f"if (p.M < {C.Q4_MIN_M}) return 1;",
            f"!((p.Ntot >= {qa[0]} && p.M >= {qa[1]} && p.Ctot < {qa[2]}) || (p.Ntot <= {qb[0]} && p.M <= {qb[1]} && p.Ctot >= {qb[2]}))) return 1;",
            "const int pre = (p.res || p.beta) ? 2 : (p.bias ? 1 : 0);", "if (pre == 2 && c.wm != 1) continue;", "if (nmt * bm > p.w_st) continue;", split_rule.replace("    sp =", "sp =").replace("            if (p.scratch", "        if (p.scratch"),
            "const double rounds = (double)cdiv64(items * sp, 256);",
            f"const double per_item = (double)bm * bn * ((double)cdiv(nchunks, sp) + {qf} + (sp > 1 ? {qs} : 0.0));",
            f"const double cost = rounds * per_item * (c.wm == 1 ? {qt:.2f} : 1.0);", "if (cost < best_cost) { best_cost = cost; best = ci; best_sp = sp; }",
            f"(force_kch ? force_kch == 32 : p.Ctot > {C.Q4_K32_MIN});", "cb = __builtin_amdgcn_readfirstlane((ks * nchunks) / p.splits);",
            "const int grid = (int)std::min<int64_t>(items, (int64_t)n_cu[dev] * per_cu);",
        ],
    }


@pytest.mark.parametrize("name", ["igemm.hip", "igemm_pc.hip", "conv_dma.hip", "conv_q4.hip"])
def test_every_threshold_of_the_restatement_stands_in_the_source(name):
    src = re.sub(r"[ \t]+", " ", _src(name))
    missing = [t for t in _thresholds()[name] if re.sub(r"[ \t]+", " ", t) not in src]
    assert not missing, f"{name} no longer says (tests/conv_dispatch.py restates it):\n  " + "\n  ".join(missing)


def test_tile_tables_of_the_restatement_are_the_parsed_ones():
    _, pix, sp = generic_launches()
    assert pix == [CD.PIX_SMALL, CD.PIX_128_K16, CD.PIX_128, CD.PIX_64, CD.PIX_32]
    assert sp == [CD.SP_128, CD.SP_64W, CD.SP_64, CD.SP_THIN512, CD.SP_THIN1024, CD.SP_32]
    assert tuple(pc_launches()[1]) == CD.PC3_GEOMS
    assert tuple(q4_launches()[1]) == CD.Q4_CANDS


# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_row_is_in_exactly_one_gpu_test():
    import inspect

    ids = [T.rid(r) for r in _rows()]
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
    cv = _cv(r)
    assert cv.family == r["fam"], f"family column {r['fam']}, the launcher takes {cv.inst} (family {cv.family}) after {cv.declined}"


def test_each_table_holds_its_own_family():
    fam = {"GENERIC": GENERIC, "PC": PC, "DMA_RING": DMA, "QUAD": Q4}
    for name, tab in T.TABLES.items():
        if name in fam:
            assert {r["fam"] for r in tab} == {fam[name]}, name


def test_tables_reach_every_reachable_instantiation():
    want = reachable()
    got = {_cv(r).inst for r in _rows()}
    missing = sorted(want - got, key=str)
    print(f"{len(want)} reachable instantiations, {len(got & want)} reached by {len(_rows())} rows")
    assert not missing, f"{len(missing)} instantiations no GPU row reaches:\n  " + "\n  ".join(map(str, missing))
    assert got <= want, f"rows reach instantiations the macros do not launch: {sorted(got - want, key=str)}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's own error: on every row's data the f32 oracle must agree with the float64 oracle to a quarter of each bar, so
# that three quarters of every bar are left for the kernel (a row that fails this gets other data - scale, seed, fill - not
# another bar)
# ---------------------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return ((a - b).abs().amax(0) / b.abs().amax(0).clamp_min(1e-20)).max().item()


@pytest.mark.parametrize("r", _rows(), ids=T.rid)
def test_f32_oracle_is_within_a_quarter_of_each_bar_of_the_float64_oracle(r):
    from s2lc_amd.plan.program import Program

    c, outs, pre, fields = T.build(r)
    prog = Program()
    prog.add(pre[0], **pre[1])
    prog.add("CONV", **fields)
    cpu, wide = c.oracles(prog.pack(), ref64=True)
    y32, y64 = c.read(cpu, "y").double(), c.read(wide, "y", wide=True)
    assert torch.isfinite(y64).all()
    n = y32.shape[1]
    per = lambda v: v.reshape(v.shape[0], n, -1).transpose(0, 1).reshape(n, -1).t()     # noqa: E731  (rows x channels, as Case.run)
    whole = (y32 - y64).abs().max().item() / y64.abs().max().item()
    worst = {"y": whole, "y per channel": _rel(per(y32), per(y64))}
    if r["stats"]:
        s32, s64 = c.read(cpu, "stats").sum(0), c.read(wide, "stats", wide=True).sum(0)
        worst["stats"] = (s32 - s64).abs().max().item() / s64.abs().max().item()
        worst["stats per column"] = _rel(s32, s64)
    bad = {k: v for k, v in worst.items() if not v < T.TOL / 4}
    assert not bad, f"the f32 oracle alone is off by {bad} (a quarter of the bar: {T.TOL / 4:.1e})"


# ---------------------------------------------------------------------------------------------------------------------------------
# edges: every one below needs a row in the table of each kernel that can meet it (Cv.edges + test_conv_kernels_gpu.row_edges)
# ---------------------------------------------------------------------------------------------------------------------------------
_EPI = ["bias", "beta", "residual", "residual x gelu'", "statistics", "statistics replicas > 1", "one statistics replica", "YC > M"]
_TILES = ["ragged last m-tile", "M one past a tile", "ragged last pixel tile", "pixel tile straddles 2 images", "pixel tile straddles >= 3 images"]
_RING = _TILES + ["K tail", "K < one chunk", "split-K", "no split-K", "split-K: the splits differ in length", "would split with SCRATCH, has none",
                  "more items than workgroups, with a remainder", "fewer items than workgroups", "32-channel stages", "16-channel stages",
                  "reduce tail: bias", "reduce tail: statistics", "reduce tail: beta", "reduce tail: residual"] + [e for e in _EPI if e != "residual x gelu'"]
REQUIRED = {
    "GENERIC": _TILES + _EPI + [
        "M = 4", "vector stager", "scalar stager", "transposed epilogue", "scalar epilogue", "partial last tile row", "partial last tile column",
        "several x tiles per row", "R capped by HO", "R cut by the halo capacity", "stride 2", "K tail", "K < one chunk", "K tail in source 2",
        "concat with pro2 != pro1", "a chunk holds channels of both sources", "split-K rule A (blocks <= 512)",
        "split-K rule B (512 < blocks <= 1024, >= 32 chunks)", "split-K: the splits differ in length", "split-K capped at 8", "split-K capped at nchunks / 2",
        "would split with SCRATCH, has none", "reduce tail: bias", "reduce tail: statistics", "reduce tail: beta", "reduce tail: residual",
        "prologue 0", "prologue 1", "prologue 2", "prologue 3", "prologue 4", "SE gate", "scatter mode", "gather mode", "SiLU beyond the exp range"],
    "PC": [e for e in _TILES if e != "pixel tile straddles >= 3 images"] + _EPI + [
        "transposed epilogue", "scalar epilogue", "partial last tile row", "several x tiles per row", "K tail", "K < one chunk", "K tail in source 2",
        "a chunk holds channels of both sources", "prologue 0", "prologue 3"],
    "DMA_RING": _RING,
    "QUAD": _RING,
}
# (the pc kernel's 1x1 tiles hold >= 64 pixels of maps with HW % 4 == 0, so a tile can straddle >= 3 images only on maps of <= 28
# pixels - with >= 192 tiles and K >= 256 that is a problem of its own size; the generic, ring and quad rows have it)


@pytest.mark.parametrize("table,edge", [(t, e) for t, es in REQUIRED.items() for e in es])
def test_required_edge_has_a_row_in_the_kernels_table(table, edge):
    assert any(edge in T.row_edges(r) for r in T.TABLES[table]), f"no {table} row meets: {edge}"


def _some(table, pred):
    return any(pred(r, _cv(r), T.row_edges(r)) for r in T.TABLES[table])


def test_combined_edges():
    """edges that only count together; every missing combination is reported"""
    g = "GENERIC"
    want = []

    def need(what, table, pred):
        want.append((f"{table}: {what}", _some(table, pred)))
    # HW % 4 == 0 with the transposed store on and off (off: a K split or the scatter mode)
    need("vector stager + transposed store", g, lambda r, cv, e: "vector stager" in e and "transposed epilogue" in e)
    need("vector stager + K split", g, lambda r, cv, e: "vector stager" in e and "split-K" in e)
    need("vector stager + scatter mode", g, lambda r, cv, e: "vector stager" in e and "scatter mode" in e)
    # every prologue with and without the SE gate (1x1), and on both stagers
    for pro in range(5):
        for gate in (False, True):
            need(f"1x1 prologue {pro}, gate {gate}", g, lambda r, cv, e, pro=pro, gate=gate: r["pro"] == pro and r["gate"] == gate and r["k"] == 1)
        for stager in ("vector stager", "scalar stager"):
            need(f"prologue {pro} on the {stager}", g, lambda r, cv, e, pro=pro, stager=stager: r["pro"] == pro and stager in e)
    # the halo with zero padding applied after each prologue (3x3), generic and pc (thin and not)
    for pro in (1, 2, 3, 4):
        need(f"3x3 prologue {pro}", g, lambda r, cv, e, pro=pro: r["pro"] == pro and r["k"] == 3)
    for thin in (False, True):
        need(f"3x3 ReLU prologue, thin {thin}", "PC", lambda r, cv, e, thin=thin: r["pro"] == 3 and r["k"] == 3 and cv.args[6] == thin)
    # a ragged last m-tile on each BM; a K tail and K < one chunk for each chunk depth a kernel has
    for table, bms in ((g, (32, 64, 128)), ("PC", (32, 64, 128)), ("DMA_RING", (64, 128, 192, 256, 320)), ("QUAD", (128, 256))):
        for bm in bms:
            need(f"ragged last m-tile, BM {bm}", table, lambda r, cv, e, bm=bm: cv.BM == bm and cv.ragged_m)
    for table, kchs, short in ((g, (64, 16, 8), (64, 16, 8)), ("PC", (32, 4, 8), (4, 8)), ("DMA_RING", (32, 16), (16,)), ("QUAD", (32, 16), (16,))):
        for kch in kchs:
            need(f"K tail, KCH {kch}", table, lambda r, cv, e, kch=kch: cv.KCH == kch and "K tail" in e)
        for kch in short:
            need(f"K < one chunk, KCH {kch}", table, lambda r, cv, e, kch=kch: cv.KCH == kch and "K < one chunk" in e)
    # SiLU beyond the exp range on both 1x1 stagers and under the 3x3 halo
    for what in ("vector stager", "scalar stager", "partial last tile row"):
        need(f"SiLU beyond the exp range + {what}", g, lambda r, cv, e, what=what: "SiLU beyond the exp range" in e and what in e)
    # stride 2 with TF-SAME pads on an odd and an even size
    for odd in (0, 1):
        need(f"stride 2, W % 2 == {odd}", g, lambda r, cv, e, odd=odd: r["s"] == 2 and r["W"] % 2 == odd)
    # the K split of the ring kernels at 8 splits, and the generic rule A without a cap
    for table in ("DMA_RING", "QUAD"):
        need("8 splits", table, lambda r, cv, e: cv.splits == 8)
    need("rule A, no cap", g, lambda r, cv, e: cv.split_rule == "A" and not cv.split_cap8 and not cv.split_cap_half)
    # statistics of the finished rows: STATS with a residual and with an accumulate on every kernel's direct epilogues and reduce tails
    for table in (g, "PC", "DMA_RING", "QUAD"):
        for what in ("residual", "beta"):
            need(f"statistics + {what}, no K split", table, lambda r, cv, e, what=what: "statistics" in e and what in e and cv.splits == 1)
    for epi in ("transposed epilogue", "scalar epilogue"):
        for table in (g, "PC"):
            need(f"statistics + residual or accumulate, {epi}", table, lambda r, cv, e, epi=epi: "statistics" in e and ("residual" in e or "beta" in e) and epi in e)
    for table in (g, "DMA_RING", "QUAD"):
        need("statistics + residual in the reduce tail", table, lambda r, cv, e: "reduce tail: statistics" in e and "reduce tail: residual" in e)
    # the stage depth of the ring and quad kernels on both sides of its threshold: K = 32 (16-channel stages) and K = 33 (32-channel)
    for table in ("DMA_RING", "QUAD"):
        need("K = 32 on 16-channel stages", table, lambda r, cv, e: r["C1"] == CD.DMA_K32_MIN and not cv.k32)
        need("K = 33 on 32-channel stages", table, lambda r, cv, e: r["C1"] == CD.DMA_K32_MIN + 1 and cv.k32)
    missing = [w for w, ok in want if not ok]
    assert not missing, missing


def test_declined_rows_name_the_links_that_decline():
    for r in T.TABLES["DECLINED"]:
        cv = _cv(r)
        assert (r["dma"] or r["q4"]) and cv.declined and cv.declined[0] in ("q4", "dma (flagged)"), (T.rid(r), cv.declined)


# ---------------------------------------------------------------------------------------------------------------------------------
# production plans
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan_conv_records(which):
    import s2lc_amd  # noqa: F401
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet
    from s2lc_amd.modules.prithvi import MaskedAutoencoderViT
    from s2lc_amd.modules.prithvi_segmentation import PrithviSegmentationNet, PrithviSegmentationNetConfig
    from s2lc_amd.utils import _prithvi_model_args, load_untrained_prithvi

    if which == "unet":         # the b5 U-Net at 13 x 256 x 256, batch 32
        plan = EfficientnetUnet(EfficientNetConfig("b5", 13, 4, class_distribution=[0.25] * 4))._make_plan(32, 256, 256, True)
    elif which == "mae":        # Prithvi-100M MAE pre-training, batch 64, mask 0.75
        plan = load_untrained_prithvi(1)._make_plan(64, True, 0.75, True)
    else:                       # Prithvi segmentation fine-tuning, batch 16, frozen / unfrozen backbone
        bb = MaskedAutoencoderViT(**_prithvi_model_args(1), _decoder=False, _flat=False)
        plan = PrithviSegmentationNet(PrithviSegmentationNetConfig(1, 4, 256, 1, 0.1, which == "seg_frozen"), backbone=bb)._make_plan(16, True, 0.0, True)
    return tuple(f for prog in (plan.fwd, plan.bwd) for kind, f in prog.ops if kind == "CONV")


def _as_row(f):
    """a plan's CONV record as a table row (the tables' conventions are asserted: 3x3 stride 1 pads 1, stride 2 pads TF-SAME, ...)"""
    has = lambda k: f.get(k) is not None     # noqa: E731
    flags = f.get("_flags", 0)
    assert not flags & (CD.FLAG_BF16 | CD.FLAG_SPLIT) and not f.get("X1_BF16", 0)
    r = T.R(f["B"], f["C1"], f["H"], f["W"], f["M"], None, C2=f["C2"], k=f["KH"], s=f["STRIDE"], pro=f["PRO1"], pro2=f["PRO2"], gate=has("GATE1"),
            bias=has("BIAS"), stats=has("STATS"), beta=f["BETA"], res=has("RES"), resg=bool(flags & CD.FLAG_RES_GELU_GRAD), scratch=has("SCRATCH"),
            yc=f["YC"] if (f["MODE"] == 0 and f["YC"] != f["M"]) else None, mode=f["MODE"], dma=bool(flags & CD.FLAG_DMA), q4=bool(flags & CD.FLAG_Q4),
            prod=True)
    rec = T.record(r)
    assert f["KH"] == f["KW"] and all(rec[k] == f[k] for k in ("HO", "WO", "PAD_T", "PAD_L", "PRO2")) and rec["NREP"] == max(f.get("NREP", 1), 1), f
    assert f["W_ST"] == (f["M"] + 127) // 128 * 128 and f["W_SM"] == 1 and f["FLIP"] == 0
    return r


def _prod_key(r):
    """what a PROD row must share with the plan record it stands for: instantiation, edges and the map geometry"""
    return (_cv(r).inst, T.row_edges(r), r["H"], r["W"], r["k"], r["s"], r["mode"])


@pytest.mark.parametrize("which", ["unet", "mae", "seg_frozen", "seg_unfrozen"])
def test_every_production_conv_record_has_a_prod_row_with_its_instantiation_and_edges(which):
    have = {_prod_key(r) for r in T.TABLES["PROD"]}
    recs = _plan_conv_records(which)
    assert recs
    missing = {T.rid(r): (k[0], sorted(k[1])) for r in map(_as_row, recs) for k in [_prod_key(r)] if k not in have}
    assert not missing, f"{which}: {len(missing)} CONV records without a PROD row of the same instantiation, edges and map size, e.g. {list(missing.items())[:3]}"


def test_prod_rows_are_all_needed():
    """a PROD row stands for at least one record of a production plan (nothing stale in the table)"""
    used = {_prod_key(_as_row(f)) for which in ("unet", "mae", "seg_frozen", "seg_unfrozen") for f in _plan_conv_records(which)}
    stale = [T.rid(r) for r in T.TABLES["PROD"] if _prod_key(r) not in used]
    assert not stale, stale


# ---------------------------------------------------------------------------------------------------------------------------------
# the older CONV rows of tests/test_ops_gpu.py: their family pins must be what the restated launcher takes
# ---------------------------------------------------------------------------------------------------------------------------------
def _params(fn):
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
    return mark.args[1]


def older_conv_rows():
    """the f32 CONV cases of tests/test_ops_gpu.py as table rows, as their test functions hand them to _conv_case"""
    from tests import test_ops_gpu as O

    def flagged(want):
        return dict(dma=want in (3, 4), q4=want == 4)       # _conv_case: FLAG_DMA for the ring kernel, FLAG_Q4 | FLAG_DMA for the quad kernel
    rows = []
    for B, C1, H, W, M, bias, beta, want in _params(O.test_conv1x1_times_gelu_grad_of_res):
        rows.append(T.R(B, C1, H, W, M, want, bias=bias, beta=beta, resg=True, scratch=C1 >= 1024, **flagged(want)))
    for B, C1, H, W, M, pro, gate in _params(O.test_conv1x1):
        rows.append(T.R(B, C1, H, W, M, 0, pro=pro, gate=gate, bias=M == 4, stats=M != 4))
    for B, C1, C2, H, W, M, pro1, pro2 in _params(O.test_conv3x3):
        rows.append(T.R(B, C1, H, W, M, 0, C2=C2, k=3, pro=pro1, pro2=pro2, bias=True, stats=True))
    for B, C1, H, W, M, pro, bias, stats, beta, want in O.CONV1X1_PC:
        rows.append(T.R(B, C1, H, W, M, want, pro=pro, bias=bias, stats=stats, beta=beta, **flagged(want)))
    for fn, want in ((O.test_conv1x1_dma_ring, 3), (O.test_conv1x1_quad, 4)):
        for B, C1, H, W, M, bias, stats, beta, res, scratch in _params(fn):
            rows.append(T.R(B, C1, H, W, M, want, bias=bias, stats=stats, beta=beta, res=res, scratch=scratch, **flagged(want)))
    for B, C1, C2, H, W, M, pro, beta, want in O.CONV3X3_PC:
        rows.append(T.R(B, C1, H, W, M, want, C2=C2, k=3, pro=pro, bias=True, stats=beta == 0, beta=beta, **flagged(want)))
    for C, H, W in _params(O.test_stem_conv_tf_same_stride2):
        rows.append(T.R(2, C, H, W, 48, 0, k=3, s=2, stats=True))
    for B, Cin, Cout, H, W, pro in _params(O.test_conv_transpose_scatter):
        rows.append(T.R(B, Cin, H, W, 4 * Cout, 0, pro=pro, bias=True, mode=1))
    for (beta,) in [(b,) for b in _params(O.test_conv_dgrad_3x3_flip)]:
        rows.append(T.R(2, 64, 12, 12, 24, 0, k=3, beta=beta))
    rows += [T.R(2, 144, 10, 10, 24, 0, beta=1), T.R(2, 64, 6, 10, 24, 0, mode=2)]       # test_conv_dgrad_1x1_and_gather
    split_k = [m for m in O.test_conv_1x1_split_k.pytestmark if m.name == "parametrize" and m.args[0].startswith("B,")][0].args[1]
    for B, C, M, H, stats, beta, bias in split_k:                                          # (its f32 half)
        rows.append(T.R(B, C, H, H, M, 0, pro=CD.PRO_SILU, stats=stats, beta=beta, bias=bias, scratch=True))
    B, C, H = O._big()      # the > 2 GiB cases: test_conv3x3_reads_past_2gib, test_convt_dgrad_gather_reads_past_2gib, ..._straddling_tiles_past_2gib
    rows += [T.R(B, C, H, H, 8, 0, k=3), T.R(B, 4 * C, H // 2, H // 2, 8, 0, mode=2), T.R(15, 768, 220, 222, 8, 0)]
    return rows


def test_family_pins_of_the_older_conv_rows_match_dispatch():
    rows = older_conv_rows()
    assert len(rows) >= 75
    wrong = [(T.rid(r), r["fam"], _cv(r).inst) for r in rows if _cv(r).family != r["fam"]]
    assert not wrong, wrong
    old, new = {_cv(r).inst for r in rows}, {_cv(r).inst for r in _rows()}
    print(f"older CONV rows: {len(rows)} rows reach {len(old & reachable())} of {len(reachable())} instantiations; the new tables reach {len(new & reachable())}")
    assert old <= new
