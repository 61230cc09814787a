"""Coverage of the ViT GPU tables (tests/test_vit_kernels_gpu.py, tests/test_vit_ops_gpu.py), checked without a GPU.
tests/vit_dispatch.py restates which kernel a CHAN_LN_FWD / MAE_LOSS stage runs and where the grid-stride loops of csrc/vit.hip
take a second trip; this file parses csrc/vit.hip for every constant that restatement depends on (and fails when one drifts), and
checks that the tables reach every rows-per-wave count of the LayerNorm row kernel, channel splits 1, uneven and 8, both sides of
each boundary of the dispatch, and the second trip of every loop.  The family column of each row must agree with the restatement
(the GPU test then checks the family the launcher reports)."""
import re
from pathlib import Path

import pytest

from tests import test_vit_kernels_gpu as K
from tests import test_vit_ops_gpu as O
from tests import vit_dispatch as V

CSRC = Path(__file__).resolve().parents[1] / "sentinel2-landcover-classification_amd" / "csrc"


def _src():
    return (CSRC / "vit.hip").read_text()


def _launch_cap(src, kernel):
    """the `std::min<int64_t>(..., CAP)` grid of the hipLaunchKernelGGL line of `kernel`"""
    m = re.search(r"hipLaunchKernelGGL\(" + kernel + r", dim3\(\(unsigned\)std::min<int64_t>\(([^;]*?), (\d+)\)\), dim3\(([^)]*(?:\([^)]*\))?[^)]*)\)", src)
    assert m, f"launch of {kernel} not found in its known form"
    return m.group(1), int(m.group(2)), m.group(3)


def test_row_kernel_constants_match_the_source():
    src = _src()
    assert int(re.search(r"constexpr int LNR_NW = (\d+);", src).group(1)) == V.LNR_NW
    assert int(re.search(r"constexpr int LNR_US = (\d+);", src).group(1)) == V.LNR_US
    assert int(re.search(r'tune_int\("S2K_LN_ROWS", (\d+)\)', src).group(1)) == V.LN_ROWS_DEFAULT
    # the product build ignores the environment: tune_int returns its default outside -DS2K_TUNING
    common = (CSRC / "common.h").read_text()
    assert re.search(r"inline int tune_int\(const char\* name, int dflt\) \{\s*#ifdef S2K_TUNING.*?#else\s*\(void\)name;\s*return dflt;\s*#endif", common, re.S)
    m = re.search(r"if \(!enabled \|\| \(p\.HW & 3\) \|\| p\.HW < (\d+) \|\| p\.HW > \d+ \|\| p\.C < (\d+) \|\| "
                  r"\(!all && \(p\.HW > (\d+) \|\| p\.B >= (\d+)\)\)\) return false;", src)
    assert m, "the limits of ln_rows_geometry are not in their known form"
    assert tuple(int(v) for v in m.groups()) == (V.HW_MIN, V.C_MIN, V.HW_MAX, V.B_LIMIT)
    assert re.search(r"if \(reinterpret_cast<uintptr_t>\(q\) & 15\) return false;", src)
    assert re.search(r"if \(ln_rows_geometry\(p, \{p\.x, p\.y, p\.mr\}\)\)", src)
    assert re.search(r"p\.pgroups = cdiv\(ncol, 64\);\s*p\.qw = cdiv\(ncol, p\.pgroups\);", src) and re.search(r"p\.rw = 64 / p\.qw;", src)
    assert re.search(r"const int rpi = LNR_NW \* p\.rw;\s*int cs = cdiv\((\d+), p\.B \* p\.pgroups\);", src).group(1) == str(V.WG_TARGET)
    assert re.search(r"cs = std::max\(1, std::min\(cs, std::min\((\d+), p\.C / \(rpi \* 2\)\)\)\);", src).group(1) == str(V.CSPLIT_MAX)
    assert re.search(r"const unsigned grid = 8u \* \(unsigned\)\(p\.pgroups \* p\.csplit\) \* \(unsigned\)cdiv\(p\.B, 8\);", src)
    # the launchers report their family
    assert re.search(r"hipLaunchKernelGGL\(chan_ln_fwd_rows_kernel,[^;]*;\s*g_s2k_variant = 8;", src)
    assert len(re.findall(r"mae_loss_rows_kernel<(?:true|false), false>\)[^;]*; g_s2k_variant = 9;", src)) == 2
    assert len(re.findall(r"g_s2k_variant = ", src)) == 3


def test_mae_vec_matches_the_source():
    assert re.search(r"return p\.P % 4 == 0 && p\.W % 4 == 0 && \(reinterpret_cast<uintptr_t>\(p\.x\) & 15\) == 0;", _src())


def test_grid_caps_match_the_source():
    src = _src()
    per = {"256": 256, "64 * LN_NW": 1, "NTHREADS": None}
    for name, kernel in (("chan_ln_fwd", "chan_ln_fwd_kernel"), ("chan_ln_bwd", "chan_ln_bwd_kernel"), ("act_bwd", "act_bwd_kernel"),
                         ("act_fwd", "act_fwd_kernel"), ("token_gather", "token_gather_kernel"), ("token_scatter", "token_scatter_kernel"),
                         ("patchify", "patchify_kernel"), ("ids_to_dec_idx", "ids_to_dec_idx_kernel")):
        items, cap, block = _launch_cap(src, kernel)
        assert cap == V.GRID_CAP[name], f"{kernel}: grid cap {cap}"
        if name == "token_scatter":
            assert items == "cdiv64(nrows, 4)" and V.PER_WG[name] == 4
        elif name.startswith("chan_ln"):
            assert items == "tiles" and V.PER_WG[name] == 1
        else:
            assert items == "cdiv64(n, 256)" and block == "256" and V.PER_WG[name] == per[block]
    assert int(re.search(r"keep > L \|\| L > (\d+)\)", src).group(1)) == V.MASK_INDEX_L_MAX


def _ln_rows():
    """(B, C, HW, aligned, family) of every CHAN_LN_FWD case"""
    for r in K.LN_ROWS:
        yield (*r, True, 8)
    for r in K.LN_TILE:
        yield (*r[:3], not r[3], 0)
    yield (*K.LN_FWD_STRIDE, True, 0)
    for r in O.LN_FWD:
        yield (*r[:3], True, r[4])


def test_every_layernorm_row_is_pinned_to_the_kernel_the_launcher_takes():
    for B, C, HW, aligned, fam in _ln_rows():
        assert V.ln_family(B, C, HW, aligned) == fam, (B, C, HW, aligned, fam)


def test_row_kernel_tables_reach_every_geometry():
    geos = {r[:3]: V.ln_rows(*r[:3]) for r in K.LN_ROWS}
    assert all(g is not None for g in geos.values())
    assert {g.rw for g in geos.values()} == {4, 5, 6, 7, 8}                      # 64 / (HW / 4) for HW 32..64
    assert all(g.pgroups == 1 and g.qw * g.rw <= 64 for g in geos.values())
    splits = {g.csplit for g in geos.values()}
    assert 1 in splits and 8 in splits
    uneven = [(s, g) for s, g in geos.items() if g.uneven]
    assert uneven, "no case with a short last channel range"
    for (B, C, HW), g in uneven:
        assert g.rows_cs * (g.csplit - 1) < C < g.rows_cs * g.csplit
    assert any(g.csplit > 1 and not g.uneven for g in geos.values())
    # the all-channel sums of a split start at its own range and wrap at crot
    for (B, C, HW), g in geos.items():
        if g.csplit > 1:
            step = V.LNR_NW * g.rw * V.LNR_US
            crot = V.cdiv(C, step) * step
            assert (g.csplit - 1) * g.rows_cs + C > crot
    assert geos[(2, 1000, 52)] == V.LnRows(13, 4, 1, 7, 143, 56, True)


def test_both_sides_of_every_dispatch_boundary_are_in_the_tables():
    rows = {(B, C, HW, al): fam for B, C, HW, al, fam in _ln_rows()}
    fam = lambda B, C, HW, al=True: rows[(B, C, HW, al)]          # noqa: E731  (KeyError: the case is missing)
    assert fam(127, 64, 56) == 8 and fam(128, 64, 56) == 0                        # B < 128
    assert fam(17, 64, 32) == 8 and fam(2, 64, 28) == 0                           # HW >= 32, at the smallest C
    assert fam(1, 1024, 64) == 8 and fam(2, 64, 68) == 0                          # HW <= 64
    assert fam(17, 64, 32) == 8 and fam(2, 63, 52) == 0                           # C >= 64
    assert fam(3, 768, 52) == 8 and fam(3, 768, 52, False) == 0                   # 16-byte alignment
    assert any(f == 0 and HW % 4 for (B, C, HW, al), f in rows.items())           # HW % 4 != 0


def test_mae_loss_rows_are_pinned_and_reach_both_kernels():
    fams = set()
    for B, C, T, H, P, TUB, LP, L_OFF, mis, fam in K.MAE:
        assert V.mae_family(P, H, not mis) == fam
        fams.add((fam, P % 4 == 0, mis))
    assert {(9, False, False), (9, True, True), (0, True, False)} <= fams
    assert any(V.cdiv(r[6], 256) > 1 and r[6] > (r[2] // r[5]) * (r[3] // r[4]) ** 2 + r[7] for r in K.MAE)      # two column workgroups, padded tail
    assert any(r[7] == 0 for r in K.MAE)
    for B, C, T, H, P, TUB, norm in O.MAE_LOSS:
        assert V.mae_family(P, H) == 0          # tests/test_vit_ops_gpu.py::test_mae_loss_fwd_bwd pins 0


@pytest.mark.parametrize("kernel,items", [
    ("chan_ln_fwd", K.LN_FWD_STRIDE[0] * V.cdiv(K.LN_FWD_STRIDE[2], 64)),
    ("chan_ln_bwd", K.LN_BWD_STRIDE[0] * V.cdiv(K.LN_BWD_STRIDE[2], 64)),
    ("act_fwd", K.ACT_STRIDE), ("act_bwd", K.ACT_STRIDE),
    ("token_gather", K.GATHER_STRIDE[0] * K.GATHER_STRIDE[1] * K.GATHER_STRIDE[3]),
    ("token_scatter", K.SCATTER_STRIDE[0] * K.SCATTER_STRIDE[1]),
    ("patchify", K.PATCH_STRIDE[0] * K.PATCH_STRIDE[1] * K.PATCH_STRIDE[2] * K.PATCH_STRIDE[3] ** 2),
    ("ids_to_dec_idx", max(r[0] * (1 + r[1]) for r in K.IDS)),
])
def test_grid_stride_cases_take_a_second_trip(kernel, items):
    assert V.trips(kernel, items) >= 2
    if kernel == "chan_ln_bwd":      # every workgroup collects the partials of two or three tiles
        assert items // V.GRID_CAP[kernel] == 2 and items % V.GRID_CAP[kernel]


def test_older_tables_stay_inside_one_trip_or_say_otherwise():
    """what this file claims as new: before, no LayerNorm case exceeded the grid"""
    for r in O.LN_FWD:
        assert V.trips("chan_ln_fwd", r[0] * V.cdiv(r[2], 64)) == 1


def test_mask_index_runs_at_its_limit():
    assert max(r[1] for r in K.MASK_INDEX) == V.MASK_INDEX_L_MAX
    assert any(r[3] and r[1] / r[3] > 50 for r in K.MASK_INDEX)      # heavy ties
