"""CPU: `s2k_classmap_components` and `s2k_classmap_sieve` are exported (and the stage table and the ABI version did not move), they
validate every argument on the host before anything is launched, the numpy restatement (tests/components_ref.py) gives the hand-worked
answers of 5 x 5 cases, and `classmap.connected_components` / `sieve`, the `TilePredictor` arguments and
`GpuTilePipeline.ignore_small_label_regions` / `label_components` raise ValueError for bad arguments before they refuse to run off the
GPU.  The entries are never called with valid arguments here: there is no device to launch on."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import _lib, classmap
from s2lc_amd import predict as P
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.metrics import SegMetrics
from s2lc_amd.plan import opdefs as D
from tests import classmap_ref as C
from tests import components_ref as R

ROOT = Path(__file__).resolve().parents[1]
S2K_EINVAL, S2K_EFAULT = -22, -14


def test_entries_are_exported_and_the_stage_table_is_unchanged():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g

    g.build()
    L = _lib.lib()
    so = ctypes.CDLL(str(g.LIB))
    assert hasattr(so, "s2k_classmap_components") and hasattr(so, "s2k_classmap_sieve")
    assert L.s2k_abi_version() == 2 and len(D.OPS) == 55
    assert "components.hip" in g.SOURCES
    hdr = (ROOT / "include" / "s2k.h").read_text()
    assert re.search(r"\bint s2k_classmap_components\s*\(", hdr) and re.search(r"\bint s2k_classmap_sieve\s*\(", hdr)
    assert "#define S2K_ABI_VERSION 2" in hdr
    assert (classmap.CC_TILE_H, classmap.CC_TILE_W) == (16, 64)
    src = (ROOT / "sentinel2-landcover-classification_amd" / "csrc" / "components.hip").read_text()
    assert re.search(r"CC_TILE_H = 16, CC_TILE_W = 64\b", src)      # the two numbers the GPU tests build their shapes from


# ---- host-side validation: valid calls over CPU tensors (never made): M, H, W, K = 2, 8, 8, 4 ---------------------------------------------
I32 = dict(dtype=torch.int32)
CC_GOOD = dict(M=2, H=8, W=8, K=4, connectivity=4, exclude=0b0001, src_bytes=8)
CC_TENSORS = dict(src=torch.zeros(2, 8, 8, dtype=torch.int64), src_lut=None, labels=torch.zeros(2, 8, 8, **I32), areas=torch.zeros(2, 8, 8, **I32),
                  counts=torch.zeros(2, 4, dtype=torch.int64), status=torch.zeros(1, **I32))
SV_GOOD = dict(M=2, H=8, W=8, K=4, min_area=3, fixed=0b0001, to=-1, nsrc=3, src_bytes=8, dst_bytes=8)
SV_TENSORS = dict(src=torch.zeros(2, 8, 8, dtype=torch.int64), src_lut=None, dst=torch.zeros(2, 8, 8, dtype=torch.int64),
                  labels=torch.zeros(2, 8, 8, **I32), areas=torch.zeros(2, 8, 8, **I32), best=torch.zeros(2, 8, 8, dtype=torch.int64),
                  hist_labels=torch.zeros(3, 8, 8, dtype=torch.uint8), index=torch.zeros(2, **I32), lut=torch.zeros(256, **I32),
                  hist=torch.zeros(4, 4, dtype=torch.int64), changed=torch.zeros(2, dtype=torch.int64), status=torch.zeros(1, **I32))
LUT = torch.zeros(256, **I32)


def _components(**change):
    a = {**CC_GOOD, **{k: v for k, v in change.items() if k in CC_GOOD}}
    t = {**CC_TENSORS, **{k: v for k, v in change.items() if k in CC_TENSORS}}
    rc = _lib.classmap_components(t["src"], t["src_lut"], (a["M"], a["H"], a["W"], a["K"]), a["connectivity"], a["exclude"], t["labels"],
                                  t["areas"], t["counts"], t["status"], 0, src_bytes=a["src_bytes"])
    return rc, _lib.lib().s2k_last_error().decode()


def _sieve(**change):
    a = {**SV_GOOD, **{k: v for k, v in change.items() if k in SV_GOOD}}
    t = {**SV_TENSORS, **{k: v for k, v in change.items() if k in SV_TENSORS}}
    rc = _lib.classmap_sieve(t["src"], t["src_lut"], t["dst"], (a["M"], a["H"], a["W"], a["K"]), a["min_area"], a["fixed"], a["to"], t["labels"],
                             t["areas"], t["best"], t["hist_labels"], t["index"], t["lut"], a["nsrc"], t["hist"], t["changed"], t["status"], 0,
                             src_bytes=a["src_bytes"], dst_bytes=a["dst_bytes"])
    return rc, _lib.lib().s2k_last_error().decode()


DIMS_BAD = [dict(M=0), dict(M=-2), dict(H=0), dict(W=0), dict(H=-8), dict(W=-1), dict(H=65536, W=32768), dict(H=1 << 20, W=1 << 20),
            dict(M=1 << 24), dict(M=1 << 10, H=1 << 14, W=1 << 14)]
CC_BAD = [dict(src_bytes=4), dict(src_bytes=0), dict(src_bytes=2), dict(src_lut=LUT), dict(K=0, exclude=0), dict(K=33), dict(K=-1, exclude=0),
          dict(connectivity=0), dict(connectivity=6), dict(connectivity=-4), dict(connectivity=9), dict(exclude=0b10000),
          dict(K=2, exclude=0b100), dict(exclude=0x80000000)] + DIMS_BAD
SV_BAD = [dict(src_bytes=4), dict(src_bytes=0), dict(dst_bytes=2), dict(dst_bytes=16), dict(src_lut=LUT), dict(dst=SV_TENSORS["src"]),
          dict(K=0, fixed=0), dict(K=33), dict(K=-1, fixed=0), dict(fixed=0b10000), dict(K=2, fixed=0b100), dict(fixed=0x80000000),
          dict(min_area=0), dict(min_area=-5), dict(to=4), dict(to=-2), dict(K=2, fixed=0, to=2), dict(best=None),
          dict(hist_labels=None), dict(index=None), dict(lut=None), dict(nsrc=0), dict(nsrc=-1)] + DIMS_BAD


def _ids(cases):
    return [",".join(f"{k}={'t' if isinstance(v, torch.Tensor) else v}" for k, v in b.items()) for b in cases]


@pytest.mark.parametrize("bad", CC_BAD, ids=_ids(CC_BAD))
def test_components_rejects_invalid_arguments_on_the_host(bad):
    rc, msg = _components(**bad)
    assert rc == S2K_EINVAL and msg.startswith("classmap_components: ") and len(msg) > 30, (rc, msg)


@pytest.mark.parametrize("bad", SV_BAD, ids=_ids(SV_BAD))
def test_sieve_rejects_invalid_arguments_on_the_host(bad):
    rc, msg = _sieve(**bad)
    assert rc == S2K_EINVAL and msg.startswith("classmap_sieve: ") and len(msg) > 25, (rc, msg)


@pytest.mark.parametrize("name", ["src", "labels", "areas", "status"])
def test_components_rejects_a_null_required_pointer(name):
    rc, msg = _components(**{name: None})
    assert rc == S2K_EFAULT and msg.startswith("classmap_components: null pointer"), (rc, msg)
    with pytest.raises(_lib.S2kError, match="null pointer"):
        _lib.check(rc)


@pytest.mark.parametrize("name", ["src", "dst", "labels", "areas", "status"])
def test_sieve_rejects_a_null_required_pointer(name):
    rc, msg = _sieve(**{name: None})
    assert rc == S2K_EFAULT and msg.startswith("classmap_sieve: null pointer"), (rc, msg)


def test_best_may_be_null_only_with_a_target_class():
    rc, msg = _sieve(best=None, to=-1)
    assert rc == S2K_EINVAL and "best" in msg


# ---- the restatement against hand-worked 5 x 5 cases -------------------------------------------------------------------------------------
X = -1      # a pixel outside [0, K)


def test_a_diagonal_pair_is_two_components_at_4_and_one_at_8():
    m = np.zeros((5, 5), np.int64)
    m[1, 1] = m[2, 2] = 1
    labels, areas, counts = R.components(m, 2, 4)
    want = np.zeros((5, 5), np.int64)
    want[1, 1], want[2, 2] = 6, 12
    assert np.array_equal(labels, want) and counts.tolist() == [[1, 2]]
    assert areas[0, 0] == 23 and areas[1, 1] == 1 and areas[2, 2] == 1 and areas.sum() == 25 and np.count_nonzero(areas) == 3
    labels, areas, counts = R.components(m, 2, 8)
    want[2, 2] = 6
    assert np.array_equal(labels, want) and counts.tolist() == [[1, 1]] and areas[1, 1] == 2 and areas[2, 2] == 0
    # the sieve sees what the labels see: two specks of one pixel at 4, one patch of two at 8
    assert np.array_equal(R.sieve(m, 2, 2, 4), np.zeros((5, 5), np.int64))
    assert np.array_equal(R.sieve(m, 2, 2, 8), m)
    # excluded classes are unlabelled: the background leaves, the specks stay
    labels, areas, counts = R.components(m, 2, 4, exclude=(0,))
    assert labels[1, 1] == 6 and labels[2, 2] == 12 and (labels[m == 0] == -1).all() and counts.tolist() == [[0, 2]]


TIE = np.array([[1, 1, 3, 2, 2],
                [1, 1, X, 2, 2],
                [X, X, X, X, X],
                [X, X, X, X, X],
                [X, X, X, X, X]])


def test_two_donors_of_equal_area_tie_to_the_lower_root():
    got = R.sieve(TIE, 4, 2)                    # the 3 is small; its donors, the 1s (root 0) and the 2s (root 3), have four pixels each
    want = TIE.copy()
    want[0, 2] = 1
    assert np.array_equal(got, want)
    # min_area = 5: all three are small, and all relabelling is simultaneous - the 3 takes the 1s' class of the INPUT map while the 1s
    # and the 2s, whose only donor it is, take its class
    want = np.array([[3, 3, 1, 3, 3], [3, 3, X, 3, 3]] + [[X] * 5] * 3)
    out, (relabelled, no_donor, kept) = R.sieve(TIE, 4, 5, stats=True)
    assert np.array_equal(out, want) and (relabelled, no_donor, kept) == (3, 0, 0)
    assert C.changed(TIE, out).tolist() == [9]


def test_a_donor_at_the_minimum_area_beats_a_small_one_with_a_lower_root():
    m = np.array([[1, 3, 2, 2, 2],
                  [X, X, 2, 2, X]] + [[X] * 5] * 3)
    # min_area = 5: the 3 lies between the 1 (root 0, one pixel: small) and the 2s (root 2, five pixels: at the minimum) -> 2;
    # the 1's only donor is the 3 -> 3
    want = np.array([[3, 2, 2, 2, 2],
                     [X, X, 2, 2, X]] + [[X] * 5] * 3)
    assert np.array_equal(R.sieve(m, 4, 5), want)
    # min_area = 6: nobody is at the minimum; the larger area still wins over the lower root, and the 2s take the 3
    want = np.array([[3, 2, 3, 3, 3],
                     [X, X, 3, 3, X]] + [[X] * 5] * 3)
    assert np.array_equal(R.sieve(m, 4, 6), want)
    # a second pass over that output: the same three components with the classes 3 | 2 | 3, all small again - they swap back
    twice = np.array([[2, 3, 2, 2, 2],
                      [X, X, 2, 2, X]] + [[X] * 5] * 3)
    assert np.array_equal(R.sieve(m, 4, 6, iterations=2), twice)


G = np.array([[1, X, 0, 0, 0],
              [X, X, 0, 2, 0],
              [7, X, 0, 0, 0],
              [X, X, X, X, X],
              [3, 3, X, 5, 2]])


def test_no_donor_fixed_to_and_pixels_out_of_range():
    K = 4
    labels, areas, counts = R.components(G, K)
    assert (labels[(G < 0) | (G >= K)] == -1).all() and labels[2, 0] == -1 and labels[4, 3] == -1      # 7 and 5 are no classes of K = 4
    assert labels[0, 0] == 0 and labels[1, 3] == 8 and labels[4, 0] == labels[4, 1] == 20 and labels[4, 4] == 24
    assert (labels[G == 0] == 2).all() and areas[0, 2] == 8 and areas[4, 0] == 2 and areas[4, 1] == 0
    assert counts.tolist() == [[1, 1, 2, 1]]
    # the donor rule: only the 2 inside the zeros has a neighbour across a pixel edge; the 1, the 3s and the corner 2 touch nothing
    # but pixels out of range, which donate nothing - they stay
    want = G.copy()
    want[1, 3] = 0
    out, (relabelled, no_donor, kept) = R.sieve(G, K, 3, stats=True)
    assert np.array_equal(out, want) and (relabelled, no_donor, kept) == (1, 3, 1)
    assert np.array_equal(R.sieve(G, K, 3, connectivity=8), want)                   # donors are edge neighbours whatever the connectivity
    assert np.array_equal(R.sieve(G, K, 3, fixed=(2,)), G)                          # a fixed class is never small
    # `to`: every small component goes there, donor or not; pixels out of range are copied
    to0 = np.array([[0, X, 0, 0, 0], [X, X, 0, 0, 0], [7, X, 0, 0, 0], [X, X, X, X, X], [0, 0, X, 5, 0]])
    assert np.array_equal(R.sieve(G, K, 3, to=0), to0)
    keep3 = to0.copy()
    keep3[4, :2] = 3
    assert np.array_equal(R.sieve(G, K, 3, to=0, fixed=(3,)), keep3)
    assert np.array_equal(R.sieve(G, K, 2, to=1, fixed=(0,)), np.where((G == 2), 1, G))      # the pair of 3s is at the minimum now
    assert np.array_equal(R.sieve(G, K, 1), G) and np.array_equal(R.sieve(G, K, 1, to=0), G)  # nothing is below one pixel
    assert C.confusion(G, to0, K).tolist() == [[8, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0], [2, 0, 0, 0]]


def test_maps_of_a_batch_never_see_each_other():
    rng = np.random.default_rng(5)
    m = rng.integers(0, 3, (3, 5, 5))
    labels, areas, counts = R.components(m, 3, 8)
    for i in range(3):
        one = R.components(m[i], 3, 8)
        assert np.array_equal(labels[i], one[0]) and np.array_equal(areas[i], one[1]) and np.array_equal(counts[i], one[2][0])
        assert np.array_equal(R.sieve(m, 3, 4)[i], R.sieve(m[i], 3, 4))
    assert R.tile_span(np.zeros((5, 5), np.int64), 2, 2) == (9, 1)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def _cpu_pipe(labels=True, label_map="cnes-multiclass"):
    p = GpuTilePipeline([0.1] * 4, [0.2] * 4, random_crop_size=8, label_map=label_map, device="cpu")
    g = torch.Generator().manual_seed(0)
    p.load(torch.randint(-100, 100, (3, 4, 16, 16), generator=g, dtype=torch.int32).to(torch.int16),
           torch.randint(0, 24, (3, 16, 16), generator=g, dtype=torch.int32).to(torch.uint8) if labels else None)
    return p


def test_validators_raise_before_the_gpu_refusal():
    m = torch.zeros(2, 8, 8, dtype=torch.int64)
    cc, sv = classmap.connected_components, classmap.sieve
    pipe = _cpu_pipe()
    pred = P.TilePredictor(lambda x: x, pipe, 4)
    metrics = SegMetrics(4, device="cpu")
    pal = torch.zeros(4, 3, dtype=torch.uint8)
    bad = [
        lambda: cc(m, 0), lambda: cc(m, 33), lambda: cc(m, 4.0), lambda: cc(m, 4, connectivity=6), lambda: cc(m, 4, connectivity=True),
        lambda: cc(m, 4, connectivity=8.0), lambda: cc(m, 4, exclude=(4,)), lambda: cc(m, 4, exclude=(-1,)), lambda: cc(m.float(), 4),
        lambda: cc(m.int(), 4), lambda: cc(m[0, 0], 4), lambda: cc(m[:0], 4), lambda: cc(m.numpy(), 4),
        lambda: sv(m, 4, 0), lambda: sv(m, 4, -3), lambda: sv(m, 4, 2.0), lambda: sv(m, 4, True), lambda: sv(m, 4, 1 << 31), lambda: sv(m, 0, 2),
        lambda: sv(m, 33, 2), lambda: sv(m, 4, 2, connectivity=5), lambda: sv(m, 4, 2, iterations=0), lambda: sv(m, 4, 2, iterations=1.0),
        lambda: sv(m, 4, 2, fixed=(4,)), lambda: sv(m, 4, 2, to=4), lambda: sv(m, 4, 2, to=-1), lambda: sv(m, 4, 2, to=1.0),
        lambda: sv(m.double(), 4, 2), lambda: sv(m[0, 0], 4, 2), lambda: sv(m[:0], 4, 2),
        lambda: pred.predict(min_area=0), lambda: pred.predict(min_area=2.5), lambda: pred.predict(min_area=4, connectivity=6),
        lambda: pred.predict(majority=4, min_area=4), lambda: pred.evaluate(metrics, min_area=0), lambda: pred.evaluate(metrics, min_area=4, connectivity=2),
        lambda: pred.evaluate(metrics, [7], min_area=4), lambda: pred.render([0], pal, min_area=-1), lambda: pred.render([0], pal, min_area=4, connectivity=3),
        lambda: P.TilePredictor(lambda x: x, _cpu_pipe(labels=False), 4).evaluate(metrics, min_area=4),
        lambda: pipe.ignore_small_label_regions(0), lambda: pipe.ignore_small_label_regions(4, connectivity=6),
        lambda: pipe.ignore_small_label_regions(4, ignore_index=4), lambda: pipe.ignore_small_label_regions(4, ignore_index=-1),
        lambda: _cpu_pipe(labels=False).ignore_small_label_regions(4),
        lambda: _cpu_pipe(label_map="osm-multiclass").ignore_small_label_regions(4),     # an identity map names 256 classes: beyond 32
        lambda: pipe.label_components(connectivity=5), lambda: pipe.label_components(0), lambda: pipe.label_components(33),
        lambda: pipe.label_components(indices=[3]), lambda: pipe.label_components(indices=[]),
        lambda: _cpu_pipe(labels=False).label_components(), lambda: _cpu_pipe(label_map="osm-multiclass").label_components(),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} did not raise")


def test_the_new_functions_refuse_the_cpu():
    m = torch.zeros(2, 8, 8, dtype=torch.int64)
    pipe = _cpu_pipe()
    pred = P.TilePredictor(lambda x: x, pipe, 4)
    pal = torch.zeros(4, 3, dtype=torch.uint8)
    calls = (lambda: classmap.connected_components(m, 4), lambda: classmap.connected_components(m[0].to(torch.uint8), 32, 8, (0,), True, True),
             lambda: classmap.sieve(m, 4, 8), lambda: classmap.sieve(m.to(torch.uint8), 2, 3, 8, 2, (0,), 1, True),
             lambda: pred.predict(min_area=4), lambda: pred.predict(majority=3, min_area=4, connectivity=8),
             lambda: pred.evaluate(SegMetrics(4, device="cpu"), [0, 2], min_area=4), lambda: pred.render([1], pal, min_area=4),
             lambda: pipe.ignore_small_label_regions(4), lambda: pipe.ignore_small_label_regions(9, 8, 3),
             lambda: pipe.label_components(), lambda: pipe.label_components(4, [0, 2], 8))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert pipe.label_classes == 4 and int(pipe.lut.max()) == 3      # nothing was rewritten
