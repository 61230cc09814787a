"""CPU: `s2k_classmap_distance` and `s2k_classmap_distance_workspace` are exported (and the stage table and the ABI version did not
move), the entry validates every argument on the host before anything is launched, the numpy restatement (tests/distance_ref.py) gives
the hand-worked answers of 5 x 5 cases, the bin edges convert as documented, and `classmap.distance_transform` / `boundary_band` /
`fill_nearest`, `GpuTilePipeline.ignore_label_boundaries_within`, `metrics.DistanceBinnedMetrics` and
`TilePredictor.evaluate_by_distance` raise ValueError for bad arguments before they refuse to run off the GPU.  The entry is never called
with valid arguments here: there is no device to launch on."""
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
from s2lc_amd.metrics import DistanceBinnedMetrics
from s2lc_amd.plan import opdefs as D
from tests import distance_ref as R

ROOT = Path(__file__).resolve().parents[1]
S2K_EINVAL, S2K_EFAULT = -22, -14
NO = R.NO_SITE


def test_entries_are_exported_and_the_stage_table_is_unchanged():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g

    g.build()
    L = _lib.lib()
    so = ctypes.CDLL(str(g.LIB))
    assert hasattr(so, "s2k_classmap_distance") and hasattr(so, "s2k_classmap_distance_workspace")
    assert L.s2k_abi_version() == 2 and len(D.OPS) == 55
    assert "distance.hip" in g.SOURCES
    hdr = (ROOT / "include" / "s2k.h").read_text()
    assert re.search(r"\bint s2k_classmap_distance\s*\(", hdr) and re.search(r"\bsize_t s2k_classmap_distance_workspace\s*\(", hdr)
    assert "#define S2K_ABI_VERSION 2" in hdr
    assert _lib.CLASSMAP_DISTANCE_MODES == {"classes": 0, "boundary": 1}
    assert classmap.NO_SITE == 2**31 - 1 == NO
    assert _lib.classmap_distance_workspace(2, 8, 8) == 2 * 8 * 8 * 2 and _lib.classmap_distance_workspace(0, 8, 8) == 0


def test_the_tile_constants_are_the_kernel_file_s():
    src = (ROOT / "sentinel2-landcover-classification_amd" / "csrc" / "distance.hip").read_text()
    cols = re.search(r"constexpr int EDT_COLS = (\d+);", src)
    rows = re.search(r"constexpr int EDT_ROWS = (\d+);", src)
    dim = re.search(r"EDT_MAX_EDGES = (\d+), EDT_MAX_DIM = (\d+);", src)
    assert cols and rows and dim
    assert (classmap.EDT_COLS, classmap.EDT_ROWS) == (int(cols.group(1)), int(rows.group(1)))
    assert (classmap.EDT_MAX_EDGES, classmap.EDT_MAX_DIM) == (int(dim.group(1)), int(dim.group(2))) == (8, 16384)


# ---- host-side validation: a valid call over CPU tensors (never made): M, H, W, K = 2, 8, 8, 4 -------------------------------------------
I32 = dict(dtype=torch.int32)
GOOD = dict(M=2, H=8, W=8, K=4, mode=1, sites=0, connectivity=4, exclude=0b0001, src_bytes=8, other_bytes=8, edges=[1, 4], n_edges=None)
TENSORS = dict(src=torch.zeros(2, 8, 8, dtype=torch.int64), src_lut=None, work=torch.zeros(2, 8, 8, dtype=torch.int16),
               dist2=torch.zeros(2, 8, 8, **I32), nearest=torch.zeros(2, 8, 8, **I32), other=torch.zeros(2, 8, 8, dtype=torch.int64),
               hist=torch.zeros(3, 4, 4, dtype=torch.int64))
LUT = torch.zeros(256, **I32)


def _distance(**change):
    a = {**GOOD, **{k: v for k, v in change.items() if k in GOOD}}
    t = {**TENSORS, **{k: v for k, v in change.items() if k in TENSORS}}
    rc = _lib.classmap_distance(t["src"], t["src_lut"], (a["M"], a["H"], a["W"], a["K"]), a["mode"], a["sites"], a["connectivity"], a["exclude"],
                                t["work"], t["dist2"], t["nearest"], t["other"], a["edges"], t["hist"], 0, src_bytes=a["src_bytes"],
                                other_bytes=a["other_bytes"], n_edges=a["n_edges"])
    return rc, _lib.lib().s2k_last_error().decode()


BAD = [dict(src_bytes=4), dict(src_bytes=0), dict(src_bytes=2), dict(src_lut=LUT), dict(K=0, exclude=0), dict(K=33), dict(K=-1, exclude=0),
       dict(mode=2), dict(mode=-1), dict(connectivity=0), dict(connectivity=6), dict(connectivity=-4), dict(connectivity=9),
       dict(exclude=0b10000), dict(K=2, exclude=0b100), dict(exclude=0x80000000),
       dict(mode=0, sites=0), dict(mode=0, sites=0b10000), dict(mode=0, sites=0b0011), dict(mode=0, sites=0x80000000, exclude=0),
       dict(mode=1, sites=0b0010),
       dict(edges=[]), dict(edges=[1, 4], n_edges=0), dict(edges=[1, 4], n_edges=-1), dict(edges=list(range(9))), dict(edges=[4, 1]),
       dict(edges=[1, 1]), dict(edges=[-1, 2]), dict(edges=[0, 1, 2, 2]), dict(edges=None), dict(other=None), dict(other_bytes=4),
       dict(other_bytes=0),
       dict(M=0), dict(M=-2), dict(H=0), dict(W=0), dict(H=-8), dict(W=-1), dict(H=16385), dict(W=16385), dict(H=65536, W=32768),
       dict(H=1 << 20, W=1 << 20), dict(M=1 << 24), dict(M=1 << 22, H=1 << 14, W=1 << 14), dict(M=1 << 17, W=1 << 14)]


def _ids(cases):
    return [",".join(f"{k}={'t' if isinstance(v, torch.Tensor) else v}" for k, v in b.items()) for b in cases]


@pytest.mark.parametrize("bad", BAD, ids=_ids(BAD))
def test_distance_rejects_invalid_arguments_on_the_host(bad):
    rc, msg = _distance(**bad)
    assert rc == S2K_EINVAL and msg.startswith("classmap_distance: ") and len(msg) > 30, (rc, msg)


@pytest.mark.parametrize("name", ["src", "dist2", "work"])
def test_distance_rejects_a_null_required_pointer(name):
    rc, msg = _distance(**{name: None})
    assert rc == S2K_EFAULT and msg.startswith("classmap_distance: null pointer"), (rc, msg)
    with pytest.raises(_lib.S2kError, match="null pointer"):
        _lib.check(rc)


def test_edges_and_other_are_looked_at_only_with_hist():
    """without `hist` there is no counting: the checks of its operands do not apply, and what is still wrong is still reported"""
    rc, msg = _distance(hist=None, other=None, edges=None, K=33)
    assert rc == S2K_EINVAL and "K = 33" in msg


# ---- the restatement against hand-worked 5 x 5 cases -------------------------------------------------------------------------------------
X = -1      # a pixel outside [0, K)


def test_one_site_in_the_middle():
    m = np.zeros((5, 5), np.int64)
    m[2, 2] = 1
    d2, near = R.transform(m, 2, (1,))
    want = np.array([[8, 5, 4, 5, 8],
                     [5, 2, 1, 2, 5],
                     [4, 1, 0, 1, 4],
                     [5, 2, 1, 2, 5],
                     [8, 5, 4, 5, 8]])
    assert np.array_equal(d2[0], want) and (near == 12).all()
    # thresholds 0, 1, 4 on dist2: the site | its four neighbours | dist2 2 and 4 | dist2 5 and 8
    hist = R.binned(m, m, d2, 2, [0, 1, 4])
    assert hist[:, 0, 0].tolist() == [0, 4, 8, 12] and hist[:, 1, 1].tolist() == [1, 0, 0, 0] and hist.sum() == 25
    other = np.full((5, 5), 1)
    other[0, 0] = 2                                                 # outside [0, 2): not counted
    hist = R.binned(m, other, d2, 2, [4])
    assert hist.tolist() == [[[0, 12], [0, 1]], [[0, 11], [0, 0]]]


def test_equidistant_sites_tie_to_the_smallest_index():
    m = np.zeros((5, 5), np.int64)
    m[0, 1] = m[0, 3] = 1                                           # indices 1 and 3: the whole middle column ties
    d2, near = R.transform(m, 2, (1,))
    assert np.array_equal(d2[0], np.array([1, 0, 1, 0, 1])[None] + (np.arange(5) ** 2)[:, None])
    assert np.array_equal(near[0], np.array([[1, 1, 1, 3, 3]] * 5))
    m = np.zeros((5, 5), np.int64)
    m[1, 2] = m[3, 2] = 1                                           # indices 7 and 17: the whole middle row ties, above wins
    d2, near = R.transform(m, 2, (1,))
    assert np.array_equal(d2[0], np.array([1, 0, 1, 0, 1])[:, None] + ((np.arange(5) - 2) ** 2)[None])
    assert np.array_equal(near[0], np.array([[7] * 5, [7] * 5, [7] * 5, [17] * 5, [17] * 5]))
    m = np.zeros((5, 5), np.int64)
    m[0, 2] = m[2, 0] = 1                                           # indices 2 and 10: the diagonal ties
    d2, near = R.transform(m, 2, (1,))
    assert [d2[0, i, i] for i in range(5)] == [4, 2, 4, 10, 20] and [near[0, i, i] for i in range(5)] == [2] * 5
    assert near[0, 1, 0] == 10 and near[0, 0, 1] == 2 and R.ties(R.sites(m, 2, (1,))) == 5


G = np.array([[1, 1, 2, 2, 0],
              [1, 1, 2, 2, 0],
              [1, 1, 2, 2, 0],
              [1, 1, 2, 2, 0],
              [7, 1, 2, 2, 0]])


def test_a_boundary_between_two_classes_with_an_excluded_class_beside_it():
    K = 3
    site = R.sites(G, K, "boundary", 4, (0,))
    want = np.zeros((5, 5), bool)
    want[:, 1:3] = True                                             # both sides; the 2s beside the excluded 0s are no sites, nor are the 0s
    assert np.array_equal(site[0], want)
    d2, near = R.transform(G, K, "boundary", 4, (0,))
    assert np.array_equal(d2[0], np.array([[1, 0, 0, 1, 4]] * 5))   # every pixel has a distance: the excluded, the 7 out of range
    assert np.array_equal(near[0], np.array([[5 * y + 1, 5 * y + 1, 5 * y + 2, 5 * y + 2, 5 * y + 2] for y in range(5)]))
    # without the exclusion the 0s are a class like any other: columns 3 and 4 are sites too; the 7 still makes no boundary
    site = R.sites(G, K, "boundary", 4)
    want[:, 3:] = True
    assert np.array_equal(site[0], want)
    assert np.array_equal(R.transform(G, K, "boundary", 4)[0][0], np.array([[1, 0, 0, 0, 0]] * 5))
    # the diagonals count at connectivity 8 only
    m = np.ones((5, 5), np.int64)
    m[2, 2] = 2
    d4, d8 = R.transform(m, K, "boundary", 4)[0][0], R.transform(m, K, "boundary", 8)[0][0]
    assert d4[1, 1] == 1 and d8[1, 1] == 0 and d4[2, 1] == 0 and d4[0, 0] == 5 and d8[0, 0] == 2 and (d4 == 0).sum() == 5 and (d8 == 0).sum() == 9
    # the band: the labelled pixels other than class 0 within the distance; the 7 is copied
    assert np.array_equal(R.boundary_band(G, K, 0), np.where(want & (G != 7) & (np.arange(5) < 3)[None], 0, G))
    assert np.array_equal(R.boundary_band(G, K, 1), np.where(G == 7, 7, 0))
    assert np.array_equal(R.boundary_band(G, K, 0.99), R.boundary_band(G, K, 0))


def test_no_site():
    m = np.ones((5, 5), np.int64)
    for to in ("boundary", (0,), (0, 2)):
        d2, near = R.transform(m, 3, to)
        assert (d2 == NO).all() and (near == -1).all()
    d2, near = R.transform(np.array([[0, 1], [X, 5]]), 2, "boundary", 8, (1,))      # one labelled pixel: no boundary
    assert (d2 == NO).all() and (near == -1).all()
    assert R.binned(m, m, R.transform(m, 3)[0], 3, [0, 9])[:, 1, 1].tolist() == [0, 0, 25]      # NO_SITE lands in the last bin
    assert np.array_equal(R.fill_nearest(np.zeros((5, 5), np.int64), 2, (0,)), np.zeros((5, 5)))       # nothing to fill from: unchanged


def test_fill_takes_the_class_of_the_canonical_nearest_pixel():
    m = np.array([[1, X, 0, 9, 2]] * 5)
    assert np.array_equal(R.fill_nearest(m, 3, (0,)), np.array([[1, 1, 1, 2, 2]] * 5))      # the middle ties: the smaller index, the 1
    assert np.array_equal(R.fill_nearest(m, 3, ()), np.array([[1, 1, 0, 0, 2]] * 5))        # only the pixels out of range; 1 and 0 tie at X


def test_maps_of_a_batch_never_see_each_other():
    rng = np.random.default_rng(5)
    m = rng.integers(0, 3, (3, 5, 5))
    m[1] = 2
    d2, near = R.transform(m, 3, "boundary", 8)
    for i in range(3):
        one = R.transform(m[i], 3, "boundary", 8)
        assert np.array_equal(d2[i], one[0][0]) and np.array_equal(near[i], one[1][0])
    assert (d2[1] == NO).all() and (d2[0] < NO).all()


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
def test_edges_are_converted_to_floored_squares_and_must_still_ascend():
    assert classmap.check_edges((0, 1, 1.5, 2)) == [0, 1, 2, 4] == R.thresholds((0, 1, 1.5, 2))
    assert classmap.check_edges((1, 2, 4, 8)) == [1, 4, 16, 64]
    assert classmap.check_edges([2.5]) == [6] and classmap.squared_threshold(0) == 0
    for bad in ((1, 1.2), (), (2, 1), (1, 1), (-1,), (float("inf"),), (float("nan"),), tuple(range(9)), ("a",), (None,), (True,), 3):
        with pytest.raises(ValueError):
            classmap.check_edges(bad)
    with pytest.raises(ValueError, match="ascend"):
        DistanceBinnedMetrics(4, edges=(1, 1.2), device="cpu")
    b = DistanceBinnedMetrics(4, edges=(0, 1, 1.5, 2), ignore_index=None, connectivity=8, device="cpu")
    assert b.thresholds == [0, 1, 2, 4] and tuple(b.hist.shape) == (5, 4, 4) and b.hist.dtype == torch.int64 and b.num_classes == 4
    b.hist[1, 2, 2] = 3
    b.hist[4, 1, 2] = 5
    out = b.compute()
    assert [(o["lo"], o["hi"], o["pixels"]) for o in out] == [(0.0, 0.0, 0), (0.0, 1.0, 3), (1.0, 1.5, 0), (1.5, 2.0, 0), (2.0, float("inf"), 5)]
    assert float(out[1]["accuracy"]) == 1.0 and float(out[4]["accuracy"]) == 0.0 and "iou" in out[0] and "confusion_matrix" in out[0]
    assert b.total().tolist() == b.hist.sum(0).tolist() and int(b.total()[2, 2]) == 3
    b.reset()
    assert int(b.hist.sum()) == 0


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def _cpu_pipe(labels=True, label_map="cnes-multiclass"):
    p = GpuTilePipeline([0.1] * 4, [0.2] * 4, random_crop_size=8, label_map=label_map, device="cpu")
    g = torch.Generator().manual_seed(0)
    p.load(torch.randint(-100, 100, (3, 4, 16, 16), generator=g, dtype=torch.int32).to(torch.int16),
           torch.randint(0, 24, (3, 16, 16), generator=g, dtype=torch.int32).to(torch.uint8) if labels else None)
    return p


def test_validators_raise_before_the_gpu_refusal():
    m = torch.zeros(2, 8, 8, dtype=torch.int64)
    dt, bb, fn = classmap.distance_transform, classmap.boundary_band, classmap.fill_nearest
    pipe = _cpu_pipe()
    pred = P.TilePredictor(lambda x: x, pipe, 4)
    binned = DistanceBinnedMetrics(4, device="cpu")
    new = DistanceBinnedMetrics
    bad = [
        lambda: dt(m, 0), lambda: dt(m, 33), lambda: dt(m, 4.0), lambda: dt(m, 4, to="edges"), lambda: dt(m, 4, to=()), lambda: dt(m, 4, to=(4,)),
        lambda: dt(m, 4, to=(-1,)), lambda: dt(m, 4, to=3), lambda: dt(m, 4, to=(1,), exclude=(1,)), lambda: dt(m, 4, connectivity=6),
        lambda: dt(m, 4, connectivity=True), lambda: dt(m, 4, exclude=(4,)), lambda: dt(m.float(), 4), lambda: dt(m.int(), 4),
        lambda: dt(m[0, 0], 4), lambda: dt(m[:0], 4), lambda: dt(m.numpy(), 4), lambda: dt(torch.zeros(1, 1, 16385, dtype=torch.uint8), 4),
        lambda: bb(m, 4, -1), lambda: bb(m, 4, float("nan")), lambda: bb(m, 4, float("inf")), lambda: bb(m, 4, "2"), lambda: bb(m, 4, True),
        lambda: bb(m, 0, 1), lambda: bb(m, 4, 1, connectivity=5), lambda: bb(m, 4, 1, ignore_index=4), lambda: bb(m, 4, 1, ignore_index=-1),
        lambda: bb(m, 4, 1, ignore_index=1.0), lambda: bb(m.double(), 4, 1), lambda: bb(m[:0], 4, 1),
        lambda: fn(m, 0, ()), lambda: fn(m, 33, ()), lambda: fn(m, 4, (4,)), lambda: fn(m, 4, (0, 1, 2, 3)), lambda: fn(m, 1, (0,)),
        lambda: fn(m.float(), 4, (0,)), lambda: fn(m[0, 0], 4, (0,)),
        lambda: new(0, device="cpu"), lambda: new(33, device="cpu"), lambda: new(4, edges=(), device="cpu"), lambda: new(4, edges=(2, 1), device="cpu"),
        lambda: new(4, edges=range(9), device="cpu"), lambda: new(4, edges=(-1,), device="cpu"), lambda: new(4, ignore_index=4, device="cpu"),
        lambda: new(4, connectivity=6, device="cpu"),
        lambda: binned.update(m, m[:1]), lambda: binned.update(m.int(), m), lambda: binned.update(m, m.to(torch.uint8)),
        lambda: binned.update(m[0], m[0]), lambda: binned.update(m[:0], m[:0]),
        lambda: pipe.ignore_label_boundaries_within(-1), lambda: pipe.ignore_label_boundaries_within(float("nan")),
        lambda: pipe.ignore_label_boundaries_within(2, connectivity=6), lambda: pipe.ignore_label_boundaries_within(2, ignore_index=4),
        lambda: pipe.ignore_label_boundaries_within(2, ignore_index=-1), lambda: _cpu_pipe(labels=False).ignore_label_boundaries_within(2),
        lambda: _cpu_pipe(label_map="osm-multiclass").ignore_label_boundaries_within(2),    # an identity map names 256 classes: beyond 32
        lambda: pred.evaluate_by_distance(DistanceBinnedMetrics(5, device="cpu")), lambda: pred.evaluate_by_distance(binned, [7]),
        lambda: pred.evaluate_by_distance(binned, []), lambda: pred.evaluate_by_distance(binned, majority=4),
        lambda: pred.evaluate_by_distance(binned, min_area=0), lambda: pred.evaluate_by_distance(binned, min_area=4, connectivity=6),
        lambda: P.TilePredictor(lambda x: x, _cpu_pipe(labels=False), 4).evaluate_by_distance(binned),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} did not raise")


def test_the_new_functions_refuse_the_cpu():
    m = torch.zeros(2, 8, 8, dtype=torch.int64)
    pipe = _cpu_pipe()
    pred = P.TilePredictor(lambda x: x, pipe, 4)
    binned = DistanceBinnedMetrics(4, device="cpu")
    calls = (lambda: classmap.distance_transform(m, 4), lambda: classmap.distance_transform(m[0].to(torch.uint8), 32, (0, 31), 8, (1,), True),
             lambda: classmap.boundary_band(m, 4, 2.5), lambda: classmap.boundary_band(m.to(torch.uint8), 2, 0, 8, 1),
             lambda: classmap.fill_nearest(m, 4, (0,)), lambda: classmap.fill_nearest(m[1].to(torch.uint8), 2, ()),
             lambda: binned.update(m, m), lambda: pipe.ignore_label_boundaries_within(2), lambda: pipe.ignore_label_boundaries_within(0, 8, 3),
             lambda: pred.evaluate_by_distance(binned), lambda: pred.evaluate_by_distance(binned, [0, 2], majority=3, min_area=4))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert pipe.label_classes == 4 and int(pipe.lut.max()) == 3 and int(binned.hist.sum()) == 0      # nothing was rewritten or counted
