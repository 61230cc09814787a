"""GPU: `s2k_classmap_distance` (csrc/distance.hip) against its numpy restatement (tests/distance_ref.py), and what is built on it:
`classmap.distance_transform` / `boundary_band` / `fill_nearest`, `metrics.DistanceBinnedMetrics`,
`GpuTilePipeline.ignore_label_boundaries_within` and `TilePredictor.evaluate_by_distance`.  Integer work with one exact answer - the
nearest site is canonical - so every comparison is `torch.equal`, and every call is made twice and must repeat itself bit for bit.

Shapes straddle the wave, the 64 columns of a column-pass workgroup (`classmap.EDT_COLS`), the rows a row-pass workgroup walks
(`classmap.EDT_ROWS`) and the 256 pixels its threads take at a time.  Inputs: uniform random classes with 3 % of the pixels out of
range, blob maps (the 5 x 7-pixel cells with 10 % salt and pepper of tests/test_components_gpu.py), sparse random sites, and structured
cases (no site, every pixel a site, one site in each corner - the pruned search's worst case -, a full site row, a full site column, two
sites that tie along whole lines).  That the blob and sparse maps hold large distances and many ties is asserted on the restatement, so
that a passing run cannot have skipped the search or the tie rule."""
import functools

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import classmap
from s2lc_amd import predict as P
from s2lc_amd.metrics import DistanceBinnedMetrics, SegMetrics
from tests import classmap_ref as C
from tests import distance_ref as R
from tests.test_components_gpu import _blob_pipe, blob, equal, tensor, uniform
from tests.test_predict_gpu import BANDS, Pointwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TC, TR = classmap.EDT_COLS, classmap.EDT_ROWS
SHAPES = [(1, 1), (1, TC + 1), (TR + 1, 1), (TR - 1, TC - 1), (TR, TC), (TR + 1, TC + 1), (3, 63), (3, 64), (3, 65), (3, 255), (3, 256),
          (3, 257), (3 * TR + 1, 3 * TC + 1)]
BIG, WIDE = (6 * TR + 1, 3 * TC + 1), (4 * TR + 1, 4 * TC + 1)      # 49 x 193 and 33 x 257
KS = [1, 2, 4, 9, 32]
CONN = [4, 8]


# ---- runners ------------------------------------------------------------------------------------------------------------------------------
def run(m, K, to, conn, exclude=(), dtype=torch.int64, src_lut=None, other=None, edges2=None, hist=None):
    """one s2k_classmap_distance call over the numpy maps `m` [M, H, W]: (dist2, nearest), both prefilled so that a pixel the call
    skipped shows"""
    src = tensor(m, dtype)
    before = src.clone()
    eb = classmap.class_bits(exclude, K, "exclude")
    mode, sites = classmap.check_sites(to, K, eb)
    work = torch.empty(src.shape, dtype=torch.int16, device=DEV)
    dist2 = torch.full(src.shape, -7, dtype=torch.int32, device=DEV)
    nearest = torch.full(src.shape, -7, dtype=torch.int32, device=DEV)
    classmap.launch_distance(src, K, mode, sites, conn, eb, work, dist2, nearest, src_lut=src_lut, other=other, edges=edges2, hist=hist)
    assert torch.equal(src, before)
    return dist2, nearest


def check(m, K, to, conn, exclude=(), dtype=torch.int64, cls=None, src_lut=None):
    """dist2 and nearest against the restatement, and a second call against the first; returns the restatement's pair"""
    m = np.asarray(m)
    m = m[None] if m.ndim == 2 else m
    got = run(m, K, to, conn, exclude, dtype, src_lut)
    again = run(m, K, to, conn, exclude, dtype, src_lut)
    want = R.transform(m if cls is None else cls, K, to, conn, exclude)
    assert equal(got[0], want[0]) and equal(got[1], want[1]), (m.shape, K, to, conn, exclude)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    return want


@functools.lru_cache(maxsize=None)
def sparse(seed, H, W, M=1):
    """class 0 with class 1 drawn at 0.4 % of the pixels"""
    rng = np.random.default_rng([seed, H, W, M])
    m = (rng.random((M, H, W)) < 0.004).astype(np.int64)
    m.setflags(write=False)
    return m


# ---- dist2 and nearest --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_uniform_maps_of_every_shape(shape, conn):
    K = 4
    m = uniform(K, *shape)
    check(m, K, "boundary", conn)
    check(m, K, "boundary", conn, (0,))
    check(m, K, (1, 3), conn, (0,))
    check(uniform(K, *shape, wide=False), K, "boundary", conn, (), torch.uint8)


@pytest.mark.parametrize("exclude", [(), (0,)], ids=["all", "not0"])
@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("K", KS)
def test_every_class_count(K, conn, exclude):
    shape = (TR + 1, TC + 1)
    m = uniform(K, *shape)
    want = check(m, K, "boundary", conn, exclude)
    if K - len(exclude) >= 2:
        assert (want[0] == 0).any() and (want[0] > 0).any()
    else:
        assert (want[0] == R.NO_SITE).all() and (want[1] == -1).all()        # one class left: no boundary anywhere
    if K - 1 not in exclude:
        check(m, K, (K - 1,), conn, exclude)
    check(uniform(K, *shape, wide=False), K, "boundary", conn, exclude, torch.uint8)


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", [BIG, WIDE], ids=["49x193", "33x257"])
def test_blob_maps_with_large_distances_and_many_ties(shape, seed, conn):
    K = 4
    m = blob(seed, K, *shape)
    want = check(m, K, "boundary", conn, (0,))
    site = R.sites(m, K, "boundary", conn, (0,))
    finite = want[0][want[0] < R.NO_SITE]
    assert finite.max() >= 16 and R.ties(site) >= 100             # asserted on the restatement: the search went far, the tie rule decided
    other = blob(seed + 7, K, *shape)
    edges2 = R.thresholds((1, 2, 4))
    ref = R.binned(m, other, want[0], K, edges2)
    assert (ref.sum((1, 2)) > 0).all()                              # every bin of edges (1, 2, 4) holds pixels
    for _ in range(2):
        hist = torch.zeros(4, K, K, dtype=torch.int64, device=DEV)
        got = run(m, K, "boundary", conn, (0,), other=tensor(other), edges2=edges2, hist=hist)
        assert equal(hist, ref) and equal(got[0], want[0]) and equal(got[1], want[1])


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", [BIG, WIDE], ids=["49x193", "33x257"])
def test_sparse_sites(shape, seed):
    m = sparse(seed, *shape)
    want = check(m, 2, (1,), 4)
    assert want[0].max() >= 256 and want[0].max() < R.NO_SITE and R.ties(m == 1) >= 20
    check(m, 2, (1,), 8, (0,))


def _structured(name):
    H, W = BIG
    y, x = np.indices((H, W))
    m = np.zeros((H, W), np.int64)
    if name == "checkerboard":
        m = (y + x) % 2
    elif name.startswith("corner"):
        m[{"0": 0, "1": 0, "2": H - 1, "3": H - 1}[name[-1]], {"0": 0, "1": W - 1, "2": 0, "3": W - 1}[name[-1]]] = 1
    elif name == "row":
        m[H // 3] = 1
    elif name == "column":
        m[:, 2 * W // 3] = 1
    elif name == "tie_column":                  # two sites in a row: a whole column of pixels ties
        m[5, 10] = m[5, 20] = 1
    elif name == "tie_row":                     # two sites in a column: a whole row of pixels ties, the upper site wins
        m[10, 70] = m[30, 70] = 1
    else:
        assert name == "no_site"
    return m[None]


STRUCTURED = ["no_site", "checkerboard", "corner0", "corner1", "corner2", "corner3", "row", "column", "tie_column", "tie_row"]


@pytest.mark.parametrize("name", STRUCTURED)
def test_structured_cases(name):
    H, W = BIG
    m = _structured(name)
    want = check(m, 2, (1,), 4)
    if name == "no_site":
        assert (want[0] == R.NO_SITE).all() and (want[1] == -1).all()
        check(m, 2, "boundary", 8)
    elif name == "checkerboard":
        check(m, 2, "boundary", 4)
        assert (R.transform(m, 2, "boundary", 4)[0] == 0).all()     # every pixel a site
    elif name.startswith("corner"):
        assert want[0].max() == (H - 1) ** 2 + (W - 1) ** 2 and len(np.unique(want[1])) == 1
    elif name == "tie_column":
        assert (want[1][0, :, 15] == 5 * W + 10).all() and R.ties(m == 1) == H
    elif name == "tie_row":
        assert (want[1][0, 20] == 10 * W + 70).all() and R.ties(m == 1) == W
    check(m, 2, (1,), 4, (), torch.uint8)


def test_maps_of_a_batch_never_see_each_other():
    K = 4
    H, W = 2 * TR + 1, 2 * TC + 1
    m = np.array(blob(3, K, H, W, M=3))
    m[1] = 2                                                        # the middle map has no site at all
    want = check(m, K, "boundary", 8, (0,))
    assert (want[0][1] == R.NO_SITE).all() and (want[1][1] == -1).all() and (want[0][[0, 2]] < R.NO_SITE).all()
    m[1] = 0
    want = check(m, K, (1, 2), 4)
    assert (want[0][1] == R.NO_SITE).all() and (want[0][[0, 2]] < R.NO_SITE).all()


def test_byte_maps_are_read_through_a_table():
    K = 5
    rng = np.random.default_rng(12)
    lut = rng.integers(0, K, 256).astype(np.int32)
    lut[[7, 200]] = [K + 3, -1]
    codes = blob(10, 256, *BIG, M=2)
    cls = lut[codes].astype(np.int64)
    lut_d = torch.from_numpy(lut).to(DEV)
    for to, conn, exclude in (("boundary", 4, (0,)), ("boundary", 8, ()), ((1, 4), 4, (0,))):
        want = check(codes, K, to, conn, exclude, torch.uint8, cls=cls, src_lut=lut_d)
        assert (want[0] == 0).any() and want[0].max() >= 4
    # the counts read the same table, and `other` as bytes without one
    other = blob(11, K + 2, *BIG, M=2)
    edges2 = [0, 3]
    d2 = R.transform(cls, K, "boundary", 4, (0,))[0]
    hist = torch.zeros(3, K, K, dtype=torch.int64, device=DEV)
    run(codes, K, "boundary", 4, (0,), torch.uint8, lut_d, other=tensor(other, torch.uint8), edges2=edges2, hist=hist)
    assert equal(hist, R.binned(cls, other, d2, K, edges2)) and 0 < int(hist.sum()) < cls.size


# ---- the binned counts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,conn", [(1, 4), (2, 8), (4, 4), (9, 8), (32, 4)])
@pytest.mark.parametrize("edges", [(0,), (0, 1, 2, 1000), (0, 1, 1.5, 2, 3, 4, 6, 1000)], ids=["1", "4", "8"])
def test_binned_counts_are_added_onto_what_is_there(edges, K, conn):
    H, W = 2 * TR + 1, 2 * TC + 1
    m, other = blob(4, K, H, W, M=2), uniform(K, H, W, M=2)
    edges2 = R.thresholds(edges)
    d2 = R.transform(m, K, "boundary", conn, (0,) if K > 1 else ())[0]
    ref = R.binned(m, other, d2, K, edges2)
    assert ref.sum() < m.size                                       # `other` holds pixels out of range: they are not counted
    if K > 2:                                                       # (K = 2 without class 0 is one class: no boundary)
        assert ref[0].sum() > 0 and ref[-1].sum() == (0 if len(edges) > 1 else ref[1].sum())
        if len(edges) > 1:
            assert d2[d2 < R.NO_SITE].max() < edges2[-1]          # the last edge lies beyond every distance
    rng = np.random.default_rng(K)
    before = rng.integers(0, 1 << 40, ref.shape)
    binned = DistanceBinnedMetrics(K, edges, ignore_index=0 if K > 1 else None, connectivity=conn, device=DEV)
    binned.hist.copy_(torch.from_numpy(before))
    seg = SegMetrics(K, device=DEV)
    for n in (1, 2):
        binned.update(tensor(other), tensor(m))
        seg.update(tensor(other), tensor(m))
        assert equal(binned.hist, before + n * ref)
    assert torch.equal(binned.total() - torch.from_numpy(before.sum(0)).to(DEV), seg.hist.view(K, K))
    assert equal(seg.hist.view(K, K), n * C.confusion(m, other, K))
    out = binned.compute()
    assert len(out) == len(edges) + 1 and out[-1]["hi"] == float("inf") and out[0]["pixels"] == int((before + 2 * ref)[0].sum())
    binned.reset()
    assert int(binned.hist.sum()) == 0


def test_maps_are_walked_in_chunks_of_the_workspace(monkeypatch):
    K = 4
    m = blob(12, K, 2 * TR + 1, 2 * TC + 1, M=5)
    other = blob(13, K, 2 * TR + 1, 2 * TC + 1, M=5)
    src = tensor(m)
    whole = classmap.distance_transform(src, K, "boundary", 8, (0,), True)
    monkeypatch.setattr(classmap, "WORKSPACE_BYTES", 2 * 2 * m[0].size + 1)          # two maps to a chunk: 2 + 2 + 1
    assert classmap.maps_per_chunk(*m.shape[1:], 2) == 2
    got = classmap.distance_transform(src, K, "boundary", 8, (0,), True)
    want = R.transform(m, K, "boundary", 8, (0,))
    assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1]) and equal(got[0], want[0]) and equal(got[1], want[1])
    monkeypatch.setattr(classmap, "WORKSPACE_BYTES", 2 * 6 * m[0].size + 1)
    binned = DistanceBinnedMetrics(K, (1, 2), connectivity=8, device=DEV)
    binned.update(tensor(other), src)
    assert equal(binned.hist, R.binned(m, other, want[0], K, [1, 4]))
    assert equal(classmap.boundary_band(src, K, 1.5, 8), R.boundary_band(m, K, 1.5, 8))


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------
def test_distance_transform_shapes_and_targets():
    K = 4
    m = blob(5, K, *WIDE)
    d2 = classmap.distance_transform(tensor(m[0]), K)               # [H, W] in, [H, W] out
    assert d2.shape == WIDE and d2.dtype == torch.int32 and equal(d2, R.transform(m, K)[0][0])
    d2, near = classmap.distance_transform(tensor(m, torch.uint8), K, to=[2, 3], exclude=(0,), return_nearest=True)
    want = R.transform(m, K, (2, 3), 4, (0,))
    assert near.dtype == torch.int32 and equal(d2, want[0]) and equal(near, want[1])
    d2 = classmap.distance_transform(tensor(np.ones((1, 5, 5), np.int64)), K)
    assert (d2 == classmap.NO_SITE).all()


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8], ids=["int64", "uint8"])
@pytest.mark.parametrize("conn", CONN)
def test_boundary_band_and_fill_nearest(conn, dtype):
    K = 4
    m = np.array(uniform(K, *BIG, M=2, wide=dtype == torch.int64))
    m[:, :, :96] = blob(6, K, BIG[0], 96, M=2)                      # blobs on the left, noise with pixels out of range on the right
    src = tensor(m, dtype)
    for distance, ignore in ((0, 0), (1, 0), (2.5, 2), (100, 1)):
        got = classmap.boundary_band(src, K, distance, conn, ignore)
        want = R.boundary_band(m, K, distance, conn, ignore)
        assert got.dtype == dtype and equal(got, want) and (want != m).any() and (want == m).any()
        assert torch.equal(classmap.boundary_band(src, K, distance, conn, ignore), got)
    assert equal(classmap.boundary_band(src[0], K, 1), R.boundary_band(m[0], K, 1))
    if conn == 4:
        for fill in ((0,), (), (0, 1, 3)):
            got = classmap.fill_nearest(src, K, fill)
            want = R.fill_nearest(m, K, fill)
            assert got.dtype == dtype and equal(got, want) and (want != m).any()
            assert ((want >= 0) & (want < K)).all() and not np.isin(want, fill).any()
            assert torch.equal(classmap.fill_nearest(src, K, fill), got)
        none = tensor(np.zeros((2, 9, 9), np.int64), dtype)
        assert torch.equal(classmap.fill_nearest(none, K, (0,)), none)      # nothing to fill from: unchanged


@pytest.mark.parametrize("distance,conn,ignore", [(1, 4, 0), (2.5, 8, 2)])
def test_pipeline_ignores_label_boundaries_within_a_distance(distance, conn, ignore):
    K = 4
    pipe = _blob_pipe()
    before = pipe.lut.cpu().numpy()[pipe.labels.cpu().numpy()].astype(np.int64)
    par = torch.tensor([[0, 3, 5, 0], [2, 64, 96, 0], [1, 10, 20, 0]], dtype=torch.int32)
    y_before = pipe(params=par).y                                   # packs the cached TILE_PREP call over the old tensors
    assert equal(y_before, np.stack([before[t, y:y + 32, x:x + 32] for t, y, x, _ in par.tolist()]))
    old_labels, old_lut = pipe.labels, pipe.lut
    kept = old_labels.clone()
    pipe.ignore_label_boundaries_within(distance, conn, ignore)
    want = R.boundary_band(before, K, distance, conn, ignore)
    assert (want != before).any() and (want != ignore).any()
    assert pipe.labels.dtype == torch.uint8 and equal(pipe.labels, want)
    assert torch.equal(pipe.lut.cpu(), torch.arange(256, dtype=torch.int32))
    assert pipe.labels is not old_labels and pipe.lut is not old_lut and torch.equal(old_labels, kept)      # replaced, not written
    assert equal(pipe(params=par).y, np.stack([want[t, y:y + 32, x:x + 32] for t, y, x, _ in par.tolist()]))     # TILE_PREP's y sees the band
    assert equal(pipe.label_histogram(K, [2, 0]), np.stack([np.bincount(want[t].reshape(-1), minlength=K) for t in (2, 0)]))


def test_predictor_counts_by_distance_to_the_label_boundaries():
    K = 4
    pipe = _blob_pipe()
    pred = P.TilePredictor(Pointwise(K, BANDS), pipe, K, flips=(0, 1), tiles_per_launch=2)
    idx = [1, 2, 2]
    true = pipe.lut.cpu().numpy()[pipe.labels.cpu().numpy()].astype(np.int64)[idx]
    d2 = R.transform(true, K, "boundary", 8, (0,))[0]
    for kw in (dict(), dict(majority=3, iterations=2, min_area=6, connectivity=8)):
        mask = pred.predict(idx, **kw)
        binned = DistanceBinnedMetrics(K, (0, 1, 2), connectivity=8, device=DEV)
        pred.evaluate_by_distance(binned, idx, **kw)
        ref = R.binned(true, mask.cpu().numpy(), d2, K, [0, 1, 4])
        assert equal(binned.hist, ref) and (ref.sum((1, 2)) > 0).all()
        seg = SegMetrics(K, device=DEV)
        pred.evaluate(seg, idx, **kw)
        assert torch.equal(binned.total(), seg.hist.view(K, K)) and int(binned.total().sum()) == true.size
        pred.evaluate_by_distance(binned, idx, **kw)                # accumulates, and repeats itself
        assert equal(binned.hist, 2 * ref)
    assert pipe.labels.dtype == torch.uint8 and int(pipe.lut.max()) == K - 1      # the labels were read through the table, not rewritten
