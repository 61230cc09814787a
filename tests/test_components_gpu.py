"""GPU: `s2k_classmap_components` and `s2k_classmap_sieve` (csrc/components.hip) against their numpy restatement
(tests/components_ref.py), and what is built on them: `classmap.connected_components` / `sieve`,
`TilePredictor.predict / evaluate / render(min_area=...)` and `GpuTilePipeline.ignore_small_label_regions` / `label_components`.
Integer work with one exact answer - labels are canonical - so every comparison is `torch.equal`.

Shapes straddle the tile one workgroup labels in LDS (TH x TW = `classmap.CC_TILE_H` x `CC_TILE_W`): one pixel, one row and one column
that cross a tile edge, one below, at and one above a tile, and maps of 2 x 2, 3 x 2 and 4 x 4 tiles with ragged last tiles.  Inputs:
uniform random classes with 3 % of the pixels out of range; blob maps (the "coarse 5 x 7 cell grid" is read, on purpose, as cells of
5 x 7 PIXELS of one random class, not as 5 x 7 cells per map: small cells put many components across every tile edge and a cell on
every tile corner, which is what the merge has to get right; 10 % salt and pepper on top) whose components cross tile edges and span
several tiles - asserted on the restatement, so that a passing run cannot have skipped the
merge; and structured worst cases (one class, checkerboard, stripes, a serpentine through every row, a square spiral)."""
import functools

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import classmap
from s2lc_amd import predict as P
from s2lc_amd.metrics import SegMetrics
from s2lc_amd.render import overlay
from tests import classmap_ref as C
from tests import components_ref as R
from tests.test_predict_gpu import BANDS, Pointwise, _pipe
from tests.test_predict_gpu import TH as TILE_H
from tests.test_predict_gpu import TW as TILE_W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = classmap.CC_TILE_H, classmap.CC_TILE_W
SHAPES = [(1, 1), (1, TW + 1), (TH + 1, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW - 1), (3 * TH + 1, 3 * TW + 1)]
BIG = SHAPES[-1]
BATCH = (2 * TH + 1, 2 * TW + 1)
KS = [1, 2, 4, 9, 32]
CONN = [4, 8]


# ---- inputs (read-only numpy arrays, made once) ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uniform(K, H, W, M=1, wide=True):
    """seeded uniform random classes, 3 % of the pixels outside [0, K): -1 and K + 2 in an int64 map, 255 in a uint8 one"""
    rng = np.random.default_rng([K, H, W, M])
    m = rng.integers(0, K, (M, H, W))
    out = rng.random((M, H, W)) < 0.03
    m[out] = rng.choice([-1, K + 2], int(out.sum())) if wide else 255
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def blob(seed, K, H, W, M=1):
    """cells of 5 x 7 pixels (the reading chosen on purpose, see the head of the file), each of one random class, then 10 % of the
    pixels redrawn: salt and pepper on blobs"""
    rng = np.random.default_rng([seed, K, H, W, M])
    coarse = rng.integers(0, K, (M, (H + 4) // 5, (W + 6) // 7))
    m = np.ascontiguousarray(coarse[:, np.arange(H) // 5][:, :, np.arange(W) // 7])
    noise = rng.random((M, H, W)) < 0.10
    m[noise] = rng.integers(0, K, int(noise.sum()))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def structured(name):
    """[1, H, W] maps of two classes at the largest shape; each is a worst case of one launch"""
    H, W = BIG
    y, x = np.indices((H, W))
    if name == "one_class":                     # one component of H * W pixels: every tile edge merges, every area add meets one root
        m = np.ones((H, W), np.int64)
    elif name == "checkerboard":                # H * W components at connectivity 4, two at 8
        m = (y + x) % 2
    elif name == "rows":                        # 1-pixel horizontal stripes: every one crosses every vertical tile edge
        m = y % 2
    elif name == "columns":
        m = x % 2
    elif name == "serpentine":                  # one path, one pixel wide, through every row: it crosses every tile edge many times
        m = np.zeros((H, W), np.int64)
        m[0::2] = 1
        m[1::4, W - 1] = 1
        m[3::4, 0] = 1
    else:                                       # a square spiral, one pixel wide, wound inward with one pixel between its turns
        assert name == "spiral"
        m = np.zeros((H, W), np.int64)
        top, left, bottom, right = 0, 0, H - 1, W - 1
        m[top, left:right + 1] = 1
        while True:
            m[top:bottom + 1, right] = 1
            if bottom - top < 2 or right - left < 2:
                break
            m[bottom, left:right + 1] = 1
            top += 2
            if bottom - top < 2:
                break
            m[top:bottom + 1, left] = 1
            right -= 2
            if right - left < 2:
                break
            m[top, left:right + 1] = 1
            bottom -= 2
            left += 2
    m = m[None].astype(np.int64)
    m.setflags(write=False)
    return m


STRUCTURED = ["one_class", "checkerboard", "rows", "columns", "serpentine", "spiral"]


# ---- runners ------------------------------------------------------------------------------------------------------------------------------
def tensor(m, dtype=torch.int64):
    return torch.from_numpy(np.array(m, order="C")).to(dtype).to(DEV).contiguous()


def equal(got, want):
    return torch.equal(got.cpu(), torch.from_numpy(np.array(want)).to(got.dtype))


def label(m, K, conn, exclude=(), dtype=torch.int64, src_lut=None):
    """one s2k_classmap_components call over the numpy maps `m` [M, H, W]: (labels, areas, counts), the status word checked"""
    src = tensor(m, dtype)
    before = src.clone()
    labels = torch.full(src.shape, -7, dtype=torch.int32, device=DEV)
    areas = torch.full(src.shape, -7, dtype=torch.int32, device=DEV)            # the call zeroes what it adds into
    counts = torch.zeros(src.shape[0], K, dtype=torch.int64, device=DEV)
    status = classmap.new_status(DEV)
    classmap.launch_components(src, K, conn, classmap.class_bits(exclude, K, "exclude"), labels, areas, status, counts, src_lut=src_lut)
    assert int(status.item()) == 0 and torch.equal(src, before)
    return labels, areas, counts


def check_labels(m, K, conn, exclude=(), dtype=torch.int64, cls=None, src_lut=None):
    labels, areas, counts = label(m, K, conn, exclude, dtype, src_lut)
    want = R.components(m if cls is None else cls, K, conn, exclude)
    assert equal(labels, want[0]) and equal(areas, want[1]) and equal(counts, want[2]), (np.shape(m), K, conn, exclude)
    return want


def check_sieve(m, K, min_area, conn, iterations=1, fixed=(), to=None, dtype=torch.int64):
    src = tensor(m, dtype)
    before = src.clone()
    got, changed = classmap.sieve(src, K, min_area, conn, iterations, fixed, to, return_changed=True)
    want, steps, cur = m, np.zeros(len(m), np.int64), m
    for _ in range(iterations):
        want = R.sieve(cur, K, min_area, conn, 1, fixed, to)
        steps += C.changed(cur, want)
        cur = want
    assert got.dtype == dtype and got.shape == src.shape and torch.equal(src, before)
    assert equal(got, want), (np.shape(m), K, min_area, conn, iterations, fixed, to)
    assert changed.dtype == torch.int64 and changed.cpu().tolist() == steps.tolist()
    return want


# ---- labels, areas, counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("K", KS)
def test_components_of_uniform_maps_at_every_shape(K, conn):
    for H, W in SHAPES:
        m = uniform(K, H, W)
        check_labels(m, K, conn)
        check_labels(m, K, conn, exclude=(0,))
        m8 = uniform(K, H, W, wide=False)
        check_labels(m8, K, conn, dtype=torch.uint8)
    m = uniform(K, *BATCH, M=3)                                     # three different maps: they never see each other
    assert not np.array_equal(m[0], m[1])
    check_labels(m, K, conn)
    check_labels(uniform(K, *BATCH, M=3, wide=False), K, conn, exclude=(K - 1,), dtype=torch.uint8)


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("K", KS)
def test_components_of_blob_maps_cross_the_tiles(K, conn):
    """the condition on the inputs, from the restatement alone.  The tile corners (TH, TW), (TH, 2 TW), ... fall inside a cell of 5 x 7
    pixels, not between two, so with two or more classes every blob case holds a component that spans four or more tiles: asserted for
    every K >= 2.  Some 76 cells straddle a tile edge; with K = 4, 9 and 32 most of them differ from their neighbours and at least 30
    components cross an edge: asserted.  K = 2 merges them into few large components (7 to 35 cross, printed), K = 1 is one component."""
    for seed in (1, 2, 3, 4):
        m = blob(seed, K, *BIG)
        labels, _, _ = check_labels(m, K, conn)
        span, crossing = R.tile_span(labels[0], TH, TW)
        print(f"blob seed {seed} K {K} connectivity {conn}: most tiles of one component {span}, components crossing an edge {crossing}")
        if K >= 2:
            assert span >= 4
        if K >= 4:
            assert crossing >= 30
    check_labels(blob(5, K, *BATCH, M=3), K, conn, exclude=(0,))
    for H, W in SHAPES[:-1]:
        check_labels(blob(6, K, H, W), K, conn)


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("name", STRUCTURED)
def test_components_of_structured_worst_cases(name, conn):
    m = structured(name)
    H, W = BIG
    labels, areas, counts = check_labels(m, 2, conn)
    if name == "one_class":
        assert counts.tolist() == [[0, 1]] and areas[0, 0, 0] == H * W
    elif name == "checkerboard":
        assert counts.sum() == (H * W if conn == 4 else 2)
    elif name == "rows":
        assert counts.sum() == H and areas.max() == W
    elif name == "columns":
        assert counts.sum() == W and areas.max() == H
    elif name == "serpentine":
        assert counts[0, 1] == 1 and areas[0, 0, 0] == (H + 1) // 2 * W + H // 2 and R.tile_span(labels[0], TH, TW)[0] == 16
    else:
        assert counts[0, 1] == 1 and areas[0, 0, 0] > H * W // 2 - H and R.tile_span(labels[0], TH, TW)[0] == 16
    check_labels(m, 2, conn, exclude=(0,))
    check_labels(m, 2, conn, dtype=torch.uint8)


@pytest.mark.parametrize("conn", CONN)
def test_source_table_maps_256_codes_onto_the_classes(conn):
    K = 5
    rng = np.random.default_rng(11)
    lut = rng.integers(0, K, 256).astype(np.int32)
    lut[[7, 200]] = [K + 3, -1]                                     # two codes outside [0, K): unlabelled
    raw = rng.integers(0, 256, (2,) + BATCH)
    coarse = blob(7, 256, *BATCH, M=2)                              # blobs of one CODE, so that components are larger than specks
    for codes in (raw, coarse):
        cls = lut[codes].astype(np.int64)
        check_labels(codes, K, conn, dtype=torch.uint8, cls=cls, src_lut=torch.from_numpy(lut).to(DEV))
        check_labels(codes, K, conn, exclude=(1, 4), dtype=torch.uint8, cls=cls, src_lut=torch.from_numpy(lut).to(DEV))


def test_public_function_returns_what_was_asked_for_and_is_deterministic():
    K = 4
    m = blob(8, K, *BATCH, M=3)
    src = tensor(m)
    want = R.components(m, K, 8, (0,))
    labels = classmap.connected_components(src, K, 8, exclude=(0,))
    assert labels.dtype == torch.int32 and labels.shape == src.shape and equal(labels, want[0])
    l2, areas, counts = classmap.connected_components(src, K, 8, (0,), return_areas=True, return_counts=True)
    assert torch.equal(l2, labels) and areas.dtype == torch.int32 and equal(areas, want[1])
    assert counts.dtype == torch.int64 and counts.shape == (3, K) and equal(counts, want[2])
    l3, c3 = classmap.connected_components(src, K, 8, [0], return_counts=True)
    assert torch.equal(l3, labels) and torch.equal(c3, counts)                   # a second call: bit-identical, canonical labels
    one = classmap.connected_components(src[1].to(torch.uint8), K)
    assert one.shape == src.shape[1:] and equal(one, R.components(m[1], K, 4)[0])
    assert equal(src, m)                                                         # the input is never written


def test_counts_are_added_onto_what_is_there():
    K = 4
    m = blob(9, K, *BATCH, M=2)
    src = tensor(m)
    start = torch.tensor([[5, 0, 1 << 40, 7], [0, 1, 2, 3]], dtype=torch.int64, device=DEV)
    counts, status = start.clone(), classmap.new_status(DEV)
    work = torch.empty(2, *src.shape, dtype=torch.int32, device=DEV)
    classmap.launch_components(src, K, 4, 0, work[0], work[1], status, counts)
    classmap.launch_components(src, K, 8, 0, work[0], work[1], status, counts)
    want = R.components(m, K, 4)[2] + R.components(m, K, 8)[2]
    assert int(status.item()) == 0 and equal(counts, start.cpu().numpy() + want)


# ---- the sieve ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("K", KS)
def test_sieve_is_the_restatement(K, conn):
    H, W = SHAPES[6]
    for m, dtype in ((uniform(K, H, W), torch.int64), (blob(3, K, H, W), torch.uint8)):
        for min_area in (1, 2, 8, H * W + 1):
            for to in (None, K - 1):
                for fixed in ((), (0,)):
                    for iterations in (1, 2):
                        want = check_sieve(m, K, min_area, conn, iterations, fixed, to, dtype)
                        if min_area == 1:
                            assert np.array_equal(want, m)              # nothing is below one pixel: the input comes back
    for H, W in SHAPES[:6]:
        check_sieve(uniform(K, H, W), K, 2, conn, 2)
        check_sieve(uniform(K, H, W, wide=False), K, 8, conn, 1, (0,), 0, torch.uint8)
    check_sieve(blob(4, K, *BATCH, M=3), K, 8, conn, 2)


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_sieve_of_blob_maps_relabels_hundreds_and_keeps_some(seed, conn):
    """the condition on the inputs, from the restatement alone: with min_area = 8 at least 100 components are relabelled and at least
    one is kept"""
    K = 4
    m = blob(seed, K, *BIG)
    _, (relabelled, no_donor, kept) = R.sieve(m, K, 8, conn, stats=True)
    print(f"blob seed {seed} connectivity {conn}: relabelled {relabelled}, small without a donor {no_donor}, kept {kept}")
    assert relabelled >= 100 and kept >= 1
    check_sieve(m, K, 8, conn)
    check_sieve(m, K, 8, conn, 2, (0,))
    check_sieve(m, K, 8, conn, 1, (), 0)
    check_sieve(m, K, 8, conn, 2, (0,), 0, torch.uint8)


@pytest.mark.parametrize("name", STRUCTURED)
def test_sieve_of_structured_worst_cases(name):
    m = structured(name)
    H, W = BIG
    for conn in CONN:
        check_sieve(m, 2, 8, conn)
        check_sieve(m, 2, H * W + 1, conn, 2)
        check_sieve(m, 2, W + 1, conn, 1, (1,), 0)


def test_sieve_reads_byte_labels_through_a_table_and_is_deterministic():
    K = 5
    rng = np.random.default_rng(12)
    lut = rng.integers(0, K, 256).astype(np.int32)
    lut[[7, 200]] = [K + 3, 255]
    codes = blob(10, 256, *BATCH, M=2)
    cls = lut[codes].astype(np.int64)
    src = tensor(codes, torch.uint8)
    lut_d = torch.from_numpy(lut).to(DEV)
    for to, fixed in ((-1, 0), (0, 1)):
        want = R.sieve(cls, K, 8, 8, 2, (0,) if fixed else (), None if to < 0 else to)
        got = classmap.run_sieve(src, K, 8, 8, 2, fixed, to, src_lut=lut_d)
        assert got.dtype == torch.uint8 and equal(got, want) and (want != cls).any()
        assert torch.equal(classmap.run_sieve(src, K, 8, 8, 2, fixed, to, src_lut=lut_d), got)       # a second call: bit-identical
    assert equal(src, codes)


def test_changed_and_hist_are_added_onto_what_is_there():
    K, conn = 4, 4
    H, W = BATCH
    index = [2, 0, 2, 1, 2]                                         # permuted and repeated
    m = blob(11, K, H, W, M=len(index))
    rng = np.random.default_rng(K)
    labels = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    lut = rng.integers(0, K, 256).astype(np.int32)
    lut[[0, 9, 77]] = [K, -1, 300]                                  # labels that map outside [0, K) are not counted
    true = lut[labels[index]]
    src = tensor(m)
    before = rng.integers(0, 1 << 40, (K, K))
    hist = torch.from_numpy(before.copy()).to(DEV)
    start = torch.tensor([5, 0, 1 << 40, 1, 2], dtype=torch.int64, device=DEV)
    changed = start.clone()
    last = (torch.from_numpy(labels).to(DEV), torch.tensor(index, dtype=torch.int32, device=DEV), torch.from_numpy(lut).to(DEV), hist)
    total = np.zeros_like(before)
    moved = np.zeros(len(index), np.int64)
    for to, out_dtype in ((-1, torch.int64), (1, torch.uint8)):
        want = R.sieve(m, K, 8, conn, 1, (), None if to < 0 else to)
        got = classmap.run_sieve(src if out_dtype == torch.int64 else src.to(torch.uint8), K, 8, conn, 1, 0, to, changed, last)
        total += C.confusion(true, want, K)
        moved += C.changed(m, want)
        assert equal(got, want) and equal(hist, before + total) and equal(changed, start.cpu().numpy() + moved)
    assert 0 < total.sum() < 2 * true.size and moved.min() > 0
    # two passes: changed sums both, hist counts the final map only
    want1 = R.sieve(m, K, 8, conn)
    want2 = R.sieve(want1, K, 8, conn)
    got = classmap.run_sieve(src, K, 8, conn, 2, 0, -1, changed, last)
    moved += C.changed(m, want1) + C.changed(want1, want2)
    assert equal(got, want2) and equal(hist, before + total + C.confusion(true, want2, K)) and equal(changed, start.cpu().numpy() + moved)


def test_maps_are_walked_in_chunks_of_the_workspace(monkeypatch):
    K = 4
    m = blob(12, K, *BATCH, M=5)
    src = tensor(m)
    whole = classmap.sieve(src, K, 8, 8, 2)
    monkeypatch.setattr(classmap, "WORKSPACE_BYTES", 2 * 16 * m[0].size + 1)         # two maps to a chunk: 2 + 2 + 1
    assert classmap.maps_per_chunk(*BATCH, 16) == 2
    got, changed = classmap.sieve(src, K, 8, 8, 2, return_changed=True)
    assert torch.equal(got, whole) and equal(got, R.sieve(m, K, 8, 8, 2))
    assert changed.cpu().tolist() == (C.changed(m, R.sieve(m, K, 8, 8)) + C.changed(R.sieve(m, K, 8, 8), R.sieve(m, K, 8, 8, 2))).tolist()
    monkeypatch.setattr(classmap, "WORKSPACE_BYTES", 2 * 4 * m[0].size + 1)          # areas nobody asked for: two maps to a chunk
    labels, counts = classmap.connected_components(src, K, 4, return_counts=True)
    want = R.components(m, K, 4)
    assert equal(labels, want[0]) and equal(counts, want[2])


# ---- TilePredictor ------------------------------------------------------------------------------------------------------------------------
def test_predictor_sieves_the_map_it_predicts():
    K = 4
    pipe, model = _pipe(32), Pointwise(K, BANDS)
    pred = P.TilePredictor(model, pipe, K, flips=(0, 1), tiles_per_launch=2)
    idx = [1, 2, 2]
    raw = pred.predict(idx)
    got = pred.predict(idx, min_area=6, connectivity=8)
    assert got.shape == (3, TILE_H, TILE_W) and got.dtype == torch.int64 and got.is_cuda
    assert torch.equal(got, classmap.sieve(raw, K, 6, 8)) and equal(got, R.sieve(raw.cpu().numpy(), K, 6, 8))
    assert not torch.equal(got, raw)                                # a per-pixel model on noise: specks throughout
    both = pred.predict(idx, majority=3, iterations=2, min_area=6)  # the sieve runs after the majority filter
    smooth = pred.predict(idx, majority=3, iterations=2)
    assert torch.equal(both, classmap.sieve(smooth, K, 6)) and equal(both, R.sieve(C.majority(raw.cpu().numpy(), K, 3, iterations=2), K, 6))
    assert torch.equal(pred.predict(idx), raw) and torch.equal(pred.predict(idx, min_area=None, connectivity=8), raw)

    true = pipe.lut.long()[pipe.labels[idx].long()]
    for kw, final in ((dict(min_area=6, connectivity=8), got), (dict(majority=3, iterations=2, min_area=6), both)):
        fused, staged = SegMetrics(K, device=DEV), SegMetrics(K, device=DEV)
        pred.evaluate(fused, idx, **kw)
        staged.update(final, true)
        assert torch.equal(fused.hist, staged.hist) and int(fused.hist.sum()) == 3 * TILE_H * TILE_W
        assert equal(fused.hist.view(K, K), C.confusion(true.cpu().numpy(), final.cpu().numpy(), K))
        pred.evaluate(fused, idx, **kw)                             # accumulates
        assert torch.equal(fused.hist, 2 * staged.hist)
    plain, smooth_only = SegMetrics(K, device=DEV), SegMetrics(K, device=DEV)
    pred.evaluate(plain, idx)                                       # without the new arguments: as before
    pred.evaluate(smooth_only, idx, majority=3, iterations=2)
    assert equal(plain.hist.view(K, K), C.confusion(true.cpu().numpy(), raw.cpu().numpy(), K))
    assert equal(smooth_only.hist.view(K, K), C.confusion(true.cpu().numpy(), smooth.cpu().numpy(), K))

    pal = torch.tensor([[0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=torch.uint8)
    picture = pipe.quicklook(idx, whole_tile=True)
    assert torch.equal(pred.render(idx, pal, min_area=6, connectivity=8), overlay(picture, got, pal, 0.5))
    assert torch.equal(pred.render(idx, pal, 0.25, majority=3, iterations=2, min_area=6), overlay(picture, both, pal, 0.25))


# ---- GpuTilePipeline ----------------------------------------------------------------------------------------------------------------------
def _blob_pipe():
    """the predictor tests' pipeline with label rasters made of blobs of one CNES code (uniform codes leave nothing but specks)"""
    pipe = _pipe(32)
    codes = blob(13, 24, TILE_H, TILE_W, M=pipe.labels.shape[0])
    pipe.load(pipe.raw, torch.from_numpy(np.array(codes)).to(torch.uint8))
    return pipe


@pytest.mark.parametrize("min_area,conn,ignore", [(8, 4, 0), (20, 8, 2)])
def test_pipeline_ignores_small_label_regions_once(min_area, conn, ignore):
    K = 4
    pipe = _blob_pipe()
    before = pipe.lut.cpu().numpy()[pipe.labels.cpu().numpy()].astype(np.int64)
    par = torch.tensor([[0, 3, 5, 0], [2, 64, 96, 0], [1, 10, 20, 0]], dtype=torch.int32)
    y_before = pipe(params=par).y                                   # packs the cached TILE_PREP call over the old tensors
    assert equal(y_before, np.stack([before[t, y:y + 32, x:x + 32] for t, y, x, _ in par.tolist()]))
    assert pipe.label_classes == K
    old_labels, old_lut = pipe.labels, pipe.lut
    kept = old_labels.clone()
    pipe.ignore_small_label_regions(min_area, conn, ignore)
    want, (relabelled, _, stay) = R.sieve(before, K, min_area, conn, 1, (ignore,), ignore, stats=True)
    assert relabelled >= 10 and stay >= 1 and (want != before).any() and (want != ignore).any()
    assert pipe.labels.dtype == torch.uint8 and equal(pipe.labels, want)
    assert torch.equal(pipe.lut.cpu(), torch.arange(256, dtype=torch.int32))
    assert pipe.labels is not old_labels and pipe.lut is not old_lut and torch.equal(old_labels, kept)      # replaced, not written
    assert equal(pipe(params=par).y, np.stack([want[t, y:y + 32, x:x + 32] for t, y, x, _ in par.tolist()]))
    hist = pipe.label_histogram(K, [2, 0])
    assert equal(hist, np.stack([np.bincount(want[t].reshape(-1), minlength=K) for t in (2, 0)]))
    metrics = SegMetrics(K, device=DEV)
    pred = P.TilePredictor(Pointwise(K, BANDS), pipe, K)
    pred.evaluate(metrics, [1])
    assert equal(metrics.hist.view(K, K), C.confusion(want[1], pred.predict([1]).cpu().numpy(), K))


@pytest.mark.parametrize("conn", CONN)
def test_pipeline_counts_label_components_through_the_label_map(conn):
    pipe = _blob_pipe()
    cls = pipe.lut.cpu().numpy()[pipe.labels.cpu().numpy()].astype(np.int64)
    got = pipe.label_components(connectivity=conn)
    assert got.dtype == torch.int64 and got.shape == (3, 4) and equal(got, R.components(cls, 4, conn)[2])
    assert equal(pipe.label_components(3, [2, 0, 2], conn), R.components(cls[[2, 0, 2]], 3, conn)[2])      # class 3 belongs to no region
    assert torch.equal(pipe.label_components(None, None, conn), got)
