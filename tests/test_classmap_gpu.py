"""GPU: `s2k_classmap_filter` (csrc/classmap.hip) against its numpy restatement (tests/classmap_ref.py), and what is built on it:
`classmap.majority_filter` / `boundary_to_ignore`, `TilePredictor.predict / evaluate / render(majority=...)` and
`GpuTilePipeline.ignore_label_boundaries`.  The kernel is integer work with an exact answer: every comparison is `torch.equal`.

Shapes straddle what the kernel's geometry turns on: a wave's strip has `classmap.strip_outputs(size)` = 64 - 2r output columns and a
band `classmap.BAND` = 16 rows; K straddles the dword boundaries of the packed byte counters (4 | 5, 8 | 9) and reaches 32."""
import functools

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import classmap
from s2lc_amd import predict as P
from s2lc_amd.metrics import SegMetrics
from s2lc_amd.render import overlay
from tests import classmap_ref as R
from tests.test_predict_gpu import BANDS, TH, TW, Pointwise, _pipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [3, 5, 7, 15]
KS = [1, 2, 4, 5, 8, 9, 32]
DT = {1: torch.uint8, 8: torch.int64}


def shapes(size):
    """(H, W): widths one below, at and one above the strip's output count and twice it, 1 and 2; heights 1, below `size`, and one
    below, at and one above the band height (and two bands and a row; four and a row: with HIST a workgroup walks four bands)"""
    so, band = classmap.strip_outputs(size), classmap.BAND
    return [(1, so - 1), (size - 1, so), (band - 1, so + 1), (band, 2 * so - 1), (band + 1, 2 * so), (2 * band + 1, 2 * so + 1),
            (band + 1, 1), (band, 2), (1, 1), (band, band), (4 * band + 1, so + 1)]


@functools.lru_cache(maxsize=None)
def case(size, K, H, W, M=1, wide=True):
    """seeded uniform random classes, 3 % of the pixels outside [0, K): -1 and K + 2 in an int64 map, 255 in a uint8 one"""
    rng = np.random.default_rng([size, K, H, W, M])
    m = rng.integers(0, K, (M, H, W))
    out = rng.random((M, H, W)) < 0.03
    m[out] = rng.choice([-1, K + 2], int(out.sum())) if wide else 255
    m.setflags(write=False)
    return m


def run(m, K, size, mode, src_bytes=8, dst_bytes=8, votes=None, fixed=(), ignore=0, changed=None, **kw):
    """one launch over the numpy map `m` [M, H, W]: the output as a torch tensor on the device"""
    src = torch.from_numpy(np.array(m)).to(DT[src_bytes]).to(DEV)
    dst = torch.full(src.shape, 77, dtype=DT[dst_bytes], device=DEV)
    vb = classmap.class_bits(votes, K, "votes") if mode == classmap.MAJORITY else 0
    classmap.launch(src, dst, K, size, mode, vb, classmap.class_bits(fixed, K, "fixed"), ignore, changed=changed, **kw)
    return dst


def equal(got, want):
    return torch.equal(got.cpu(), torch.from_numpy(np.array(want)).to(got.dtype))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("size", SIZES)
def test_majority_and_boundary_are_the_restatement(size, K):
    for H, W in shapes(size):
        m = case(size, K, H, W)
        assert equal(run(m, K, size, classmap.MAJORITY), R.majority(m, K, size)), (H, W)
        for ignore in {0, K - 1}:
            assert equal(run(m, K, size, classmap.BOUNDARY, ignore=ignore), R.boundary(m, K, size, ignore)), (H, W, ignore)
    H, W = shapes(size)[5]
    m = case(size, K, H, W, M=3)                                    # three different maps: they never see each other
    assert not np.array_equal(m[0], m[1])
    assert equal(run(m, K, size, classmap.MAJORITY), R.majority(m, K, size))
    assert equal(run(m, K, size, classmap.BOUNDARY, ignore=K - 1), R.boundary(m, K, size, K - 1))


@pytest.mark.parametrize("K", [2, 5, 32])
@pytest.mark.parametrize("size", SIZES)
def test_random_cases_hold_ties_centre_wins_and_changes(size, K):
    """the coverage condition, on the restatement: a case that cannot tell the tie rules apart pins nothing"""
    for H, W in shapes(size):
        if H * W >= 256:
            tied, centre_wins, changed = R.coverage(case(size, K, H, W), K, size)
            assert tied >= 1 and centre_wins >= 1 and changed >= 1, (H, W, tied, centre_wins, changed)


@pytest.mark.parametrize("dst_bytes", [1, 8])
@pytest.mark.parametrize("src_bytes", [1, 8])
@pytest.mark.parametrize("size", [3, 15])
def test_every_pair_of_element_widths(size, src_bytes, dst_bytes):
    K = 9
    for H, W in shapes(size)[3:6]:
        m = case(size, K, H, W, M=2, wide=src_bytes == 8)
        assert ((m < 0) | (m >= K)).any()
        assert equal(run(m, K, size, classmap.MAJORITY, src_bytes, dst_bytes), R.majority(m, K, size)), (H, W)
        assert equal(run(m, K, size, classmap.BOUNDARY, src_bytes, dst_bytes, ignore=2), R.boundary(m, K, size, 2)), (H, W)


@pytest.mark.parametrize("dst_bytes", [1, 8])
def test_source_table_maps_256_codes_onto_the_classes(dst_bytes):
    K, size = 5, 5
    rng = np.random.default_rng(11)
    lut = rng.integers(0, K, 256).astype(np.int32)                  # about 51 codes per class
    lut[[7, 200]] = [K + 3, 255]                                    # two codes outside [0, K): copied, never voting
    raw = rng.integers(0, 256, (2, 33, 121))
    cls = lut[raw].astype(np.int64)
    lut_d = torch.from_numpy(lut).to(DEV)
    assert equal(run(raw, K, size, classmap.MAJORITY, 1, dst_bytes, src_lut=lut_d), R.majority(cls, K, size))
    assert equal(run(raw, K, size, classmap.BOUNDARY, 1, dst_bytes, ignore=1, src_lut=lut_d), R.boundary(cls, K, size, 1))


@pytest.mark.parametrize("K,votes,fixed", [(5, (1, 2, 3, 4), (0,)), (9, (0, 8), ()), (9, (1, 3, 5, 7), (0, 8)), (32, tuple(range(16, 32)), (3, 31)),
                                           (4, (), ())])
@pytest.mark.parametrize("size", [3, 7])
def test_votes_and_fixed_masks(size, K, votes, fixed):
    H, W = shapes(size)[5]
    m = case(size, K, H, W, M=2)
    want = R.majority(m, K, size, votes, fixed)
    assert equal(run(m, K, size, classmap.MAJORITY, votes=votes, fixed=fixed), want)
    if votes:
        assert (want != m).any() and (want != R.majority(m, K, size)).any()
    else:
        assert np.array_equal(want, m)                              # nobody votes: best == 0 everywhere


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_public_functions_iterate_and_count_changes(dtype):
    K, size = 4, 5
    m = case(size, K, 37, 131, M=3, wide=dtype == torch.int64)
    src = torch.from_numpy(m.copy()).to(dtype).to(DEV)
    got, changed = classmap.majority_filter(src, K, size, iterations=3, return_changed=True)
    want, steps = m, np.zeros(3, np.int64)
    for _ in range(3):
        nxt = R.majority(want, K, size)
        steps += R.changed(want, nxt)
        want = nxt
    assert got.dtype == dtype and got.shape == src.shape and equal(got, want) and equal(src, m)
    assert changed.dtype == torch.int64 and changed.cpu().tolist() == steps.tolist() and steps.min() > 0
    assert equal(classmap.majority_filter(src, K, size, iterations=2), R.majority(m, K, size, iterations=2))
    one = classmap.majority_filter(src[1], K, size, votes=(1, 2, 3), fixed=[0])
    assert one.shape == src.shape[1:] and equal(one, R.majority(m[1], K, size, (1, 2, 3), (0,)))
    band = classmap.boundary_to_ignore(src, K, size, ignore_index=3)
    assert band.dtype == dtype and equal(band, R.boundary(m, K, size, 3))
    assert equal(classmap.boundary_to_ignore(src[2], K), R.boundary(m[2], K, 3, 0))


def test_changed_is_added_onto_what_is_there():
    K, size = 5, 3
    H, W = shapes(size)[5]
    m = case(size, K, H, W, M=3)
    start = torch.tensor([5, 0, 1 << 40], dtype=torch.int64, device=DEV)
    changed = start.clone()
    got = run(m, K, size, classmap.MAJORITY, changed=changed)
    want = R.changed(m, R.majority(m, K, size))
    assert want.min() > 0 and equal(got, R.majority(m, K, size)) and equal(changed, start.cpu().numpy() + want)
    run(m, K, size, classmap.BOUNDARY, changed=changed, ignore=2)
    assert equal(changed, start.cpu().numpy() + want + R.changed(m, R.boundary(m, K, size, 2)))


@pytest.mark.parametrize("K,size", [(4, 3), (9, 5), (32, 15)])
def test_hist_is_the_confusion_of_the_output_against_the_labels(K, size):
    H, W = 4 * classmap.BAND + 1, 2 * classmap.strip_outputs(size) + 1      # a second workgroup with one band of its four
    index = [2, 0, 2, 1, 2]                                         # permuted and repeated
    m = case(size, K, H, W, M=len(index))
    rng = np.random.default_rng(K)
    labels = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    lut = rng.integers(0, K, 256).astype(np.int32)
    lut[[0, 9, 77]] = [K, -1, 300]                                  # labels that map outside [0, K) are not counted
    before = rng.integers(0, 1 << 40, (K, K))
    hist = torch.from_numpy(before.copy()).to(DEV)
    kw = dict(labels=torch.from_numpy(labels).to(DEV), index=torch.tensor(index, dtype=torch.int32, device=DEV),
              lut=torch.from_numpy(lut).to(DEV), hist=hist)
    want = R.majority(m, K, size)
    assert equal(run(m, K, size, classmap.MAJORITY, **kw), want)
    true = lut[labels[index]]
    assert ((true < 0) | (true >= K)).any() and ((want < 0) | (want >= K)).any()
    count = R.confusion(true, want, K)
    assert 0 < count.sum() < true.size and equal(hist, before + count)
    band = R.boundary(m, K, size, 0)
    assert equal(run(m, K, size, classmap.BOUNDARY, 8, 1, **kw), band) and equal(hist, before + count + R.confusion(true, band, K))


# ---- TilePredictor --------------------------------------------------------------------------------------------------------------------
def test_predictor_filters_the_map_it_predicts():
    K = 4
    pipe, model = _pipe(32), Pointwise(K, BANDS)
    pred = P.TilePredictor(model, pipe, K, flips=(0, 1), tiles_per_launch=2)
    idx = [1, 2, 2]
    raw = pred.predict(idx)
    got = pred.predict(idx, majority=5, iterations=2)
    assert got.shape == (3, TH, TW) and got.dtype == torch.int64 and got.is_cuda
    assert torch.equal(got, classmap.majority_filter(raw, K, 5, iterations=2)) and equal(got, R.majority(raw.cpu().numpy(), K, 5, iterations=2))
    assert not torch.equal(got, raw)                                # a per-pixel model on noise: salt and pepper throughout
    assert torch.equal(pred.predict(idx), raw) and torch.equal(pred.predict(idx, majority=None, iterations=7), raw)

    fused, plain, staged = SegMetrics(K, device=DEV), SegMetrics(K, device=DEV), SegMetrics(K, device=DEV)
    pred.evaluate(fused, idx, majority=5)
    once = R.majority(raw.cpu().numpy(), K, 5)
    true = pipe.lut.cpu().numpy()[pipe.labels.cpu().numpy()[idx]]
    assert equal(fused.hist.view(K, K), R.confusion(true, once, K)) and int(fused.hist.sum()) == 3 * TH * TW
    pred.evaluate(fused, idx, majority=5, iterations=1)             # accumulates
    assert equal(fused.hist.view(K, K), 2 * R.confusion(true, once, K))
    pred.evaluate(plain, idx)                                       # without the new arguments: WINDOW_BLEND's fused count
    staged.update(raw, pipe.lut.long()[pipe.labels[idx].long()])
    assert torch.equal(plain.hist, staged.hist) and not torch.equal(plain.hist, fused.hist)

    pal = torch.tensor([[0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=torch.uint8)
    picture = pipe.quicklook(idx, whole_tile=True)
    assert torch.equal(pred.render(idx, pal), overlay(picture, raw, pal, 0.5))
    assert torch.equal(pred.render(idx, pal, 0.25, majority=5, iterations=2), overlay(picture, got, pal, 0.25))


# ---- GpuTilePipeline.ignore_label_boundaries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,ignore", [(3, 0), (5, 2)])
def test_pipeline_rewrites_its_labels_once(size, ignore):
    K = 4
    pipe = _pipe(32)
    before = pipe.lut.cpu().numpy()[pipe.labels.cpu().numpy()].astype(np.int64)
    par = torch.tensor([[0, 3, 5, 0], [2, 64, 96, 0], [1, 10, 20, 0]], dtype=torch.int32)
    y_before = pipe(params=par).y                                   # packs the cached TILE_PREP call over the old tensors
    assert equal(y_before, np.stack([before[t, y:y + 32, x:x + 32] for t, y, x, _ in par.tolist()]))
    assert pipe.label_classes == K
    pipe.ignore_label_boundaries(size, ignore)
    want = R.boundary(before, K, size, ignore)
    assert (want != before).any() and (want != ignore).any()
    assert pipe.labels.dtype == torch.uint8 and equal(pipe.labels, want)
    assert torch.equal(pipe.lut.cpu(), torch.arange(256, dtype=torch.int32))
    assert equal(pipe(params=par).y, np.stack([want[t, y:y + 32, x:x + 32] for t, y, x, _ in par.tolist()]))
    hist = pipe.label_histogram(K, [2, 0])
    assert equal(hist, np.stack([np.bincount(want[t].reshape(-1), minlength=K) for t in (2, 0)]))
    metrics = SegMetrics(K, device=DEV)
    pred = P.TilePredictor(Pointwise(K, BANDS), pipe, K)
    pred.evaluate(metrics, [1])
    assert equal(metrics.hist.view(K, K), R.confusion(want[1], pred.predict([1]).cpu().numpy(), K))
