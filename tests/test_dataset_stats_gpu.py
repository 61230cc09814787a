"""GPU: the dataset-statistics stages TILE_LABEL_HIST and TILE_MOMENTS (csrc/input.hip) as one-record programs through the C ABI
against their numpy restatement (tests/stats_ref.py; the ops have no entry in oracle/ops_ref.py), and `GpuTilePipeline`'s
statistics methods end to end against the reference's stored results (tests/golden/make_golden_stats.py).

Bars.  Integer outputs (HIST, SUMS) are exact.  The f64 outputs derived from SUMS / SDPART - at most a few hundred f64 additions
of positive terms, rounding below 1e-13 - are compared with the float64 restatement at 1e-12 relative.  Against the fixture:
1e-6 relative to the vector's maximum (about eight float32 ulps, 4x the reference's own largest distance from float64).  The
float32 results of `band_mean_std` against float64: one float32 ulp, 2^-23 (an f64-accurate value rounded once)."""
import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd.data import dataset_stats as DS
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan.program import Program
from tests.stats_ref import mean_std_f64, numpy_hist, numpy_moments, rel
from tests.test_ops_gpu import Case

pytestmark = pytest.mark.gpu

TOL = 1e-6


def run_records(c: Case, records) -> torch.Tensor:
    """the records through `_lib.run` over c's arena; returns the arena's bytes afterwards (c.read takes tensors out of them)"""
    from s2lc_amd import _lib

    prog = Program()
    for kind, fields in records:
        prog.add(kind, **fields)
    cpu = torch.zeros(c.arena.top + 256, dtype=torch.uint8)
    for ref, data in c.items.values():
        cpu[ref.off:ref.off + ref.nbytes] = data.contiguous().reshape(-1).view(torch.uint8)
    gpu = cpu.cuda()
    _lib.run(prog.pack(), _lib.Bases().set("WS", gpu), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return gpu.cpu()


# ---- TILE_LABEL_HIST ----------------------------------------------------------------------------------------------------------
def _label_tiles(n, H, W, seed):
    """tile 0 one label throughout, tile 1 coherent patches (waves that agree and waves that do not), the rest random bytes"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, 256, (n, H, W), generator=g, dtype=torch.int32)
    lab[0] = 2
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    lab[1] = (yy // 7 + xx // 19) % 6
    return lab.to(torch.uint8)


def _lut(kind):
    if kind == "k4_skip":       # values 0..6, of which 4..6 fall outside K = 4 and are skipped
        return 4, torch.arange(256, dtype=torch.int32) % 7
    if kind == "k2":
        return 2, torch.arange(256, dtype=torch.int32) % 2
    return 256, torch.arange(256, dtype=torch.int32)


def _hist_case(lab, index, lut, K, win, repeat=1):
    n, H, W = lab.shape
    M = len(index)
    c = Case(3)
    fields = dict(LABELS=c.t("lab", (n, H, W), lab, "u8"), INDEX=c.t("index", (M,), torch.tensor(index), "i32"),
                  LUT=c.t("lut", (256,), lut, "i32"), HIST=c.t("hist", (M, K), torch.zeros(M, K), "i64"),
                  M=M, H=H, W=W, K=K, Y0=win[0], X0=win[1], WH=win[2], WW=win[3], NSRC=n)
    got = c.read(run_records(c, [("TILE_LABEL_HIST", fields)] * repeat), "hist").numpy()
    y0, x0, h, w = win
    want = numpy_hist(lab.numpy()[index][:, y0:y0 + h, x0:x0 + w], K, lut.numpy())
    return got, want


@pytest.mark.parametrize("lut_kind", ["k4_skip", "k2", "k256_identity"])
@pytest.mark.parametrize("win", [(0, 0, 40, 52), (4, 10, 32, 32), (1, 3, 7, 13), (0, 36, 40, 16)],
                         ids=["tile", "aligned_width_unaligned_start", "odd_start_narrow", "right_edge"])
def test_label_hist_equals_bincount(win, lut_kind):
    K, lut = _lut(lut_kind)
    got, want = _hist_case(_label_tiles(4, 40, 52, 1), [3, 0, 3, 1], lut, K, win)
    assert want.sum() > 0 and (lut_kind != "k4_skip" or want.sum() < 4 * win[2] * win[3])
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], got[2])       # the duplicate tile has its own, equal row


def test_label_hist_single_label_tile_512():
    """262,144 hits in one bin (every lane of every wave collides; the count needs more than 16 bits), next to a tile of
    coherent patches"""
    lab = _label_tiles(2, 512, 512, 2)
    K, lut = _lut("k4_skip")
    got, want = _hist_case(lab, [0, 1], lut, K, (0, 0, 512, 512))
    assert want[0].tolist() == [0, 0, 512 * 512, 0]
    assert np.array_equal(got, want)


def test_label_hist_accumulates():
    K, lut = _lut("k4_skip")
    got, want = _hist_case(_label_tiles(4, 40, 52, 1), [3, 0, 3, 1], lut, K, (1, 3, 30, 45), repeat=2)
    assert np.array_equal(got, 2 * want)


# ---- TILE_MOMENTS -------------------------------------------------------------------------------------------------------------
def _moments_inputs(name, M, C, H, W):
    g = torch.Generator().manual_seed(M * 1000 + C * 100 + H)
    if name == "min":
        return torch.full((M, C, H, W), -32768, dtype=torch.int16), list(range(M))
    if name == "alternating":
        raw = torch.full((M, C, H, W), -32768, dtype=torch.int16)
        raw[1::2] = 32767
        return raw, list(range(M))
    nsrc = max(2, M // 4) if name == "duplicates" else M + 1
    raw = torch.randint(-3000, 12000, (nsrc, C, H, W), generator=g, dtype=torch.int32).to(torch.int16)
    index = torch.randint(0, nsrc, (M,), generator=g).tolist() if name == "duplicates" else torch.randperm(nsrc, generator=g)[:M].tolist()
    return raw, index


def _moments_run(raw, index):
    nsrc, C, H, W = raw.shape
    M, NB = len(index), D.moments_blocks(H * W)
    c = Case(4)
    fields = dict(RAW=c.t("raw", (nsrc, C, H, W), raw, "i16"), INDEX=c.t("index", (M,), torch.tensor(index), "i32"),
                  SUMS=c.t("sums", (C, 2), torch.zeros(C, 2), "i64"), SDPART=c.t("sdpart", (C, NB), "nan", "f64"),
                  M=M, C=C, H=H, W=W, NSRC=nsrc, NB=NB)
    img = run_records(c, [("TILE_MOMENTS", fields)])
    return c.read(img, "sums").clone(), c.read(img, "sdpart").clone()


@pytest.mark.parametrize("name,M,C,H,W", [
    ("vector", 5, 3, 8, 12),            # H*W % 8 == 0
    ("scalar_tail", 7, 6, 5, 7),        # H*W = 35: the scalar path and its tail
    ("two_tiles", 2, 13, 16, 20),       # smallest M with a variance
    ("one_tile", 1, 2, 8, 8),           # std exactly 0
    ("duplicates", 37, 6, 16, 20),      # duplicates in INDEX; 4 unrolled groups of 8 tiles + 5
    ("min", 64, 1, 8, 8),               # s2 = 2^36 per position: a 32-bit square accumulator fails
    ("alternating", 64, 1, 8, 8),       # -32768 / 32767 by tile: the largest numerator
    ("vector_two_blocks", 3, 2, 48, 50),    # H*W = 2400 > 2048: a second workgroup per band, its last threads idle
    ("scalar_two_blocks", 9, 1, 45, 47),    # H*W = 2115, odd: the same on the scalar path
])
def test_moments_exact_sums_and_f64_std(name, M, C, H, W):
    raw, index = _moments_inputs(name, M, C, H, W)
    sums, sdpart = _moments_run(raw, index)
    sel = raw.numpy()[index]
    want_sums, want_part, _, HW = numpy_moments(sel)
    assert np.array_equal(sums.numpy(), want_sums)
    assert sdpart.shape == want_part.shape and torch.isfinite(sdpart).all()
    mean = sums[:, 0].double().numpy() / (M * HW)
    std = sdpart.numpy().sum(1) / HW
    want_mean, want_std = mean_std_f64(sel)
    if name in ("one_tile", "min"):
        assert np.array_equal(std, np.zeros(C)) and np.array_equal(want_std, np.zeros(C))
    else:
        e = rel(std, want_std)
        print(f"{name}: std vs float64 {e:.2e}")
        assert e < 1e-12
    assert rel(mean, want_mean) < 1e-12
    assert rel(sdpart.numpy(), want_part) < 1e-12 if want_part.any() else not sdpart.any()
    sums2, sdpart2 = _moments_run(raw, index)      # a second run: bit-identical
    assert torch.equal(sums, sums2) and torch.equal(sdpart.view(torch.int64), sdpart2.view(torch.int64))
    if name == "min":
        assert sums[0].tolist() == [-32768 * 64 * 64, (1 << 30) * 64 * 64]


# ---- GpuTilePipeline end to end -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(golden_dir / "dataset_stats.npz")


def _pipe(fx, name, C):
    pipe = GpuTilePipeline([0.1] * C, [0.05] * C, random_crop_size=8, squeeze_time_dim=True)
    pipe.load(torch.from_numpy(fx[f"{name}.raw"]), torch.from_numpy(fx[f"{name}.labels"]))
    return pipe


@pytest.mark.parametrize("case", [0, 1, 2])
def test_pipeline_statistics_match_the_reference(fx, case):
    N, C, H, W, K = fx["cases"].tolist()[case]
    name = f"n{N}_c{C}_{H}x{W}_k{K}"
    pipe = _pipe(fx, name, C)
    mean, std = pipe.band_mean_std()
    assert mean.dtype == std.dtype == torch.float32 and not mean.is_cuda
    errs = {"mean": rel(mean, fx[f"{name}.mean"]), "std": rel(std, fx[f"{name}.std"])}
    for ign in (False, True):
        prob = pipe.class_probabilities(K, ign)
        w = pipe.sample_weights(prob, ign, window="tile")
        errs[f"prob{int(ign)}"] = rel(prob, fx[f"{name}.prob.ign{int(ign)}"])
        errs[f"weights{int(ign)}"] = rel(w, fx[f"{name}.weights.ign{int(ign)}"])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < TOL for v in errs.values()), errs
    # the statistics feed the constructor they were computed for
    GpuTilePipeline(mean, std, random_crop_size=8).load(torch.from_numpy(fx[f"{name}.raw"]), None)


def test_pipeline_subset_center_window_and_draws(fx):
    N, C, H, W, K = fx["cases"].tolist()[1]          # 37 tiles of 6 x 16 x 20
    name = f"n{N}_c{C}_{H}x{W}_k{K}"
    pipe = _pipe(fx, name, C)
    raw, lab = fx[f"{name}.raw"], fx[f"{name}.labels"]
    subset = [30, 2, 2, 17, 9, 36, 0, 9, 11, 5, 23]      # unsorted, with duplicates
    for pooled in (False, True):
        mean, std = pipe.band_mean_std(indices=subset, pooled=pooled)
        want_mean, want_std = mean_std_f64(raw[subset])
        if pooled:
            want_std = raw[subset].astype(np.float64).transpose(1, 0, 2, 3).reshape(C, -1).std(axis=1, ddof=1)
        assert rel(mean, want_mean) <= 2.0 ** -23 and rel(std, want_std) <= 2.0 ** -23
    # the centre window is TILE_PREP's centre crop
    hist = pipe.label_histogram(K, subset, window="center")
    assert hist.is_cuda and hist.dtype == torch.int64 and hist.shape == (len(subset), K)
    y = pipe(subset, training=False).y.cpu().numpy()
    assert y.shape == (len(subset), 8, 8) and np.array_equal(hist.cpu().numpy(), numpy_hist(y, K))
    assert np.array_equal(pipe.label_histogram(K, subset, window=(4, 6, 8, 8)).cpu().numpy(), hist.cpu().numpy())
    assert np.array_equal(pipe.label_histogram(K, None, "tile").cpu().numpy(), numpy_hist(lab, K))
    for bad in ((0, 0, 17, 8), (-1, 0, 4, 4), (0, 13, 4, 8), "middle"):
        with pytest.raises(ValueError):
            pipe.label_histogram(K, subset, window=bad)
    # more tiles than max_tiles: a host-drawn subset without replacement
    prob = pipe.class_probabilities(K, True, max_tiles=10, generator=torch.Generator().manual_seed(4))
    drawn = torch.randperm(N, generator=torch.Generator().manual_seed(4))[:10].numpy()
    assert torch.equal(prob, DS.probabilities_from_hist(torch.from_numpy(numpy_hist(lab[drawn], K)), True))
    w = pipe.sample_weights(prob, True)
    got = pipe.weighted_indices(w, 64, generator=torch.Generator().manual_seed(6))
    assert got.tolist() == list(torch.utils.data.WeightedRandomSampler(w, 64, True, generator=torch.Generator().manual_seed(6)))
    assert pipe.draw_params(got, training=False).shape == (64, 4)
