"""CPU: the dataset-statistics stage kinds are registered (and no earlier kind moved), the host derivations of
data/dataset_stats.py reproduce the reference's three dataset passes on the stored fixture (tests/golden/make_golden_stats.py),
and the new `GpuTilePipeline` methods validate their arguments and refuse to run off the GPU.

Fixture bar: 1e-6 relative to the vector's maximum - about eight float32 ulps, 4x the reference's own largest distance from a
float64 restatement (2.7e-7, sample weights; see the generator's docstring)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd.data import dataset_stats as DS
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.plan import opdefs as D
from tests.stats_ref import numpy_hist, numpy_moments, rel

ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-6
# the stage kinds as they were numbered before TILE_LABEL_HIST / TILE_MOMENTS were appended
KINDS_BEFORE = ["MEMSET", "AXPY", "WEIGHT_PACK", "CONV", "WGRAD", "WGRAD_FINALIZE", "DWCONV_FWD", "DWCONV_DGRAD", "DWCONV_WGRAD",
                "BN_FINALIZE", "SE_POOL", "SE_FC", "SE_FC_BWD", "SE_BWD_REDUCE", "BN_BWD_REDUCE", "BN_BWD_FINALIZE", "BN_BWD_APPLY",
                "BN_RESIDUAL", "CHANNEL_SUM", "LOSS_FWD", "LOSS_BWD", "ARGMAX", "CHAN_LN_FWD", "CHAN_LN_BWD", "ACT_BWD", "ACT_FWD",
                "ATTN_FWD", "ATTN_BWD", "MAE_MASK_INDEX", "IDS_TO_DEC_IDX", "TOKEN_GATHER", "TOKEN_SCATTER", "PATCHIFY", "MAE_LOSS_FWD",
                "MAE_LOSS_BWD", "TRANSPOSE_CL", "CONFUSION", "DROP_GATE", "TILE_PREP", "SE_BN_SUMS", "SE_BN_COMBINE", "SPACE_TO_DEPTH",
                "UPSAMPLE_ZERO", "SE_FC_WGRAD", "IM2COL"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(golden_dir / "dataset_stats.npz")


def case_names(fx):
    return [f"n{N}_c{C}_{H}x{W}_k{K}" for N, C, H, W, K in fx["cases"].tolist()]


def test_new_kinds_are_appended_and_named_by_the_library():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g
    from s2lc_amd import _lib

    g.build()
    assert D.KIND["IM2COL"] == 45
    assert [D.KIND[k] for k in KINDS_BEFORE] == list(range(1, 46))
    assert D.KIND["TILE_LABEL_HIST"] == 46 and D.KIND["TILE_MOMENTS"] == 47
    L = _lib.lib()
    assert L.s2k_abi_version() == 2
    for name in ("TILE_LABEL_HIST", "TILE_MOMENTS"):
        assert L.s2k_kind_name(D.KIND[name]).decode() == name
        assert name in D.WRITES


def test_launchers_reject_bad_dims_on_the_host():
    """Range checks happen before any launch, so they can be exercised without a GPU."""
    from s2lc_amd import _lib
    from s2lc_amd.plan.program import Program, TRef

    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    t = lambda off, shape, dt: TRef(D.BASE["WS"], off, shape, dt)      # noqa: E731
    hist = dict(LABELS=t(0, (2, 8, 8), "u8"), INDEX=t(256, (1,), "i32"), LUT=t(512, (256,), "i32"), HIST=t(2048, (1, 4), "i64"),
                M=1, H=8, W=8, K=4, Y0=0, X0=0, WH=8, WW=8, NSRC=2)
    for bad in (dict(K=0), dict(K=257), dict(Y0=1), dict(X0=4, WW=5), dict(WH=0), dict(M=0), dict(Y0=-1, WH=4)):
        p = Program()
        p.add("TILE_LABEL_HIST", **{**hist, **bad})
        with pytest.raises(_lib.S2kError, match="tile_label_hist: bad dims"):
            _lib.run(p.pack(), _lib.Bases().set("WS", ws), 0)
    mom = dict(RAW=t(0, (2, 3, 8, 8), "i16"), INDEX=t(4096, (1,), "i32"), SUMS=t(8192, (3, 2), "i64"), SDPART=t(8448, (3, 1), "f64"),
               M=1, C=3, H=8, W=8, NSRC=2, NB=1)
    for bad, msg in ((dict(M=65536), "bad dims"), (dict(M=0), "bad dims"), (dict(NB=2), "NB must be"), (dict(H=1 << 15, W=1 << 15), "bad dims")):
        p = Program()
        p.add("TILE_MOMENTS", **{**mom, **bad})
        with pytest.raises(_lib.S2kError, match="tile_moments: " + msg):
            _lib.run(p.pack(), _lib.Bases().set("WS", ws), 0)


def test_mean_std_from_moments_matches_the_reference(fx):
    for name in case_names(fx):
        raw = fx[f"{name}.raw"]
        sums, part, M, HW = numpy_moments(raw)
        mean, std, pooled = DS.mean_std_from_moments(torch.from_numpy(sums), torch.from_numpy(part), M, HW)
        assert mean.dtype == std.dtype == pooled.dtype == torch.float32
        e_mean, e_std = rel(mean, fx[f"{name}.mean"]), rel(std, fx[f"{name}.std"])
        print(f"{name}: mean {e_mean:.2e} std {e_std:.2e}")
        assert e_mean < TOL and e_std < TOL
        want_pooled = raw.astype(np.float64).transpose(1, 0, 2, 3).reshape(raw.shape[1], -1).std(axis=1, ddof=1)
        assert rel(pooled, want_pooled) < TOL
        assert rel(std, want_pooled) > 1e-4, "the per-position statistic is not the pooled one: the fixture must tell them apart"


def test_mean_std_single_tile_and_unsigned_sum_of_squares():
    raw = np.full((1, 2, 8, 8), -7, dtype=np.int16)
    sums, part, M, HW = numpy_moments(raw)
    mean, std, pooled = DS.mean_std_from_moments(torch.from_numpy(sums), torch.from_numpy(part), M, HW)
    assert mean.tolist() == [-7.0, -7.0] and std.tolist() == [0.0, 0.0] and pooled.tolist() == [0.0, 0.0]
    # 65535 tiles of 512 x 512 pixels, all -32768: the sum of squares is 65535 * 2^48 >= 2^63 and arrives as a negative int64
    M, HW = 65535, 512 * 512
    s1, s2 = -32768 * M * HW, (1 << 30) * M * HW
    assert s2 >= 1 << 63
    sums = torch.tensor([[s1, s2 - (1 << 64)]], dtype=torch.int64)
    mean, _, pooled = DS.mean_std_from_moments(sums, torch.zeros(1, 128, dtype=torch.float64), M, HW)
    assert mean.tolist() == [-32768.0] and pooled.tolist() == [0.0]


@pytest.mark.parametrize("ign", [False, True])
def test_probabilities_and_sample_weights_match_the_reference(fx, ign):
    for name, (N, C, H, W, K) in zip(case_names(fx), fx["cases"].tolist()):
        hist = torch.from_numpy(numpy_hist(fx[f"{name}.labels"], K))
        prob = DS.probabilities_from_hist(hist, ign)
        w = DS.sample_weights_from_hist(hist, prob.tolist(), ign)
        assert prob.dtype == w.dtype == torch.float32 and prob.shape == (K,) and w.shape == (N,)
        e_p, e_w = rel(prob, fx[f"{name}.prob.ign{int(ign)}"]), rel(w, fx[f"{name}.weights.ign{int(ign)}"])
        print(f"{name} ignore={ign}: prob {e_p:.2e} weights {e_w:.2e}")
        assert e_p < TOL and e_w < TOL
        assert (prob[0] == 0) == ign


def test_missing_class_stays_at_its_own_index():
    hist = torch.tensor([[10, 0, 30, 0], [10, 0, 50, 0]])
    assert torch.equal(DS.probabilities_from_hist(hist, False), torch.tensor([0.2, 0.0, 0.8, 0.0]))
    assert torch.equal(DS.probabilities_from_hist(hist, True), torch.tensor([0.0, 0.0, 1.0, 0.0]))


def test_empty_window_gets_weight_zero():
    hist = torch.tensor([[64, 0, 0, 0], [16, 16, 16, 16], [0, 64, 0, 0], [32, 0, 32, 0]])
    w = DS.sample_weights_from_hist(hist, [0.0, 0.5, 0.25, 0.25], ignore_zero_label=True)
    assert w[0] == 0 and torch.isfinite(w).all() and (w[1:] > 0).all()
    assert abs(float(w.double().sum()) - 1.0) < 1e-6
    full = DS.sample_weights_from_hist(hist, [0.25] * 4, ignore_zero_label=False)
    assert (full > 0).sum() == 3 and full[1] == 0      # the tile that matches the global distribution exactly


def test_weighted_indices_equal_the_weighted_random_sampler():
    w = torch.rand(50, generator=torch.Generator().manual_seed(1))
    w[7] = 0
    w = w / w.sum()
    want = list(torch.utils.data.WeightedRandomSampler(w, 200, True, generator=torch.Generator().manual_seed(5)))
    got = DS.weighted_indices(w, 200, torch.Generator().manual_seed(5))
    assert got.dtype == torch.int64 and got.tolist() == want and 7 not in want


def _cpu_pipe(n=3, labels=True):
    p = GpuTilePipeline([0.1] * 3, [0.2] * 3, random_crop_size=8, device="cpu")
    g = torch.Generator().manual_seed(0)
    raw = torch.randint(-100, 100, (n, 3, 16, 16), generator=g, dtype=torch.int32).to(torch.int16)
    lab = torch.randint(0, 4, (n, 16, 16), generator=g, dtype=torch.int32).to(torch.uint8)
    p.load(raw, lab if labels else None)
    return p


def test_more_tiles_than_the_exact_integer_bound_raise():
    p = _cpu_pipe()
    assert DS.MAX_MOMENT_TILES == 65535
    with pytest.raises(ValueError, match="65535"):
        p.band_mean_std(indices=torch.zeros(65536, dtype=torch.int64))


def test_label_methods_raise_without_labels():
    p = _cpu_pipe(labels=False)
    for call in (lambda: p.label_histogram(4), lambda: p.class_probabilities(4, False), lambda: p.sample_weights([0.25] * 4)):
        with pytest.raises(ValueError, match="without labels"):
            call()


def test_indices_are_validated_on_the_host():
    p = _cpu_pipe()
    for bad in ([3], [-1], []):
        with pytest.raises(ValueError, match="out of range"):
            p.label_histogram(4, indices=bad)
        with pytest.raises(ValueError, match="out of range"):
            p.band_mean_std(indices=bad)


def test_every_new_method_refuses_the_cpu():
    p = _cpu_pipe()
    calls = (lambda: p.band_mean_std(), lambda: p.band_mean_std(indices=[2, 0, 2], pooled=True), lambda: p.label_histogram(4),
             lambda: p.label_histogram(4, [1], window="center"), lambda: p.class_probabilities(4, True),
             lambda: p.sample_weights([0.25] * 4), lambda: p.weighted_indices([0.5, 0.25, 0.25], 6))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
