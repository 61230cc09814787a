"""CPU: `s2k_calibration` is exported and declared (and the stage table and the ABI version did not move), the entry validates every
argument on the host before anything is launched, the numpy restatement (tests/calibration_ref.py) gives the hand-worked answers of
small cases, `metrics.calibration_from_sums` derives the restatement's figures from hand-made integer tables, `refine_temperature`
finds the temperature of synthetic logits with a float64 numpy evaluator, and `classmap.confidence`, `metrics.CalibrationMetrics`,
`metrics.fit_temperature`, `TilePredictor.predict_with_confidence` and `evaluate_calibration` raise ValueError for bad arguments before
they refuse to run off the GPU.  The entry is never called with valid arguments here: there is no device to launch on."""
import ctypes
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import _lib, classmap
from s2lc_amd import metrics as MT
from s2lc_amd import predict as P
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.plan import opdefs as D
from tests import calibration_ref as R

ROOT = Path(__file__).resolve().parents[1]
S2K_EINVAL, S2K_EFAULT = -22, -14


def test_the_entry_is_exported_and_the_stage_table_is_unchanged():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g

    g.build()
    L = _lib.lib()
    so = ctypes.CDLL(str(g.LIB))
    assert hasattr(so, "s2k_calibration")
    assert L.s2k_abi_version() == 2 and len(D.OPS) == 55
    assert "calibration.hip" in g.SOURCES
    hdr = (ROOT / "include" / "s2k.h").read_text()
    assert re.search(r"\bint s2k_calibration\s*\(", hdr) and "#define S2K_ABI_VERSION 2" in hdr
    assert _lib.CALIBRATION_MODES == {"probs": 0, "logits": 1} and _lib.CALIBRATION_MEASURES == {"max": 0, "margin": 1}


def test_the_constants_are_the_kernel_file_s():
    src = (ROOT / "sentinel2-landcover-classification_amd" / "csrc" / "calibration.hip").read_text()
    lim = re.search(r"CAL_MAXK = (\d+), CAL_MAX_BINS = (\d+), CAL_MAX_TEMPS = (\d+);", src)
    grid = re.search(r"constexpr int CAL_MAX_GRID = (\d+);", src)
    assert lim and grid and "CAL_ONE = 1048576.0f" in src
    assert (classmap.MAX_CLASSES, classmap.CAL_MAX_BINS, classmap.CAL_MAX_TEMPS) == tuple(int(v) for v in lim.groups()) == (32, 64, 8)
    assert classmap.CAL_MAX_GRID == int(grid.group(1)) and classmap.CAL_ONE == 2 ** 20 == R.ONE


# ---- host-side validation: a valid call over CPU tensors (never made): N, K, P = 2, 4, 64 -------------------------------------------------
I64 = dict(dtype=torch.int64)
GOOD = dict(mode=1, N=2, K=4, P=64, exclude=0b0001, temps=[1.0, 2.0], n_temps=None, bins=15, measure=0, reject_below=0.5, reject_to=0,
            label_bytes=8, pred_bytes=8)
TENSORS = dict(scores=torch.zeros(2, 4, 64), labels=torch.zeros(2, 64, **I64), label_lut=None, conf=torch.zeros(2, 64),
               pred=torch.zeros(2, 64, **I64), hist=torch.zeros(4, 15, 3, **I64), totals=torch.zeros(2, 2, **I64), skipped=torch.zeros(1, **I64))
LUT = torch.zeros(256, dtype=torch.int32)
NO_OUT = dict(conf=None, pred=None, hist=None, totals=None, skipped=None)


def _call(**change):
    a = {**GOOD, **{k: v for k, v in change.items() if k in GOOD}}
    t = {**TENSORS, **{k: v for k, v in change.items() if k in TENSORS}}
    rc = _lib.calibration(t["scores"], a["mode"], t["labels"], t["label_lut"], (a["N"], a["K"], a["P"]), a["exclude"], a["temps"], a["bins"],
                          a["measure"], a["reject_below"], a["reject_to"], t["conf"], t["pred"], t["hist"], t["totals"], t["skipped"], 0,
                          label_bytes=a["label_bytes"], pred_bytes=a["pred_bytes"], n_temps=a["n_temps"])
    return rc, _lib.lib().s2k_last_error().decode()


BAD = [dict(K=0, exclude=0, reject_to=-1), dict(K=33), dict(K=-1, exclude=0, reject_to=-1), dict(bins=0), dict(bins=65), dict(bins=-3),
       dict(temps=[]), dict(temps=[1.0] * 9), dict(temps=[1.0, 2.0], n_temps=0), dict(temps=[1.0, 2.0], n_temps=-1), dict(temps=None),
       dict(temps=[0.0]), dict(temps=[-1.0]), dict(temps=[1.0, float("nan")]), dict(temps=[float("inf")]), dict(temps=[1e-45]),
       dict(mode=0, temps=[2.0]), dict(mode=0, temps=[1.0, 1.0]), dict(mode=2), dict(mode=-1), dict(measure=2), dict(measure=-1),
       dict(label_bytes=4), dict(label_bytes=0), dict(label_bytes=2), dict(pred_bytes=4), dict(pred_bytes=0),
       dict(label_lut=LUT), dict(label_lut=LUT, labels=None, hist=None, totals=None),
       dict(exclude=0b10000), dict(K=2, exclude=0b100, reject_to=1), dict(exclude=0x80000000),
       dict(reject_to=4), dict(reject_to=-2), dict(K=2, exclude=0, reject_to=2),
       dict(labels=None), dict(labels=None, totals=None), dict(labels=None, hist=None), NO_OUT, {**NO_OUT, "labels": None},
       dict(N=0), dict(N=-2), dict(P=0), dict(P=-64), dict(N=1 << 30, P=8), dict(N=4, P=(1 << 31) - 1), dict(N=1 << 16, P=1 << 17)]


def _ids(cases):
    return [",".join(f"{k}={'t' if isinstance(v, torch.Tensor) else v}" for k, v in b.items()) for b in cases]


@pytest.mark.parametrize("bad", BAD, ids=_ids(BAD))
def test_calibration_rejects_invalid_arguments_on_the_host(bad):
    rc, msg = _call(**bad)
    assert rc == S2K_EINVAL and msg.startswith("calibration: ") and len(msg) > 24, (rc, msg)


def test_calibration_rejects_null_scores():
    rc, msg = _call(scores=None)
    assert rc == S2K_EFAULT and msg.startswith("calibration: null pointer"), (rc, msg)
    with pytest.raises(_lib.S2kError, match="null pointer"):
        _lib.check(rc)
    rc, msg = _call(scores=None, K=33)                     # the NULL is reported first
    assert rc == S2K_EFAULT


def test_widths_are_looked_at_only_with_their_tensor():
    """without labels / pred their byte widths mean nothing, and what is still wrong is still reported"""
    rc, msg = _call(labels=None, hist=None, totals=None, label_bytes=3, pred=None, pred_bytes=3, bins=65)
    assert rc == S2K_EINVAL and "bins = 65" in msg


# ---- the restatement against hand-worked cases -------------------------------------------------------------------------------------------
def test_the_restatement_on_a_hand_worked_row():
    nan = float("nan")
    #                 tie 0/1   plain   edge 0.3  one      above 1  NaN first  NaN later  negative max
    s = np.array([[[0.5, 0.1, 0.3, 1.0, 1.5, nan, 0.25, -0.5],
                   [0.5, 0.7, 0.3, 0.0, 0.2, 0.9, nan, -0.6],
                   [0.0, 0.2, 0.3, 0.0, 0.1, 0.1, 0.75, -0.7]]], np.float32)
    a, c, conf = R.confidence_probs(s, 0)
    assert a[0].tolist() == [0, 1, 0, 0, 0, 0, 2, 0]            # the first maximum; a NaN is never chosen over s[0], nor s[0] = NaN replaced
    assert np.array_equal(c[0, :5], np.float32([0.5, 0.7, 0.3, 1.0, 1.5])) and np.isnan(c[0, 5]) and c[0, 6] == 0.75 and c[0, 7] == -0.5
    _, _, margin = R.confidence_probs(s, 1)
    assert margin[0, 0] == 0.0 and margin[0, 1] == np.float32(0.7) - np.float32(0.2) and margin[0, 6] == 0.5 and np.isnan(margin[0, 5])
    cls = np.array([[0, 1, 2, 0, 0, 1, 2, 5]])
    hist, counted, skipped = R.sums(a, c, cls, 3, 10)
    assert counted[0].tolist() == [True, True, True, True, False, False, True, False] and skipped == 2      # 1.5 and NaN; class 5 is no label
    assert hist[0, 5].tolist() == [1, 1, 2 ** 19] and hist[1, 7].tolist() == [1, 1, int(np.rint(np.float32(0.7) * 2 ** 20))]
    assert hist[0, 3].tolist() == [1, 0, int(np.rint(np.float32(0.3) * 2 ** 20))]       # float32 0.3 * 10 = 3.0000001: bin 3
    assert hist[0, 9].tolist() == [1, 1, 2 ** 20] and hist[2, 7, :2].tolist() == [1, 1] and hist[:, :, 0].sum() == 5      # c = 1 lands in the last bin
    hist, counted, skipped = R.sums(a, c, cls, 3, 10, exclude=(0,))
    assert counted[0].tolist() == [False, True, True, False, False, False, True, False] and skipped == 1
    assert R.reject(a, conf, 0.5, 2)[0].tolist() == [0, 1, 2, 0, 0, 0, 2, 2] and R.reject(a, conf, 0.5, -1)[0].tolist() == a[0].tolist()
    one = R.confidence_probs(s[:, :1], 1)
    assert np.array_equal(one[1][0, :5], one[2][0, :5]) and (one[0] == 0).all()      # K = 1: the margin is c itself


def test_the_float64_reference_and_its_tolerances():
    z = np.float32([[[0.0], [math.log(3.0)]]])
    p, nll = R.softmax64(z, 1.0)
    assert np.allclose(p[0, :, 0], [0.25, 0.75], atol=1e-7) and np.allclose(nll[0, :, 0], [math.log(4), math.log(4 / 3)], atol=1e-7)
    assert np.allclose(R.confidence64(z, 1.0, 1), 0.5, atol=1e-7) and np.allclose(R.confidence64(z, 2.0, 0), math.sqrt(3) / (1 + math.sqrt(3)), atol=1e-7)
    assert R.conf_tolerance(1) < R.conf_tolerance(4) < R.conf_tolerance(32) < 6e-6 and R.conf_tolerance(4, 1) > 2 * R.conf_tolerance(4)
    assert 2.0 ** -21 < R.nll_tolerance(4, z, 1.0) < 2e-6 and R.nll_tolerance(4, z, 1.0, probs=True) < 2e-5
    assert abs(R.nll64(np.float32([[[0.25], [0.75]]]), np.array([[1]]), np.array([[True]]), probs=True) - math.log(4 / 3)) < 1e-7
    assert R.nll64(np.float32([[[0.0], [1.0]]]), np.array([[0]]), np.array([[True]]), probs=True) == 128.0


# ---- compute(): the figures from integer tables -----------------------------------------------------------------------------------------
def _table(K, bins, cells):
    h = np.zeros((K, bins, 3), np.int64)
    for (a, b), (n, ok, mean_conf) in cells.items():
        h[a, b] = [n, ok, int(round(mean_conf * R.ONE)) * n]
    return h


TABLES = {
    "empty_bins": (_table(3, 10, {(0, 2): (10, 1, 0.25), (1, 9): (30, 27, 0.95), (2, 9): (10, 10, 1.0), (2, 5): (50, 20, 0.55)}), [100, 37 * R.ONE], 3),
    "single_bin": (_table(2, 1, {(0, 0): (7, 3, 0.6), (1, 0): (5, 5, 0.9)}), [12, 5 * R.ONE + 17], 0),
    "all_in_the_last_bin": (_table(4, 15, {(1, 14): (64, 64, 1.0)}), [64, 0], 0),
    "nothing_counted": (np.zeros((4, 15, 3), np.int64), [0, 0], 9),
}


@pytest.mark.parametrize("name", list(TABLES))
def test_compute_derives_the_restatement_s_figures_from_the_integer_sums(name):
    hist, totals, skipped = TABLES[name]
    got = MT.calibration_from_sums(torch.from_numpy(hist), torch.tensor(totals), skipped)
    want = R.figures(hist, totals, skipped)
    K, bins = hist.shape[:2]
    for key in ("ece", "mce", "nll", "accuracy"):
        assert got[key] == pytest.approx(want[key], rel=1e-12, abs=1e-15), key
    assert got["pixels"] == want["pixels"] and got["skipped"] == skipped
    rows = got["reliability"]
    assert len(rows) == bins and [r["count"] for r in rows] == want["count"]
    assert [r["accuracy"] for r in rows] == pytest.approx(want["bin_accuracy"], rel=1e-12) and [r["confidence"] for r in rows] == pytest.approx(want["bin_confidence"], rel=1e-12)
    assert [(r["lo"], r["hi"]) for r in rows] == [(b / bins, (b + 1) / bins) for b in range(bins)]
    assert [r["coverage"] for r in got["coverage"]] == pytest.approx(want["coverage"], rel=1e-12)
    assert [r["accuracy"] for r in got["coverage"]] == pytest.approx(want["coverage_accuracy"], rel=1e-12)
    assert [r["min_confidence"] for r in got["coverage"]] == [j / bins for j in range(bins)]
    assert len(got["per_class"]) == K
    for a in range(K):
        g, w = got["per_class"][a], want["per_class"][a]
        assert g["pixels"] == w["pixels"] and g["ece"] == pytest.approx(w["ece"], rel=1e-12) and g["mce"] == pytest.approx(w["mce"], rel=1e-12)
        assert g["accuracy"] == pytest.approx(w["accuracy"], rel=1e-12) and [r["count"] for r in g["reliability"]] == w["count"]


def test_compute_on_hand_worked_numbers():
    hist, totals, _ = TABLES["empty_bins"]
    got = MT.calibration_from_sums(hist, totals, 3)
    # bins 2, 5, 9 hold 10, 50, 40 pixels with accuracy 0.1, 0.4, 0.925 and confidence 0.25, 0.55, 0.9625
    assert got["pixels"] == 100 and got["accuracy"] == pytest.approx(0.58) and got["nll"] == pytest.approx(0.37)
    assert got["ece"] == pytest.approx(0.1 * 0.15 + 0.5 * 0.15 + 0.4 * 0.0375, abs=1e-6) and got["mce"] == pytest.approx(0.15, abs=1e-6)
    assert got["coverage"][0] == {"min_confidence": 0.0, "coverage": 1.0, "accuracy": pytest.approx(0.58)}
    assert got["coverage"][3]["coverage"] == pytest.approx(0.9) and got["coverage"][9]["coverage"] == pytest.approx(0.4)
    assert got["coverage"][9]["accuracy"] == pytest.approx(0.925) and got["reliability"][0]["count"] == 0 and got["reliability"][0]["accuracy"] == 0.0
    last = MT.calibration_from_sums(*TABLES["all_in_the_last_bin"][:2])
    assert last["ece"] == 0.0 and last["accuracy"] == 1.0 and last["nll"] == 0.0 and all(r["coverage"] == 1.0 for r in last["coverage"])
    none = MT.calibration_from_sums(*TABLES["nothing_counted"])
    assert none["pixels"] == 0 and none["ece"] == 0.0 and none["nll"] == 0.0 and none["skipped"] == 9 and none["coverage"][0]["coverage"] == 0.0


def test_the_metric_object_on_the_cpu_holds_its_sums_and_ignore_index_none_excludes_nothing():
    m = MT.CalibrationMetrics(4, bins=10, ignore_index=None, device="cpu")
    assert m.exclude == 0 and tuple(m.hist.shape) == (4, 10, 3) and m.hist.dtype == torch.int64 and m.num_classes == 4
    assert MT.CalibrationMetrics(4, device="cpu").exclude == 1 and MT.CalibrationMetrics(4, ignore_index=2, device="cpu").exclude == 4
    assert tuple(MT.CalibrationMetrics(4, device="cpu").hist.shape) == (4, 15, 3)
    m.hist[1, 9] = torch.tensor([4, 3, 4 * R.ONE])
    m.totals[0] = torch.tensor([4, 2 * R.ONE])
    out = m.compute()
    assert out["pixels"] == 4 and out["accuracy"] == 0.75 and out["ece"] == 0.25 and out["nll"] == 0.5 and out["per_class"][1]["pixels"] == 4
    m.reset()
    assert int(m.hist.sum()) == 0 and int(m.totals.sum()) == 0 and int(m.skipped.sum()) == 0


# ---- the temperature search -----------------------------------------------------------------------------------------------------------
def test_the_grid_is_even_in_log_t_and_keeps_its_ends():
    g = MT.temperature_grid(0.05, 20.0)
    assert len(g) == 8 and g[0] == 0.05 and g[-1] == 20.0
    steps = np.diff(np.log(g))
    assert np.allclose(steps, math.log(400.0) / 7, rtol=1e-12)


@pytest.mark.parametrize("s", [0.5, 1.0, 3.0])
def test_refine_temperature_finds_the_dense_scan_minimiser(s):
    """The NLL has one minimum in log T and the search keeps it bracketed, so the returned grid point is within one spacing of the last
    grid of the true minimiser; the scan's own resolution (its spacing) is added, nothing else."""
    logits, labels = R.synthetic_logits(s, (1, 4, 40, 41), seed=3)
    T, step = MT.refine_temperature(R.nll_evaluator(logits, labels, 4, (0,)), 0.05, 20.0, 6, return_step=True)
    want, spacing = R.dense_scan(logits, labels, 4, (0,))
    print(f"s = {s}: T = {T:.5f}, dense scan {want:.5f}, last step {step:.3e} (log T), scan spacing {spacing:.3e}")
    assert step == pytest.approx(math.log(400.0) / 7 * (2 / 7) ** 5, rel=1e-9)
    assert abs(math.log(T) - math.log(want)) <= step + spacing
    assert abs(math.log(T) - math.log(s)) < 0.15                        # the data were drawn at temperature s
    assert MT.refine_temperature(R.nll_evaluator(logits, labels, 4, (0,))) == T


def test_the_lowest_index_wins_ties_and_the_ends_clamp():
    seen = []

    def flat(temps):
        seen.append(list(temps))
        return [7] * len(temps)

    T, step = MT.refine_temperature(flat, 0.5, 8.0, 3, return_step=True)
    assert T == 0.5 and len(seen) == 3 and all(len(g) == 8 for g in seen)
    assert seen[1][0] == 0.5 and seen[1][-1] == seen[0][1] and seen[2][-1] == seen[1][1]      # index 0 every time: the bracket is [g0, g1]
    assert step == pytest.approx(math.log(16.0) / 7 / 49)
    two = lambda temps: [3, 1, 1, 2, 1, 5, 5, 5]      # noqa: E731
    seen.clear()
    assert MT.refine_temperature(lambda t: (seen.append(list(t)), two(t))[1], 1.0, 128.0, 2) == seen[1][1]
    assert seen[1][0] == seen[0][0] and seen[1][-1] == seen[0][2]                             # the first of the equal points, index 1
    up = MT.refine_temperature(lambda t: [-v for v in t], 1.0, 2.0, 4)                      # ever lower towards hi: the top end
    assert up == 2.0
    for bad in (dict(lo=0.0), dict(lo=2.0, hi=1.0), dict(hi=float("inf")), dict(rounds=0), dict(rounds=2.0), dict(lo=float("nan"))):
        with pytest.raises(ValueError):
            MT.refine_temperature(flat, **bad)
    with pytest.raises(ValueError, match="one loss per temperature"):
        MT.refine_temperature(lambda t: [1.0], 1.0, 2.0, 1)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def _cpu_pipe(labels=True):
    p = GpuTilePipeline([0.1] * 4, [0.2] * 4, random_crop_size=8, label_map="cnes-multiclass", device="cpu")
    g = torch.Generator().manual_seed(0)
    p.load(torch.randint(-100, 100, (3, 4, 16, 16), generator=g, dtype=torch.int32).to(torch.int16),
           torch.randint(0, 24, (3, 16, 16), generator=g, dtype=torch.int32).to(torch.uint8) if labels else None)
    return p


def test_validators_raise_before_the_gpu_refusal():
    s = torch.zeros(2, 4, 8, 8)
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    cf, new, fit = classmap.confidence, MT.CalibrationMetrics, MT.fit_temperature
    cal = new(4, device="cpu")
    pred = P.TilePredictor(lambda x: x, _cpu_pipe(), 4)
    bad = [
        lambda: cf(s, "prob"), lambda: cf(s, measure="entropy"), lambda: cf(s, "probs", temperature=2.0), lambda: cf(s, "logits", temperature=0.0),
        lambda: cf(s, "logits", temperature=float("nan")), lambda: cf(s, "logits", temperature=-1.0), lambda: cf(s, "logits", temperature=True),
        lambda: cf(s, min_confidence="0.5"), lambda: cf(s, min_confidence=float("nan")), lambda: cf(s, min_confidence=0.5, reject_to=4),
        lambda: cf(s, min_confidence=0.5, reject_to=-1), lambda: cf(s, min_confidence=0.5, reject_to=None), lambda: cf(s, dtype=torch.int32),
        lambda: cf(s.double()), lambda: cf(s[0, 0]), lambda: cf(s[:0]), lambda: cf(s.numpy()), lambda: cf(torch.zeros(1, 33, 4, 4)),
        lambda: new(0, device="cpu"), lambda: new(33, device="cpu"), lambda: new(4, bins=0, device="cpu"), lambda: new(4, bins=65, device="cpu"),
        lambda: new(4, bins=15.0, device="cpu"), lambda: new(4, ignore_index=4, device="cpu"), lambda: new(4, ignore_index=-1, device="cpu"),
        lambda: new(4, temperature=0.0, device="cpu"), lambda: new(4, temperature=float("inf"), device="cpu"),
        lambda: cal.update(s, y, "softmax"), lambda: cal.update(s, y[:1]), lambda: cal.update(s, y.int()), lambda: cal.update(s.double(), y),
        lambda: cal.update(s[:, :3], y), lambda: cal.update(s[0], y[0]), lambda: cal.update(s, y, label_lut=torch.zeros(256, dtype=torch.int32)),
        lambda: cal.update(s, y.to(torch.uint8), label_lut=torch.zeros(255, dtype=torch.int32)),
        lambda: new(4, temperature=2.0, device="cpu").update(s, y, "probs"),
        lambda: fit(s, y, 0), lambda: fit(s, y, 4, ignore_index=4), lambda: fit(s, y, 5), lambda: fit(s, y[:, :4], 4), lambda: fit(s, y, 4, lo=0.0),
        lambda: fit(s, y, 4, lo=2.0, hi=1.0), lambda: fit(s, y, 4, rounds=0),
        lambda: pred.predict_with_confidence(measure="entropy"), lambda: pred.predict_with_confidence([7]),
        lambda: pred.evaluate_calibration(new(5, device="cpu")), lambda: pred.evaluate_calibration(cal, [7]), lambda: pred.evaluate_calibration(cal, []),
        lambda: P.TilePredictor(lambda x: x, _cpu_pipe(labels=False), 4).evaluate_calibration(cal),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} did not raise")


def test_the_new_functions_refuse_the_cpu():
    s = torch.zeros(2, 4, 8, 8)
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    cal = MT.CalibrationMetrics(4, device="cpu")
    pred = P.TilePredictor(lambda x: x, _cpu_pipe(), 4)
    calls = (lambda: classmap.confidence(s), lambda: classmap.confidence(s[0], "logits", "margin", 1.5, 0.3, 2, torch.uint8),
             lambda: cal.update(s, y), lambda: cal.update(s, y.to(torch.uint8), "probs", label_lut=torch.zeros(256, dtype=torch.int32)),
             lambda: MT.fit_temperature(s, y, 4), lambda: MT.fit_temperature(s, y.to(torch.uint8), 4, None, 0.5, 4.0, 2),
             lambda: pred.predict_with_confidence(), lambda: pred.predict_with_confidence([0, 2], "margin", 0.4, 1),
             lambda: pred.evaluate_calibration(cal), lambda: pred.evaluate_calibration(cal, [1]))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert int(cal.hist.sum()) == 0 and int(cal.totals.sum()) == 0      # nothing was counted
