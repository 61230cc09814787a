"""GPU: `s2k_calibration` (csrc/calibration.hip) through `_lib.calibration` against its numpy restatement (tests/calibration_ref.py), and
the Python surface built on it.  Every call is made twice; the second result must be `torch.equal` to the first.

Bars.
* Mode 0 (probabilities): `hist`, `skipped`, `pred` and `conf` under both measures are EQUAL to the restatement: c is a copy of a
  score, the margin one float32 subtraction, and everything after c is integer work.  (A NaN has no value to compare: the NaN
  positions must agree, and every other value must be equal.)
* Mode 1 (logits) is pinned by two checks together.  (a) The written `conf`, and the mean NLL implied by `totals`, lie within
  `calibration_ref.conf_tolerance` / `nll_tolerance` of the float64 reference.  Those are derived from the operation order stated in
  include/s2k.h - three roundings on the exponent's argument, expf within 1 ulp and logf within 1 ulp (ROCm's HIP math API tables), a
  correctly rounded division, K - 1 additions, and the 2^-21 quantisation of the NLL; the derivations are in the two functions'
  docstrings - and not from anything the kernel returned.  (b) `hist` and `pred` are EQUAL to the restatement applied to the kernel's
  own `conf` map (measure 0: the binning confidence) and the raw scores, under either measure.
* Sums over several temperatures in one call equal those of single-temperature calls exactly.
* `fit_temperature`: within two steps of the last grid, in log T, of the float64 dense-scan minimiser (plus that scan's own spacing):
  one step because the search returns a grid point next to the minimiser, a second because the argmin may move by one point where
  neighbouring sums differ by less than the float32 rounding of their terms - the next bracket still contains the optimum."""
import functools
import math

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import _lib, classmap
from s2lc_amd import metrics as MT
from s2lc_amd import predict as P
from tests import calibration_ref as R
from tests.test_predict_gpu import BANDS, TH, TW, Pointwise, _pipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U64 = dict(dtype=torch.int64, device=DEV)


def run(scores, mode, K, bins=15, labels=None, lut=None, exclude=0, temps=(1.0,), measure=0, reject_below=0.0, reject_to=-1,
        want=("conf", "pred", "hist", "totals", "skipped"), pred_dtype=torch.int64, fill=None):
    """two s2k_calibration calls over numpy inputs -> {name: numpy array} of the first, after checking the second is equal.  Outputs
    are prefilled (conf -7, pred 99, the sums with `fill`) so that a pixel that was not written, or a sum that was overwritten, shows;
    the inputs are compared with their copies afterwards."""
    N, _, Pn = scores.shape
    dev = {"scores": torch.from_numpy(scores).to(DEV)}
    dev["labels"] = None if labels is None else torch.from_numpy(labels).to(DEV)
    dev["lut"] = None if lut is None else torch.from_numpy(lut).to(DEV)
    before = {k: None if v is None else v.clone() for k, v in dev.items()}
    fill = fill or {}
    outs = []
    for _ in range(2):
        o = {"conf": torch.full((N, Pn), -7.0, device=DEV) if "conf" in want else None,
             "pred": torch.full((N, Pn), 99, dtype=pred_dtype, device=DEV) if "pred" in want else None,
             "hist": torch.full((K, bins, 3), fill.get("hist", 0), **U64) if "hist" in want else None,
             "totals": torch.full((len(temps), 2), fill.get("totals", 0), **U64) if "totals" in want else None,
             "skipped": torch.full((1,), fill.get("skipped", 0), **U64) if "skipped" in want else None}
        _lib.check(_lib.calibration(dev["scores"], mode, dev["labels"], dev["lut"], (N, K, Pn), exclude, list(temps), bins, measure, reject_below,
                                    reject_to, o["conf"], o["pred"], o["hist"], o["totals"], o["skipped"],
                                    torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        outs.append(o)
    for k in outs[0]:
        if outs[0][k] is not None:
            a, b = outs[0][k], outs[1][k]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    for k, v in dev.items():
        assert v is None or torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v, before[k].view(torch.int32) if v.dtype == torch.float32 else before[k]), k
    return {k: v.cpu().numpy() for k, v in outs[0].items() if v is not None}


def same(got, want):
    """equal, a NaN matching a NaN only"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


# ---- mode 0: exact --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probs_case(N, K, Pn, bins):
    """float32 scores [N, K, P] whose maxima populate every bin, with exact ties between classes, maxima on bin edges and at 1.0, NaN,
    values above 1 and negative maxima; int64 labels with 3 % out of range; uint8 labels and a table that give the same classes"""
    rng = np.random.default_rng(1000 * K + 10 * Pn + bins + N)
    n = N * Pn
    want_c = ((rng.permutation(n) % bins + rng.random(n)) / bins).astype(np.float32)       # a maximum for every bin, whatever n allows
    s = np.empty((n, K), np.float32)
    win = rng.integers(0, K, n)
    for k in range(K):
        s[:, k] = want_c * rng.random(n).astype(np.float32) * np.float32(0.999)
    s[np.arange(n), win] = want_c
    kind = rng.integers(0, 20, n)
    edge = (rng.integers(0, bins + 1, n).astype(np.float32) / np.float32(bins)).astype(np.float32)
    on_edge = kind == 0
    s[on_edge] = np.minimum(s[on_edge], edge[on_edge, None] * np.float32(0.5))
    s[on_edge, win[on_edge]] = edge[on_edge]                    # exactly on a bin edge, 0.0 and 1.0 included
    if K > 1:
        tie = kind == 1
        other = (win + 1 + rng.integers(0, K - 1, n)) % K
        s[tie, other[tie]] = s[tie, win[tie]]                   # two classes share the maximum: the lower index must win
    s[kind == 2, 0] = np.nan                                    # NaN in front: it stays the "maximum"
    s[kind == 3, K - 1] = np.nan if K > 1 else 1.5              # NaN behind: never chosen (K = 1: a value above 1)
    s[kind == 4, win[kind == 4]] = 1.25                         # above 1
    s[kind == 5] = -np.abs(s[kind == 5]) - np.float32(0.01)     # every score negative
    if n >= 8:                                                  # whatever the draw, the small maps hold one of each
        s[0, :] = 0.5
        s[1, 0] = np.nan
        s[2, :] = -0.25
        s[3, :] = 0.0
        s[3, win[3]] = 1.0
    scores = np.ascontiguousarray(s.reshape(N, Pn, K).transpose(0, 2, 1))
    lab = rng.integers(0, K, (N, Pn))
    lab[rng.random((N, Pn)) < 0.03] = K + 1                     # 3 % out of range
    if n >= 8:
        lab.reshape(-1)[:4] = K - 1                             # ... and counts them (or skips them) unless class K - 1 is excluded
    lut = (np.arange(256) % (K + 3)).astype(np.int32)           # the table maps raw bytes onto 0 .. K + 2
    raw = (lab + (K + 3) * rng.integers(0, 256 // (K + 3) - 1, (N, Pn))).astype(np.uint8)
    assert np.array_equal(lut[raw], lab)
    return scores, lab.astype(np.int64), raw, lut


SHAPES0 = ([(1, 4, Pn, 15) for Pn in (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)] + [(3, 4, Pn, 10) for Pn in (5, 257, 1024, 1025)]
           + [(3, K, 1023, 15) for K in (1, 2, 3, 9, 32)] + [(1, K, 1024, 10) for K in (1, 2, 3, 9, 32)] + [(3, 4, 257, b) for b in (1, 64)]
           + [(1, 9, 1024, 64), (3, 32, 256, 1)])


@pytest.mark.parametrize("exclude", [0, 1], ids=["all", "not0"])
@pytest.mark.parametrize("N,K,Pn,bins", SHAPES0, ids=[f"N{n}_K{k}_P{p}_b{b}" for n, k, p, b in SHAPES0])
def test_mode_0_is_exact(N, K, Pn, bins, exclude):
    scores, lab, raw, lut = probs_case(N, K, Pn, bins)
    a, c, _ = R.confidence_probs(scores, 0)
    ex = (0,) if exclude else ()
    hist, counted, skipped = R.sums(a, c, lab, K, bins, ex)
    if N * Pn >= 1023 and not (K == 1 and exclude):          # the inputs hold what the case is about: every bin, ties, bin edges, 1.0, and skipped pixels
        top2 = np.sort(np.nan_to_num(scores, nan=-9.0), axis=1)
        assert (hist[:, :, 0].sum(0) > 0).all() and skipped > 0 and counted.sum() > 0 and (K == 1 or ((top2[:, -1] == top2[:, -2]) & counted).any())
        assert ((c == 1.0) & counted).any() and (np.isnan(c)).any() and (c > 1).any() and (c < 0).any()
        assert bins == 1 or (counted & (c > 0) & (c < 1) & (np.float32(c * np.float32(bins)) == np.floor(c * np.float32(bins)))).any()
    for measure in (0, 1):
        _, _, conf = R.confidence_probs(scores, measure)
        for labels, table in ((lab, None), (raw, lut)):
            got = run(scores, 0, K, bins, labels, table, exclude, measure=measure, reject_below=0.5, reject_to=K - 1, fill=dict(hist=3, skipped=5))
            assert same(got["conf"], conf), f"conf, measure {measure}"
            assert np.array_equal(got["pred"], R.reject(a, conf, 0.5, K - 1))
            assert np.array_equal(got["hist"], hist + 3) and int(got["skipped"][0]) == skipped + 5       # added to, never overwritten
            assert int(got["totals"][0, 0]) == int(counted.sum())
            tol = R.nll_tolerance(K, scores, 1.0, probs=True)
            if counted.any():
                mean = int(got["totals"][0, 1]) / R.ONE / counted.sum()
                assert abs(mean - R.nll64(scores, lab, counted, probs=True) / counted.sum()) <= tol


def test_a_cell_holds_more_than_32_bits_of_confidence():
    """8192 pixels of one class at confidence 1.0 in one map: 2^20 per pixel passes 2^32 after 4096 of them in one cell"""
    K, Pn, bins = 3, 8192 + 4, 15
    scores = np.zeros((1, K, Pn), np.float32)
    scores[0, 1] = 1.0
    lab = np.ones((1, Pn), np.int64)
    got = run(scores, 0, K, bins, lab, want=("hist", "totals", "skipped"))
    want = np.zeros((K, bins, 3), np.int64)
    want[1, bins - 1] = [Pn, Pn, Pn * 2 ** 20]
    assert Pn * 2 ** 20 > 2 ** 32 and np.array_equal(got["hist"], want) and got["totals"].tolist() == [[Pn, 0]] and int(got["skipped"][0]) == 0
    got = run(scores * 4.0, 1, K, bins, lab, temps=(0.25,), want=("hist", "totals"))        # logits: softmax gives 1 - 2 e^-16, bin 14 still
    assert got["hist"][1, bins - 1, 0] == Pn and got["hist"][1, bins - 1, 2] > 2 ** 32 and got["hist"].sum(0).sum(0)[0] == Pn
    # five grid passes: every workgroup adds more than 4096 pixels, 2^32 in all, to ONE of its own cells before it flushes
    Pn = 5 * classmap.CAL_MAX_GRID * 1024 + 4
    scores = np.zeros((1, 2, Pn), np.float32)
    scores[0, 1] = 1.0
    got = run(scores, 0, 2, 1, np.ones((1, Pn), np.uint8), want=("hist", "totals"))
    assert got["hist"].tolist() == [[[0, 0, 0]], [[Pn, Pn, Pn * 2 ** 20]]] and got["totals"].tolist() == [[Pn, 0]]


def test_more_quads_than_one_grid_pass():
    """CAL_MAX_GRID workgroups of 256 quads make one pass; this map takes a little more than two, with a ragged end"""
    K, bins = 2, 10
    Pn = (2 * classmap.CAL_MAX_GRID * 256 + 300) * 4 + 2
    rng = np.random.default_rng(2)
    scores = rng.random((1, K, Pn), dtype=np.float32)
    lab = rng.integers(0, K + 1, (1, Pn))
    a, c, conf = R.confidence_probs(scores, 1)
    hist, counted, skipped = R.sums(a, c, lab, K, bins)
    for s, l in ((scores, lab), (scores[:, :, :Pn - 2], lab[:, :Pn - 2])):       # P % 4 == 2: the scalar path; P % 4 == 0: quads
        s, l = np.ascontiguousarray(s), np.ascontiguousarray(l)
        got = run(s, 0, K, bins, l, measure=1)
        n = s.shape[2]
        assert same(got["conf"], conf[:, :n]) and np.array_equal(got["pred"], a[:, :n])
        h, cnt, sk = (hist, counted, skipped) if n == Pn else R.sums(a[:, :n], c[:, :n], l, K, bins)
        assert np.array_equal(got["hist"], h) and int(got["totals"][0, 0]) == int(cnt.sum()) and int(got["skipped"][0]) == sk == 0


# ---- mode 1: a derived tolerance and the kernel's own confidence ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logits_case(N, K, Pn):
    rng = np.random.default_rng(77 * K + Pn + N)
    scores = (rng.normal(0.0, 3.0, (N, K, Pn)) * rng.choice([0.1, 1.0, 3.0], (N, 1, Pn))).astype(np.float32)
    if K > 1:
        scores[:, 0, ::7] = scores[:, 1, ::7] = scores.max(1)[:, ::7] + np.float32(0.5)      # exact ties at the top: class 0 must win
    lab = rng.integers(0, K, (N, Pn))
    lab[rng.random((N, Pn)) < 0.03] = K + 2
    return scores, lab.astype(np.int64)


SHAPES1 = [(1, 4, 1024), (3, 4, 1025), (3, 3, 257), (1, 1, 256), (3, 2, 1023), (1, 9, 1024), (3, 32, 255), (1, 32, 1024), (1, 4, 5)]


@pytest.mark.parametrize("T", [0.5, 1.0, 2.5])
@pytest.mark.parametrize("N,K,Pn", SHAPES1, ids=[f"N{n}_K{k}_P{p}" for n, k, p in SHAPES1])
def test_mode_1_conf_and_nll_within_the_derived_tolerance_and_counts_from_its_own_conf(N, K, Pn, T):
    scores, lab = logits_case(N, K, Pn)
    bins, exclude = 15, 1 if K > 1 else 0
    ex = (0,) if exclude else ()
    got = run(scores, 1, K, bins, lab, exclude=exclude, temps=(T,), fill=dict(totals=11))
    # (a) the written confidence and the NLL against float64
    err = float(np.abs(got["conf"].astype(np.float64) - R.confidence64(scores, T, 0)).max())
    tol = R.conf_tolerance(K, 0)
    print(f"N={N} K={K} P={Pn} T={T}: conf err {err:.3e} tol {tol:.3e}")
    assert np.isfinite(got["conf"]).all() and err <= tol
    # (b) the counts are those of the restatement over the kernel's own confidence and the raw scores
    a, _ = R.argmax_first(scores)
    hist, counted, skipped = R.sums(a, got["conf"], lab, K, bins, ex)
    assert np.array_equal(got["pred"], a) and np.array_equal(got["hist"], hist) and int(got["skipped"][0]) == skipped == 0
    n = int(counted.sum())
    assert int(got["totals"][0, 0]) == n + 11 and (n > 0 or Pn < 64)
    if n:
        mean = (int(got["totals"][0, 1]) - 11) / R.ONE / n
        ref = R.nll64(scores, lab, counted, T) / n
        ntol = R.nll_tolerance(K, scores, T)
        print(f"    mean nll {mean:.6f} ref {ref:.6f} |diff| {abs(mean - ref):.3e} tol {ntol:.3e}")
        assert abs(mean - ref) <= ntol
    # the margin is written, the maximum is binned: same hist, and the rejection follows the written value
    m = run(scores, 1, K, bins, lab, exclude=exclude, temps=(T,), measure=1, reject_below=0.3, reject_to=0, pred_dtype=torch.uint8)
    merr = float(np.abs(m["conf"].astype(np.float64) - R.confidence64(scores, T, 1)).max())
    print(f"    margin err {merr:.3e} tol {R.conf_tolerance(K, 1):.3e}")
    assert merr <= R.conf_tolerance(K, 1)
    assert np.array_equal(m["hist"], hist) and m["totals"].tolist() == (got["totals"] - 11).tolist()
    assert m["pred"].dtype == np.uint8 and np.array_equal(m["pred"], R.reject(a, m["conf"], 0.3, 0))
    if K > 1 and Pn >= 255:
        top2 = np.sort(scores, axis=1)
        tie = top2[:, -1] == top2[:, -2]
        assert (m["pred"] != a).any() and (m["pred"] == a).any() and tie.any() and (m["conf"][tie] == 0).all()      # ties have no margin


@pytest.mark.parametrize("N,K,Pn", [(3, 4, 1025), (1, 9, 1024), (1, 2, 4096)])
def test_eight_temperatures_in_one_call_equal_eight_calls(N, K, Pn):
    scores, lab = logits_case(N, K, Pn)
    temps = (0.5, 1.0, 2.5, 0.05, 20.0, 0.9, 1.1, 7.0)
    eight = run(scores, 1, K, 15, lab, exclude=1, temps=temps, want=("totals", "hist", "conf"))
    for t, T in enumerate(temps):
        one = run(scores, 1, K, 15, lab, exclude=1, temps=(T,), want=("totals",))
        assert one["totals"][0].tolist() == eight["totals"][t].tolist(), T
    first = run(scores, 1, K, 15, lab, exclude=1, temps=temps[:1], want=("hist", "conf"))
    assert np.array_equal(first["hist"], eight["hist"]) and same(first["conf"], eight["conf"])      # temps[0] alone decides the confidence
    assert len({int(v) for v in eight["totals"][:, 1]}) == 8 and (eight["totals"][:, 0] == eight["totals"][0, 0]).all()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("measure", [0, 1], ids=["max", "margin"])
def test_rejection_changes_pred_and_nothing_else(measure, dtype):
    N, K, Pn, bins = 3, 4, 1025, 15
    scores, lab, raw, lut = probs_case(N, K, Pn, bins)
    a, c, conf = R.confidence_probs(scores, measure)
    plain = run(scores, 0, K, bins, raw, lut, 1, measure=measure, pred_dtype=dtype)
    assert np.array_equal(plain["pred"], a) and plain["pred"].dtype == (np.uint8 if dtype == torch.uint8 else np.int64)
    for below, to in ((0.6, 0), (0.25, 3), (2.0, 1), (-5.0, 2)):
        got = run(scores, 0, K, bins, raw, lut, 1, measure=measure, reject_below=below, reject_to=to, pred_dtype=dtype)
        want = R.reject(a, conf, below, to)
        assert np.array_equal(got["pred"], want) and ((want != a).any() == (below > 0))
        for k in ("hist", "totals", "skipped"):
            assert np.array_equal(got[k], plain[k]), k
        assert same(got["conf"], plain["conf"])
    # a NaN confidence is never below anything
    assert (np.isnan(conf) & (R.reject(a, conf, 2.0, 1) == a) & (a != 1)).any()


def test_outputs_are_optional_and_labels_are_only_needed_for_sums():
    scores, lab, _, _ = probs_case(3, 4, 1025, 15)
    a, c, conf = R.confidence_probs(scores, 0)
    only_conf = run(scores, 0, 4, want=("conf",))
    only_pred = run(scores, 0, 4, want=("pred",), pred_dtype=torch.uint8)
    assert same(only_conf["conf"], conf) and np.array_equal(only_pred["pred"], a)
    only_skipped = run(scores, 0, 4, labels=lab, want=("skipped",))
    assert int(only_skipped["skipped"][0]) == R.sums(a, c, lab, 4, 15)[2]


# ---- CalibrationMetrics and fit_temperature ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic(s):
    logits, labels = R.synthetic_logits(s)                     # K = 4 on 3 x 65 x 67
    return logits, labels, R.dense_scan(logits, labels, 4, (0,))


def test_update_over_two_batches_equals_one_update():
    logits, labels, _ = synthetic(3.0)
    z, y = torch.from_numpy(logits).to(DEV), torch.from_numpy(labels).to(DEV)
    whole, parts, again = (MT.CalibrationMetrics(4, device=DEV) for _ in range(3))
    whole.update(z, y)
    parts.update(z[:1], y[:1])
    parts.update(z[1:], y[1:])
    again.update(z, y)
    for a in ("hist", "totals", "skipped"):
        assert torch.equal(getattr(whole, a), getattr(parts, a)) and torch.equal(getattr(whole, a), getattr(again, a)), a
    out = whole.compute()
    a, _ = R.argmax_first(logits.reshape(3, 4, -1))
    keep = labels.reshape(3, -1) != 0
    assert out["pixels"] == int(keep.sum()) and out["skipped"] == 0 and out["accuracy"] == pytest.approx((a == labels.reshape(3, -1))[keep].mean(), abs=1e-12)
    want = R.figures(whole.hist.cpu().numpy(), whole.totals.cpu().numpy()[0])
    assert out["ece"] == pytest.approx(want["ece"], rel=1e-12) and out["nll"] == pytest.approx(want["nll"], rel=1e-12)
    assert abs(out["nll"] - R.nll64(logits.reshape(3, 4, -1), labels.reshape(3, -1), keep) / keep.sum()) <= R.nll_tolerance(4, logits.reshape(3, 4, -1), 1.0)
    u8 = MT.CalibrationMetrics(4, device=DEV)
    u8.update(z, y.to(torch.uint8))
    assert torch.equal(u8.hist, whole.hist) and torch.equal(u8.totals, whole.totals)
    probs = MT.CalibrationMetrics(4, device=DEV)
    probs.update(torch.softmax(z, 1), y, "probs")
    assert probs.compute()["pixels"] == out["pixels"] and abs(probs.compute()["ece"] - out["ece"]) < 1e-4
    whole.reset()
    assert int(whole.hist.sum()) == 0 and int(whole.totals.sum()) == 0


@pytest.mark.parametrize("s", [0.5, 1.0, 3.0])
def test_fit_temperature_finds_the_dense_scan_minimiser(s):
    """Measured on an MI355X: 1.2e-4 / 2.7e-4 / 8.2e-4 in log T for s = 0.5 / 1 / 3, under ONE step of the last grid (1.63e-3); the bar
    is two steps plus the scan's spacing (module docstring)."""
    logits, labels, (want, spacing) = synthetic(s)
    z, y = torch.from_numpy(logits).to(DEV), torch.from_numpy(labels).to(DEV)
    T = MT.fit_temperature(z, y, 4)
    step = math.log(400.0) / 7 * (2 / 7) ** 5
    dist = abs(math.log(T) - math.log(want))
    print(f"s = {s}: fitted T = {T:.6f}, dense scan {want:.6f}, distance {dist:.3e} in log T, last step {step:.3e}")
    assert dist <= 2 * step + spacing
    assert MT.fit_temperature(z, y, 4) == T and MT.fit_temperature(z, y.to(torch.uint8), 4) == T      # bit for bit
    if s == 3.0:
        before, after = MT.CalibrationMetrics(4, device=DEV), MT.CalibrationMetrics(4, temperature=T, device=DEV)
        before.update(z, y)
        after.update(z, y)
        e0, e1 = before.compute()["ece"], after.compute()["ece"]
        print(f"    ece at T = 1: {e0:.4f}, at the fitted T: {e1:.4f}")
        assert e1 < e0 and after.compute()["nll"] < before.compute()["nll"]


def test_confidence_returns_the_class_map_and_the_raster():
    scores, _, _, _ = probs_case(3, 4, 1024, 15)
    s = torch.from_numpy(scores).to(DEV).view(3, 4, 32, 32)
    a, c, conf = R.confidence_probs(scores, 1)
    cm, cf = classmap.confidence(s, "probs", "margin", min_confidence=0.5, reject_to=2, dtype=torch.uint8)
    assert cm.shape == cf.shape == (3, 32, 32) and cm.dtype == torch.uint8 and cf.dtype == torch.float32
    assert same(cf.cpu().numpy().reshape(3, -1), conf) and np.array_equal(cm.cpu().numpy().reshape(3, -1), R.reject(a, conf, 0.5, 2))
    cm, cf = classmap.confidence(s[1])
    assert cm.shape == (32, 32) and cm.dtype == torch.int64 and np.array_equal(cm.cpu().numpy().reshape(-1), a[1]) and same(cf.cpu().numpy().reshape(-1), c[1])
    z, _ = logits_case(1, 4, 1024)
    cm, cf = classmap.confidence(torch.from_numpy(z).to(DEV).view(1, 4, 32, 32), "logits", temperature=2.5)
    assert float(np.abs(cf.cpu().numpy().reshape(1, -1) - R.confidence64(z, 2.5)).max()) <= R.conf_tolerance(4)


# ---- TilePredictor --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", ["probs", "logits"])
def test_predictor_confidence_and_calibration(blend):
    K = 4
    pipe, model = _pipe(32), Pointwise(K, BANDS)
    pred = P.TilePredictor(model, pipe, K, flips=(0, 1), blend=blend, tiles_per_launch=2)
    idx = [1, 2, 2]
    scores = pred.predict_blend(idx)
    flat = scores.cpu().numpy().reshape(3, K, -1)
    cm, cf = pred.predict_with_confidence(idx)
    assert cm.shape == (3, TH, TW) and cm.dtype == torch.int64 and cf.dtype == torch.float32 and torch.equal(cm, pred.predict(idx))
    a, c = R.argmax_first(flat)
    if blend == "probs":
        assert same(cf.cpu().numpy().reshape(3, -1), c)
        mcm, mcf = pred.predict_with_confidence(idx, "margin", 0.2, 0)
        _, _, margin = R.confidence_probs(flat, 1)
        assert same(mcf.cpu().numpy().reshape(3, -1), margin) and np.array_equal(mcm.cpu().numpy().reshape(3, -1), R.reject(a, margin, 0.2, 0))
        assert (mcm != cm).any()
    else:
        assert float(np.abs(cf.cpu().numpy().reshape(3, -1) - R.confidence64(flat, 1.0)).max()) <= R.conf_tolerance(K)
    fused, staged = MT.CalibrationMetrics(K, device=DEV), MT.CalibrationMetrics(K, device=DEV)
    pred.evaluate_calibration(fused, idx)
    remapped = pipe.lut.long()[pipe.labels[idx].long()]
    staged.update(scores, remapped, blend)
    for name in ("hist", "totals", "skipped"):
        assert torch.equal(getattr(fused, name), getattr(staged, name)), name
    out = fused.compute()
    ignored = int(((remapped < 0) | (remapped >= K) | (remapped == 0)).sum())
    assert out["skipped"] == 0 and out["pixels"] + ignored == remapped.numel() and 0 < out["pixels"] < remapped.numel()
    pred.evaluate_calibration(fused, idx)                       # accumulates
    assert torch.equal(fused.hist, 2 * staged.hist) and torch.equal(fused.totals, 2 * staged.totals)
