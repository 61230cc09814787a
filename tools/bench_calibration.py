"""Time of the calibration launch (s2k_calibration, csrc/calibration.hip) on 64 maps of 512 x 512 with K = 4 and K = 10 classes, as
blended probabilities and as logits of the same size, against the torch expression of the same result on the same device.

    python tools/bench_calibration.py [--maps 64] [--iters 10] [--reps 5]

Calls timed, each over all maps:
  histogram   `CalibrationMetrics.update`: the reliability histogram, the NLL sum and the skipped count, int64 labels.
              torch: softmax (logits only) / max / the bin index / three bincounts, and log_softmax / gather for the NLL.
  maps        `classmap.confidence`: the int64 class map and the float32 confidence raster.  torch: softmax (logits only) / max.
  8 temps     one launch that takes `totals` only, for 8 temperatures (logits only).  torch: log_softmax(z / T) / gather per temperature.
  fit         a whole `fit_temperature` (6 rounds of 8 temperatures, one host read per round; logits only).  torch: the same search
              (`refine_temperature`) over the torch evaluator.
Times are HIP events around `iters` whole calls (allocation of the outputs and the host's argument checks included) after a warm-up;
every configuration is timed `reps` times, alternating with its baseline, and the median and the range are printed.  Bytes are
algorithmic, from the shapes, per call: the scores read once (4 K B / pixel) plus 8 B of label for the sums, or 12 B of outputs for the
maps; `fit` reads that `rounds` times.  Their rate is printed beside the copy ceiling `s2k_measure_peaks` measures on the same device at
the start of the run.  The torch results are compared with the kernel's: the counts must agree except where a confidence sits within
float32 rounding of a bin edge (printed), the NLL to 1e-5 relative.  Nothing here is a pass bar."""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from s2lc_amd import _lib, classmap  # noqa: E402
from s2lc_amd import metrics as MT  # noqa: E402

BINS = 15


def timed(fn, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def alternate(ours, base, iters, reps):
    ours(), ours(), base()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(ours, iters))
        b.append(timed(base, max(1, iters // 5)))
    return a, b


def line(name, a, b, byts, ceiling, note):
    med, bmed = statistics.median(a), statistics.median(b)
    span = f"{med:8.4f} ({min(a):.4f} .. {max(a):.4f})"
    bspan = f"{bmed:9.3f} ({min(b):.3f} .. {max(b):.3f})"
    rate = byts / (med * 1e-3)
    print(f"{name:34s} {span:>28s} {rate / 1e12:6.3f} {100.0 * rate / ceiling:6.1f}% {bspan:>30s} {bmed / med:7.1f}x  {note}", flush=True)


def torch_hist(scores, labels, K, logits):
    """(hist int64 [K, BINS, 2], conf sum float64 [K, BINS], nll sum float64) of the torch expression; class 0 is not counted"""
    p = torch.softmax(scores, 1) if logits else scores
    conf, pred = p.max(1)
    b = (conf * BINS).long().clamp_(max=BINS - 1)
    keep = (labels > 0) & (labels < K)
    cell = (pred * BINS + b)[keep]
    n = torch.bincount(cell, minlength=K * BINS)
    ok = torch.bincount(cell, weights=(pred == labels)[keep].double(), minlength=K * BINS)
    cs = torch.bincount(cell, weights=conf[keep].double(), minlength=K * BINS)
    lp = torch.log_softmax(scores, 1) if logits else torch.log(scores)
    nll = -lp.gather(1, labels.clamp(0, K - 1).unsqueeze(1)).squeeze(1)[keep].double().sum()
    return torch.stack([n, ok.long()], 1).view(K, BINS, 2), cs.view(K, BINS), nll


def torch_nll(scores, labels, K, temps):
    keep = (labels > 0) & (labels < K)
    idx = labels.clamp(0, K - 1).unsqueeze(1)
    return [float(-torch.log_softmax(scores / T, 1).gather(1, idx).squeeze(1)[keep].double().sum()) for T in temps]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_calibration.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    M, H, W = a.maps, 512, 512
    pix = M * H * W
    ceiling = _lib.measure_peaks(dev)["copy_gbps"] * 1e9
    print(f"{M} maps of {H} x {W}, {BINS} bins, {a.iters} calls per window, {a.reps} windows each, one run; {torch.cuda.get_device_name(0)}; "
          f"measured copy ceiling {ceiling / 1e12:.2f} TB/s (read + write)")
    print(f"{'configuration':34s} {'ms median (min .. max)':>28s} {'TB/s':>6s} {'of copy':>7s} {'torch ms median (min .. max)':>30s} {'ratio':>8s}  note")
    g = torch.Generator().manual_seed(0)
    for K in (4, 10):
        z0 = torch.randn(min(M, 4), K, H, W, generator=g) * 1.5                   # four maps drawn, repeated to M with their labels
        labels = torch.multinomial(torch.softmax(z0.permute(0, 2, 3, 1).reshape(-1, K), 1), 1, generator=g).view(-1, H, W)
        labels = labels.repeat((M + 3) // 4, 1, 1)[:M].contiguous().to(dev)       # drawn from softmax(z0)
        logits = (z0 * 2.0).repeat((M + 3) // 4, 1, 1, 1)[:M].contiguous().to(dev)      # twice too sharp: the fitted temperature is near 2
        del z0
        for kind, scores in (("probs", torch.softmax(logits, 1)), ("logits", logits)):
            is_logits = kind == "logits"
            cal = MT.CalibrationMetrics(K, BINS, device=dev)
            cal.update(scores, labels, kind)
            th, tcs, tnll = torch_hist(scores, labels, K, is_logits)
            off = int((cal.hist[:, :, 0] - th[:, :, 0]).abs().sum()) // 2
            same = (torch.equal(cal.hist[:, :, :2].sum(1), th.sum(1))
                    and abs(float(cal.totals[0, 1]) / classmap.CAL_ONE - float(tnll)) <= 1e-5 * float(tnll))
            ours = lambda: (cal.reset(), cal.update(scores, labels, kind))      # noqa: E731
            base = lambda: torch_hist(scores, labels, K, is_logits)             # noqa: E731
            t, b = alternate(ours, base, a.iters, a.reps)
            line(f"histogram K={K} {kind}", t, b, (4 * K + 8) * pix, ceiling,
                 f"per-class counts and NLL {'agree' if same else 'DIFFER'}; {off} of {int(th[:, :, 0].sum())} pixels in a neighbouring bin")
            ours = lambda: classmap.confidence(scores, kind)                    # noqa: E731
            base = lambda: (torch.softmax(scores, 1) if is_logits else scores).max(1)      # noqa: E731
            cm, cf = ours()
            bc, bp = base()
            note = f"class maps {'equal' if torch.equal(cm, bp) else 'DIFFER'}; largest |conf - torch| {float((cf - bc).abs().max()):.2e}"
            t, b = alternate(ours, base, a.iters, a.reps)
            line(f"maps K={K} {kind}", t, b, (4 * K + 12) * pix, ceiling, note)
            del cm, cf, bc, bp
        temps = MT.temperature_grid(0.5, 8.0)
        totals = torch.zeros(8, 2, dtype=torch.int64, device=dev)
        ours = lambda: (totals.zero_(), classmap.launch_calibration(logits, 1, temps, labels=labels, exclude=1, totals=totals))      # noqa: E731
        base = lambda: torch_nll(logits, labels, K, temps)                      # noqa: E731
        ours()
        want = base()
        worst = max(abs(int(totals[i, 1]) / classmap.CAL_ONE - want[i]) / want[i] for i in range(8))
        t, b = alternate(ours, base, a.iters, a.reps)
        line(f"8 temperatures K={K} logits", t, b, (4 * K + 8) * pix, ceiling, f"largest relative NLL difference {worst:.1e}")
        t0 = time.perf_counter()
        T = MT.fit_temperature(logits, labels, K)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        Tt = MT.refine_temperature(lambda ts: torch_nll(logits, labels, K, ts))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        fits = [(t1 - t0) * 1e3]
        for _ in range(a.reps - 1):
            t0 = time.perf_counter()
            MT.fit_temperature(logits, labels, K)
            torch.cuda.synchronize()
            fits.append((time.perf_counter() - t0) * 1e3)
        line(f"fit_temperature K={K} (6 rounds)", fits, [(t2 - t1) * 1e3], 6 * (4 * K + 8) * pix, ceiling,
             f"host clock, whole calls; T = {T:.5f}, torch search {Tt:.5f} (one run)")
        del logits, labels


if __name__ == "__main__":
    main()
