"""Time of flat_stats (csrc/flat_stats.hip: SEG_STATS, SEG_HIST, GRAD_CLIP) over the flat buffers of U-Net b5 (13 bands) and
Prithvi-100M (the MAE), next to what the same numbers cost through torch one tensor at a time.  No training step is needed: the
gradient buffer is filled with N(0, 1e-3) values and every parameter on the network's path gets its `.grad` view.

    python tools/bench_flat_stats.py [--iters 50] [--runs 3] [--models unet_b5,prithvi_100m]

Per model and run:
  * `FlatStats.gradients()` with and without histograms, `grad_norm`, `clip_grad_norm_` when it clips (every call asks for 0.9 times
    the norm the call before left) and when it does not (max_norm above the norm): milliseconds
    per call and the effective read bandwidth, counting the selected floats once per pass over them (statistics 1 pass, with
    histograms 2, the norm 1, clipping 2; clipping also writes them once, which is not counted; STATS' own traffic is negligible);
  * the per-tensor torch loop `wandb.watch(log="all")` amounts to on the GPU - min, max, both copied to the host, `histc(64)`, copied
    to the host - over the same gradients, and `torch.nn.utils.clip_grad_norm_(model.parameters(), ...)`; the ratios.
Every timing is a host clock around `iters` calls that end in a device synchronise, after warm-up calls of the same shape (the torch
loops synchronise per tensor by construction); a call of ours is a few launches whose enqueue costs more host time than the kernels
take, so the device time of the call's stages (HIP events around every stage, median of 20 calls, taken separately) stands next to
it, and the bandwidth is bytes over THAT.  A buffer below 256 MB (U-Net b5: 161 MB) can stay in the Infinity Cache between calls.  The parent process never touches the GPU: every model is measured by a child process
of its own under a time limit, and the first child that fails ends the run."""
import argparse
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
MODELS = ("unet_b5", "prithvi_100m")
CHILD_LIMIT = 420       # seconds per model


def build(name, dev):
    import torch

    import s2lc_amd  # noqa: F401

    torch.manual_seed(0)
    if name == "unet_b5":
        from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet

        model = EfficientnetUnet(EfficientNetConfig("b5", 13, 4, class_distribution=[0.25] * 4))
    elif name == "prithvi_100m":
        from s2lc_amd.modules.prithvi import MaskedAutoencoderViT
        from s2lc_amd.utils import _prithvi_model_args

        model = MaskedAutoencoderViT(**_prithvi_model_args(1))
    else:
        raise SystemExit(f"unknown model {name}")
    model.to(dev).train()
    g = model._grad_buffer()
    g.normal_(0.0, 1e-3)
    model._publish_grads(model._no_grad_params)         # what a backward leaves behind: .grad views into the flat gradient buffer
    return model


def timed(fn, iters, warm=3):
    import torch

    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def child(name, iters, runs):
    import torch

    import numpy as np

    from s2lc_amd import _lib
    from s2lc_amd import flat_stats as FS

    if not torch.cuda.is_available():
        raise SystemExit("bench_flat_stats.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    model = build(name, dev)
    stats = FS.FlatStats(model, bins=64)
    sel = stats.gradients(hist=False)
    n = sum(sel.numel)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) == len(sel.names)
    norm0 = float(FS.grad_norm(model))
    print(f"{name}: {len(sel.names)} gradient tensors, {n / 1e6:.2f} M floats ({n * 4 / 1e6:.1f} MB), norm {norm0:.4f}, {iters} timed calls, "
          f"{torch.cuda.get_device_name(0)}", flush=True)

    def watch_loop():
        for t in grads:
            lo, hi = t.min().item(), t.max().item()
            torch.histc(t, bins=64, min=lo, max=hi).cpu()

    calls = [0]

    def refill():
        model._grad_buffer().normal_(0.0, 1e-3)
        calls[0] = 0

    def clipping(clip):
        """every call clips: after k calls the norm is norm0 * 0.9^k, so call k + 1 asks for norm0 * 0.9^(k + 1)"""
        def fn():
            calls[0] += 1
            return clip(norm0 * 0.9 ** calls[0])
        return fn

    def device_ms(fn, reps=20):
        """median over `reps` calls of the per-stage device times (HIP events around every stage: `_lib.profile_ops` in place of
        `_lib.run`), summed over the call's stages"""
        rec = []
        run = _lib.run
        _lib.run = lambda packed, bases, stream: rec.append(_lib.profile_ops(packed, bases, stream))
        try:
            for _ in range(reps + 2):
                fn()
        finally:
            _lib.run = run
        torch.cuda.synchronize()
        per_stage = np.median(np.stack(rec[2:]), axis=0)
        return float(per_stage.sum()), per_stage

    for run in range(runs):
        print(f"-- run {run + 1} of {runs}", flush=True)
        rows = [("gradients() stats only", lambda: stats.gradients(hist=False), 1),
                ("gradients() stats + hist", lambda: stats.gradients(), 2),
                ("grad_norm", lambda: FS.grad_norm(model), 1),
                ("clip_grad_norm_, not clipping", lambda: FS.clip_grad_norm_(model, 1e6), 1),
                ("clip_grad_norm_, clipping", clipping(lambda m: FS.clip_grad_norm_(model, m)), 2)]
        ms = {}
        for label, fn, passes in rows:
            refill()
            ms[label] = timed(fn, iters)
            refill()
            dev_ms, per_stage = device_ms(fn)
            print(f"  {label:32s} {ms[label]:8.4f} ms per call   device {dev_ms:7.4f} ms ({' + '.join(f'{v:.4f}' for v in per_stage)})   "
                  f"{passes * n * 4 / dev_ms / 1e9:6.3f} TB/s read", flush=True)
        refill()
        t_watch = timed(watch_loop, max(1, iters // 10), warm=1)
        refill()
        t_clip = timed(clipping(lambda m: torch.nn.utils.clip_grad_norm_(model.parameters(), m)), iters)
        refill()
        t_noclip = timed(lambda: torch.nn.utils.clip_grad_norm_(model.parameters(), 1e6), iters)
        print(f"  torch per-tensor min / max / histc loop {t_watch:8.3f} ms   = {t_watch / ms['gradients() stats + hist']:7.1f}x gradients() with hist")
        print(f"  torch clip_grad_norm_, clipping         {t_clip:8.3f} ms   = {t_clip / ms['clip_grad_norm_, clipping']:7.1f}x")
        print(f"  torch clip_grad_norm_, not clipping     {t_noclip:8.3f} ms   = {t_noclip / ms['clip_grad_norm_, not clipping']:7.1f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3, help="repeat the whole table (the spread between runs is the noise of a figure)")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.iters, a.runs)
        return
    for name in a.models.split(","):
        # a fresh process per model, under its own time limit; nothing more is started after one that failed
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, str(Path(__file__).resolve()), "--child", name,
                            "--iters", str(a.iters), "--runs", str(a.runs)])
        if r.returncode != 0:
            raise SystemExit(f"{name}: the measuring process ended with status {r.returncode}; stopping")


if __name__ == "__main__":
    main()
