"""The U-Net training step (b5, 13 x 256 x 256, bs 32: bench.py's workload) in "f32" and "f32-split" in one process, same weights,
same batch, driver-timed (bench.py time_steps: synchronize on both sides), in alternating rounds so that clock / thermal drift
(DVFS on random data) hits both modes alike.  Step = forward + focal loss + backward + fused Adam.
    python tools/bench_precision.py [--batch 32] [--steps 20] [--warmup 5] [--rounds 3]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from bench import time_steps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="f32,f32-split")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from s2lc_amd.losses import FocalLoss
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet
    from s2lc_amd.optim import FlatAdam

    torch.manual_seed(0)
    B, H = a.batch, a.size
    x = torch.randn(B, 13, H, H, device=dev)
    y = torch.randint(0, 4, (B, H, H), device=dev)
    lossf = FocalLoss(torch.ones(4), 2.0, 0.0, ignore_index=0)
    modes = a.modes.split(",")
    models = {}
    for mode in modes:
        torch.manual_seed(1)
        m = EfficientnetUnet(EfficientNetConfig("b5", 13, 4, class_distribution=[0.25] * 4)).to(dev).train()
        m.precision = mode
        models[mode] = (m, FlatAdam(m, lr=1e-4))

    def stepper(mode):
        m, opt = models[mode]

        def step():
            opt.zero_grad()
            lossf(m(x), y).backward()
            opt.step()
        return step

    for mode in modes:
        time_steps(stepper(mode), a.warmup, None, dev)
    res = {mode: [] for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            res[mode].append(time_steps(stepper(mode), a.steps, None, dev) / a.steps)
    out = {"workload": f"unet-b5 13x{H}x{H} bs{B} train step", "rounds": a.rounds, "steps_per_round": a.steps}
    for mode in modes:
        best = min(res[mode])
        out[mode] = {"ms_per_step": round(best * 1e3, 3), "tiles_per_s": round(B / best, 1),
                     "ms_per_round": [round(t * 1e3, 3) for t in res[mode]]}
    if "f32" in res and "f32-split" in res:
        out["split_speedup"] = round(min(res["f32"]) / min(res["f32-split"]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
