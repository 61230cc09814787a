"""Where the f32-split kernels win: every CONV / WGRAD stage of a U-Net b5 training step (13 x 256 x 256, bs 32 by default) timed
on the kernel its launcher picks in the "f32" plan and on the split kernels (the same stage with FLAG_SPLIT: plan/split.py with
every shape class routed), summed per shape class of plan/split.py.  The ROUTE table there is read off this output.
    python tools/exp_split_mfma.py [--batch 32] [--reps 3] [--out profiles/split_mfma.md]"""
import argparse
import collections
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from s2lc_amd import _lib  # noqa: E402
from s2lc_amd.plan import opdefs as D  # noqa: E402
from s2lc_amd.plan import split as SP  # noqa: E402


def stage_times(model, B, H, reps, dev):
    """(per-stage ms of the forward and backward programs, minimum over reps; the plan's (kind, fields) lists)"""
    x = torch.randn(B, 13, H, H, device=dev)
    model(x)
    eng = next(iter(model._engines.values()))
    st = torch.cuda.current_stream().cuda_stream
    noise = torch.rand(eng.n_noise_rows, B, device=dev)
    out = torch.empty(eng.plan.logits_shape, device=dev)
    dout = torch.randn(eng.plan.logits_shape, device=dev) * 1e-3
    grads = torch.zeros_like(model._flat_params)
    res = []
    for prog, ops, bases in ((eng.fwd, eng.plan.fwd.ops, eng.bases(model, x, out, noise=noise)),
                             (eng.bwd, eng.plan.bwd.ops, eng.bases(model, x, None, dout=dout, noise=noise, grads=grads))):
        best = None
        for _ in range(reps):
            ms, var = _lib.profile_variants(prog, bases, st)
            best = ms if best is None else np.minimum(best, ms)
        res.append((best, var, ops))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from s2lc_amd.modules.efficientnet_unet import EfficientNetConfig, EfficientnetUnet

    torch.manual_seed(0)
    model = EfficientnetUnet(EfficientNetConfig("b5", 13, 4, class_distribution=[0.25] * 4)).to(dev).train()
    saved = dict(SP.ROUTE)
    SP.ROUTE.update({k: True for k in SP.ROUTE})
    try:
        t32 = stage_times(model, a.batch, a.size, a.reps, dev)
        model.precision = "f32-split"
        tsp = stage_times(model, a.batch, a.size, a.reps, dev)
    finally:
        SP.ROUTE.clear()
        SP.ROUTE.update(saved)
    cls = collections.defaultdict(lambda: [0, 0.0, 0.0])
    rows = []
    for (ms32, var32, ops), (mss, vars_, opss) in zip(t32, tsp):
        for i, (kind, f) in enumerate(opss):
            if kind not in ("CONV", "WGRAD") or not f.get("_flags", 0) & D.FLAG_SPLIT:
                continue
            c = SP.shape_class(kind, f)
            cls[c][0] += 1
            cls[c][1] += float(ms32[i])
            cls[c][2] += float(mss[i])
            shape = f"{f['B']}x{f.get('C1', f.get('C'))}x{f['H']}x{f['W']}->{f['M']} k{f['KH']}"
            rows.append((c, kind, shape, int(var32[i]), float(ms32[i]) * 1e3, float(mss[i]) * 1e3))
    lines = [f"# f32-split vs f32 kernels per stage class (U-Net b5, 13 x {a.size} x {a.size}, bs {a.batch}, training step, "
             f"min of {a.reps} profiled runs)", "",
             "| class | stages | f32 kernels ms | split ms | split / f32 |", "|---|---|---|---|---|"]
    for c, (n, m32, msp) in sorted(cls.items()):
        lines.append(f"| {c} | {n} | {m32:.3f} | {msp:.3f} | {msp / max(m32, 1e-9):.3f} |")
    tot32 = sum(v[1] for v in cls.values())
    totsp = sum(v[2] for v in cls.values())
    lines += ["", f"all flagged stages: f32 {tot32:.3f} ms, split {totsp:.3f} ms", "",
              "| class | kind | shape | f32 family | f32 us | split us |", "|---|---|---|---|---|---|"]
    lines += [f"| {c} | {k} | {s} | {v} | {u32:.1f} | {usp:.1f} |" for c, k, s, v, u32, usp in rows]
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        Path(a.out).write_text(txt)


if __name__ == "__main__":
    main()
