"""Throughput of WINDOW_BLEND (csrc/predict.hip), the stage behind predict.TilePredictor, alone: 512 x 512 tiles predicted as
224 x 224 windows at stride 112 (4 x 4 windows per tile, one flip variant), K = 4 and 23 classes, logits (MODE 0) and softmax
(MODE 1) blending, for the three launches TilePredictor issues: MASK (predict, no HIST), HIST (evaluate: the fused confusion counts
as the only output) and BLEND (predict_blend).  Next to each: a plain-torch assembly of the same result from slice-adds, and
TILE_PREP - the other HBM-bound kernel of the input side - timed in the same run as the bandwidth yardstick.

    python tools/bench_predict.py [--gib 2.0] [--iters 10] [--runs 1]

Times are HIP events around `iters` launches of one packed record; TB/s counts the bytes of LOGITS only (read exactly once), the
tile count per launch is chosen so that LOGITS holds about `--gib` GiB - far beyond the 256 MiB Infinity Cache."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from s2lc_amd import predict as P  # noqa: E402
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline  # noqa: E402
from s2lc_amd.stage_call import StageCall  # noqa: E402

H = W = 512
S, STRIDE = 224, 112


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def stage(logits, ys, xs, w1, mode, out, labels, index, lut):
    """a callable that launches one WINDOW_BLEND (predict.add_window_blend) over `logits` [M, 1, NY, NX, K, S, S] writing the output
    named `out`"""
    dev = logits.device
    M, K = logits.shape[0], logits.shape[4]
    blend = torch.empty(M, K, H, W, dtype=torch.float32, device=dev) if out == "blend" else None
    mask = torch.empty(M, H, W, dtype=torch.int64, device=dev) if out == "mask" else None
    hist = torch.zeros(K, K, dtype=torch.int64, device=dev) if out == "hist" else None
    call = StageCall()
    P.add_window_blend(call, logits, ys, xs, [0], w1, mode, H, W, labels.shape[0], blend, mask, labels, index, lut, hist)
    call.pack()
    stream = torch.cuda.current_stream(dev).cuda_stream
    return lambda: call.run(stream)


def torch_assembly(logits, ys, xs, w1, mode, out, labels, index, lut):
    """the same result from plain torch: one slice-add per window into a [M, K, H, W] accumulator, then divide / argmax / bincount"""
    M, _, NY, NX, K = logits.shape[:5]
    w2 = w1[:, None] * w1[None, :]

    def run():
        acc = torch.zeros(M, K, H, W, dtype=torch.float32, device=logits.device)
        ws = torch.zeros(H, W, dtype=torch.float32, device=logits.device)
        for i, y0 in enumerate(ys):
            for j, x0 in enumerate(xs):
                v = logits[:, 0, i, j]
                if mode:
                    v = torch.softmax(v, dim=1)
                acc[:, :, y0:y0 + S, x0:x0 + S] += w2 * v
                ws[y0:y0 + S, x0:x0 + S] += w2
        acc /= ws
        if out == "blend":
            return acc
        mask = acc.argmax(dim=1)
        if out == "mask":
            return mask
        t = lut.long()[labels[index.long().to(labels.device)].long()]
        ok = t < K
        return torch.bincount((t[ok] * K + mask[ok]), minlength=K * K)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0, help="size of the LOGITS buffer per launch")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--runs", type=int, default=1, help="repeat the whole table (the spread between runs is the noise of a figure)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    ys, xs = P.window_origins(H, S, STRIDE), P.window_origins(W, S, STRIDE)
    w1 = P.window_profile(S, "hann").to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    print(f"{H} x {W} tiles, windows {S} at stride {STRIDE} ({len(ys)} x {len(xs)} per tile), {a.iters} timed launches each, "
          f"{torch.cuda.get_device_name(0)}")
    for run in range(a.runs):
        print(f"-- run {run + 1} of {a.runs}")
        for K in (4, 23):
            per_tile = len(ys) * len(xs) * K * S * S
            M = max(1, min(int(a.gib * (1 << 30) / 4) // per_tile, P.MAX_LOGITS // per_tile))
            logits = torch.empty(M, 1, len(ys), len(xs), K, S, S, dtype=torch.float32, device=dev)
            for m in range(M):
                logits[m].normal_(0, 3, generator=g)
            labels = torch.randint(0, 24, (M, H, W), generator=g, device=dev, dtype=torch.uint8)
            index = torch.arange(M, dtype=torch.int32)
            lut = (torch.arange(256, dtype=torch.int32) % 24 % K).to(dev)
            byts = logits.numel() * 4
            print(f"K = {K}: {M} tiles per launch, LOGITS {byts / 1e9:.3f} GB")
            for mode in (0, 1):
                for out in ("mask", "hist", "blend"):
                    args = (logits, ys, xs, w1, mode, out, labels, index, lut)
                    ms = timed(stage(*args), a.iters)
                    ms_t = timed(torch_assembly(*args), max(1, a.iters // 3))
                    print(f"  MODE {mode} -> {out:5s}  {ms:8.3f} ms  {byts / ms / 1e9:6.3f} TB/s of LOGITS   torch assembly {ms_t:8.3f} ms  "
                          f"= {ms_t / ms:5.1f}x")
            del logits, labels
        # the yardstick: TILE_PREP, bytes read + written
        N, C, B = 256, 6, 256
        raw = torch.randint(0, 9000, (N, C, H, W), generator=g, device=dev, dtype=torch.int16)
        lab = torch.randint(0, 24, (N, H, W), generator=g, device=dev, dtype=torch.uint8)
        pipe = GpuTilePipeline([0.05] * C, [0.02] * C, random_crop_size=S, augment=True, random_horizontal_flip_p=0.5,
                               random_vertical_flip_p=0.5, label_map="cnes-multiclass", squeeze_time_dim=True)
        pipe.load(raw, lab)
        gh = torch.Generator().manual_seed(0)
        par = pipe.draw_params(torch.randint(0, N, (B,), generator=gh), training=True, generator=gh)
        byts = B * S * S * (C * (2 + 4) + 1 + 8)
        ms = timed(lambda: pipe(params=par), a.iters)
        print(f"TILE_PREP B={B} (yardstick, read + written)  {ms:8.3f} ms  {byts / 1e9:6.3f} GB moved  {byts / ms / 1e9:6.3f} TB/s")
        del raw, lab, pipe


if __name__ == "__main__":
    main()
