"""Throughput of the on-GPU dataset statistics (TILE_MOMENTS / TILE_LABEL_HIST behind GpuTilePipeline.band_mean_std,
.label_histogram, .sample_weights) over N resident 6 x 512 x 512 int16 tiles + label rasters, with TILE_PREP - the other HBM-bound
kernel of the input pipeline - timed in the same run as the yardstick.

    python tools/bench_stats.py [--tiles 2048] [--iters 10]

Times are HIP events around whole method calls (the host's index upload, the result download and the host derivation included),
bytes are what the stage must read, computed from the shapes.  The tiles are generated on the device: 2048 of them are 6.4 GB."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline  # noqa: E402


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


def report(name, ms, byts):
    print(f"{name:44s} {ms:9.3f} ms   {byts / 1e9:8.3f} GB read   {byts / ms / 1e9:6.3f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stats.py needs a GPU (there is no CPU fallback)")
    N, C, H, S, K, B = a.tiles, 6, 512, 224, 4, 256
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    raw = torch.empty(N, C, H, H, dtype=torch.int16, device=dev)
    for i in range(0, N, 64):
        raw[i:i + 64] = torch.randint(0, 9000, raw[i:i + 64].shape, generator=g, device=dev, dtype=torch.int16)
    # land cover is spatially coherent: 32 x 32 patches of one CNES class; the random raster is the worst case for the histogram
    coherent = torch.randint(0, 24, (N, H // 32, H // 32), generator=g, device=dev, dtype=torch.uint8)
    coherent = coherent.repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous()
    random = torch.randint(0, 24, (N, H, H), generator=g, device=dev, dtype=torch.uint8)
    pipe = GpuTilePipeline([0.05] * C, [0.02] * C, random_crop_size=S, augment=True, random_horizontal_flip_p=0.5,
                           random_vertical_flip_p=0.5, label_map="cnes-multiclass", squeeze_time_dim=True)
    pipe.load(raw, coherent)
    print(f"{N} tiles of {C} x {H} x {H} int16 ({raw.numel() * 2 / 1e9:.2f} GB) + uint8 labels, {a.iters} timed calls each, "
          f"{torch.cuda.get_device_name(0)}")
    report("band_mean_std (TILE_MOMENTS)", timed(lambda: pipe.band_mean_std(), a.iters), N * C * H * H * 2)
    report("label_histogram tile, coherent labels", timed(lambda: pipe.label_histogram(K), a.iters), N * H * H)
    report(f"sample_weights center {S}, coherent labels", timed(lambda: pipe.sample_weights([0.25] * K), a.iters), N * S * S)
    pipe.load(raw, random)
    report("label_histogram tile, random labels", timed(lambda: pipe.label_histogram(K), a.iters), N * H * H)
    report(f"sample_weights center {S}, random labels", timed(lambda: pipe.sample_weights([0.25] * K), a.iters), N * S * S)
    gh = torch.Generator().manual_seed(0)
    par = pipe.draw_params(torch.randint(0, N, (B,), generator=gh), training=True, generator=gh)
    byts = B * S * S * (C * (2 + 4) + 1 + 8)
    ms = timed(lambda: pipe(params=par), a.iters)
    print(f"{'TILE_PREP B=' + str(B) + ' (yardstick, read + written)':44s} {ms:9.3f} ms   {byts / 1e9:8.3f} GB moved  {byts / ms / 1e9:6.3f} TB/s")


if __name__ == "__main__":
    main()
