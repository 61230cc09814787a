"""Throughput of the on-GPU tile quicklooks (TILE_RADIX_HIST / TILE_RANK_PICK / TILE_QUICKLOOK behind GpuTilePipeline.band_percentiles,
.zero_fraction, .quicklook) over N resident 6 x 512 x 512 int16 tiles, against torch's sort / kthvalue over the same groups on the same
device and the numpy path after a device-to-host copy, with TILE_PREP - the other HBM-bound kernel of the input pipeline - timed in the
same run as the yardstick.

    python tools/bench_quicklook.py [--tiles 2048] [--iters 10] [--data sentinel|uniform]

Times are HIP events around whole method calls (the host's uploads, the result download and the host derivation included); bytes are
what the stages must read, computed from the shapes: a selection reads its groups TWICE (the coarse and the fine pass).  The tiles
are generated on the device: 2048 of them are 6.4 GB.  "sentinel": 30 % nodata zeros in 64 x 64 patches, reflectances 1..4000 smooth
over 8 x 8 patches plus noise; "uniform": the whole int16 range, every pixel independent (no runs to combine, no hot bin)."""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from s2lc_amd.data import quicklook as QL  # noqa: E402
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline  # noqa: E402
from s2lc_amd.stage_call import StageCall  # noqa: E402


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


def report(name, ms, byts, what="read"):
    print(f"{name:56s} {ms:9.3f} ms   {byts / 1e9:8.3f} GB {what:5s}  {byts / ms / 1e9:6.3f} TB/s", flush=True)


def make_tiles(N, C, H, kind, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    raw = torch.empty(N, C, H, H, dtype=torch.int16, device=dev)
    for i in range(0, N, 64):
        n = min(64, N - i)
        if kind == "uniform":
            raw[i:i + n] = torch.randint(-32768, 32768, (n, C, H, H), generator=g, device=dev, dtype=torch.int32).to(torch.int16)
            continue
        smooth = torch.randint(1, 3800, (n, C, H // 8, H // 8), generator=g, device=dev, dtype=torch.int32)
        smooth = smooth.repeat_interleave(8, 2).repeat_interleave(8, 3) + torch.randint(0, 200, (n, C, H, H), generator=g, device=dev, dtype=torch.int32)
        nodata = (torch.rand(n, 1, H // 64, H // 64, generator=g, device=dev) < 0.3).repeat_interleave(64, 2).repeat_interleave(64, 3)
        raw[i:i + n] = torch.where(nodata, torch.zeros_like(smooth), smooth).to(torch.int16)
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--data", default="sentinel", choices=["sentinel", "uniform"])
    ap.add_argument("--selection-only", action="store_true", help="stop after the selection lines (comparing tuning-build switches)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quicklook.py needs a GPU (there is no CPU fallback)")
    N, C, H, S, B = a.tiles, 6, 512, 224, 256
    dev = torch.device("cuda")
    raw = make_tiles(N, C, H, a.data, dev)
    pipe = GpuTilePipeline([0.05] * C, [0.02] * C, random_crop_size=S, augment=True, random_horizontal_flip_p=0.5,
                           random_vertical_flip_p=0.5, squeeze_time_dim=True)
    pipe.load(raw, None)
    rgb, q = (2, 1, 0), [2.0, 98.0]
    print(f"{N} tiles of {C} x {H} x {H} int16 ({raw.numel() * 2 / 1e9:.2f} GB), {a.data} data, {a.iters} timed calls each, "
          f"{torch.cuda.get_device_name(0)}")
    plane = H * H * 2
    ms_tile = timed(lambda: pipe.band_percentiles(q, bands=rgb, pooled=False), a.iters)
    report("band_percentiles per tile, bands (2,1,0), q (2,98)", ms_tile, 2 * N * 3 * plane)
    ms_pool = timed(lambda: pipe.band_percentiles(q, pooled=True), a.iters)
    report("band_percentiles pooled, 6 bands, q (2,98)", ms_pool, 2 * N * C * plane)
    report("zero_fraction band 0", timed(lambda: pipe.zero_fraction(), a.iters), N * plane)
    if a.selection_only:
        return

    gh = torch.Generator().manual_seed(0)
    par = pipe.draw_params(torch.randint(0, N, (B,), generator=gh), training=True, generator=gh)
    ntile = len(set(par[:, 0].tolist()))
    ms = timed(lambda: pipe.quicklook(params=par), a.iters)
    report(f"quicklook B={B} crops {S} (selection of {ntile} tiles + stretch)", ms, 2 * ntile * 3 * plane + B * S * S * 3 * 3, "moved")
    # the stretch stage alone, bounds given
    pct = torch.tensor([[100.0, 3000.0]] * B, dtype=torch.float64, device=dev)
    out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    call = StageCall()
    QL.add_quicklook(call, raw, par, torch.arange(B, dtype=torch.int32), rgb, call.t(pct), out, B)
    call.pack()
    stream = torch.cuda.current_stream().cuda_stream
    report(f"TILE_QUICKLOOK stage alone, B={B} crops {S}", timed(lambda: call.run(stream), a.iters), B * S * S * 3 * (2 + 1), "moved")
    byts = B * S * S * C * (2 + 4)
    ms = timed(lambda: pipe(params=par), a.iters)
    report(f"TILE_PREP B={B} (yardstick, read + written)", ms, byts, "moved")

    # ---- baselines over the same groups, same device --------------------------------------------------------------------------
    nb = min(N, 64)                               # torch.sort returns int64 indices beside the values: 64 tiles are 0.4 GB of them
    grp = raw[:nb][:, list(rgb)].reshape(nb, -1).contiguous()
    n = grp.shape[1]
    ranks = [int(0.02 * (n - 1)), int(0.02 * (n - 1)) + 1, int(0.98 * (n - 1)), int(0.98 * (n - 1)) + 1]
    ms_sort = timed(lambda: torch.sort(grp, dim=1).values[:, ranks].cpu(), max(2, a.iters // 2)) / nb
    ms_kth = timed(lambda: [torch.kthvalue(grp, r + 1, dim=1).values.cpu() for r in ranks], max(2, a.iters // 2)) / nb
    ours = ms_tile / N
    print(f"per tile (3 bands jointly, 4 ranks): selection {ours * 1e3:8.2f} us   torch.sort {ms_sort * 1e3:8.2f} us ({ms_sort / ours:5.1f}x)   "
          f"torch.kthvalue x4 {ms_kth * 1e3:8.2f} us ({ms_kth / ours:5.1f}x)      [torch on {nb} tiles, gathered copy not timed]")
    band = raw[:, 0].reshape(-1)                  # one band over all tiles: the pooled group (a strided gather, made contiguous untimed)
    nn = band.numel()
    rp = [int(0.02 * (nn - 1)), int(0.98 * (nn - 1))]
    ms_psort = timed(lambda: torch.sort(band).values[rp].cpu(), 2)
    print(f"per band pooled over {N} tiles: selection {ms_pool / C:9.3f} ms   torch.sort {ms_psort:9.3f} ms ({ms_psort / (ms_pool / C):5.1f}x)")
    t0 = time.perf_counter()
    k = min(N, 8)
    for i in range(k):
        np.percentile(raw[i][list(rgb)].cpu().numpy(), (2, 98))
    ms_np = (time.perf_counter() - t0) * 1e3 / k
    print(f"numpy after a device-to-host copy, per tile: {ms_np * 1e3:8.2f} us ({ms_np / ours:5.1f}x)")


if __name__ == "__main__":
    main()
