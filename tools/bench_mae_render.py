"""Time of the MAE reconstruction pictures (render.mae_panels: one launch of s2k_mae_panels, csrc/mae_render.hip) at Prithvi's own
shape - 64 samples of 6 x 1 x 224 x 224, 16 x 16 patches, mask ratio 0.75, four panels - against the torch expression of the same
result on the same device and seeded inputs, alternating with it in the same run.

    python tools/bench_mae_render.py [--batch 64] [--iters 500] [--reps 5]

Times are HIP events around `iters` whole calls (output allocation and the host's argument checks included) after a warm-up; every
configuration is timed `reps` times, alternating with its baseline, and the median and the range are printed.  Bytes are algorithmic,
from the shapes: what the result depends on and what is written.  Without norm_pix / patch_mse that is three of the six channels of
imgs and of pred; pred interleaves its channels, so the lines the kernel touches hold all six ("touched").  The torch baseline is
`unpatchify`, `where` on the mask, the affine de-normalisation, the stretch, `clamp`, `to(uint8)`: in float64 it gives the same bytes
(compared before timing; with norm_pix up to one level apart where a value sits on an integer), in float32 - what one would write
without thinking about it - pictures that differ by one level in places.  Nothing here is a pass bar."""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import s2lc_amd  # noqa: E402,F401
from s2lc_amd import render  # noqa: E402
from s2lc_amd.modules.prithvi import MaskedAutoencoderViT  # noqa: E402

COPY_CEILING = 6.3e12      # bytes / s, the float4 stream copy of an MI355X
RGB = [2, 1, 0]


def timed(fn, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def torch_panels(model, x, pred, mask, norm, bounds, dtype, want_mse, fill=128):
    s = model.spec
    B, P, g = x.shape[0], s.patch_size, s.img_size // s.patch_size
    full = pred.to(dtype)
    target = None
    if s.norm_pix_loss or want_mse:
        target = model.patchify(x).to(dtype)
    if s.norm_pix_loss:
        mean, sd = target.mean(-1, keepdim=True), (target.var(-1, keepdim=True) + 1e-6).sqrt()
        target = (target - mean) / sd
        full = full * sd + mean
    mse = ((pred.to(dtype) - target) ** 2).mean(-1).float() if want_mse else None
    rec, org = model.unpatchify(full)[:, RGB, 0], x[:, RGB, 0].to(dtype)
    rem = (mask.reshape(B, 1, g, g) != 0).repeat_interleave(P, 2).repeat_interleave(P, 3)
    m, r = norm[0][RGB].to(dtype).view(1, 3, 1, 1), norm[1][RGB].to(dtype).view(1, 3, 1, 1)
    lo, hi = bounds[:, 0].to(dtype).view(B, 1, 1, 1), bounds[:, 1].to(dtype).view(B, 1, 1, 1)

    def stretch(v):
        return (((v / r + m) - lo) / (hi - lo) * 255.0).clamp(0.0, 255.0).to(torch.uint8)

    o, c = stretch(org), stretch(rec)
    out = torch.stack([o, torch.where(rem, torch.full_like(o, fill), o), torch.where(rem, c, o), c], 1).permute(0, 1, 3, 4, 2).contiguous()
    return out, mse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mae_render.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda")
    B, C, S, P = a.batch, 6, 224, 16
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C, 1, S, S, generator=g).to(dev)
    L, PD = (S // P) ** 2, P * P * C
    ids = torch.rand(B, L, generator=g).argsort(1)
    mask = (ids >= L - int(L * 0.75)).float().to(dev)            # 0.75 of every sample's patches removed
    noise = torch.randn(B, L, PD, generator=g).to(dev)
    norm = torch.stack([torch.rand(C, generator=g) * 1000 + 500, 1.0 / (torch.rand(C, generator=g) * 400 + 200)]).float().to(dev)
    bounds = torch.tensor([[400.0 + b, 1800.0 + 2 * b] for b in range(B)], dtype=torch.float64, device=dev)
    print(f"{B} samples of {C} x 1 x {S} x {S}, patches {P} x {P}, mask ratio 0.75, four panels, {a.iters} calls per window, "
          f"{a.reps} windows each, {torch.cuda.get_device_name(0)}")
    print(f"{'configuration':34s} {'ms median (min .. max)':>28s} {'GB':>7s} {'TB/s':>6s} {'of 6.3':>7s} {'touched GB':>10s}   baselines: torch f64, torch f32")
    pix = B * S * S
    for norm_pix in (False, True):
        model = MaskedAutoencoderViT(img_size=S, patch_size=P, num_frames=1, tubelet_size=1, in_chans=C, embed_dim=16, depth=1, num_heads=2,
                                     decoder_embed_dim=16, decoder_depth=1, decoder_num_heads=2, norm_pix_loss=norm_pix)
        patches = model.patchify(x)
        if norm_pix:
            patches = (patches - patches.mean(-1, keepdim=True)) / (patches.var(-1, keepdim=True) + 1e-6).sqrt()
        pred = (patches + 0.1 * noise).contiguous()
        for want_mse in (False, True):
            ours = lambda: render.mae_panels(model, x, pred, mask, norm, bounds, patch_mse=want_mse)      # noqa: E731
            base = {dt: (lambda dt=dt: torch_panels(model, x, pred, mask, norm, bounds, dt, want_mse)) for dt in (torch.float64, torch.float32)}
            got = ours()
            got, got_mse = got if want_mse else (got, None)
            for dt, fn in base.items():
                ref, ref_mse = fn()
                d = (got.int() - ref.int()).abs()
                line = f"  against torch {str(dt)[6:]}: {int((d != 0).sum())} of {d.numel()} bytes differ, largest difference {int(d.max())}"
                if want_mse:
                    line += f"; PATCH_MSE largest relative difference {float(((got_mse - ref_mse).abs() / ref_mse.abs().max()).max()):.1e}"
                print(line)
            for fn in (ours, *base.values()):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in ("ours", torch.float64, torch.float32)}
            for _ in range(a.reps):                                   # alternating: every window of ours beside one of each baseline
                ms["ours"].append(timed(ours, a.iters))
                for dt, fn in base.items():
                    ms[dt].append(timed(fn, max(2, a.iters // 5)))
            whole = norm_pix or want_mse                              # the patch sums need every channel of imgs
            read_imgs = pix * (C if whole else 3) * 4
            read_pred = pix * (C if want_mse else 3) * 4
            written = 4 * pix * 3 + (B * L * 4 if want_mse else 0)
            byts = read_imgs + read_pred + written + B * L * 4
            touched = read_imgs + pix * C * 4 + written + B * L * 4
            med = statistics.median(ms["ours"])
            span = f"{med:8.4f} ({min(ms['ours']):.4f} .. {max(ms['ours']):.4f})"
            tail = ", ".join(f"{statistics.median(ms[dt]):8.3f} ms ({statistics.median(ms[dt]) / med:5.1f}x)" for dt in (torch.float64, torch.float32))
            print(f"norm_pix={int(norm_pix)} patch_mse={int(want_mse):d}{'':12s} {span:>28s} {byts / 1e9:7.4f} {byts / med / 1e9:6.3f} "
                  f"{100.0 * byts / (med * 1e-3) / COPY_CEILING:6.1f}% {touched / 1e9:10.4f}   {tail}", flush=True)
            print(f"  reads: imgs {read_imgs / 1e6:.1f} MB, pred {read_pred / 1e6:.1f} MB (touched {pix * C * 4 / 1e6:.1f} MB); written {written / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
