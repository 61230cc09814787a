// MAE reconstruction pictures on the GPU (render.mae_panels; C entry s2k_mae_panels, include/s2k.h): what the model made of a crop, on
// the colour scale of GpuTilePipeline.quicklook.  The reference's MAE trainer logs `unpatchify(pred)[:3, 0][[2, 1, 0]]` beside the
// original every validation epoch (src/train_mae_prithvi.py:169-203) and leaves the masked input and the reconstruction pasted into the
// visible patches as a TODO; here the four panels - original, masked, pasted, reconstruction - and the per-patch squared error come
// from ONE launch over `imgs`, `pred` and `mask` as MaskedAutoencoderViT.forward leaves them on the device.
//
// Per output pixel (i, j) of sample b, colour k, c = BANDS[k]:  t = frame / TUB, tt = frame % TUB, l = (t*g + i/P)*g + j/P,
// e = ((tt*P + i%P)*P + j%P)*C + c;  x_orig = IMGS[b][c][frame][i][j], x_pred = PRED[b][l][e] (with norm_pix: x_pred*sqrt(var + 1e-6) +
// mean over the patch's PD features of IMGS, unbiased variance, f64);  v = x / NORM[1][c] + NORM[0][c] in f64 (the inverse of
// TILE_PREP);  OUT = (uint8) trunc(clip((v - lo) / (hi - lo) * 255, 0, 255)), TILE_QUICKLOOK's stretch, every operation rounded on its
// own.  Bounds without a range and a NaN give 0.  PATCH_MSE[b][l] = mean over PD of (PRED - target)^2 for EVERY patch: the masked mean
// of it is the model's loss.
//
// One wave per patch, the four waves of a workgroup on neighbouring patches of one patch row: a patch's PRED row is PD contiguous
// floats, IMGS gives P contiguous floats per (channel, row), and OUT only 3*P contiguous bytes per patch row - the four waves together
// write 12*P.  The per-patch sums are wave reductions in f64 in a fixed lane order (no atomics): results repeat from run to run.
// All indexing derives from the dimensions the launcher validated; there are no index tables on the device.
#include "plain.h"

namespace s2k {

constexpr int MAE_PANEL_ORIGINAL = 0, MAE_PANEL_MASKED = 1, MAE_PANEL_PASTED = 2, MAE_PANEL_RECONSTRUCTION = 3;
constexpr int MAE_WAVES = NTHREADS / WAVE;       // patches per workgroup

struct MaePanelsP {
    const float* imgs;          // [B][C][T][H][W]
    const float* pred;          // [B][L][PD]
    const float* mask;          // [B][L]
    const float* norm;          // [2][C]
    const double* bounds;       // [B][2]
    unsigned char* out;         // [B][NP][H][W][3]
    float* mse;                 // [B][L] or null
    int C, T, H, W, P, TUB, G, L, PD, GW;      // G = H / P patches per side, GW = workgroups per patch row
    int HW, THW;                // elements per frame, per channel
    int frame, fill, NP;
    int bands[3], panel[4];
    int dc, dpx, dpy, dtt;      // 64 features further in (tt, py, px, c) order: 64 = ((dtt*P + dpy)*P + dpx)*C + dc
};

// feature e = ((tt*P + py)*P + px)*C + c of a patch, walked 64 at a time without a division per element
struct Feat {
    int c, px, py, tt;
    __device__ __forceinline__ void init(int e, int C, int P) {
        c = e % C; e /= C;
        px = e % P; e /= P;
        py = e % P; tt = e / P;
    }
    __device__ __forceinline__ void step(const MaePanelsP& p) {      // every carry is at most one: dc < C, dpx < P, dpy < P
        c += p.dc;   if (c >= p.C) { c -= p.C; ++px; }
        px += p.dpx; if (px >= p.P) { px -= p.P; ++py; }
        py += p.dpy; if (py >= p.P) { py -= p.P; ++tt; }
        tt += p.dtt;
    }
    __device__ __forceinline__ int img_off(const MaePanelsP& p) const { return c * p.THW + tt * p.HW + py * p.W + px; }
};

// TILE_QUICKLOOK's stretch of the de-normalised value: NaN -> 0, +inf -> 255, -inf -> 0
__device__ __forceinline__ unsigned char mae_stretch(double x, double rstd, double mean, double lo, double width, bool ok) {
#pragma clang fp contract(off)
    const double v = x / rstd + mean;
    double r = (v - lo) / width * 255.0;
    r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
    return (ok && r == r) ? (unsigned char)(int)r : (unsigned char)0;
}

// grid: (G * GW, 1 or T / TUB tubelet rows, B).  grid.y == 1: only the tubelet row of `frame` (nothing else is drawn); otherwise every
// patch, for PATCH_MSE.
template <bool NORM_PIX>
__global__ void __launch_bounds__(NTHREADS) mae_panels_kernel(const MaePanelsP p) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int pi = (int)(blockIdx.x / (unsigned)p.GW), pj = (int)(blockIdx.x - (unsigned)pi * (unsigned)p.GW) * MAE_WAVES + wave;
    if (pj >= p.G) return;                           // whole waves leave: there is no barrier below
    const int b = blockIdx.z, t0 = p.frame / p.TUB;
    const int t = gridDim.y == 1 ? t0 : (int)blockIdx.y;
    const int l = (t * p.G + pi) * p.G + pj;
    const float* prow = p.pred + ((int64_t)b * p.L + l) * p.PD;
    // channel 0, first frame of the tubelet, first pixel of the patch
    const float* ibase = p.imgs + (int64_t)b * p.C * p.THW + (int64_t)(t * p.TUB) * p.HW + (pi * p.P) * p.W + pj * p.P;

    double mean = 0.0, sd = 1.0;
    if (NORM_PIX) {
        // one pass, shifted by the patch's first value: the sums are of differences within the patch, so the subtraction in the
        // variance does not cancel whatever offset the patch carries
        const double k0 = (double)ibase[0];
        double s1 = 0.0, s2 = 0.0;
        Feat f;
        f.init(lane, p.C, p.P);
#pragma unroll 4
        for (int e = lane; e < p.PD; e += WAVE, f.step(p)) {
            const double d = (double)ibase[f.img_off(p)] - k0;
            s1 += d;
            s2 += d * d;
        }
        s1 = wave_sum_d(s1);
        s2 = wave_sum_d(s2);
        const double n = (double)p.PD;
        double var = (s2 - s1 * s1 / n) / (n - 1.0);
        if (var < 0.0) var = 0.0;
        mean = k0 + s1 / n;
        sd = sqrt(var + 1e-6);
    }

    if (p.mse) {
        double acc = 0.0;
        Feat f;
        f.init(lane, p.C, p.P);
#pragma unroll 4
        for (int e = lane; e < p.PD; e += WAVE, f.step(p)) {
            double target = (double)ibase[f.img_off(p)];
            if (NORM_PIX) target = (target - mean) / sd;
            const double d = (double)prow[e] - target;
            acc += d * d;
        }
        acc = wave_sum_d(acc);
        if (lane == 0) p.mse[(int64_t)b * p.L + l] = (float)(acc / (double)p.PD);
    }

    if (t != t0) return;
    const int tt0 = p.frame - t0 * p.TUB;
    const bool removed = p.mask[(int64_t)b * p.L + l] != 0.0f;
    const double lo = p.bounds[2 * b], hi = p.bounds[2 * b + 1];
    const bool ok = hi > lo && __builtin_isfinite(lo) && __builtin_isfinite(hi);
    const double width = hi - lo;
    const int qpr = (p.P + 3) >> 2;                  // a lane draws up to 4 neighbouring pixels of one patch row
    for (int q = lane; q < p.P * qpr; q += WAVE) {
        const int py = q / qpr, px = (q - py * qpr) * 4;
        const int n = p.P - px < 4 ? p.P - px : 4;
        unsigned char orig[12], reco[12];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int c = p.bands[k];
            const double bmean = (double)p.norm[c], brstd = (double)p.norm[p.C + c];
            const float* src = ibase + (c * p.THW + tt0 * p.HW + py * p.W + px);
            const float* pp = prow + ((int64_t)((tt0 * p.P + py) * p.P + px) * p.C + c);
            float xo[4] = {0.0f, 0.0f, 0.0f, 0.0f}, xp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (n == 4 && (reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
                const float4 u = *reinterpret_cast<const float4*>(src);
                xo[0] = u.x; xo[1] = u.y; xo[2] = u.z; xo[3] = u.w;
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (m < n) xo[m] = src[m];
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < n) xp[m] = pp[m * p.C];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                double r = (double)xp[m];
                if (NORM_PIX) r = r * sd + mean;
                orig[3 * m + k] = mae_stretch((double)xo[m], brstd, bmean, lo, width, ok);
                reco[3 * m + k] = mae_stretch(r, brstd, bmean, lo, width, ok);
            }
        }
        const int i = pi * p.P + py, j = pj * p.P + px;
        for (int s = 0; s < p.NP; ++s) {
            const int code = p.panel[s];
            unsigned char o[12];
#pragma unroll
            for (int m = 0; m < 12; ++m) {
                unsigned char v = orig[m];
                if (code == MAE_PANEL_RECONSTRUCTION || (code == MAE_PANEL_PASTED && removed)) v = reco[m];
                if (code == MAE_PANEL_MASKED && removed) v = (unsigned char)p.fill;
                o[m] = v;
            }
            unsigned char* dst = p.out + ((((int64_t)b * p.NP + s) * p.H + i) * p.W + j) * 3;
            if (n == 4 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
                unsigned int* d4 = reinterpret_cast<unsigned int*>(dst);
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    d4[m] = (unsigned int)o[4 * m] | ((unsigned int)o[4 * m + 1] << 8) | ((unsigned int)o[4 * m + 2] << 16) | ((unsigned int)o[4 * m + 3] << 24);
            } else {
#pragma unroll
                for (int m = 0; m < 12; ++m)
                    if (m < 3 * n) dst[m] = o[m];
            }
        }
    }
}

// Every argument checked and the kernel's parameters derived, in plain host code without a HIP call: s2k_mae_panels runs
// check_mae_panels before it as much as asks which device the stream belongs to, so a refused call has touched no device.
static int mae_panels_params(const float* imgs, const float* pred, const float* mask, const float* norm, const double* bounds,
                             unsigned char* out, float* patch_mse, int B, int C, int T, int H, int W, int P, int TUB, const int* bands,
                             int frame, const int* panels, int n_panels, int fill, int norm_pix, MaePanelsP& p) {
    if (!imgs || !pred || !mask || !norm || !bounds || !out || !bands || !panels) {
        set_error("mae_panels: null pointer (IMGS, PRED, MASK, NORM, BOUNDS, OUT, bands and panels are required)");
        return S2K_EFAULT;
    }
    if (B <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || P <= 0 || TUB <= 0) {
        set_error("mae_panels: bad dims (B, C, T, H, W, P and TUB must be positive)");
        return S2K_EINVAL;
    }
    if (H != W || H % P != 0 || T % TUB != 0) {
        set_error("mae_panels: bad dims (H == W, P divides H, TUB divides T)");
        return S2K_EINVAL;
    }
    const int64_t pd = (int64_t)TUB * P * P * C, sample = (int64_t)C * T * H * W;
    if (norm_pix != 0 && norm_pix != 1) { set_error("mae_panels: norm_pix must be 0 or 1"); return S2K_EINVAL; }
    if (norm_pix && pd < 2) { set_error("mae_panels: bad dims (norm_pix needs PD >= 2 features per patch: the variance is unbiased)"); return S2K_EINVAL; }
    if (n_panels < 1 || n_panels > 4) { set_error("mae_panels: 1 to 4 panels"); return S2K_EINVAL; }
    for (int s = 0; s < n_panels; ++s)
        if (panels[s] < MAE_PANEL_ORIGINAL || panels[s] > MAE_PANEL_RECONSTRUCTION) {
            set_error("mae_panels: bad panel code %d (0 original, 1 masked, 2 pasted, 3 reconstruction)", panels[s]);
            return S2K_EINVAL;
        }
    for (int k = 0; k < 3; ++k)
        if (bands[k] < 0 || bands[k] >= C) { set_error("mae_panels: band %d outside [0, %d)", bands[k], C); return S2K_EINVAL; }
    if (bands[0] == bands[1] || bands[0] == bands[2] || bands[1] == bands[2]) { set_error("mae_panels: the three bands must be distinct"); return S2K_EINVAL; }
    if (frame < 0 || frame >= T) { set_error("mae_panels: frame %d outside [0, %d)", frame, T); return S2K_EINVAL; }
    if (fill < 0 || fill > 255) { set_error("mae_panels: fill %d outside 0..255", fill); return S2K_EINVAL; }
    // launch grid (B and the tubelet rows are grid dimensions) and the 32-bit offsets inside one sample
    if (B > 65535 || T / TUB > 65535 || sample > 0x7fffffffll || (int64_t)n_panels * H * W * 3 > 0x7fffffffll) {
        set_error("mae_panels: bad dims (at most 65535 samples and tubelet rows, C*T*H*W and NP*H*W*3 below 2^31)");
        return S2K_EINVAL;
    }
    p = MaePanelsP{};
    p.imgs = imgs; p.pred = pred; p.mask = mask; p.norm = norm; p.bounds = bounds; p.out = out; p.mse = patch_mse;
    p.C = C; p.T = T; p.H = H; p.W = W; p.P = P; p.TUB = TUB;
    p.G = H / P;
    p.L = (T / TUB) * p.G * p.G;
    p.PD = (int)pd;
    p.GW = cdiv(p.G, MAE_WAVES);
    p.HW = H * W;
    p.THW = T * H * W;
    p.frame = frame; p.fill = fill; p.NP = n_panels;
    for (int k = 0; k < 3; ++k) p.bands[k] = bands[k];
    for (int s = 0; s < n_panels; ++s) p.panel[s] = panels[s];
    int r = WAVE;
    p.dc = r % C; r /= C;
    p.dpx = r % P; r /= P;
    p.dpy = r % P; p.dtt = r / P;
    return S2K_OK;
}

int check_mae_panels(const float* imgs, const float* pred, const float* mask, const float* norm, const double* bounds, unsigned char* out,
                     float* patch_mse, int B, int C, int T, int H, int W, int P, int TUB, const int* bands, int frame, const int* panels,
                     int n_panels, int fill, int norm_pix) {
    MaePanelsP p;
    return mae_panels_params(imgs, pred, mask, norm, bounds, out, patch_mse, B, C, T, H, W, P, TUB, bands, frame, panels, n_panels, fill,
                             norm_pix, p);
}

int launch_mae_panels(const float* imgs, const float* pred, const float* mask, const float* norm, const double* bounds, unsigned char* out,
                      float* patch_mse, int B, int C, int T, int H, int W, int P, int TUB, const int* bands, int frame, const int* panels,
                      int n_panels, int fill, int norm_pix, hipStream_t st) {
    MaePanelsP p;
    const int rc = mae_panels_params(imgs, pred, mask, norm, bounds, out, patch_mse, B, C, T, H, W, P, TUB, bands, frame, panels, n_panels,
                                     fill, norm_pix, p);
    if (rc != S2K_OK) return rc;
    const dim3 grid((unsigned)(p.G * p.GW), patch_mse ? (unsigned)(T / TUB) : 1u, (unsigned)B);
    if (norm_pix) hipLaunchKernelGGL(mae_panels_kernel<true>, grid, dim3(NTHREADS), 0, st, p);
    else hipLaunchKernelGGL(mae_panels_kernel<false>, grid, dim3(NTHREADS), 0, st, p);
    return S2K_OK;
}

}  // namespace s2k
