// Per-pixel cross-entropy / focal loss (+ gradient) and the class mask.
//
// Replaces /root/reference/src/losses.py:24-89 (get_loss -> nn.CrossEntropyLoss | FocalLoss.__call__:
// F.cross_entropy(reduction="none", label_smoothing, ignore_index) -> pt = exp(-ce) ->
// alpha[y] * (1-pt)^gamma * ce -> mean over ALL pixels) and logits.argmax(dim=1)
// (train_segmentation.py:145,206).  One thread per pixel: the C logits of a pixel are C coalesced
// plane reads; log-softmax, NLL, smoothing term and focal modulation stay in registers; the sum
// is a wave shuffle reduction + one f64 atomic per wave.  Pure HBM streaming (read logits once).
#include <algorithm>

#include "common.h"

namespace s2k {

constexpr int MAXC = 64;

struct LossP {
    const float* logits;
    const int64_t* labels;
    const float* alpha;
    double* acc;        // [2]: numerator, denominator
    float* loss;        // [1]
    const float* gout;  // [1] upstream gradient (backward)
    float* dlogits;
    int B, C, HW, mode, ignore, reduce_sum;
    float gamma, smooth;
};


// pow(om, g) for the exponents the configs use (gamma = 2 in the benchmark recipe) without the general powf
__device__ __forceinline__ float pow_gamma(float om, float g) {
    if (g == 2.0f) return om * om;
    if (g == 1.0f) return om;
    if (g == 0.0f) return 1.0f;
    return powf(om, g);
}

// log-softmax of one pixel: lp[c] = x[c] - logsumexp(x), e[c] = exp(x[c] - max) / sum (the softmax, reused by the backward).
// CC > 0: the class count is a compile-time constant and everything stays in registers (CC = 0: run-time C, at most MAXC).
template <int CC>
__device__ __forceinline__ void pixel_logp(const LossP& p, int b, int hw, float* lp, float* sm) {
    const int C = CC > 0 ? CC : p.C;
    const float* src = p.logits + ((int64_t)b * C) * p.HW + hw;
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < (CC > 0 ? CC : MAXC); ++c) {
        if (c >= C) break;
        lp[c] = src[(int64_t)c * p.HW];
        mx = fmaxf(mx, lp[c]);
    }
    float se = 0.0f;
#pragma unroll
    for (int c = 0; c < (CC > 0 ? CC : MAXC); ++c) {
        if (c >= C) break;
        sm[c] = expf(lp[c] - mx);
        se += sm[c];
    }
    const float lse = mx + logf(se), inv = 1.0f / se;
#pragma unroll
    for (int c = 0; c < (CC > 0 ? CC : MAXC); ++c) {
        if (c >= C) break;
        lp[c] -= lse;
        sm[c] *= inv;
    }
}

// value of arr[y] without a dynamic register index
template <int CC>
__device__ __forceinline__ float pick(const float* arr, int y, int C) {
    if (CC == 0) return arr[y];
    float v = 0.0f;
#pragma unroll
    for (int c = 0; c < (CC > 0 ? CC : 1); ++c) v = (c == y) ? arr[c] : v;
    return v;
}

// grid: (pixel blocks, B): no per-pixel division; one thread per pixel of sample blockIdx.y
template <int CC>
__global__ void __launch_bounds__(NTHREADS) loss_fwd_kernel(const LossP p) {
    const int C = CC > 0 ? CC : p.C;
    const int b = blockIdx.y;
    double num = 0.0, den = 0.0;
    float lp[CC > 0 ? CC : MAXC], sm[CC > 0 ? CC : MAXC];
    for (int hw = blockIdx.x * blockDim.x + threadIdx.x; hw < p.HW; hw += gridDim.x * blockDim.x) {
        const int64_t y64 = p.labels[(int64_t)b * p.HW + hw];
        if (y64 == p.ignore || y64 < 0 || y64 >= C) continue;
        const int y = (int)y64;
        pixel_logp<CC>(p, b, hw, lp, sm);
        const float lpy = pick<CC>(lp, y, C);
        if (p.mode == 0) {
            const float wy = p.alpha ? p.alpha[y] : 1.0f;
            float ce = (1.0f - p.smooth) * wy * (-lpy);
            if (p.smooth > 0.0f) {
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < (CC > 0 ? CC : MAXC); ++c) {
                    if (c >= C) break;
                    s -= (p.alpha ? p.alpha[c] : 1.0f) * lp[c];
                }
                ce += (p.smooth / C) * s;
            }
            num += ce;
            den += wy;
        } else {
            float ce = (1.0f - p.smooth) * (-lpy);
            if (p.smooth > 0.0f) {
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < (CC > 0 ? CC : MAXC); ++c) {
                    if (c >= C) break;
                    s -= lp[c];
                }
                ce += (p.smooth / C) * s;
            }
            const float pt = expf(-ce);
            const float a = p.alpha ? p.alpha[y] : 1.0f;
            num += a * pow_gamma(1.0f - pt, p.gamma) * ce;
        }
    }
    // one atomic pair per WORKGROUP: the two sums live at one address each, and same-address f64 atomics execute one after the
    // other at the memory side (16 k waves adding there took 200 us of a kernel whose data streams in 15)
    __shared__ double red[8];
    num = wave_sum_d(num);
    den = wave_sum_d(den);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave] = num; red[4 + wave] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        num = (red[0] + red[1]) + (red[2] + red[3]);
        den = (red[4] + red[5]) + (red[6] + red[7]);
        if (num != 0.0) atomic_add_d(p.acc, num);
        if (den != 0.0) atomic_add_d(p.acc + 1, den);
    }
}

__global__ void loss_finish_kernel(const LossP p) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double v;
    if (p.mode == 0) v = p.acc[0] / p.acc[1];  // mean over non-ignored (NaN when none, as torch)
    else v = p.reduce_sum ? p.acc[0] : p.acc[0] / ((double)p.B * p.HW);
    p.loss[0] = (float)v;
}

template <int CC>
__global__ void __launch_bounds__(NTHREADS) loss_bwd_kernel(const LossP p) {
    const int C = CC > 0 ? CC : p.C;
    const int b = blockIdx.y;
    const float go = p.gout ? p.gout[0] : 1.0f;
    float norm;
    if (p.mode == 0) norm = go / (float)p.acc[1];
    else norm = p.reduce_sum ? go : go / (float)((double)p.B * p.HW);
    float lp[CC > 0 ? CC : MAXC], sm[CC > 0 ? CC : MAXC];
    for (int hw = blockIdx.x * blockDim.x + threadIdx.x; hw < p.HW; hw += gridDim.x * blockDim.x) {
        float* dst = p.dlogits + ((int64_t)b * C) * p.HW + hw;
        const int64_t y64 = p.labels[(int64_t)b * p.HW + hw];
        if (y64 == p.ignore || y64 < 0 || y64 >= C) {
#pragma unroll
            for (int c = 0; c < (CC > 0 ? CC : MAXC); ++c) {
                if (c >= C) break;
                dst[(int64_t)c * p.HW] = 0.0f;
            }
            continue;
        }
        const int y = (int)y64;
        pixel_logp<CC>(p, b, hw, lp, sm);      // sm[c] = softmax = exp(lp[c])
        if (p.mode == 0) {
            const float wy = p.alpha ? p.alpha[y] : 1.0f;
            float wsum = 0.0f;
            if (p.smooth > 0.0f)
                for (int c = 0; c < C; ++c) wsum += p.alpha ? p.alpha[c] : 1.0f;
#pragma unroll
            for (int c = 0; c < (CC > 0 ? CC : MAXC); ++c) {
                if (c >= C) break;
                const float pc = expf(lp[c]);      // (not sm[c]: keeps the round-1 rounding the gradient fixtures were checked with)
                float d = (1.0f - p.smooth) * wy * (pc - (c == y ? 1.0f : 0.0f));
                if (p.smooth > 0.0f) d += (p.smooth / C) * (pc * wsum - (p.alpha ? p.alpha[c] : 1.0f));
                dst[(int64_t)c * p.HW] = d * norm;
            }
        } else {
            float ce = (1.0f - p.smooth) * (-pick<CC>(lp, y, C));
            if (p.smooth > 0.0f) {
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < (CC > 0 ? CC : MAXC); ++c) {
                    if (c >= C) break;
                    s -= lp[c];
                }
                ce += (p.smooth / C) * s;
            }
            const float pt = expf(-ce);
            const float om = 1.0f - pt;
            const float a = p.alpha ? p.alpha[y] : 1.0f;
            float dfl = 0.0f;  // d focal / d ce
            if (om > 0.0f) dfl = a * (pow_gamma(om, p.gamma) + p.gamma * pow_gamma(om, p.gamma - 1.0f) * pt * ce);
            else if (p.gamma == 0.0f) dfl = a;
#pragma unroll
            for (int c = 0; c < (CC > 0 ? CC : MAXC); ++c) {
                if (c >= C) break;
                const float pc = expf(lp[c]);      // (not sm[c]: keeps the round-1 rounding the gradient fixtures were checked with)
                const float dce = (1.0f - p.smooth) * (pc - (c == y ? 1.0f : 0.0f)) + p.smooth * (pc - 1.0f / C);
                dst[(int64_t)c * p.HW] = dfl * dce * norm;
            }
        }
    }
}

__global__ void __launch_bounds__(NTHREADS) argmax_kernel(const float* logits, int64_t* mask, int B, int C, int HW) {
    const int b = blockIdx.y;
    for (int hw = blockIdx.x * blockDim.x + threadIdx.x; hw < HW; hw += gridDim.x * blockDim.x) {
        const int64_t i = (int64_t)b * HW + hw;
        const float* src = logits + ((int64_t)b * C) * HW + hw;
        float best = src[0];
        int idx = 0;
        for (int c = 1; c < C; ++c) {
            const float v = src[(int64_t)c * HW];
            if (v > best) { best = v; idx = c; }   // strict >: the first maximum wins
        }
        mask[i] = idx;
    }
}

// pixel blocks per sample: one thread per pixel until ~4 blocks per CU exist, grid-stride beyond
static unsigned pixel_blocks(int B, int HW) {
    const int per = cdiv(HW, NTHREADS);
    return (unsigned)std::max(1, std::min(per, cdiv(1024, B)));
}

static int fill(LossP& p, const S2kOp& op, const Ctx& c, bool bwd) {
    const int32_t* d = op.d;
    p.B = d[0]; p.C = d[1]; p.HW = d[2]; p.mode = d[3]; p.ignore = d[4]; p.reduce_sum = d[5];
    p.gamma = op.f[0]; p.smooth = op.f[1];
    if (p.B <= 0 || p.C <= 1 || p.C > MAXC || p.HW <= 0) { set_error("loss: unsupported shape C=%d", p.C); return S2K_EINVAL; }
    (void)c; (void)bwd;
    return S2K_OK;
}

int launch_loss_fwd(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    LossP p{};
    if (int e = fill(p, op, c, false)) return e;
    p.logits = r.ptr<const float>(op.t[S2K_LOSS_FWD_T_LOGITS]);
    p.labels = r.ptr<const int64_t>(op.t[S2K_LOSS_FWD_T_LABELS]);
    p.alpha = r.ptr<const float>(op.t[S2K_LOSS_FWD_T_ALPHA]);
    p.loss = r.ptr<float>(op.t[S2K_LOSS_FWD_T_LOSS]);
    p.acc = r.ptr<double>(op.t[S2K_LOSS_FWD_T_ACC]);
    if (r.absent) { set_error("loss_fwd: null base"); return S2K_EFAULT; }
    if (!p.logits || !p.labels || !p.loss || !p.acc) { set_error("loss_fwd: missing tensor"); return S2K_EINVAL; }
    if (hipMemsetAsync(p.acc, 0, 2 * sizeof(double), c.stream) != hipSuccess) { set_error("loss_fwd: memset failed"); return S2K_EHIP; }
    if (p.B > 65535) { set_error("loss: batch beyond the launch grid"); return S2K_EINVAL; }
    const dim3 grid(pixel_blocks(p.B, p.HW), (unsigned)p.B);
#define LOSS_CC(N) case N: hipLaunchKernelGGL(loss_fwd_kernel<N>, grid, dim3(NTHREADS), 0, c.stream, p); break
    switch (p.C) {
        LOSS_CC(2); LOSS_CC(3); LOSS_CC(4); LOSS_CC(5); LOSS_CC(6); LOSS_CC(7); LOSS_CC(8);
        default: hipLaunchKernelGGL(loss_fwd_kernel<0>, grid, dim3(NTHREADS), 0, c.stream, p);
    }
#undef LOSS_CC
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64), 0, c.stream, p);
    return S2K_OK;
}

int launch_loss_bwd(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    LossP p{};
    if (int e = fill(p, op, c, true)) return e;
    p.logits = r.ptr<const float>(op.t[S2K_LOSS_BWD_T_LOGITS]);
    p.labels = r.ptr<const int64_t>(op.t[S2K_LOSS_BWD_T_LABELS]);
    p.alpha = r.ptr<const float>(op.t[S2K_LOSS_BWD_T_ALPHA]);
    p.acc = r.ptr<double>(op.t[S2K_LOSS_BWD_T_ACC]);
    p.gout = r.ptr<const float>(op.t[S2K_LOSS_BWD_T_GOUT]);
    p.dlogits = r.ptr<float>(op.t[S2K_LOSS_BWD_T_DLOGITS]);
    if (r.absent) { set_error("loss_bwd: null base"); return S2K_EFAULT; }
    if (!p.logits || !p.labels || !p.acc || !p.dlogits) { set_error("loss_bwd: missing tensor"); return S2K_EINVAL; }
    if (p.B > 65535) { set_error("loss: batch beyond the launch grid"); return S2K_EINVAL; }
    const dim3 grid(pixel_blocks(p.B, p.HW), (unsigned)p.B);
#define LOSS_CC(N) case N: hipLaunchKernelGGL(loss_bwd_kernel<N>, grid, dim3(NTHREADS), 0, c.stream, p); break
    switch (p.C) {
        LOSS_CC(2); LOSS_CC(3); LOSS_CC(4); LOSS_CC(5); LOSS_CC(6); LOSS_CC(7); LOSS_CC(8);
        default: hipLaunchKernelGGL(loss_bwd_kernel<0>, grid, dim3(NTHREADS), 0, c.stream, p);
    }
#undef LOSS_CC
    return S2K_OK;
}

int launch_argmax(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    const float* logits = r.ptr<const float>(op.t[S2K_ARGMAX_T_LOGITS]);
    int64_t* mask = r.ptr<int64_t>(op.t[S2K_ARGMAX_T_MASK]);
    if (r.absent) { set_error("argmax: null base"); return S2K_EFAULT; }
    const int B = op.d[S2K_ARGMAX_D_B], C = op.d[S2K_ARGMAX_D_C], HW = op.d[S2K_ARGMAX_D_HW];
    if (!logits || !mask || B <= 0 || C <= 0 || HW <= 0) { set_error("argmax: bad args"); return S2K_EINVAL; }
    if (B > 65535) { set_error("argmax: batch beyond the launch grid"); return S2K_EINVAL; }
    hipLaunchKernelGGL(argmax_kernel, dim3(pixel_blocks(B, HW), (unsigned)B), dim3(NTHREADS), 0, c.stream, logits, mask, B, C, HW);
    return S2K_OK;
}

// ---------------- confusion histogram ----------------------------------------------------------------------
// hist[t][p] += 1 per pixel: per-workgroup LDS histogram (C <= 64), flushed with one 64-bit atomic per non-empty bin
__global__ void __launch_bounds__(NTHREADS) confusion_kernel(const int64_t* pred, const int64_t* labels, unsigned long long* hist,
                                                             int64_t n, int C) {
    extern __shared__ unsigned int bins[];
    for (int i = threadIdx.x; i < C * C; i += NTHREADS) bins[i] = 0u;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t t = labels[i], q = pred[i];
        if (t >= 0 && t < C && q >= 0 && q < C) atomicAdd(&bins[(int)t * C + (int)q], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += NTHREADS)
        if (bins[i]) atomicAdd(hist + i, (unsigned long long)bins[i]);
}

int launch_confusion(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    const int64_t* pred = r.ptr<const int64_t>(op.t[S2K_CONFUSION_T_PRED]);
    const int64_t* labels = r.ptr<const int64_t>(op.t[S2K_CONFUSION_T_LABELS]);
    unsigned long long* hist = r.ptr<unsigned long long>(op.t[S2K_CONFUSION_T_HIST]);
    if (r.absent) { set_error("confusion: null base"); return S2K_EFAULT; }
    const int64_t n = op.n[S2K_CONFUSION_N_COUNT];
    const int C = op.d[S2K_CONFUSION_D_C];
    if (!pred || !labels || !hist || n <= 0 || C <= 0 || C > MAXC) { set_error("confusion: bad args (C <= %d)", MAXC); return S2K_EINVAL; }
    // each workgroup counts at most 2^32 - 1 pixels per bin: cap the pixels per workgroup
    const int blocks = (int)std::min<int64_t>(std::max<int64_t>(cdiv64(n, 1 << 20), std::min<int64_t>(cdiv64(n, 4096), 1024)), 65535);
    hipLaunchKernelGGL(confusion_kernel, dim3(blocks), dim3(NTHREADS), (size_t)C * C * sizeof(unsigned int), c.stream, pred, labels, hist, n, C);
    return S2K_OK;
}

}  // namespace s2k
