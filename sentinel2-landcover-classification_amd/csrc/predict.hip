// Whole-tile prediction (predict.py): the logits a model returned for overlapping S x S windows of a tile - cut by TILE_PREP from
// explicit {tile, y0, x0, flips} params, possibly under several flip variants - blended into ONE [K][H][W] prediction per tile, its
// class map and, against the resident label rasters, the confusion counts of metrics.SegMetrics.  The reference stops at per-crop
// logits (src/train_segmentation.py:106 predict_step, src/experiments/inference_demo.py); Prithvi's fixed 224 x 224 position tables
// make windows the only way to predict a 512 x 512 tile at all.
//
// A gather, not a scatter: a thread owns four consecutive pixels of an output row and sums the windows that cover them in the fixed
// order (flip variant, window row, window column) - no float atomics, bit-identical from run to run.  HBM-bound on LOGITS, which is
// read exactly once: lanes run along x, so per class plane a wave reads 1 KB of one window row (reversed under a horizontal flip:
// the quad is loaded from its mirrored place and its four values swapped in registers).  Where a window's rows are not 16-byte
// aligned for the quad (an origin such as W - S = 38, or S % 4 != 0) the quad is read element by element, with the window's edge
// checked per element.
#include "common.h"

namespace s2k {

constexpr int BLEND_MAXK = 32;

struct BlendP {
    const float* logits;            // [M][F][NY][NX][K][S][S]
    const int *ys, *xs, *flips;     // [NY], [NX], [F]
    const float* w1;                // [S]
    float* blend;                   // [M][K][H][W] or null
    long long* mask;                // [M][H][W] or null
    const unsigned char* labels;    // [NSRC][H][W]
    const int* index;               // [M]
    const int* lut;                 // [256]
    unsigned long long* hist;       // [K][K] or null
    int M, F, NY, NX, K, H, W, S, NSRC;
    int vec;                        // LOGITS 16-byte aligned and S % 4 == 0: a window whose origin is a multiple of 4 is read in quads
    int bvec, mvec;                 // BLEND / MASK rows 16-byte aligned (W % 4 == 0): quad stores
    int bpt;                        // workgroups per tile
};

// grid: M * bpt workgroups; workgroup (m, blk) owns 256 consecutive pixel quads of tile m in row-major order, so it never straddles
// two tiles and its LDS confusion bins count at most 1024 pixels.  KMAX: the compiled class capacity (K <= KMAX; the per-class
// registers are indexed by unrolled loops only), MODE 1: softmax over the classes of every window pixel before blending.
template <int KMAX, int MODE>
__global__ void __launch_bounds__(NTHREADS) window_blend_kernel(const BlendP p) {
    __shared__ unsigned int bins[BLEND_MAXK * BLEND_MAXK];
    const int tid = threadIdx.x, K = p.K, S = p.S;
    const int m = blockIdx.x / p.bpt, blk = blockIdx.x - m * p.bpt;
    if (p.hist) {
        for (int i = tid; i < K * K; i += NTHREADS) bins[i] = 0u;
        __syncthreads();
    }
    const int Q = (p.W + 3) >> 2;                                  // quads per row; the last one hangs over the edge when W % 4 != 0
    const int64_t e = (int64_t)blk * NTHREADS + tid;
    if (e < (int64_t)p.H * Q) {
        const int y = (int)(e / Q), x0 = (int)(e - (int64_t)y * Q) * 4;
        const int64_t SS = (int64_t)S * S;
        float acc[KMAX][4], ws[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < KMAX; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0f;
        for (int f = 0; f < p.F; ++f) {
            const int fl = p.flips[f];
            for (int i = 0; i < p.NY; ++i) {
                const int ly = y - p.ys[i];
                if ((unsigned)ly >= (unsigned)S) continue;
                const float wy = p.w1[ly];
                const int ry = (fl & 2) ? S - 1 - ly : ly;
                for (int j = 0; j < p.NX; ++j) {
                    const int xs = p.xs[j], lx0 = x0 - xs;         // local column of the quad's first pixel
                    if (lx0 + 3 < 0 || lx0 >= S) continue;
                    const float* win = p.logits + ((((int64_t)m * p.F + f) * p.NY + i) * p.NX + j) * K * SS + (int64_t)ry * S;
                    float v[KMAX][4], w[4];
                    if (p.vec && !(xs & 3)) {                      // lx0 % 4 == 0 and S % 4 == 0: the whole quad lies inside the window
                        const float4 wx = *reinterpret_cast<const float4*>(p.w1 + lx0);
                        w[0] = wy * wx.x; w[1] = wy * wx.y; w[2] = wy * wx.z; w[3] = wy * wx.w;
                        const float* src = win + ((fl & 1) ? S - 4 - lx0 : lx0);
#pragma unroll
                        for (int k = 0; k < KMAX; ++k) {
                            float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                            if (k < K) t = *reinterpret_cast<const float4*>(src + k * SS);
                            if (fl & 1) { v[k][0] = t.w; v[k][1] = t.z; v[k][2] = t.y; v[k][3] = t.x; }
                            else { v[k][0] = t.x; v[k][1] = t.y; v[k][2] = t.z; v[k][3] = t.w; }
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int lx = lx0 + q;
                            const bool in = (unsigned)lx < (unsigned)S;
                            w[q] = in ? wy * p.w1[lx] : 0.0f;      // a pixel outside this window adds 0 * 0: nothing
                            const float* src = win + ((fl & 1) ? S - 1 - lx : lx);
#pragma unroll
                            for (int k = 0; k < KMAX; ++k) {
                                v[k][q] = 0.0f;
                                if (in && k < K) v[k][q] = src[k * SS];
                            }
                        }
                    }
                    if (MODE == 1) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float mx = v[0][q];
#pragma unroll
                            for (int k = 1; k < KMAX; ++k)
                                if (k < K) mx = fmaxf(mx, v[k][q]);
                            float s = 0.0f;
#pragma unroll
                            for (int k = 0; k < KMAX; ++k)
                                if (k < K) { v[k][q] = expf(v[k][q] - mx); s += v[k][q]; }
                            const float inv = 1.0f / s;
#pragma unroll
                            for (int k = 0; k < KMAX; ++k) v[k][q] *= inv;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        ws[q] += w[q];
#pragma unroll
                        for (int k = 0; k < KMAX; ++k)
                            if (k < K) acc[k][q] += w[q] * v[k][q];
                    }
                }
            }
        }
        // acc / ws with a true division: the exact case (integer sums) stays within one rounding
        int best[4] = {0, 0, 0, 0};
        float top[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) {
                    acc[k][q] = acc[k][q] / ws[q];
                    if (k == 0) top[q] = acc[0][q];
                    else if (acc[k][q] > top[q]) { top[q] = acc[k][q]; best[q] = k; }      // strict >: the first maximum wins (ARGMAX)
                }
        }
        const int64_t pix = ((int64_t)m * p.H + y) * p.W + x0;
        if (p.blend) {
            float* dst = p.blend + ((int64_t)m * K * p.H + y) * p.W + x0;
            const int64_t HW = (int64_t)p.H * p.W;
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) {
                    if (p.bvec) *reinterpret_cast<float4*>(dst + k * HW) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
                    else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (x0 + q < p.W) dst[k * HW + q] = acc[k][q];
                    }
                }
        }
        if (p.mask) {
            if (p.mvec) {
                longlong2* dst = reinterpret_cast<longlong2*>(p.mask + pix);
                dst[0] = make_longlong2(best[0], best[1]);
                dst[1] = make_longlong2(best[2], best[3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.W) p.mask[pix + q] = best[q];
            }
        }
        if (p.hist) {
            const int src = p.index[m];
            if ((unsigned)src < (unsigned)p.NSRC) {
                const unsigned char* lab = p.labels + ((int64_t)src * p.H + y) * p.W + x0;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.W) {
                        const int t = p.lut[lab[q]];
                        if ((unsigned)t < (unsigned)K) atomicAdd(&bins[t * K + best[q]], 1u);
                    }
            }
        }
    }
    if (p.hist) {
        __syncthreads();
        for (int i = tid; i < K * K; i += NTHREADS)
            if (bins[i]) atomicAdd(p.hist + i, (unsigned long long)bins[i]);
    }
}

template <int KMAX>
static void launch_k(const BlendP& p, int mode, unsigned grid, hipStream_t stream) {
    if (mode) hipLaunchKernelGGL((window_blend_kernel<KMAX, 1>), dim3(grid), dim3(NTHREADS), 0, stream, p);
    else hipLaunchKernelGGL((window_blend_kernel<KMAX, 0>), dim3(grid), dim3(NTHREADS), 0, stream, p);
}

// YS / XS / FLIPS / INDEX are not range-checked against the tile on the device beyond what keeps every access inside its tensor (a
// window position is always formed from a local coordinate inside [0, S)); the host (predict.py) builds and validates them.
int launch_window_blend(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    BlendP p{};
    p.logits = r.ptr<const float>(op.t[S2K_WINDOW_BLEND_T_LOGITS]);
    p.ys = r.ptr<const int>(op.t[S2K_WINDOW_BLEND_T_YS]);
    p.xs = r.ptr<const int>(op.t[S2K_WINDOW_BLEND_T_XS]);
    p.flips = r.ptr<const int>(op.t[S2K_WINDOW_BLEND_T_FLIPS]);
    p.w1 = r.ptr<const float>(op.t[S2K_WINDOW_BLEND_T_W1]);
    p.blend = r.ptr<float>(op.t[S2K_WINDOW_BLEND_T_BLEND]);
    p.mask = r.ptr<long long>(op.t[S2K_WINDOW_BLEND_T_MASK]);
    p.labels = r.ptr<const unsigned char>(op.t[S2K_WINDOW_BLEND_T_LABELS]);
    p.index = r.ptr<const int>(op.t[S2K_WINDOW_BLEND_T_INDEX]);
    p.lut = r.ptr<const int>(op.t[S2K_WINDOW_BLEND_T_LUT]);
    p.hist = r.ptr<unsigned long long>(op.t[S2K_WINDOW_BLEND_T_HIST]);
    if (r.absent) return r.fault("window_blend");
    if (!p.logits || !p.ys || !p.xs || !p.flips || !p.w1) { set_error("window_blend: missing tensor"); return S2K_EINVAL; }
    const int* d = op.d;
    p.M = d[S2K_WINDOW_BLEND_D_M]; p.F = d[S2K_WINDOW_BLEND_D_F]; p.NY = d[S2K_WINDOW_BLEND_D_NY]; p.NX = d[S2K_WINDOW_BLEND_D_NX];
    p.K = d[S2K_WINDOW_BLEND_D_K]; p.H = d[S2K_WINDOW_BLEND_D_H]; p.W = d[S2K_WINDOW_BLEND_D_W]; p.S = d[S2K_WINDOW_BLEND_D_S];
    p.NSRC = d[S2K_WINDOW_BLEND_D_NSRC];
    const int mode = d[S2K_WINDOW_BLEND_D_MODE];
    bool ok = p.K >= 1 && p.K <= BLEND_MAXK && p.F >= 1 && p.F <= 4 && p.S >= 1 && p.S <= p.H && p.S <= p.W && p.M >= 1 && p.NY >= 1 &&
              p.NX >= 1 && (mode == 0 || mode == 1) && (p.blend || p.mask || p.hist) &&
              (!p.hist || (p.labels && p.index && p.lut && p.NSRC >= 1));
    int64_t n = 1;                                                  // elements of LOGITS, kept below 2^31 factor by factor
    const int fac[] = {p.M, p.F, p.NY, p.NX, p.K, p.S, p.S};
    for (int i = 0; ok && i < 7; ++i) {
        n *= fac[i];
        ok = n < (1ll << 31);
    }
    const int64_t quads = ok ? (int64_t)p.H * ((p.W + 3) >> 2) : 0;
    const int64_t bpt = cdiv64(quads, NTHREADS);
    if (!ok || bpt * p.M > 0x7fffffffll) {
        set_error("window_blend: bad dims (1 <= K <= 32, 1 <= F <= 4, 1 <= S <= H, W, M >= 1, MODE 0 or 1, an output, HIST with LABELS / "
                  "INDEX / LUT, LOGITS < 2^31 elements)");
        return S2K_EINVAL;
    }
    p.bpt = (int)bpt;
    p.vec = (reinterpret_cast<uintptr_t>(p.logits) % 16 == 0 && reinterpret_cast<uintptr_t>(p.w1) % 16 == 0 && p.S % 4 == 0) ? 1 : 0;
    p.bvec = (p.blend && reinterpret_cast<uintptr_t>(p.blend) % 16 == 0 && p.W % 4 == 0) ? 1 : 0;
    p.mvec = (p.mask && reinterpret_cast<uintptr_t>(p.mask) % 16 == 0 && p.W % 4 == 0) ? 1 : 0;
    const unsigned grid = (unsigned)(bpt * p.M);
    if (p.K <= 2) launch_k<2>(p, mode, grid, c.stream);
    else if (p.K <= 4) launch_k<4>(p, mode, grid, c.stream);
    else if (p.K <= 8) launch_k<8>(p, mode, grid, c.stream);
    else if (p.K <= 16) launch_k<16>(p, mode, grid, c.stream);
    else if (p.K <= 24) launch_k<24>(p, mode, grid, c.stream);
    else launch_k<32>(p, mode, grid, c.stream);
    return S2K_OK;
}

}  // namespace s2k
