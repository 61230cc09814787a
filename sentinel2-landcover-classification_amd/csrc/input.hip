// GPU-side input pipeline: raw int16 Sentinel-2 tiles + uint8 label rasters -> the network's
// fp32 NCHW crops and int64 label maps, one pass.  Replaces, per sample, the reference's CPU chain
//   s2osm_dataset.py:51-71   cnes_transform (np.vectorize remap, cnes_labell_mappings.py:85-95), channel-last round trip,
//                            .float(), .long()
//   s2osm_datamodule.py:75-87  A.RandomCrop / A.CenterCrop -> A.HorizontalFlip -> A.VerticalFlip -> A.Normalize
// which runs on one loader worker in the reference.  HBM-bound: 2 B read + 4 B written per image element; lanes run along
// the output row (128-B coalesced stores; the int16 reads of a row are contiguous too, reversed under a horizontal flip).
// The crop offsets and flip decisions come from the host (PARAMS), like every other random draw of this library.
#include "common.h"

namespace s2k {

struct PrepP {
    const short* raw;
    const unsigned char* labels;
    const int* params;     // [B][4] = {src, y0, x0, flips}
    const float* norm;     // [2][C] = {mean * max_pixel_value, 1 / (std * max_pixel_value)}
    const int* lut;        // [256]
    float* x;
    long long* y;
    int B, C, H, W, S, NSRC;
};

// grid: (row groups, C + 1 planes, B); plane C is the label map.  One thread per 4 output columns.
__global__ void __launch_bounds__(NTHREADS) tile_prep_kernel(const PrepP p) {
    const int b = blockIdx.z, plane = blockIdx.y;
    const int q = p.S >> 2;                                   // column quads per row (S % 4 == 0, host check)
    const int e = blockIdx.x * NTHREADS + threadIdx.x;
    if (e >= p.S * q) return;
    const int i = e / q, j = (e - i * q) * 4;
    const int src = p.params[4 * b], y0 = p.params[4 * b + 1], x0 = p.params[4 * b + 2], flips = p.params[4 * b + 3];
    const int si = y0 + ((flips & 2) ? p.S - 1 - i : i);
    const int sj = x0 + ((flips & 1) ? p.S - 1 - j : j);      // source column of output column j; j + k maps to sj -/+ k
    const int step = (flips & 1) ? -1 : 1;
    if (plane < p.C) {
        const short* row = p.raw + (((int64_t)src * p.C + plane) * p.H + si) * p.W;
        const float m = p.norm[plane], d = p.norm[p.C + plane];
        float4 o;
        o.x = __fmul_rn(__fsub_rn((float)row[sj], m), d);
        o.y = __fmul_rn(__fsub_rn((float)row[sj + step], m), d);
        o.z = __fmul_rn(__fsub_rn((float)row[sj + 2 * step], m), d);
        o.w = __fmul_rn(__fsub_rn((float)row[sj + 3 * step], m), d);
        *reinterpret_cast<float4*>(p.x + (((int64_t)b * p.C + plane) * p.S + i) * p.S + j) = o;
    } else if (p.y) {
        const unsigned char* row = p.labels + ((int64_t)src * p.H + si) * p.W;
        long long* dst = p.y + ((int64_t)b * p.S + i) * p.S + j;
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = p.lut[row[sj + k * step]];
    }
}

// PARAMS are not range-checked on the device (that would cost a sync or a branch per element): the host mirror
// (data/gpu_pipeline.py) draws / validates them before upload: 0 <= src < NSRC, 0 <= y0 <= H - S, 0 <= x0 <= W - S.
int launch_tile_prep(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    PrepP p{};
    p.raw = r.ptr<const short>(op.t[S2K_TILE_PREP_T_RAW]);
    p.labels = r.ptr<const unsigned char>(op.t[S2K_TILE_PREP_T_LABELS]);
    p.params = r.ptr<const int>(op.t[S2K_TILE_PREP_T_PARAMS]);
    p.norm = r.ptr<const float>(op.t[S2K_TILE_PREP_T_NORM]);
    p.lut = r.ptr<const int>(op.t[S2K_TILE_PREP_T_LUT]);
    p.x = r.ptr<float>(op.t[S2K_TILE_PREP_T_X]);
    p.y = r.ptr<long long>(op.t[S2K_TILE_PREP_T_Y]);
    if (r.absent) return r.fault("tile_prep");
    p.B = op.d[S2K_TILE_PREP_D_B]; p.C = op.d[S2K_TILE_PREP_D_C]; p.H = op.d[S2K_TILE_PREP_D_H]; p.W = op.d[S2K_TILE_PREP_D_W];
    p.S = op.d[S2K_TILE_PREP_D_S]; p.NSRC = op.d[S2K_TILE_PREP_D_NSRC];
    if (!p.raw || !p.params || !p.norm || !p.x || (p.y && (!p.labels || !p.lut))) { set_error("tile_prep: missing tensor"); return S2K_EINVAL; }
    if (p.B <= 0 || p.C <= 0 || p.S <= 0 || (p.S & 3) || p.S > p.H || p.S > p.W || p.NSRC <= 0 || p.B > 65535 || p.C >= 65535) {
        set_error("tile_prep: bad dims (crop size must be a multiple of 4 and fit the tile)"); return S2K_EINVAL;
    }
    const int per_plane = p.S * (p.S >> 2);
    hipLaunchKernelGGL(tile_prep_kernel, dim3(cdiv(per_plane, NTHREADS), p.C + (p.y ? 1 : 0), p.B), dim3(NTHREADS), 0, c.stream, p);
    return S2K_OK;
}

// ---------------- dataset statistics over the resident tiles ----------------------------------------------------------------
// The three passes the reference makes over the whole dataset before a run starts - calculate_mean_std (Welford over all tiles,
// src/data/calculate_dataset_statistics.py:10-43), get_class_probabilities and get_sample_weights (src/utils.py:152-217) - read
// nothing but the raw tiles and label rasters that TILE_PREP already keeps in HBM, so each is one streaming read: TILE_LABEL_HIST
// gives the per-tile class counts both label passes derive from, TILE_MOMENTS the per-position sums of the mean / std pass.
// Integer arithmetic throughout (the one f64 sum has a fixed order): results are bit-identical from run to run.

struct HistP {
    const unsigned char* labels;
    const int* index;      // [M] source tile of every HIST row
    const int* lut;        // [256]
    long long* hist;       // [M][K]
    int M, H, W, K, Y0, X0, WH, WW;
};

// 0x80 in every byte of x that is zero (no carry crosses a byte: (x & 0x7f) + 0x7f <= 0xfe)
__device__ __forceinline__ unsigned int zero_bytes(unsigned int x) {
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_mov0_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false); }
// sum over the (converged) wave, in every lane: wave_sum of common.h on integers
__device__ __forceinline__ int wave_sum_i(int v) {
    v += dpp_mov0_i<DPP_XOR1>(v);
    v += dpp_mov0_i<DPP_XOR2>(v);
    v += dpp_mov0_i<DPP_HALF_MIRROR>(v);
    v += dpp_mov0_i<DPP_MIRROR>(v);
    v += dpp_mov0_i<DPP_BCAST15, 0xa>(v);
    v += dpp_mov0_i<DPP_BCAST31, 0xc>(v);
    return __builtin_amdgcn_readlane(v, 63);
}

// grid: M workgroups, one selected tile each.  A window row is cut into units - the bytes before the first 16-byte boundary, whole
// 16-byte vectors, the bytes after the last one - and a lane takes one unit per round, so a wave holds up to 1024 pixels.  Land
// cover is spatially coherent and a label map has few classes: those pixels fall into a handful of bins.  The wave therefore counts
// bin by bin - every lane counts its bytes of the bin with byte-parallel compares, one cross-lane sum, ONE add into the wave's own
// LDS bins - instead of issuing 64 LDS atomics that collide on the same few addresses.
__global__ void __launch_bounds__(NTHREADS) tile_label_hist_kernel(const HistP p) {
    __shared__ unsigned int bins[NTHREADS / WAVE][256];      // 32-bit: a window holds < 2^32 pixels (launcher check)
    __shared__ int lut[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < (NTHREADS / WAVE) * 256; i += NTHREADS) (&bins[0][0])[i] = 0u;
    lut[tid] = ((unsigned)p.lut[tid] < (unsigned)p.K) ? p.lut[tid] : -1;      // NTHREADS == 256 entries; -1: not counted
    __syncthreads();
    const int m = blockIdx.x;
    const unsigned char* win = p.labels + ((int64_t)p.index[m] * p.H + p.Y0) * p.W + p.X0;
    const int U = (p.WW >> 4) + 2;                          // units per row, at most: head, WW / 16 vectors, tail
    const int64_t total = (int64_t)p.WH * U;
    unsigned int* mine = bins[wave];
    for (int64_t e0 = (int64_t)wave * WAVE; e0 < total; e0 += NTHREADS) {      // wave-uniform trip count: the wave stays converged
        const int64_t e = e0 + lane;
        unsigned int w[4] = {0u, 0u, 0u, 0u};
        int nb = 0;                                         // bytes this lane holds (in w, little endian)
        if (e < total) {
            const int i = (int)(e / U), u = (int)(e - (int64_t)i * U);
            const unsigned char* row = win + (int64_t)i * p.W;
            const int head = min(p.WW, (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u));
            const int nvec = (p.WW - head) >> 4;
            if (u >= 1 && u <= nvec) {
                const uint4 v = *reinterpret_cast<const uint4*>(row + head + (u - 1) * 16);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
                nb = 16;
            } else if (u == 0 || u == nvec + 1) {
                const unsigned char* q = u == 0 ? row : row + head + nvec * 16;
                nb = u == 0 ? head : p.WW - head - nvec * 16;
#pragma unroll
                for (int k = 0; k < 15; ++k)
                    if (k < nb) w[k >> 2] |= (unsigned int)q[k] << (8 * (k & 3));
            }
        }
        // through the LUT: bin[j] holds four bins as bytes, live[j] 0x80 in every byte that is still to be counted
        unsigned int bin[4] = {0u, 0u, 0u, 0u}, live[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int b = lut[(w[k >> 2] >> (8 * (k & 3))) & 255u];
            bin[k >> 2] |= (unsigned int)(b & 255) << (8 * (k & 3));
            if (k < nb && b >= 0) live[k >> 2] |= 0x80u << (8 * (k & 3));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            for (;;) {
                const unsigned long long lanes = __ballot(live[j] != 0u);
                if (!lanes) break;
                // the bin of the first live byte of the first lane that has one; then every lane counts ALL its bytes of that bin
                const unsigned int cur = (bin[j] >> ((__ffs((int)live[j]) - 8) & 31)) & 255u;
                const unsigned int b = __builtin_amdgcn_readlane(cur, __ffsll(lanes) - 1);
                int n = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned int eq = zero_bytes(bin[i] ^ (b * 0x01010101u)) & live[i];
                    live[i] &= ~eq;
                    n += __popc(eq);
                }
                n = wave_sum_i(n);
                if (lane == 0) mine[b] += (unsigned int)n;
            }
        }
    }
    __syncthreads();
    if (tid < p.K) {                                        // this workgroup is the only writer of row m: plain 64-bit adds
        long long s = 0;
#pragma unroll
        for (int v = 0; v < NTHREADS / WAVE; ++v) s += bins[v][tid];
        p.hist[(int64_t)m * p.K + tid] += s;
    }
}

int launch_tile_label_hist(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    HistP p{};
    p.labels = r.ptr<const unsigned char>(op.t[S2K_TILE_LABEL_HIST_T_LABELS]);
    p.index = r.ptr<const int>(op.t[S2K_TILE_LABEL_HIST_T_INDEX]);
    p.lut = r.ptr<const int>(op.t[S2K_TILE_LABEL_HIST_T_LUT]);
    p.hist = r.ptr<long long>(op.t[S2K_TILE_LABEL_HIST_T_HIST]);
    if (r.absent) return r.fault("tile_label_hist");
    if (!p.labels || !p.index || !p.lut || !p.hist) { set_error("tile_label_hist: missing tensor"); return S2K_EINVAL; }
    const int* d = op.d;
    p.M = d[S2K_TILE_LABEL_HIST_D_M]; p.H = d[S2K_TILE_LABEL_HIST_D_H]; p.W = d[S2K_TILE_LABEL_HIST_D_W]; p.K = d[S2K_TILE_LABEL_HIST_D_K];
    p.Y0 = d[S2K_TILE_LABEL_HIST_D_Y0]; p.X0 = d[S2K_TILE_LABEL_HIST_D_X0]; p.WH = d[S2K_TILE_LABEL_HIST_D_WH]; p.WW = d[S2K_TILE_LABEL_HIST_D_WW];
    const int nsrc = d[S2K_TILE_LABEL_HIST_D_NSRC];
    if (p.M <= 0 || p.H <= 0 || p.W <= 0 || nsrc <= 0 || p.K < 1 || p.K > 256 || p.Y0 < 0 || p.X0 < 0 || p.WH <= 0 || p.WW <= 0 ||
        (int64_t)p.Y0 + p.WH > p.H || (int64_t)p.X0 + p.WW > p.W || (int64_t)p.WH * p.WW >= (1ll << 32)) {
        set_error("tile_label_hist: bad dims (1 <= K <= 256, the window must lie inside the tile and hold < 2^32 pixels)"); return S2K_EINVAL;
    }
    static_assert(NTHREADS == 256, "tile_label_hist_kernel loads the 256 LUT entries one per thread");
    hipLaunchKernelGGL(tile_label_hist_kernel, dim3(p.M), dim3(NTHREADS), 0, c.stream, p);
    return S2K_OK;
}

struct MomP {
    const short* raw;
    const int* index;              // [M]
    unsigned long long* sums;      // [C][2], two's complement: the adds are those of the int64 sums
    double* sdpart;                // [C][NB]
    int M, C, HW, NB;
};

constexpr int MOM_POS = 8;         // positions per thread: one 16-byte load per tile
constexpr int MOM_UNROLL = 8;      // tiles whose loads are in flight per thread: its stream is 16 bytes every C*H*W*2 bytes, so only
                                   // memory-level parallelism ACROSS tiles fills HBM

template <bool VEC>
__device__ __forceinline__ void mom_load(const short* q, int n, short (&x)[MOM_POS]) {
    if (VEC) {
        const uint4 v = *reinterpret_cast<const uint4*>(q);
        const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < MOM_POS; ++k) x[k] = (short)(w[k >> 1] >> (16 * (k & 1)));
    } else {
#pragma unroll
        for (int k = 0; k < MOM_POS; ++k) x[k] = k < n ? q[k] : (short)0;
    }
}

// grid: (NB, C); thread t of block blk owns positions (blk * 256 + t) * 8 .. + 7 of band blockIdx.y.  VEC: H*W % 8 == 0 and RAW is
// 16-byte aligned, so every plane base and every thread's first position is; otherwise scalar loads with a guarded tail.
template <bool VEC>
__global__ void __launch_bounds__(NTHREADS) tile_moments_kernel(const MomP p) {
    __shared__ double red[NTHREADS / WAVE];
    const int c = blockIdx.y;
    const int p0 = (blockIdx.x * NTHREADS + threadIdx.x) * MOM_POS;
    const int n = min(MOM_POS, p.HW - p0);                  // <= 0: nothing to do here (the thread still joins the block sums)
    const int64_t plane = (int64_t)p.HW, tile = (int64_t)p.C * plane;
    const short* base = p.raw + (int64_t)c * plane + p0;
    int s1[MOM_POS];
    long long s2[MOM_POS];
#pragma unroll
    for (int k = 0; k < MOM_POS; ++k) { s1[k] = 0; s2[k] = 0; }
    if (n > 0) {
        int m = 0;
        for (; m + MOM_UNROLL <= p.M; m += MOM_UNROLL) {
            short x[MOM_UNROLL][MOM_POS];
#pragma unroll
            for (int j = 0; j < MOM_UNROLL; ++j) mom_load<VEC>(base + p.index[m + j] * tile, n, x[j]);
#pragma unroll
            for (int j = 0; j < MOM_UNROLL; ++j)
#pragma unroll
                for (int k = 0; k < MOM_POS; ++k) { const int v = x[j][k]; s1[k] += v; s2[k] += (long long)(v * v); }
        }
        for (; m < p.M; ++m) {
            short x[MOM_POS];
            mom_load<VEC>(base + p.index[m] * tile, n, x);
#pragma unroll
            for (int k = 0; k < MOM_POS; ++k) { const int v = x[k]; s1[k] += v; s2[k] += (long long)(v * v); }
        }
    }
    // per position: unbiased std across the M samples from the exact integer numerator M*s2 - s1^2 (< 2^63 for M <= 65535)
    long long t1 = 0;
    unsigned long long t2 = 0;
    double sd = 0.0;
    const double denom = (double)p.M * (double)(p.M - 1);
#pragma unroll
    for (int k = 0; k < MOM_POS; ++k) {
        t1 += s1[k];
        t2 += (unsigned long long)s2[k];
        if (p.M > 1 && k < n) sd += sqrt((double)((long long)p.M * s2[k] - (long long)s1[k] * (long long)s1[k]) / denom);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { t1 += __shfl_xor(t1, o, 64); t2 += __shfl_xor(t2, o, 64); }
    if ((threadIdx.x & 63) == 0) {                          // integer adds commute: atomics leave the result order-free
        atomicAdd(p.sums + 2 * c, (unsigned long long)t1);
        atomicAdd(p.sums + 2 * c + 1, t2);
    }
    sd = block_sum_d(sd, red);                              // fixed order: lanes by butterfly, then waves 0..3
    if (threadIdx.x == 0) p.sdpart[(int64_t)c * p.NB + blockIdx.x] = sd;      // one writer per slot
}

int launch_tile_moments(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    MomP p{};
    p.raw = r.ptr<const short>(op.t[S2K_TILE_MOMENTS_T_RAW]);
    p.index = r.ptr<const int>(op.t[S2K_TILE_MOMENTS_T_INDEX]);
    p.sums = r.ptr<unsigned long long>(op.t[S2K_TILE_MOMENTS_T_SUMS]);
    p.sdpart = r.ptr<double>(op.t[S2K_TILE_MOMENTS_T_SDPART]);
    if (r.absent) return r.fault("tile_moments");
    if (!p.raw || !p.index || !p.sums || !p.sdpart) { set_error("tile_moments: missing tensor"); return S2K_EINVAL; }
    p.M = op.d[S2K_TILE_MOMENTS_D_M]; p.C = op.d[S2K_TILE_MOMENTS_D_C]; p.NB = op.d[S2K_TILE_MOMENTS_D_NB];
    const int H = op.d[S2K_TILE_MOMENTS_D_H], W = op.d[S2K_TILE_MOMENTS_D_W], nsrc = op.d[S2K_TILE_MOMENTS_D_NSRC];
    const int64_t hw = (int64_t)H * W;
    if (p.M <= 0 || p.M > 65535 || p.C <= 0 || p.C > 65535 || H <= 0 || W <= 0 || nsrc <= 0 || hw > 0x7fffffffll / 2 ||
        (int64_t)p.M * hw >= (1ll << 34)) {
        set_error("tile_moments: bad dims (1 <= M <= 65535 keeps the integer sums exact, M*H*W < 2^34 keeps the sum of squares in 64 bits)");
        return S2K_EINVAL;
    }
    p.HW = (int)hw;
    const int per_block = NTHREADS * MOM_POS;
    if (p.NB != cdiv(p.HW, per_block)) { set_error("tile_moments: NB must be ceil(H*W / %d)", per_block); return S2K_EINVAL; }
    const bool vec = (p.HW % MOM_POS) == 0 && (reinterpret_cast<uintptr_t>(p.raw) & 15u) == 0;
    if (vec) hipLaunchKernelGGL(tile_moments_kernel<true>, dim3(p.NB, p.C), dim3(NTHREADS), 0, c.stream, p);
    else hipLaunchKernelGGL(tile_moments_kernel<false>, dim3(p.NB, p.C), dim3(NTHREADS), 0, c.stream, p);
    return S2K_OK;
}

}  // namespace s2k
