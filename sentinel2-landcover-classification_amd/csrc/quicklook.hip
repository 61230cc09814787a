// Tile quicklooks on the GPU (data/quicklook.py, render.py; stages TILE_RADIX_HIST, TILE_RANK_PICK, TILE_QUICKLOOK, CLASS_OVERLAY): the
// picture side of the reference's per-epoch loop - `np.percentile(image, (2, 98))` over the three display bands of ONE tile jointly, the
// stretch to uint8 (src/plotting.py:75-96) and the class masks laid over it (src/train_segmentation.py:166-219) - from what is resident
// in HBM already: the raw int16 tiles of GpuTilePipeline and the int64 class maps of TilePredictor.
//
// The percentile is an exact order statistic of 786,432 int16 values per tile.  It is found WITHOUT a sort by a two-level radix select
// over key(v) = (uint16)(v + 32768), which keeps the order: count the high bytes (PASS 0), pick the high byte that holds each rank
// (STEP 0), count the low bytes of the values with that high byte (PASS 1), pick the low byte (STEP 1) - four records of one program,
// two streaming reads, no host in between.  Everything is integer or separately rounded f64 arithmetic in a fixed order (no FMA
// contraction, no float atomics; integer atomics commute): results equal the numpy restatement bit for bit and repeat from run to run.
#include "common.h"

namespace s2k {

// ---- TILE_RADIX_HIST ------------------------------------------------------------------------------------------------------------
constexpr int RSEL_CHUNK = 16384;       // values per work item: 256 threads x 8 vectors of 8 int16
constexpr int RSEL_UNROLL = 4;          // 16-byte loads a thread keeps in flight
constexpr int RSEL_REPSH0 = 3;          // log2 of the copies of the 256 coarse bins in LDS: 8 copies, 8 KiB
constexpr int RSEL_MAX_R = 8;
constexpr int RSEL_TARGET_WGS = 4096;   // workgroups a launch aims at (16 per CU)

struct RadixP {
    const short* raw;
    const int* index;                   // [M]
    const int* bands;                   // [NBND]
    const int* bucket;                  // [G][R], PASS 1
    unsigned long long* hist;           // two's complement: the adds are those of the int64 counts
    int M, C, HW, NBND, POOLED, R, NCH, NSL, REPSH;      // REPSH: log2 of the copies of every LDS bin
};

// log2 of the copies of the R x 256 fine bins: as many as fit 16 KiB (so that LDS never limits the waves per CU), at most 16
static int fine_repsh(int R) { return R == 1 ? 4 : (R == 2 ? 3 : (R <= 4 ? 2 : 1)); }

// A group is P planes of H*W contiguous int16 (POOLED: band BANDS[g] of the M tiles; else the NBND bands of tile INDEX[g]); a plane is
// cut into NCH chunks of RSEL_CHUNK values and workgroup (g, slice) takes the work items slice, slice + NSL, ... of the P * NCH.  A
// chunk is read like a chunk of csrc/flat_stats.hip: the values in front of the first 16-byte boundary by threads 0..6, then 16-byte
// vectors (four unconditional loads per round), the values behind the last vector by threads 0..6.
//
// Counter form: bins in LDS, lane-replicated (thread t counts into copy t % REP; copy c of bin b at b * REP + c), one LDS atomic per
// value.  Sentinel-2 reflectances sit in about twenty high bytes and nodata is a run of zeros, so a wave's 64 atomics land on a few
// addresses and serialise: with ONE copy of the coarse bins a selection takes twice as long on such data.  Eight copies of the
// coarse bins remove that; the fine bins get as many copies as fit 16 KiB (four for the quicklook's R = 4) - beyond 16 KiB per
// workgroup LDS, not registers, limits the waves per CU, and this is a latency-bound HBM stream.  Measured and NOT taken: combining
// runs of equal bins among a thread's eight values into one atomic (COMBINE, tuning build only) - its data-dependent branches cost
// more than the atomics they save, on smooth data too.  (The bin-by-bin ballot count of tile_label_hist_kernel pays one cross-lane
// round per DISTINCT bin of a wave's 512 values: right for a label map's handful of classes, not for twenty to 256 bins.)
template <int PASS, bool COMBINE>
__global__ void __launch_bounds__(NTHREADS) tile_radix_hist_kernel(const RadixP p) {
    extern __shared__ unsigned int bins[];           // PASS 0: [256][REP];  PASS 1: [R][256][REP]
    __shared__ int first[RSEL_MAX_R];                // PASS 1: the first rank with the same coarse bin as rank r
    const int REPSH = p.REPSH, REP = 1 << p.REPSH;
    const int nb = PASS == 0 ? 256 : p.R * 256;
    const int tid = threadIdx.x;
    for (int i = tid; i < nb * REP; i += NTHREADS) bins[i] = 0u;
    const int g = (int)(blockIdx.x / (unsigned)p.NSL), slice = (int)(blockIdx.x - (unsigned)g * (unsigned)p.NSL);
    // the coarse bins PASS 1 keeps; -1 matches no high byte.  The two ranks of a percentile nearly always share their coarse bin: a
    // bin that an earlier rank names already is counted once, for that rank, and its counts are written out for both.
    int bk[RSEL_MAX_R];
#pragma unroll
    for (int r = 0; r < RSEL_MAX_R; ++r) bk[r] = (PASS == 1 && r < p.R) ? p.bucket[(int64_t)g * p.R + r] : -1;
    if (PASS == 1) {
#pragma unroll
        for (int r = 0; r < RSEL_MAX_R; ++r) {
            int f = r;
#pragma unroll
            for (int s = RSEL_MAX_R - 1; s >= 0; --s)
                if (s < r && bk[s] == bk[r]) f = s;
            if (tid == 0) first[r] = f;
            if (f != r) bk[r] = -1;                  // ranks before r keep their value: later comparisons still find the first
        }
    }
    __syncthreads();
    unsigned int* mine = bins + (tid & (REP - 1));

    auto one = [&](short v) {                        // a single value (heads and tails)
        const unsigned int key = (unsigned int)((int)v + 32768);
        if (PASS == 0) {
            atomicAdd(mine + ((key >> 8) << REPSH), 1u);
        } else {
#pragma unroll
            for (int r = 0; r < RSEL_MAX_R; ++r)
                if ((int)(key >> 8) == bk[r]) atomicAdd(mine + ((r * 256 + (int)(key & 255u)) << REPSH), 1u);
        }
    };
    auto vec = [&](const uint4& q) {                 // eight values (COMBINE: runs of equal bins become one atomic)
        const unsigned int w[4] = {q.x ^ 0x80008000u, q.y ^ 0x80008000u, q.z ^ 0x80008000u, q.w ^ 0x80008000u};
        if (PASS == 0) {
            int cur = (int)((w[0] >> 8) & 255u);
            unsigned int n = 1u;
#pragma unroll
            for (int k = 1; k < 8; ++k) {
                const int h = (int)((w[k >> 1] >> (16 * (k & 1) + 8)) & 255u);
                if (COMBINE && h == cur) { ++n; } else { atomicAdd(mine + (cur << REPSH), n); cur = h; n = 1u; }
            }
            atomicAdd(mine + (cur << REPSH), n);
        } else {
#pragma unroll
            for (int r = 0; r < RSEL_MAX_R; ++r) {
                if (bk[r] < 0) continue;
                int cur = -1;
                unsigned int n = 0u;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const unsigned int key = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
                    if ((int)(key >> 8) != bk[r]) continue;
                    const int l = (int)(key & 255u);
                    if (COMBINE && l == cur) { ++n; } else { if (n) atomicAdd(mine + ((r * 256 + cur) << REPSH), n); cur = l; n = 1u; }
                }
                if (n) atomicAdd(mine + ((r * 256 + cur) << REPSH), n);
            }
        }
    };

    const int P = p.POOLED ? p.M : p.NBND;
    const int64_t items = (int64_t)P * p.NCH;
    for (int64_t w = slice; w < items; w += p.NSL) {
        const int j = (int)(w / p.NCH), k = (int)(w - (int64_t)j * p.NCH);
        const int tile = p.index[p.POOLED ? j : g], band = p.bands[p.POOLED ? g : j];
        const short* x = p.raw + ((int64_t)tile * p.C + band) * p.HW + (int64_t)k * RSEL_CHUNK;
        const int left = p.HW - k * RSEL_CHUNK;
        const int n = left < RSEL_CHUNK ? left : RSEL_CHUNK;
        int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 1);      // RAW is 2-byte aligned (launcher)
        if (head > n) head = n;
        const int nv = (n - head) >> 3, tail = n - head - 8 * nv;
        if (tid < head) one(x[tid]);
        if (nv > 0) {
            const uint4* xv = reinterpret_cast<const uint4*>(x + head);
            for (int j0 = tid; j0 < nv; j0 += RSEL_UNROLL * NTHREADS) {
                uint4 v[RSEL_UNROLL];
#pragma unroll
                for (int u = 0; u < RSEL_UNROLL; ++u) {
                    const int jj = j0 + u * NTHREADS;
                    v[u] = xv[jj < nv ? jj : nv - 1];
                }
#pragma unroll
                for (int u = 0; u < RSEL_UNROLL; ++u)
                    if (j0 + u * NTHREADS < nv) vec(v[u]);
            }
        }
        if (tid < tail) one(x[head + 8 * nv + tid]);
    }
    __syncthreads();
    unsigned long long* out = p.hist + (int64_t)g * nb;
    for (int b = tid; b < nb; b += NTHREADS) {
        const int src = PASS == 0 ? b : first[b >> 8] * 256 + (b & 255);
        unsigned int t = 0u;
        for (int r = 0; r < REP; ++r) t += bins[(src << REPSH) + r];
        if (t) {
            if (p.NSL == 1) out[b] += (unsigned long long)t;      // the only writer of this group's rows
            else atomicAdd(out + b, (unsigned long long)t);       // integer adds commute: the sum is order-free
        }
    }
}

int launch_tile_radix_hist(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    RadixP p{};
    p.raw = r.ptr<const short>(op.t[S2K_TILE_RADIX_HIST_T_RAW]);
    p.index = r.ptr<const int>(op.t[S2K_TILE_RADIX_HIST_T_INDEX]);
    p.bands = r.ptr<const int>(op.t[S2K_TILE_RADIX_HIST_T_BANDS]);
    p.bucket = r.ptr<const int>(op.t[S2K_TILE_RADIX_HIST_T_BUCKET]);
    p.hist = r.ptr<unsigned long long>(op.t[S2K_TILE_RADIX_HIST_T_HIST]);
    if (r.absent) return r.fault("tile_radix_hist");
    const int* d = op.d;
    const int pass = d[S2K_TILE_RADIX_HIST_D_PASS];
    if (!p.raw || !p.index || !p.bands || !p.hist || (pass == 1 && !p.bucket)) { set_error("tile_radix_hist: missing tensor"); return S2K_EINVAL; }
    p.M = d[S2K_TILE_RADIX_HIST_D_M]; p.C = d[S2K_TILE_RADIX_HIST_D_C]; p.NBND = d[S2K_TILE_RADIX_HIST_D_NBND];
    p.POOLED = d[S2K_TILE_RADIX_HIST_D_POOLED]; p.R = d[S2K_TILE_RADIX_HIST_D_R];
    const int H = d[S2K_TILE_RADIX_HIST_D_H], W = d[S2K_TILE_RADIX_HIST_D_W], nsrc = d[S2K_TILE_RADIX_HIST_D_NSRC];
    const int64_t hw = (int64_t)H * W;
    if (p.M <= 0 || p.C <= 0 || H <= 0 || W <= 0 || nsrc <= 0 || hw > (1ll << 30) || p.NBND < 1 || p.NBND > 16 || p.NBND > p.C ||
        (p.POOLED != 0 && p.POOLED != 1) || (pass != 0 && pass != 1) || p.R < 1 || p.R > RSEL_MAX_R ||
        (reinterpret_cast<uintptr_t>(p.raw) & 1u)) {
        set_error("tile_radix_hist: bad dims (1 <= NBND <= min(16, C), POOLED and PASS 0 or 1, 1 <= R <= 8, H*W <= 2^30, RAW 2-byte aligned)");
        return S2K_EINVAL;
    }
    p.HW = (int)hw;
    p.NCH = cdiv(p.HW, RSEL_CHUNK);
    const int G = p.POOLED ? p.NBND : p.M;
    const int64_t items = (int64_t)(p.POOLED ? p.M : p.NBND) * p.NCH;
    int64_t nsl = cdiv64(RSEL_TARGET_WGS, G);
    const int64_t need = cdiv64(items * RSEL_CHUNK, 1ll << 31);      // a workgroup's 32-bit LDS counters hold at most 2^31 values
    if (nsl < need) nsl = need;
    if (nsl > items) nsl = items;
    if ((int64_t)G * nsl > 0x7fffffffll) { set_error("tile_radix_hist: bad dims (too many groups for one launch)"); return S2K_EINVAL; }
    p.NSL = (int)nsl;
    const unsigned grid = (unsigned)((int64_t)G * nsl);
    p.REPSH = pass == 0 ? RSEL_REPSH0 : fine_repsh(p.R);
#ifdef S2K_TUNING
    // tuning build only: other replications, and the count without run combining, to compare
    static const int rep0 = tune_int("S2K_RSEL_REPSH0", -1), rep1 = tune_int("S2K_RSEL_REPSH1", -1), combine = tune_int("S2K_RSEL_COMBINE", 0);
    if (pass == 0 && rep0 >= 0 && rep0 <= 5) p.REPSH = rep0;
    if (pass == 1 && rep1 >= 0 && (p.R << rep1) <= 32) p.REPSH = rep1;
    if (combine) {
        const size_t lds = (size_t)(pass == 0 ? 256 : p.R * 256) * sizeof(unsigned int) << p.REPSH;
        if (pass == 0) hipLaunchKernelGGL((tile_radix_hist_kernel<0, true>), dim3(grid), dim3(NTHREADS), lds, c.stream, p);
        else hipLaunchKernelGGL((tile_radix_hist_kernel<1, true>), dim3(grid), dim3(NTHREADS), lds, c.stream, p);
        return S2K_OK;
    }
#endif
    const size_t lds = (size_t)(pass == 0 ? 256 : p.R * 256) * sizeof(unsigned int) << p.REPSH;      // at most 16 KiB (tuning: 32)
    if (pass == 0) hipLaunchKernelGGL((tile_radix_hist_kernel<0, false>), dim3(grid), dim3(NTHREADS), lds, c.stream, p);
    else hipLaunchKernelGGL((tile_radix_hist_kernel<1, false>), dim3(grid), dim3(NTHREADS), lds, c.stream, p);
    return S2K_OK;
}

// ---- TILE_RANK_PICK -------------------------------------------------------------------------------------------------------------
struct PickP {
    const long long* hist;
    const long long* ranks;     // [R]
    int* bucket;                // [G][R]
    long long* rest;            // [G][R]
    int* values;                // [G][R]
    const double* frac;         // [R / 2]
    double* pct;                // [G][R / 2]
    int G, R;
};

// Eight neighbouring lanes per group, lane r of them for rank r (a 256-bin prefix walk each); the pair (2q, 2q + 1) of a percentile
// sits in neighbouring lanes of one wave, so the interpolation takes its upper value with one shuffle.  numpy's linear method,
// `_lerp`: every operation rounded on its own - a contraction of a + d*t into an FMA changes the last bit.
template <int STEP>
__global__ void __launch_bounds__(NTHREADS) tile_rank_pick_kernel(const PickP p) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * NTHREADS + threadIdx.x;
    const int g = t >> 3, r = t & 7;
    const bool live = g < p.G && r < p.R;
    int val = 0;
    if (live) {
        const int64_t gr = (int64_t)g * p.R + r;
        const long long* h = p.hist + (STEP == 0 ? (int64_t)g : gr) * 256;
        const long long want = STEP == 0 ? p.ranks[r] : p.rest[gr];
        long long below = 0;
        int bin = 0;
        for (; bin < 255; ++bin) {                   // first bin whose inclusive prefix exceeds `want`; 255 if none does
            const long long cnt = h[bin];
            if (below + cnt > want) break;
            below += cnt;
        }
        if (STEP == 0) {
            p.bucket[gr] = bin;
            p.rest[gr] = want - below;
        } else {
            val = ((p.bucket[gr] << 8) | bin) - 32768;
            p.values[gr] = val;
        }
    }
    if (STEP == 1 && p.pct) {                        // wave-uniform: every lane takes part in the shuffle
        const int nxt = __shfl_down(val, 1, 64);
        if (live && !(r & 1) && r + 1 < p.R) {
            const int q = r >> 1;
            const double a = (double)val, b = (double)nxt, f = p.frac[q];
            // plain operators under the pragma above: the __dmul_rn / __dadd_rn wrappers are compiled with contraction allowed and
            // carry that permission with them when they are inlined, so the pair still becomes one v_fma_f64
            const double d = b - a;
            double res = a + d * f;
            if (f >= 0.5) res = b - d * (1.0 - f);
            p.pct[(int64_t)g * (p.R >> 1) + q] = res;
        }
    }
}

int launch_tile_rank_pick(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    PickP p{};
    p.hist = r.ptr<const long long>(op.t[S2K_TILE_RANK_PICK_T_HIST]);
    p.ranks = r.ptr<const long long>(op.t[S2K_TILE_RANK_PICK_T_RANKS]);
    p.bucket = r.ptr<int>(op.t[S2K_TILE_RANK_PICK_T_BUCKET]);
    p.rest = r.ptr<long long>(op.t[S2K_TILE_RANK_PICK_T_REST]);
    p.values = r.ptr<int>(op.t[S2K_TILE_RANK_PICK_T_VALUES]);
    p.frac = r.ptr<const double>(op.t[S2K_TILE_RANK_PICK_T_FRAC]);
    p.pct = r.ptr<double>(op.t[S2K_TILE_RANK_PICK_T_PCT]);
    if (r.absent) return r.fault("tile_rank_pick");
    const int step = op.d[S2K_TILE_RANK_PICK_D_STEP];
    p.G = op.d[S2K_TILE_RANK_PICK_D_G]; p.R = op.d[S2K_TILE_RANK_PICK_D_R];
    const int64_t N = op.n[S2K_TILE_RANK_PICK_N_N];
    if (!p.hist || !p.bucket || !p.rest || (step == 0 && !p.ranks) || (step == 1 && (!p.values || (p.pct && !p.frac)))) {
        set_error("tile_rank_pick: missing tensor"); return S2K_EINVAL;
    }
    if (p.G < 1 || p.G > (1 << 27) || p.R < 1 || p.R > RSEL_MAX_R || (step != 0 && step != 1) || N < 1 || (p.pct && p.R < 2)) {
        set_error("tile_rank_pick: bad dims (1 <= G <= 2^27 groups, 1 <= R <= 8 ranks, STEP 0 or 1, N >= 1 values per group, PCT needs R >= 2)");
        return S2K_EINVAL;
    }
    const unsigned grid = (unsigned)cdiv64((int64_t)p.G * 8, NTHREADS);
    if (step == 0) hipLaunchKernelGGL(tile_rank_pick_kernel<0>, dim3(grid), dim3(NTHREADS), 0, c.stream, p);
    else hipLaunchKernelGGL(tile_rank_pick_kernel<1>, dim3(grid), dim3(NTHREADS), 0, c.stream, p);
    return S2K_OK;
}

// ---- TILE_QUICKLOOK -------------------------------------------------------------------------------------------------------------
struct LookP {
    const short* raw;
    const int* params;          // [B][4] = {tile, y0, x0, flips}
    const int* slot;            // [B]
    const int* bands;           // [3]
    const double* pct;          // [NROW][NQ]
    unsigned char* out;         // [B][SH][SW][3]
    int B, C, H, W, SH, SW, NQ;
};

// grid: (row groups, B); one thread per 4 output columns of a row: per band one 8-byte load where the four source values are 8-byte
// aligned (element loads otherwise, and for the last columns of a width that is no multiple of 4), 12 contiguous bytes stored.
__global__ void __launch_bounds__(NTHREADS) tile_quicklook_kernel(const LookP p) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int q = (p.SW + 3) >> 2;
    const int e = blockIdx.x * NTHREADS + threadIdx.x;
    if (e >= p.SH * q) return;
    const int i = e / q, j = (e - i * q) * 4;
    const int n = p.SW - j < 4 ? p.SW - j : 4;
    const int tile = p.params[4 * b], y0 = p.params[4 * b + 1], x0 = p.params[4 * b + 2], flips = p.params[4 * b + 3];
    const int si = y0 + ((flips & 2) ? p.SH - 1 - i : i);
    const double lo = p.pct[(int64_t)p.slot[b] * p.NQ], hi = p.pct[(int64_t)p.slot[b] * p.NQ + 1];
    const bool ok = hi > lo && __builtin_isfinite(lo) && __builtin_isfinite(hi);      // a constant tile: black, not a division by zero
    const double width = hi - lo;
    unsigned char o[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const short* row = p.raw + (((int64_t)tile * p.C + p.bands[k]) * p.H + si) * p.W + x0;
        short v[4] = {0, 0, 0, 0};
        // output column j + m reads source column j + m, or SW - 1 - (j + m) under a horizontal flip
        const short* src = (flips & 1) ? row + (p.SW - 1 - j - 3) : row + j;
        if (n == 4 && (reinterpret_cast<uintptr_t>(src) & 7u) == 0) {
            const uint2 u = *reinterpret_cast<const uint2*>(src);
            const short s[4] = {(short)(u.x & 0xffffu), (short)(u.x >> 16), (short)(u.y & 0xffffu), (short)(u.y >> 16)};
#pragma unroll
            for (int m = 0; m < 4; ++m) v[m] = (flips & 1) ? s[3 - m] : s[m];
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < n) v[m] = (flips & 1) ? row[p.SW - 1 - j - m] : row[j + m];
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double r = ((double)v[m] - lo) / width * 255.0;       // this order, every operation rounded: numpy's
            r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
            o[m * 3 + k] = ok ? (unsigned char)(int)r : (unsigned char)0;
        }
    }
    unsigned char* dst = p.out + (((int64_t)b * p.SH + i) * p.SW + j) * 3;
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

// PARAMS, SLOT and BANDS are not range-checked on the device: the host (data/quicklook.py) validates them before upload.
int launch_tile_quicklook(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    LookP p{};
    p.raw = r.ptr<const short>(op.t[S2K_TILE_QUICKLOOK_T_RAW]);
    p.params = r.ptr<const int>(op.t[S2K_TILE_QUICKLOOK_T_PARAMS]);
    p.slot = r.ptr<const int>(op.t[S2K_TILE_QUICKLOOK_T_SLOT]);
    p.bands = r.ptr<const int>(op.t[S2K_TILE_QUICKLOOK_T_BANDS]);
    p.pct = r.ptr<const double>(op.t[S2K_TILE_QUICKLOOK_T_PCT]);
    p.out = r.ptr<unsigned char>(op.t[S2K_TILE_QUICKLOOK_T_OUT]);
    if (r.absent) return r.fault("tile_quicklook");
    if (!p.raw || !p.params || !p.slot || !p.bands || !p.pct || !p.out) { set_error("tile_quicklook: missing tensor"); return S2K_EINVAL; }
    const int* d = op.d;
    p.B = d[S2K_TILE_QUICKLOOK_D_B]; p.C = d[S2K_TILE_QUICKLOOK_D_C]; p.H = d[S2K_TILE_QUICKLOOK_D_H]; p.W = d[S2K_TILE_QUICKLOOK_D_W];
    p.SH = d[S2K_TILE_QUICKLOOK_D_SH]; p.SW = d[S2K_TILE_QUICKLOOK_D_SW]; p.NQ = d[S2K_TILE_QUICKLOOK_D_NQ];
    const int nsrc = d[S2K_TILE_QUICKLOOK_D_NSRC], nrow = d[S2K_TILE_QUICKLOOK_D_NROW];
    if (p.B <= 0 || p.B > 65535 || p.C <= 0 || p.H <= 0 || p.W <= 0 || p.SH <= 0 || p.SW <= 0 || p.SH > p.H || p.SW > p.W || nsrc <= 0 ||
        nrow <= 0 || p.NQ < 2 || (int64_t)p.SH * ((p.SW + 3) >> 2) > 0x7fffffffll || (reinterpret_cast<uintptr_t>(p.raw) & 1u)) {
        set_error("tile_quicklook: bad dims (1 <= B <= 65535, the SH x SW window must fit the tile, NROW >= 1 rows of NQ >= 2 percentiles)");
        return S2K_EINVAL;
    }
    const int per_image = p.SH * ((p.SW + 3) >> 2);
    hipLaunchKernelGGL(tile_quicklook_kernel, dim3(cdiv(per_image, NTHREADS), p.B), dim3(NTHREADS), 0, c.stream, p);
    return S2K_OK;
}

// ---- CLASS_OVERLAY --------------------------------------------------------------------------------------------------------------
struct OverP {
    const long long* cls;
    const unsigned char* palette;      // [K][3]
    const unsigned char* base;         // may be null: black
    unsigned char* out;
    long long count;                   // B * SH * SW pixels
    int K, A, SKIP0;
};

// One thread per 4 consecutive pixels of the flat [B*SH*SW] image: VEC (CLS 16-byte, BASE / OUT 4-byte aligned) reads the classes as
// two 16-byte loads and the picture as three dwords, and stores three dwords; otherwise element accesses.  The palette sits in LDS.
template <bool VEC>
__global__ void __launch_bounds__(NTHREADS) class_overlay_kernel(const OverP p) {
    __shared__ unsigned char pal[256 * 3];
    for (int i = threadIdx.x; i < p.K * 3; i += NTHREADS) pal[i] = p.palette[i];
    __syncthreads();
    const long long p0 = ((long long)blockIdx.x * NTHREADS + threadIdx.x) * 4;
    if (p0 >= p.count) return;
    const int n = p.count - p0 < 4 ? (int)(p.count - p0) : 4;
    long long cls[4] = {-1, -1, -1, -1};
    unsigned char px[12];
#pragma unroll
    for (int m = 0; m < 12; ++m) px[m] = 0;
    if (VEC && n == 4) {
        const longlong2 c0 = *reinterpret_cast<const longlong2*>(p.cls + p0), c1 = *reinterpret_cast<const longlong2*>(p.cls + p0 + 2);
        cls[0] = c0.x; cls[1] = c0.y; cls[2] = c1.x; cls[3] = c1.y;
        if (p.base) {
            const unsigned int* b4 = reinterpret_cast<const unsigned int*>(p.base + p0 * 3);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const unsigned int u = b4[m];
                px[4 * m] = (unsigned char)(u & 255u); px[4 * m + 1] = (unsigned char)((u >> 8) & 255u);
                px[4 * m + 2] = (unsigned char)((u >> 16) & 255u); px[4 * m + 3] = (unsigned char)(u >> 24);
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (m < n) {
                cls[m] = p.cls[p0 + m];
                if (p.base) { px[3 * m] = p.base[(p0 + m) * 3]; px[3 * m + 1] = p.base[(p0 + m) * 3 + 1]; px[3 * m + 2] = p.base[(p0 + m) * 3 + 2]; }
            }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const long long cl = cls[m];
        if (cl < 0 || cl >= p.K || (p.SKIP0 && cl == 0)) continue;      // keeps BASE
#pragma unroll
        for (int k = 0; k < 3; ++k)
            px[3 * m + k] = (unsigned char)(((int)px[3 * m + k] * (256 - p.A) + (int)pal[(int)cl * 3 + k] * p.A + 128) >> 8);
    }
    unsigned char* dst = p.out + p0 * 3;
    if (VEC && n == 4) {
        unsigned int* d4 = reinterpret_cast<unsigned int*>(dst);
#pragma unroll
        for (int m = 0; m < 3; ++m)
            d4[m] = (unsigned int)px[4 * m] | ((unsigned int)px[4 * m + 1] << 8) | ((unsigned int)px[4 * m + 2] << 16) | ((unsigned int)px[4 * m + 3] << 24);
    } else {
#pragma unroll
        for (int m = 0; m < 12; ++m)
            if (m < 3 * n) dst[m] = px[m];
    }
}

int launch_class_overlay(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    OverP p{};
    p.cls = r.ptr<const long long>(op.t[S2K_CLASS_OVERLAY_T_CLS]);
    p.palette = r.ptr<const unsigned char>(op.t[S2K_CLASS_OVERLAY_T_PALETTE]);
    p.base = r.ptr<const unsigned char>(op.t[S2K_CLASS_OVERLAY_T_BASE]);
    p.out = r.ptr<unsigned char>(op.t[S2K_CLASS_OVERLAY_T_OUT]);
    if (r.absent) return r.fault("class_overlay");
    if (!p.cls || !p.palette || !p.out) { set_error("class_overlay: missing tensor"); return S2K_EINVAL; }
    const int* d = op.d;
    const int B = d[S2K_CLASS_OVERLAY_D_B], SH = d[S2K_CLASS_OVERLAY_D_SH], SW = d[S2K_CLASS_OVERLAY_D_SW];
    p.K = d[S2K_CLASS_OVERLAY_D_K]; p.A = d[S2K_CLASS_OVERLAY_D_ALPHA]; p.SKIP0 = d[S2K_CLASS_OVERLAY_D_SKIP0];
    if (B <= 0 || SH <= 0 || SW <= 0 || p.K < 1 || p.K > 256 || p.A < 0 || p.A > 256 || (p.SKIP0 != 0 && p.SKIP0 != 1) ||
        (int64_t)B * SH * SW > (1ll << 40) || (reinterpret_cast<uintptr_t>(p.cls) & 7u)) {
        set_error("class_overlay: bad dims (1 <= K <= 256 colours, 0 <= ALPHA <= 256, SKIP0 0 or 1, at most 2^40 pixels, CLS 8-byte aligned)");
        return S2K_EINVAL;
    }
    p.count = (long long)B * SH * SW;
    const unsigned grid = (unsigned)cdiv64(p.count, 4ll * NTHREADS);
    const bool vec = (reinterpret_cast<uintptr_t>(p.cls) & 15u) == 0 && (reinterpret_cast<uintptr_t>(p.out) & 3u) == 0 &&
                     (!p.base || (reinterpret_cast<uintptr_t>(p.base) & 3u) == 0);
    if (vec) hipLaunchKernelGGL(class_overlay_kernel<true>, dim3(grid), dim3(NTHREADS), 0, c.stream, p);
    else hipLaunchKernelGGL(class_overlay_kernel<false>, dim3(grid), dim3(NTHREADS), 0, c.stream, p);
    return S2K_OK;
}

}  // namespace s2k
