// Class-map neighbourhood filters (classmap.py; C entry s2k_classmap_filter, include/s2k.h): the k x k majority (mode) filter that takes
// the salt-and-pepper out of a predicted land-cover map, and the ignore band around label boundaries.  Both are one kernel: the
// per-pixel histogram of classes over the size x size window [y-r, y+r] x [x-r, x+r] clipped to the image (r = size / 2, no padding,
// maps never see each other).  The reference has neither (its maps end at per-crop argmax, its labels are rasterised OSM polygons used
// as they come: src/data/s2osm_dataset.py:51-71); the definition in include/s2k.h is the oracle.
//
// The histogram is kept as PACKED BYTE COUNTERS: size <= 15 means at most 225 votes per class, so four classes share a dword and K <= 32
// classes are KD = ceil(K / 4) dwords.  Adding or removing a pixel, a row or a column histogram is one 32-bit add or sub per dword; every
// partial sum is the true count of some sub-window, so no byte overflows or borrows.
//
// One wave owns a strip of 64 columns (lane l holds column x0 - r + l; lanes r .. 63 - r are outputs, CLASSMAP_STRIP - 2r of them) and
// walks down a band of CLASSMAP_BAND rows.  Each lane keeps its column's vertical histogram in KD registers: the row entering the window
// is added, the row leaving it subtracted (both re-read, one row ahead of their use: they sit in L1 / L2), the band is primed with the r rows above it.  The `size`
// neighbouring column histograms are summed across lanes with wave shuffles in a doubling scheme (S1, S2, S4, S8: at most 6 shuffles per
// dword at size 15) - never a prefix sum over the wave, whose 64 x 15 would overflow a byte.  Everything is unrolled over KD and over
// the classes: no register is selected by a run-time index, so nothing goes to scratch.  VALU / LDS-crossbar bound: it moves 2 - 16 bytes
// per pixel.
//
// A workgroup is ONE wave, so a single 512 x 512 map at size 5 is already 9 strips x 32 bands = 288 workgroups - except with HIST, where
// four waves on consecutive bands share the bins: every workgroup ends with up to K x K atomics on the SAME K x K global counters, and
// at 73,728 one-wave workgroups (256 maps) those queued for longer than the filter ran (1.01 ms against 0.39 ms).  HIST is accumulated as
// WINDOW_BLEND's (csrc/predict.hip): 32-bit LDS bins per workgroup (it counts at most 16 x 62 pixels; several copies of each bin where
// K is small, so that a wave's adds do not queue on one address), then one 64-bit atomic per non-zero bin; CHANGED is one 64-bit atomic
// per workgroup.  Integer sums: exact, independent of launch geometry.
#include "plain.h"

namespace s2k {

constexpr int CLASSMAP_STRIP = WAVE;        // columns a wave holds; CLASSMAP_STRIP - 2r of them are outputs
constexpr int CLASSMAP_BAND = 16;           // output rows a wave walks
constexpr int CLASSMAP_MAXK = 32;
constexpr int CLASSMAP_MAJORITY = 0, CLASSMAP_BOUNDARY = 1;
constexpr int CLASSMAP_HIST_WAVES = NTHREADS / WAVE;        // waves (bands) per workgroup when HIST is counted: they share its LDS bins, so a
                                                            // quarter as many workgroups queue their atomics on the K x K global counters
constexpr int64_t CLASSMAP_MAX_GRID = (1ll << 24) - 1;      // workgroups of up to 256 threads: fewer than 2^32 threads in the grid

struct ClassmapP {
    const void* src;                // [M][H][W] uint8 or int64
    void* dst;                      // [M][H][W] uint8 or int64
    const int* src_lut;             // [256] or null
    const unsigned char* labels;    // [NSRC][H][W]
    const int* index;               // [M]
    const int* lut;                 // [256]
    unsigned long long* hist;       // [K][K] or null
    unsigned long long* changed;    // [M] or null
    int M, H, W, K, R, NSRC;
    int src8, dst8;                 // 8-byte elements
    int ignore;
    unsigned votes, fixed;          // MAJORITY: as given; BOUNDARY: votes = every class
    int NS, NB, NBG;                // strips per row, bands per map, workgroups (band groups) per strip of a map
};

// the class of pixel `off` of the map at `src` (a 64-bit value: an int64 map may hold anything)
__device__ __forceinline__ long long classmap_load(const ClassmapP& p, const void* src, int off) {
    if (p.src8) return static_cast<const long long*>(src)[off];
    const int raw = static_cast<const unsigned char*>(src)[off];
    return p.src_lut ? (long long)p.src_lut[raw] : (long long)raw;
}

// the class of pixel (yy, x) of the map at `src`; -1, which never votes, where the image has no such pixel (`col`: x is inside)
__device__ __forceinline__ long long classmap_pixel(const ClassmapP& p, const void* src, bool col, int yy, int x) {
    return (col && yy >= 0 && yy < p.H) ? classmap_load(p, src, yy * p.W + x) : -1ll;
}

// +1 (or -1, by `sub`) on the packed byte counter of class c in the column histogram, if c is a class that votes
template <int KD>
__device__ __forceinline__ void classmap_count(unsigned (&h)[KD], long long c, unsigned votes, bool sub) {
    const bool ok = (unsigned long long)c < 32ull && ((votes >> (int)(c & 31)) & 1u);
    const unsigned inc = ok ? (1u << (((int)c & 3) * 8)) : 0u;
    const int d = (int)c >> 2;
#pragma unroll
    for (int i = 0; i < KD; ++i) {
        const unsigned v = d == i ? inc : 0u;
        h[i] = sub ? h[i] - v : h[i] + v;
    }
}

// copies of each of `n` HIST bins that fit 1024 LDS counters: a power of two, at most 16 (the flush sums them unrolled)
constexpr int classmap_copies(int n) {
    int c = 1;
    while (c < 16 && 2 * c * n <= 1024) c *= 2;
    return c;
}

// grid: M * NBG * NS workgroups; workgroup ((m * NBG + band group) * NS + strip), its waves (one, or CLASSMAP_HIST_WAVES with HIST) on
// consecutive bands of that strip.  The waves meet only at the barriers around the HIST bins.
template <int KD, int MODE>
__global__ void __launch_bounds__(NTHREADS) classmap_filter_kernel(const ClassmapP p) {
    constexpr int KP = 4 * KD;                                   // classes the packed histogram has room for (K <= KP)
    // HIST bins, COPIES of each side by side (lane l adds to copy l % COPIES): a map is mostly agreement, so a wave's 64 adds would
    // otherwise queue on a handful of LDS addresses.  At most 1024 counters (4 KiB): 16 copies up to K = 8, 4 to 16, 2 to 20
    constexpr int COPIES = classmap_copies(KP * KP);
    __shared__ unsigned int bins[KP * KP * COPIES];
    const int lane = threadIdx.x & (WAVE - 1), K = p.K, r = p.R, H = p.H, W = p.W;
    const unsigned bid = blockIdx.x;
    const int strip = (int)(bid % (unsigned)p.NS);
    const unsigned mb = bid / (unsigned)p.NS;
    const int m = (int)(mb / (unsigned)p.NBG);
    const int band = (int)(mb % (unsigned)p.NBG) * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    const bool live = band < p.NB;                               // a wave past the last band only keeps the barriers
    if (p.hist) {
        for (int i = threadIdx.x; i < K * K * COPIES; i += blockDim.x) bins[i] = 0u;
        __syncthreads();
    }
    const int64_t mapoff = (int64_t)m * H * W;
    const void* src = p.src8 ? static_cast<const void*>(static_cast<const long long*>(p.src) + mapoff)
                             : static_cast<const void*>(static_cast<const unsigned char*>(p.src) + mapoff);
    const int x = strip * (CLASSMAP_STRIP - 2 * r) - r + lane;   // this lane's column
    const bool col = x >= 0 && x < W;
    const bool outl = lane >= r && lane < CLASSMAP_STRIP - r && x < W;      // x >= 0 follows from lane >= r
    const int y0 = live ? band * CLASSMAP_BAND : H, y1 = live ? min(y0 + CLASSMAP_BAND, H) : H;
    const unsigned votes = p.votes;

    unsigned h[KD];
#pragma unroll
    for (int i = 0; i < KD; ++i) h[i] = 0u;
    for (int yy = max(y0 - r, 0); live && yy < min(y0 + r, H); ++yy)     // prime: the rows of the first window but its last
        classmap_count<KD>(h, classmap_pixel(p, src, col, yy, x), votes, false);

    const unsigned char* lab = nullptr;
    if (p.hist) {
        const int s = p.index[m];
        if ((unsigned)s < (unsigned)p.NSRC) lab = p.labels + (int64_t)s * H * W;
    }
    // the doubling scheme reads lane + 1, + 2, + 4; the pieces of a window are gathered from these lanes (all inside 0..63 for an
    // output lane: the window spans lanes lane - r .. lane + r)
    const int left = lane - r, size = 2 * r + 1;
    unsigned nchanged = 0u;
    // the three pixels a row needs - entering, centre, leaving - are loaded one row ahead: a wave that loaded each where it uses it
    // sat in s_waitcnt for 85 % of its cycles (three L2 round trips per row, in series)
    long long enter = 0, centre = 0, leave = 0;
    if (y0 < y1) {
        enter = classmap_pixel(p, src, col, y0 + r, x);
        centre = classmap_pixel(p, src, col, y0, x);
        leave = classmap_pixel(p, src, col, y0 - r, x);
    }
    for (int y = y0; y < y1; ++y) {
        const long long ce = enter, c = centre, cl = leave;
        if (y + 1 < y1) {
            enter = classmap_pixel(p, src, col, y + 1 + r, x);
            centre = classmap_pixel(p, src, col, y + 1, x);
            leave = classmap_pixel(p, src, col, y + 1 - r, x);
        }
        classmap_count<KD>(h, ce, votes, false);
        unsigned w[KD];
#pragma unroll
        for (int i = 0; i < KD; ++i) {
            // S_n[l] = h[l] + ... + h[l + n - 1]; window = the pieces of size's binary digits, largest first, from `left` on
            const unsigned s1 = h[i];
            const unsigned s2 = s1 + (unsigned)__shfl_down((int)s1, 1);
            unsigned s4 = 0u, s8 = 0u, acc = 0u;
            int at = left;
            if (size >= 4) s4 = s2 + (unsigned)__shfl_down((int)s2, 2);
            if (size >= 8) s8 = s4 + (unsigned)__shfl_down((int)s4, 4);
            if (size & 8) { acc += (unsigned)__shfl((int)s8, at & 63); at += 8; }
            if (size & 4) { acc += (unsigned)__shfl((int)s4, at & 63); at += 4; }
            if (size & 2) { acc += (unsigned)__shfl((int)s2, at & 63); at += 2; }
            acc += (unsigned)__shfl((int)s1, at & 63);          // size is odd
            w[i] = acc;
        }
        if (outl) {
            const int off = y * W + x;
            const bool inr = (unsigned long long)c < (unsigned long long)K;
            const int ci = (int)c & 31;
            long long o = c;
            if (inr) {
                unsigned own = 0u;                               // the dword that holds the centre's counter
#pragma unroll
                for (int i = 0; i < KD; ++i) own = (ci >> 2) == i ? w[i] : own;
                if (MODE == CLASSMAP_MAJORITY) {
                    const unsigned cc = (own >> ((ci & 3) * 8)) & 0xffu;
                    unsigned best = 0u;
                    int arg = 0;
#pragma unroll
                    for (int k = 0; k < KP; ++k) {
                        const unsigned n = (w[k >> 2] >> ((k & 3) * 8)) & 0xffu;
                        if (n > best) { best = n; arg = k; }    // strict >: the lowest index among equals
                    }
                    if (!(cc == best || ((p.fixed >> ci) & 1u))) o = arg;      // best == 0 gives cc == best
                } else if (ci != p.ignore) {
                    // any counter left once the centre's and the ignored class's are cleared: another class is in the window
                    unsigned other = 0u;
#pragma unroll
                    for (int i = 0; i < KD; ++i) {
                        unsigned v = w[i];
                        if ((ci >> 2) == i) v &= ~(0xffu << ((ci & 3) * 8));
                        if ((p.ignore >> 2) == i) v &= ~(0xffu << ((p.ignore & 3) * 8));
                        other |= v;
                    }
                    if (other) o = p.ignore;
                }
            }
            if (p.dst8) static_cast<long long*>(p.dst)[mapoff + off] = o;
            else static_cast<unsigned char*>(p.dst)[mapoff + off] = (unsigned char)o;
            nchanged += o != c ? 1u : 0u;
            if (lab) {
                const int t = p.lut[lab[off]];
                if ((unsigned)t < (unsigned)K && (unsigned long long)o < (unsigned long long)K) atomicAdd(&bins[(t * K + (int)o) * COPIES + (lane & (COPIES - 1))], 1u);
            }
        }
        classmap_count<KD>(h, cl, votes, true);
    }
    if (p.changed) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) nchanged += (unsigned)__shfl_xor((int)nchanged, s);
        if (lane == 0 && nchanged) atomicAdd(p.changed + m, (unsigned long long)nchanged);
    }
    if (p.hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < K * K; i += blockDim.x) {
            unsigned n = 0u;
#pragma unroll
            for (int c = 0; c < COPIES; ++c) n += bins[i * COPIES + ((c + lane) & (COPIES - 1))];      // staggered: no two lanes on a bank
            if (n) atomicAdd(p.hist + i, (unsigned long long)n);
        }
    }
}

// Every argument checked and the kernel's parameters derived, in plain host code without a HIP call (as mae_panels_params).
static int classmap_params(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K,
                           int size, int mode, unsigned votes, unsigned fixed, int ignore, const unsigned char* labels, const int* index,
                           const int* lut, int nsrc, unsigned long long* hist, unsigned long long* changed, ClassmapP& p) {
    if (!src || !dst) { set_error("classmap_filter: null pointer (src and dst are required)"); return S2K_EFAULT; }
    if ((src_bytes != 1 && src_bytes != 8) || (dst_bytes != 1 && dst_bytes != 8)) {
        set_error("classmap_filter: element widths must be 1 (uint8) or 8 (int64) bytes, got %d and %d", src_bytes, dst_bytes);
        return S2K_EINVAL;
    }
    if (src_lut && src_bytes != 1) { set_error("classmap_filter: src_lut reads a 1-byte src only"); return S2K_EINVAL; }
    if (src == dst) { set_error("classmap_filter: dst must not alias src"); return S2K_EINVAL; }
    if (K < 1 || K > CLASSMAP_MAXK) { set_error("classmap_filter: K = %d outside 1..%d", K, CLASSMAP_MAXK); return S2K_EINVAL; }
    if (size < 3 || size > 15 || !(size & 1)) { set_error("classmap_filter: size = %d must be odd, in 3..15", size); return S2K_EINVAL; }
    if (mode != CLASSMAP_MAJORITY && mode != CLASSMAP_BOUNDARY) { set_error("classmap_filter: mode %d (0 majority, 1 boundary)", mode); return S2K_EINVAL; }
    const unsigned all = K == 32 ? 0xffffffffu : (1u << K) - 1u;
    if (mode == CLASSMAP_MAJORITY && ((votes & ~all) || (fixed & ~all))) {
        set_error("classmap_filter: votes / fixed name a class at or above K = %d", K);
        return S2K_EINVAL;
    }
    if (mode == CLASSMAP_BOUNDARY && (votes || fixed)) { set_error("classmap_filter: votes and fixed must be 0 in boundary mode"); return S2K_EINVAL; }
    if (mode == CLASSMAP_BOUNDARY && (ignore < 0 || ignore >= K)) { set_error("classmap_filter: ignore = %d outside [0, %d)", ignore, K); return S2K_EINVAL; }
    if (M < 1 || H < 1 || W < 1) { set_error("classmap_filter: bad dims (M, H and W must be positive)"); return S2K_EINVAL; }
    if ((int64_t)H * W > 0x7fffffffll) { set_error("classmap_filter: bad dims (H * W must stay below 2^31: offsets inside a map are 32-bit)"); return S2K_EINVAL; }
    const int r = size / 2;
    const int64_t ns = cdiv64(W, CLASSMAP_STRIP - 2 * r), nb = cdiv64(H, CLASSMAP_BAND);
    if (ns * nb > CLASSMAP_MAX_GRID || ns * nb * M > CLASSMAP_MAX_GRID) {
        set_error("classmap_filter: bad dims (M * strips * bands must stay below 2^24 workgroups)");
        return S2K_EINVAL;
    }
    if (hist && (!labels || !index || !lut || nsrc < 1)) {
        set_error("classmap_filter: hist needs labels, index, lut and nsrc >= 1");
        return S2K_EINVAL;
    }
    p = ClassmapP{};
    p.src = src; p.dst = dst; p.src_lut = src_lut; p.labels = labels; p.index = index; p.lut = lut; p.hist = hist; p.changed = changed;
    p.M = M; p.H = H; p.W = W; p.K = K; p.R = r; p.NSRC = nsrc;
    p.src8 = src_bytes == 8; p.dst8 = dst_bytes == 8;
    p.ignore = mode == CLASSMAP_BOUNDARY ? ignore : 0;
    p.votes = mode == CLASSMAP_BOUNDARY ? all : votes;
    p.fixed = fixed;
    p.NS = (int)ns; p.NB = (int)nb;
    p.NBG = hist ? cdiv(p.NB, CLASSMAP_HIST_WAVES) : p.NB;
    return S2K_OK;
}

int check_classmap_filter(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K, int size,
                          int mode, unsigned votes, unsigned fixed, int ignore, const unsigned char* labels, const int* index, const int* lut,
                          int nsrc, unsigned long long* hist, unsigned long long* changed) {
    ClassmapP p;
    return classmap_params(src, src_bytes, src_lut, dst, dst_bytes, M, H, W, K, size, mode, votes, fixed, ignore, labels, index, lut, nsrc,
                           hist, changed, p);
}

template <int KD>
static void classmap_launch_kd(const ClassmapP& p, int mode, unsigned grid, hipStream_t st) {
    const dim3 block(p.hist ? NTHREADS : WAVE);
    if (mode == CLASSMAP_BOUNDARY) hipLaunchKernelGGL((classmap_filter_kernel<KD, CLASSMAP_BOUNDARY>), dim3(grid), block, 0, st, p);
    else hipLaunchKernelGGL((classmap_filter_kernel<KD, CLASSMAP_MAJORITY>), dim3(grid), block, 0, st, p);
}

int launch_classmap_filter(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K, int size,
                           int mode, unsigned votes, unsigned fixed, int ignore, const unsigned char* labels, const int* index, const int* lut,
                           int nsrc, unsigned long long* hist, unsigned long long* changed, hipStream_t st) {
    ClassmapP p;
    const int rc = classmap_params(src, src_bytes, src_lut, dst, dst_bytes, M, H, W, K, size, mode, votes, fixed, ignore, labels, index, lut,
                                   nsrc, hist, changed, p);
    if (rc != S2K_OK) return rc;
    const unsigned grid = (unsigned)((int64_t)p.M * p.NS * p.NBG);
    switch ((K + 3) / 4) {
        case 1: classmap_launch_kd<1>(p, mode, grid, st); break;
        case 2: classmap_launch_kd<2>(p, mode, grid, st); break;
        case 3: classmap_launch_kd<3>(p, mode, grid, st); break;
        case 4: classmap_launch_kd<4>(p, mode, grid, st); break;
        case 5: classmap_launch_kd<5>(p, mode, grid, st); break;
        case 6: classmap_launch_kd<6>(p, mode, grid, st); break;
        case 7: classmap_launch_kd<7>(p, mode, grid, st); break;
        default: classmap_launch_kd<8>(p, mode, grid, st); break;
    }
    return S2K_OK;
}

}  // namespace s2k
