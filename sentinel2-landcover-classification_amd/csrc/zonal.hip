// Zonal statistics: class votes and band statistics per polygon or per component (zonal.py; C entries s2k_zonal_histogram,
// s2k_zonal_bands, s2k_zonal_majority, s2k_zonal_paint, include/s2k.h).  A zone raster - the polygon index per pixel from
// rasterize(burn="index"), or the component labels of a class map - says which row of a table a pixel belongs to; the reference asks the
// same questions per dataset and per tile on the host (calculate_dataset_statistics.py, experiments/label_EDA.py), here they are asked per
// object.  Integer work with one exact answer: the definitions in include/s2k.h are the oracle (tests/zonal_ref.py restates them in numpy).
//
// The two counting kernels stream the rasters once.  One workgroup owns one ZONAL_BLOCK_H x ZONAL_BLOCK_W block of one map; a thread
// owns a QUAD of four neighbouring pixels of a row per pass (a wave one row of the block: 16-byte zone loads, coalesced), ZONAL_BLOCK_H *
// ZONAL_BLOCK_W / (4 * NTHREADS) passes.  Zones are spatially coherent, so a block sees few distinct keys:
//   claim   the key's HOME slot in an LDS open-addressing table of ZONAL_SLOTS keys is zonal_home(key) = (u32(key) * ZONAL_HASH) >>
//           (32 - ZONAL_SLOT_BITS); the thread compare-and-swaps its key into the first free slot among ZONAL_PROBES consecutive slots
//           (wrapping), or finds it there.  A pixel of a quad whose key equals its left neighbour's reuses that slot.
//   count   LDS atomics into the slot's counters; contributions of a quad to the same (slot, bin) are summed in registers first.  The
//           counters are u32 (a block holds 4096 pixels), the band sum i32 (below 2^27), the band sum of squares u64 (a 64-bit LDS atomic).
//   flush   after one barrier every non-empty (slot, bin) goes to the tables with ONE 64-bit global atomic (min / max: one 32-bit each).
//   overflow  a key that finds no slot within ZONAL_PROBES probes goes to the tables directly with global atomics: every-pixel-its-own-
//           zone inputs take this path, and it is the whole kernel when the table is compiled out (-DS2K_ZONAL_NO_TABLE: tools/
//           bench_zonal.py builds that variant next to the product library to measure what the table buys; never the shipped library).
// Every loop is bounded by a compile-time constant or a count passed by value.  Every zone value is range-checked in 64 bits before it
// becomes an index (a value at or above zone_limit sets ZONAL_BAD_ZONE in `status` and is skipped), every class before it becomes a bin.
// Map offsets are 64-bit, offsets inside a map 32-bit.  Integer sums: independent of the order of arrival and of how M is chunked.
#include "plain.h"

#include <climits>

namespace s2k {

constexpr int ZONAL_BLOCK_H = 16, ZONAL_BLOCK_W = 256;     // zonal.ZONAL_BLOCK_H, ZONAL_BLOCK_W: the block one workgroup owns
constexpr int ZONAL_SLOT_BITS = 6;                          // zonal.ZONAL_SLOT_BITS
constexpr int ZONAL_SLOTS = 64;                             // zonal.ZONAL_SLOTS: keys of the LDS table, 1 << ZONAL_SLOT_BITS
constexpr int ZONAL_PROBES = 8;                             // zonal.ZONAL_PROBES: slots tried before a pixel goes to global memory
constexpr unsigned ZONAL_HASH = 2654435761u;                // zonal.ZONAL_HASH: 2^32 / golden ratio, odd
constexpr int ZONAL_MAX_K = 32, ZONAL_MAX_C = 16;
constexpr unsigned ZONAL_BAD_ZONE = 1u;                     // zonal.ZONAL_BAD_ZONE: a zone value at or above zone_limit
constexpr int ZONAL_QUADS_W = ZONAL_BLOCK_W / 4;            // quads of a block row: one wave
constexpr int ZONAL_PASSES = ZONAL_BLOCK_H * ZONAL_QUADS_W / NTHREADS;
constexpr int64_t ZONAL_MAX_GRID = 0x7fffffffll;
#ifdef S2K_ZONAL_NO_TABLE
constexpr int ZONAL_TABLE_PROBES = 0;                       // measurement only: every pixel is a global atomic
#else
constexpr int ZONAL_TABLE_PROBES = ZONAL_PROBES;
#endif
static_assert(ZONAL_SLOTS == 1 << ZONAL_SLOT_BITS && ZONAL_PROBES <= ZONAL_SLOTS, "table geometry");
static_assert(ZONAL_QUADS_W == WAVE && ZONAL_PASSES * NTHREADS == ZONAL_BLOCK_H * ZONAL_QUADS_W, "a wave owns a row of quads");

struct ZonalP {
    const void* zone;               // [M][H][W], 4 or 8 bytes an element
    unsigned* status;
    long long zone_limit;           // raw values at or above it are out of range
    int zone_bytes, zone_stride;
    int M, H, W, Z;
    int NBY, NBX;                   // blocks of a map
    int vec;                        // quads are read whole: W % 4 == 0 and every raster 16-byte aligned
};

struct ZonalHistP {
    ZonalP z;
    const void* cls;                // [M][H][W], 1 or 8 bytes an element
    const int* src_lut;             // int32[256] or null
    unsigned long long* hist;       // [Z][K]
    int cls_bytes, K;
};

struct ZonalBandP {
    ZonalP z;
    const short* vals;              // [M][C][H][W]
    unsigned long long *count, *sum, *sumsq;        // [Z][C]
    int *mn, *mx;                   // [Z][C]
    int C, nodata, has_nodata;
};

struct ZonalPaintP {
    ZonalP z;
    const int* table;               // [Z]
    void* dst;                      // [M][H][W], 1, 4 or 8 bytes an element
    int dst_bytes, mode, fill;
};

__device__ __forceinline__ int zonal_home(int key) { return (int)(((unsigned)key * ZONAL_HASH) >> (32 - ZONAL_SLOT_BITS)); }

// the key of a raw zone value of map m, or -1 for "no zone"; the comparison is made in 64 bits, so an int64 raster is never truncated
__device__ __forceinline__ int zonal_key(const ZonalP& p, long long raw, int m, unsigned& bad) {
    if (raw < 0) return -1;
    if (raw >= p.zone_limit) { bad |= ZONAL_BAD_ZONE; return -1; }
    return (int)(raw + (long long)m * p.zone_stride);           // below Z: M * zone_stride == Z, or zone_stride == 0 and zone_limit == Z
}

// the keys of the n (1..4) pixels of a quad at element offset `off`
__device__ __forceinline__ void zonal_quad_keys(const ZonalP& p, int64_t off, int n, int m, int (&key)[4], unsigned& bad) {
    long long raw[4] = {-1, -1, -1, -1};
    if (p.zone_bytes == 4) {
        const int* z = static_cast<const int*>(p.zone) + off;
        if (p.vec) { const int4 v = *reinterpret_cast<const int4*>(z); raw[0] = v.x; raw[1] = v.y; raw[2] = v.z; raw[3] = v.w; }
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < n) raw[j] = z[j];
        }
    } else {
        const long long* z = static_cast<const long long*>(p.zone) + off;
        if (p.vec) {
            const longlong2 a = *reinterpret_cast<const longlong2*>(z), b = *reinterpret_cast<const longlong2*>(z + 2);
            raw[0] = a.x; raw[1] = a.y; raw[2] = b.x; raw[3] = b.y;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < n) raw[j] = z[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) key[j] = zonal_key(p, raw[j], m, bad);
}

// the slot of `key` (>= 0) in the workgroup's table, claiming it if need be; -1 after ZONAL_TABLE_PROBES probes without one
__device__ __forceinline__ int zonal_claim(int* keys, int key) {
    const int h = zonal_home(key);
#pragma unroll
    for (int i = 0; i < ZONAL_TABLE_PROBES; ++i) {
        const int s = (h + i) & (ZONAL_SLOTS - 1);
        const int old = atomicCAS(&keys[s], -1, key);
        if (old == -1 || old == key) return s;
    }
    return -1;
}

// the slots of a quad's keys: -1 overflow (or no key); a key equal to its left neighbour's shares the slot
__device__ __forceinline__ void zonal_quad_slots(int* keys, const int (&key)[4], int (&slot)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (key[j] < 0) slot[j] = -1;
        else if (ZONAL_TABLE_PROBES > 0 && j > 0 && key[j] == key[j - 1]) slot[j] = slot[j - 1];
        else slot[j] = zonal_claim(keys, key[j]);
    }
}

// block and quad geometry shared by the two counting kernels
struct ZonalBlock { int m, row0, col0; };
__device__ __forceinline__ ZonalBlock zonal_block(const ZonalP& p) {
    const unsigned per = (unsigned)(p.NBY * p.NBX), bid = blockIdx.x;
    ZonalBlock b;
    b.m = (int)(bid / per);
    b.row0 = (int)((bid % per) / (unsigned)p.NBX) * ZONAL_BLOCK_H;
    b.col0 = (int)((bid % per) % (unsigned)p.NBX) * ZONAL_BLOCK_W;
    return b;
}

// ---- HISTOGRAM: grid M * NBY * NBX ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void zonal_hist_add(const ZonalHistP& p, unsigned* cnt, int slot, int key, int c, unsigned n) {
    if (slot >= 0) atomicAdd(&cnt[slot * p.K + c], n);
    else atomicAdd(p.hist + (int64_t)key * p.K + c, (unsigned long long)n);
}

__global__ void __launch_bounds__(NTHREADS) zonal_hist_kernel(const ZonalHistP p) {
    __shared__ int keys[ZONAL_SLOTS];
    __shared__ unsigned cnt[ZONAL_SLOTS * ZONAL_MAX_K];
    const int tid = threadIdx.x, K = p.K, H = p.z.H, W = p.z.W;
    if (tid < ZONAL_SLOTS) keys[tid] = -1;
    for (int i = tid; i < ZONAL_SLOTS * K; i += NTHREADS) cnt[i] = 0u;
    __syncthreads();
    const ZonalBlock b = zonal_block(p.z);
    const int64_t map = (int64_t)b.m * H * W;
    unsigned bad = 0u;
#pragma unroll
    for (int it = 0; it < ZONAL_PASSES; ++it) {
        const int q = it * NTHREADS + tid, y = b.row0 + q / ZONAL_QUADS_W, x = b.col0 + 4 * (q % ZONAL_QUADS_W);
        if (y >= H || x >= W) continue;
        const int n = min(4, W - x);
        const int64_t off = map + (int64_t)y * W + x;
        int key[4], slot[4], c[4] = {-1, -1, -1, -1};
        zonal_quad_keys(p.z, off, n, b.m, key, bad);
        if (p.cls_bytes == 1) {
            const unsigned char* s = static_cast<const unsigned char*>(p.cls) + off;
            unsigned raw[4] = {0u, 0u, 0u, 0u};
            if (p.z.vec) { const unsigned v = *reinterpret_cast<const unsigned*>(s); raw[0] = v & 255u; raw[1] = (v >> 8) & 255u; raw[2] = (v >> 16) & 255u; raw[3] = v >> 24; }
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < n) raw[j] = s[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < n) c[j] = p.src_lut ? p.src_lut[raw[j]] : (int)raw[j];
        } else {
            const long long* s = static_cast<const long long*>(p.cls) + off;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < n) { const long long v = s[j]; c[j] = (v >= 0 && v < K) ? (int)v : -1; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) if (c[j] < 0 || c[j] >= K) key[j] = -1;      // a class outside [0, K) is skipped: it claims no slot either
        zonal_quad_slots(keys, key, slot);
        // runs of equal (key, class) inside the quad are one add
        int rk = -1, rs = -1, rc = 0;
        unsigned rn = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (key[j] < 0) continue;
            if (ZONAL_TABLE_PROBES > 0 && rn && key[j] == rk && c[j] == rc) { rn += 1u; continue; }
            if (rn) zonal_hist_add(p, cnt, rs, rk, rc, rn);
            rk = key[j]; rs = slot[j]; rc = c[j]; rn = 1u;
        }
        if (rn) zonal_hist_add(p, cnt, rs, rk, rc, rn);
    }
    if (bad) atomicOr(p.z.status, bad);
    __syncthreads();
    for (int i = tid; i < ZONAL_SLOTS * K; i += NTHREADS) {
        const unsigned v = cnt[i];
        if (v) atomicAdd(p.hist + (int64_t)keys[i / K] * K + i % K, (unsigned long long)v);    // a counted slot holds a checked key
    }
}

// ---- BANDS: grid M * NBY * NBX -------------------------------------------------------------------------------------------------------------
struct ZonalRun { int key, slot, n, sum, mn, mx; unsigned long long sq; };

__device__ __forceinline__ void zonal_band_add(const ZonalBandP& p, unsigned* cnt, int* sum, unsigned long long* sq, int* mn, int* mx, int c,
                                               const ZonalRun& r) {
    if (r.slot >= 0) {
        const int i = r.slot * p.C + c;
        atomicAdd(&cnt[i], (unsigned)r.n); atomicAdd(&sum[i], r.sum); atomicAdd(&sq[i], r.sq);
        atomicMin(&mn[i], r.mn); atomicMax(&mx[i], r.mx);
    } else {
        const int64_t i = (int64_t)r.key * p.C + c;
        atomicAdd(p.count + i, (unsigned long long)r.n);
        atomicAdd(p.sum + i, (unsigned long long)(long long)r.sum);          // two's complement: a signed add
        atomicAdd(p.sumsq + i, r.sq);
        atomicMin(p.mn + i, r.mn); atomicMax(p.mx + i, r.mx);
    }
}

__global__ void __launch_bounds__(NTHREADS) zonal_band_kernel(const ZonalBandP p) {
    __shared__ int keys[ZONAL_SLOTS];
    __shared__ unsigned cnt[ZONAL_SLOTS * ZONAL_MAX_C];
    __shared__ int sum[ZONAL_SLOTS * ZONAL_MAX_C], mn[ZONAL_SLOTS * ZONAL_MAX_C], mx[ZONAL_SLOTS * ZONAL_MAX_C];
    __shared__ unsigned long long sq[ZONAL_SLOTS * ZONAL_MAX_C];
    const int tid = threadIdx.x, C = p.C, H = p.z.H, W = p.z.W;
    if (tid < ZONAL_SLOTS) keys[tid] = -1;
    for (int i = tid; i < ZONAL_SLOTS * C; i += NTHREADS) { cnt[i] = 0u; sum[i] = 0; sq[i] = 0ull; mn[i] = INT_MAX; mx[i] = INT_MIN; }
    __syncthreads();
    const ZonalBlock b = zonal_block(p.z);
    const int64_t plane = (int64_t)H * W, map = (int64_t)b.m * plane;
    unsigned bad = 0u;
#pragma unroll 1
    for (int it = 0; it < ZONAL_PASSES; ++it) {
        const int q = it * NTHREADS + tid, y = b.row0 + q / ZONAL_QUADS_W, x = b.col0 + 4 * (q % ZONAL_QUADS_W);
        if (y >= H || x >= W) continue;
        const int n = min(4, W - x);
        const int64_t in_map = (int64_t)y * W + x;
        int key[4], slot[4];
        zonal_quad_keys(p.z, map + in_map, n, b.m, key, bad);
        if (key[0] < 0 && key[1] < 0 && key[2] < 0 && key[3] < 0) continue;
        zonal_quad_slots(keys, key, slot);
        for (int c = 0; c < C; ++c) {                               // C <= ZONAL_MAX_C, passed by value
            const short* s = p.vals + ((int64_t)b.m * C + c) * plane + in_map;
            int v[4] = {0, 0, 0, 0};
            if (p.z.vec) { const short4 w = *reinterpret_cast<const short4*>(s); v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w; }
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < n) v[j] = s[j];
            }
            ZonalRun r;
            r.n = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (key[j] < 0 || (p.has_nodata && v[j] == p.nodata)) continue;
                const unsigned long long vv = (unsigned long long)(v[j] * v[j]);      // at most 2^30
                if (ZONAL_TABLE_PROBES > 0 && r.n && key[j] == r.key) {
                    r.n += 1; r.sum += v[j]; r.sq += vv; r.mn = min(r.mn, v[j]); r.mx = max(r.mx, v[j]);
                    continue;
                }
                if (r.n) zonal_band_add(p, cnt, sum, sq, mn, mx, c, r);
                r.key = key[j]; r.slot = slot[j]; r.n = 1; r.sum = v[j]; r.sq = vv; r.mn = v[j]; r.mx = v[j];
            }
            if (r.n) zonal_band_add(p, cnt, sum, sq, mn, mx, c, r);
        }
    }
    if (bad) atomicOr(p.z.status, bad);
    __syncthreads();
    for (int i = tid; i < ZONAL_SLOTS * C; i += NTHREADS) {
        const unsigned v = cnt[i];
        if (!v) continue;                                           // nothing counted: min and max keep what the caller put there
        const int64_t o = (int64_t)keys[i / C] * C + i % C;         // a counted slot holds a checked key
        atomicAdd(p.count + o, (unsigned long long)v);
        atomicAdd(p.sum + o, (unsigned long long)(long long)sum[i]);
        atomicAdd(p.sumsq + o, sq[i]);
        atomicMin(p.mn + o, mn[i]); atomicMax(p.mx + o, mx[i]);
    }
}

// ---- MAJORITY: one thread per zone ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NTHREADS) zonal_majority_kernel(const long long* __restrict__ hist, int Z, int K, unsigned votes,
                                                                  long long min_count, int fill, int* __restrict__ out_cls,
                                                                  long long* __restrict__ out_best) {
    const int64_t z = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
    if (z >= Z) return;
    long long best = LLONG_MIN;
    int cls = fill;
    for (int c = 0; c < K; ++c) {                                   // K <= ZONAL_MAX_K; strict >: the lowest class keeps a tie
        if (!((votes >> c) & 1u)) continue;
        const long long v = hist[z * K + c];
        if (v > best) { best = v; cls = c; }
    }
    out_cls[z] = best >= min_count ? cls : fill;
    if (out_best) out_best[z] = best;
}

// ---- PAINT: one thread per pixel ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NTHREADS) zonal_paint_kernel(const ZonalPaintP p) {
    const int64_t plane = (int64_t)p.z.H * p.z.W, i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
    if (i >= plane * p.z.M) return;
    const int m = (int)(i / plane);
    unsigned bad = 0u;
    const long long raw = p.z.zone_bytes == 4 ? (long long)static_cast<const int*>(p.z.zone)[i] : static_cast<const long long*>(p.z.zone)[i];
    const int key = zonal_key(p.z, raw, m, bad);
    if (bad) atomicOr(p.z.status, bad);
    int v = key >= 0 ? p.table[key] : -1;
    if (v < 0) {
        if (p.mode != 0) return;                                    // mode 1: dst keeps what it held
        v = p.fill;
    }
    if (p.dst_bytes == 1) static_cast<unsigned char*>(p.dst)[i] = (unsigned char)v;
    else if (p.dst_bytes == 4) static_cast<int*>(p.dst)[i] = v;
    else static_cast<long long*>(p.dst)[i] = (long long)v;
}

// ---- host side: every argument checked and the kernels' parameters derived, in plain host code without a HIP call ----------------------
static bool zonal_aligned(const void* ptr, uintptr_t a) { return reinterpret_cast<uintptr_t>(ptr) % a == 0; }

// the zone raster's part of every entry; `blocks`: the entry runs one workgroup per block of a map
static int zonal_zone_params(const char* who, int zone_bytes, int zone_stride, int M, int H, int W, int Z, bool blocks, ZonalP& z) {
    if (zone_bytes != 4 && zone_bytes != 8) { set_error("%s: the element width of zone must be 4 or 8 bytes, got %d", who, zone_bytes); return S2K_EINVAL; }
    if (Z < 1) { set_error("%s: Z = %d must be positive", who, Z); return S2K_EINVAL; }
    if (M < 1 || H < 1 || W < 1) { set_error("%s: bad dims (M, H and W must be positive)", who); return S2K_EINVAL; }
    if (zone_stride < 0) { set_error("%s: zone_stride = %d must not be negative", who, zone_stride); return S2K_EINVAL; }
    if (zone_stride > 0 && (int64_t)M * zone_stride != Z) {
        set_error("%s: zone_stride = %d with M = %d maps needs Z = M * zone_stride rows, got Z = %d", who, zone_stride, M, Z);
        return S2K_EINVAL;
    }
    if ((int64_t)H * W > 0x7fffffffll) { set_error("%s: bad dims (H * W must stay below 2^31: offsets inside a map are 32-bit)", who); return S2K_EINVAL; }
    const int NBY = cdiv(H, ZONAL_BLOCK_H), NBX = cdiv(W, ZONAL_BLOCK_W);
    const int64_t grid = blocks ? (int64_t)M * NBY * NBX : cdiv64((int64_t)M * H * W, NTHREADS);
    if (grid > ZONAL_MAX_GRID) {
        if (blocks) set_error("%s: bad dims (M * ceil(H / %d) * ceil(W / %d) must stay below 2^31 workgroups)", who, ZONAL_BLOCK_H, ZONAL_BLOCK_W);
        else set_error("%s: bad dims (ceil(M * H * W / %d) must stay below 2^31 workgroups)", who, NTHREADS);
        return S2K_EINVAL;
    }
    z.zone_bytes = zone_bytes; z.zone_stride = zone_stride; z.zone_limit = zone_stride > 0 ? zone_stride : Z;
    z.M = M; z.H = H; z.W = W; z.Z = Z; z.NBY = NBY; z.NBX = NBX;
    return S2K_OK;
}

static int zonal_histogram_params(const void* zone, int zone_bytes, int zone_stride, const void* cls, int cls_bytes, const int* src_lut, int M,
                                  int H, int W, int Z, int K, long long* hist, unsigned* status, ZonalHistP& p) {
    const char* who = "zonal: histogram";
    if (!zone || !cls || !hist || !status) { set_error("%s: null pointer (zone, cls, hist and status are required)", who); return S2K_EFAULT; }
    if (cls_bytes != 1 && cls_bytes != 8) { set_error("%s: the element width of cls must be 1 or 8 bytes, got %d", who, cls_bytes); return S2K_EINVAL; }
    if (src_lut && cls_bytes != 1) { set_error("%s: src_lut needs a 1-byte cls", who); return S2K_EINVAL; }
    if (K < 1 || K > ZONAL_MAX_K) { set_error("%s: K = %d must lie in 1..%d", who, K, ZONAL_MAX_K); return S2K_EINVAL; }
    p = ZonalHistP{};
    const int rc = zonal_zone_params(who, zone_bytes, zone_stride, M, H, W, Z, true, p.z);
    if (rc != S2K_OK) return rc;
    p.z.zone = zone; p.z.status = status;
    p.z.vec = W % 4 == 0 && zonal_aligned(zone, 16) && zonal_aligned(cls, cls_bytes == 1 ? 4 : 16);
    p.cls = cls; p.src_lut = src_lut; p.hist = reinterpret_cast<unsigned long long*>(hist); p.cls_bytes = cls_bytes; p.K = K;
    return S2K_OK;
}

int check_zonal_histogram(const void* zone, int zone_bytes, int zone_stride, const void* cls, int cls_bytes, const int* src_lut, int M, int H,
                          int W, int Z, int K, long long* hist, unsigned* status) {
    ZonalHistP p;
    return zonal_histogram_params(zone, zone_bytes, zone_stride, cls, cls_bytes, src_lut, M, H, W, Z, K, hist, status, p);
}

int launch_zonal_histogram(const void* zone, int zone_bytes, int zone_stride, const void* cls, int cls_bytes, const int* src_lut, int M, int H,
                           int W, int Z, int K, long long* hist, unsigned* status, hipStream_t st) {
    ZonalHistP p;
    const int rc = zonal_histogram_params(zone, zone_bytes, zone_stride, cls, cls_bytes, src_lut, M, H, W, Z, K, hist, status, p);
    if (rc != S2K_OK) return rc;
    hipLaunchKernelGGL(zonal_hist_kernel, dim3((unsigned)((int64_t)M * p.z.NBY * p.z.NBX)), dim3(NTHREADS), 0, st, p);
    return S2K_OK;
}

static int zonal_bands_params(const void* zone, int zone_bytes, int zone_stride, const short* vals, int M, int C, int H, int W, int Z,
                              int nodata, int has_nodata, long long* count, long long* sum, long long* sumsq, int* mn, int* mx,
                              unsigned* status, ZonalBandP& p) {
    const char* who = "zonal: bands";
    if (!zone || !vals || !count || !sum || !sumsq || !mn || !mx || !status) {
        set_error("%s: null pointer (zone, vals, count, sum, sumsq, min, max and status are required)", who);
        return S2K_EFAULT;
    }
    if (C < 1 || C > ZONAL_MAX_C) { set_error("%s: C = %d must lie in 1..%d", who, C, ZONAL_MAX_C); return S2K_EINVAL; }
    if (has_nodata != 0 && has_nodata != 1) { set_error("%s: has_nodata = %d (0 or 1)", who, has_nodata); return S2K_EINVAL; }
    p = ZonalBandP{};
    const int rc = zonal_zone_params(who, zone_bytes, zone_stride, M, H, W, Z, true, p.z);
    if (rc != S2K_OK) return rc;
    p.z.zone = zone; p.z.status = status;
    p.z.vec = W % 4 == 0 && zonal_aligned(zone, 16) && zonal_aligned(vals, 8);
    p.vals = vals; p.count = reinterpret_cast<unsigned long long*>(count); p.sum = reinterpret_cast<unsigned long long*>(sum);
    p.sumsq = reinterpret_cast<unsigned long long*>(sumsq); p.mn = mn; p.mx = mx; p.C = C; p.nodata = nodata; p.has_nodata = has_nodata;
    return S2K_OK;
}

int check_zonal_bands(const void* zone, int zone_bytes, int zone_stride, const short* vals, int M, int C, int H, int W, int Z, int nodata,
                      int has_nodata, long long* count, long long* sum, long long* sumsq, int* mn, int* mx, unsigned* status) {
    ZonalBandP p;
    return zonal_bands_params(zone, zone_bytes, zone_stride, vals, M, C, H, W, Z, nodata, has_nodata, count, sum, sumsq, mn, mx, status, p);
}

int launch_zonal_bands(const void* zone, int zone_bytes, int zone_stride, const short* vals, int M, int C, int H, int W, int Z, int nodata,
                       int has_nodata, long long* count, long long* sum, long long* sumsq, int* mn, int* mx, unsigned* status, hipStream_t st) {
    ZonalBandP p;
    const int rc = zonal_bands_params(zone, zone_bytes, zone_stride, vals, M, C, H, W, Z, nodata, has_nodata, count, sum, sumsq, mn, mx, status, p);
    if (rc != S2K_OK) return rc;
    hipLaunchKernelGGL(zonal_band_kernel, dim3((unsigned)((int64_t)M * p.z.NBY * p.z.NBX)), dim3(NTHREADS), 0, st, p);
    return S2K_OK;
}

int check_zonal_majority(const long long* hist, int Z, int K, unsigned votes, long long min_count, int fill, int* out_cls, long long* out_best) {
    const char* who = "zonal: majority";
    (void)fill; (void)out_best;
    if (!hist || !out_cls) { set_error("%s: null pointer (hist and out_cls are required)", who); return S2K_EFAULT; }
    if (K < 1 || K > ZONAL_MAX_K) { set_error("%s: K = %d must lie in 1..%d", who, K, ZONAL_MAX_K); return S2K_EINVAL; }
    if (Z < 1) { set_error("%s: Z = %d must be positive", who, Z); return S2K_EINVAL; }
    if (votes == 0u || (K < 32 && (votes >> K) != 0u)) { set_error("%s: votes = %#x must name at least one class, all below K = %d", who, votes, K); return S2K_EINVAL; }
    if (min_count < 1) { set_error("%s: min_count = %lld must be at least 1", who, min_count); return S2K_EINVAL; }
    return S2K_OK;
}

int launch_zonal_majority(const long long* hist, int Z, int K, unsigned votes, long long min_count, int fill, int* out_cls, long long* out_best,
                          hipStream_t st) {
    const int rc = check_zonal_majority(hist, Z, K, votes, min_count, fill, out_cls, out_best);
    if (rc != S2K_OK) return rc;
    hipLaunchKernelGGL(zonal_majority_kernel, dim3((unsigned)cdiv(Z, NTHREADS)), dim3(NTHREADS), 0, st, hist, Z, K, votes, min_count, fill, out_cls,
                       out_best);
    return S2K_OK;
}

static int zonal_paint_params(const void* zone, int zone_bytes, int zone_stride, const int* table, int M, int H, int W, int Z, void* dst,
                              int dst_bytes, int mode, int fill, unsigned* status, ZonalPaintP& p) {
    const char* who = "zonal: paint";
    if (!zone || !table || !dst || !status) { set_error("%s: null pointer (zone, table, dst and status are required)", who); return S2K_EFAULT; }
    if (dst_bytes != 1 && dst_bytes != 4 && dst_bytes != 8) { set_error("%s: the element width of dst must be 1, 4 or 8 bytes, got %d", who, dst_bytes); return S2K_EINVAL; }
    if (mode != 0 && mode != 1) { set_error("%s: mode = %d (0 fill, 1 keep)", who, mode); return S2K_EINVAL; }
    if (dst_bytes == 1 && (fill < 0 || fill > 255)) { set_error("%s: fill = %d does not fit a 1-byte dst", who, fill); return S2K_EINVAL; }
    p = ZonalPaintP{};
    const int rc = zonal_zone_params(who, zone_bytes, zone_stride, M, H, W, Z, false, p.z);
    if (rc != S2K_OK) return rc;
    p.z.zone = zone; p.z.status = status;
    p.table = table; p.dst = dst; p.dst_bytes = dst_bytes; p.mode = mode; p.fill = fill;
    return S2K_OK;
}

int check_zonal_paint(const void* zone, int zone_bytes, int zone_stride, const int* table, int M, int H, int W, int Z, void* dst, int dst_bytes,
                      int mode, int fill, unsigned* status) {
    ZonalPaintP p;
    return zonal_paint_params(zone, zone_bytes, zone_stride, table, M, H, W, Z, dst, dst_bytes, mode, fill, status, p);
}

int launch_zonal_paint(const void* zone, int zone_bytes, int zone_stride, const int* table, int M, int H, int W, int Z, void* dst, int dst_bytes,
                       int mode, int fill, unsigned* status, hipStream_t st) {
    ZonalPaintP p;
    const int rc = zonal_paint_params(zone, zone_bytes, zone_stride, table, M, H, W, Z, dst, dst_bytes, mode, fill, status, p);
    if (rc != S2K_OK) return rc;
    hipLaunchKernelGGL(zonal_paint_kernel, dim3((unsigned)cdiv64((int64_t)M * H * W, NTHREADS)), dim3(NTHREADS), 0, st, p);
    return S2K_OK;
}

}  // namespace s2k
