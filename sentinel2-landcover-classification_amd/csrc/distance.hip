// Exact Euclidean distance transform of class maps, with the nearest site and distance-binned confusion counts (classmap.py; C entry
// s2k_classmap_distance, include/s2k.h).  How far a pixel is from the nearest class boundary, or from the nearest pixel of a set of
// classes: the quantity behind an ignore band measured in pixels rather than in windows, behind "do the errors sit at the boundaries",
// and behind filling no-data from the nearest labelled pixel.  The reference has no such operation; the definition in include/s2k.h
// is the oracle (tests/distance_ref.py restates it in numpy).  Integer work with one exact answer.
//
// The transform is separable, two plain launches whatever the map looks like, no grid-wide barrier:
//   COLUMN   one thread per column of a map (lanes run along x, so every row of the map is read coalesced) sweeps down and writes, per
//            pixel, the offset to the nearest site ABOVE it in its column (0 at a site, EDT_NONE where there is none), then sweeps
//            up over what it wrote (a site is a 0) and replaces the offset where a site BELOW is strictly nearer: above wins ties.
//            The site predicate is evaluated on the fly: in mode 1 a thread carries the 3 x 3 classes around its pixel in registers and
//            loads three per row, EDT_BATCH rows' loads in flight at a time.  Offsets are 16 bits (H <= 16384) in the caller's workspace.  No bands: a thread walks its whole
//            column, so one 512 x 512 map is 512 threads - the transform is meant for batches of maps.
//   ROW      one workgroup walks up to EDT_ROWS consecutive rows of a map, one at a time: the row's offsets are staged in LDS, and every
//            pixel searches outwards, k = 1, 2, ..., over the columns x - k and x + k for the smallest (k^2 + dy^2, site index),
//            until k * k > best (strict, so that every tie is seen and `nearest` is canonical) or both columns left the map.  A row
//            whose map columns hold no site is seen while staging (one __syncthreads_or) and written as NO_SITE without a search.
//            The same launch writes dist2 and nearest and counts the distance-binned confusion histogram: 16-bit LDS bins, two to a
//            dword, in `copies` keyed by the lane (a workgroup sees at most 65535 pixels: EDT_ROWS is cut down for wide maps), then one
//            64-bit atomic per non-zero bin.  Without `hist` the kernel does no counting work.
// A globally nearest site is always its column's choice (anything nearer in the column would be nearer overall; of two at the same
// vertical distance the upper has the smaller index), so comparing (dist2, index) over the columns' choices gives the smallest index
// among the nearest sites.
// Every loop is bounded by construction and carries that bound as its trip limit - the sweeps by H, the search by W, the rows of a
// workgroup by EDT_ROWS; there is no data-dependent `while`, and therefore no status word.  The worst case of the pruned search is one
// site in a corner: about W steps per pixel (tools/bench_distance.py times it).
// Map offsets are 64-bit, offsets inside a map 32-bit.
#include "plain.h"

namespace s2k {

constexpr int EDT_COLS = 64;                                // classmap.EDT_COLS: columns (threads) of a COLUMN workgroup, one wave
constexpr int EDT_ROWS = 8;                                 // classmap.EDT_ROWS: rows a ROW workgroup walks (fewer where EDT_ROWS * W > 65535)
constexpr int EDT_BATCH = 8;                                // rows of a column sweep whose loads are in flight together
constexpr int EDT_MAXK = 32, EDT_MAX_EDGES = 8, EDT_MAX_DIM = 16384;
constexpr int EDT_NONE = -32768;                            // "no site in this column" in the 16-bit offsets
constexpr int EDT_NO_SITE = 0x7fffffff;
constexpr int EDT_WG_PIXELS = 65535;                        // what a 16-bit bin can count
constexpr int64_t EDT_MAX_GRID = (1ll << 24) - 1;           // workgroups of at most 256 threads: fewer than 2^32 threads in the grid

struct DistanceP {
    const void* src;                // [M][H][W] uint8 or int64
    const int* src_lut;             // [256] or null
    const void* other;              // [M][H][W] uint8 or int64, or null
    short* work;                    // [M][H][W] column offsets
    int* dist2;                     // [M][H][W]
    int* nearest;                   // [M][H][W] or null
    unsigned long long* hist;       // [n_edges + 1][K][K] or null
    int M, H, W, K, src8, other8, mode, conn8;
    unsigned sites, exclude;
    int CB;                         // COLUMN: workgroups per map
    int R, RB;                      // ROW: rows per workgroup, workgroups per map
    int n_edges, nbins, bin_words, copies;      // bins of the histogram, dwords of one copy, copies
    int edges[EDT_MAX_EDGES];
};

__device__ __forceinline__ long long edt_load(const void* src, int src8, const int* src_lut, int off) {
    if (src8) return static_cast<const long long*>(src)[off];
    const int raw = static_cast<const unsigned char*>(src)[off];
    return src_lut ? (long long)src_lut[raw] : (long long)raw;
}

__device__ __forceinline__ const void* edt_map(const void* src, int src8, int64_t mapoff) {
    return src8 ? static_cast<const void*>(static_cast<const long long*>(src) + mapoff)
                : static_cast<const void*>(static_cast<const unsigned char*>(src) + mapoff);
}

// the class of the labelled pixel (y, x), -1 for an unlabelled one or one outside the map
__device__ __forceinline__ int edt_class(const DistanceP& p, const void* src, int y, int x) {
    if ((unsigned)y >= (unsigned)p.H || (unsigned)x >= (unsigned)p.W) return -1;
    const long long c = edt_load(src, p.src8, p.src_lut, y * p.W + x);
    return ((unsigned long long)c < (unsigned long long)p.K && !((p.exclude >> (int)(c & 31)) & 1u)) ? (int)c : -1;
}

__device__ __forceinline__ bool edt_differs(int c, int n) { return n >= 0 && n != c; }

// ---- COLUMN: grid M * CB, thread = one column of one map ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(EDT_COLS) edt_column_kernel(const DistanceP p) {
    const int H = p.H, W = p.W;
    const unsigned bid = blockIdx.x;
    const int m = (int)(bid / (unsigned)p.CB);
    const int x = (int)(bid % (unsigned)p.CB) * EDT_COLS + (int)threadIdx.x;
    if (x >= W) return;
    const int64_t mapoff = (int64_t)m * H * W;
    const void* __restrict__ src = edt_map(p.src, p.src8, mapoff);
    short* __restrict__ work = p.work + mapoff;
    // down: the nearest site above.  a / b / c are the classes of rows y - 1 / y / y + 1 at columns x - 1, x, x + 1 (mode 1).  Rows are
    // taken EDT_BATCH at a time, the loads of a batch issued before its first use: the sweep is a chain of H dependent steps per
    // thread, and with one row in flight it waits out a memory latency per row.
    int a0 = -1, a1 = -1, a2 = -1, b0 = -1, b1, b2 = -1;
    b1 = edt_class(p, src, 0, x);
    if (p.mode) { b0 = edt_class(p, src, 0, x - 1); b2 = edt_class(p, src, 0, x + 1); }
    int last = -1;
    for (int yb = 0; yb < H; yb += EDT_BATCH) {                 // ceil(H / EDT_BATCH) steps
        int n0[EDT_BATCH], n1[EDT_BATCH], n2[EDT_BATCH];
#pragma unroll
        for (int j = 0; j < EDT_BATCH; ++j) {                   // rows at or past H read as unlabelled
            n1[j] = edt_class(p, src, yb + j + 1, x);
            n0[j] = p.mode ? edt_class(p, src, yb + j + 1, x - 1) : -1;
            n2[j] = p.mode ? edt_class(p, src, yb + j + 1, x + 1) : -1;
        }
#pragma unroll
        for (int j = 0; j < EDT_BATCH; ++j) {
            const int y = yb + j;
            if (y < H) {
                const int c0 = n0[j], c1 = n1[j], c2 = n2[j];
                bool site;
                if (p.mode) {
                    site = b1 >= 0 && (edt_differs(b1, a1) || edt_differs(b1, c1) || edt_differs(b1, b0) || edt_differs(b1, b2) ||
                                       (p.conn8 && (edt_differs(b1, a0) || edt_differs(b1, a2) || edt_differs(b1, c0) || edt_differs(b1, c2))));
                } else {
                    site = b1 >= 0 && ((p.sites >> b1) & 1u);
                }
                if (site) last = y;
                work[y * W + x] = (short)(last >= 0 ? last - y : EDT_NONE);
                a0 = b0; a1 = b1; a2 = b2; b0 = c0; b1 = c1; b2 = c2;
            }
        }
    }
    // up: a site below replaces the offset only where it is strictly nearer
    int next = -1;
    for (int yt = H - 1; yt >= 0; yt -= EDT_BATCH) {            // ceil(H / EDT_BATCH) steps
        int v[EDT_BATCH];
#pragma unroll
        for (int j = 0; j < EDT_BATCH; ++j) v[j] = yt - j >= 0 ? (int)work[(yt - j) * W + x] : EDT_NONE;
#pragma unroll
        for (int j = 0; j < EDT_BATCH; ++j) {
            const int y = yt - j;
            if (y >= 0) {
                if (v[j] == 0) next = y;
                else if (next >= 0 && (v[j] == EDT_NONE || next - y < -v[j])) work[y * W + x] = (short)(next - y);
            }
        }
    }
}

// ---- ROW: grid M * RB; workgroup (m, row block) walks R rows -----------------------------------------------------------------------------
__global__ void __launch_bounds__(NTHREADS) edt_row_kernel(const DistanceP p) {
    extern __shared__ unsigned int edt_lds[];                   // bins: copies * bin_words dwords; then the staged row: W offsets
    unsigned int* bins = edt_lds;
    short* row = reinterpret_cast<short*>(edt_lds + p.copies * p.bin_words);
    const int H = p.H, W = p.W, K = p.K, lane = threadIdx.x & (WAVE - 1);
    const unsigned bid = blockIdx.x;
    const int m = (int)(bid / (unsigned)p.RB), y0 = (int)(bid % (unsigned)p.RB) * p.R;
    const int64_t mapoff = (int64_t)m * H * W;
    const short* work = p.work + mapoff;
    const void* src = nullptr;
    const void* other = nullptr;
    if (p.hist) {
        src = edt_map(p.src, p.src8, mapoff);
        other = edt_map(p.other, p.other8, mapoff);
        for (int i = threadIdx.x; i < p.copies * p.bin_words; i += NTHREADS) bins[i] = 0u;      // the staging barrier below orders it
    }
    for (int r = 0; r < p.R; ++r) {                             // at most EDT_ROWS rows
        const int y = y0 + r;
        if (y >= H) break;                                      // the whole workgroup leaves together
        const int rowoff = y * W;
        int any = 0;
        for (int x = threadIdx.x; x < W; x += NTHREADS) {
            const short d = work[rowoff + x];
            row[x] = d;
            any |= d != EDT_NONE;
        }
        any = __syncthreads_or(any);
        for (int x = threadIdx.x; x < W; x += NTHREADS) {
            int best = EDT_NO_SITE, bi = -1;
            if (any) {
                const int d0 = row[x];
                if (d0 != EDT_NONE) { best = d0 * d0; bi = rowoff + d0 * W + x; }
                for (int k = 1; k < W; ++k) {                   // fewer than W steps
                    const int kk = k * k;                       // k < 2^14
                    if (kk > best) break;
                    const int xl = x - k, xr = x + k;
                    if (xl < 0 && xr >= W) break;
                    if (xl >= 0) {
                        const int d = row[xl];
                        if (d != EDT_NONE) {
                            const int c = kk + d * d, idx = rowoff + d * W + xl;
                            if (c < best || (c == best && idx < bi)) { best = c; bi = idx; }
                        }
                    }
                    if (xr < W) {
                        const int d = row[xr];
                        if (d != EDT_NONE) {
                            const int c = kk + d * d, idx = rowoff + d * W + xr;
                            if (c < best || (c == best && idx < bi)) { best = c; bi = idx; }
                        }
                    }
                }
            }
            p.dist2[mapoff + rowoff + x] = best;
            if (p.nearest) p.nearest[mapoff + rowoff + x] = bi;
            if (p.hist) {
                const long long t = edt_load(src, p.src8, p.src_lut, rowoff + x);
                const long long o = edt_load(other, p.other8, nullptr, rowoff + x);
                if ((unsigned long long)t < (unsigned long long)K && (unsigned long long)o < (unsigned long long)K) {
                    int b = 0;
#pragma unroll
                    for (int j = 0; j < EDT_MAX_EDGES; ++j) b += (j < p.n_edges && best > p.edges[j]) ? 1 : 0;
                    const int bin = (b * K + (int)t) * K + (int)o;
                    atomicAdd(&bins[(lane & (p.copies - 1)) * p.bin_words + (bin >> 1)], 1u << ((bin & 1) * 16));
                }
            }
        }
        __syncthreads();                                        // the row is staged anew; after the last row: the bins are complete
    }
    if (p.hist) {
        for (int i = threadIdx.x; i < p.nbins; i += NTHREADS) {
            unsigned n = 0u;
            for (int c = 0; c < p.copies; ++c) n += (bins[c * p.bin_words + (i >> 1)] >> ((i & 1) * 16)) & 0xffffu;
            if (n) atomicAdd(p.hist + i, (unsigned long long)n);
        }
    }
}

// ---- host side: every argument checked and the kernels' parameters derived, in plain host code without a HIP call ----------------------
static int distance_params(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int mode, unsigned sites,
                           int connectivity, unsigned exclude, void* work, int* dist2, int* nearest, const void* other, int other_bytes,
                           const int* edges, int n_edges, unsigned long long* hist, DistanceP& p) {
    const char* who = "classmap_distance";
    if (!src || !dist2 || !work) { set_error("%s: null pointer (src, dist2 and work are required)", who); return S2K_EFAULT; }
    if (src_bytes != 1 && src_bytes != 8) { set_error("%s: the element width of src must be 1 (uint8) or 8 (int64) bytes, got %d", who, src_bytes); return S2K_EINVAL; }
    if (src_lut && src_bytes != 1) { set_error("%s: src_lut reads a 1-byte src only", who); return S2K_EINVAL; }
    if (K < 1 || K > EDT_MAXK) { set_error("%s: K = %d outside 1..%d", who, K, EDT_MAXK); return S2K_EINVAL; }
    if (mode != 0 && mode != 1) { set_error("%s: mode = %d (0 classes, 1 boundary)", who, mode); return S2K_EINVAL; }
    if (connectivity != 4 && connectivity != 8) { set_error("%s: connectivity = %d (4 or 8)", who, connectivity); return S2K_EINVAL; }
    const unsigned all = K == 32 ? 0xffffffffu : (1u << K) - 1u;
    if (exclude & ~all) { set_error("%s: exclude names a class at or above K = %d", who, K); return S2K_EINVAL; }
    if (sites & ~all) { set_error("%s: sites names a class at or above K = %d", who, K); return S2K_EINVAL; }
    if (mode == 0 && sites == 0u) { set_error("%s: mode 0 needs at least one class in sites", who); return S2K_EINVAL; }
    if (mode == 0 && (sites & exclude)) { set_error("%s: sites and exclude overlap", who); return S2K_EINVAL; }
    if (mode == 1 && sites != 0u) { set_error("%s: sites must be 0 in mode 1 (the sites are the boundaries)", who); return S2K_EINVAL; }
    if (M < 1 || H < 1 || W < 1) { set_error("%s: bad dims (M, H and W must be positive)", who); return S2K_EINVAL; }
    if (H > EDT_MAX_DIM || W > EDT_MAX_DIM) { set_error("%s: bad dims (H and W must not exceed %d: offsets are 16-bit, dist2 31-bit)", who, EDT_MAX_DIM); return S2K_EINVAL; }
    if ((int64_t)H * W > 0x7fffffffll) { set_error("%s: bad dims (H * W must stay below 2^31: offsets inside a map are 32-bit)", who); return S2K_EINVAL; }
    if (hist) {
        if (!other || !edges) { set_error("%s: hist needs other and edges", who); return S2K_EINVAL; }
        if (other_bytes != 1 && other_bytes != 8) { set_error("%s: the element width of other must be 1 (uint8) or 8 (int64) bytes, got %d", who, other_bytes); return S2K_EINVAL; }
        if (n_edges < 1 || n_edges > EDT_MAX_EDGES) { set_error("%s: n_edges = %d outside 1..%d", who, n_edges, EDT_MAX_EDGES); return S2K_EINVAL; }
        for (int j = 0; j < n_edges; ++j) {
            if (edges[j] < 0 || (j > 0 && edges[j] <= edges[j - 1])) {
                set_error("%s: edges must be non-negative and ascend strictly (edges[%d] = %d)", who, j, edges[j]);
                return S2K_EINVAL;
            }
        }
    }
    p = DistanceP{};
    p.src = src; p.src_lut = src_lut; p.other = other; p.work = static_cast<short*>(work); p.dist2 = dist2; p.nearest = nearest; p.hist = hist;
    p.M = M; p.H = H; p.W = W; p.K = K; p.src8 = src_bytes == 8; p.other8 = other_bytes == 8; p.mode = mode; p.conn8 = connectivity == 8;
    p.sites = sites; p.exclude = exclude;
    p.CB = cdiv(W, EDT_COLS);
    p.R = EDT_WG_PIXELS / W < EDT_ROWS ? EDT_WG_PIXELS / W : EDT_ROWS;        // >= 3: W <= 16384
    p.RB = cdiv(H, p.R);
    if ((int64_t)M * p.CB > EDT_MAX_GRID || (int64_t)M * p.RB > EDT_MAX_GRID) {
        set_error("%s: bad dims (M * ceil(W / %d) and M * ceil(H / rows per workgroup) must stay below 2^24 workgroups)", who, EDT_COLS);
        return S2K_EINVAL;
    }
    p.copies = 1;
    if (hist) {
        p.n_edges = n_edges;
        for (int j = 0; j < n_edges; ++j) p.edges[j] = edges[j];
        p.nbins = (n_edges + 1) * K * K;
        p.bin_words = (p.nbins + 1) / 2;
        while (p.copies < 16 && 2 * p.copies * p.bin_words * 4 <= 16384) p.copies *= 2;
    }
    return S2K_OK;
}

int check_classmap_distance(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int mode, unsigned sites,
                            int connectivity, unsigned exclude, void* work, int* dist2, int* nearest, const void* other, int other_bytes,
                            const int* edges, int n_edges, unsigned long long* hist) {
    DistanceP p;
    return distance_params(src, src_bytes, src_lut, M, H, W, K, mode, sites, connectivity, exclude, work, dist2, nearest, other, other_bytes,
                           edges, n_edges, hist, p);
}

int launch_classmap_distance(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int mode, unsigned sites,
                             int connectivity, unsigned exclude, void* work, int* dist2, int* nearest, const void* other, int other_bytes,
                             const int* edges, int n_edges, unsigned long long* hist, hipStream_t st) {
    DistanceP p;
    const int rc = distance_params(src, src_bytes, src_lut, M, H, W, K, mode, sites, connectivity, exclude, work, dist2, nearest, other,
                                   other_bytes, edges, n_edges, hist, p);
    if (rc != S2K_OK) return rc;
    // at most 18 KB of bins (9 * 32 * 32 of 16 bits, one copy) and 32 KB of row
    const size_t lds = (size_t)p.copies * p.bin_words * sizeof(unsigned int) + (((size_t)W + 1) & ~(size_t)1) * sizeof(short);
    hipLaunchKernelGGL(edt_column_kernel, dim3((unsigned)((int64_t)M * p.CB)), dim3(EDT_COLS), 0, st, p);
    hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)((int64_t)M * p.RB)), dim3(NTHREADS), lds, st, p);
    return S2K_OK;
}

size_t classmap_distance_workspace(int M, int H, int W) {
    if (M < 1 || H < 1 || W < 1) return 0;
    return (size_t)M * (size_t)H * (size_t)W * sizeof(short);
}

}  // namespace s2k
