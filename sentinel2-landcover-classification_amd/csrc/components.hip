// Connected-component labelling of class maps and the minimum-area sieve built on it (classmap.py; C entries s2k_classmap_components
// and s2k_classmap_sieve, include/s2k.h).  What a window filter cannot give: the REGIONS of a map - the minimum mapping unit of a
// land-cover product, slivers of rasterised polygons, patches per class.  The reference has no such operation; the definition in
// include/s2k.h is the oracle (tests/components_ref.py restates it in numpy).
//
// Labelling is union-find in three plain launches, no grid-wide barrier, no wait on a value another thread has yet to write:
//   LOCAL    one workgroup labels one CC_TILE_H x CC_TILE_W tile in LDS (256 threads, four pixels each; a wave holds a row): parents
//            start as the first pixel of the pixel's run of equal classes in its row (one ballot), the runs are united with those of
//            the row above (straight up, and the two upper diagonals at connectivity 8) wherever the runs do not imply the union
//            already, the tile is flattened and `labels` gets the GLOBAL index of the local root.  The local index is row-major like
//            the global one, so the local root (the smallest local index) is the component's smallest global index inside the tile.
//   MERGE    one thread per pixel on a tile's top or left edge unites it with its same-class neighbours across the edge, `labels`
//            being the parent array (connectivity 8: the three pixels across, which covers the pairs across tile corners).
//   FLATTEN  every pixel replaces its label by its root; roots are counted per class (LDS bins, one 64-bit atomic per non-zero bin) and
//            areas are added into areas[root] - PRE-AGGREGATED: a wave adds one number per run of equal roots among its 64 consecutive
//            pixels into a 256-slot LDS table keyed by root, and the workgroup sends one global atomic per occupied slot (a slot taken
//            by another root sends the run's atomic straight to memory).  A one-class map would otherwise send every pixel to a single
//            address (csrc/loss.hip on what same-address atomics cost).
// The parent array keeps parent[i] <= i: find walks strictly downward, union links the LARGER root under the smaller one with atomicMin
// and retries with the value it found there, which is smaller.  The sum of a union's two operands therefore never rises and falls by at
// least one with every find step and every failed link: a union ends within 2 n steps, a find within n (n = parents in the array).
// Every loop carries exactly that budget; a thread that overruns it ORs a bit into `status`, and writes nothing further (it still
// reaches the barriers).  The root of a component is its smallest linear index whatever the order threads ran in: labels are canonical.
//
// The sieve is two more launches over flattened labels, neither with a loop that depends on data:
//   DONOR    (only without `to`) every pixel of a small component looks at its four edge neighbours; the best donor key among those of
//            other components goes into best[root] with one 64-bit atomicMax.  Key: bit 62 = area >= min_area, bits 31..61 = area,
//            bits 0..30 = 2^31 - 1 - root, so that the maximum is the donor the definition orders first.
//   RELABEL  every pixel of a small component writes `to` or the class of its donor's root in the INPUT map, everything else is
//            copied; CHANGED and HIST are counted as s2k_classmap_filter counts them (LDS bins in copies, one 64-bit atomic per bin).
// Map offsets are 64-bit, offsets inside a map 32-bit.
#include "plain.h"

namespace s2k {

constexpr int CC_TILE_H = 16, CC_TILE_W = 64;               // classmap.CC_TILE_H / CC_TILE_W
constexpr int CC_TILE = CC_TILE_H * CC_TILE_W;              // pixels of a tile = pixels a workgroup of the flat kernels walks
constexpr int CC_PER_THREAD = CC_TILE / NTHREADS;
constexpr int CC_MAXK = 32;
constexpr int CC_SLOTS = NTHREADS;                          // FLATTEN's LDS table of (root, pixels): one slot per thread to flush
constexpr int64_t CC_MAX_GRID = (1ll << 24) - 1;            // workgroups of 256 threads: fewer than 2^32 threads in the grid
constexpr unsigned CC_ST_LOCAL = 1u, CC_ST_MERGE = 2u, CC_ST_FLATTEN = 4u, CC_ST_LABELS = 8u;      // bits of `status`
constexpr unsigned long long CC_ROOT_MASK = 0x7fffffffull;

struct ComponentsP {
    const void* src;                // [M][H][W] uint8 or int64
    const int* src_lut;             // [256] or null
    int* labels;                    // [M][H][W]
    int* areas;                     // [M][H][W]
    unsigned long long* counts;     // [M][K] or null
    unsigned* status;
    int M, H, W, K, src8, conn8;
    unsigned exclude;
    int TX, TY;                     // tiles per row, tile rows
    int NR, NC, E, EB;              // MERGE: tile-top rows, tile-left columns, edge pixels per map, workgroups per map
    int FB;                         // FLATTEN: workgroups per map
};

struct SieveP {
    const void* src;
    void* dst;
    const int* src_lut;
    const int* labels;
    const int* areas;
    unsigned long long* best;       // [M][H][W] or null (with `to`)
    const unsigned char* hist_labels;
    const int* index;
    const int* lut;
    unsigned long long* hist;
    unsigned long long* changed;
    unsigned* status;
    int M, H, W, K, NSRC, src8, dst8, min_area, to;
    unsigned fixed;
    int FB, copies;                 // workgroups per map; copies of each HIST bin in LDS
};

// the value of pixel `off` of the map at `src` (a 64-bit value: an int64 map may hold anything)
__device__ __forceinline__ long long cc_load(const void* src, int src8, const int* src_lut, int off) {
    if (src8) return static_cast<const long long*>(src)[off];
    const int raw = static_cast<const unsigned char*>(src)[off];
    return src_lut ? (long long)src_lut[raw] : (long long)raw;
}

__device__ __forceinline__ const void* cc_map(const void* src, int src8, int64_t mapoff) {
    return src8 ? static_cast<const void*>(static_cast<const long long*>(src) + mapoff)
                : static_cast<const void*>(static_cast<const unsigned char*>(src) + mapoff);
}

// the class of a labelled pixel, -1 for an unlabelled one (outside [0, K), or excluded)
__device__ __forceinline__ int cc_class(const ComponentsP& p, const void* src, int off) {
    const long long c = cc_load(src, p.src8, p.src_lut, off);
    return ((unsigned long long)c < (unsigned long long)p.K && !((p.exclude >> (int)(c & 31)) & 1u)) ? (int)c : -1;
}

// ---- union-find over LDS parents --------------------------------------------------------------------------------------------------------
// the root of i, or -1 when `steps` ran out; every step goes strictly downward (parent[i] <= i)
__device__ __forceinline__ int cc_lds_find(const volatile int* parent, int i, int& steps) {
    int up = parent[i];
    while (up != i) {
        if (steps-- <= 0) return -1;
        i = up;
        up = parent[i];
    }
    return i;
}

// false when the budget of 2 n steps ran out (it cannot, see the head of the file)
__device__ __forceinline__ bool cc_lds_union(int* parent, int a, int b, int n) {
    int steps = 2 * n;
    for (;;) {
        a = cc_lds_find(parent, a, steps);
        b = cc_lds_find(parent, b, steps);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a < b) { const int t = a; a = b; b = t; }          // a is the larger root
        const int old = atomicMin(&parent[a], b);
        if (old == a) return true;                              // a was a root and now hangs under b
        if (steps-- <= 0) return false;
        a = old;                                                // somebody linked a first, to old < a: unite that with b
    }
}

// ---- union-find over the global labels (other workgroups link at the same time: every read is an atomic load) ---------------------------
__device__ __forceinline__ int cc_parent(const int* labels, int i) {
    return __hip_atomic_load(labels + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// n = H * W bounds every index; a value outside [0, n) (labels that no LOCAL pass wrote) ends the walk as an overrun does
__device__ __forceinline__ int cc_find(const int* labels, int i, unsigned n, unsigned& steps) {
    int up = cc_parent(labels, i);
    while (up != i) {
        if (steps == 0u || (unsigned)up >= n) return -1;
        --steps;
        i = up;
        up = cc_parent(labels, i);
    }
    return i;
}

__device__ __forceinline__ bool cc_union(int* labels, int a, int b, unsigned n) {
    unsigned steps = 2u * n;                                    // n < 2^31
    for (;;) {
        a = cc_find(labels, a, n, steps);
        b = cc_find(labels, b, n, steps);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&labels[a], b);
        if (old == a) return true;
        if (steps == 0u || (unsigned)old >= n) return false;
        --steps;
        a = old;
    }
}

// ---- LOCAL: grid M * TY * TX, workgroup ((m * TY + tile row) * TX + tile column) --------------------------------------------------------
__global__ void __launch_bounds__(NTHREADS) cc_local_kernel(const ComponentsP p) {
    __shared__ int cls[CC_TILE];
    __shared__ int parent[CC_TILE];
    const int H = p.H, W = p.W;
    const unsigned bid = blockIdx.x;
    const int tx = (int)(bid % (unsigned)p.TX);
    const unsigned mt = bid / (unsigned)p.TX;
    const int ty = (int)(mt % (unsigned)p.TY), m = (int)(mt / (unsigned)p.TY);
    const int64_t mapoff = (int64_t)m * H * W;
    const void* src = cc_map(p.src, p.src8, mapoff);
    const int y0 = ty * CC_TILE_H, x0 = tx * CC_TILE_W;
#pragma unroll
    for (int j = 0; j < CC_PER_THREAD; ++j) {
        const int li = j * NTHREADS + (int)threadIdx.x;
        const int y = y0 + li / CC_TILE_W, x = x0 + li % CC_TILE_W;
        cls[li] = (y < H && x < W) ? cc_class(p, src, y * W + x) : -1;
    }
    __syncthreads();
    // A wave holds one row of the tile (lane = column), so the runs of a row need no union at all: every pixel starts under the
    // first pixel of its run, found with one ballot.  (A one-class tile would otherwise queue 63 unions of a row on one LDS address.)
    static_assert(CC_TILE_W == WAVE && NTHREADS % WAVE == 0, "a wave is one row of the tile");
    const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int j = 0; j < CC_PER_THREAD; ++j) {
        const int li = j * NTHREADS + (int)threadIdx.x;
        const int c = cls[li];
        const bool head = lane == 0 || cls[li - 1] != c;
        const unsigned long long heads = __ballot(head);
        const unsigned long long upto = lane == WAVE - 1 ? heads : heads & ((1ull << (lane + 1)) - 1ull);      // bit 0 is always set
        parent[li] = c >= 0 ? li - lane + (WAVE - 1 - __clzll((long long)upto)) : li;
    }
    __syncthreads();
    // What is left are the unions between rows, and only those that the runs do not already imply: straight up unless the left
    // neighbour makes the same union one column over (it is in this pixel's run, the pixel above it in the upper pixel's run); a
    // diagonal only where neither the pixel above nor the pixel beside it joins the two runs anyway.
    bool dead = false;                                          // this thread overran a step bound: it writes nothing further
#pragma unroll
    for (int j = 0; j < CC_PER_THREAD; ++j) {
        const int li = j * NTHREADS + (int)threadIdx.x;
        const int ly = li / CC_TILE_W, lx = li % CC_TILE_W, c = cls[li];
        if (dead || c < 0 || ly == 0) continue;
        const bool l = lx > 0 && cls[li - 1] == c, r = lx < CC_TILE_W - 1 && cls[li + 1] == c;
        const bool u = cls[li - CC_TILE_W] == c;
        const bool ul = lx > 0 && cls[li - CC_TILE_W - 1] == c, ur = lx < CC_TILE_W - 1 && cls[li - CC_TILE_W + 1] == c;
        if (u && !(l && ul)) dead = !cc_lds_union(parent, li, li - CC_TILE_W, CC_TILE);
        if (p.conn8) {
            if (!dead && ul && !u && !l) dead = !cc_lds_union(parent, li, li - CC_TILE_W - 1, CC_TILE);
            if (!dead && ur && !u && !r) dead = !cc_lds_union(parent, li, li - CC_TILE_W + 1, CC_TILE);
        }
    }
    __syncthreads();                                            // from here on the parents are only read
    int* labels = p.labels + mapoff;
#pragma unroll
    for (int j = 0; j < CC_PER_THREAD; ++j) {
        const int li = j * NTHREADS + (int)threadIdx.x;
        const int y = y0 + li / CC_TILE_W, x = x0 + li % CC_TILE_W;
        if (dead || y >= H || x >= W) continue;
        int out = -1;
        if (cls[li] >= 0) {
            int steps = CC_TILE;
            const int root = cc_lds_find(parent, li, steps);
            if (root < 0) { dead = true; continue; }
            out = (y0 + root / CC_TILE_W) * W + x0 + root % CC_TILE_W;
        }
        labels[y * W + x] = out;
    }
    if (dead) atomicOr(p.status, CC_ST_LOCAL);
}

// ---- MERGE: grid M * EB; thread e of a map: one pixel of a tile-top row (e < NR * W) or of a tile-left column ---------------------------
__global__ void __launch_bounds__(NTHREADS) cc_merge_kernel(const ComponentsP p) {
    const int H = p.H, W = p.W;
    const unsigned bid = blockIdx.x;
    const int m = (int)(bid / (unsigned)p.EB);
    const int e = (int)(bid % (unsigned)p.EB) * NTHREADS + (int)threadIdx.x;
    if (e >= p.E) return;
    const int64_t mapoff = (int64_t)m * H * W;
    const void* src = cc_map(p.src, p.src8, mapoff);
    int* labels = p.labels + mapoff;
    const unsigned n = (unsigned)(H * W);
    const bool top = e < p.NR * W;
    int y, x;
    if (top) { y = (e / W + 1) * CC_TILE_H; x = e % W; }
    else { const int j = e - p.NR * W; x = (j / H + 1) * CC_TILE_W; y = j % H; }
    const int i = y * W + x, c = cc_class(p, src, i);
    if (c < 0) return;
    // The pixels across the edge: straight across, then (connectivity 8) the two beside it, where the map has them.  Most of these
    // unions are implied by others, and on a one-class map every one of them would walk to, and link at, the same few roots:
    //   straight  is left out where the previous pixel ALONG the edge makes the same union and lies in this pixel's tile (so the tile
    //             pass joined the two pixels on this side, and the two on the far side): the chain of such pixels ends, at the latest
    //             at the tile's corner, in one that makes its union unconditionally;
    //   diagonal  is left out where the pixel straight across has this class: it is joined to this pixel by the rule above and to
    //             the diagonal one as its neighbour in a row (top edge) or column (left edge), inside a tile or across an edge.
    const int back = top ? 1 : W;                               // one pixel back along the edge
    const int across = top ? W : 1;
    int nb[3] = {-1, -1, -1};
    if (cc_class(p, src, i - across) == c) {
        const bool inside = top ? x % CC_TILE_W != 0 : y % CC_TILE_H != 0;
        if (!(inside && cc_class(p, src, i - back) == c && cc_class(p, src, i - across - back) == c)) nb[0] = i - across;
    } else if (p.conn8) {
        const bool before = top ? x > 0 : y > 0, after = top ? x + 1 < W : y + 1 < H;
        if (before && cc_class(p, src, i - across - back) == c) nb[1] = i - across - back;
        if (after && cc_class(p, src, i - across + back) == c) nb[2] = i - across + back;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (nb[k] < 0) continue;
        if (!cc_union(labels, i, nb[k], n)) { atomicOr(p.status, CC_ST_MERGE); return; }
    }
}

// ---- FLATTEN: grid M * FB; a workgroup walks CC_TILE consecutive pixels of a map, a wave 64 consecutive ones at a time ------------------
__global__ void __launch_bounds__(NTHREADS) cc_flatten_kernel(const ComponentsP p) {
    __shared__ int keys[CC_SLOTS];
    __shared__ unsigned int cnt[CC_SLOTS];
    __shared__ unsigned int bins[CC_MAXK];
    const int HW = p.H * p.W, lane = threadIdx.x & (WAVE - 1);
    const unsigned bid = blockIdx.x;
    const int m = (int)(bid / (unsigned)p.FB), base = (int)(bid % (unsigned)p.FB) * CC_TILE;
    const int64_t mapoff = (int64_t)m * HW;
    const void* src = cc_map(p.src, p.src8, mapoff);
    int* labels = p.labels + mapoff;
    int* areas = p.areas + mapoff;
    keys[threadIdx.x] = -1;
    cnt[threadIdx.x] = 0u;
    if (threadIdx.x < CC_MAXK) bins[threadIdx.x] = 0u;
    __syncthreads();
    bool dead = false;
#pragma unroll
    for (int j = 0; j < CC_PER_THREAD; ++j) {
        const unsigned u = (unsigned)base + (unsigned)(j * NTHREADS) + threadIdx.x;      // may pass 2^31 in the last workgroup: unsigned
        const bool in = u < (unsigned)HW;
        const int i = (int)u;
        int root = -1;
        if (in && !dead) {
            const int l = labels[i];
            if (l >= 0) {
                unsigned steps = (unsigned)HW;
                root = (unsigned)l < (unsigned)HW ? cc_find(labels, l, (unsigned)HW, steps) : -1;
                if (root < 0) dead = true;
                else if (root != l) labels[i] = root;              // a root of the same component: walks that pass here stay valid
            }
        }
        // one add per run of equal roots among the wave's 64 consecutive pixels
        const int prev = __shfl_up(root, 1);
        const bool head = lane == 0 || prev != root;
        const unsigned long long heads = __ballot(head);
        if (head && root >= 0) {
            const unsigned long long later = lane == WAVE - 1 ? 0ull : heads >> (lane + 1);
            const unsigned run = later ? (unsigned)__ffsll((long long)later) : (unsigned)(WAVE - lane);
            const int slot = (int)(((unsigned)root * 2654435761u) >> 24);
            const int old = atomicCAS(&keys[slot], -1, root);
            if (old == -1 || old == root) atomicAdd(&cnt[slot], run);
            else atomicAdd(&areas[root], (int)run);
        }
        if (in && root == i && p.counts) {
            const int c = cc_class(p, src, i);
            if (c >= 0) atomicAdd(&bins[c], 1u);
        }
    }
    if (dead) atomicOr(p.status, CC_ST_FLATTEN);
    __syncthreads();
    if (keys[threadIdx.x] >= 0 && cnt[threadIdx.x]) atomicAdd(&areas[keys[threadIdx.x]], (int)cnt[threadIdx.x]);
    if (p.counts && (int)threadIdx.x < p.K && bins[threadIdx.x])
        atomicAdd(p.counts + (int64_t)m * p.K + threadIdx.x, (unsigned long long)bins[threadIdx.x]);
}

// ---- DONOR: grid M * FB -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long cc_donor_key(const SieveP& p, const int* labels, const int* areas, int own, int nb, unsigned HW) {
    const int l = labels[nb];
    if (l < 0 || l == own || (unsigned)l >= HW) return 0ull;
    const int a = areas[l];
    return ((unsigned long long)(a >= p.min_area) << 62) | ((unsigned long long)(unsigned)a << 31) | (CC_ROOT_MASK - (unsigned long long)l);
}

__global__ void __launch_bounds__(NTHREADS) cc_donor_kernel(const SieveP p) {
    const int H = p.H, W = p.W;
    const unsigned HW = (unsigned)(H * W);
    const unsigned bid = blockIdx.x;
    const int m = (int)(bid / (unsigned)p.FB);
    const unsigned base = (bid % (unsigned)p.FB) * CC_TILE;
    const int64_t mapoff = (int64_t)m * H * W;
    const void* src = cc_map(p.src, p.src8, mapoff);
    const int* labels = p.labels + mapoff;
    const int* areas = p.areas + mapoff;
#pragma unroll
    for (int j = 0; j < CC_PER_THREAD; ++j) {
        const unsigned u = base + (unsigned)(j * NTHREADS) + threadIdx.x;
        if (u >= HW) continue;
        const int i = (int)u, l = labels[i];
        if (l < 0) continue;
        if ((unsigned)l >= HW) { atomicOr(p.status, CC_ST_LABELS); continue; }
        if (areas[l] >= p.min_area) continue;
        const long long c = cc_load(src, p.src8, p.src_lut, i);
        if ((unsigned long long)c >= (unsigned long long)p.K || ((p.fixed >> (int)(c & 31)) & 1u)) continue;
        const int y = i / W, x = i - y * W;
        unsigned long long key = 0ull;
        if (x > 0) key = max(key, cc_donor_key(p, labels, areas, l, i - 1, HW));
        if (x + 1 < W) key = max(key, cc_donor_key(p, labels, areas, l, i + 1, HW));
        if (y > 0) key = max(key, cc_donor_key(p, labels, areas, l, i - W, HW));
        if (y + 1 < H) key = max(key, cc_donor_key(p, labels, areas, l, i + W, HW));
        if (key) atomicMax(p.best + mapoff + l, key);
    }
}

// ---- RELABEL: grid M * FB ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NTHREADS) cc_relabel_kernel(const SieveP p) {
    __shared__ unsigned int bins[1024];                         // K * K bins, `copies` of each side by side (classmap_filter_kernel)
    __shared__ unsigned int wchanged[NTHREADS / WAVE];
    const int H = p.H, W = p.W, K = p.K, COPIES = p.copies, lane = threadIdx.x & (WAVE - 1);
    const unsigned HW = (unsigned)(H * W);
    const unsigned bid = blockIdx.x;
    const int m = (int)(bid / (unsigned)p.FB);
    const unsigned base = (bid % (unsigned)p.FB) * CC_TILE;
    const int64_t mapoff = (int64_t)m * H * W;
    const void* src = cc_map(p.src, p.src8, mapoff);
    const int* labels = p.labels + mapoff;
    const int* areas = p.areas + mapoff;
    const unsigned char* lab = nullptr;
    if (p.hist) {
        for (int i = threadIdx.x; i < K * K * COPIES; i += NTHREADS) bins[i] = 0u;
        const int s = p.index[m];
        if ((unsigned)s < (unsigned)p.NSRC) lab = p.hist_labels + (int64_t)s * H * W;
        __syncthreads();
    }
    unsigned nchanged = 0u;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < CC_PER_THREAD; ++j) {
        const unsigned u = base + (unsigned)(j * NTHREADS) + threadIdx.x;
        if (u >= HW) continue;
        const int i = (int)u, l = labels[i];
        if (l >= 0 && (unsigned)l >= HW) { bad = true; continue; }     // labels that no components call wrote: nothing is written for it
        const long long c = cc_load(src, p.src8, p.src_lut, i);
        long long o = c;
        if (l >= 0 && areas[l] < p.min_area && (unsigned long long)c < (unsigned long long)K && !((p.fixed >> (int)(c & 31)) & 1u)) {
            if (p.to >= 0) o = p.to;
            else {
                const unsigned long long key = p.best[mapoff + l];
                const unsigned donor = (unsigned)(CC_ROOT_MASK - (key & CC_ROOT_MASK));
                if (key && donor < HW) o = cc_load(src, p.src8, p.src_lut, (int)donor);     // the donor's class in the pass's INPUT map
            }
        }
        if (p.dst8) static_cast<long long*>(p.dst)[mapoff + i] = o;
        else static_cast<unsigned char*>(p.dst)[mapoff + i] = (unsigned char)o;
        nchanged += o != c ? 1u : 0u;
        if (lab) {
            const int t = p.lut[lab[i]];
            if ((unsigned)t < (unsigned)K && (unsigned long long)o < (unsigned long long)K) atomicAdd(&bins[(t * K + (int)o) * COPIES + (lane & (COPIES - 1))], 1u);
        }
    }
    if (bad) atomicOr(p.status, CC_ST_LABELS);
    if (p.changed) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) nchanged += (unsigned)__shfl_xor((int)nchanged, s);
        if (lane == 0) wchanged[threadIdx.x >> 6] = nchanged;
    }
    if (p.changed || p.hist) __syncthreads();
    if (p.changed && threadIdx.x == 0) {
        unsigned n = 0u;
#pragma unroll
        for (int w = 0; w < NTHREADS / WAVE; ++w) n += wchanged[w];
        if (n) atomicAdd(p.changed + m, (unsigned long long)n);
    }
    if (p.hist) {
        for (int i = threadIdx.x; i < K * K; i += NTHREADS) {
            unsigned n = 0u;
            for (int c = 0; c < COPIES; ++c) n += bins[i * COPIES + ((c + lane) & (COPIES - 1))];      // staggered: no two lanes on a bank
            if (n) atomicAdd(p.hist + i, (unsigned long long)n);
        }
    }
}

// ---- host side: every argument checked and the kernels' parameters derived, in plain host code without a HIP call ----------------------
static int cc_common(const char* who, const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int64_t& tx, int64_t& ty,
                     int64_t& fb) {
    if (src_bytes != 1 && src_bytes != 8) { set_error("%s: the element width of src must be 1 (uint8) or 8 (int64) bytes, got %d", who, src_bytes); return S2K_EINVAL; }
    if (src_lut && src_bytes != 1) { set_error("%s: src_lut reads a 1-byte src only", who); return S2K_EINVAL; }
    if (K < 1 || K > CC_MAXK) { set_error("%s: K = %d outside 1..%d", who, K, CC_MAXK); return S2K_EINVAL; }
    if (M < 1 || H < 1 || W < 1) { set_error("%s: bad dims (M, H and W must be positive)", who); return S2K_EINVAL; }
    if ((int64_t)H * W > 0x7fffffffll) { set_error("%s: bad dims (H * W must stay below 2^31: offsets inside a map are 32-bit)", who); return S2K_EINVAL; }
    tx = cdiv64(W, CC_TILE_W);
    ty = cdiv64(H, CC_TILE_H);
    fb = cdiv64((int64_t)H * W, CC_TILE);
    if (tx * ty > CC_MAX_GRID || tx * ty * M > CC_MAX_GRID) {
        set_error("%s: bad dims (M * tile rows * tile columns must stay below 2^24 workgroups)", who);
        return S2K_EINVAL;
    }
    return S2K_OK;
}

static int components_params(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int connectivity, unsigned exclude,
                             int* labels, int* areas, unsigned long long* counts, unsigned* status, ComponentsP& p) {
    const char* who = "classmap_components";
    if (!src || !labels || !areas || !status) { set_error("%s: null pointer (src, labels, areas and status are required)", who); return S2K_EFAULT; }
    int64_t tx, ty, fb;
    const int rc = cc_common(who, src, src_bytes, src_lut, M, H, W, K, tx, ty, fb);
    if (rc != S2K_OK) return rc;
    if (connectivity != 4 && connectivity != 8) { set_error("%s: connectivity = %d (4 or 8)", who, connectivity); return S2K_EINVAL; }
    const unsigned all = K == 32 ? 0xffffffffu : (1u << K) - 1u;
    if (exclude & ~all) { set_error("%s: exclude names a class at or above K = %d", who, K); return S2K_EINVAL; }
    p = ComponentsP{};
    p.src = src; p.src_lut = src_lut; p.labels = labels; p.areas = areas; p.counts = counts; p.status = status;
    p.M = M; p.H = H; p.W = W; p.K = K; p.src8 = src_bytes == 8; p.conn8 = connectivity == 8; p.exclude = exclude;
    p.TX = (int)tx; p.TY = (int)ty; p.FB = (int)fb;
    p.NR = (H - 1) / CC_TILE_H; p.NC = (W - 1) / CC_TILE_W;
    p.E = p.NR * W + p.NC * H;                                  // < H * W / 16 + H * W / 64
    p.EB = cdiv(p.E, NTHREADS);
    if ((int64_t)p.EB * M > CC_MAX_GRID) { set_error("%s: bad dims (the tile edges of M maps must stay below 2^24 workgroups)", who); return S2K_EINVAL; }
    return S2K_OK;
}

int check_classmap_components(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int connectivity, unsigned exclude,
                              int* labels, int* areas, unsigned long long* counts, unsigned* status) {
    ComponentsP p;
    return components_params(src, src_bytes, src_lut, M, H, W, K, connectivity, exclude, labels, areas, counts, status, p);
}

int launch_classmap_components(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int connectivity, unsigned exclude,
                               int* labels, int* areas, unsigned long long* counts, unsigned* status, hipStream_t st) {
    ComponentsP p;
    const int rc = components_params(src, src_bytes, src_lut, M, H, W, K, connectivity, exclude, labels, areas, counts, status, p);
    if (rc != S2K_OK) return rc;
    if (hipMemsetAsync(areas, 0, (size_t)M * H * W * sizeof(int), st) != hipSuccess) { set_error("classmap_components: hipMemsetAsync failed"); return S2K_EHIP; }
    hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)((int64_t)M * p.TY * p.TX)), dim3(NTHREADS), 0, st, p);
    if (p.E > 0) hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)((int64_t)M * p.EB)), dim3(NTHREADS), 0, st, p);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)((int64_t)M * p.FB)), dim3(NTHREADS), 0, st, p);
    return S2K_OK;
}

static int sieve_params(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K, int min_area,
                        unsigned fixed, int to, const int* labels, const int* areas, unsigned long long* best, const unsigned char* hist_labels,
                        const int* index, const int* lut, int nsrc, unsigned long long* hist, unsigned long long* changed, unsigned* status,
                        SieveP& p) {
    const char* who = "classmap_sieve";
    if (!src || !dst || !labels || !areas || !status) {
        set_error("%s: null pointer (src, dst, labels, areas and status are required)", who);
        return S2K_EFAULT;
    }
    if (dst_bytes != 1 && dst_bytes != 8) { set_error("%s: the element width of dst must be 1 (uint8) or 8 (int64) bytes, got %d", who, dst_bytes); return S2K_EINVAL; }
    int64_t tx, ty, fb;
    const int rc = cc_common(who, src, src_bytes, src_lut, M, H, W, K, tx, ty, fb);
    if (rc != S2K_OK) return rc;
    if (src == dst) { set_error("%s: dst must not alias src", who); return S2K_EINVAL; }
    if (min_area < 1) { set_error("%s: min_area = %d must be at least 1", who, min_area); return S2K_EINVAL; }
    const unsigned all = K == 32 ? 0xffffffffu : (1u << K) - 1u;
    if (fixed & ~all) { set_error("%s: fixed names a class at or above K = %d", who, K); return S2K_EINVAL; }
    if (to < -1 || to >= K) { set_error("%s: to = %d must be -1 or a class in [0, %d)", who, to, K); return S2K_EINVAL; }
    if (to < 0 && !best) { set_error("%s: best is required without `to` (the donor workspace)", who); return S2K_EINVAL; }
    if (hist && (!hist_labels || !index || !lut || nsrc < 1)) {
        set_error("%s: hist needs hist_labels, index, lut and nsrc >= 1", who);
        return S2K_EINVAL;
    }
    p = SieveP{};
    p.src = src; p.dst = dst; p.src_lut = src_lut; p.labels = labels; p.areas = areas; p.best = to < 0 ? best : nullptr;
    p.hist_labels = hist_labels; p.index = index; p.lut = lut; p.hist = hist; p.changed = changed; p.status = status;
    p.M = M; p.H = H; p.W = W; p.K = K; p.NSRC = nsrc; p.src8 = src_bytes == 8; p.dst8 = dst_bytes == 8; p.min_area = min_area; p.to = to;
    p.fixed = fixed;
    p.FB = (int)fb;
    p.copies = 1;
    while (p.copies < 16 && 2 * p.copies * K * K <= 1024) p.copies *= 2;
    return S2K_OK;
}

int check_classmap_sieve(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K, int min_area,
                         unsigned fixed, int to, const int* labels, const int* areas, unsigned long long* best, const unsigned char* hist_labels,
                         const int* index, const int* lut, int nsrc, unsigned long long* hist, unsigned long long* changed, unsigned* status) {
    SieveP p;
    return sieve_params(src, src_bytes, src_lut, dst, dst_bytes, M, H, W, K, min_area, fixed, to, labels, areas, best, hist_labels, index, lut, nsrc,
                        hist, changed, status, p);
}

int launch_classmap_sieve(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K, int min_area,
                          unsigned fixed, int to, const int* labels, const int* areas, unsigned long long* best, const unsigned char* hist_labels,
                          const int* index, const int* lut, int nsrc, unsigned long long* hist, unsigned long long* changed, unsigned* status,
                          hipStream_t st) {
    SieveP p;
    const int rc = sieve_params(src, src_bytes, src_lut, dst, dst_bytes, M, H, W, K, min_area, fixed, to, labels, areas, best, hist_labels, index, lut,
                                nsrc, hist, changed, status, p);
    if (rc != S2K_OK) return rc;
    const dim3 grid((unsigned)((int64_t)M * p.FB));
    if (p.best) {
        if (hipMemsetAsync(p.best, 0, (size_t)M * H * W * sizeof(unsigned long long), st) != hipSuccess) {
            set_error("classmap_sieve: hipMemsetAsync failed");
            return S2K_EHIP;
        }
        hipLaunchKernelGGL(cc_donor_kernel, grid, dim3(NTHREADS), 0, st, p);
    }
    hipLaunchKernelGGL(cc_relabel_kernel, grid, dim3(NTHREADS), 0, st, p);
    return S2K_OK;
}

}  // namespace s2k
