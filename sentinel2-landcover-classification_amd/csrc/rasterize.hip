// Exact polygon rasterisation into label tiles (classmap.py: PolygonSet, rasterize; C entry s2k_rasterize, include/s2k.h).  The reference
// burns OSM polygons into 512 x 512 uint8 rasters on the host with rasterio.features.rasterize, one segment at a time
// (src/data/download_labels.py:203-227: the last overlapping feature wins); here the polygons are resident and every tile of a batch is
// burned on the GPU.  Integer work with one exact answer: vertices are fixed point (RAST_Q units per pixel), a pixel centre is inside a
// shape by the even-odd rule over half-open edges with the crossing compared exactly in int64 (the top-left rule), shapes are painted in
// index order.  The definition in include/s2k.h is the oracle (tests/rasterize_ref.py restates it in numpy).
//
// Three plain launches whatever the geometry looks like, nothing read back between them:
//   BOX    one wave per shape: the rings of a shape are consecutive in the tables (ring_shape does not decrease), so two binary searches
//          give its ring range and with it ONE vertex range; the wave strides over those vertices and stores the bounding box in units
//          and the two ranges, RAST_BOX_INTS ints per shape.  An empty shape gets an empty box.  The same launch checks the ring tables
//          (a grid-stride loop over the rings) and the vertex range, and reports into `status`.
//   LIST   one workgroup per tile walks the S boxes in chunks of its size and appends, in shape order (ballot + prefix, no unordered
//          append), the shapes whose box holds a pixel centre of the tile to the tile's list; then the list's length.
//   FILL   one workgroup per RAST_BLOCK_H x RAST_BLOCK_W block of a tile.  It walks the tile's list a chunk at a time, compacts - again in
//          order - the shapes whose box holds a centre of the BLOCK into a queue in LDS, and burns the queue one shape after the other:
//            edges   threads stride over the shape's edges (the ring of an edge: a binary search inside the shape's ring range, no step
//                    for a shape of one ring); for every block row whose centre the edge spans, the first column whose centre is not
//                    left of the crossing - ceil((num - 128 dy) / (256 dy)), one true floor division for the first row and an exact
//                    quotient / remainder step for the next - toggles a bit of an LDS parity plane (atomicXor); a column before the
//                    block's first toggles bit 0 (the parity entering from the left), one past its last nothing;
//            prefix  a prefix XOR along every row turns toggles into coverage: in-word by shifts, across the 16 words of a row by the
//                    parity of the preceding words' popcounts (a 64-bit ballot holds four rows of 16 words);
//            paint   the shape's value goes into the LDS value plane where the bit is set, the bit into a "covered" plane.
//          Two parity planes alternate, so a shape costs two barriers.  After the last shape the block is written to dst once; uncovered
//          pixels get `fill` (mode 0) or are left alone (mode 1), and their number is added to unfilled[m] with one atomic per workgroup.
// Every loop is bounded by a count passed by value or a compile-time constant: the searches by RAST_SEARCH_STEPS, the rows of an edge by
// RAST_BLOCK_H, a list by S, a vertex range by V - whatever the tables hold.  Every index read from a table is clamped before it is
// used, every coordinate to +-RAST_MAX_COORD, every origin to +-RAST_MAX_ORIGIN, so that tables the host could not see do no harm: they
// set a bit in `status` and the output is then not to be used.  Tile offsets are 64-bit, offsets inside a tile 32-bit.
#include "plain.h"

#include <climits>

namespace s2k {

constexpr int RAST_BLOCK_H = 32, RAST_BLOCK_W = 512;        // classmap.RAST_BLOCK_H, RAST_BLOCK_W: the block one FILL workgroup owns
constexpr int RAST_Q = 256;                                 // classmap.RAST_Q: units per pixel
constexpr int RAST_MAX_COORD = 1 << 28;                     // classmap.RAST_MAX_COORD: largest magnitude of a coordinate in units
constexpr int RAST_MAX_ORIGIN = RAST_MAX_COORD / RAST_Q;    // ... of a tile origin in pixels
constexpr int RAST_ROW_WORDS = RAST_BLOCK_W / 32, RAST_PLANE_WORDS = RAST_BLOCK_H * RAST_ROW_WORDS;
constexpr int RAST_BOX_INTS = 8;                            // x0, y0, x1, y1 (units), first ring, end ring, first vertex, end vertex
constexpr int RAST_SEARCH_STEPS = 32;                       // a binary search over fewer than 2^31 entries
constexpr int RAST_ENTRY_INTS = 8;                          // of the FILL queue: shape, columns, rows, v0, v1, r0, r1, value
constexpr unsigned RAST_BAD_TABLES = 1u, RAST_BAD_COORD = 2u, RAST_BAD_ORIGIN = 4u;
constexpr int64_t RAST_MAX_GRID = 0x7fffffffll;
constexpr size_t RAST_FILL_LDS = ((size_t)RAST_BLOCK_H * RAST_BLOCK_W + 3 * RAST_PLANE_WORDS + NTHREADS * RAST_ENTRY_INTS + NTHREADS / WAVE) * 4;

struct RastP {
    const int* verts;               // [V][2]
    const int* ring_start;          // [R + 1]
    const int* ring_shape;          // [R]
    const int* values;              // [S] or null (burn = index)
    const int* origins;             // [M][2]
    void* dst;                      // [M][H][W], 1, 4 or 8 bytes an element
    int* boxes;                     // work: [S][RAST_BOX_INTS]
    int* counts;                    // work: [M]
    int* lists;                     // work: [M][S]
    unsigned long long* unfilled;   // [M] or null
    unsigned* status;
    int V, R, S, M, H, W, dst_bytes, mode, burn, fill;
    int NBY, NBX;                   // blocks of a tile
};

__device__ __forceinline__ int rast_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int64_t rast_min64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t rast_max64(int64_t a, int64_t b) { return a > b ? a : b; }

// the first pixel whose centre 256 c + 128 is not below `units` (|units| <= 2^28): ceil((units - 128) / 256), the shift is a true floor
__device__ __forceinline__ int rast_first_centre(int units) { return (units + RAST_Q / 2 - 1) >> 8; }

// the first ring in [0, R] whose shape is not below s; at most RAST_SEARCH_STEPS steps whatever the table holds
__device__ __forceinline__ int rast_first_ring(const int* __restrict__ ring_shape, int R, int s) {
    int lo = 0, hi = R;
    for (int it = 0; it < RAST_SEARCH_STEPS && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ring_shape[mid] < s) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The rank of a keeping thread among the keeping threads of its workgroup, in thread order, and their number: a 64-bit ballot per wave,
// the waves' counts through `wave_n` (NTHREADS / WAVE ints of LDS).  Two barriers; every thread of the workgroup calls it.
__device__ __forceinline__ int rast_rank(bool keep, int* wave_n, int& total) {
    const unsigned long long b = __ballot(keep);
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    if (lane == 0) wave_n[w] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < NTHREADS / WAVE; ++i) {
        const int n = wave_n[i];
        before += i < w ? n : 0;
        total += n;
    }
    __syncthreads();
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// ---- BOX: grid ceil(S / 4), one wave per shape ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NTHREADS) rast_box_kernel(const RastP p) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int V = p.V, R = p.R, S = p.S;
    unsigned bad = 0u;
    // the ring tables: non-decreasing, ring_start from 0 to V, ring_shape inside [0, S)
    const int64_t threads = (int64_t)gridDim.x * NTHREADS;
    for (int64_t r = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; r < R; r += threads) {       // ceil(R / threads) steps
        const int a = p.ring_start[r], b = p.ring_start[r + 1], sh = p.ring_shape[r];
        if (a < 0 || b < a || b > V || sh < 0 || sh >= S || (r == 0 && a != 0) || (r == R - 1 && b != V) ||
            (r + 1 < R && p.ring_shape[r + 1] < sh))
            bad |= RAST_BAD_TABLES;
    }
    const int s = (int)blockIdx.x * (NTHREADS / WAVE) + ((int)threadIdx.x >> 6);
    if (s < S) {
        int r0 = rast_first_ring(p.ring_shape, R, s), r1 = rast_first_ring(p.ring_shape, R, s + 1);
        if (r1 < r0) r1 = r0;
        int v0 = rast_clamp(p.ring_start[r0], 0, V), v1 = rast_clamp(p.ring_start[r1], 0, V);
        if (v1 < v0) v1 = v0;
        int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
        const int2* __restrict__ verts = reinterpret_cast<const int2*>(p.verts);
        for (int i = v0 + lane; i < v1; i += WAVE) {            // ceil(V / 64) steps at most
            int2 v = verts[i];
            if (v.x < -RAST_MAX_COORD || v.x > RAST_MAX_COORD || v.y < -RAST_MAX_COORD || v.y > RAST_MAX_COORD) bad |= RAST_BAD_COORD;
            v.x = rast_clamp(v.x, -RAST_MAX_COORD, RAST_MAX_COORD);
            v.y = rast_clamp(v.y, -RAST_MAX_COORD, RAST_MAX_COORD);
            x0 = min(x0, v.x); y0 = min(y0, v.y); x1 = max(x1, v.x); y1 = max(y1, v.y);
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            x0 = min(x0, __shfl_xor(x0, o, WAVE)); y0 = min(y0, __shfl_xor(y0, o, WAVE));
            x1 = max(x1, __shfl_xor(x1, o, WAVE)); y1 = max(y1, __shfl_xor(y1, o, WAVE));
        }
        if (lane == 0) {
            if (x1 < x0) { x0 = y0 = 1; x1 = y1 = 0; }           // no vertex: a box that holds no centre
            int4* box = reinterpret_cast<int4*>(p.boxes + (int64_t)s * RAST_BOX_INTS);
            box[0] = make_int4(x0, y0, x1, y1);
            box[1] = make_int4(r0, r1, v0, v1);
        }
    }
    if (bad) atomicOr(p.status, bad);
}

// the origin of tile m in pixels, clamped; `bad` takes RAST_BAD_ORIGIN if it was out of range
__device__ __forceinline__ int2 rast_origin(const RastP& p, int m, unsigned& bad) {
    int2 o = reinterpret_cast<const int2*>(p.origins)[m];
    if (o.x < -RAST_MAX_ORIGIN || o.x > RAST_MAX_ORIGIN || o.y < -RAST_MAX_ORIGIN || o.y > RAST_MAX_ORIGIN) bad |= RAST_BAD_ORIGIN;
    o.x = rast_clamp(o.x, -RAST_MAX_ORIGIN, RAST_MAX_ORIGIN);
    o.y = rast_clamp(o.y, -RAST_MAX_ORIGIN, RAST_MAX_ORIGIN);
    return o;
}

// ---- LIST: grid M, one workgroup per tile ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NTHREADS) rast_list_kernel(const RastP p) {
    __shared__ int wave_n[NTHREADS / WAVE];
    const int m = blockIdx.x, S = p.S;
    unsigned bad = 0u;
    const int2 o = rast_origin(p, m, bad);
    if (bad && threadIdx.x == 0) atomicOr(p.status, bad);
    const int64_t c0 = o.x, c1 = (int64_t)o.x + p.W, r0 = o.y, r1 = (int64_t)o.y + p.H;      // the tile in AOI pixels
    int* __restrict__ list = p.lists + (int64_t)m * S;
    int base = 0;
    for (int s0 = 0; s0 < S; s0 += NTHREADS) {                  // ceil(S / 256) chunks
        const int s = s0 + (int)threadIdx.x;
        bool keep = false;
        if (s < S) {
            const int4 b = *reinterpret_cast<const int4*>(p.boxes + (int64_t)s * RAST_BOX_INTS);
            const int cl = rast_first_centre(b.x), ch = rast_first_centre(b.z), rl = rast_first_centre(b.y), rh = rast_first_centre(b.w);
            keep = cl < ch && rl < rh && cl < c1 && ch > c0 && rl < r1 && rh > r0;
        }
        int total;
        const int slot = rast_rank(keep, wave_n, total);
        if (keep) list[base + slot] = s;
        base += total;
    }
    if (threadIdx.x == 0) p.counts[m] = base;
}

// ---- FILL: grid M * NBY * NBX, one workgroup per block of a tile -------------------------------------------------------------------------------
__device__ __forceinline__ void rast_store(void* dst, int dst_bytes, int64_t off, int v) {
    if (dst_bytes == 1) static_cast<unsigned char*>(dst)[off] = (unsigned char)v;
    else if (dst_bytes == 4) static_cast<int*>(dst)[off] = v;
    else static_cast<long long*>(dst)[off] = (long long)v;
}

__global__ void __launch_bounds__(NTHREADS) rast_fill_kernel(const RastP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned int rast_lds[];
    int* val = reinterpret_cast<int*>(rast_lds);                            // [RAST_BLOCK_H][RAST_BLOCK_W] the value of the last shape
    unsigned int* cov = rast_lds + RAST_BLOCK_H * RAST_BLOCK_W;             // [RAST_BLOCK_H][RAST_ROW_WORDS] covered by any shape
    unsigned int* par = cov + RAST_PLANE_WORDS;                             // two parity planes
    int* queue = reinterpret_cast<int*>(par + 2 * RAST_PLANE_WORDS);        // [NTHREADS][RAST_ENTRY_INTS]
    int* wave_n = queue + NTHREADS * RAST_ENTRY_INTS;                       // [NTHREADS / WAVE]
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int V = p.V, S = p.S, H = p.H, W = p.W;
    const unsigned per = (unsigned)(p.NBY * p.NBX), bid = blockIdx.x;
    const int m = (int)(bid / per), by = (int)((bid % per) / (unsigned)p.NBX), bx = (int)((bid % per) % (unsigned)p.NBX);
    unsigned bad = 0u;
    const int2 o = rast_origin(p, m, bad);                                  // LIST reported it
    const int row0 = by * RAST_BLOCK_H, col0 = bx * RAST_BLOCK_W;
    const int nrows = min(RAST_BLOCK_H, H - row0), ncols = min(RAST_BLOCK_W, W - col0);
    const int64_t ar0 = (int64_t)o.y + row0, ac0 = (int64_t)o.x + col0;     // the block's first row and column in AOI pixels
    for (int i = tid; i < 3 * RAST_PLANE_WORDS; i += NTHREADS) cov[i] = 0u; // cov and both parity planes; rast_rank's barriers order it
    const int n = rast_clamp(p.counts[m], 0, S);
    const int* __restrict__ list = p.lists + (int64_t)m * S;
    const int2* __restrict__ verts = reinterpret_cast<const int2*>(p.verts);
    int flip = 0;
    for (int l0 = 0; l0 < n; l0 += NTHREADS) {                  // ceil(S / 256) chunks at most
        // the shapes of this chunk whose box holds a centre of the block, in list order, into the queue
        const int li = l0 + tid;
        bool keep = false;
        int s = 0, lc0 = 0, lc1 = 0, lr0 = 0, lr1 = 0;
        int4 rng = make_int4(0, 0, 0, 0);
        if (li < n) {
            s = rast_clamp(list[li], 0, S - 1);
            const int4 b = *reinterpret_cast<const int4*>(p.boxes + (int64_t)s * RAST_BOX_INTS);
            rng = *reinterpret_cast<const int4*>(p.boxes + (int64_t)s * RAST_BOX_INTS + 4);
            lc0 = (int)rast_max64((int64_t)rast_first_centre(b.x) - ac0, 0);
            lc1 = (int)rast_min64((int64_t)rast_first_centre(b.z) - ac0, ncols);
            lr0 = (int)rast_max64((int64_t)rast_first_centre(b.y) - ar0, 0);
            lr1 = (int)rast_min64((int64_t)rast_first_centre(b.w) - ar0, nrows);
            keep = lc0 < lc1 && lr0 < lr1;
        }
        int total;
        const int slot = rast_rank(keep, wave_n, total);        // its first barrier: every thread is done with the previous queue
        if (keep) {
            int4* e = reinterpret_cast<int4*>(queue + slot * RAST_ENTRY_INTS);
            e[0] = make_int4(s, lc0 | (lc1 << 16), lr0 | (lr1 << 16), p.burn ? s : p.values[s]);
            e[1] = rng;
        }
        __syncthreads();
        for (int q = 0; q < total; ++q) {                       // at most 256 shapes
            const int4 e0 = *reinterpret_cast<const int4*>(queue + q * RAST_ENTRY_INTS);
            const int4 e1 = *reinterpret_cast<const int4*>(queue + q * RAST_ENTRY_INTS + 4);
            const int qc0 = e0.y & 0xffff, qc1 = e0.y >> 16, qr0 = e0.z & 0xffff, qr1 = e0.z >> 16, value = e0.w;
            const int r0 = rast_clamp(e1.x, 0, p.R), r1 = rast_clamp(e1.y, r0, p.R), v0 = rast_clamp(e1.z, 0, V), v1 = rast_clamp(e1.w, v0, V);
            unsigned int* pp = par + flip * RAST_PLANE_WORDS;   // zero: cleared at the start, or during the shape before the last
            // edges: toggle the first column at or right of every crossing
            for (int e = v0 + tid; e < v1; e += NTHREADS) {     // ceil(V / 256) steps at most
                int lo = r0, hi = r1;                           // the ring of vertex e: the last ring of [r0, r1) that starts at or before e
                for (int it = 0; it < RAST_SEARCH_STEPS && hi - lo > 1; ++it) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (p.ring_start[mid] <= e) lo = mid; else hi = mid;
                }
                if (lo >= p.R) continue;                        // r0 == r1 == R: corrupt tables only
                const int a = rast_clamp(p.ring_start[lo], 0, V), b = rast_clamp(p.ring_start[lo + 1], 0, V);
                if (b - a < 3 || e < a || e >= b) continue;     // a ring of fewer than 3 vertices covers nothing
                int2 u = verts[e], w = verts[e + 1 == b ? a : e + 1];
                u.x = rast_clamp(u.x, -RAST_MAX_COORD, RAST_MAX_COORD); u.y = rast_clamp(u.y, -RAST_MAX_COORD, RAST_MAX_COORD);
                w.x = rast_clamp(w.x, -RAST_MAX_COORD, RAST_MAX_COORD); w.y = rast_clamp(w.y, -RAST_MAX_COORD, RAST_MAX_COORD);
                if (u.y == w.y) continue;                       // horizontal edges never count
                const int xlo = u.y < w.y ? u.x : w.x, ylo = u.y < w.y ? u.y : w.y, xhi = u.y < w.y ? w.x : u.x, yhi = u.y < w.y ? w.y : u.y;
                // the AOI rows whose centre lies in [ylo, yhi), cut to the rows of the block the box reaches
                const int64_t ra = rast_max64(rast_first_centre(ylo), ar0 + qr0), rb = rast_min64(rast_first_centre(yhi), ar0 + qr1);
                if (ra >= rb) continue;
                const int64_t dy = (int64_t)yhi - ylo, dx = (int64_t)xhi - xlo, D = RAST_Q * dy;
                const int64_t cy = RAST_Q * ra + RAST_Q / 2;
                // first column: ceil(N / D), N = xlo dy + (cy - ylo) dx - 128 dy; |N| < 2^60.  q = floor(N / D), rm = N - q D in [0, D)
                const int64_t N = (int64_t)xlo * dy + (cy - ylo) * dx - (RAST_Q / 2) * dy;
                int64_t q64 = N / D, rm = N % D;
                if (rm < 0) { q64 -= 1; rm += D; }              // C++ division truncates: make it a true floor
                const int64_t step = RAST_Q * dx;               // N of the next row
                int64_t sq = step / D, sr = step % D;
                if (sr < 0) { sq -= 1; sr += D; }
                const int row = (int)(ra - ar0);
                for (int i = 0; i < RAST_BLOCK_H; ++i) {
                    if (ra + i >= rb) break;
                    const int64_t col = q64 + (rm > 0 ? 1 : 0) - ac0;       // block column of the first centre not left of the crossing
                    if (col < ncols) {
                        const int j = col <= 0 ? 0 : (int)col;              // before the block: the parity enters at bit 0
                        atomicXor(&pp[(row + i) * RAST_ROW_WORDS + (j >> 5)], 1u << (j & 31));
                    }
                    q64 += sq; rm += sr;
                    if (rm >= D) { rm -= D; q64 += 1; }
                }
            }
            __syncthreads();
            // prefix XOR along every row; 16 lanes hold the 16 words of a row, a wave four rows
#pragma unroll
            for (int k = 0; k < RAST_PLANE_WORDS / NTHREADS; ++k) {
                const int idx = k * NTHREADS + tid;
                unsigned int w = pp[idx];
                const unsigned long long odd = __ballot(__popc(w) & 1);
                const unsigned before = (unsigned)(odd >> (lane & ~(RAST_ROW_WORDS - 1))) & ((1u << (lane & (RAST_ROW_WORDS - 1))) - 1u);
                w ^= w << 1; w ^= w << 2; w ^= w << 4; w ^= w << 8; w ^= w << 16;
                if (__popc(before) & 1) w = ~w;
                pp[idx] = w;
                cov[idx] |= w;                                  // idx is this thread's own in every shape
                par[(flip ^ 1) * RAST_PLANE_WORDS + idx] = 0u;  // the next shape's plane: last read before the barrier above
            }
            __syncthreads();
            // paint the box's part of the block
            const int wd = qc1 - qc0, cells = (qr1 - qr0) * wd;
            for (int i = tid; i < cells; i += NTHREADS) {       // at most RAST_BLOCK_H * RAST_BLOCK_W / 256 steps
                const int r = qr0 + i / wd, c = qc0 + i % wd;
                if ((pp[r * RAST_ROW_WORDS + (c >> 5)] >> (c & 31)) & 1u) val[r * RAST_BLOCK_W + c] = value;
            }
            flip ^= 1;
        }
    }
    __syncthreads();
    // the block, once
    const int64_t tile = (int64_t)m * H * W;
    unsigned long long open = 0ull;
    for (int it = 0; it < nrows * (RAST_BLOCK_W / NTHREADS); ++it) {
        const int pix = it * NTHREADS + tid, r = pix / RAST_BLOCK_W, c = pix % RAST_BLOCK_W;
        const bool valid = c < ncols;
        const bool covered = (cov[r * RAST_ROW_WORDS + (c >> 5)] >> (c & 31)) & 1u;
        if (valid) {
            const int64_t off = tile + (int64_t)(row0 + r) * W + (col0 + c);
            if (covered) rast_store(p.dst, p.dst_bytes, off, val[pix]);
            else if (p.mode == 0) rast_store(p.dst, p.dst_bytes, off, p.fill);
        }
        open += (unsigned long long)__popcll(__ballot(valid && !covered));
    }
    if (p.unfilled) {
        if (lane == 0) wave_n[tid >> 6] = (int)open;            // at most RAST_BLOCK_H * RAST_BLOCK_W
        __syncthreads();
        if (tid == 0) {
            unsigned long long sum = 0ull;
            for (int i = 0; i < NTHREADS / WAVE; ++i) sum += (unsigned long long)wave_n[i];
            if (sum) atomicAdd(p.unfilled + m, sum);
        }
    }
}

// ---- host side: every argument checked and the kernels' parameters derived, in plain host code without a HIP call ----------------------
static int rasterize_params(const int* verts, int V, const int* ring_start, const int* ring_shape, int R, const int* values, int S,
                            const int* origins, int M, int H, int W, void* dst, int dst_bytes, int mode, int burn, int fill, void* work,
                            long long* unfilled, int* status, RastP& p) {
    const char* who = "rasterize";
    if (!verts || !ring_start || !ring_shape || !origins || !dst || !work || !status) {
        set_error("%s: null pointer (verts, ring_start, ring_shape, origins, dst, work and status are required)", who);
        return S2K_EFAULT;
    }
    if (reinterpret_cast<uintptr_t>(verts) % 8 || reinterpret_cast<uintptr_t>(origins) % 8 || reinterpret_cast<uintptr_t>(work) % 16) {
        set_error("%s: verts and origins must be 8-byte aligned (pairs are read whole), work 16-byte aligned", who);
        return S2K_EINVAL;
    }
    if (V < 0 || R < 0 || S < 0) { set_error("%s: V = %d, R = %d, S = %d must not be negative", who, V, R, S); return S2K_EINVAL; }
    if (R > V || (R > 0 && S == 0)) { set_error("%s: R = %d rings need at least as many vertices (V = %d) and a shape (S = %d)", who, R, V, S); return S2K_EINVAL; }
    if (R == 0 && V != 0) { set_error("%s: V = %d vertices without a ring (ring_start runs from 0 to V)", who, V); return S2K_EINVAL; }
    if (dst_bytes != 1 && dst_bytes != 4 && dst_bytes != 8) { set_error("%s: the element width of dst must be 1, 4 or 8 bytes, got %d", who, dst_bytes); return S2K_EINVAL; }
    if (mode != 0 && mode != 1) { set_error("%s: mode = %d (0 fill, 1 onto)", who, mode); return S2K_EINVAL; }
    if (burn != 0 && burn != 1) { set_error("%s: burn = %d (0 value, 1 index)", who, burn); return S2K_EINVAL; }
    if (burn == 1 && dst_bytes == 1) { set_error("%s: burn = index needs a dst of 4 or 8 bytes an element", who); return S2K_EINVAL; }
    if (burn == 0 && !values && S > 0) { set_error("%s: burn = value needs values", who); return S2K_EINVAL; }
    if (dst_bytes == 1 && (fill < 0 || fill > 255)) { set_error("%s: fill = %d does not fit a 1-byte dst", who, fill); return S2K_EINVAL; }
    if (M < 1 || H < 1 || W < 1) { set_error("%s: bad dims (M, H and W must be positive)", who); return S2K_EINVAL; }
    if ((int64_t)H * W > 0x7fffffffll) { set_error("%s: bad dims (H * W must stay below 2^31: offsets inside a tile are 32-bit)", who); return S2K_EINVAL; }
    const int NBY = cdiv(H, RAST_BLOCK_H), NBX = cdiv(W, RAST_BLOCK_W);
    if ((int64_t)M * NBY * NBX > RAST_MAX_GRID) {
        set_error("%s: bad dims (M * ceil(H / %d) * ceil(W / %d) must stay below 2^31 workgroups)", who, RAST_BLOCK_H, RAST_BLOCK_W);
        return S2K_EINVAL;
    }
    p = RastP{};
    p.verts = verts; p.ring_start = ring_start; p.ring_shape = ring_shape; p.values = values; p.origins = origins; p.dst = dst;
    p.boxes = static_cast<int*>(work);
    p.counts = p.boxes + (size_t)S * RAST_BOX_INTS;
    p.lists = p.counts + M;
    p.unfilled = reinterpret_cast<unsigned long long*>(unfilled);
    p.status = reinterpret_cast<unsigned*>(status);
    p.V = V; p.R = R; p.S = S; p.M = M; p.H = H; p.W = W; p.dst_bytes = dst_bytes; p.mode = mode; p.burn = burn; p.fill = fill;
    p.NBY = NBY; p.NBX = NBX;
    return S2K_OK;
}

int check_rasterize(const int* verts, int V, const int* ring_start, const int* ring_shape, int R, const int* values, int S, const int* origins,
                    int M, int H, int W, void* dst, int dst_bytes, int mode, int burn, int fill, void* work, long long* unfilled, int* status) {
    RastP p;
    return rasterize_params(verts, V, ring_start, ring_shape, R, values, S, origins, M, H, W, dst, dst_bytes, mode, burn, fill, work, unfilled,
                            status, p);
}

int launch_rasterize(const int* verts, int V, const int* ring_start, const int* ring_shape, int R, const int* values, int S, const int* origins,
                     int M, int H, int W, void* dst, int dst_bytes, int mode, int burn, int fill, void* work, long long* unfilled, int* status,
                     hipStream_t st) {
    RastP p;
    const int rc = rasterize_params(verts, V, ring_start, ring_shape, R, values, S, origins, M, H, W, dst, dst_bytes, mode, burn, fill, work,
                                    unfilled, status, p);
    if (rc != S2K_OK) return rc;
    static PerDeviceOnce attr_once;                             // 77 KB of LDS: above the 64 KB a kernel gets unasked
    attr_once.run([&] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(rast_fill_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RAST_FILL_LDS); });
    // the same three launches whatever V, R and S are: with S = 0 BOX has one idle workgroup and every list is empty
    hipLaunchKernelGGL(rast_box_kernel, dim3((unsigned)(S > 0 ? cdiv(S, NTHREADS / WAVE) : 1)), dim3(NTHREADS), 0, st, p);
    hipLaunchKernelGGL(rast_list_kernel, dim3((unsigned)M), dim3(NTHREADS), 0, st, p);
    hipLaunchKernelGGL(rast_fill_kernel, dim3((unsigned)((int64_t)M * p.NBY * p.NBX)), dim3(NTHREADS), RAST_FILL_LDS, st, p);
    return S2K_OK;
}

// boxes, counts and lists, 4 bytes each
size_t rasterize_workspace(int M, int S) {
    if (M < 1 || S < 0) return 0;
    return ((size_t)S * RAST_BOX_INTS + (size_t)M + (size_t)M * (size_t)S) * sizeof(int);
}

}  // namespace s2k
