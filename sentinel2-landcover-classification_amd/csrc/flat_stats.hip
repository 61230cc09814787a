// Per-tensor statistics, histograms and global-norm clipping over a flat f32 buffer (flat_stats.py; stages SEG_STATS, SEG_HIST,
// GRAD_CLIP).  Every parameter and every gradient of a network is a slice of one contiguous buffer (flat.py), so what the reference's
// `logger.watch(model, log="all")` gathers with a min / max / histc and two host copies PER TENSOR (556 gradient tensors for U-Net b5) and what
// `clip_grad_norm_` gathers with a host loop over the same tensors are two streaming reads here, without the host in between.
//
// Work decomposition: the host cuts every segment {first, n} of SEGS into chunks of at most SEG_CHUNK floats and uploads one row
// {segment, chunk index within it} per chunk (CHUNKS, ascending).  One workgroup owns one chunk: a 2.4 M-float conv weight is 147
// workgroups side by side, 556 small tensors are 556 workgroups side by side, and the number of launches never depends on the number
// of segments.  The tables are validated on the host before upload; nothing here range-checks them.
//
// All three kernels are HBM streams: a chunk is read as 16-byte loads from the first 16-byte boundary on (every tensor of the flat
// buffers starts on a 64-float boundary and SEG_CHUNK keeps that for the later chunks), with up to three scalar elements in front and
// behind for any other start.  No floating-point atomics: sums have a fixed order - per thread in ascending address, a butterfly through
// the wave, the four waves in order, then the chunks of a segment in ascending order - so the same bytes give the same bits.
#include "common.h"

namespace s2k {

constexpr int SEG_CHUNK = 16384;        // floats per chunk (flat_stats.CHUNK): 256 threads x 16 quads
constexpr int SEG_UNROLL = 4;           // 16-byte loads a thread keeps in flight

// chunk c of the table -> its segment p and its floats [x, x + n)
__device__ __forceinline__ const float* chunk_span(const float* X, const int* segs, const int* chunks, int c, int& p, int& n) {
    p = chunks[2 * c];
    const int k = chunks[2 * c + 1];
    const int left = segs[2 * p + 1] - k * SEG_CHUNK;
    n = left < SEG_CHUNK ? left : SEG_CHUNK;
    return X + ((int64_t)segs[2 * p] + (int64_t)k * SEG_CHUNK);
}

// f(v) for every element of [x, x + n), each thread in ascending address: the (at most three) elements in front of the first 16-byte
// boundary go to threads 0..2 before their quads, quad j to thread j % 256, the elements behind the last quad to threads 0..2 after
// their quads.  The quad loads of one round are unconditional (a clamped index), so the compiler issues them together.
template <typename F>
__device__ __forceinline__ void chunk_visit(const float* x, int n, F&& f) {
    const int tid = threadIdx.x;
    int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(x) >> 2) & 3u)) & 3u);
    if (head > n) head = n;
    const int nv = (n - head) >> 2, tail = n - head - 4 * nv;
    if (tid < head) f(x[tid]);
    if (nv > 0) {
        const float4* xv = reinterpret_cast<const float4*>(x + head);
        for (int j0 = tid; j0 < nv; j0 += SEG_UNROLL * NTHREADS) {
            float4 v[SEG_UNROLL];
#pragma unroll
            for (int u = 0; u < SEG_UNROLL; ++u) {
                const int j = j0 + u * NTHREADS;
                v[u] = xv[j < nv ? j : nv - 1];
            }
#pragma unroll
            for (int u = 0; u < SEG_UNROLL; ++u)
                if (j0 + u * NTHREADS < nv) { f(v[u].x); f(v[u].y); f(v[u].z); f(v[u].w); }
        }
    }
    if (tid < tail) f(x[head + 4 * nv + tid]);
}

// ---- SEG_STATS ------------------------------------------------------------------------------------------------------------------
// pass 1, one workgroup per chunk: PART[c] = {sum, sumsq, min, max, #NaN, #Inf} (the counts as int64 bit patterns in the f64 slots)
__global__ void __launch_bounds__(NTHREADS) seg_stats_chunk_kernel(const float* X, const int* segs, const int* chunks, double* part) {
    __shared__ double ws[4], wq[4];
    __shared__ float wmn[4], wmx[4];
    __shared__ int wnan[4], winf[4];
    int p, n;
    const float* x = chunk_span(X, segs, chunks, blockIdx.x, p, n);
    double s = 0.0, q = 0.0;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int nnan = 0, ninf = 0;
    chunk_visit(x, n, [&](float v) {
        const double d = (double)v;
        q += d * d;                                  // over ALL elements: a NaN / Inf propagates (torch's norm)
        const bool fin = __builtin_isfinite(v);
        s += fin ? d : 0.0;                          // sum, min, max over the finite ones
        mn = fminf(mn, fin ? v : __builtin_inff());
        mx = fmaxf(mx, fin ? v : -__builtin_inff());
        nnan += (v != v) ? 1 : 0;
        ninf += (!fin && v == v) ? 1 : 0;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {               // butterfly: every lane ends with the same bits
        s += __shfl_xor(s, o, 64);
        q += __shfl_xor(q, o, 64);
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        nnan += __shfl_xor(nnan, o, 64);
        ninf += __shfl_xor(ninf, o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { ws[w] = s; wq[w] = q; wmn[w] = mn; wmx[w] = mx; wnan[w] = nnan; winf[w] = ninf; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < NTHREADS / WAVE; ++i) {
            s += ws[i]; q += wq[i]; mn = fminf(mn, wmn[i]); mx = fmaxf(mx, wmx[i]); nnan += wnan[i]; ninf += winf[i];
        }
        double* o = part + 6 * (int64_t)blockIdx.x;
        o[0] = s; o[1] = q; o[2] = (double)mn; o[3] = (double)mx;
        o[4] = __builtin_bit_cast(double, (long long)nnan);
        o[5] = __builtin_bit_cast(double, (long long)ninf);
    }
}

// pass 2, one thread per chunk: the thread of a segment's first chunk adds that segment's partials in ascending order
__global__ void __launch_bounds__(NTHREADS) seg_stats_combine_kernel(const int* segs, const int* chunks, const double* part, double* stats,
                                                                     long long* counts, int NC) {
    const int c = blockIdx.x * NTHREADS + threadIdx.x;
    if (c >= NC || chunks[2 * c + 1] != 0) return;
    const int p = chunks[2 * c];
    const int nch = (segs[2 * p + 1] + SEG_CHUNK - 1) / SEG_CHUNK;
    const double* a = part + 6 * (int64_t)c;
    double s = a[0], q = a[1], mn = a[2], mx = a[3];
    long long nnan = __builtin_bit_cast(long long, a[4]), ninf = __builtin_bit_cast(long long, a[5]);
    for (int i = 1; i < nch; ++i) {
        a += 6;
        s += a[0]; q += a[1]; mn = fmin(mn, a[2]); mx = fmax(mx, a[3]);
        nnan += __builtin_bit_cast(long long, a[4]); ninf += __builtin_bit_cast(long long, a[5]);
    }
    double* o = stats + 4 * (int64_t)p;
    o[0] = s; o[1] = q; o[2] = mn; o[3] = mx;
    counts[2 * (int64_t)p] = nnan;
    counts[2 * (int64_t)p + 1] = ninf;
}

// ---- SEG_HIST -------------------------------------------------------------------------------------------------------------------
// One workgroup per chunk counts into u32 LDS bins and flushes the non-empty ones with 64-bit integer atomics (exact, order-free).
// Gradient values pile up in a few central bins and same-address LDS atomics of one wave serialise, so the bins exist R times: thread t
// counts into copy t % R (neighbouring lanes never share an address; copy r of bin b sits at b * R + r, neighbouring banks), and the
// flush adds the copies.  The product runs (and ships) R = 8 only; the tuning build can select 1, 4, 16, 32 to compare (S2K_HIST_REP; DESIGN section 4:
// one copy drops to a quarter of the rate when most values share a bin, 32 copies cost their zeroing and flush at 256 bins).
template <int R>
__global__ void __launch_bounds__(NTHREADS) seg_hist_kernel(const float* X, const int* segs, const int* chunks, const double* stats,
                                                            unsigned long long* hist, int NB) {
    extern __shared__ unsigned int bins[];           // [NB][R]
    const int tid = threadIdx.x;
    for (int i = tid; i < NB * R; i += NTHREADS) bins[i] = 0u;
    __syncthreads();
    int p, n;
    const float* x = chunk_span(X, segs, chunks, blockIdx.x, p, n);
    double lo = stats[4 * (int64_t)p + 2], hi = stats[4 * (int64_t)p + 3];
    if (lo == hi) { lo -= 1.0; hi += 1.0; }          // torch.histc's rule for a constant tensor
    const double width = hi - lo, nb = (double)NB;
    unsigned int* mine = bins + (tid & (R - 1));
    chunk_visit(x, n, [&](float v) {
        if (__builtin_isfinite(v)) {
            const double t = floor(((double)v - lo) / width * nb);
            // t == NB for v == hi; anything else outside [0, NB) can only come from a STATS that is not this buffer's: end bins
            const int b = (t >= 0.0 && t < nb) ? (int)t : (t >= nb ? NB - 1 : 0);
            atomicAdd(mine + b * R, 1u);
        }
    });
    __syncthreads();
    for (int b = tid; b < NB; b += NTHREADS) {
        unsigned int t = 0u;
#pragma unroll
        for (int r = 0; r < R; ++r) t += bins[b * R + r];
        if (t) atomicAdd(hist + (int64_t)p * NB + b, (unsigned long long)t);
    }
}

// ---- GRAD_CLIP ------------------------------------------------------------------------------------------------------------------
// Every workgroup adds the segments' sums of squares itself (ascending p, f64: staged through LDS 1024 at a time, one thread adds), so
// all of them hold the same coef bit for bit and nothing travels through the host or a second launch.  coef >= 1: nothing is written.
__global__ void __launch_bounds__(NTHREADS) grad_clip_kernel(float* X, const int* segs, const int* chunks, const double* stats, float* norm,
                                                             int P, double max_norm, int apply) {
    __shared__ double buf[1024];
    __shared__ float coef_s;
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int p0 = 0; p0 < P; p0 += 1024) {
        const int m = P - p0 < 1024 ? P - p0 : 1024;
        for (int i = tid; i < m; i += NTHREADS) buf[i] = stats[4 * (int64_t)(p0 + i) + 1];
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < m; ++i) total += buf[i];
        __syncthreads();
    }
    if (tid == 0) {
        const double nrm = sqrt(total);
        if (blockIdx.x == 0) norm[0] = (float)nrm;
        double coef = max_norm / (nrm + 1e-6);
        coef = coef > 1.0 ? 1.0 : coef;              // a NaN stays a NaN (torch.clamp(nan, max=1)); fmin would return 1
        coef_s = (float)coef;
    }
    __syncthreads();
    const float coef = coef_s;
    if (!apply || coef >= 1.0f) return;
    int p, n;
    float* x = const_cast<float*>(chunk_span(X, segs, chunks, blockIdx.x, p, n));
    int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(x) >> 2) & 3u)) & 3u);
    if (head > n) head = n;
    const int nv = (n - head) >> 2, tail = n - head - 4 * nv;
    if (tid < head) x[tid] *= coef;
    float4* xv = reinterpret_cast<float4*>(x + head);
    for (int j0 = tid; j0 < nv; j0 += SEG_UNROLL * NTHREADS) {
        float4 v[SEG_UNROLL];
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) {
            const int j = j0 + u * NTHREADS;
            v[u] = xv[j < nv ? j : j0];              // a lane without a quad re-reads its OWN first one: no other lane ever stores there
        }
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) {
            const int j = j0 + u * NTHREADS;
            if (j < nv) xv[j] = make_float4(v[u].x * coef, v[u].y * coef, v[u].z * coef, v[u].w * coef);
        }
    }
    if (tid < tail) x[head + 4 * nv + tid] *= coef;
}

// ---- launchers: every check happens on the host before any HIP call ---------------------------------------------------------------
int launch_seg_stats(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    const float* X = r.ptr<const float>(op.t[S2K_SEG_STATS_T_X]);
    const int* segs = r.ptr<const int>(op.t[S2K_SEG_STATS_T_SEGS]);
    const int* chunks = r.ptr<const int>(op.t[S2K_SEG_STATS_T_CHUNKS]);
    double* part = r.ptr<double>(op.t[S2K_SEG_STATS_T_PART]);
    double* stats = r.ptr<double>(op.t[S2K_SEG_STATS_T_STATS]);
    long long* counts = r.ptr<long long>(op.t[S2K_SEG_STATS_T_COUNTS]);
    if (r.absent) return r.fault("seg_stats");
    if (!X || !segs || !chunks || !part || !stats || !counts) { set_error("seg_stats: missing tensor"); return S2K_EINVAL; }
    const int P = op.d[S2K_SEG_STATS_D_P], NC = op.d[S2K_SEG_STATS_D_NC];
    if (P < 1 || NC < P) { set_error("seg_stats: bad dims (P >= 1 segments, NC >= P chunks)"); return S2K_EINVAL; }
    hipLaunchKernelGGL(seg_stats_chunk_kernel, dim3((unsigned)NC), dim3(NTHREADS), 0, c.stream, X, segs, chunks, part);
    hipLaunchKernelGGL(seg_stats_combine_kernel, dim3((unsigned)cdiv(NC, NTHREADS)), dim3(NTHREADS), 0, c.stream, segs, chunks, part, stats,
                       counts, NC);
    return S2K_OK;
}

template <int R>
static void launch_hist_r(unsigned grid, hipStream_t stream, const float* X, const int* segs, const int* chunks, const double* stats,
                          unsigned long long* hist, int NB) {
    hipLaunchKernelGGL((seg_hist_kernel<R>), dim3(grid), dim3(NTHREADS), (size_t)NB * R * sizeof(unsigned int), stream, X, segs, chunks,
                       stats, hist, NB);
}

int launch_seg_hist(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    const float* X = r.ptr<const float>(op.t[S2K_SEG_HIST_T_X]);
    const int* segs = r.ptr<const int>(op.t[S2K_SEG_HIST_T_SEGS]);
    const int* chunks = r.ptr<const int>(op.t[S2K_SEG_HIST_T_CHUNKS]);
    const double* stats = r.ptr<const double>(op.t[S2K_SEG_HIST_T_STATS]);
    unsigned long long* hist = r.ptr<unsigned long long>(op.t[S2K_SEG_HIST_T_HIST]);
    if (r.absent) return r.fault("seg_hist");
    if (!X || !segs || !chunks || !stats || !hist) { set_error("seg_hist: missing tensor"); return S2K_EINVAL; }
    const int P = op.d[S2K_SEG_HIST_D_P], NC = op.d[S2K_SEG_HIST_D_NC], NB = op.d[S2K_SEG_HIST_D_NB];
    if (P < 1 || NC < P || NB < 1 || NB > 256) {
        set_error("seg_hist: bad dims (P >= 1 segments, NC >= P chunks, 1 <= NB <= 256)");
        return S2K_EINVAL;
    }
    const unsigned grid = (unsigned)NC;
#ifdef S2K_TUNING
    static const int rep = tune_int("S2K_HIST_REP", 8);        // tuning build only: other replications to compare
    switch (rep) {
        case 1: launch_hist_r<1>(grid, c.stream, X, segs, chunks, stats, hist, NB); return S2K_OK;
        case 4: launch_hist_r<4>(grid, c.stream, X, segs, chunks, stats, hist, NB); return S2K_OK;
        case 16: launch_hist_r<16>(grid, c.stream, X, segs, chunks, stats, hist, NB); return S2K_OK;
        case 32: launch_hist_r<32>(grid, c.stream, X, segs, chunks, stats, hist, NB); return S2K_OK;
        default: break;
    }
#endif
    launch_hist_r<8>(grid, c.stream, X, segs, chunks, stats, hist, NB);        // 8 copies of the LDS bins: the measured choice
    return S2K_OK;
}

int launch_grad_clip(const S2kOp& op, const Ctx& c) {
    Refs r(c);
    float* X = r.ptr<float>(op.t[S2K_GRAD_CLIP_T_X]);
    const int* segs = r.ptr<const int>(op.t[S2K_GRAD_CLIP_T_SEGS]);
    const int* chunks = r.ptr<const int>(op.t[S2K_GRAD_CLIP_T_CHUNKS]);
    const double* stats = r.ptr<const double>(op.t[S2K_GRAD_CLIP_T_STATS]);
    float* norm = r.ptr<float>(op.t[S2K_GRAD_CLIP_T_NORM]);
    if (r.absent) return r.fault("grad_clip");
    const int P = op.d[S2K_GRAD_CLIP_D_P], NC = op.d[S2K_GRAD_CLIP_D_NC], apply = op.d[S2K_GRAD_CLIP_D_APPLY];
    if (!stats || !norm || (apply && (!X || !segs || !chunks))) { set_error("grad_clip: missing tensor"); return S2K_EINVAL; }
    const float max_norm = op.f[S2K_GRAD_CLIP_F_MAX_NORM];
    if (P < 1 || (apply != 0 && apply != 1) || (apply && (NC < P || !(max_norm > 0.0f) || !__builtin_isfinite(max_norm)))) {
        set_error("grad_clip: bad dims (P >= 1 segments, APPLY 0 or 1; with APPLY: NC >= P chunks, MAX_NORM positive and finite)");
        return S2K_EINVAL;
    }
    hipLaunchKernelGGL(grad_clip_kernel, dim3(apply ? (unsigned)NC : 1u), dim3(NTHREADS), 0, c.stream, X, segs, chunks, stats, norm, P,
                       apply ? (double)max_norm : 1.0, apply);
    return S2K_OK;
}

}  // namespace s2k
