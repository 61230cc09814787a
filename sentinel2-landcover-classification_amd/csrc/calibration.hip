// Calibration of a probability map (metrics.CalibrationMetrics, classmap.confidence): from [N][K][P] scores - blended probabilities or
// logits - and the labels, in ONE streaming pass: the confidence raster, the class map with an optional abstention class, the
// reliability histogram per predicted class, and the negative log-likelihood under up to eight temperatures.  The definitions are in
// include/s2k.h at s2k_calibration; the reference project has no such operation (its metrics are functions of argmax alone,
// src/train_segmentation.py:145-159).
//
// The access pattern is WINDOW_BLEND's output side (predict.hip): a thread owns four consecutive pixels of a row and keeps their K
// scores in registers, so per class plane a wave reads 1 KB with one float4 per lane.  HBM-bound on SCORES, which is read exactly once
// whatever is asked for.  Where P is no multiple of 4, or a pointer is not 16-byte aligned, rows start unaligned and the quad is read
// and written element by element (VEC = false), its overhang past the row's end masked per element.
//
// Every sum is an integer: counts, and confidences / negative log-likelihoods quantised to 2^-20 per pixel BEFORE they are added.  A
// workgroup walks CAL_MAX_GRID-strided passes over the quads and counts in LDS - one 64-bit cell {count | correct << 32} and one 64-bit
// cell of quantised confidence per (class, bin), so a cell cannot overflow whatever a workgroup sees (at most 2^22 pixels, checked on the
// host) - and adds its non-zero cells to HIST with one 64-bit global atomic each when it ends.  The per-temperature sums live in one
// 64-bit LDS slot per (temperature, thread), are summed per wave and per workgroup, and reach TOTALS as one atomic per workgroup and
// temperature.  Integer addition commutes: the results are independent of the launch geometry and bit-identical from run to run.
#include "plain.h"

#include <cmath>

namespace s2k {

constexpr int CAL_MAXK = 32, CAL_MAX_BINS = 64, CAL_MAX_TEMPS = 8;
constexpr int CAL_MAX_GRID = 1024;                  // workgroups of one launch: 4 per CU; a workgroup walks passes of NTHREADS quads
constexpr int64_t CAL_MAX_QUADS = 0x7fffffffll;     // N * ceil(P / 4): a workgroup then counts at most 2^22 pixels (32-bit halves of a cell)
constexpr float CAL_ONE = 1048576.0f;               // 2^20: the quantum of the confidence and NLL sums
constexpr float CAL_NLL_MAX = 128.0f;
constexpr int CAL_TAIL = 2 + CAL_MAX_TEMPS;         // LDS words after the cells: skipped, counted, the workgroup's NLL sum per temperature

struct CalP {
    const float* scores;            // [N][K][P]
    const void* labels;             // [N][P] u8 or i64, or null
    const int* lut;                 // [256] or null
    float* conf;                    // [N][P] or null
    void* pred;                     // [N][P] u8 or i64, or null
    unsigned long long* hist;       // [K][bins][3] or null
    unsigned long long* totals;     // [NT][2] or null
    unsigned long long* skipped;    // [1] or null
    float rtemp[CAL_MAX_TEMPS];     // 1 / temps[t], rounded once on the host
    float reject_below;
    int N, K, P, Q;                 // Q = ceil(P / 4) quads per row
    int bins, NT, measure, reject_to, lab8, pred8;
    unsigned exclude;
    int64_t passes;                 // ceil(N * Q / NTHREADS)
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// min(max(nll, 0), 128) * 2^20 to the nearest integer; a NaN counts as 0
__device__ __forceinline__ unsigned nll_quantum(float nll) {
    if (!(nll > 0.0f)) nll = 0.0f;
    if (nll > CAL_NLL_MAX) nll = CAL_NLL_MAX;
    return (unsigned)rintf(nll * CAL_ONE);
}

// KMAX: the compiled class capacity (K <= KMAX; the per-class registers are indexed by unrolled loops only), MODE 1: SCORES are logits.
template <int KMAX, int MODE, bool VEC>
__global__ void __launch_bounds__(NTHREADS) calibration_kernel(const CalP p) {
#pragma clang fp contract(off)      // the operation order of include/s2k.h, one rounding per written operator
    extern __shared__ unsigned long long cal_lds[];
    const int tid = threadIdx.x, K = p.K, P = p.P;
    const int cells = p.hist ? K * p.bins : 0;
    unsigned long long* cellA = cal_lds;                        // count | correct << 32
    unsigned long long* cellB = cal_lds + cells;                // sum of rint(c * 2^20)
    unsigned long long* tail = cellB + cells;                   // [CAL_TAIL]
    unsigned long long* slot = tail + CAL_TAIL;                 // [NT][NTHREADS], only with TOTALS
    const int nt = p.totals ? p.NT : 0;
    for (int i = tid; i < 2 * cells + CAL_TAIL; i += NTHREADS) cal_lds[i] = 0ull;
    for (int t = 0; t < nt; ++t) slot[t * NTHREADS + tid] = 0ull;
    __syncthreads();

    unsigned n_counted = 0u, n_skipped = 0u;
    const int64_t NQ = (int64_t)p.N * p.Q;
    for (int64_t pass = blockIdx.x; pass < p.passes; pass += gridDim.x) {
        const int64_t e = pass * NTHREADS + tid;
        if (e >= NQ) continue;
        const int n = (int)(e / p.Q), x0 = (int)(e - (int64_t)n * p.Q) * 4;
        const int64_t pix = (int64_t)n * P + x0;
        const float* src = p.scores + (int64_t)n * K * P + x0;
        bool in[4];
        float v[KMAX][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) in[q] = VEC || x0 + q < P;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            v[k][0] = v[k][1] = v[k][2] = v[k][3] = 0.0f;
            if (k < K) {
                if (VEC) {
                    const float4 t = *reinterpret_cast<const float4*>(src + (int64_t)k * P);
                    v[k][0] = t.x; v[k][1] = t.y; v[k][2] = t.z; v[k][3] = t.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (in[q]) v[k][q] = src[(int64_t)k * P + q];
                }
            }
        }
        // the label class after the table; -1 = not to be counted (no labels, outside [0, K), excluded)
        int lab[4] = {-1, -1, -1, -1};
        if (p.labels) {
            long long raw[4] = {-1, -1, -1, -1};
            if (p.lab8) {
                const long long* l = static_cast<const long long*>(p.labels) + pix;
                if (VEC) {
                    const longlong2 l0 = *reinterpret_cast<const longlong2*>(l), l1 = *reinterpret_cast<const longlong2*>(l + 2);
                    raw[0] = l0.x; raw[1] = l0.y; raw[2] = l1.x; raw[3] = l1.y;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (in[q]) raw[q] = l[q];
                }
            } else {
                const unsigned char* l = static_cast<const unsigned char*>(p.labels) + pix;
                unsigned char b[4] = {0, 0, 0, 0};
                if (VEC) {
                    const uchar4 t = *reinterpret_cast<const uchar4*>(l);
                    b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (in[q]) b[q] = l[q];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (in[q]) raw[q] = p.lut ? (long long)p.lut[b[q]] : (long long)b[q];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (in[q] && (unsigned long long)raw[q] < (unsigned long long)K && !((p.exclude >> (int)raw[q]) & 1u)) lab[q] = (int)raw[q];
        }

        // ARGMAX on the raw scores: strict >, the first maximum wins (predict.hip)
        int a[4];
        float top[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = 0;
            top[q] = v[0][q];
#pragma unroll
            for (int k = 1; k < KMAX; ++k)
                if (k < K && v[k][q] > top[q]) { top[q] = v[k][q]; a[q] = k; }
        }

        float c[4], cf[4];              // the binning confidence (always the max) and the written one
        bool counted[4];
        if (MODE == 0) {
            unsigned long long sum = 0ull;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                c[q] = top[q];
                float second = -INFINITY, pl = 0.0f;
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) {
                        if (k != a[q] && v[k][q] > second) second = v[k][q];
                        if (k == lab[q]) pl = v[k][q];
                    }
                cf[q] = (p.measure && K > 1) ? c[q] - second : c[q];
                const bool unit = c[q] >= 0.0f && c[q] <= 1.0f;
                counted[q] = lab[q] >= 0 && unit;
                if (lab[q] >= 0 && !unit) ++n_skipped;
                if (counted[q]) {
                    ++n_counted;
                    sum += nll_quantum(pl > 0.0f ? -logf(pl) : CAL_NLL_MAX);      // a score <= 0 or NaN at the label: 128
                }
            }
            if (nt) slot[tid] += sum;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) v[k][q] = v[k][q] - top[q];          // d <= 0, and exactly 0 at the maximum
            float dl[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                dl[q] = 0.0f;
                counted[q] = false;
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K && k == lab[q]) dl[q] = v[k][q];
            }
            const int rounds = nt > 1 ? nt : 1;                     // temperature 0 gives the confidence; the others only their NLL
#pragma unroll 1
            for (int t = 0; t < rounds; ++t) {
                const float r = p.rtemp[t];
                unsigned long long sum = 0ull;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float S = 0.0f, second = -INFINITY;
#pragma unroll
                    for (int k = 0; k < KMAX; ++k)
                        if (k < K) {
                            const float ex = expf(v[k][q] * r);
                            S += ex;
                            if (k != a[q] && ex > second) second = ex;
                        }
                    if (t == 0) {
                        c[q] = 1.0f / S;                             // exp(0) / S
                        cf[q] = (p.measure && K > 1) ? c[q] - second / S : c[q];
                        const bool unit = c[q] >= 0.0f && c[q] <= 1.0f;
                        counted[q] = in[q] && lab[q] >= 0 && unit;
                        if (in[q] && lab[q] >= 0 && !unit) ++n_skipped;
                        if (counted[q]) ++n_counted;
                    }
                    if (counted[q]) sum += nll_quantum(logf(S) - dl[q] * r);      // logsumexp(z) - z[label], the maximum taken out of both
                }
                if (nt) slot[t * NTHREADS + tid] += sum;
            }
        }

        if (p.hist) {
            // neighbouring pixels mostly share a cell: the quad's equal runs are merged before they touch LDS
            int cur = -1;
            unsigned cnt = 0u, cor = 0u, qs = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (counted[q]) {
                    int b = (int)(c[q] * (float)p.bins);
                    if (b > p.bins - 1) b = p.bins - 1;
                    const int cell = a[q] * p.bins + b;
                    if (cell != cur) {
                        if (cur >= 0) {
                            atomicAdd(&cellA[cur], (unsigned long long)cnt | ((unsigned long long)cor << 32));
                            atomicAdd(&cellB[cur], (unsigned long long)qs);
                        }
                        cur = cell; cnt = cor = qs = 0u;
                    }
                    cnt += 1u;
                    cor += lab[q] == a[q] ? 1u : 0u;
                    qs += (unsigned)rintf(c[q] * CAL_ONE);
                }
            if (cur >= 0) {
                atomicAdd(&cellA[cur], (unsigned long long)cnt | ((unsigned long long)cor << 32));
                atomicAdd(&cellB[cur], (unsigned long long)qs);
            }
        }
        if (p.conf) {
            if (VEC) *reinterpret_cast<float4*>(p.conf + pix) = make_float4(cf[0], cf[1], cf[2], cf[3]);
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (in[q]) p.conf[pix + q] = cf[q];
            }
        }
        if (p.pred) {
            int out[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) out[q] = (p.reject_to >= 0 && cf[q] < p.reject_below) ? p.reject_to : a[q];
            if (p.pred8) {
                long long* dst = static_cast<long long*>(p.pred) + pix;
                if (VEC) {
                    reinterpret_cast<longlong2*>(dst)[0] = make_longlong2(out[0], out[1]);
                    reinterpret_cast<longlong2*>(dst)[1] = make_longlong2(out[2], out[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (in[q]) dst[q] = out[q];
                }
            } else {
                unsigned char* dst = static_cast<unsigned char*>(p.pred) + pix;
                if (VEC) *reinterpret_cast<uchar4*>(dst) = make_uchar4((unsigned char)out[0], (unsigned char)out[1], (unsigned char)out[2], (unsigned char)out[3]);
                else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (in[q]) dst[q] = (unsigned char)out[q];
                }
            }
        }
    }

    if (!p.labels) return;                                          // kernel-uniform: nothing was counted
    {
        const unsigned long long sk = wave_sum_u64(n_skipped), ct = wave_sum_u64(n_counted);
        if ((tid & (WAVE - 1)) == 0) {
            if (sk) atomicAdd(&tail[0], sk);
            if (ct) atomicAdd(&tail[1], ct);
        }
        for (int t = 0; t < nt; ++t) {
            const unsigned long long s = wave_sum_u64(slot[t * NTHREADS + tid]);
            if ((tid & (WAVE - 1)) == 0 && s) atomicAdd(&tail[2 + t], s);
        }
    }
    __syncthreads();
    for (int i = tid; i < cells; i += NTHREADS) {
        const unsigned long long A = cellA[i];
        if (A) {
            atomicAdd(p.hist + 3 * i, A & 0xffffffffull);
            if (A >> 32) atomicAdd(p.hist + 3 * i + 1, A >> 32);
            if (cellB[i]) atomicAdd(p.hist + 3 * i + 2, cellB[i]);
        }
    }
    if (tid == 0 && p.skipped && tail[0]) atomicAdd(p.skipped, tail[0]);
    if (tid < nt && tail[1]) {
        atomicAdd(p.totals + 2 * tid, tail[1]);
        if (tail[2 + tid]) atomicAdd(p.totals + 2 * tid + 1, tail[2 + tid]);
    }
}

// ---- host side: every argument checked and the kernel's parameters derived, in plain host code without a HIP call ----------------------
static int calibration_params(const float* scores, int mode, const void* labels, int label_bytes, const int* label_lut, int N, int K, int P,
                              unsigned exclude, const float* temps, int n_temps, int bins, int measure, float reject_below, int reject_to,
                              float* conf, void* pred, int pred_bytes, unsigned long long* hist, unsigned long long* totals,
                              unsigned long long* skipped, CalP& p) {
    const char* who = "calibration";
    if (!scores) { set_error("%s: null pointer (scores is required)", who); return S2K_EFAULT; }
    if (mode != 0 && mode != 1) { set_error("%s: mode = %d (0 probabilities, 1 logits)", who, mode); return S2K_EINVAL; }
    if (measure != 0 && measure != 1) { set_error("%s: measure = %d (0 max, 1 margin)", who, measure); return S2K_EINVAL; }
    if (K < 1 || K > CAL_MAXK) { set_error("%s: K = %d outside 1..%d", who, K, CAL_MAXK); return S2K_EINVAL; }
    if (bins < 1 || bins > CAL_MAX_BINS) { set_error("%s: bins = %d outside 1..%d", who, bins, CAL_MAX_BINS); return S2K_EINVAL; }
    if (n_temps < 1 || n_temps > CAL_MAX_TEMPS) { set_error("%s: n_temps = %d outside 1..%d", who, n_temps, CAL_MAX_TEMPS); return S2K_EINVAL; }
    if (!temps) { set_error("%s: temps is required (host memory, n_temps values)", who); return S2K_EINVAL; }
    for (int t = 0; t < n_temps; ++t) {
        const float r = 1.0f / temps[t];
        if (!std::isfinite(temps[t]) || !(temps[t] > 0.0f) || !std::isfinite(r) || !(r > 0.0f)) {
            set_error("%s: temps[%d] = %g must be finite and above 0 (and so must its reciprocal)", who, t, (double)temps[t]);
            return S2K_EINVAL;
        }
    }
    if (mode == 0 && (n_temps != 1 || temps[0] != 1.0f)) { set_error("%s: mode 0 takes probabilities as given: temps must be {1}", who); return S2K_EINVAL; }
    if (labels && label_bytes != 1 && label_bytes != 8) { set_error("%s: the element width of labels must be 1 (uint8) or 8 (int64) bytes, got %d", who, label_bytes); return S2K_EINVAL; }
    if (pred && pred_bytes != 1 && pred_bytes != 8) { set_error("%s: the element width of pred must be 1 (uint8) or 8 (int64) bytes, got %d", who, pred_bytes); return S2K_EINVAL; }
    if (label_lut && (!labels || label_bytes != 1)) { set_error("%s: label_lut reads 1-byte labels only", who); return S2K_EINVAL; }
    const unsigned all = K == 32 ? 0xffffffffu : (1u << K) - 1u;
    if (exclude & ~all) { set_error("%s: exclude names a class at or above K = %d", who, K); return S2K_EINVAL; }
    if (reject_to < -1 || reject_to >= K) { set_error("%s: reject_to = %d outside -1..%d", who, reject_to, K - 1); return S2K_EINVAL; }
    if ((hist || totals) && !labels) { set_error("%s: hist and totals need labels", who); return S2K_EINVAL; }
    if (!conf && !pred && !hist && !totals && !skipped) { set_error("%s: no output (conf, pred, hist, totals and skipped are all null)", who); return S2K_EINVAL; }
    if (N < 1 || P < 1) { set_error("%s: bad dims (N and P must be positive)", who); return S2K_EINVAL; }
    const int Q = (int)(((int64_t)P + 3) / 4);
    if ((int64_t)N * Q > CAL_MAX_QUADS) { set_error("%s: bad dims (N * ceil(P / 4) must stay below 2^31 pixel quads)", who); return S2K_EINVAL; }
    p = CalP{};
    p.scores = scores; p.labels = labels; p.lut = label_lut; p.conf = conf; p.pred = pred; p.hist = hist; p.totals = totals; p.skipped = skipped;
    for (int t = 0; t < n_temps; ++t) p.rtemp[t] = 1.0f / temps[t];
    p.reject_below = reject_below;
    p.N = N; p.K = K; p.P = P; p.Q = Q; p.bins = bins; p.NT = n_temps; p.measure = measure; p.reject_to = reject_to;
    p.lab8 = label_bytes == 8; p.pred8 = pred_bytes == 8; p.exclude = exclude;
    p.passes = cdiv64((int64_t)N * Q, NTHREADS);
    return S2K_OK;
}

int check_calibration(const float* scores, int mode, const void* labels, int label_bytes, const int* label_lut, int N, int K, int P,
                      unsigned exclude, const float* temps, int n_temps, int bins, int measure, float reject_below, int reject_to, float* conf,
                      void* pred, int pred_bytes, unsigned long long* hist, unsigned long long* totals, unsigned long long* skipped) {
    CalP p;
    return calibration_params(scores, mode, labels, label_bytes, label_lut, N, K, P, exclude, temps, n_temps, bins, measure, reject_below,
                              reject_to, conf, pred, pred_bytes, hist, totals, skipped, p);
}

template <int KMAX>
static void launch_cal(const CalP& p, int mode, bool vec, unsigned grid, size_t lds, hipStream_t st) {
    if (mode) {
        if (vec) hipLaunchKernelGGL((calibration_kernel<KMAX, 1, true>), dim3(grid), dim3(NTHREADS), lds, st, p);
        else hipLaunchKernelGGL((calibration_kernel<KMAX, 1, false>), dim3(grid), dim3(NTHREADS), lds, st, p);
    } else {
        if (vec) hipLaunchKernelGGL((calibration_kernel<KMAX, 0, true>), dim3(grid), dim3(NTHREADS), lds, st, p);
        else hipLaunchKernelGGL((calibration_kernel<KMAX, 0, false>), dim3(grid), dim3(NTHREADS), lds, st, p);
    }
}

int launch_calibration(const float* scores, int mode, const void* labels, int label_bytes, const int* label_lut, int N, int K, int P,
                       unsigned exclude, const float* temps, int n_temps, int bins, int measure, float reject_below, int reject_to, float* conf,
                       void* pred, int pred_bytes, unsigned long long* hist, unsigned long long* totals, unsigned long long* skipped,
                       hipStream_t st) {
    CalP p;
    const int rc = calibration_params(scores, mode, labels, label_bytes, label_lut, N, K, P, exclude, temps, n_temps, bins, measure, reject_below,
                                      reject_to, conf, pred, pred_bytes, hist, totals, skipped, p);
    if (rc != S2K_OK) return rc;
    // quad loads and stores: every row of every tensor then starts on 16 bytes (4 for one-byte elements)
    const auto aligned = [](const void* q) { return reinterpret_cast<uintptr_t>(q) % 16 == 0; };
    const bool vec = P % 4 == 0 && aligned(scores) && aligned(labels) && aligned(conf) && aligned(pred);
    // at most 48 KB: 2 * 32 * 64 cells, the tail, 8 * 256 slots, 8 bytes each
    const size_t lds = ((size_t)(hist ? 2 * K * bins : 0) + CAL_TAIL + (size_t)(totals ? n_temps : 0) * NTHREADS) * sizeof(unsigned long long);
    const unsigned grid = (unsigned)(p.passes < CAL_MAX_GRID ? p.passes : CAL_MAX_GRID);
    if (K <= 2) launch_cal<2>(p, mode, vec, grid, lds, st);
    else if (K <= 4) launch_cal<4>(p, mode, vec, grid, lds, st);
    else if (K <= 8) launch_cal<8>(p, mode, vec, grid, lds, st);
    else if (K <= 16) launch_cal<16>(p, mode, vec, grid, lds, st);
    else launch_cal<32>(p, mode, vec, grid, lds, st);
    return S2K_OK;
}

}  // namespace s2k
