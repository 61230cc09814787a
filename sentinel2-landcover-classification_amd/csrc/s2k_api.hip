// C-ABI entry points (include/s2k.h) and the native stage executor.
//
// The executor is the "runtime" of this path: a plain loop over POD stage records that enqueues
// hand-written kernels on the caller's HIP stream.  No device allocation, no synchronisation; the only
// mutable global is a mutex-guarded pool of per-device side streams leased per call — so a whole
// forward or backward is graph-capturable, costs one FFI call, and may be issued from several host
// threads / streams / devices at once.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include <stdlib.h>

#include "common.h"
#include "plain.h"

namespace s2k {

static thread_local char g_err[512] = "";
thread_local int g_s2k_variant = 0;

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int launch_conv(const S2kOp&, const Ctx&);
int launch_wgrad(const S2kOp&, const Ctx&);
int launch_dwconv_fwd(const S2kOp&, const Ctx&);
int launch_dwconv_dgrad(const S2kOp&, const Ctx&);
int launch_dwconv_wgrad(const S2kOp&, const Ctx&);
int launch_axpy(const S2kOp&, const Ctx&);
int launch_weight_pack(const S2kOp&, const Ctx&);
int launch_wgrad_finalize(const S2kOp&, const Ctx&);
int launch_bn_finalize(const S2kOp&, const Ctx&);
int launch_se_pool(const S2kOp&, const Ctx&);
int launch_se_fc(const S2kOp&, const Ctx&);
int launch_se_fc_bwd(const S2kOp&, const Ctx&);
int launch_se_bwd_reduce(const S2kOp&, const Ctx&);
int launch_bn_bwd_reduce(const S2kOp&, const Ctx&);
int launch_bn_bwd_finalize(const S2kOp&, const Ctx&);
int launch_bn_bwd_apply(const S2kOp&, const Ctx&);
int launch_bn_residual(const S2kOp&, const Ctx&);
int launch_channel_sum(const S2kOp&, const Ctx&);
int launch_loss_fwd(const S2kOp&, const Ctx&);
int launch_loss_bwd(const S2kOp&, const Ctx&);
int launch_argmax(const S2kOp&, const Ctx&);
int launch_chan_ln_fwd(const S2kOp&, const Ctx&);
int launch_chan_ln_bwd(const S2kOp&, const Ctx&);
int launch_act_bwd(const S2kOp&, const Ctx&);
int launch_act_fwd(const S2kOp&, const Ctx&);
int launch_attn_fwd(const S2kOp&, const Ctx&);
int launch_attn_bwd(const S2kOp&, const Ctx&);
int launch_mae_mask_index(const S2kOp&, const Ctx&);
int launch_token_gather(const S2kOp&, const Ctx&);
int launch_token_scatter(const S2kOp&, const Ctx&);
int launch_patchify(const S2kOp&, const Ctx&);
int launch_mae_loss_fwd(const S2kOp&, const Ctx&);
int launch_mae_loss_bwd(const S2kOp&, const Ctx&);
int launch_transpose_cl(const S2kOp&, const Ctx&);
int launch_drop_gate(const S2kOp&, const Ctx&);
int launch_confusion(const S2kOp&, const Ctx&);
int launch_tile_prep(const S2kOp&, const Ctx&);
int launch_se_bn_sums(const S2kOp&, const Ctx&);
int launch_se_bn_combine(const S2kOp&, const Ctx&);
int launch_space_to_depth(const S2kOp&, const Ctx&);
int launch_se_fc_wgrad(const S2kOp&, const Ctx&);
int launch_ids_to_dec_idx(const S2kOp&, const Ctx&);
int launch_upsample_zero(const S2kOp&, const Ctx&);
int launch_im2col(const S2kOp&, const Ctx&);
int launch_tile_label_hist(const S2kOp&, const Ctx&);
int launch_tile_moments(const S2kOp&, const Ctx&);
int launch_window_blend(const S2kOp&, const Ctx&);
int launch_seg_stats(const S2kOp&, const Ctx&);
int launch_seg_hist(const S2kOp&, const Ctx&);
int launch_grad_clip(const S2kOp&, const Ctx&);
int launch_tile_radix_hist(const S2kOp&, const Ctx&);
int launch_tile_rank_pick(const S2kOp&, const Ctx&);
int launch_tile_quicklook(const S2kOp&, const Ctx&);
int launch_class_overlay(const S2kOp&, const Ctx&);
int launch_dw_bwd_chain(const S2kOp*, const Ctx&);

static int launch_memset(const S2kOp& op, const Ctx& c) {
    const int64_t ref = op.t[S2K_MEMSET_T_DST];
    const int64_t bytes = op.n[S2K_MEMSET_N_BYTES];
    if (ref < 0 || bytes <= 0) { set_error("memset: bad args"); return S2K_EINVAL; }
    Refs r(c);
    char* dst = r.ptr<char>(ref);
    if (r.absent) { set_error("memset: null base %d", Refs::base_of(ref)); return S2K_EFAULT; }
    if (hipMemsetAsync(dst, 0, (size_t)bytes, c.stream) != hipSuccess) { set_error("memset: hipMemsetAsync failed"); return S2K_EHIP; }
    return S2K_OK;
}

static const char* const kNames[S2K_N_KINDS + 1] = {
    nullptr,
    "MEMSET", "AXPY", "WEIGHT_PACK", "CONV", "WGRAD", "WGRAD_FINALIZE", "DWCONV_FWD", "DWCONV_DGRAD", "DWCONV_WGRAD",
    "BN_FINALIZE", "SE_POOL", "SE_FC", "SE_FC_BWD", "SE_BWD_REDUCE", "BN_BWD_REDUCE", "BN_BWD_FINALIZE", "BN_BWD_APPLY",
    "BN_RESIDUAL", "CHANNEL_SUM", "LOSS_FWD", "LOSS_BWD", "ARGMAX", "CHAN_LN_FWD", "CHAN_LN_BWD", "ACT_BWD", "ACT_FWD",
    "ATTN_FWD", "ATTN_BWD", "MAE_MASK_INDEX", "IDS_TO_DEC_IDX", "TOKEN_GATHER", "TOKEN_SCATTER", "PATCHIFY", "MAE_LOSS_FWD",
    "MAE_LOSS_BWD", "TRANSPOSE_CL", "CONFUSION", "DROP_GATE", "TILE_PREP", "SE_BN_SUMS", "SE_BN_COMBINE", "SPACE_TO_DEPTH",
    "UPSAMPLE_ZERO", "SE_FC_WGRAD", "IM2COL", "TILE_LABEL_HIST", "TILE_MOMENTS", "WINDOW_BLEND",
    "SEG_STATS", "SEG_HIST", "GRAD_CLIP", "TILE_RADIX_HIST", "TILE_RANK_PICK", "TILE_QUICKLOOK", "CLASS_OVERLAY"};

static int dispatch(const S2kOp& op, const Ctx& c) {
    switch (op.kind) {
        case S2K_OP_MEMSET: return launch_memset(op, c);
        case S2K_OP_AXPY: return launch_axpy(op, c);
        case S2K_OP_WEIGHT_PACK: return launch_weight_pack(op, c);
        case S2K_OP_CONV: return launch_conv(op, c);
        case S2K_OP_WGRAD: return launch_wgrad(op, c);
        case S2K_OP_WGRAD_FINALIZE: return launch_wgrad_finalize(op, c);
        case S2K_OP_DWCONV_FWD: return launch_dwconv_fwd(op, c);
        case S2K_OP_DWCONV_DGRAD: return launch_dwconv_dgrad(op, c);
        case S2K_OP_DWCONV_WGRAD: return launch_dwconv_wgrad(op, c);
        case S2K_OP_BN_FINALIZE: {
#ifdef S2K_TUNING
            static const int skip = tune_int("S2K_EXP_SKIP_BN_FINALIZE", 0);   // timing experiment only: stale scale / shift
            if (skip) return S2K_OK;
#endif
            return launch_bn_finalize(op, c);
        }
        case S2K_OP_SE_POOL: return launch_se_pool(op, c);
        case S2K_OP_SE_FC: return launch_se_fc(op, c);
        case S2K_OP_SE_FC_BWD: return launch_se_fc_bwd(op, c);
        case S2K_OP_SE_BWD_REDUCE: return launch_se_bwd_reduce(op, c);
        case S2K_OP_BN_BWD_REDUCE: return launch_bn_bwd_reduce(op, c);
        case S2K_OP_BN_BWD_FINALIZE: return launch_bn_bwd_finalize(op, c);
        case S2K_OP_BN_BWD_APPLY: return launch_bn_bwd_apply(op, c);
        case S2K_OP_BN_RESIDUAL: return launch_bn_residual(op, c);
        case S2K_OP_CHANNEL_SUM: return launch_channel_sum(op, c);
        case S2K_OP_LOSS_FWD: return launch_loss_fwd(op, c);
        case S2K_OP_LOSS_BWD: return launch_loss_bwd(op, c);
        case S2K_OP_ARGMAX: return launch_argmax(op, c);
        case S2K_OP_CHAN_LN_FWD: return launch_chan_ln_fwd(op, c);
        case S2K_OP_CHAN_LN_BWD: return launch_chan_ln_bwd(op, c);
        case S2K_OP_ACT_BWD: return launch_act_bwd(op, c);
        case S2K_OP_ACT_FWD: return launch_act_fwd(op, c);
        case S2K_OP_ATTN_FWD: return launch_attn_fwd(op, c);
        case S2K_OP_ATTN_BWD: return launch_attn_bwd(op, c);
        case S2K_OP_MAE_MASK_INDEX: return launch_mae_mask_index(op, c);
        case S2K_OP_TOKEN_GATHER: return launch_token_gather(op, c);
        case S2K_OP_TOKEN_SCATTER: return launch_token_scatter(op, c);
        case S2K_OP_PATCHIFY: return launch_patchify(op, c);
        case S2K_OP_MAE_LOSS_FWD: return launch_mae_loss_fwd(op, c);
        case S2K_OP_MAE_LOSS_BWD: return launch_mae_loss_bwd(op, c);
        case S2K_OP_TRANSPOSE_CL: return launch_transpose_cl(op, c);
        case S2K_OP_DROP_GATE: return launch_drop_gate(op, c);
        case S2K_OP_CONFUSION: return launch_confusion(op, c);
        case S2K_OP_TILE_PREP: return launch_tile_prep(op, c);
        case S2K_OP_SE_BN_SUMS: return launch_se_bn_sums(op, c);
        case S2K_OP_SE_BN_COMBINE: return launch_se_bn_combine(op, c);
        case S2K_OP_SPACE_TO_DEPTH: return launch_space_to_depth(op, c);
        case S2K_OP_SE_FC_WGRAD: return launch_se_fc_wgrad(op, c);
        case S2K_OP_IDS_TO_DEC_IDX: return launch_ids_to_dec_idx(op, c);
        case S2K_OP_UPSAMPLE_ZERO: return launch_upsample_zero(op, c);
        case S2K_OP_IM2COL: return launch_im2col(op, c);
        case S2K_OP_TILE_LABEL_HIST: return launch_tile_label_hist(op, c);
        case S2K_OP_TILE_MOMENTS: return launch_tile_moments(op, c);
        case S2K_OP_WINDOW_BLEND: return launch_window_blend(op, c);
        case S2K_OP_SEG_STATS: return launch_seg_stats(op, c);
        case S2K_OP_SEG_HIST: return launch_seg_hist(op, c);
        case S2K_OP_GRAD_CLIP: return launch_grad_clip(op, c);
        case S2K_OP_TILE_RADIX_HIST: return launch_tile_radix_hist(op, c);
        case S2K_OP_TILE_RANK_PICK: return launch_tile_rank_pick(op, c);
        case S2K_OP_TILE_QUICKLOOK: return launch_tile_quicklook(op, c);
        case S2K_OP_CLASS_OVERLAY: return launch_class_overlay(op, c);
        default: set_error("unknown stage kind %d", op.kind); return S2K_ENOSYS;
    }
}

static int check_launch(int rc, const S2kOp& op, int index) {
    if (rc != S2K_OK) {
        char tmp[400];
        snprintf(tmp, sizeof(tmp), "%s", g_err);
        set_error("op %d (%s): %s", index, (op.kind > 0 && op.kind <= S2K_N_KINDS) ? kNames[op.kind] : "?", tmp);
        return rc;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("op %d (%s): HIP launch error: %s", index, (op.kind > 0 && op.kind <= S2K_N_KINDS) ? kNames[op.kind] : "?",
                  hipGetErrorString(e));
        return S2K_EHIP;
    }
    return S2K_OK;
}

}  // namespace s2k

using namespace s2k;

extern "C" {

int s2k_abi_version(void) { return S2K_ABI_VERSION; }
size_t s2k_op_size(void) { return sizeof(S2kOp); }
const char* s2k_last_error(void) { return g_err; }
const char* s2k_kind_name(int kind) { return (kind > 0 && kind <= S2K_N_KINDS) ? kNames[kind] : nullptr; }

// Side stream for stages flagged S2K_FLAG_SIDE (weight gradients: nothing downstream in the backward chain reads them
// until the bucket's WGRAD_FINALIZE): they run concurrently with the main chain, so an MFMA-bound wgrad overlaps the
// HBM-bound BatchNorm / depthwise stages of the layers below.  Fork = event on the caller's stream the side stream waits
// for (re-armed whenever main-stream work was issued since the last fork); join = the reverse, in front of every stage
// flagged S2K_FLAG_JOIN and at the end of the call, so on return all work is ordered on the caller's stream again.
//
// Side queues are pooled PER DEVICE and leased for the duration of one s2k_program_run: two host threads, two caller
// streams or two devices in one process never share a stream or an event pair (the pool, guarded by a mutex, is the only
// mutable global of the library; a queue goes back to the pool when the call returns — by then every event it recorded has
// been waited for by the caller's stream, so the next lessee may re-record them).
struct SideQueue {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
constexpr int kMaxDevices = 64;
static std::mutex g_pool_mu;
static std::vector<SideQueue*> g_pool[kMaxDevices];

static bool side_streams_enabled() {
    static const bool on = tune_int("S2K_NO_SIDE_STREAM", 0) == 0;
    return on;
}

static SideQueue* lease_side_queue(int device) {
    if (device < 0 || device >= kMaxDevices || !side_streams_enabled()) return nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (!g_pool[device].empty()) {
            SideQueue* q = g_pool[device].back();
            g_pool[device].pop_back();
            return q;
        }
    }
    SideQueue* q = new SideQueue;   // created with `device` current (the caller holds the device guard)
    if (hipStreamCreateWithFlags(&q->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&q->fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&q->join, hipEventDisableTiming) != hipSuccess) {
        if (q->fork) (void)hipEventDestroy(q->fork);
        if (q->stream) (void)hipStreamDestroy(q->stream);
        delete q;
        (void)hipGetLastError();
        return nullptr;                   // no side stream: everything runs on the caller's stream (still correct)
    }
    return q;
}

static void release_side_queue(int device, SideQueue* q) {
    if (!q) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool[device].push_back(q);
}

// Makes the device that owns `stream` current for the duration of a call (kernel launches, event / stream creation and
// hipFuncSetAttribute all act on the current device) and restores the caller's device afterwards.
struct DeviceGuard {
    int prev = -1, dev = -1;
    bool switched = false;
    explicit DeviceGuard(hipStream_t st) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        dev = prev;
        int sd = -1;
        if (st != nullptr && hipStreamGetDevice(st, &sd) == hipSuccess && sd >= 0) dev = sd;
        (void)hipGetLastError();
        if (dev != prev && dev >= 0) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched && prev >= 0) (void)hipSetDevice(prev);
    }
};

// A depthwise backward chain (plan/opdefs.py FLAG_CHAIN) starts at ops[i]: BN_BWD_APPLY (depthwise BatchNorm, recomputing form) ->
// DWCONV_WGRAD -> DWCONV_DGRAD (SiLU, statistics) -> BN_BWD_APPLY (expand BatchNorm) over one expanded tensor.  The flag is a
// permission, not an order: the pattern and the shapes are checked again here, and whatever does not fit runs record by record
// as if the flag were not there.  Returns the number of records consumed: 4 (one launch of dw_bwd_chain_kernel on c.stream, *rc
// its status) or 0 (declined: nothing was launched).
static int try_dw_chain(const S2kOp* ops, int i, int end, const Ctx& c, int* rc) {
    if (!(ops[i].flags & S2K_FLAG_CHAIN) || i + 3 >= end) return 0;
    const S2kOp &a1 = ops[i], &wg = ops[i + 1], &dg = ops[i + 2], &a2 = ops[i + 3];
    if (a1.kind != S2K_OP_BN_BWD_APPLY || wg.kind != S2K_OP_DWCONV_WGRAD || dg.kind != S2K_OP_DWCONV_DGRAD || a2.kind != S2K_OP_BN_BWD_APPLY) return 0;
    if ((a1.flags | wg.flags | dg.flags | a2.flags) & (S2K_FLAG_BF16 | S2K_FLAG_SPLIT)) return 0;
    const int64_t dy = a1.t[S2K_BN_BWD_APPLY_T_DY], x = dg.t[S2K_DWCONV_DGRAD_T_XRAW], g = dg.t[S2K_DWCONV_DGRAD_T_G];
    // first APPLY: SiLU, g' recomputed from the SE backward's plane sums, train mode, f32 in place
    if (dy < 0 || a1.t[S2K_BN_BWD_APPLY_T_GP] != dy || a1.t[S2K_BN_BWD_APPLY_T_COEF] >= 0 || a1.t[S2K_BN_BWD_APPLY_T_PS] < 0 ||
        a1.t[S2K_BN_BWD_APPLY_T_MULBC] < 0 || a1.t[S2K_BN_BWD_APPLY_T_ADDBC] < 0 || a1.d[S2K_BN_BWD_APPLY_D_ACT] != S2K_PRO_SILU ||
        a1.d[S2K_BN_BWD_APPLY_D_EVAL] || a1.d[S2K_BN_BWD_APPLY_D_OUT_BF16] || a1.n[S2K_BN_BWD_APPLY_N_COUNT] <= 0) return 0;
    // the two depthwise gradients read that dY and the same expanded activation
    if (wg.t[S2K_DWCONV_WGRAD_T_DY] != dy || dg.t[S2K_DWCONV_DGRAD_T_DY] != dy || x < 0 || wg.t[S2K_DWCONV_WGRAD_T_X] != x ||
        dg.t[S2K_DWCONV_DGRAD_T_BNV] < 0 || wg.t[S2K_DWCONV_WGRAD_T_BNV] != dg.t[S2K_DWCONV_DGRAD_T_BNV] || g < 0 || g == dy || g == x ||
        dg.t[S2K_DWCONV_DGRAD_T_STATS2] < 0) return 0;
    for (int k = 0; k <= 10; ++k)          // B, C, H, W, K, STRIDE, PAD_T, PAD_L, HO, WO, PRO: the same slots in both records
        if (wg.d[k] != dg.d[k]) return 0;
    const int B = dg.d[0], C = dg.d[1], H = dg.d[2], W = dg.d[3], K = dg.d[4];
    if (B <= 0 || C <= 0 || H != W || (W != 8 && W != 16) || (K != 3 && K != 5) || dg.d[5] != 1 || dg.d[6] != (K - 1) / 2 || dg.d[7] != (K - 1) / 2 ||
        dg.d[8] != H || dg.d[9] != W || dg.d[10] != S2K_PRO_SILU || dg.d[S2K_DWCONV_DGRAD_D_BETA] != 0) return 0;
    if ((int64_t)B * C * H * W * 4 >= 0x7ffffff0ll) return 0;
    // second APPLY: the plain fused form, in place on the data gradient, with the sums the data gradient would have written
    if (a2.t[S2K_BN_BWD_APPLY_T_GP] != g || a2.t[S2K_BN_BWD_APPLY_T_DY] != g || a2.t[S2K_BN_BWD_APPLY_T_Y] != x ||
        a2.t[S2K_BN_BWD_APPLY_T_BNV] != dg.t[S2K_DWCONV_DGRAD_T_BNV] || a2.t[S2K_BN_BWD_APPLY_T_STATS2] != dg.t[S2K_DWCONV_DGRAD_T_STATS2] ||
        a2.t[S2K_BN_BWD_APPLY_T_COEF] >= 0 || a2.t[S2K_BN_BWD_APPLY_T_PS] >= 0 || a2.t[S2K_BN_BWD_APPLY_T_MULBC] >= 0 ||
        a2.t[S2K_BN_BWD_APPLY_T_ADDBC] >= 0 || a2.d[S2K_BN_BWD_APPLY_D_ACT] != S2K_PRO_NONE || a2.d[S2K_BN_BWD_APPLY_D_EVAL] ||
        a2.d[S2K_BN_BWD_APPLY_D_OUT_BF16] || a2.n[S2K_BN_BWD_APPLY_N_COUNT] <= 0) return 0;
    const int HW = H * W;
    if (a1.d[S2K_BN_BWD_APPLY_D_B] != B || a1.d[S2K_BN_BWD_APPLY_D_C] != C || a1.d[S2K_BN_BWD_APPLY_D_HW] != HW ||
        a2.d[S2K_BN_BWD_APPLY_D_B] != B || a2.d[S2K_BN_BWD_APPLY_D_C] != C || a2.d[S2K_BN_BWD_APPLY_D_HW] != HW) return 0;
    *rc = check_launch(launch_dw_bwd_chain(&ops[i], c), ops[i], i);
    return 4;
}

// Issues ops[i] on c.stream: the depthwise backward chain that starts there as one launch, else the record's own stage.  *rc is the
// status; returns the number of records consumed (4 or 1).  g_s2k_variant then names the kernel family the launcher picked.
static int issue_step(const S2kOp* ops, int i, int end, const Ctx& c, int* rc) {
    g_s2k_variant = 0;
    const int used = try_dw_chain(ops, i, end, c, rc);
    if (used) return used;
    *rc = check_launch(dispatch(ops[i], c), ops[i], i);
    return 1;
}

int s2k_program_run(const S2kOp* ops, int begin, int end, void* const* bases, int n_bases, void* stream) {
    if (!ops || !bases || begin < 0 || end < begin) { set_error("program_run: bad arguments"); return S2K_EINVAL; }
    hipStream_t main_st = static_cast<hipStream_t>(stream);
    DeviceGuard guard(main_st);
    Ctx c{bases, n_bases, main_st};
    bool any_side = false;
    for (int i = begin; i < end && !any_side; ++i) any_side = (ops[i].flags & S2K_FLAG_SIDE) != 0;
    SideQueue* sq = any_side ? lease_side_queue(guard.dev) : nullptr;
    bool side_busy = false;      // side work issued and not yet joined
    bool main_dirty = true;      // main-stream work issued since the last fork
    auto join = [&]() {
        if (!side_busy) return;
        (void)hipEventRecord(sq->join, sq->stream);
        (void)hipStreamWaitEvent(main_st, sq->join, 0);
        side_busy = false;
    };
    int rc = S2K_OK;
    for (int i = begin; i < end; ++i) {
        const S2kOp& op = ops[i];
        // a join asked for by any record of a chain is honoured in front of it (merely early if the chain is then declined)
        const bool chain = (op.flags & S2K_FLAG_CHAIN) && i + 3 < end;
        if (chain && ((op.flags | ops[i + 1].flags | ops[i + 2].flags | ops[i + 3].flags) & S2K_FLAG_JOIN)) join();
        if ((op.flags & S2K_FLAG_SIDE) && sq && !chain) {     // (a chain runs on the caller's stream)
            if (main_dirty) {
                (void)hipEventRecord(sq->fork, main_st);
                (void)hipStreamWaitEvent(sq->stream, sq->fork, 0);
                main_dirty = false;
            }
            Ctx cs{bases, n_bases, sq->stream};
            i += issue_step(ops, i, end, cs, &rc) - 1;
            side_busy = true;
        } else {
            if (op.flags & S2K_FLAG_JOIN) join();
            i += issue_step(ops, i, end, c, &rc) - 1;    // a chain consumes its DWCONV_WGRAD: that record is not issued to the side stream
            main_dirty = true;
        }
        if (rc != S2K_OK) break;
    }
    join();
    release_side_queue(guard.dev, sq);
    return rc;
}

int s2k_op_launch(const S2kOp* op, void* const* bases, int n_bases, void* stream) {
    if (!op || !bases) { set_error("op_launch: bad arguments"); return S2K_EINVAL; }
    DeviceGuard guard(static_cast<hipStream_t>(stream));
    Ctx c{bases, n_bases, static_cast<hipStream_t>(stream)};
    return check_launch(dispatch(*op, c), *op, 0);
}

static int profile_impl(const S2kOp* ops, int begin, int end, void* const* bases, int n_bases, void* stream, float* ms_by_kind,
                        int* launches_by_kind, float* ms_per_op, int* variant_per_op);

int s2k_program_profile(const S2kOp* ops, int begin, int end, void* const* bases, int n_bases, void* stream, float* ms_by_kind,
                        int* launches_by_kind) {
    return profile_impl(ops, begin, end, bases, n_bases, stream, ms_by_kind, launches_by_kind, nullptr, nullptr);
}

int s2k_program_profile_ops(const S2kOp* ops, int begin, int end, void* const* bases, int n_bases, void* stream,
                            float* ms_per_op) {
    float ms[S2K_N_KINDS + 1];
    int cnt[S2K_N_KINDS + 1];
    return profile_impl(ops, begin, end, bases, n_bases, stream, ms, cnt, ms_per_op, nullptr);
}

int s2k_program_profile_variants(const S2kOp* ops, int begin, int end, void* const* bases, int n_bases, void* stream,
                                 float* ms_per_op, int* variant_per_op) {
    float ms[S2K_N_KINDS + 1];
    int cnt[S2K_N_KINDS + 1];
    if (!ms_per_op || !variant_per_op) { set_error("program_profile_variants: bad arguments"); return S2K_EINVAL; }
    return profile_impl(ops, begin, end, bases, n_bases, stream, ms, cnt, ms_per_op, variant_per_op);
}

static int profile_impl(const S2kOp* ops, int begin, int end, void* const* bases, int n_bases, void* stream, float* ms_by_kind,
                        int* launches_by_kind, float* ms_per_op, int* variant_per_op) {
    if (!ops || !bases || !ms_by_kind || !launches_by_kind || begin < 0 || end < begin) {
        set_error("program_profile: bad arguments");
        return S2K_EINVAL;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    DeviceGuard guard(st);
    Ctx c{bases, n_bases, st};
    const int n = end - begin;
    hipEvent_t* ev = new hipEvent_t[n + 1];
    for (int i = 0; i <= n; ++i) hipEventCreate(&ev[i]);
    int rc = S2K_OK;
    hipEventRecord(ev[0], st);
    int done = 0;
    std::vector<char> fused(n, 0);      // records consumed by the launch of an earlier one: 0 ms, no launch of their own
    for (int i = 0; i < n; ++i) {
        const int used = issue_step(ops, begin + i, end, c, &rc);
        if (rc != S2K_OK) break;
        for (int k = 0; k < used; ++k) {
            if (variant_per_op) variant_per_op[i + k] = g_s2k_variant;
            hipEventRecord(ev[i + k + 1], st);
            if (k) fused[i + k] = 1;
        }
        i += used - 1;
        done = i + 1;
    }
    hipStreamSynchronize(st);
    if (rc == S2K_OK) {
        for (int k = 0; k <= S2K_N_KINDS; ++k) { ms_by_kind[k] = 0.0f; launches_by_kind[k] = 0; }
        for (int i = 0; i < done; ++i) {
            float ms = 0.0f;
            if (!fused[i]) hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            const int k = ops[begin + i].kind;
            if (ms_per_op) ms_per_op[i] = ms;
            if (k > 0 && k <= S2K_N_KINDS && !fused[i]) { ms_by_kind[k] += ms; launches_by_kind[k] += 1; }
        }
    }
    for (int i = 0; i <= n; ++i) hipEventDestroy(ev[i]);
    delete[] ev;
    return rc;
}

}  // extern "C"

namespace {

template <typename T>
struct as_given { using type = T; };

// Every plain C-ABI function (csrc/plain.h) is this sequence: validate all arguments with no HIP call before it, make the device that
// owns the stream current, launch, report a launch error as "<name>: <hip error>".  A... is deduced from check's signature alone.
template <typename... A>
int guarded_call(const char* name, void* stream, int (*check)(A...), int (*launch)(A..., hipStream_t), typename as_given<A>::type... args) {
    const int bad = check(args...);
    if (bad != S2K_OK) return bad;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DeviceGuard guard(st);
    const int rc = launch(args..., st);
    if (rc != S2K_OK) return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s: %s", name, hipGetErrorString(e)); return S2K_EHIP; }
    return S2K_OK;
}

}  // namespace

extern "C" {

int s2k_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int step, void* stream) {
    return guarded_call("adam", stream, check_adam, launch_adam, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step);
}

int s2k_mae_panels(const float* imgs, const float* pred, const float* mask, const float* norm, const double* bounds, unsigned char* out,
                   float* patch_mse, int B, int C, int T, int H, int W, int P, int TUB, const int* bands, int frame, const int* panels,
                   int n_panels, int fill, int norm_pix, void* stream) {
    return guarded_call("mae_panels", stream, check_mae_panels, launch_mae_panels, imgs, pred, mask, norm, bounds, out, patch_mse, B, C, T, H, W,
                        P, TUB, bands, frame, panels, n_panels, fill, norm_pix);
}

int s2k_classmap_filter(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K, int size,
                        int mode, unsigned votes, unsigned fixed, int ignore, const unsigned char* labels, const int* index, const int* lut,
                        int nsrc, unsigned long long* hist, unsigned long long* changed, void* stream) {
    return guarded_call("classmap_filter", stream, check_classmap_filter, launch_classmap_filter, src, src_bytes, src_lut, dst, dst_bytes, M, H,
                        W, K, size, mode, votes, fixed, ignore, labels, index, lut, nsrc, hist, changed);
}

int s2k_classmap_components(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int connectivity,
                            unsigned exclude, int* labels, int* areas, unsigned long long* counts, unsigned* status, void* stream) {
    return guarded_call("classmap_components", stream, check_classmap_components, launch_classmap_components, src, src_bytes, src_lut, M, H, W,
                        K, connectivity, exclude, labels, areas, counts, status);
}

int s2k_classmap_sieve(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K,
                       int min_area, unsigned fixed, int to, const int* labels, const int* areas, unsigned long long* best,
                       const unsigned char* hist_labels, const int* index, const int* lut, int nsrc, unsigned long long* hist,
                       unsigned long long* changed, unsigned* status, void* stream) {
    return guarded_call("classmap_sieve", stream, check_classmap_sieve, launch_classmap_sieve, src, src_bytes, src_lut, dst, dst_bytes, M, H, W,
                        K, min_area, fixed, to, labels, areas, best, hist_labels, index, lut, nsrc, hist, changed, status);
}

int s2k_classmap_distance(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int mode, unsigned sites,
                          int connectivity, unsigned exclude, void* work, int* dist2, int* nearest, const void* other, int other_bytes,
                          const int* edges, int n_edges, unsigned long long* hist, void* stream) {
    return guarded_call("classmap_distance", stream, check_classmap_distance, launch_classmap_distance, src, src_bytes, src_lut, M, H, W, K,
                        mode, sites, connectivity, exclude, work, dist2, nearest, other, other_bytes, edges, n_edges, hist);
}

size_t s2k_classmap_distance_workspace(int M, int H, int W) { return classmap_distance_workspace(M, H, W); }

int s2k_calibration(const float* scores, int mode, const void* labels, int label_bytes, const int* label_lut, int N, int K, int P,
                    unsigned exclude, const float* temps, int n_temps, int bins, int measure, float reject_below, int reject_to, float* conf,
                    void* pred, int pred_bytes, unsigned long long* hist, unsigned long long* totals, unsigned long long* skipped,
                    void* stream) {
    return guarded_call("calibration", stream, check_calibration, launch_calibration, scores, mode, labels, label_bytes, label_lut, N, K, P,
                        exclude, temps, n_temps, bins, measure, reject_below, reject_to, conf, pred, pred_bytes, hist, totals, skipped);
}

int s2k_rasterize(const int* verts, int V, const int* ring_start, const int* ring_shape, int R, const int* values, int S, const int* origins,
                  int M, int H, int W, void* dst, int dst_bytes, int mode, int burn, int fill, void* work, long long* unfilled, int* status,
                  void* stream) {
    return guarded_call("rasterize", stream, check_rasterize, launch_rasterize, verts, V, ring_start, ring_shape, R, values, S, origins, M, H, W,
                        dst, dst_bytes, mode, burn, fill, work, unfilled, status);
}

size_t s2k_rasterize_workspace(int M, int S) { return rasterize_workspace(M, S); }

int s2k_zonal_histogram(const void* zone, int zone_bytes, int zone_stride, const void* cls, int cls_bytes, const int* src_lut, int M, int H,
                        int W, int Z, int K, long long* hist, unsigned* status, void* stream) {
    return guarded_call("zonal: histogram", stream, check_zonal_histogram, launch_zonal_histogram, zone, zone_bytes, zone_stride, cls, cls_bytes,
                        src_lut, M, H, W, Z, K, hist, status);
}

int s2k_zonal_bands(const void* zone, int zone_bytes, int zone_stride, const short* vals, int M, int C, int H, int W, int Z, int nodata,
                    int has_nodata, long long* count, long long* sum, long long* sumsq, int* min, int* max, unsigned* status, void* stream) {
    return guarded_call("zonal: bands", stream, check_zonal_bands, launch_zonal_bands, zone, zone_bytes, zone_stride, vals, M, C, H, W, Z, nodata,
                        has_nodata, count, sum, sumsq, min, max, status);
}

int s2k_zonal_majority(const long long* hist, int Z, int K, unsigned votes, long long min_count, int fill, int* out_cls, long long* out_best,
                       void* stream) {
    return guarded_call("zonal: majority", stream, check_zonal_majority, launch_zonal_majority, hist, Z, K, votes, min_count, fill, out_cls,
                        out_best);
}

int s2k_zonal_paint(const void* zone, int zone_bytes, int zone_stride, const int* table, int M, int H, int W, int Z, void* dst, int dst_bytes,
                    int mode, int fill, unsigned* status, void* stream) {
    return guarded_call("zonal: paint", stream, check_zonal_paint, launch_zonal_paint, zone, zone_bytes, zone_stride, table, M, H, W, Z, dst,
                        dst_bytes, mode, fill, status);
}

int s2k_selftest_mfma(const float* a, const float* b, float* d, void* stream) {
    return guarded_call("selftest", stream, check_mfma_selftest, launch_mfma_selftest, a, b, d);
}

}  // extern "C"
