/* s2k — C ABI of the MI355X-native segmentation hot path (libs2k.so, gfx950 only).
 *
 * Drop-in boundary.  The reference's hot path is pure Python calling ATen:
 *   EfficientnetUnet.forward            /root/reference/src/modules/efficientnet_unet.py:125-138
 *   EfficientNet.encode / MBConvBlock   efficientnet_unet.py:251-263, :377-387
 *   FocalLoss.__call__ / CrossEntropy   /root/reference/src/losses.py:24-89
 *   logits.argmax(dim=1)                /root/reference/src/train_segmentation.py:145
 *   loss.backward() (torch autograd)    train_segmentation.py:87-93 via Lightning
 * There is no FFI in the reference for this path, so the entry points below are what a binding
 * for it would call: a whole forward (or backward) of the network is ONE `s2k_program_run` over
 * an array of fused-stage records planned on the host; every stage kind is also launchable on
 * its own (`s2k_op_launch`) for parity tests.  INTEGRATION.md shows the ctypes stub.
 *
 * Rules of the boundary
 *   - plain C: pointers, sizes, POD structs; no torch / HIP types in signatures except the
 *     stream, passed as an opaque `void*` (a hipStream_t);
 *   - every device pointer is BORROWED: the library never allocates, frees or synchronises;
 *     all work is enqueued on the caller's stream (graph-capturable);
 *   - return 0 on success, a negative S2K_E* code on failure, never throw; the message for the
 *     last failure on the calling thread is `s2k_last_error()`;
 *   - re-entrant: may be called concurrently from several host threads, on several streams and
 *     on several devices of one process.  The device that owns `stream` is made current for the
 *     duration of a call and restored afterwards (a NULL stream means the caller's current
 *     device).  The only mutable global is a mutex-guarded pool of per-device side streams;
 *     a side stream + event pair is leased for ONE s2k_program_run and returned when it ends,
 *     by which time all of its work has been ordered back onto the caller's stream;
 *   - no environment variable changes what the shipped library computes (tuning switches exist
 *     only in builds made with -DS2K_TUNING).
 */
#ifndef S2K_H
#define S2K_H

#include <stddef.h>
#include <stdint.h>

#include "s2k_ops.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S2K_ABI_VERSION 2

#define S2K_OK 0
#define S2K_EINVAL (-22)   /* malformed stage record / unsupported geometry */
#define S2K_ENOSYS (-38)   /* unknown stage kind */
#define S2K_EFAULT (-14)   /* null base for a referenced tensor */
#define S2K_EHIP (-5)      /* a HIP launch failed; see s2k_last_error() */

/* One fused stage.  Field meaning per kind: include/s2k_ops.h (generated from plan/opdefs.py).
 * t[]: tensor refs = (base_id << 56) | byte_offset, -1 = null.  256 bytes. */
typedef struct S2kOp {
    int32_t kind;
    int32_t flags;
    int64_t t[S2K_N_T];
    int64_t n[S2K_N_N];
    int32_t d[S2K_N_D];
    float f[S2K_N_F];
} S2kOp;

int s2k_abi_version(void);
size_t s2k_op_size(void);                 /* sizeof(S2kOp), for binding self-checks */
const char* s2k_last_error(void);         /* thread-local, never NULL */
const char* s2k_kind_name(int kind);      /* "CONV", ... or NULL */

/* Enqueue ops[begin, end) on `stream`.  bases[i] is the device pointer of base i
 * (S2K_BASE_*), NULL if that base is not used by the range. */
int s2k_program_run(const S2kOp* ops, int begin, int end, void* const* bases, int n_bases, void* stream);

/* Single stage (parity tests, loss, argmax). */
int s2k_op_launch(const S2kOp* op, void* const* bases, int n_bases, void* stream);

/* Device-side timing of a program range with HIP events on `stream` (bench.py roofline leg):
 * per-kind accumulated milliseconds into ms_by_kind[S2K_N_KINDS + 1]; synchronises the stream. */
int s2k_program_profile(const S2kOp* ops, int begin, int end, void* const* bases, int n_bases, void* stream,
                        float* ms_by_kind, int* launches_by_kind);

/* same, one entry per stage: ms_per_op[end - begin] */
int s2k_program_profile_ops(const S2kOp* ops, int begin, int end, void* const* bases, int n_bases, void* stream,
                            float* ms_per_op);

/* same, plus which kernel the stage's launcher picked: variant_per_op[i] = 0 for the stage's generic kernel
 * (conv_igemm_kernel, wgrad_kernel, ...), 1 for the producer/consumer kernel (conv_pc_kernel / wgrad_pc_kernel), 2 for the
 * bf16 MFMA kernels (conv_bf16_kernel / wgrad_bf16_kernel; S2K_FLAG_BF16 stages), 3 for the LDS-DMA ring kernel
 * (conv_dma_kernel), 4 for the quad-read kernels (conv_q4_kernel: S2K_FLAG_Q4 stages; wgrad_q4_kernel: picked by the launcher),
 * 5 for the f32-split kernels (conv_bf16_kernel / wgrad_bf16_kernel with SPLIT: S2K_FLAG_SPLIT stages, which run nowhere else).
 * Depthwise stages (DWCONV_FWD / _DGRAD / _WGRAD): 0 for the band kernels (dwconv_fwd_kernel, dwconv_dgrad_s1_kernel,
 * dwconv_dgrad_s2_kernel, dwconv_wgrad_kernel), 6 for the wave-per-channel plane kernels (dwconv_{fwd,dgrad,wgrad}_plane_kernel,
 * dwconv_{fwd,dgrad}_plane_s2_kernel), 7 for dwconv_wgrad_kernel walking images inside the workgroup (its image loop).
 * ViT stages: CHAN_LN_FWD 0 for the tile kernel (chan_ln_fwd_kernel), 8 for the row kernel (chan_ln_fwd_rows_kernel);
 * MAE_LOSS_FWD / _BWD 0 for the float4 form of mae_loss_rows_kernel (<*, true>), 9 for its scalar form (<*, false>).
 * 10 on all four records of a small-plane depthwise backward chain (BN_BWD_APPLY flagged S2K_FLAG_CHAIN, DWCONV_WGRAD,
 * DWCONV_DGRAD, BN_BWD_APPLY) that ran as ONE kernel (dw_bwd_chain_kernel): its time is reported on the first record, the other
 * three report 0 ms and no launch.
 * BatchNorm / squeeze-excitation / residual / reduction stages (csrc/ew.hip): 0 for their generic kernels (plane_reduce_kernel,
 * plane_map_kernel, se_bn_sums_kernel, bn_bwd_reduce_kernel, se_fc_bwd_a1 / _a2 / _b_kernel, ...); 11 for the wave-per-channel
 * small-plane kernels (SE_POOL se_pool_small_kernel, SE_BN_SUMS se_bn_sums_small_kernel, BN_BWD_APPLY bn_bwd_apply_small_kernel,
 * BN_RESIDUAL bn_residual_small_kernel); 12 for the workgroup-per-plane kernels (SE_POOL se_pool_big_kernel, SE_BN_SUMS
 * se_bn_sums_big_kernel); 13 for CHANNEL_SUM's channel_sum_rows_kernel; 14 for SE_FC_BWD's se_fc_bwd_small_kernel - SE_FC_BWD
 * reports the route of its data-gradient phase, whichever kernel formed its parameter gradients; 15 for SE_FC_WGRAD's
 * se_fc_wgrad_tile_kernel.
 * bench.py uses it to attribute time and algorithmic FLOPs to the kernel names a rocprofv3 trace shows. */
int s2k_program_profile_variants(const S2kOp* ops, int begin, int end, void* const* bases, int n_bases, void* stream,
                                 float* ms_per_op, int* variant_per_op);

/* fused Adam step (L2-coupled decay, train_segmentation.py:109-127): p, g, m, v flat fp32 [n].  Hyper-parameters are
 * doubles, as Python hands them to torch.optim.Adam: `1 - beta2` and `lr / (1 - beta1**step)` are formed in double and
 * rounded to fp32 once, which is what makes the update bit-compatible with torch's (ABI 2; ABI 1 took floats). */
int s2k_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int step, void* stream);

/* MAE reconstruction pictures (render.mae_panels; csrc/mae_render.hip): up to four uint8 panels of what a masked autoencoder made of
 * a crop, and the per-patch squared error, in ONE launch on `stream`.  A plain function like s2k_adam_step, not a stage kind: it is
 * never part of a program (nothing plans it, nothing profiles it per kind), and the stage table is frozen at 55 kinds - bindings and
 * tests enumerate it - so a picture for people does not get to renumber it.  Adding a function leaves S2K_ABI_VERSION at 2.
 *
 * Geometry (MaeSpec): C channels, T frames, H == W, patch P | H, tubelet TUB | T; g = H / P, L = (T / TUB) * g * g patches of
 * PD = TUB * P * P * C features in (tt, py, px, c) order.  Device pointers, borrowed:
 *   imgs   f32 [B][C][T][H][W]   what the model consumed          pred   f32 [B][L][PD]   MaskedAutoencoderViT.forward's
 *   mask   f32 [B][L]            non-zero = removed               norm   f32 [2][C]       {mean * 255, 1 / (std * 255)} (TILE_PREP's NORM)
 *   bounds f64 [B][2]            (lo, hi) of the stretch          out    u8  [B][n_panels][H][W][3]   h w rgb
 *   patch_mse f32 [B][L] or NULL: mean over PD of (pred - target)^2, target standardised per patch when norm_pix
 * Host values: bands[3] distinct in [0, C); frame in [0, T); panels[n_panels], 1 <= n_panels <= 4, codes 0 original, 1 masked (removed
 * patches = `fill`, 0..255), 2 pasted (pred in removed patches, imgs elsewhere), 3 reconstruction; norm_pix 0 or 1 (pred is
 * de-standardised with the patch's mean and unbiased variance, in f64).
 * Pixel: v = x / norm[1][c] + norm[0][c]; out = (uint8) trunc(clip((v - lo) / (hi - lo) * 255, 0, 255)) in f64, as TILE_QUICKLOOK;
 * bounds without a range (hi <= lo, non-finite) and NaN give 0.
 * Every argument is validated on the host before anything is launched: S2K_EFAULT for a NULL required pointer, S2K_EINVAL for a
 * dimension, band, frame, fill or panel code out of range, for B or T / TUB above 65535 (grid dimensions) and for C*T*H*W or
 * n_panels*H*W*3 of 2^31 or more (32-bit offsets inside a sample).  No allocation, no copy, no synchronisation. */
int s2k_mae_panels(const float* imgs, const float* pred, const float* mask, const float* norm, const double* bounds, unsigned char* out,
                   float* patch_mse, int B, int C, int T, int H, int W, int P, int TUB, const int* bands, int frame, const int* panels,
                   int n_panels, int fill, int norm_pix, void* stream);

/* Class-map neighbourhood filters (classmap.py; csrc/classmap.hip): the size x size majority (mode) filter of a class map and the
 * ignore band around class boundaries, in ONE launch on `stream`.  A plain function like s2k_mae_panels, not a stage kind: the stage
 * table stays at 55 kinds and S2K_ABI_VERSION at 2.
 *
 * src, dst: [M][H][W] class maps, uint8 (`*_bytes` == 1) or int64 (== 8), independently; device pointers, borrowed; dst must not alias
 * src.  src_lut: int32[256] or NULL, only with a 1-byte src: the class of a pixel is then src_lut[raw] (how the pipeline's resident
 * labels are read through its label map).  1 <= K <= 32 classes; size odd in 3..15, r = size / 2.  The window of pixel (y, x) is
 * [y-r, y+r] x [x-r, x+r] clipped to the image: no padding, and maps never see each other.  A pixel whose class lies outside [0, K)
 * never votes and is copied unchanged (into a 1-byte dst: its low byte).
 *   mode 0, MAJORITY: classes whose bit is set in `votes` vote, the others count 0; best = the largest count in the window.  The output
 *     is the centre's class if its own count equals best, or best == 0, or the centre's bit is set in `fixed`; otherwise the LOWEST
 *     class whose count equals best (the centre wins ties, then the lowest index).  `ignore` is unused.
 *   mode 1, BOUNDARY: a centre of class c != ignore becomes `ignore` iff its window holds a pixel of a class in [0, K) that is neither c
 *     nor ignore; everything else is copied (touching only the ignored class is no boundary).  votes and fixed must be 0.
 * changed: u64 [M] or NULL; changed[m] += pixels of map m whose output class differs from their input class.
 * hist: u64 [K][K] or NULL; with it labels (u8 [nsrc][H][W]), index (device i32 [M], values in [0, nsrc)) and lut (i32[256]) are
 * required: hist[t][p] += 1 with t = lut[labels[index[m]][y][x]] and p the output class wherever both lie in [0, K) - WINDOW_BLEND's
 * HIST (LDS bins per workgroup, one 64-bit atomic per non-zero bin).  Both counters are integer sums: exact.
 * Every argument is validated on the host before anything is launched: S2K_EFAULT for a NULL src or dst; S2K_EINVAL for a width other
 * than 1 or 8, src_lut with an 8-byte src, src == dst, K, size, mode, ignore (mode 1) out of range, bits of votes / fixed at K and
 * above (mode 0) or any set (mode 1), M, H or W below 1, H * W >= 2^31 (offsets inside a map are 32-bit; the map offset is 64-bit),
 * M * ceil(W / (64 - 2r)) * ceil(H / 16) >= 2^24 (one workgroup per strip and band of a map), hist without labels, index, lut or with
 * nsrc < 1.  Messages begin with "classmap_filter: ".  No allocation, no copy, no synchronisation. */
int s2k_classmap_filter(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K,
                        int size, int mode, unsigned votes, unsigned fixed, int ignore, const unsigned char* labels, const int* index,
                        const int* lut, int nsrc, unsigned long long* hist, unsigned long long* changed, void* stream);

/* Connected components of class maps and the minimum-area sieve (classmap.py; csrc/components.hip).  Two plain functions like
 * s2k_classmap_filter, not stage kinds: the stage table stays at 55 kinds and S2K_ABI_VERSION at 2.  Each is a fixed, small number of
 * plain launches on `stream` (three for the labels; one or two for the sieve): no grid-wide barrier, no cooperative launch.
 *
 * Definitions (they are the oracle; the reference project has no such operation).  src: [M][H][W] class maps, uint8 (src_bytes == 1) or
 * int64 (== 8); src_lut: int32[256] or NULL, only with a 1-byte src: the class of a pixel is then src_lut[raw].  A pixel is LABELLED if
 * its class lies in [0, K), 1 <= K <= 32, and its class bit is not set in `exclude`.  Two labelled pixels are adjacent if they have the
 * same class and are 4-neighbours (connectivity 4) or 4-neighbours or diagonal neighbours (connectivity 8); components are the connected
 * classes of that relation.  Maps never see each other, and there is no padding.
 *   labels  i32 [M][H][W]: the smallest linear index y * W + x over the pixels of the pixel's component (that pixel is the ROOT); -1 for
 *           an unlabelled pixel.  Canonical: independent of the order in which threads run.
 *   areas   i32 [M][H][W]: areas[m][i] = pixels of the component whose root is i, 0 where i is no root.  Zeroed by the call.
 *   counts  u64 [M][K] or NULL: counts[m][k] += components of class k in map m.
 *   status  u32 [1]: OR-ed into, never cleared.  The parent array keeps parent[i] <= i, so every find / union loop ends within 2 * H * W
 *           steps by construction; each loop also carries that bound, and a thread that overruns it sets a bit here (1 the tile pass,
 *           2 the merge across tile edges, 4 the flatten pass, 8 the sieve was handed labels outside [-1, H * W)) and writes nothing
 *           further.  Non-zero means the outputs are not to be used.
 * s2k_classmap_components validates every argument on the host before anything is launched: S2K_EFAULT for a NULL src, labels, areas or
 * status; S2K_EINVAL for src_bytes other than 1 or 8, src_lut with an 8-byte src, K outside 1..32, connectivity other than 4 or 8, bits of
 * exclude at K or above, M, H or W below 1, H * W >= 2^31 (offsets inside a map are 32-bit; the map offset is 64-bit),
 * M * ceil(H / 16) * ceil(W / 64) >= 2^24 (one workgroup per 16 x 64 tile of a map).  Messages begin with "classmap_components: ".
 *
 * s2k_classmap_sieve, ONE pass: `labels` and `areas` are those of s2k_classmap_components over the same src (with exclude == 0 every
 * pixel with a class is in a component).  A component is SMALL if its area is below min_area (>= 1) and its class bit is not set in
 * `fixed`.  With to >= 0 every pixel of a small component becomes `to`.  With to == -1 every small component takes the class of its best
 * DONOR: a donor is a component that shares at least one pixel EDGE with it (4-neighbour pairs only, whatever the connectivity) and has
 * a different class; donors are ordered by area >= min_area first, then larger area, then lower root; a small component without a
 * donor stays as it is.  The class taken is the donor's class in src - all relabelling of a pass is simultaneous.  Unlabelled pixels
 * are copied unchanged (into a 1-byte dst: their low byte) and donate nothing.  dst: [M][H][W], uint8 or int64 independently of src;
 * it must not alias src.  best: u64 [M][H][W] workspace for the donor keys, zeroed by the call; NULL is allowed with to >= 0.
 * changed (u64 [M] or NULL) and hist (u64 [K][K] or NULL, with hist_labels u8 [nsrc][H][W], index i32 [M] and lut i32[256]) are counted
 * exactly as by s2k_classmap_filter and added to.
 * Validated on the host before anything is launched: S2K_EFAULT for a NULL src, dst, labels, areas or status; S2K_EINVAL for a width
 * other than 1 or 8, src_lut with an 8-byte src, src == dst, K outside 1..32, bits of fixed at K or above, min_area < 1, `to` outside
 * -1..K-1, best NULL with to < 0, M, H or W below 1, H * W >= 2^31, M * ceil(H / 16) * ceil(W / 64) >= 2^24, hist without hist_labels,
 * index or lut or with nsrc < 1.  Messages begin with "classmap_sieve: ".  Neither function allocates, copies or synchronises. */
int s2k_classmap_components(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int connectivity,
                            unsigned exclude, int* labels, int* areas, unsigned long long* counts, unsigned* status, void* stream);
int s2k_classmap_sieve(const void* src, int src_bytes, const int* src_lut, void* dst, int dst_bytes, int M, int H, int W, int K,
                       int min_area, unsigned fixed, int to, const int* labels, const int* areas, unsigned long long* best,
                       const unsigned char* hist_labels, const int* index, const int* lut, int nsrc, unsigned long long* hist,
                       unsigned long long* changed, unsigned* status, void* stream);

/* Exact Euclidean distance transform of class maps, the nearest site and distance-binned confusion counts (classmap.py;
 * csrc/distance.hip).  A plain function like s2k_classmap_components, not a stage kind: the stage table stays at 55 kinds and
 * S2K_ABI_VERSION at 2.  Two plain launches on `stream` whatever the map looks like (a column pass into `work`, a row pass): no
 * grid-wide barrier, no cooperative launch.
 *
 * Definitions (they are the oracle; the reference project has no such operation).  src: [M][H][W] class maps, uint8 (src_bytes == 1) or
 * int64 (== 8); src_lut: int32[256] or NULL, only with a 1-byte src: the class of a pixel is then src_lut[raw].  1 <= K <= 32.  A pixel
 * is LABELLED if its class lies in [0, K) and its class bit is not set in `exclude`.  A pixel is a SITE
 *   mode 0 (classes)   if it is labelled and its class bit is set in `sites` (non-zero, inside [0, K), disjoint from exclude);
 *   mode 1 (boundary)  if it is labelled and at least one neighbour is labelled with a DIFFERENT class: the 4-neighbours at
 *                      connectivity 4, those and the diagonals at 8, only neighbours inside the map.  Unlabelled pixels are never
 *                      sites and never make a neighbour a site; both sides of a boundary are sites.  `sites` must be 0.
 *   dist2    i32 [M][H][W]: for EVERY pixel, labelled or not, the minimum over the sites s of its own map of (y - ys)^2 + (x - xs)^2;
 *            0 at a site; 2^31 - 1 (NO_SITE) where the map has no site.  Maps never see each other.
 *   nearest  i32 [M][H][W] or NULL: the linear index ys * W + xs of a nearest site, -1 where there is none.  The tie rule is canonical
 *            and part of the contract: among the sites at distance dist2, the one with the smallest linear index.
 *   work     M * H * W 16-bit column offsets (s2k_classmap_distance_workspace(M, H, W) bytes), written and read by the call.
 *   hist     u64 [n_edges + 1][K][K] or NULL, ADDED to by the launch that writes dist2 (without it that launch does no counting work):
 *            with other ([M][H][W], uint8 or int64: other_bytes; no table) and edges (i32 [n_edges] in HOST memory, 1 <= n_edges <= 8,
 *            each >= 0, strictly ascending: thresholds on dist2), for every pixel whose src class and whose `other` class both lie in
 *            [0, K): hist[b][src class][other class] += 1, b = the number of j with dist2 > edges[j].  This count ignores `exclude`
 *            (the CONFUSION convention); NO_SITE lands in the last bin.  Integer sums: exact.
 * Limits, all checked on the host before anything is launched: H, W <= 16384 (an offset then fits 16 bits and dist2 31 bits);
 * H * W < 2^31 (offsets inside a map are 32-bit; the map offset is 64-bit); M * ceil(W / 64) < 2^24 (one 64-thread workgroup per 64
 * columns of a map) and M * ceil(H / R) < 2^24 with R = min(8, 65535 / W) (one workgroup per R rows of a map: it counts its pixels in
 * 16-bit bins).  S2K_EFAULT for a NULL src, dist2 or work; S2K_EINVAL for src_bytes (or, with hist, other_bytes) other than 1 or 8,
 * src_lut with an 8-byte src, K outside 1..32, mode other than 0 or 1, connectivity other than 4 or 8, bits of sites or exclude at K or
 * above, mode 0 with sites == 0 or sites overlapping exclude, mode 1 with sites != 0, hist without other or edges, n_edges outside
 * 1..8, an edge below 0 or not above its predecessor, M, H or W below 1, a limit exceeded.  Messages begin with "classmap_distance: ".
 * Every loop of the kernels is bounded by construction and carries that bound as its trip limit (the column sweeps H, the search W):
 * there is no data-dependent loop and therefore no status word.  The function does no allocation, no copy and no synchronisation.
 * s2k_classmap_distance_workspace: bytes of `work` (0 for M, H or W below 1). */
int s2k_classmap_distance(const void* src, int src_bytes, const int* src_lut, int M, int H, int W, int K, int mode, unsigned sites,
                          int connectivity, unsigned exclude, void* work, int* dist2, int* nearest, const void* other, int other_bytes,
                          const int* edges, int n_edges, unsigned long long* hist, void* stream);
size_t s2k_classmap_distance_workspace(int M, int H, int W);

/* Calibration of a probability map: the confidence raster, the class map with an abstention class, the reliability histogram and the
 * negative log-likelihood under several temperatures (metrics.CalibrationMetrics, metrics.fit_temperature, classmap.confidence;
 * csrc/calibration.hip).  A plain function like s2k_classmap_distance, not a stage kind: the stage table stays at 55 kinds and
 * S2K_ABI_VERSION at 2.  ONE launch on `stream`; every loop is bounded by construction (a workgroup walks a fixed number of passes).
 *
 * Inputs.  scores: f32 [N][K][P], the NCHW layout with P = H * W; 1 <= K <= 32.  mode 0: the scores are probabilities and are taken as
 * given; mode 1: logits.  labels: uint8 (label_bytes == 1) or int64 (== 8) [N][P], or NULL; label_lut: int32[256] or NULL, only with
 * 1-byte labels: the class of a pixel is then label_lut[raw].  exclude: bit mask of label classes that are not counted.  temps:
 * f32[n_temps] in HOST memory, 1 <= n_temps <= 8, each finite and above 0 (mode 0: the single value 1); the kernel multiplies by
 * r_t = 1.0f / temps[t], rounded once on the host.  1 <= bins <= 64.  measure 0 max, 1 margin.  reject_to: a class in [0, K), or -1.
 * Outputs, each may be NULL, at least one is required; device pointers, borrowed:
 *   conf f32 [N][P];  pred uint8 or int64 [N][P] (pred_bytes);  hist u64 [K][bins][3], ADDED to;  totals u64 [n_temps][2], ADDED to;
 *   skipped u64 [1], ADDED to.  hist and totals need labels.
 *
 * Definitions (they are the oracle; the reference project has no such operation), per pixel with scores s[0..K):
 *   a      the first maximum of s: top = s[0], then for k = 1..K-1 in order `if (s[k] > top)` - strict >, WINDOW_BLEND's ARGMAX rule; a
 *          NaN is therefore never chosen over s[0].  Taken on the raw scores in both modes (T > 0 keeps the order).
 *   mode 0 p[k] = s[k].  c = p[a].  nll_0 = 128 if !(p[label] > 0) (a score <= 0, or NaN), else -logf(p[label]).
 *   mode 1 d[k] = s[k] - s[a] (f32; 0 at a); under temperature t: e[k] = expf(d[k] * r_t), S = e[0] + ... + e[K-1] added in index
 *          order, p_t[k] = e[k] / S.  c = 1.0f / S under temps[0].  nll_t = logf(S) - d[label] * r_t, which is logsumexp(z) - z[label]
 *          with the maximum taken out of both.  One rounding per written operator (no contraction).
 *   c      is ALWAYS the binning confidence, whatever `measure` says.
 *   conf   the written value: c for measure 0; for measure 1 c - second with second = the largest p[k], k != a (scanned from -infinity
 *          with strict >; mode 1: (largest e[k], k != a) / S under temps[0]), and c itself when K == 1.
 *   pred   (reject_to >= 0 && conf < reject_below) ? reject_to : a.  A NaN conf is never below anything.  Rejection never affects the
 *          counts: the histogram is that of a.
 *   A pixel is COUNTED if its label class (after the table) lies in [0, K), its class bit is not set in exclude, and 0 <= c <= 1.  A
 *   labelled pixel that fails only the last test (c above 1, negative or NaN) adds 1 to skipped[0].  For a counted pixel, with
 *   b = min(bins - 1, (int)(c * (float)bins)) (an f32 product, truncated):
 *     hist[a][b][0] += 1;  hist[a][b][1] += (label == a);  hist[a][b][2] += rint(c * 2^20)
 *     for every t: totals[t][0] += 1;  totals[t][1] += rint(min(max(nll_t, 0), 128) * 2^20)   (a NaN nll_t counts as 0)
 * Given the per-pixel c every sum is an integer function: exact, independent of the launch geometry and bit-identical from run to run.
 * In mode 0 c itself is exact (a copy; the margin is one f32 subtraction); only nll in mode 0, and c and nll in mode 1, go through expf
 * and logf.
 * Every argument is validated on the host before anything is launched: S2K_EFAULT for a NULL scores; S2K_EINVAL for mode or measure
 * other than 0 or 1, K outside 1..32, bins outside 1..64, n_temps outside 1..8, temps NULL, a temperature (or its f32 reciprocal) that is
 * not finite and above 0, mode 0 with temps other than {1}, label_bytes (with labels) or pred_bytes (with pred) other than 1 or 8,
 * label_lut without 1-byte labels, bits of exclude at K or above, reject_to outside -1..K-1, hist or totals without labels, no output at
 * all, N or P below 1, N * ceil(P / 4) >= 2^31 (a thread owns a quad of pixels; at most 1024 workgroups walk the quads, and a
 * workgroup's 32-bit counter halves then hold whatever it sees).  Messages begin with "calibration: ".  Quad loads and stores are used
 * when P % 4 == 0 and scores, labels, conf and pred are 16-byte aligned; otherwise every element is read and written on its own.  No
 * allocation, no copy, no synchronisation. */
int s2k_calibration(const float* scores, int mode, const void* labels, int label_bytes, const int* label_lut, int N, int K, int P,
                    unsigned exclude, const float* temps, int n_temps, int bins, int measure, float reject_below, int reject_to, float* conf,
                    void* pred, int pred_bytes, unsigned long long* hist, unsigned long long* totals, unsigned long long* skipped,
                    void* stream);

/* Exact polygon rasterisation into label tiles (classmap.PolygonSet, classmap.rasterize, GpuTilePipeline.rasterize_labels;
 * csrc/rasterize.hip).  A plain function like s2k_calibration, not a stage kind: the stage table stays at 55 kinds and S2K_ABI_VERSION at
 * 2.  Three plain launches on `stream` whatever the geometry looks like (boxes, per-tile lists, fill): no grid-wide barrier, no host read.
 *
 * Definitions (they are the oracle; the reference burns its labels with rasterio.features.rasterize on the host, whose tie rule on an
 * edge is GDAL's own).  One pixel frame for the whole area of interest: x to the right, y down.  Pixel (i, j) of a tile with origin
 * (ox, oy), in whole pixels, has its centre at (ox + j + 1/2, oy + i + 1/2).  Coordinates are fixed point, 256 units per pixel, i32: in
 * units the centre is cx = 256 (ox + j) + 128, cy = 256 (oy + i) + 128.  Every vertex coordinate and every 256 * origin has magnitude at
 * most 2^28; every product below then fits int64 (each is below 2^29 * 2^29).
 *   verts       i32 [V][2]: (x, y) in units.
 *   ring_start  i32 [R + 1]: ring r is the closed polyline over verts[ring_start[r] .. ring_start[r + 1]), the closing edge implied;
 *               non-decreasing, ring_start[0] = 0, ring_start[R] = V.  A ring of fewer than 3 vertices covers nothing.
 *   ring_shape  i32 [R]: the shape a ring belongs to; non-decreasing, in [0, S).  A SHAPE is the set of its rings - exterior, holes and
 *               the parts of a multi-polygon alike; a shape without rings covers nothing.
 *   INSIDE      a centre is inside a shape when the number of edges over all its rings with BOTH properties is odd (even-odd rule):
 *               (1) ylo <= cy < yhi, (xlo, ylo) the end of the edge with the smaller y and (xhi, yhi) the other: horizontal edges never
 *               count; (2) xlo * (yhi - ylo) + (cy - ylo) * (xhi - xlo) <= cx * (yhi - ylo), exactly, in int64: the crossing is not to
 *               the right of the centre.  This is the top-left rule: a centre on a left or top edge is inside, one on a right or bottom
 *               edge outside, so shapes that share an edge partition the centres on it.
 *   ORDER       shapes are burned in index order; a pixel inside several takes the last.
 *   values      i32 [S]: what shape s burns (burn == 0); with burn == 1 it burns s itself and values may be NULL.
 *   origins     i32 [M][2]: (ox, oy) of tile m, a device pointer like the rest.
 *   dst         [M][H][W], dst_bytes 1 (uint8), 4 (int32) or 8 (int64) an element; a burned value is stored by conversion (a 1-byte dst
 *               takes its low byte).  mode 0 (fill): a pixel inside no shape gets `fill`; mode 1 (onto): it keeps what dst held.
 *   unfilled    i64 [M] or NULL, ADDED to: the pixels of tile m inside no shape.
 *   work        s2k_rasterize_workspace(M, S) bytes, written and read by the call: 8 ints per shape (box and ranges), M list lengths,
 *               M * S list entries.  16-byte aligned; verts and origins 8-byte aligned.
 *   status      u32 [1], OR-ed into: what only the device can see.  1 the ring tables are out of order or out of range, 2 a vertex
 *               beyond +-2^28, 4 an origin beyond +-2^20.  The kernels clamp every index and coordinate they read, and every loop is
 *               bounded by a count passed by value or a compile-time constant, so that such tables cause neither a read out of bounds
 *               nor an endless loop; the output is then not to be used.
 * Validated on the host before anything is launched: S2K_EFAULT for a NULL verts, ring_start, ring_shape, origins, dst, work or status
 * (reported first); S2K_EINVAL for a misaligned verts, origins or work, V, R or S below 0, R > V, rings without a shape (R > 0, S == 0),
 * vertices without a ring (R == 0, V > 0), dst_bytes other than 1, 4 or 8, mode or burn other than 0 or 1, burn == 1 with a 1-byte dst,
 * burn == 0 with values NULL and S > 0, fill outside 0..255 with a 1-byte dst, M, H or W below 1, H * W >= 2^31 (offsets inside a tile are
 * 32-bit; the tile offset is 64-bit), M * ceil(H / 32) * ceil(W / 512) >= 2^31 (one workgroup per 32 x 512 block of a tile).  V = 0,
 * R = 0 and S = 0 are valid: every tile is `fill`, or dst is left as it is.  Messages begin with "rasterize: ".  The result is the
 * definition bit for bit and identical from run to run.  No allocation, no copy, no synchronisation.
 * s2k_rasterize_workspace: bytes of `work` (0 for M below 1 or S below 0). */
int s2k_rasterize(const int* verts, int V, const int* ring_start, const int* ring_shape, int R, const int* values, int S, const int* origins,
                  int M, int H, int W, void* dst, int dst_bytes, int mode, int burn, int fill, void* work, long long* unfilled, int* status,
                  void* stream);
size_t s2k_rasterize_workspace(int M, int S);

/* Zonal statistics: per-zone class votes and band statistics, the majority class per zone and painting a per-zone table back into a
 * raster (zonal.py; csrc/zonal.hip).  Four plain functions like s2k_rasterize, not stage kinds: the stage table stays at 55 kinds and
 * S2K_ABI_VERSION at 2.  Each is ONE plain launch on `stream`: no grid-wide barrier, no host read.
 *
 * Definitions (they are the oracle; the reference asks these questions per dataset and per tile on the host, never per object).
 *   zone         [M][H][W], int32 (zone_bytes == 4) or int64 (== 8): the RAW zone value of every pixel.
 *   zone_stride  0: raw values are global ids, as rasterize(burn = index) writes them; zone_limit = Z.
 *                > 0: raw values are ids inside their own map, as s2k_classmap_components writes them with zone_stride = H * W;
 *                zone_limit = zone_stride, and M * zone_stride == Z is required.
 *   KEY          of pixel (m, y, x) with raw value r: r < 0 (the fill = -1 convention): the pixel has NO KEY and is skipped silently;
 *                r >= zone_limit, compared in 64 bits (an int64 value is never truncated): no key either, and 1 is OR-ed into status[0];
 *                otherwise z = r + m * zone_stride, which lies in [0, Z).  Tables have Z rows; 1 <= Z < 2^31.
 *   status       u32 [1], OR-ed into, never cleared: 1 = a raw zone value at or above zone_limit was met (and skipped).
 * s2k_zonal_histogram.  cls: [M][H][W], uint8 (cls_bytes == 1) or int64 (== 8); src_lut: int32[256] or NULL, only with a 1-byte cls: the
 *   class of a pixel is then src_lut[raw].  1 <= K <= 32.  hist: i64 [Z][K], ADDED to: for every pixel with a key z and a class c in
 *   [0, K): hist[z][c] += 1.  A class outside [0, K) is skipped silently.
 * s2k_zonal_bands.  vals: int16 [M][C][H][W], 1 <= C <= 16.  A band value v of a pixel with key z is COUNTED for band c unless has_nodata
 *   is 1 and v == nodata (for that band only; the other bands of the pixel are judged on their own).  Outputs, all [Z][C]: for every
 *   counted value   count[z][c] += 1;  sum[z][c] += v;  sumsq[z][c] += v * v   (i64, ADDED to);
 *                   min[z][c] = min(min[z][c], v);  max[z][c] = max(max[z][c], v)   (i32; the caller initialises them, usually to
 *   INT32_MAX and INT32_MIN, and a (z, c) without a counted value keeps what it held).  sum is exact; sumsq is exact while it stays
 *   below 2^63, which 2^33 values of magnitude 32768 cannot reach.
 * s2k_zonal_majority.  hist: i64 [Z][K]; votes: bit mask of the classes that vote (non-zero, no bit at K or above); min_count >= 1.
 *   best[z] = the largest hist[z][c] over the voting classes c (signed comparison);
 *   out_cls[z] (i32 [Z]) = the LOWEST voting class c with hist[z][c] == best[z] if best[z] >= min_count, else `fill` (any int32);
 *   out_best (i64 [Z] or NULL)[z] = best[z].  No zone raster and no status.
 * s2k_zonal_paint.  table: i32 [Z]; dst: [M][H][W], dst_bytes 1 (uint8), 4 (int32) or 8 (int64).  A pixel with a key z and
 *   table[z] >= 0 gets table[z], stored by conversion (a 1-byte dst takes its low byte).  Every other pixel - no key, or a negative
 *   table entry - gets `fill` in mode 0 and keeps what dst held in mode 1.
 * Every argument is validated on the host before anything is launched: S2K_EFAULT, reported first, for a NULL zone, cls, hist, vals,
 * count, sum, sumsq, min, max, table, dst, out_cls or (where the entry takes one) status; S2K_EINVAL for zone_bytes other than 4 or 8,
 * cls_bytes other than 1 or 8, dst_bytes other than 1, 4 or 8, src_lut with an 8-byte cls, K outside 1..32, C outside 1..16, has_nodata
 * other than 0 or 1, Z, M, H or W below 1, zone_stride < 0, zone_stride > 0 with M * zone_stride != Z, H * W >= 2^31 (offsets inside a map
 * are 32-bit; the map offset is 64-bit), M * ceil(H / 16) * ceil(W / 256) >= 2^31 (histogram and bands: one workgroup per 16 x 256 block
 * of a map) or ceil(M * H * W / 256) >= 2^31 (paint: one thread per pixel), votes zero or with a bit at K or above, min_count < 1, mode
 * other than 0 or 1, fill outside 0..255 with a 1-byte dst.  Messages begin with "zonal: ".
 * All results are integer functions of the inputs: bit-identical from run to run, whatever the order in which workgroups arrive, and
 * independent of how M is split over several calls (zone_stride == 0).  Quad loads are used when W % 4 == 0 and the rasters are 16-byte
 * aligned; otherwise every element is read on its own.  No allocation, no copy, no synchronisation, no host read. */
int s2k_zonal_histogram(const void* zone, int zone_bytes, int zone_stride, const void* cls, int cls_bytes, const int* src_lut, int M, int H,
                        int W, int Z, int K, long long* hist, unsigned* status, void* stream);
int s2k_zonal_bands(const void* zone, int zone_bytes, int zone_stride, const short* vals, int M, int C, int H, int W, int Z, int nodata,
                    int has_nodata, long long* count, long long* sum, long long* sumsq, int* min, int* max, unsigned* status, void* stream);
int s2k_zonal_majority(const long long* hist, int Z, int K, unsigned votes, long long min_count, int fill, int* out_cls, long long* out_best,
                       void* stream);
int s2k_zonal_paint(const void* zone, int zone_bytes, int zone_stride, const int* table, int M, int H, int W, int Z, void* dst, int dst_bytes,
                    int mode, int fill, unsigned* status, void* stream);

/* Measured ceilings of the current device for roofline reporting (bench.py): sustained v_mfma_f32_32x32x2_f32 rate with every
 * SIMD issuing back to back (TFLOP/s), the shader clock held meanwhile (MHz), and a float4 stream copy (GB/s, read + write).
 * `scratch`: >= 64 MiB of device memory (size the copy past the caches: 1 GiB+).  Synchronises `stream`.  Not on the hot path. */
int s2k_measure_peaks(void* scratch, size_t scratch_bytes, int waves_per_simd, double* mfma_tflops, double* mfma_clock_mhz,
                      double* copy_gbps, void* stream);

/* Diagnostics for tests: run a 32x32x2 f32 MFMA on A[32x2], B[2x32] and return D[32x32]
 * (checks the lane maps the kernels rely on with exact integer data). */
int s2k_selftest_mfma(const float* a, const float* b, float* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S2K_H */
