"""ctypes binding of libs2k.so (include/s2k.h).  There is no fallback: if the HIP library is not
built, or a tensor is not on the GPU, the product path raises."""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np
import torch  # noqa: F401  -- BEFORE libs2k.so is loaded: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64; dlopen-ing
#                        libs2k.so first would bind the process to /opt/rocm's copies (same SONAME) and leave two HIP runtimes that
#                        do not see each other's device state (launches then fail with "no ROCm-capable device is detected")

from .plan import opdefs as D
from .plan.program import OP_DTYPE

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "libs2k.so"
_lib = None


class S2kError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = Path(os.environ.get("S2K_LIB", LIB_PATH))
    if not path.exists():
        raise S2kError(f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'); "
                       "there is no CPU fallback for this path")
    L = ctypes.CDLL(str(path))
    L.s2k_abi_version.restype = ctypes.c_int
    L.s2k_op_size.restype = ctypes.c_size_t
    L.s2k_last_error.restype = ctypes.c_char_p
    L.s2k_kind_name.restype = ctypes.c_char_p
    L.s2k_kind_name.argtypes = [ctypes.c_int]
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.s2k_program_run.restype = i32
    L.s2k_program_run.argtypes = [vp, i32, i32, vp, i32, vp]
    L.s2k_op_launch.restype = i32
    L.s2k_op_launch.argtypes = [vp, vp, i32, vp]
    L.s2k_program_profile.restype = i32
    L.s2k_program_profile.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp]
    L.s2k_program_profile_ops.restype = i32
    L.s2k_program_profile_ops.argtypes = [vp, i32, i32, vp, i32, vp, vp]
    L.s2k_program_profile_variants.restype = i32
    L.s2k_program_profile_variants.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp]
    f64 = ctypes.c_double
    L.s2k_adam_step.restype = i32
    L.s2k_adam_step.argtypes = [vp, vp, vp, vp, ctypes.c_int64, f64, f64, f64, f64, f64, i32, vp]
    L.s2k_measure_peaks.restype = i32
    L.s2k_measure_peaks.argtypes = [vp, ctypes.c_size_t, i32, vp, vp, vp, vp]
    L.s2k_selftest_mfma.restype = i32
    L.s2k_selftest_mfma.argtypes = [vp, vp, vp, vp]
    L.s2k_mae_panels.restype = i32
    L.s2k_mae_panels.argtypes = [vp] * 7 + [i32] * 7 + [vp, i32, vp, i32, i32, i32, vp]
    u32 = ctypes.c_uint
    L.s2k_classmap_filter.restype = i32
    L.s2k_classmap_filter.argtypes = [vp, i32, vp, vp, i32] + [i32] * 6 + [u32, u32, i32, vp, vp, vp, i32, vp, vp, vp]
    L.s2k_classmap_components.restype = i32
    L.s2k_classmap_components.argtypes = [vp, i32, vp] + [i32] * 5 + [u32, vp, vp, vp, vp, vp]
    L.s2k_classmap_sieve.restype = i32
    L.s2k_classmap_sieve.argtypes = [vp, i32, vp, vp, i32] + [i32] * 5 + [u32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.s2k_classmap_distance.restype = i32
    L.s2k_classmap_distance.argtypes = [vp, i32, vp] + [i32] * 5 + [u32, i32, u32, vp, vp, vp, vp, i32, vp, i32, vp, vp]
    L.s2k_classmap_distance_workspace.restype = ctypes.c_size_t
    L.s2k_classmap_distance_workspace.argtypes = [i32] * 3
    L.s2k_calibration.restype = i32
    L.s2k_calibration.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, u32, vp, i32, i32, i32, ctypes.c_float, i32, vp, vp, i32, vp, vp, vp, vp]
    L.s2k_rasterize.restype = i32
    L.s2k_rasterize.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, i32, i32, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.s2k_rasterize_workspace.restype = ctypes.c_size_t
    L.s2k_rasterize_workspace.argtypes = [i32] * 2
    i64 = ctypes.c_longlong
    L.s2k_zonal_histogram.restype = i32
    L.s2k_zonal_histogram.argtypes = [vp, i32, i32, vp, i32, vp] + [i32] * 5 + [vp, vp, vp]
    L.s2k_zonal_bands.restype = i32
    L.s2k_zonal_bands.argtypes = [vp, i32, i32, vp] + [i32] * 7 + [vp] * 7
    L.s2k_zonal_majority.restype = i32
    L.s2k_zonal_majority.argtypes = [vp, i32, i32, u32, i64, i32, vp, vp, vp]
    L.s2k_zonal_paint.restype = i32
    L.s2k_zonal_paint.argtypes = [vp, i32, i32, vp] + [i32] * 4 + [vp, i32, i32, i32, vp, vp]
    if L.s2k_abi_version() != 2:
        raise S2kError(f"libs2k ABI {L.s2k_abi_version()} != 2")
    if L.s2k_op_size() != D.OP_BYTES or OP_DTYPE.itemsize != D.OP_BYTES:
        raise S2kError("S2kOp layout mismatch between Python and libs2k")
    for name, kind in D.KIND.items():
        got = L.s2k_kind_name(kind)
        if got is None or got.decode() != name:
            raise S2kError(f"stage kind table mismatch at {name}")
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        raise S2kError(f"s2k error {rc}: {lib().s2k_last_error().decode()}")


class Bases:
    """The `void* bases[]` array handed to s2k_program_run."""

    def __init__(self):
        self.arr = (ctypes.c_void_p * len(D.BASES))()
        self.keep = {}
        self.device = None      # device of the tensors behind the bases: made current around every launch (run / profile)

    def set(self, name: str, tensor) -> "Bases":
        self.keep[name] = tensor
        if tensor is not None and self.device is None and tensor.is_cuda:
            self.device = tensor.device
        self.arr[D.BASE[name]] = None if tensor is None else tensor.data_ptr()
        return self

    @property
    def ptr(self):
        return ctypes.cast(self.arr, ctypes.c_void_p)


def _guard(bases: Bases):
    """The default stream's handle is 0 on every device, so the library cannot tell the device from the stream alone:
    make the device that owns the tensors current for the call (a module on cuda:1 with cuda:0 current otherwise launches
    on the wrong device)."""
    import contextlib

    return torch.cuda.device(bases.device) if bases.device is not None else contextlib.nullcontext()


def run(packed: np.ndarray, bases: Bases, stream: int, begin: int = 0, end: int | None = None) -> None:
    end = len(packed) if end is None else end
    with _guard(bases):
        check(lib().s2k_program_run(packed.ctypes.data, begin, end, bases.ptr, len(D.BASES), stream))


def profile(packed: np.ndarray, bases: Bases, stream: int):
    nk = len(D.OPS) + 1
    ms = np.zeros(nk, dtype=np.float32)
    cnt = np.zeros(nk, dtype=np.int32)
    with _guard(bases):
        check(lib().s2k_program_profile(packed.ctypes.data, 0, len(packed), bases.ptr, len(D.BASES), stream,
                                        ms.ctypes.data, cnt.ctypes.data))
    names = {v: k for k, v in D.KIND.items()}
    return {names[k]: (float(ms[k]), int(cnt[k])) for k in range(1, nk) if cnt[k]}


def profile_ops(packed: np.ndarray, bases: Bases, stream: int) -> np.ndarray:
    """Per-stage device milliseconds (HIP events on the launch stream)."""
    ms = np.zeros(len(packed), dtype=np.float32)
    with _guard(bases):
        check(lib().s2k_program_profile_ops(packed.ctypes.data, 0, len(packed), bases.ptr, len(D.BASES), stream, ms.ctypes.data))
    return ms


def profile_variants(packed: np.ndarray, bases: Bases, stream: int):
    """(ms per stage, variant per stage): the kernel family each stage's launcher picked (include/s2k.h,
    s2k_program_profile_variants): 0 generic, 1 producer / consumer, 2 bf16 MFMA, 3 LDS-DMA ring, 4 quad reads, 5 f32-split;
    depthwise stages: 0 band kernels, 6 wave-per-channel plane kernels, 7 the weight gradient's image loop; ViT stages: 8 the
    LayerNorm row kernel (0 its tile kernel), 9 the scalar MAE-loss kernel (0 its float4 form); 10 a depthwise backward chain run as
    one kernel; the BatchNorm / SE / residual / reduction stages of csrc/ew.hip: 0 their generic kernels, 11 the wave-per-channel
    small-plane kernels, 12 the workgroup-per-plane kernels, 13 channel_sum_rows_kernel, 14 se_fc_bwd_small_kernel (SE_FC_BWD
    reports its data-gradient route), 15 se_fc_wgrad_tile_kernel."""
    ms = np.zeros(len(packed), dtype=np.float32)
    var = np.zeros(len(packed), dtype=np.int32)
    with _guard(bases):
        check(lib().s2k_program_profile_variants(packed.ctypes.data, 0, len(packed), bases.ptr, len(D.BASES), stream,
                                                 ms.ctypes.data, var.ctypes.data))
    return ms, var


def measure_peaks(device=None, waves_per_simd: int = 1, scratch_gib: float = 2.0) -> dict:
    """{"mfma_f32_tflops", "mfma_clock_mhz", "copy_gbps"} measured on `device` (include/s2k.h, s2k_measure_peaks)."""
    dev = torch.device(device if device is not None else "cuda")
    buf = torch.empty(int(scratch_gib * (1 << 30)), dtype=torch.uint8, device=dev)
    buf.view(torch.float32)[: (1 << 22)].normal_()
    out = (ctypes.c_double * 3)()
    addr = ctypes.addressof(out)
    with torch.cuda.device(dev):
        check(lib().s2k_measure_peaks(buf.data_ptr(), buf.numel(), waves_per_simd, addr, addr + 8, addr + 16,
                                      torch.cuda.current_stream(dev).cuda_stream))
    return {"mfma_f32_tflops": out[0], "mfma_clock_mhz": out[1], "copy_gbps": out[2]}


CLASSMAP_MODES = {"majority": 0, "boundary": 1}      # modes of s2k_classmap_filter (include/s2k.h)


def classmap_filter(src, src_lut, dst, dims, size: int, mode: int, votes: int, fixed: int, ignore: int, labels, index, lut, nsrc: int,
                    hist, changed, stream: int, src_bytes: int | None = None, dst_bytes: int | None = None) -> int:
    """s2k_classmap_filter (include/s2k.h) as it is: tensors (or None) for the eight pointers, dims = (M, H, W, K); the element widths
    default to the tensors' own.  Returns the library's code; `check` turns it into S2kError.  The library validates every argument
    on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    sb = (8 if src is None else src.element_size()) if src_bytes is None else int(src_bytes)
    db = (8 if dst is None else dst.element_size()) if dst_bytes is None else int(dst_bytes)
    return lib().s2k_classmap_filter(ptr(src), sb, ptr(src_lut), ptr(dst), db, *[int(d) for d in dims], int(size), int(mode),
                                     int(votes) & 0xffffffff, int(fixed) & 0xffffffff, int(ignore), ptr(labels), ptr(index), ptr(lut),
                                     int(nsrc), ptr(hist), ptr(changed), stream)


def classmap_components(src, src_lut, dims, connectivity: int, exclude: int, labels, areas, counts, status, stream: int,
                        src_bytes: int | None = None) -> int:
    """s2k_classmap_components (include/s2k.h) as it is: tensors (or None) for the six pointers, dims = (M, H, W, K).  Returns the
    library's code; the library validates every argument on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    sb = (8 if src is None else src.element_size()) if src_bytes is None else int(src_bytes)
    return lib().s2k_classmap_components(ptr(src), sb, ptr(src_lut), *[int(d) for d in dims], int(connectivity), int(exclude) & 0xffffffff,
                                         ptr(labels), ptr(areas), ptr(counts), ptr(status), stream)


def classmap_sieve(src, src_lut, dst, dims, min_area: int, fixed: int, to: int, labels, areas, best, hist_labels, index, lut, nsrc: int,
                   hist, changed, status, stream: int, src_bytes: int | None = None, dst_bytes: int | None = None) -> int:
    """s2k_classmap_sieve (include/s2k.h) as it is: tensors (or None) for the twelve pointers, dims = (M, H, W, K), to = -1 for the
    donor rule.  Returns the library's code; the library validates every argument on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    sb = (8 if src is None else src.element_size()) if src_bytes is None else int(src_bytes)
    db = (8 if dst is None else dst.element_size()) if dst_bytes is None else int(dst_bytes)
    return lib().s2k_classmap_sieve(ptr(src), sb, ptr(src_lut), ptr(dst), db, *[int(d) for d in dims], int(min_area), int(fixed) & 0xffffffff,
                                    int(to), ptr(labels), ptr(areas), ptr(best), ptr(hist_labels), ptr(index), ptr(lut), int(nsrc), ptr(hist),
                                    ptr(changed), ptr(status), stream)


CLASSMAP_DISTANCE_MODES = {"classes": 0, "boundary": 1}      # site modes of s2k_classmap_distance (include/s2k.h)


def classmap_distance(src, src_lut, dims, mode: int, sites: int, connectivity: int, exclude: int, work, dist2, nearest, other, edges, hist,
                      stream: int, src_bytes: int | None = None, other_bytes: int | None = None, n_edges: int | None = None) -> int:
    """s2k_classmap_distance (include/s2k.h) as it is: tensors (or None) for the seven pointers, dims = (M, H, W, K), `edges` a sequence
    of ints (host memory) or None.  Returns the library's code; the library validates every argument on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    sb = (8 if src is None else src.element_size()) if src_bytes is None else int(src_bytes)
    ob = (8 if other is None else other.element_size()) if other_bytes is None else int(other_bytes)
    ne = (0 if edges is None else len(edges)) if n_edges is None else int(n_edges)
    arr = None if edges is None else (ctypes.c_int * max(len(edges), 1))(*[int(e) for e in edges])
    return lib().s2k_classmap_distance(ptr(src), sb, ptr(src_lut), *[int(d) for d in dims], int(mode), int(sites) & 0xffffffff,
                                       int(connectivity), int(exclude) & 0xffffffff, ptr(work), ptr(dist2), ptr(nearest), ptr(other), ob,
                                       arr, ne, ptr(hist), stream)


def classmap_distance_workspace(M: int, H: int, W: int) -> int:
    """bytes of the `work` buffer of s2k_classmap_distance for M maps of H x W"""
    return int(lib().s2k_classmap_distance_workspace(int(M), int(H), int(W)))


CALIBRATION_MODES = {"probs": 0, "logits": 1}      # what the scores of s2k_calibration are (include/s2k.h)
CALIBRATION_MEASURES = {"max": 0, "margin": 1}     # the written confidence


def calibration(scores, mode: int, labels, label_lut, dims, exclude: int, temps, bins: int, measure: int, reject_below: float,
                reject_to: int, conf, pred, hist, totals, skipped, stream: int, label_bytes: int | None = None,
                pred_bytes: int | None = None, n_temps: int | None = None) -> int:
    """s2k_calibration (include/s2k.h) as it is: tensors (or None) for the eight device pointers, dims = (N, K, P), `temps` a sequence
    of floats (host memory) or None.  Returns the library's code; the library validates every argument on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    lb = (8 if labels is None else labels.element_size()) if label_bytes is None else int(label_bytes)
    pb = (8 if pred is None else pred.element_size()) if pred_bytes is None else int(pred_bytes)
    nt = (0 if temps is None else len(temps)) if n_temps is None else int(n_temps)
    arr = None if temps is None else (ctypes.c_float * max(len(temps), 1))(*[float(t) for t in temps])
    return lib().s2k_calibration(ptr(scores), int(mode), ptr(labels), lb, ptr(label_lut), *[int(d) for d in dims], int(exclude) & 0xffffffff,
                                 arr, nt, int(bins), int(measure), float(reject_below), int(reject_to), ptr(conf), ptr(pred), pb, ptr(hist),
                                 ptr(totals), ptr(skipped), stream)


RASTERIZE_MODES = {"fill": 0, "onto": 1}           # what s2k_rasterize does with a pixel inside no shape (include/s2k.h)
RASTERIZE_BURN = {"value": 0, "index": 1}          # what a shape burns


def rasterize(verts, ring_start, ring_shape, values, origins, dst, dims, mode: int, burn: int, fill: int, work, unfilled, status, stream: int,
              dst_bytes: int | None = None) -> int:
    """s2k_rasterize (include/s2k.h) as it is: tensors (or None) for the nine pointers, dims = (V, R, S, M, H, W); the element width of
    dst defaults to the tensor's own.  Returns the library's code; the library validates every argument on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    V, R, S, M, H, W = (int(d) for d in dims)
    db = (8 if dst is None else dst.element_size()) if dst_bytes is None else int(dst_bytes)
    return lib().s2k_rasterize(ptr(verts), V, ptr(ring_start), ptr(ring_shape), R, ptr(values), S, ptr(origins), M, H, W, ptr(dst), db, int(mode),
                               int(burn), int(fill), ptr(work), ptr(unfilled), ptr(status), stream)


def rasterize_workspace(M: int, S: int) -> int:
    """bytes of the `work` buffer of s2k_rasterize for M tiles and S shapes"""
    return int(lib().s2k_rasterize_workspace(int(M), int(S)))


ZONAL_PAINT_MODES = {"fill": 0, "keep": 1}          # what s2k_zonal_paint does with a pixel it has no value for (include/s2k.h)


def zonal_histogram(zone, zone_stride: int, cls, src_lut, dims, hist, status, stream: int, zone_bytes: int | None = None,
                    cls_bytes: int | None = None) -> int:
    """s2k_zonal_histogram (include/s2k.h) as it is: tensors (or None) for the five pointers, dims = (M, H, W, Z, K); the element widths
    default to the tensors' own.  Returns the library's code; the library validates every argument on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    zb = (4 if zone is None else zone.element_size()) if zone_bytes is None else int(zone_bytes)
    cb = (8 if cls is None else cls.element_size()) if cls_bytes is None else int(cls_bytes)
    return lib().s2k_zonal_histogram(ptr(zone), zb, int(zone_stride), ptr(cls), cb, ptr(src_lut), *[int(d) for d in dims], ptr(hist), ptr(status),
                                     stream)


def zonal_bands(zone, zone_stride: int, vals, dims, nodata, count, total, sumsq, lo, hi, status, stream: int,
                zone_bytes: int | None = None) -> int:
    """s2k_zonal_bands (include/s2k.h) as it is: tensors (or None) for the eight pointers, dims = (M, C, H, W, Z), `nodata` an int or None
    (no value is skipped).  Returns the library's code; the library validates every argument on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    zb = (4 if zone is None else zone.element_size()) if zone_bytes is None else int(zone_bytes)
    return lib().s2k_zonal_bands(ptr(zone), zb, int(zone_stride), ptr(vals), *[int(d) for d in dims], 0 if nodata is None else int(nodata),
                                 0 if nodata is None else 1, ptr(count), ptr(total), ptr(sumsq), ptr(lo), ptr(hi), ptr(status), stream)


def zonal_majority(hist, dims, votes: int, min_count: int, fill: int, out_cls, out_best, stream: int) -> int:
    """s2k_zonal_majority (include/s2k.h) as it is: tensors (or None) for the three pointers, dims = (Z, K).  Returns the library's code;
    the library validates every argument on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    Z, K = (int(d) for d in dims)
    return lib().s2k_zonal_majority(ptr(hist), Z, K, int(votes) & 0xffffffff, int(min_count), int(fill), ptr(out_cls), ptr(out_best), stream)


def zonal_paint(zone, zone_stride: int, table, dims, dst, mode: int, fill: int, status, stream: int, zone_bytes: int | None = None,
                dst_bytes: int | None = None) -> int:
    """s2k_zonal_paint (include/s2k.h) as it is: tensors (or None) for the four pointers, dims = (M, H, W, Z); the element widths default
    to the tensors' own.  Returns the library's code; the library validates every argument on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    zb = (4 if zone is None else zone.element_size()) if zone_bytes is None else int(zone_bytes)
    db = (8 if dst is None else dst.element_size()) if dst_bytes is None else int(dst_bytes)
    return lib().s2k_zonal_paint(ptr(zone), zb, int(zone_stride), ptr(table), *[int(d) for d in dims], ptr(dst), db, int(mode), int(fill),
                                 ptr(status), stream)


MAE_PANELS = {"original": 0, "masked": 1, "pasted": 2, "reconstruction": 3}      # panel codes of s2k_mae_panels (include/s2k.h)


def mae_panels(imgs, pred, mask, norm, bounds, out, patch_mse, dims, bands, frame: int, panels, fill: int, norm_pix: bool,
               stream: int) -> int:
    """s2k_mae_panels (include/s2k.h) as it is: tensors (or None) for the seven pointers, dims = (B, C, T, H, W, P, TUB), `bands`
    three ints, `panels` panel codes.  Returns the library's code; `check` turns it into S2kError.  The library validates every
    argument on the host before it launches."""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    pl = [] if panels is None else [int(c) for c in panels]
    b3 = None if bands is None else (ctypes.c_int * 3)(*[int(b) for b in bands])
    pn = None if panels is None else (ctypes.c_int * max(len(pl), 4))(*pl)
    return lib().s2k_mae_panels(ptr(imgs), ptr(pred), ptr(mask), ptr(norm), ptr(bounds), ptr(out), ptr(patch_mse), *[int(d) for d in dims],
                                b3, int(frame), pn, len(pl), int(fill), int(norm_pix), stream)
