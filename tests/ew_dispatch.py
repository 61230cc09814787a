"""Which kernel a BatchNorm / squeeze-excitation / residual / reduction stage of csrc/ew.hip runs, and which run-time facts of that
kernel a shape exercises, restated in plain Python from the launchers - test infrastructure.

    dispatch(kind, **fields) -> Ew      fields as the stage record names them (tensor fields: anything that is not None counts
                                        as given); Ew.family is the code the launcher leaves in g_s2k_variant (include/s2k.h)
    form(kind, **fields) -> tuple       the structural switches of the record (prologue, fold, EVAL, ...), for coverage tables

Families: 0 the generic kernels (plane_reduce_kernel, plane_map_kernel, se_bn_sums_kernel, bn_bwd_reduce_kernel, the a1 / a2 / b SE
kernels, ...), 11 the wave-per-channel small-plane kernels, 12 the workgroup-per-plane kernels, 13 channel_sum_rows_kernel,
14 se_fc_bwd_small_kernel (SE_FC_BWD reports its data-gradient route), 15 se_fc_wgrad_tile_kernel.
tests/test_ew_dispatch_cpu.py parses csrc/ew.hip for every constant used here and fails when one drifts."""
from __future__ import annotations

from dataclasses import dataclass, field

GENERIC, SMALL, BIG, ROWS, FC_SMALL, WG_TILE = 0, 11, 12, 13, 14, 15

NTHREADS = 256
CHUNK = 4096                 # elements of a plane one wave of the chunked kernels handles
SMALL_HW = {"SE_POOL": 256, "BN_RESIDUAL": 256, "SE_BN_SUMS": 64, "BN_BWD_APPLY": 64}    # HW <= ..., HW % 4 == 0, B > 1
SMALL_WAVES = 2048           # bsplit = min(cdiv(B, planes per pass), cdiv(SMALL_WAVES, C))
SMALL_UNROLL = 4             # passes in flight in se_bn_sums_small_kernel / bn_bwd_apply_small_kernel
BIG_HW = 4096                # HW >= ..., HW % 4 == 0, B * C <= BIG_PLANES
BIG_PLANES = 8192
ROWS_C, ROWS_HW = 256, 512   # channel_sum_rows_kernel: C >= ROWS_C and HW <= ROWS_HW
ROWS_UNROLL = 8              # rows in flight per wave (rows b, b + 4, ..., b + 28)
FC_SMALL_Q = 64              # se_fc_bwd_small_kernel: Q <= ...
SEW_QMAX, SEW_BT, SEW_CT = 224, 32, 8
REP_SCALAR = 8               # bn_fold_wave / bn_fuse_sums: nrep <= ... is a loop of wave-uniform loads, beyond a lane loop + wave sum


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


@dataclass(frozen=True)
class Ew:
    family: int
    kernels: tuple                 # the instantiations launched, e.g. ("plane_reduce_kernel<0, true>",)
    vec: bool = False              # float4 body (False: scalar)
    # wave-per-channel small-plane kernels
    lpp: int = 0                   # lanes per plane
    pp: int = 0                    # planes (samples) per pass
    bsplit: int = 0                # batch chunks = gridDim.y
    bper: int = 0                  # samples per chunk
    idle_lanes: bool = False       # lanes of a group beyond the plane (4 * li >= HW)
    last_short: bool = False       # the last batch chunk holds fewer samples than the others
    last_empty: bool = False       # ... none at all
    ragged_pass: bool = False      # a chunk whose last pass is not full (samples % pp != 0)
    partial_unroll: bool = False   # a chunk whose passes are no multiple of SMALL_UNROLL
    full_unroll: bool = False      # a chunk with at least SMALL_UNROLL passes
    # chunked kernels
    chunks: int = 1                # tasks per plane
    last_chunk: int = 0            # elements of the last one
    # workgroup-per-plane kernels: trips of thread 0 and how many threads take a tail trip
    main_trips: int = 0
    tail_trips: int = 0
    tail_threads: int = 0
    idle_workgroup_waves: bool = False     # B * C > 4 (most planes are not the folded writer's: plane >= C)
    # replica / batch lane loops
    rep_path: str = ""             # "scalar" | "wave" ("" where no replicas are read)
    rep_trips: int = 0             # trips of the lane loop (wave path, BN_FINALIZE, BN_BWD_FINALIZE, SE_BN_COMBINE, PS sums)
    # channel_sum_rows_kernel: per wave (unrolled trips, tail trips)
    rows_waves: tuple = ()
    # se_fc_wgrad_tile_kernel
    sample_chunks: int = 0
    last_samples: int = 0
    ragged_ctile: bool = False
    extra: dict = field(default_factory=dict, compare=False)

    @property
    def mixed_rows(self) -> bool:
        """some waves take the 8-row unrolled loop, others only the tail"""
        return any(u for u, _ in self.rows_waves) and any(not u for u, _ in self.rows_waves)


def _given(v) -> bool:
    return v is not None and not (isinstance(v, int) and v < 0)


def _small(kind, B, C, HW):
    """geometry of the wave-per-channel kernels, or None when the launcher does not take them"""
    if HW > SMALL_HW[kind] or HW % 4 or B < 2:
        return None
    lpp = 1
    while 4 * lpp < HW:
        lpp <<= 1
    pp = 64 // lpp
    bsplit = max(1, min(cdiv(B, pp), cdiv(SMALL_WAVES, C)))
    bper = cdiv(B, bsplit)
    sizes = [max(0, min(B, (y + 1) * bper) - y * bper) for y in range(bsplit)]
    passes = [cdiv(n, pp) for n in sizes if n]
    return dict(lpp=lpp, pp=pp, bsplit=bsplit, bper=bper, idle_lanes=4 * lpp > HW, last_short=0 < sizes[-1] < bper, last_empty=sizes[-1] == 0,
                ragged_pass=any(n % pp for n in sizes), partial_unroll=any(p % SMALL_UNROLL for p in passes),
                full_unroll=any(p >= SMALL_UNROLL for p in passes))


def _big(HW):
    """trips of se_pool_big_kernel / se_bn_sums_big_kernel: `for (; i + 256 < n4; i += 512)` then `for (; i < n4; i += 256)`"""
    n4 = HW // 4

    def trips(t):
        i, m, k = t, 0, 0
        while i + NTHREADS < n4:
            i += 2 * NTHREADS
            m += 1
        while i < n4:
            i += NTHREADS
            k += 1
        return m, k
    m0, k0 = trips(0)
    return dict(main_trips=m0, tail_trips=k0, tail_threads=sum(1 for t in range(NTHREADS) if trips(t)[1]))


def _chunks(HW):
    n = cdiv(HW, CHUNK)
    return dict(chunks=n, last_chunk=HW - (n - 1) * CHUNK)


def _rep(nrep):
    nrep = max(int(nrep or 0), 1)
    return dict(rep_path="scalar" if nrep <= REP_SCALAR else "wave", rep_trips=cdiv(nrep, 64))


def _tf(v: bool) -> str:
    return "true" if v else "false"


def dispatch(kind: str, **f) -> Ew:
    B, C, HW = f.get("B"), f.get("C"), f.get("HW")
    vec = HW is not None and HW % 4 == 0
    if kind == "SE_POOL":
        rep = _rep(f.get("FNREP")) if _given(f.get("FSTATS")) else {}
        if HW >= BIG_HW and vec and B * C <= BIG_PLANES:
            return Ew(BIG, ("se_pool_big_kernel",), True, idle_workgroup_waves=B * C > 4, **_big(HW), **rep)
        g = _small(kind, B, C, HW)
        if g:
            return Ew(SMALL, ("se_pool_small_kernel",), True, **g, **rep)
        return Ew(GENERIC, (f"plane_reduce_kernel<0, {_tf(vec)}>",), vec, **rep)
    if kind == "SE_BWD_REDUCE":
        return Ew(GENERIC, (f"plane_reduce_kernel<1, {_tf(vec)}>",), vec)
    if kind == "CHANNEL_SUM":
        if B > 0 and C >= ROWS_C and 0 < HW <= ROWS_HW:
            waves = []
            for w in range(4):
                b, u, t = w, 0, 0
                while b + 4 * (ROWS_UNROLL - 1) < B:
                    b += 4 * ROWS_UNROLL
                    u += 1
                while b < B:
                    b += 4
                    t += 1
                waves.append((u, t))
            return Ew(ROWS, ("channel_sum_rows_kernel",), False, rows_waves=tuple(waves))
        return Ew(GENERIC, (f"plane_reduce_kernel<2, {_tf(vec)}>",), vec, **_chunks(HW))
    if kind == "SE_BN_SUMS":
        if HW >= BIG_HW and vec and B * C <= BIG_PLANES:
            return Ew(BIG, ("se_bn_sums_big_kernel",), True, idle_workgroup_waves=B * C > 4, **_big(HW))
        g = _small(kind, B, C, HW)
        if g:
            return Ew(SMALL, ("se_bn_sums_small_kernel",), True, **g)
        return Ew(GENERIC, (f"se_bn_sums_kernel<{_tf(vec)}>",), vec)
    if kind == "SE_BN_COMBINE":
        return Ew(GENERIC, ("se_bn_combine_kernel",), rep_trips=cdiv(B, 64))
    if kind == "SE_FC":
        return Ew(GENERIC, ("se_fc1_kernel", "se_fc2_kernel"))
    if kind in ("SE_FC_BWD", "SE_FC_WGRAD"):
        Q = f["CSQ"]
        tile = Q <= SEW_QMAX
        wg = dict(sample_chunks=cdiv(B, SEW_BT), last_samples=B - (cdiv(B, SEW_BT) - 1) * SEW_BT, ragged_ctile=C % SEW_CT != 0) if tile else {}
        pk = "se_fc_wgrad_tile_kernel" if tile else "se_fc_bwd_b_kernel"
        if kind == "SE_FC_WGRAD":
            return Ew(WG_TILE if tile else GENERIC, (pk,), **wg)
        params = _given(f.get("DW1"))
        small = Q <= FC_SMALL_Q
        ks = ("se_fc_bwd_small_kernel",) if small else ("se_fc_bwd_a1_kernel", "se_fc_bwd_a2_kernel")
        return Ew(FC_SMALL if small else GENERIC, ks + ((pk,) if params else ()), **(wg if params else {}))
    if kind == "BN_BWD_REDUCE":
        return Ew(GENERIC, (f"bn_bwd_reduce_kernel<{_tf(vec)}>",), vec, **_chunks(HW))
    if kind == "BN_BWD_FINALIZE":
        return Ew(GENERIC, ("bn_bwd_finalize_kernel",), rep_trips=cdiv(max(f.get("NREP") or 0, 1), 64))
    if kind == "BN_FINALIZE":
        return Ew(GENERIC, ("bn_finalize_kernel",), rep_trips=cdiv(max(f.get("NREP") or 0, 1), 64) if f.get("TRAIN") else 0)
    if kind == "BN_BWD_APPLY":
        if _given(f.get("COEF")):
            return Ew(GENERIC, (f"plane_map_kernel<0, {_tf(vec)}>",), vec, **_chunks(HW))
        ps = _given(f.get("PS"))
        rep = dict(rep_path="wave", rep_trips=cdiv(B, 64)) if ps else _rep(f.get("NREP"))
        out16 = bool(f.get("OUT_BF16"))
        recompute = bool(f.get("ACT")) or _given(f.get("MULBC")) or _given(f.get("ADDBC"))
        mode = 3 if recompute else 2
        g = _small(kind, B, C, HW)
        if g:
            return Ew(SMALL, (f"bn_bwd_apply_small_kernel<{mode}{', true' if out16 else ''}>",), True, **g, **rep)
        if out16:
            return Ew(GENERIC, ("plane_map_kernel<2, true, true>",), True, **_chunks(HW), **rep)
        return Ew(GENERIC, (f"plane_map_kernel<{mode}, {_tf(vec)}>",), vec, **_chunks(HW), **rep)
    if kind == "BN_RESIDUAL":
        rep = _rep(f.get("FNREP")) if _given(f.get("FSTATS")) else {}
        g = _small(kind, B, C, HW)
        if g:
            return Ew(SMALL, ("bn_residual_small_kernel",), True, **g, **rep)
        return Ew(GENERIC, (f"plane_map_kernel<1, {_tf(vec)}>",), vec, **_chunks(HW), **rep)
    if kind == "UPSAMPLE_ZERO":
        total = B * C * f["HO"] * f["WO"]
        return Ew(GENERIC, ("upsample_zero_kernel",), extra=dict(trips=cdiv(cdiv(total, 256), min(cdiv(total, 256), 65536)),
                                                                trailing=f["HO"] > f["S"] * f["H"] or f["WO"] > f["S"] * f["W"]))
    raise KeyError(kind)


KINDS = ("BN_FINALIZE", "SE_POOL", "SE_FC", "SE_FC_BWD", "SE_FC_WGRAD", "SE_BWD_REDUCE", "SE_BN_SUMS", "SE_BN_COMBINE", "BN_BWD_REDUCE",
         "BN_BWD_FINALIZE", "BN_BWD_APPLY", "BN_RESIDUAL", "CHANNEL_SUM", "UPSAMPLE_ZERO")


def form(kind: str, **f) -> tuple:
    """the switches of a record that select code inside a kernel (not its shape)"""
    g = lambda k: _given(f.get(k))      # noqa: E731
    if kind == "SE_POOL":
        return (f.get("PRO") or 0, "fold" if g("FSTATS") else "bnv")
    if kind == "SE_BWD_REDUCE":
        return (f.get("PRO") or 0,)
    if kind == "BN_BWD_REDUCE":
        return (f.get("ACT") or 0, "mul" if g("MULBC") else "", "add" if g("ADDBC") else "", "noise" if g("NOISE") else "")
    if kind == "BN_BWD_APPLY":
        if g("COEF"):
            return ("coef",)
        return ("fused", f.get("ACT") or 0, "mul" if g("MULBC") else "", "add" if g("ADDBC") else "", "ps" if g("PS") else "st2",
                "eval" if f.get("EVAL") else "train", "bf16" if f.get("OUT_BF16") else "f32")
    if kind == "BN_RESIDUAL":
        return ("ident" if g("IDENT") else "", "noise" if g("NOISE") else "", "fold" if g("FSTATS") else "bnv")
    if kind == "BN_FINALIZE":
        return ("train" if f.get("TRAIN") else "eval",)
    if kind == "SE_BN_COMBINE":
        return ("mul" if g("MULBC") else "", "add" if g("ADDBC") else "")
    if kind == "SE_FC_BWD":
        return ("params" if g("DW1") else "split",)
    if kind == "UPSAMPLE_ZERO":
        return (f["S"],)
    return ()


def facts(kind: str, **f) -> tuple:
    """what a cut-down production row must keep: the family, the kernels, and the loop facts that the plane size, the replica
    count, the batch lane loops and the SE sample chunks decide - float4 / scalar body, lanes per plane and idle lanes, chunks per
    plane and the last one's length, main / tail trips of the workgroup-per-plane kernels, replica path and lane-loop trips, the
    per-wave trips of channel_sum_rows_kernel, SE sample chunks.  (How the wave-per-channel kernels split the BATCH - bsplit, bper,
    short / empty chunks, ragged and partial passes - depends on B and C themselves: those edges are the hand tables' rows.)"""
    d = dispatch(kind, **f)
    return (d.family, d.kernels, d.vec, d.lpp, d.idle_lanes, d.chunks, d.last_chunk, d.main_trips, d.tail_trips, d.tail_threads, d.rep_path,
            d.rep_trips, d.rows_waves, d.sample_chunks)
