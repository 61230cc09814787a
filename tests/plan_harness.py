"""Run planned s2k programs through the CPU emulator (oracle/ops_ref.py) — test infrastructure."""
from __future__ import annotations

import numpy as np
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd.plan import opdefs as D
from oracle import ops_ref
from tests import pack_ref as _PR
from tests import stream_order as _SO

NARROW = (D.BASE["CONST"],)


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().reshape(-1).view(torch.uint8)


def make_bases(plan, flat_params, flat_bufs, x, noise, n_out, wide: bool = False):
    """wide: hold every f32 tensor as float64 (see ops_ref.Mem)."""
    fd = torch.float64 if wide else torch.float32
    k = 2 if wide else 1
    pad8 = lambda n: (n + 7) // 8 * 8  # noqa: E731
    bases = {
        D.BASE["WS"]: torch.zeros(k * pad8(plan.ws_bytes) + 64, dtype=torch.uint8),
        D.BASE["AUX"]: torch.zeros(k * pad8(plan.aux_bytes) + 64, dtype=torch.uint8),
        D.BASE["PARAMS"]: _bytes(flat_params.detach().to(fd).clone()),
        D.BASE["GRADS"]: _bytes(torch.zeros_like(flat_params, dtype=fd)),
        D.BASE["WGS"]: _bytes(torch.zeros_like(flat_params, dtype=fd)),
        D.BASE["BUFS"]: _bytes(flat_bufs.detach().to(fd).clone()),
        D.BASE["X"]: _bytes(x.to(fd).clone()),
        D.BASE["OUT"]: _bytes(torch.zeros(n_out, dtype=fd)),
        D.BASE["DOUT"]: _bytes(torch.zeros(n_out, dtype=fd)),
        D.BASE["NOISE"]: _bytes(noise.clone().to(fd)),
        D.BASE["CONST"]: _bytes(torch.tensor(plan.const_table if plan.const_table else [0] * 8, dtype=torch.int32)),
        D.BASE["WPACK"]: torch.zeros(k * pad8(plan.wpack_bytes) + 64, dtype=torch.uint8),
        D.BASE["DX"]: _bytes(torch.full(tuple(x.shape), float("nan"), dtype=fd)),
    }
    # poison the workspace so that reads of never-written memory show up as NaN
    bases[D.BASE["WS"]][: k * pad8(plan.ws_bytes)].view(fd).fill_(float("nan"))
    return bases


def fview(bases, name: str, wide: bool = False) -> torch.Tensor:
    return bases[D.BASE[name]].view(torch.float64 if wide else torch.float32)


def emulate(packed: np.ndarray, bases, wide: bool = False) -> None:
    ops_ref.run_program(packed, bases, D, wide=wide, narrow_bases=NARROW)


def make_bases_vit(plan, flat_params, flat_bufs, x, noise_f32: torch.Tensor, wide: bool = False):
    """Bases for a VitPlan (plan/vit_plan.py): OUT / DOUT / NOISE are sized from the plan."""
    fd = torch.float64 if wide else torch.float32
    k = 2 if wide else 1
    pad8 = lambda n: (n + 7) // 8 * 8  # noqa: E731
    n_dout = int(np.prod(plan.dout_shape))
    nz = torch.zeros(plan.noise_bytes // 4, dtype=fd)
    nz[: noise_f32.numel()] = noise_f32.reshape(-1).to(fd)
    bases = {
        D.BASE["WS"]: torch.zeros(k * pad8(plan.ws_bytes) + 64, dtype=torch.uint8),
        D.BASE["AUX"]: torch.zeros(k * pad8(plan.aux_bytes) + 64, dtype=torch.uint8),
        D.BASE["PARAMS"]: _bytes(flat_params.detach().to(fd).clone()),
        D.BASE["GRADS"]: _bytes(torch.zeros_like(flat_params, dtype=fd)),
        D.BASE["WGS"]: _bytes(torch.zeros_like(flat_params, dtype=fd)),
        D.BASE["BUFS"]: _bytes(flat_bufs.detach().to(fd).clone()),
        D.BASE["X"]: _bytes(x.to(fd).clone()),
        D.BASE["OUT"]: torch.zeros(k * pad8(plan.out_bytes) + 64, dtype=torch.uint8),
        D.BASE["DOUT"]: (torch.zeros(k * pad8(plan.dout_bytes) + 64, dtype=torch.uint8) if getattr(plan, "dout_bytes", 0)
                         else _bytes(torch.zeros(n_dout, dtype=fd))),
        D.BASE["DX"]: torch.zeros(k * pad8(x.numel() * 4) + 64, dtype=torch.uint8),
        D.BASE["NOISE"]: _bytes(nz),
        D.BASE["CONST"]: _bytes(torch.tensor(plan.const_table if plan.const_table else [0] * 8, dtype=torch.int32)),
        D.BASE["WPACK"]: torch.zeros(k * pad8(plan.wpack_bytes) + 64, dtype=torch.uint8),
    }
    bases[D.BASE["WS"]][: k * pad8(plan.ws_bytes)].view(fd).fill_(float("nan"))
    return bases


def flat_from_state(layout, sd, dtype=torch.float32):
    """Flat parameter / buffer vectors in the plan's layout from a reference-named state dict."""
    fp = torch.zeros(layout.n_params, dtype=dtype)
    fb = torch.zeros(max(layout.n_bufs, 1), dtype=dtype)
    for name, (off, shape) in layout.params.items():
        fp[off:off + int(np.prod(shape))] = sd[name].detach().reshape(-1).to(dtype)
    for name, (off, shape) in layout.bufs.items():
        fb[off:off + int(np.prod(shape))] = sd[name].detach().reshape(-1).to(dtype)
    return fp, fb


def out_view(bases, tref, wide: bool = False) -> torch.Tensor:
    """A tensor of the OUT base (any dtype) of a VitPlan."""
    mem = ops_ref.Mem(bases, wide, NARROW)
    return mem.view(tref.ref, tref.shape, tref.dtype)


def method_bases(plan, fp, fb, inputs: dict, noise: dict, wide=True):
    """Packed X / NOISE / DOUT / DX bases of a MethodPlan (plan/vit_plan.py) for the emulator: (bases, Mem over them)."""
    shim = type("P", (), dict(ws_bytes=plan.ws_bytes, aux_bytes=plan.aux_bytes, out_bytes=plan.out_bytes, noise_bytes=max(plan.noise_bytes, 4),
                              dout_shape=(1,), const_table=plan.const_table, wpack_bytes=plan.wpack_bytes))()
    bases = make_bases_vit(shim, fp, fb, torch.zeros(1), torch.zeros(1), wide)
    k = 2 if wide else 1
    for base, size in (("X", plan.x_bytes), ("DOUT", plan.dout_bytes), ("DX", plan.dx_bytes), ("NOISE", max(plan.noise_bytes, 8))):
        bases[D.BASE[base]] = torch.zeros(k * ((size + 7) // 8 * 8) + 64, dtype=torch.uint8)
    m = ops_ref.Mem(bases, wide, NARROW)
    for name, t in inputs.items():
        r = plan.inputs[name]
        m.view(r.ref, r.shape, r.dtype).copy_(t)
    for name, t in noise.items():
        r = plan.noise[name]
        m.view(r.ref, r.shape, r.dtype).copy_(t)
    return bases, m


# ---------------------------------------------------------------------------------------------------------------------------------
# Stage-by-stage comparison of a planned program's GPU run with its emulation (tests/test_vit_stages_gpu.py; the CPU half is
# exercised by tests/test_vit_stage_cover_cpu.py).  An IMAGE is {base id: flat uint8 CPU tensor}; a WIDE image holds every f32
# tensor as float64 at twice its offset (ops_ref.Mem).  Which bytes a record writes comes from tests/stream_order.footprint: the
# slots of opdefs.WRITES, BNV / FRM / FRV of a foldable kind only when it folds, byte exact through the CONST tables.
# ---------------------------------------------------------------------------------------------------------------------------------
_TDT = {"f32": torch.float32, "f64": torch.float64, "i64": torch.int64, "i32": torch.int32, "i16": torch.int16, "u8": torch.uint8}
MUTABLE = ("WS", "AUX", "OUT", "GRADS", "BUFS", "DX", "WGS", "WPACK")       # the bases a program may write

# The bar of a stage kind, max |a - b| / max |b| over the tensor.  Every number is the one the kind's own op test uses:
#   tests/test_vit_kernels_gpu.py (docstring): LayerNorm forward 2e-5, backward 1e-4; attention 1e-4 / 2e-4; MAE loss 2e-5 (and
#       PATCHIFY INVERSE 4, the loss target's gradient); activations 1e-5
#   tests/test_ops_gpu.py: CONV 1e-4, WGRAD 2e-4, CHANNEL_SUM 1e-4, the BatchNorm stages of the head 1e-4; AXPY 1e-7
#   tests/test_vit_ops_gpu.py: TOKEN_GATHER with POS 1e-6, TOKEN_SCATTER 1e-5
#   tests/test_pack_kernels_gpu.py: WGRAD_FINALIZE adds once (1e-7, one f32 rounding against float64)
# 0.0 = bit for bit: index outputs and data movement.
OP_BAR = {
    "CHAN_LN_FWD": 2e-5, "CHAN_LN_BWD": 1e-4, "ATTN_FWD": 1e-4, "ATTN_BWD": 2e-4, "MAE_LOSS_FWD": 2e-5, "MAE_LOSS_BWD": 2e-5,
    "ACT_FWD": 1e-5, "ACT_BWD": 1e-5, "CONV": 1e-4, "WGRAD": 2e-4, "CHANNEL_SUM": 1e-4, "BN_FINALIZE": 1e-4, "BN_BWD_REDUCE": 1e-4,
    "BN_BWD_FINALIZE": 1e-4, "BN_BWD_APPLY": 1e-4, "AXPY": 1e-7, "WGRAD_FINALIZE": 1e-7, "TOKEN_SCATTER": 1e-5,
    "MAE_MASK_INDEX": 0.0, "IDS_TO_DEC_IDX": 0.0, "TRANSPOSE_CL": 0.0, "SPACE_TO_DEPTH": 0.0, "MEMSET": 0.0, "WEIGHT_PACK": 0.0,
    "DROP_GATE": 0.0, "UPSAMPLE_ZERO": 0.0, "IM2COL": 0.0,
}
# Stages that move values or add once.  In a WHOLE program such a stage cannot be held tighter than the tensor it moves: there it
# inherits the bars of the records of the same program that wrote what it reads (bit for bit when nothing it reads was computed).
TRANSPARENT = ("TRANSPOSE_CL", "SPACE_TO_DEPTH", "TOKEN_GATHER", "TOKEN_SCATTER", "PATCHIFY", "AXPY", "WGRAD_FINALIZE", "UPSAMPLE_ZERO", "IM2COL")
# Written slots whose CONTENT the stage's contract leaves open; they count as written, are not compared, and unspecified_reads()
# asserts that nothing else reads them:
#   CONV.SCRATCH - opdefs.py: "lets the kernel cut a long reduction over few output tiles into split-K partials that a tail kernel
#   adds" (the emulator never writes it).
UNSPECIFIED = {("CONV", "SCRATCH")}
# [NREP][2][C] statistics: opdefs.py, "a workgroup adds into replica (its id % NREP) and the finalize stages sum the replicas" - the
# emulator adds into replica 0.  Compared after summing the replicas; unspecified_reads() asserts the readers are the summing slots.
REPLICATED = ("STATS", "STATS2")
REPLICA_READERS = ("STATS", "STATS2", "FSTATS")


def op_bar(kind: str, f: dict, slot: str) -> float:
    t = f[slot]
    if t.dtype not in ("f32", "f64"):
        return 0.0
    if kind == "TOKEN_GATHER":
        return 0.0 if f.get("POS") is None else 1e-6
    if kind == "PATCHIFY":      # 0 / 1 copy, 2 negates: exact; 3 adds once; 4 is arithmetic
        return {0: 0.0, 1: 0.0, 2: 0.0, 3: 1e-7, 4: 2e-5}[f.get("INVERSE", 0)]
    return OP_BAR[kind]


def slot_writes(kind: str, f: dict, blob) -> list:
    """[(slot, TRef, (n, 2) byte intervals)] of what one record writes"""
    out = []
    for w in D.WRITES[kind]:
        if not isinstance(f.get(w), _SO.TRef):
            continue
        alone = {k: (None if (k in D.WRITES[kind] and k != w) else v) for k, v in f.items()}
        iv = _SO.footprint(kind, alone, blob).writes.get(f[w].base)
        if iv is not None and len(iv):
            out.append((w, f[w], iv))
    return out


def written_ranges(prog, blob, begin: int = 0, end: int | None = None) -> dict:
    """{base id: (n, 2) sorted disjoint byte intervals} that records [begin, end) of a program write"""
    pieces: dict = {}
    for kind, f in prog.ops[begin:end]:
        for _, t, iv in slot_writes(kind, f, blob):
            pieces.setdefault(t.base, []).append((iv[:, 0], iv[:, 1]))
    return {b: _SO._merge(p) for b, p in pieces.items()}


def typed_refs(plan) -> list:
    """every tensor reference of a plan that is not f32: the regions a wide image holds as they are"""
    refs = {}
    groups = [getattr(plan, n, None) or {} for n in ("tensors", "outputs", "inputs", "noise", "douts", "dins")]
    every = [t for g in groups for t in g.values()]
    for prog in (plan.fwd, plan.bwd):
        every += [v for _, f in (prog.ops if prog is not None else ()) for v in f.values()]
    for t in every:
        if isinstance(t, _SO.TRef) and t.dtype != "f32":
            refs[(t.base, t.off, t.nbytes)] = t
    return list(refs.values())


def widen(image: dict, refs) -> dict:
    """the wide image of an f32 image: f32 -> f64 at twice the offset, the tensors of `refs` (typed_refs) copied as they are"""
    wide = {}
    for b, img in image.items():
        if b in NARROW:
            wide[b] = img.clone()
            continue
        n = img.numel() // 4 * 4
        w = torch.zeros(2 * n + 64, dtype=torch.uint8)
        w[:2 * n].view(torch.float64).copy_(img[:n].view(torch.float32))
        for t in refs:
            if t.base == b and t.off + t.nbytes <= n:
                w[2 * t.off:2 * t.off + t.nbytes] = img[t.off:t.off + t.nbytes]
        wide[b] = w
    return wide


def _take(img: torch.Tensor, iv, dtype: str, wide: bool) -> torch.Tensor:
    """the elements of byte intervals `iv` of an image (wide: of the wide image, f32 read as float64)"""
    k = 2 if wide else 1
    dt = torch.float64 if (wide and dtype == "f32") else _TDT[dtype]
    grow = 2 if (wide and dtype == "f32") else 1
    parts = [img[k * int(lo):k * int(lo) + grow * int(hi - lo)] for lo, hi in iv]
    flat = parts[0] if len(parts) == 1 else torch.cat(parts)
    return flat.view(dt)


def _subtract(iv: np.ndarray, cut: np.ndarray) -> np.ndarray:
    """sorted disjoint intervals `iv` minus the intervals `cut`"""
    out = []
    for lo, hi in iv.tolist():
        for clo, chi in cut.tolist():
            if chi <= lo or clo >= hi:
                continue
            if clo > lo:
                out.append((lo, clo))
            lo = max(lo, chi)
            if lo >= hi:
                break
        if lo < hi:
            out.append((lo, hi))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


class StageReport:
    def __init__(self):
        self.worst: dict = {}        # kind -> (error against the f32 emulator, against float64 or None, bar, E or None)
        self.nonfinite: list = []    # (kind, slot): the emulator's value is not finite (the GPU's is held to the same positions)
        self.wlog: list = []         # (base, lo, hi, bar without E): every compared write, for the per-parameter gradient bars
        self.fails: list = []
        self.compared = 0

    def note(self, kind, e32, e64, bar, E):
        old = self.worst.get(kind)
        if old is None or max(e32, e64 or 0.0) >= max(old[0], old[1] or 0.0):
            self.worst[kind] = (e32, e64, bar, E)

    def check(self, what=""):
        assert not self.fails, f"{what}: {len(self.fails)} written ranges off, first: " + "; ".join(self.fails[:6])


def _weight_pack_check(rep, f, blob, gpu, emu32, copies=True):
    """WEIGHT_PACK against tests/pack_ref.py, every copy bit for bit (the emulator models the f32 pack only; copies=False: the image
    under test is an emulator's, so only the f32 pack is asked of it)"""
    rows = _SO.table_rows(blob, f["TABLE"], f["N_ENTRIES"], 12)
    src, dst = f["SRC"], f["DST"]
    params = gpu[src.base][src.off:].view(torch.float32).numpy()
    got = gpu[dst.base].numpy()
    for off, want in (_PR.weight_pack_writes(rows, params, int(f.get("BF16_BASE") or 0), int(f.get("Q4_BASE") or 0), int(f.get("SPLIT_BASE") or 0))
                      if copies else _PR.f32_pack(rows, params)):
        a = dst.off + off
        rep.compared += 1
        if not np.array_equal(got[a:a + want.size], want):
            rep.fails.append(f"WEIGHT_PACK: bytes {a}..{a + want.size} of {D.BASES[dst.base]} differ from the layout reference")
    for off, want in _PR.f32_pack(rows, params):
        a = dst.off + off
        if not np.array_equal(emu32[dst.base].numpy()[a:a + want.size], want):
            rep.fails.append(f"WEIGHT_PACK: the emulator's f32 pack at byte {a} differs from the layout reference")
    rep.note("WEIGHT_PACK", 0.0, 0.0, 0.0, None)


def compare_written(prog, blob, gpu: dict, emu32: dict, emu64: dict | None = None, before: dict | None = None, whole: bool = True,
                    begin: int = 0, end: int | None = None, rep: StageReport | None = None, pack_copies: bool = True) -> StageReport:
    """Every byte range records [begin, end) of `prog` write: the GPU image against the f32 emulator's and (emu64) the wide one's.
    Bit for bit where the bar is 0; otherwise max |a - b| / max |b| over the range, against both emulators, below
        whole = False (one stage from the GPU's own state): the op bar of the writing kind;
        whole = True: max(op bar, 8 E), E = the f32 emulator's own distance from float64 in that range (the `stress` rule of
                      tests/test_vit_kernels_gpu.py::_check), the op bar alone without emu64; TRANSPARENT kinds inherit the bars of
                      what they read.
    The GPU's value must be finite exactly where the emulator's is; ranges with non-finite emulator values are listed in the report.
    The whole declared range is compared, row padding included.  before: images from before the records ran - every byte of them
    outside the written ranges must be unchanged in `gpu`.  Failures are collected: call report.check()."""
    rep = rep or StageReport()
    end = len(prog.ops) if end is None else end
    todo = []                # (record, kind, slot, TRef, intervals, bar before E): first every record's bar, then the comparisons
    for i in range(begin, end):
        kind, f = prog.ops[i]
        inherit = 0.0
        if whole and kind in TRANSPARENT:
            reads = _SO.footprint(kind, f, blob).reads
            for b, lo, hi, bar in rep.wlog:
                iv = reads.get(b)
                if iv is not None and len(iv) and bool(((iv[:, 0] < hi) & (iv[:, 1] > lo)).any()):
                    inherit = max(inherit, bar)
        if kind == "WEIGHT_PACK":
            _weight_pack_check(rep, f, blob, gpu, emu32, pack_copies)
            continue
        for slot, t, iv in slot_writes(kind, f, blob):
            if t.base not in gpu:
                continue
            base_bar = max(op_bar(kind, f, slot), inherit) if t.dtype in ("f32", "f64") else 0.0
            for lo, hi in (iv.tolist() if len(iv) <= 64 else [(iv[0, 0], iv[-1, 1])]):
                rep.wlog.append((t.base, int(lo), int(hi), base_bar))
            todo.append((i, kind, slot, t, iv, base_bar))
    for n, (i, kind, slot, t, iv, base_bar) in enumerate(todo):
        if (kind, slot) in UNSPECIFIED:
            continue
        later = [e for e in todo[n + 1:] if e[3].base == t.base and e[4][0, 0] < iv[-1, 1] and e[4][-1, 1] > iv[0, 0]]
        where = f"#{i} {kind}.{slot} ({t.name or D.BASES[t.base]} @{t.off})"
        rep.compared += 1
        if kind == "MEMSET":
            # zero bytes, whatever tensor type the planner clears; what a later record of the program accumulates into is compared there
            rest = _SO._merge([(iv[:, 0], iv[:, 1])])
            for e in later:
                rest = _subtract(rest, e[4])
            if any(bool(img[t.base][k * int(lo):k * int(hi)].any()) for lo, hi in rest for img, k in ((gpu, 1), (emu32, 1)) + (((emu64, 2),) if emu64 is not None else ())):
                rep.fails.append(f"{where}: not zero")
            rep.note(kind, 0.0, 0.0 if emu64 is not None else None, 0.0, None)
            continue
        # what a later record of the same program writes again (an in-place update, an accumulation) is held to the larger bar
        base_bar = max([base_bar] + [e[5] for e in later]) if t.dtype in ("f32", "f64") else 0.0
        a = _take(gpu[t.base], iv, t.dtype, False)
        b = _take(emu32[t.base], iv, t.dtype, False)
        c = _take(emu64[t.base], iv, t.dtype, True) if emu64 is not None else None
        if t.dtype not in ("f32", "f64"):
            if not torch.equal(a, b) or (c is not None and not torch.equal(a, c)):
                rep.fails.append(f"{where}: integer output differs")
            rep.note(kind, 0.0, 0.0 if c is not None else None, 0.0, None)
            continue
        if slot in REPLICATED and t.dtype == "f64" and len(t.shape) == 3:
            a, b = a.view(t.shape).sum(0), b.view(t.shape).sum(0)
            c = c.view(t.shape).sum(0) if c is not None else None
        a, b = a.double().reshape(-1), b.double().reshape(-1)
        c = c.double().reshape(-1) if c is not None else None
        fin = torch.isfinite(b)
        if not torch.equal(torch.isfinite(a), fin) or (c is not None and not torch.equal(torch.isfinite(c), fin)):
            rep.fails.append(f"{where}: finite at different positions (GPU {int((~torch.isfinite(a)).sum())} non-finite, emulator {int((~fin).sum())})")
            continue
        if not bool(fin.all()):
            rep.nonfinite.append((kind, slot))
            if not torch.equal(torch.isnan(a), torch.isnan(b)):
                rep.fails.append(f"{where}: NaN at different positions")
                continue
            if not bool(fin.any()):
                continue
            a, b, c = a[fin], b[fin], (c[fin] if c is not None else None)
        e32 = _rel(a, b)
        e64 = _rel(a, c) if c is not None else None
        E = _rel(b, c) if c is not None else None
        if base_bar == 0.0:      # the f32 emulator's values exactly; float64's within one f32 rounding (DROP_GATE divides once)
            ok = torch.equal(a, b) and (c is None or bool(((a - c).abs() <= 2.0 ** -23 * c.abs()).all()))
            bar = 0.0
        else:
            bar = max(base_bar, 8 * E) if (whole and E is not None) else base_bar
            ok = e32 < bar and (e64 is None or e64 < bar)
        rep.note(kind, e32, e64, bar, E)
        if not ok:
            rep.fails.append(f"{where}: rel err {e32:.3e} (f32 emulator) {e64 if e64 is None else format(e64, '.3e')} (float64), bar {bar:.1e}")
    if before is not None:
        wr = written_ranges(prog, blob, begin, end)
        for b, was in before.items():
            now = gpu[b]
            n = min(was.numel(), now.numel())
            edges = [0] + [int(v) for v in wr.get(b, np.zeros((0, 2), dtype=np.int64)).reshape(-1)] + [n]
            for lo, hi in zip(edges[0::2], edges[1::2]):
                lo, hi = min(lo, n), min(hi, n)
                if hi > lo and not torch.equal(now[lo:hi], was[lo:hi]):
                    at = lo + int(torch.nonzero(now[lo:hi] != was[lo:hi])[0])
                    rep.fails.append(f"records {begin}..{end}: byte {at} of {D.BASES[b]} changed outside every written range")
                    break
    return rep


def compare_grads(plan, rep: StageReport, gpu: dict, emu32: dict, emu64: dict | None, exact_zero=()) -> dict:
    """GRADS parameter by parameter (plan.layout.params) after compare_written() of the backward program: the error relative to
    the parameter's OWN max |ref|, below max(the bars of the records that wrote it, 8 E).  A parameter no record writes (frozen,
    absent) and those of `exact_zero` must be exactly 0.  A parameter whose float64 (else f32) reference stays below 1e-7 of the
    network's largest gradient is held to 1e-5 of that largest gradient in absolute terms (tests/test_unet_gpu.py's rule).
    Returns {name: (e32, e64, bar)}; failures go to rep.fails."""
    G = D.BASE["GRADS"]
    g = gpu[G].view(torch.float32).double()
    r32 = emu32[G].view(torch.float32).double()
    r64 = emu64[G].view(torch.float64) if emu64 is not None else None
    ref = r64 if r64 is not None else r32
    n_all = plan.layout.n_params
    scale = ref[:n_all].abs().max().item()
    out = {}
    for name, (off, shape) in plan.layout.params.items():
        n = int(np.prod(shape))
        a, b = g[off:off + n], r32[off:off + n]
        c = r64[off:off + n] if r64 is not None else None
        bars = [bar for (bb, lo, hi, bar) in rep.wlog if bb == G and lo < 4 * (off + n) and hi > 4 * off]
        if not bars or name in exact_zero:
            if a.abs().max().item() != 0 or b.abs().max().item() != 0:
                rep.fails.append(f"grad {name}: must be exactly 0, GPU max {a.abs().max().item():.3e}, emulator {b.abs().max().item():.3e}")
            out[name] = (0.0, 0.0, 0.0)
            continue
        if not bool(torch.isfinite(a).all()):
            rep.fails.append(f"grad {name}: GPU gradient not finite")
            continue
        r = c if c is not None else b
        if r.abs().max().item() < 1e-7 * scale:
            if a.abs().max().item() >= 1e-5 * scale:
                rep.fails.append(f"grad {name}: reference ~0, GPU max {a.abs().max().item():.3e} (largest gradient {scale:.3e})")
            continue
        e32 = _rel(a, b)
        e64 = _rel(a, c) if c is not None else None
        bar = max(max(bars), 8 * _rel(b, c)) if c is not None else max(bars)
        out[name] = (e32, e64, bar)
        if not (e32 < bar and (e64 is None or e64 < bar)):
            rep.fails.append(f"grad {name}: rel err {e32:.3e} (f32 emulator) {e64 if e64 is None else format(e64, '.3e')} (float64), bar {bar:.1e}")
    return out


def unspecified_reads(prog, blob) -> list:
    """Records that read bytes whose content a contract leaves open (UNSPECIFIED slots, until a later record overwrites them), or
    that read a replicated statistics tensor through a slot that does not sum its replicas: must be empty."""
    bad, open_ = [], []          # open_: (base, lo, hi)
    for i, (kind, f) in enumerate(prog.ops):
        for slot in D.OPS[kind][0]:
            t = f.get(slot)
            if not isinstance(t, _SO.TRef) or (kind, slot) in UNSPECIFIED:
                continue
            if slot not in D.WRITES[kind] or slot in _SO.ACCUM.get(kind, ()):
                if any(b == t.base and lo < t.off + t.nbytes and t.off < hi for b, lo, hi in open_):
                    bad.append((i, kind, slot, "reads split-K scratch"))
        for slot, t, iv in slot_writes(kind, f, blob):
            lo, hi = int(iv[0, 0]), int(iv[-1, 1])
            if (kind, slot) in UNSPECIFIED:
                open_.append((t.base, lo, hi))
            else:
                open_ = [(b, l, h) for b, l, h in open_ if not (b == t.base and lo <= l and h <= hi)]
    rep_ranges = [(f[s].base, f[s].off, f[s].off + f[s].nbytes) for k, f in prog.ops for s in REPLICATED
                  if s in D.WRITES.get(k, ()) and isinstance(f.get(s), _SO.TRef)]
    for i, (kind, f) in enumerate(prog.ops):
        for slot in D.OPS[kind][0]:
            t = f.get(slot)
            if isinstance(t, _SO.TRef) and slot not in REPLICA_READERS and any(b == t.base and lo < t.off + t.nbytes and t.off < hi for b, lo, hi in rep_ranges):
                if kind != "MEMSET":
                    bad.append((i, kind, slot, "reads replicated statistics"))
    return bad


def predicted_family(kind: str, f: dict):
    """the kernel family the restated launchers (tests/conv_dispatch.py, wgrad_dispatch.py, vit_dispatch.py) predict for a CONV,
    WGRAD, CHAN_LN_FWD or MAE_LOSS_* record, with its instantiation where the restatement has one: (family, inst or None); None for
    every other kind.  A FLAG_SPLIT record must run the f32-split kernels (family 5)."""
    from tests import conv_dispatch as CD
    from tests import vit_dispatch as VD
    from tests import wgrad_dispatch as WD

    has = lambda k: f.get(k) is not None     # noqa: E731
    flags = int(f.get("_flags", 0))
    al = lambda *ks: all(f[k].off % 16 == 0 for k in ks if has(k))       # noqa: E731
    if kind in ("CONV", "WGRAD") and flags & D.FLAG_SPLIT:
        return 5, None
    if kind == "CONV":
        cv = CD.dispatch(B=f["B"], C1=f["C1"], C2=f["C2"], H=f["H"], W=f["W"], M=f["M"], KH=f["KH"], KW=f["KW"], STRIDE=f["STRIDE"],
                         PAD_T=f["PAD_T"], PAD_L=f["PAD_L"], HO=f["HO"], WO=f["WO"], PRO1=f["PRO1"], PRO2=f["PRO2"], MODE=f["MODE"],
                         GATE=has("GATE1"), BIAS=has("BIAS"), RES=has("RES"), STATS=has("STATS"), SCRATCH=has("SCRATCH"), BETA=f["BETA"],
                         YC=f["YC"], NREP=f.get("NREP", 1), W_ST=f["W_ST"], X1_BF16=f.get("X1_BF16", 0), flags=flags)
        return cv.family, cv.inst
    if kind == "WGRAD":
        v = WD.dispatch(B=f["B"], M=f["M"], C=f["C"], CTOT=f["CTOT"], H=f["H"], W=f["W"], KH=f["KH"], KW=f["KW"], STRIDE=f["STRIDE"],
                        PAD_T=f["PAD_T"], PAD_L=f["PAD_L"], HO=f["HO"], WO=f["WO"], PROP=f["PROP"], PROQ=f["PROQ"], MODE=f["MODE"],
                        GATEP=has("GATEP"), GATEQ=has("GATEQ"), P_ALIGNED16=al("P"), Q_ALIGNED16=al("Q"), P_BF16=f.get("P_BF16", 0), flags=flags)
        return v.family, v.inst
    if kind == "CHAN_LN_FWD":
        return VD.ln_family(f["B"], f["C"], f["HW"], al("X", "Y", "MR")), None
    if kind in ("MAE_LOSS_FWD", "MAE_LOSS_BWD"):
        return VD.mae_family(f["P"], f["W"], al("IMGS")), None
    return None


def launch_set(plan) -> set:
    """{(kind, family, instantiation or None)} over the CONV / WGRAD / CHAN_LN_FWD / MAE_LOSS_* records of a plan's two programs"""
    out = set()
    for prog in (plan.fwd, plan.bwd):
        for kind, f in (prog.ops if prog is not None else ()):
            p = predicted_family(kind, f)
            if p is not None:
                out.add((kind,) + p)
    return out


# ---- the cases of tests/test_vit_stages_gpu.py (tests/test_vit_stage_cover_cpu.py proves what they cover) ---------------------------
FULL_MAE = dict(img_size=224, patch_size=16, num_frames=1, tubelet_size=1, in_chans=6, embed_dim=768, depth=1, num_heads=12,
                decoder_embed_dim=512, decoder_depth=1, decoder_num_heads=16)       # Prithvi-100M's widths, one block each
# name: what, fixture tag or None, options.  MAE: (B, ratio, seed) of the full-width plan; seg: (B, classes, fcn_out, seed)
STAGE_CASES = {
    "mae_small_bs2": dict(net="mae", tag="small_bs2"),
    "mae_small_bs2_norm_pix": dict(net="mae", tag="small_bs2", norm_pix=True),
    "mae_small_t3_bs2": dict(net="mae", tag="small_t3_bs2"),
    "mae_small_r0_bs2": dict(net="mae", tag="small_r0_bs2", bwd=False),
    "mae_small_bs2_dx": dict(net="mae", tag="small_bs2", want_dx=True),
    "seg_small_eval": dict(net="seg", tag="small_eval", bwd=False),
    "seg_small_train_frozen": dict(net="seg", tag="small_train_frozen"),
    "seg_small_train_unfrozen": dict(net="seg", tag="small_train_unfrozen"),
    "seg_small_eval_bwd": dict(net="seg", tag="small_train_unfrozen", train=False),
    "mae_full_b8": dict(net="mae", full=(8, 0.75, 41)),
    "seg_full_b1": dict(net="seg", full=(1, 4, 256, 43)),
    "mae_full_b8_split": dict(net="mae", full=(8, 0.75, 41), precision="f32-split"),
    "seg_full_b1_split": dict(net="seg", full=(1, 4, 256, 43), precision="f32-split"),
}


class StageCase:
    """One whole-network case: the module on the CPU with its seeded state, the inputs, and how its plan is made."""


def stage_case(name: str) -> StageCase:
    from oracle import detgen
    from oracle import prithvi_ref as P
    from s2lc_amd.modules.prithvi import MaskedAutoencoderViT
    from s2lc_amd.modules.prithvi_segmentation import PrithviSegmentationNet, PrithviSegmentationNetConfig
    from tests.helpers import MAE_CASES, SEG_CASES, mae_inputs, seg_inputs

    o = STAGE_CASES[name]
    c = StageCase()
    c.name, c.net, c.want_dx, c.precision = name, o["net"], o.get("want_dx", False), o.get("precision", "f32")
    c.y = c.drop_u = None
    if c.net == "mae":
        if "tag" in o:
            cfg, sd, c.x, c.noise, c.ratio = mae_inputs(o["tag"])
            args = dict(MAE_CASES[o["tag"]][0])
        else:
            B, c.ratio, seed = o["full"]
            args = dict(FULL_MAE)
            cfg = P.MaeCfg(**args)
            sd = detgen.fill_state(P.mae_state_shapes(cfg), seed=seed)
            sd["pos_embed"] = P.sincos_pos_embed(cfg.embed_dim, cfg.grid)
            sd["decoder_pos_embed"] = P.sincos_pos_embed(cfg.decoder_embed_dim, cfg.grid)
            c.x = detgen.normal(f"{name}.x", (B, cfg.in_chans, cfg.num_frames, cfg.img_size, cfg.img_size), seed=seed)
            c.noise = detgen.uniform(f"{name}.noise", (B, cfg.num_patches), 0.0, 1.0, seed=seed)
        c.module = MaskedAutoencoderViT(**args, norm_pix_loss=o.get("norm_pix", False))
        c.want_bwd = o.get("bwd", True)
        c.training = c.want_bwd          # (no BatchNorm / dropout: the MAE's plan is a training plan iff it carries a backward)
    else:
        if "tag" in o:
            cfg, sd, c.x, c.y, c.noise, c.drop_u, train = seg_inputs(o["tag"])
            args = dict(SEG_CASES[o["tag"]][0])
        else:
            B, ncls, fcn, seed = o["full"]
            args, train = dict(FULL_MAE), True
            m = P.MaeCfg(**args)
            cfg = P.SegCfg(mae=m, num_classes=ncls, fcn_out_channels=fcn, fcn_num_convs=1, fcn_dropout=0.1, frozen_backbone=False)
            sd = detgen.fill_state(P.seg_state_shapes(cfg), seed=seed)
            sd["backbone.pos_embed"] = P.sincos_pos_embed(m.embed_dim, m.grid)
            sd["backbone.decoder_pos_embed"] = P.sincos_pos_embed(m.decoder_embed_dim, m.grid)
            c.x = detgen.normal(f"{name}.x", (B, m.in_chans, m.num_frames, m.img_size, m.img_size), seed=seed)
            c.y = detgen.labels(f"{name}.y", (B, m.img_size, m.img_size), ncls, seed=seed)
            c.noise = detgen.uniform(f"{name}.noise", (B, m.num_patches), 0.0, 1.0, seed=seed)
            c.drop_u = detgen.uniform(f"{name}.drop", (B, fcn), 0.0, 1.0, seed=seed)
        c.ratio = 0.0
        c.training = o.get("train", train)
        c.want_bwd = o.get("bwd", True)
        g = cfg.mae.img_size // cfg.mae.patch_size
        bb = MaskedAutoencoderViT(**args, _decoder=False, _flat=False)
        c.module = PrithviSegmentationNet(PrithviSegmentationNetConfig(cfg.mae.num_frames, cfg.num_classes, cfg.fcn_out_channels, cfg.fcn_num_convs,
                                                                        cfg.fcn_dropout, cfg.frozen_backbone, embed_dim=cfg.mae.embed_dim,
                                                                        patch_height=g, patch_width=g), backbone=bb)
    c.module.load_state_dict(sd)
    c.module.train(c.training)
    c.module.precision = c.precision
    c.B = c.x.shape[0]
    return c


def stage_plan(c: StageCase):
    return c.module._make_plan(c.B, c.training, c.ratio, c.want_bwd, c.want_dx)


def stage_dout(c: StageCase, plan, emu32: dict) -> torch.Tensor:
    """the upstream gradient of a case as flat f32.  MAE: d loss = 1 and no gradient on pred (the packed DOUT buffer).  Segmentation:
    d cross_entropy / d logits (oracle/losses_ref.py, ignore_index 0) of the logits the image `emu32` holds."""
    from oracle import losses_ref

    if c.net == "mae":
        g = torch.zeros(plan.dout_bytes // 4)
        g[0] = 1.0
        return g
    lg = out_view(emu32, plan.outputs["logits"]).double().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(losses_ref.cross_entropy(lg, c.y, ignore_index=0), lg)
    return g.float().reshape(-1)


def poison_accumulators(bases: dict, wide: bool = False) -> None:
    """NaN over AUX and WGS of an emulator's bases, as the workspace: an engine reuses both from step to step without clearing them,
    so a program must MEMSET what it accumulates into (the stage test poisons the GPU's the same way)"""
    for name in ("AUX", "WGS"):
        fview(bases, name, wide).fill_(float("nan"))


def cpu_half(c: StageCase, plan, plan_run=None):
    """The stage test without a GPU: the f32 emulation of `plan_run` (default: of `plan` itself) stands where the GPU's run stands in
    tests/test_vit_stages_gpu.py, and is compared with the f32 and float64 emulations of `plan` - forward from the poisoned
    workspace, backward from the forward state of the run under test.  -> (forward report, backward report or None, gradient table);
    a plan against itself must come out with no failure and every error 0, a plan_run that differs in a record must not."""
    plan_run = plan_run or plan
    fp, fb = c.module._flat_params.detach().cpu().clone(), c.module._flat_bufs.detach().cpu().clone()
    nz = stage_noise(c, plan)
    e32, e64 = make_bases_vit(plan, fp, fb, c.x, nz, False), make_bases_vit(plan, fp, fb, c.x, nz, True)
    run = make_bases_vit(plan_run, fp, fb, c.x, nz, False)
    for bases, wide in ((run, False), (e32, False), (e64, True)):
        poison_accumulators(bases, wide)
    mutable = [D.BASE[n] for n in MUTABLE]
    refs, blob = typed_refs(plan), plan.const_table
    before = {b: run[b].clone() for b in mutable}
    emulate(plan_run.fwd.pack(), run)
    emulate(plan.fwd.pack(), e32)
    emulate(plan.fwd.pack(), e64, True)
    rf = compare_written(plan.fwd, blob, run, e32, e64, before=before, pack_copies=False)
    if plan.bwd is None:
        return rf, None, {}
    g = stage_dout(c, plan, e32)
    for bases, wide in ((run, False), (e32, False), (e64, True)):
        fview(bases, "DOUT", wide)[: g.numel()].copy_(g)
    before = {b: run[b].clone() for b in mutable}
    wide_state = widen(before, refs)
    for b in mutable:
        n, n2 = min(e32[b].numel(), before[b].numel()), min(e64[b].numel(), wide_state[b].numel())
        e32[b][:n].copy_(before[b][:n])
        e64[b][:n2].copy_(wide_state[b][:n2])
    emulate(plan_run.bwd.pack(), run)
    emulate(plan.bwd.pack(), e32)
    emulate(plan.bwd.pack(), e64, True)
    rb = compare_written(plan.bwd, blob, run, e32, e64, before=before, pack_copies=False)
    return rf, rb, compare_grads(plan, rb, run, e32, e64, exact_zero=("head.net.0.bias",) if c.training else ())


def stage_noise(c: StageCase, plan) -> torch.Tensor:
    """the NOISE base of a case as a flat f32 CPU tensor (engine.fill_noise's layout)"""
    nz = torch.zeros(max(plan.noise_bytes // 4, 1))
    for name, src in (("noise", c.noise), ("drop_u", c.drop_u)):
        if name in plan.noise and src is not None:
            off = plan.noise[name].off // 4
            nz[off:off + src.numel()] = src.reshape(-1)
    return nz
