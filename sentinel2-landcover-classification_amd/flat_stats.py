"""Per-tensor gradient / parameter statistics and global gradient-norm clipping on the flat buffers.

The reference's training scripts call `logger.watch(model, log="all", log_freq=30)` (src/train_segmentation.py:271-272,
train_mae_prithvi.py): at a logging step wandb walks every parameter and every gradient - 556 gradient tensors for U-Net b5, 252 for
Prithvi-100M - and takes min, max and a 64-bin `histc` of each, with a host copy after each.  `gradient_clip_val`, one Trainer argument
there, is `torch.nn.utils.clip_grad_norm_` over the same `.grad` views.  Here every parameter and every gradient is a slice of one
contiguous f32 buffer (flat.py), so the same numbers for all tensors are two streaming reads of that buffer (stages SEG_STATS, SEG_HIST)
and clipping is one more in-place pass (GRAD_CLIP) - no host round trip anywhere; csrc/flat_stats.hip, plan/opdefs.py.

    stats = FlatStats(model, bins=64)
    loss.backward()
    total = clip_grad_norm_(model, max_norm=1.0)      # 0-dim f32 device tensor: the norm BEFORE clipping; no sync
    if step % 30 == 0:
        g = stats.gradients()                         # device tensors, no sync
        log(g.cpu())                                  # the one sync, at logging time
    optimizer.step()

`gradients()`, `clip_grad_norm_` and `grad_norm` cover exactly the parameters `FlatAdam` would step: not in `module._no_grad_params`,
`requires_grad`, `p.grad is not None`.  Like everywhere else there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from .plan import opdefs as D
from .stage_call import StageCall

CHUNK = D.SEG_CHUNK          # floats per workgroup of the three stages
MAX_BINS = 256


# ---- segment and chunk tables ---------------------------------------------------------------------------------------------------
def build_tables(segments) -> tuple[np.ndarray, np.ndarray]:
    """segments: [(first float, number of floats)] -> (SEGS int32 [P, 2], CHUNKS int32 [NC, 2] = {segment, chunk index within it}):
    segment p becomes ceil(n / CHUNK) chunks of CHUNK floats (the last one shorter), rows ascending by (segment, index)."""
    segs = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
    nch = (segs[:, 1] + CHUNK - 1) // CHUNK
    seg_of = np.repeat(np.arange(len(segs), dtype=np.int64), nch)
    first = np.cumsum(nch) - nch
    k = np.arange(int(nch.sum()), dtype=np.int64) - np.repeat(first, nch)
    return segs.astype(np.int32), np.stack([seg_of, k], axis=1).astype(np.int32)


def check_tables(segs: np.ndarray, chunks: np.ndarray, total: int) -> None:
    """What the stages assume of SEGS / CHUNKS and do not check on the device: every segment holds at least one float and lies inside
    the buffer of `total` floats, segments do not overlap, and the chunks tile every segment exactly once in ascending order."""
    segs, chunks = np.asarray(segs, dtype=np.int64), np.asarray(chunks, dtype=np.int64)
    if segs.ndim != 2 or segs.shape[1] != 2 or len(segs) < 1 or chunks.ndim != 2 or chunks.shape[1] != 2:
        raise ValueError("SEGS must be [P, 2] with P >= 1 and CHUNKS [NC, 2]")
    if int(total) >= 1 << 31:
        raise ValueError("the flat buffer must hold fewer than 2^31 floats")
    first, n = segs[:, 0], segs[:, 1]
    if (n < 1).any() or (first < 0).any() or (first + n > int(total)).any():
        raise ValueError("every segment must hold at least one float and lie inside the buffer")
    order = np.argsort(first, kind="stable")
    if (first[order][1:] < (first + n)[order][:-1]).any():
        raise ValueError("segments overlap")
    nch = (n + CHUNK - 1) // CHUNK
    want_seg = np.repeat(np.arange(len(segs), dtype=np.int64), nch)
    want_k = np.arange(int(nch.sum()), dtype=np.int64) - np.repeat(np.cumsum(nch) - nch, nch)
    if len(chunks) != len(want_seg) or not np.array_equal(chunks[:, 0], want_seg) or not np.array_equal(chunks[:, 1], want_k):
        raise ValueError("the chunks must tile every segment exactly once in ascending order")


def param_list(module):
    """[(name, parameter, first float, numel)] in named_parameters() order.  `named_parameters()` walks the module tree (~0.5 ms for
    U-Net b5), so `FlatStats` takes this list once: like `FlatAdam._plist` it assumes that the module keeps its Parameter objects
    (`_flatten()` rebinds their `.data` on a move and keeps the objects)."""
    named = dict(module.named_parameters())
    return [(name, named[name], int(off), int(named[name].numel())) for name, (off, _shape) in module._layout.params.items()]


def select(module, gradients: bool, plist=None):
    """([name], [(first float, numel)]) in named_parameters() order: every parameter (gradients=False) or the ones `FlatAdam._ranges`
    would step (not in module._no_grad_params - read at every call -, requires_grad, p.grad is not None).  Segments carry the true
    numel, not the padded one.  `plist`: a cached `param_list(module)`.  The one selection rule of this module: `FlatStats` calls it."""
    rows = param_list(module) if plist is None else plist
    if gradients:
        skip = module._no_grad_params
        rows = [r for r in rows if r[0] not in skip and r[1].requires_grad and r[1].grad is not None]
    return [r[0] for r in rows], [(r[2], r[3]) for r in rows]


class _Tables:
    """the device side of one selection: SEGS and CHUNKS in one upload, SEG_STATS's scratch, the packed calls"""

    def __init__(self, names, segments, total: int, device):
        self.names, self.numel = list(names), [n for _, n in segments]
        segs, chunks = build_tables(segments)
        check_tables(segs, chunks, total)
        self.segs, self.chunks = segs, chunks
        self.P, self.NC = len(segs), len(chunks)
        tab = StageCall()           # only its byte image is used: uploaded here, once, and bound as raw bytes by every call
        self.segs_off, self.chunks_off = tab.const(segs, "i32").off, tab.const(chunks, "i32").off
        self.aux = tab.image().to(device)
        self.part = torch.empty(self.NC, 6, dtype=torch.float64, device=device)
        self.calls = {}             # the packed calls over these tables (FlatStats._call)


class SegmentStats:
    """Result of `FlatStats.gradients()` / `.parameters()`: `names`, `numel` (host lists, named_parameters() order) and the device
    tensors `stats` f64 [P, 4] = {sum, sumsq, min, max}, `counts` i64 [P, 2] = {NaN, +-Inf}, `hist` i64 [P, bins] or None."""

    def __init__(self, names, numel, stats, counts, hist):
        self.names, self.numel, self.stats, self.counts, self.hist = names, numel, stats, counts, hist

    def cpu(self) -> dict:
        """{name: {"norm", "mean", "min", "max", "nan", "inf", "hist", "edges"}} on the host - the one synchronisation.  norm =
        sqrt(sumsq) over all elements (NaN / Inf propagate); mean, min, max over the finite elements (none: NaN, +inf, -inf); hist /
        edges (numpy int64 [bins] / float64 [bins + 1], torch.histc's range rule) are None without histograms."""
        st, ct = self.stats.cpu().numpy(), self.counts.cpu().numpy()
        hs = None if self.hist is None else self.hist.cpu().numpy()
        out = {}
        for i, (name, n) in enumerate(zip(self.names, self.numel)):
            s, q, lo, hi = (float(v) for v in st[i])
            finite = n - int(ct[i, 0]) - int(ct[i, 1])
            edges = None
            if hs is not None:
                a, b = (lo - 1.0, hi + 1.0) if lo == hi else (lo, hi)
                edges = np.linspace(a, b, hs.shape[1] + 1) if finite else np.full(hs.shape[1] + 1, np.nan)
            out[name] = {"norm": float(np.sqrt(q)), "mean": s / finite if finite else float("nan"), "min": lo, "max": hi,
                         "nan": int(ct[i, 0]), "inf": int(ct[i, 1]), "hist": None if hs is None else hs[i].copy(), "edges": edges}
        return out


def _check_module(module, reducer=None) -> None:
    if not hasattr(module, "_flat_params") or not hasattr(module, "_layout"):
        raise TypeError("flat statistics need a module that keeps its parameters in one flat buffer (flat.FlatParamsMixin)")
    if reducer is not None:
        if reducer.module is not module:
            raise ValueError("the reducer belongs to another module")
        if reducer.mode == "sharded":
            raise NotImplementedError("with a sharded FlatGradReducer a rank holds reduced gradients only for its own slices: a global "
                                      "gradient norm needs a collective, which is not implemented (use the all-reduce mode)")


def _refuse_cpu(buf: torch.Tensor) -> None:
    if not buf.is_cuda:
        raise RuntimeError("flat statistics and gradient clipping run on the GPU (there is no CPU fallback)")


class FlatStats:
    """Statistics of every tensor of a `FlatParamsMixin` module (EfficientnetUnet, MaskedAutoencoderViT, PrithviSegmentationNet) in
    one launch sequence per call; `bins` (1..256) is the histogram resolution.  The segment / chunk tables of a selection are built
    once and cached on the device; they are rebuilt only when the selection changes (freeze / unfreeze, a moved module)."""

    def __init__(self, module, bins: int = 64, reducer=None):
        bins = int(bins)
        if not 1 <= bins <= MAX_BINS:
            raise ValueError(f"bins must be in 1..{MAX_BINS}")
        _check_module(module, reducer)
        self.module, self.bins = module, bins
        self._tables = {}
        self._plist = None

    def gradients(self, hist: bool = True) -> SegmentStats:
        """SEG_STATS (+ SEG_HIST) over the gradient buffer, for the parameters `FlatAdam` would step; device tensors, no sync."""
        return self._run(True, hist)

    def parameters(self, hist: bool = True) -> SegmentStats:
        """SEG_STATS (+ SEG_HIST) over the parameter buffer, for every parameter; device tensors, no sync."""
        return self._run(False, hist)

    # ---- implementation ----------------------------------------------------------------------------------------------------------
    def _selection(self, gradients: bool):
        """`select()` over the cached parameter list: the current ([name], [(first float, numel)]); needs no GPU"""
        if self._plist is None:
            self._plist = param_list(self.module)
        return select(self.module, gradients, self._plist)

    def _select(self, gradients: bool):
        """(buffer, tables) of the current selection.  Per call this costs one pass over the parameter objects, as `FlatAdam._ranges`
        does per step."""
        mod = self.module
        _refuse_cpu(mod._flat_params)
        buf = mod._grad_buffer() if gradients else mod._flat_params
        names, segments = self._selection(gradients)
        if not names:
            raise RuntimeError("no parameter holds a gradient: call backward() first")
        key = (buf.device, buf.numel(), tuple(first for first, _ in segments))
        hit = self._tables.get(gradients)
        if hit is None or hit[0] != key:
            hit = (key, _Tables(names, segments, buf.numel(), buf.device))
            self._tables[gradients] = hit
        return buf, hit[1]

    def _call(self, t: _Tables, hist: bool, clip: str | None, buf, stats, counts, last) -> StageCall:
        """SEG_STATS, then SEG_HIST (hist; last = HIST) or GRAD_CLIP (clip = "norm": the norm only, "apply": MAX_NORM is written into
        the record per call; last = NORM).  The tables fix every shape, so the call is packed once per kind and kept with them; a
        later use only puts its own tensors behind the slots."""
        hit = t.calls.get((hist, clip))
        if hit is not None:
            for ref, tensor in zip(hit[1], (buf, stats, counts, last)):
                if ref is not None:
                    hit[0].rebind(ref, tensor)
            return hit[0]
        call = StageCall()
        x, st, cn, ls = call.t(buf), call.t(stats), call.t(counts), call.t(last)
        refs = dict(SEGS=call.t(t.aux, (t.P, 2), "i32", t.segs_off), CHUNKS=call.t(t.aux, (t.NC, 2), "i32", t.chunks_off), STATS=st,
                    P=t.P, NC=t.NC)
        call.add("SEG_STATS", X=x, PART=call.t(t.part), COUNTS=cn, **refs)
        if hist:
            call.add("SEG_HIST", X=x, HIST=ls, NB=self.bins, **refs)
        if clip == "norm":
            call.add("GRAD_CLIP", STATS=st, NORM=ls, P=t.P, NC=t.NC, APPLY=0)
        elif clip == "apply":
            call.add("GRAD_CLIP", X=x, NORM=ls, APPLY=1, MAX_NORM=1.0, **refs)
        call.pack()
        t.calls[(hist, clip)] = call, (x, st, cn, ls)
        return call

    def _run(self, gradients: bool, hist: bool) -> SegmentStats:
        buf, t = self._select(gradients)
        dev = buf.device
        stats = torch.empty(t.P, 4, dtype=torch.float64, device=dev)
        counts = torch.empty(t.P, 2, dtype=torch.int64, device=dev)
        hst = torch.zeros(t.P, self.bins, dtype=torch.int64, device=dev) if hist else None
        self._call(t, hist, None, buf, stats, counts, hst).run()
        return SegmentStats(t.names, t.numel, stats, counts, hst)

    def _norm(self, max_norm: float | None) -> torch.Tensor:
        """SEG_STATS + GRAD_CLIP over the gradient buffer (max_norm None: the norm only); returns NORM as a 0-dim f32 device tensor"""
        buf, t = self._select(True)
        dev = buf.device
        stats = torch.empty(t.P, 4, dtype=torch.float64, device=dev)
        counts = torch.empty(t.P, 2, dtype=torch.int64, device=dev)
        norm = torch.empty(1, dtype=torch.float32, device=dev)
        call = self._call(t, False, "norm" if max_norm is None else "apply", buf, stats, counts, norm)
        if max_norm is not None:
            call.packed[1]["f"][D.slot("GRAD_CLIP", "MAX_NORM")[1]] = max_norm
        call.run()
        return norm.view(())


def _helper(module, reducer) -> FlatStats:
    """the FlatStats behind clip_grad_norm_ / grad_norm: kept on the module itself (a private attribute, like `_engines`), so it and
    its device tables live exactly as long as the module does"""
    _check_module(module, reducer)
    h = module.__dict__.get("_flat_stats_helper")
    if h is None:
        h = module.__dict__["_flat_stats_helper"] = FlatStats(module, bins=1)
    return h


def grad_norm(module, reducer=None) -> torch.Tensor:
    """The global 2-norm of the gradients `FlatAdam` would step, as a 0-dim f32 device tensor; the gradients are not touched, nothing
    synchronises."""
    return _helper(module, reducer)._norm(None)


def clip_grad_norm_(module, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False, reducer=None) -> torch.Tensor:
    """`torch.nn.utils.clip_grad_norm_(module.parameters(), max_norm)` in place on the flat gradient buffer, before `optimizer.step()`:
    gradients are scaled by max_norm / (norm + 1e-6) where that is below 1 (otherwise the buffer is not written at all).  Returns the
    norm BEFORE clipping as a 0-dim f32 device tensor, without synchronising.  Only norm_type 2.  error_if_nonfinite=True is the one
    variant that synchronises: it reads the norm back first and raises RuntimeError, leaving the gradients alone, if it is NaN / Inf.
    `reducer`: as for `FlatAdam`; the all-reduce mode needs nothing special, the sharded mode raises NotImplementedError."""
    if float(norm_type) != 2.0:
        raise ValueError("clip_grad_norm_ on the flat buffers implements norm_type = 2 only")
    max_norm = float(max_norm)
    if not max_norm > 0.0 or not np.isfinite(np.float32(max_norm)):
        raise ValueError("max_norm must be positive and finite")
    h = _helper(module, reducer)
    if error_if_nonfinite:
        total = h._norm(None)
        if not bool(torch.isfinite(total)):
            raise RuntimeError("the total norm of the gradients is non-finite, so it cannot be clipped")
    return h._norm(max_norm)
