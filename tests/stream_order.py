"""TEST INFRASTRUCTURE ONLY - the order in which `s2k_program_run` (csrc/s2k_api.hip) leaves the records of a program, and the bytes
every record reads and writes, stated once more without a GPU.

The executor model (`execute_order`, `unordered_pairs`) is a restatement of the loop of s2k_program_run from its text:

  * a record flagged FLAG_SIDE is issued to the leased side stream.  In front of it the fork event is recorded on the caller's
    stream and waited for by the side stream - but only when main-stream work was issued since the last fork (the "dirty" bit,
    true at the start of a call).  The side stream is serial.  So a side record is ordered after EVERY earlier record;
  * every other record is issued to the caller's stream.  Nothing orders it after the side records that are pending (issued and
    not yet joined) unless it carries FLAG_JOIN: then the side stream's join event is recorded and waited for in front of it;
  * a FLAG_CHAIN head with three more records inside the call: a join asked for by ANY of the four records is honoured in front of
    the head.  Then either the four records run as one launch on the caller's stream (accepted: the DWCONV_WGRAD's FLAG_SIDE is
    ignored) or the flag has no further effect and the records are issued one by one (declined).  Both outcomes are modelled;
  * the end of a call is a join.

Two records are UNORDERED when one is a pending side record and the other a later main-stream record.  They CONFLICT when a byte
one of them writes is read or written by the other.

The footprints (`footprint`) are per base and byte exact where a declared tensor range would not do: WEIGHT_PACK and
WGRAD_FINALIZE are expanded through their CONST tables with the layout functions of tests/pack_ref.py, MEMSET takes its BYTES, a
WGRAD with CTOT > C and a CONV with YC > M take the rows they own, a CONV's WTB takes the size of the copy its flag names.  Every
other tensor slot takes the range the planner declared for it (TRef.nbytes).  Whatever a stage accumulates into is read AND written.
tests/test_stream_order_cpu.py holds all of it against the emulator (oracle/ops_ref.py), record signature by record signature."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan.program import TRef
from tests import pack_ref as PR

SIDE, JOIN, CHAIN = D.FLAG_SIDE, D.FLAG_JOIN, D.FLAG_CHAIN
CHAIN_KINDS = ("BN_BWD_APPLY", "DWCONV_WGRAD", "DWCONV_DGRAD", "BN_BWD_APPLY")


# ---- the executor's ordering ---------------------------------------------------------------------------------------------------------
def kinds_flags(prog) -> list[tuple[str, int]]:
    """(kind, flags) per record of a Program, a list of (kind, fields) or a packed S2kOp array"""
    if isinstance(prog, np.ndarray):
        return [(D.NAME_OF[int(r["kind"])], int(r["flags"])) for r in prog]
    return [(k, int(f.get("_flags", 0))) for k, f in getattr(prog, "ops", prog)]


@dataclass
class Order:
    begin: int
    end: int
    stream: list                 # per record: "S" (side stream), "M" (caller's stream), None outside [begin, end)
    join_before: list            # per record: the main stream waits for the side stream in front of it
    forks: list = field(default_factory=list)     # side records in front of which the fork event is re-armed
    chains: list = field(default_factory=list)    # heads of the chains that ran as one launch
    end_join: bool = False       # side work was still pending when the call ended (the final join did something)


def execute_order(prog, accept_chains: bool, begin: int = 0, end: int | None = None) -> Order:
    """One call s2k_program_run(ops, begin, end).  accept_chains: every FLAG_CHAIN head whose four kinds and flags allow it is taken
    as one launch; False: every chain is declined (the shape and tensor checks of try_dw_chain can only decline)."""
    recs = kinds_flags(prog)
    end = len(recs) if end is None else end
    o = Order(begin, end, [None] * len(recs), [False] * len(recs))
    side_busy, main_dirty = False, True
    i = begin
    while i < end:
        kind, fl = recs[i]
        if fl & CHAIN and i + 3 < end:
            four = recs[i:i + 4]
            if any(f & JOIN for _, f in four) and side_busy:
                o.join_before[i], side_busy = True, False
            if (accept_chains and tuple(k for k, _ in four) == CHAIN_KINDS
                    and not any(f & (D.FLAG_BF16 | D.FLAG_SPLIT) for _, f in four)):
                for k in range(4):
                    o.stream[i + k] = "M"
                o.chains.append(i)
                main_dirty = True
                i += 4
                continue
        if fl & SIDE:
            if main_dirty:
                o.forks.append(i)
                main_dirty = False
            o.stream[i] = "S"
            side_busy = True
        else:
            if fl & JOIN and side_busy:
                o.join_before[i], side_busy = True, False
            o.stream[i] = "M"
            main_dirty = True
        i += 1
    o.end_join = side_busy
    return o


def windows(o: Order) -> list[tuple[int, int]]:
    """(s, e) per side record s: the main-stream records in (s, e) are unordered with it"""
    out, pending = [], []
    for j in range(o.begin, o.end):
        if o.join_before[j]:
            out += [(s, j) for s in pending]
            pending = []
        if o.stream[j] == "S":
            pending.append(j)
    return sorted(out + [(s, o.end) for s in pending])


def unordered_pairs(prog, accept_chains: bool, begin: int = 0, end: int | None = None) -> set:
    """{(i, j), i < j}: the record pairs one call leaves unordered"""
    o = execute_order(prog, accept_chains, begin, end)
    return {(s, j) for s, e in windows(o) for j in range(s + 1, e) if o.stream[j] == "M"}


# ---- footprints ----------------------------------------------------------------------------------------------------------------------
# tensor slots a stage both reads and writes (accumulators and in-place updates); slots of opdefs.WRITES not listed here are only
# written, every other slot is only read.  Conditional ones (BETA, ACCUM, folded BatchNorm) are handled in footprint().
ACCUM = {
    "AXPY": ("Y",), "CONV": ("STATS", "SCRATCH"), "WGRAD": ("WGS",), "WGRAD_FINALIZE": ("GRADS",), "DWCONV_FWD": ("STATS", "FRM", "FRV"),
    "DWCONV_DGRAD": ("STATS2",), "DWCONV_WGRAD": ("DW",), "BN_FINALIZE": ("RM", "RV"), "SE_POOL": ("FRM", "FRV"),
    "SE_FC_BWD": ("DGATE", "HPRE", "DW1", "DB1", "DW2", "DB2"), "BN_BWD_REDUCE": ("STATS2",), "BN_BWD_FINALIZE": ("DGAMMA", "DBETA"),
    "BN_BWD_APPLY": ("DGAMMA", "DBETA"), "BN_RESIDUAL": ("FRM", "FRV"), "CHANNEL_SUM": ("OUT",), "CHAN_LN_BWD": ("DGAMMA", "DBETA", "DSUM"),
    "ACT_BWD": ("G",), "TOKEN_SCATTER": ("DFILL",), "MAE_LOSS_FWD": ("ACC",), "SE_FC_WGRAD": ("DW1", "DB1", "DW2", "DB2"),
    "CONFUSION": ("HIST",), "LOSS_FWD": ("ACC",),
}


def strided(off: int, dims, itemsize: int = 4):
    """byte intervals (lo[], hi[]) of the elements off + sum_i k_i * stride_i, k_i < n_i, dims = [(n, stride), ...] in elements:
    dimensions that continue a contiguous run are merged into it, the others become one interval per index"""
    dims = sorted(((int(n), int(s)) for n, s in dims if n > 1), key=lambda d: d[1])
    run = 1
    while dims and dims[0][1] == run:
        run *= dims[0][0]
        dims.pop(0)
    starts = np.zeros(1, dtype=np.int64)
    for n, s in dims:
        assert s >= run, "overlapping strides"
        starts = (starts[:, None] + np.arange(n, dtype=np.int64)[None, :] * s).reshape(-1)
    lo = off + starts * itemsize
    return lo, lo + run * itemsize


def _merge(pieces):
    """[(lo[], hi[])] -> one sorted (n, 2) array of disjoint intervals"""
    if not pieces:
        return np.zeros((0, 2), dtype=np.int64)
    lo = np.concatenate([np.atleast_1d(np.asarray(p[0], dtype=np.int64)) for p in pieces])
    hi = np.concatenate([np.atleast_1d(np.asarray(p[1], dtype=np.int64)) for p in pieces])
    keep = hi > lo
    lo, hi = lo[keep], hi[keep]
    if lo.size < 2:
        return np.stack([lo, hi], 1)
    order = np.argsort(lo, kind="stable")
    lo, hi = lo[order], hi[order]
    top = np.maximum.accumulate(hi)
    first = np.concatenate([[True], lo[1:] > top[:-1]])
    idx = np.nonzero(first)[0]
    return np.stack([lo[idx], np.maximum.reduceat(hi, idx)], 1)


class Footprint:
    """reads / writes: base -> (n, 2) int64 array of sorted, disjoint byte intervals"""

    def __init__(self):
        self._r: dict = {}
        self._w: dict = {}
        self.reads: dict = {}
        self.writes: dict = {}

    def add(self, base: int, lo, hi, read: bool, write: bool):
        if read:
            self._r.setdefault(base, []).append((lo, hi))
        if write:
            self._w.setdefault(base, []).append((lo, hi))

    def ref(self, t: TRef, read: bool, write: bool, nbytes: int | None = None):
        self.add(t.base, t.off, t.off + (t.nbytes if nbytes is None else nbytes), read, write)

    def close(self) -> "Footprint":
        self.reads = {b: _merge(p) for b, p in self._r.items()}
        self.writes = {b: _merge(p) for b, p in self._w.items()}
        return self

    def touched(self, base: int) -> np.ndarray:
        return _merge([(a[:, 0], a[:, 1]) for a in (self.reads.get(base), self.writes.get(base)) if a is not None])


def table_rows(blob, t: TRef, n: int, width: int) -> list:
    """rows of a CONST table (the int32 words of the plan's const_table)"""
    assert t.base == D.BASE["CONST"] and t.off % 4 == 0
    w = np.asarray(blob[t.off // 4:t.off // 4 + n * width], dtype=np.int64)
    assert w.size == n * width, "the table runs past the constants"
    return w.reshape(n, width).tolist()


def footprint(kind: str, f: dict, blob) -> Footprint:
    """the bytes one record reads and writes"""
    fp = Footprint()
    names = D.OPS[kind][0]
    writes = set(D.WRITES[kind])
    both = set(ACCUM.get(kind, ()))
    exact: dict = {}            # slot -> [(lo[], hi[])] overriding the declared range
    fl = int(f.get("_flags", 0))
    if kind == "MEMSET":
        exact["DST"] = [(f["DST"].off, f["DST"].off + int(f["BYTES"]))]
    elif kind == "WEIGHT_PACK":
        rows = table_rows(blob, f["TABLE"], f["N_ENTRIES"], 12)
        src, dst = f["SRC"], f["DST"]
        exact["TABLE"] = [(f["TABLE"].off, f["TABLE"].off + 48 * len(rows))]
        exact["SRC"], exact["DST"] = [], []
        for r in rows:
            src_off, dst_off, M, K, T, s_m, s_k, s_t = r[:8]
            exact["SRC"].append(strided(src.off + 4 * src_off, [(M, s_m), (K, s_k), (T, s_t)]))
            n = PR.entry_floats(r)
            exact["DST"].append((dst.off + 4 * dst_off, dst.off + 4 * dst_off + 4 * n))
            if f.get("BF16_BASE"):
                a = dst.off + PR.bf16_addr(int(f["BF16_BASE"]), dst_off)
                exact["DST"].append((a, a + 2 * n))
            if f.get("Q4_BASE") and PR.q4_wanted(r):
                a = dst.off + PR.q4_addr(int(f["Q4_BASE"]), dst_off)
                exact["DST"].append((a, a + 4 * n))
            if f.get("SPLIT_BASE"):
                a = dst.off + PR.split_addr(int(f["SPLIT_BASE"]), dst_off, 0, n)
                assert PR.split_addr(int(f["SPLIT_BASE"]), dst_off, 2, n) - a == 4 * n
                exact["DST"].append((a, a + 6 * n))
    elif kind == "WGRAD_FINALIZE":
        rows = table_rows(blob, f["TABLE"], f["N_ENTRIES"], 5)
        exact["TABLE"] = [(f["TABLE"].off, f["TABLE"].off + 20 * len(rows))]
        exact["WGS"] = [(f["WGS"].off + 4 * off, f["WGS"].off + 4 * (off + M * C * T)) for off, M, C, T, _ in rows]
        exact["GRADS"] = [(f["GRADS"].off + 4 * off, f["GRADS"].off + 4 * (off + M * C * T)) for off, M, C, T, _ in rows]
    elif kind == "WGRAD":
        T = f["KH"] * f["KW"]
        exact["WGS"] = [strided(f["WGS"].off, [(f["C"], 1), (f["M"], f["CTOT"]), (T, f["M"] * f["CTOT"])])]
    elif kind == "CONV":
        hw = f["HO"] * f["WO"]
        rows_ = f["M"] * hw                       # MODE_CONVT_SCATTER: M / 4 channels of 4 * HO * WO pixels
        ystride = f["YC"] * hw * (4 if f["MODE"] == D.MODE_CONVT_SCATTER else 1)
        for slot in ("Y", "RES"):
            if isinstance(f.get(slot), TRef):
                exact[slot] = [strided(f[slot].off, [(rows_, 1), (f["B"], ystride)])]
        if f.get("BETA"):
            both.add("Y")
        if isinstance(f.get("WTB"), TRef):
            per = 6 if fl & D.FLAG_SPLIT else 2 if fl & D.FLAG_BF16 else 4
            exact["WTB"] = [(f["WTB"].off, f["WTB"].off + per * f["WTB"].numel)]
    elif kind == "DWCONV_DGRAD":
        if f.get("BETA"):
            both.add("G")
    elif kind == "CHAN_LN_BWD":
        if f.get("ACCUM") and f.get("DXIN") is None:
            both.add("DX")
    elif kind == "PATCHIFY":
        inv = f.get("INVERSE", 0)
        writes = {"OUT"} if inv == 0 else {"X"}
        both = {"X"} if inv == 3 else set()
    if kind in D.FOLD_KINDS and f.get("FSTATS") is None:
        writes -= {"BNV", "FRM", "FRV"}           # not folded: BNV is an input
    if kind == "BN_FINALIZE" and not f.get("TRAIN"):
        writes -= {"RM", "RV"}
    if kind == "BN_BWD_APPLY" and f.get("COEF") is not None:
        writes -= {"DGAMMA", "DBETA"}
    for slot in names:
        t = f.get(slot)
        if not isinstance(t, TRef):
            continue
        w = slot in writes
        r = (not w) or slot in both
        if slot in exact:
            for lo, hi in exact[slot]:
                fp.add(t.base, lo, hi, r, w)
        else:
            fp.ref(t, r, w)
    return fp.close()


def footprints(ops, blob) -> list:
    return [footprint(k, f, blob) for k, f in ops]


# ---- conflicts -----------------------------------------------------------------------------------------------------------------------
def _hit(a: np.ndarray, b: np.ndarray):
    """first overlap of two sorted disjoint interval arrays, or None"""
    if a is None or b is None or not len(a) or not len(b):
        return None
    if len(a) > len(b):
        a, b = b, a
    k = np.searchsorted(b[:, 1], a[:, 0], side="right")         # first interval of b that ends behind a's start
    ok = k < len(b)
    ok[ok] = b[k[ok], 0] < a[ok, 1]
    i = np.nonzero(ok)[0]
    if not i.size:
        return None
    i = int(i[0])
    return max(int(a[i, 0]), int(b[k[i], 0])), min(int(a[i, 1]), int(b[k[i], 1]))


def pair_conflict(fa: Footprint, fb: Footprint):
    """(what, base, lo, hi) of the first byte range one record writes and the other reads or writes, or None"""
    for what, x, y in (("write/write", fa.writes, fb.writes), ("write/read", fa.writes, fb.reads), ("read/write", fa.reads, fb.writes)):
        for base, iv in x.items():
            h = _hit(iv, y.get(base))
            if h is not None:
                return what, D.BASES[base], h[0], h[1]
    return None


class Hulls:
    """one bounding interval per (record, base, read or write): the candidate filter in front of the exact comparison"""

    def __init__(self, fps):
        rec, base, lo, hi, w = [], [], [], [], []
        for i, fp in enumerate(fps):
            for isw, d in ((0, fp.reads), (1, fp.writes)):
                for b, iv in d.items():
                    if len(iv):
                        rec.append(i), base.append(b), lo.append(int(iv[0, 0])), hi.append(int(iv[-1, 1])), w.append(isw)
        self.rec, self.base, self.lo, self.hi, self.w = (np.asarray(v, dtype=np.int64) for v in (rec, base, lo, hi, w))
        self.first = np.searchsorted(self.rec, np.arange(len(fps) + 1))

    def of(self, i):
        return slice(int(self.first[i]), int(self.first[i + 1]))


def find_conflicts(ops, blob, accept_chains: bool, fps=None, hulls=None, limit: int = 20):
    """-> (conflicts [(i, j, what, base, lo, hi)], Order, number of unordered pairs examined)"""
    fps = fps if fps is not None else footprints(ops, blob)
    h = hulls if hulls is not None else Hulls(fps)
    o = execute_order(ops, accept_chains)
    main = np.asarray([s == "M" for s in o.stream], dtype=bool)
    n_main_upto = np.concatenate([[0], np.cumsum(main)])
    out, pairs = [], 0
    for s, e in windows(o):
        pairs += int(n_main_upto[e] - n_main_upto[s + 1])
        if e <= s + 1:
            continue
        win = slice(int(h.first[s + 1]), int(h.first[e]))
        rec, base, lo, hi, w = h.rec[win], h.base[win], h.lo[win], h.hi[win], h.w[win]
        cand = np.zeros(rec.size, dtype=bool)
        own = h.of(s)
        for b, l, u, isw in zip(h.base[own], h.lo[own], h.hi[own], h.w[own]):
            m = (base == b) & (lo < u) & (hi > l)
            if not isw:
                m &= w == 1
            cand |= m
        cand &= main[rec]
        for j in np.unique(rec[cand]):
            c = pair_conflict(fps[s], fps[int(j)])
            if c is not None and len(out) < limit:
                out.append((s, int(j)) + c)
    return out, o, pairs


# ---- gradient buckets ----------------------------------------------------------------------------------------------------------------
def bucket_touches(fps, segments, n_params: int, trainable_lo: int = 0):
    """records at or behind a segment's end that still touch its bucket GRADS[4 lo, 4 hi): [(segment, record, lo byte, hi byte)]"""
    g = D.BASE["GRADS"]
    rec, lo, hi = [], [], []
    for i, fp in enumerate(fps):
        iv = fp.touched(g)
        rec += [i] * len(iv)
        lo += iv[:, 0].tolist()
        hi += iv[:, 1].tolist()
    rec, lo, hi = (np.asarray(v, dtype=np.int64) for v in (rec, lo, hi))
    out = []
    for k, (_a, b, slo, shi) in enumerate(segments):
        slo = max(slo, trainable_lo)
        if slo >= shi:
            continue
        m = (rec >= b) & (lo < 4 * shi) & (hi > 4 * slo)
        for i in np.nonzero(m)[0][:5]:
            out.append((k, int(rec[i]), int(max(lo[i], 4 * slo)), int(min(hi[i], 4 * shi))))
    return out


def segments_tile(segments, n_ops: int, n_params: int) -> bool:
    """the op ranges tile [0, n_ops) in order and the buckets tile [0, n_params) from the top down"""
    if not segments:
        return False
    ok = segments[0][0] == 0 and segments[-1][1] == n_ops and segments[0][3] == n_params and segments[-1][2] == 0
    for (a0, b0, lo0, hi0), (a1, b1, lo1, hi1) in zip(segments[:-1], segments[1:]):
        ok = ok and b0 == a1 and lo0 == hi1
    return ok and all(a <= b and lo < hi for a, b, lo, hi in segments)
