"""The kernels that carry parameters to the convolutions and gradients back - WEIGHT_PACK (weight_pack_kernel, _bf16_, _q4_ and
_split_kernel), WGRAD_FINALIZE, AXPY, SPACE_TO_DEPTH, IM2COL (csrc/ew.hip) and MEMSET (csrc/s2k_api.hip) - bit for bit.

All of them move data, plus one add (WGRAD_FINALIZE, AXPY) or one rounding (the bf16 / hi-mid-lo copies), so nothing here has a
tolerance: each test is a one-record program through the C ABI over a tests/test_ops_gpu.Case arena whose every tensor has a
256-byte NaN guard in front and behind, every destination is uploaded NaN-filled, and the WHOLE arena image after the run must equal
`upload + the writes tests/pack_ref.py states` byte for byte - the guards, the quad areas of unflagged rows, the gaps between the
entries and the slack between allocations included.  Layout cases use a seeded permutation of distinct, exactly representable floats,
so a value in the wrong place can never equal the right one.  tests/test_pack_ref_cpu.py holds the reference to the oracle and the
planners' tables to what the kernels assume.

Reached: weight_pack_kernel both branches (LDS transpose `kfast` / lanes along m) at T = 1 and T = 9, every planner stride pattern,
ragged and exact M / K tiles, the per-workgroup binary search on 1 / 2 / 3 / 33 rows with mixed MP, T and quad flags and gaps
between the entries, all four mirror combinations the plans emit; the rounding of the bf16 and split copies on ties, carries, +-0,
+-Inf and the largest finite f32; the launcher's refusals; wgrad_finalize_kernel's search and its grid-stride second trip
(TOTAL > 4096 x 256); axpy_kernel's float4 and tail loops and the float4 loop's second trip (COUNT > 2048 x 256 x 4); both
SPACE_TO_DEPTH kernels and the scalar one's second trip (> 65536 x 256 elements); IM2COL's float4 and ragged stores.

Left out: denormal weights, and weights whose mid / lo terms are denormal, in the bf16 / split copies - how the hardware conversion
treats them is not pinned anywhere in the project; and misaligned AXPY operands (the kernel casts to float4 unconditionally; the
plans' operands are checked on the CPU)."""
import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan.program import Program, TRef
from tests import pack_ref as PR
from tests.test_ops_gpu import WS, Case

pytestmark = pytest.mark.gpu

GUARD_FLOATS = 64          # 256 bytes
NAN16 = 0x7fc1             # a bf16 NaN: the fill of the 2-byte mirror regions


class ByteCase(Case):
    """Case with a NaN guard around every tensor and a byte-for-byte comparison of the whole arena"""

    def __init__(self, seed=0):
        super().__init__(seed)
        self.n_guards = 0
        self._guard()

    def _guard(self):
        Case.t(self, f"guard{self.n_guards}", (GUARD_FLOATS,), "nan")
        self.n_guards += 1

    def t(self, name, shape, fill="randn", dtype="f32", scale=1.0):
        ref = Case.t(self, name, shape, fill, dtype, scale)
        self._guard()
        return ref

    def arena_ref(self) -> TRef:
        """byte 0 of the arena: the SRC / DST of a table whose offsets count from there"""
        return TRef(WS, 0, (1,), "f32", "arena")

    def launch(self, kind, **fields) -> np.ndarray:
        """one record over this arena; leaves the uploaded image in self.sent and the image after the run in self.got (also when
        the launcher refuses the record)"""
        from s2lc_amd import _lib

        prog = Program()
        prog.add(kind, **fields)
        self.sent = self.image().numpy()
        gpu = torch.from_numpy(self.sent).cuda()
        try:
            _lib.run(prog.pack(), _lib.Bases().set("WS", gpu), torch.cuda.current_stream().cuda_stream)
        finally:
            torch.cuda.synchronize()
            self.got = gpu.cpu().numpy()
        return self.got

    def owner(self, at: int) -> str:
        for name, (ref, _) in self.items.items():
            if ref.off <= at < ref.off + ref.nbytes:
                return f"{name} + {at - ref.off}"
        return "the slack between allocations"

    def same(self, want: np.ndarray, what: str, got: np.ndarray | None = None):
        got = self.got if got is None else got
        assert got.size == want.size
        if np.array_equal(got, want):
            return
        bad = np.flatnonzero(got != want)
        at = int(bad[0]) & ~3
        raise AssertionError(f"{what}: {bad.size} bytes differ from upload + reference writes, first at byte {int(bad[0])} ({self.owner(int(bad[0]))}): "
                             f"got {got[at:at + 4].tobytes().hex()}, expected {want[at:at + 4].tobytes().hex()}; last at byte {int(bad[-1])} "
                             f"({self.owner(int(bad[-1]))})")

    def put(self, want: np.ndarray, ref: TRef, data: np.ndarray):
        b = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert b.size == ref.nbytes
        want[ref.off:ref.off + ref.nbytes] = b


def distinct(n, gen, first=1):
    """n distinct non-zero floats k / 4 in a seeded order (exact in f32 up to 2^24 / 4 values)"""
    assert first + n < 1 << 24
    return torch.from_numpy((np.arange(first, first + n, dtype=np.float32) * np.float32(0.25))[gen.permutation(n)])


def spread(n, gen):
    """2^-20 .. 2^20, random signs, all 23 stored significand bits random (tests/test_b16_kernels_gpu.spread)"""
    return (gen.choice([-1.0, 1.0], n) * (1.0 + gen.random(n)) * 2.0 ** gen.integers(-20, 21, n)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# WEIGHT_PACK
# ---------------------------------------------------------------------------------------------------------------------------------------
MIRRORS = {"none": (), "q4": ("Q4_BASE",), "bf16": ("BF16_BASE",), "q4+split": ("Q4_BASE", "SPLIT_BASE")}     # what the plans emit


def kfast(row) -> bool:
    """weight_pack_kernel's LDS-transpose branch: (k, tap) contiguous in the source and no tap reversal"""
    return row[7] == 1 and row[6] == row[4] and not row[8] & 1


def pack_case(entries, mirrors, seed, values=None):
    """A WEIGHT_PACK record over `entries` = [(floats of the parameter, [src_elem_off, M, K, T, s_m, s_k, s_t, flip]), ...]: the packs
    lie in one NaN-filled zone with gaps of 256 .. 384 bytes in front of, between and behind them, each mirror region is a NaN-filled
    tensor of its own, each parameter a tensor of its own.  values(i, n): the parameter's floats (default: distinct over the case).
    -> (case, fields, rows)"""
    gen = np.random.default_rng(seed)
    c = ByteCase(seed)
    sizes = [((e[1] + 127) // 128 * 128) * e[3] * ((e[2] + 63) // 64 * 64) for _, e in entries]
    gaps = [GUARD_FLOATS + 8 * (i % 5) for i in range(len(entries) + 1)]
    zone_floats = sum(sizes) + sum(gaps)
    zone = c.t("zone", (zone_floats,), "nan")
    fields = {}
    if "BF16_BASE" in mirrors:
        m16 = c.t("mirror_bf16", (zone_floats,), torch.full((zone_floats,), NAN16, dtype=torch.int16), "i16")
        fields["BF16_BASE"] = m16.off - zone.off // 2
    if "Q4_BASE" in mirrors:
        mq = c.t("mirror_quad", (zone_floats,), "nan")
        fields["Q4_BASE"] = mq.off - zone.off
    if "SPLIT_BASE" in mirrors:
        ms = c.t("mirror_split", (3 * zone_floats,), torch.full((3 * zone_floats,), NAN16, dtype=torch.int16), "i16")
        fields["SPLIT_BASE"] = ms.off - 3 * zone.off // 2
    assert all(v > 0 and v % 16 == 0 for v in fields.values())
    flat, dst_offs, at, first = [], [], zone.off // 4, 1
    for i, ((n_src, e), size) in enumerate(zip(entries, sizes)):
        at += gaps[i]
        dst_offs.append(at)
        at += size
        data = distinct(n_src, gen, first) if values is None else values(i, n_src)
        first += n_src
        w = c.t(f"w{i}", (n_src,), data)
        flat.append([w.off // 4 + e[0]] + list(e[1:]))
    rows, total = PR.table_rows(flat, dst_offs)
    tab = c.t("table", (len(rows), 12), torch.tensor(rows, dtype=torch.int32), "i32")
    fields.update(TABLE=tab, SRC=c.arena_ref(), DST=c.arena_ref(), TOTAL=total, N_ENTRIES=len(rows))
    return c, fields, rows


def pack_want(c, fields, rows):
    src = c.sent.view(np.float32)
    return PR.apply(c.sent.copy(), 0, PR.weight_pack_writes(rows, src, fields.get("BF16_BASE", 0), fields.get("Q4_BASE", 0),
                                                           fields.get("SPLIT_BASE", 0)))


def test_single_rows_reach_both_branches_at_one_and_nine_taps():
    hit = set()
    for pattern, M, K, T in PR.SINGLE_ROWS:
        rows, _ = PR.table_rows([PR.pattern_row(pattern, M, K, T)[1]], [0])
        assert kfast(rows[0]) == PR.PATTERNS[pattern][1], pattern
        hit.add((kfast(rows[0]), T))
    assert {(True, 1), (False, 1), (True, 9), (False, 9), (True, 25)} <= hit
    assert {r[1] for r in PR.SINGLE_ROWS} == {24, 128, 130} and {r[2] for r in PR.SINGLE_ROWS} == {13, 64, 65, 200}
    assert {r[0] for r in PR.SINGLE_ROWS} == set(PR.PATTERNS)


@pytest.mark.parametrize("mirrors", list(MIRRORS))
@pytest.mark.parametrize("pattern,M,K,T", PR.SINGLE_ROWS, ids=["-".join(str(v) for v in r) for r in PR.SINGLE_ROWS])
def test_weight_pack_single_row(pattern, M, K, T, mirrors):
    n_src, e = PR.pattern_row(pattern, M, K, T)
    if T == 1 and "Q4_BASE" in MIRRORS[mirrors]:
        e[7] |= 2                                             # a 1x1 entry a FLAG_Q4 stage reads
    c, fields, rows = pack_case([(n_src, e)], MIRRORS[mirrors], seed=M + 3 * K + 7 * T)
    assert kfast(rows[0]) == PR.PATTERNS[pattern][1]
    c.launch("WEIGHT_PACK", **fields)
    c.same(pack_want(c, fields, rows), f"WEIGHT_PACK {pattern} {'kfast' if kfast(rows[0]) else 'lanes along m'} [{mirrors}]")


# (pattern, M, K, T, quad flag): T = 1 and 9, MP = 128 and 256, flagged and unflagged 1x1 rows, both branches
MULTI = [("dense_fwd", 24, 13, 1, True), ("dense_fwd", 130, 13, 9, False), ("linear_dgrad", 130, 64, 1, False), ("concat_dgrad", 24, 65, 9, False),
         ("linear_fwd", 128, 200, 1, True), ("convt_fwd", 24, 13, 1, False), ("concat_dgrad", 130, 13, 1, True), ("dense_fwd", 24, 65, 9, False)]


@pytest.mark.parametrize("mirrors", list(MIRRORS))
@pytest.mark.parametrize("n_rows", [1, 2, 3, 33])
def test_weight_pack_multi_row(n_rows, mirrors):
    """every kernel resolves its row per workgroup (binary search over `start`): with distinct values and the whole arena compared, the
    first and the last workgroup of every row must have landed in that row"""
    entries = []
    for i in range(n_rows):
        pattern, M, K, T, quad = MULTI[i % len(MULTI)]
        n_src, e = PR.pattern_row(pattern, M, K, T)
        e[7] |= 2 if quad else 0
        entries.append((n_src, e))
    c, fields, rows = pack_case(entries, MIRRORS[mirrors], seed=100 + n_rows)
    if n_rows >= 3:
        assert {r[9] for r in rows} == {128, 256} and {r[4] for r in rows} == {1, 9}
        assert any(PR.q4_wanted(r) for r in rows) and any(r[4] == 1 and not PR.q4_wanted(r) for r in rows)
    c.launch("WEIGHT_PACK", **fields)
    c.same(pack_want(c, fields, rows), f"WEIGHT_PACK {n_rows} rows [{mirrors}]")


def _rounding_values(n, seed, nans=False):
    gen = np.random.default_rng(seed)
    v = spread(n, gen)
    tie = PR.tie_vector()
    v[gen.permutation(n)[:tie.size]] = tie
    if nans:
        pats = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff812345, 0x7fffffff, 0x7fc00001], dtype=np.uint32)
        where = gen.permutation(n)[:48]
        v.view(np.uint32)[where] = np.resize(pats, 48)
    return torch.from_numpy(v)


@pytest.mark.parametrize("mirrors", ["bf16", "q4+split"])
def test_weight_pack_rounding_and_special_values(mirrors):
    """ties to even and to odd, one ulp either side, carries, +-0, +-Inf, +-0x7f7fffff (-> Inf; hi not finite: mid = lo = 0) and values
    over 2^-20 .. 2^20 with every significand bit random: the bf16 copy and the hi / mid / lo planes are bit-exact"""
    n_src, e = PR.pattern_row("dense_fwd", 130, 65, 1)
    e[7] |= 2
    c, fields, rows = pack_case([(n_src, e)], MIRRORS[mirrors], seed=7, values=lambda i, n: _rounding_values(n, 11))
    c.launch("WEIGHT_PACK", **fields)
    c.same(pack_want(c, fields, rows), f"WEIGHT_PACK rounding [{mirrors}]")


@pytest.mark.parametrize("mirrors", ["bf16", "q4+split"])
def test_weight_pack_nan_weights_by_position(mirrors):
    """NaN weights: a NaN wherever the reference has one - in the f32 pack, the quad copy, the bf16 copy and the hi plane - with
    mid = lo = 0 there; the payload is not compared.  Every other byte of the arena is compared as it is."""
    n_src, e = PR.pattern_row("dense_fwd", 130, 65, 1)
    e[7] |= 2
    c, fields, rows = pack_case([(n_src, e)], MIRRORS[mirrors], seed=8, values=lambda i, n: _rounding_values(n, 12, nans=True))
    c.launch("WEIGHT_PACK", **fields)
    want, got = pack_want(c, fields, rows), c.got.copy()
    n = PR.entry_floats(rows[0])
    d = rows[0][1]
    wide = [(4 * d, n)] + ([(PR.q4_addr(fields["Q4_BASE"], d), n)] if "Q4_BASE" in fields else [])
    narrow = ([(PR.bf16_addr(fields["BF16_BASE"], d), n)] if "BF16_BASE" in fields else []) + \
             ([(PR.split_addr(fields["SPLIT_BASE"], d, 0, n), 3 * n)] if "SPLIT_BASE" in fields else [])
    n_nan = 0
    for img in (want, got):         # inside what the record writes, every NaN becomes one and the same NaN
        for a, cnt in wide:
            u = img[a:a + 4 * cnt].view(np.uint32)
            isnan = (u & 0x7fffffff) > 0x7f800000
            u[isnan] = 0x7fc00000
            n_nan += int(isnan.sum())
        for a, cnt in narrow:
            u = img[a:a + 2 * cnt].view(np.uint16)
            isnan = (u & 0x7fff) > 0x7f80
            u[isnan] = 0x7fc0
            n_nan += int(isnan.sum())
    c.same(want, f"WEIGHT_PACK NaN weights [{mirrors}]", got)
    assert n_nan >= 2 * 2 * 48          # the f32 pack and at least one copy, in both images


@pytest.mark.parametrize("what", ["total_not_a_multiple_of_4096", "no_entries", "bf16_base_misaligned", "q4_base_misaligned", "split_base_misaligned"])
def test_weight_pack_refusals_leave_the_arena_as_uploaded(what):
    from s2lc_amd._lib import S2kError

    n_src, e = PR.pattern_row("dense_fwd", 24, 13, 1)
    e[7] |= 2
    c, fields, rows = pack_case([(n_src, e)], ("BF16_BASE", "Q4_BASE", "SPLIT_BASE"), seed=9)
    if what == "total_not_a_multiple_of_4096":
        fields["TOTAL"] += 2048
    elif what == "no_entries":
        fields["N_ENTRIES"] = 0
    else:
        fields[what.split("_")[0].upper() + "_BASE"] += 8
    with pytest.raises(S2kError, match="weight_pack"):
        c.launch("WEIGHT_PACK", **fields)
    c.same(c.sent, f"WEIGHT_PACK refused ({what})")


# ---------------------------------------------------------------------------------------------------------------------------------------
# WGRAD_FINALIZE
# ---------------------------------------------------------------------------------------------------------------------------------------
def _finalize_case(shapes, seed):
    """rows {off, M, C, T, start} in the order of `shapes`; their offsets lie in a seeded order with odd gaps in between"""
    gen = np.random.default_rng(seed)
    order = gen.permutation(len(shapes))
    offs, at = [0] * len(shapes), 5
    for slot, i in enumerate(order):
        M, C, T = shapes[i]
        offs[i] = at
        at += M * C * T + 3 + 2 * (slot % 4)
    n = at + 7
    rows, start = [], 0
    for (M, C, T), off in zip(shapes, offs):
        rows.append([off, M, C, T, start])
        start += M * C * T
    c = ByteCase(seed)
    wgs = c.t("wgs", (n,), torch.from_numpy(gen.standard_normal(n).astype(np.float32)))
    grads = c.t("grads", (n,), torch.from_numpy(gen.standard_normal(n).astype(np.float32)))
    tab = c.t("table", (len(rows), 5), torch.tensor(rows, dtype=torch.int32), "i32")
    return c, rows, start, dict(TABLE=tab, WGS=wgs, GRADS=grads, TOTAL=start, N_ENTRIES=len(rows))


def _finalize_shapes(n):
    Ms, Cs, Ts = (3, 5, 7, 9, 11), (1, 3, 5, 13), (1, 4, 9, 25)
    return [(Ms[i % 5], Cs[(i // 2) % 4], Ts[i % 4]) for i in range(n)]


@pytest.mark.parametrize("shapes", [_finalize_shapes(1), _finalize_shapes(2), _finalize_shapes(3), _finalize_shapes(40),
                                    [(351, 349, 9), (5, 3, 4)]], ids=["1", "2", "3", "40", "second_trip"])
def test_wgrad_finalize_exact(shapes):
    """GRADS (random before) += the scratch in parameter order, one f32 add per element, nothing between the entries touched;
    second_trip: TOTAL > 4096 x 256, the grid stride loops, and the loop's last elements fall into the second row"""
    c, rows, total, fields = _finalize_case(shapes, seed=len(shapes))
    if len(shapes) == 40:
        assert {r[3] for r in rows} == {1, 4, 9, 25} and sorted(r[0] for r in rows) != [r[0] for r in rows]
    if shapes[0][0] == 351:
        assert total > 4096 * 256
    c.launch("WGRAD_FINALIZE", **fields)
    want = c.sent.copy()
    wgs, grads = (c.sent[r.off:r.off + r.nbytes].view(np.float32) for r in (fields["WGS"], fields["GRADS"]))
    c.put(want, fields["GRADS"], PR.wgrad_fold(rows, wgs, grads))
    assert not np.array_equal(want, c.sent)
    c.same(want, f"WGRAD_FINALIZE {len(shapes)} rows")


# ---------------------------------------------------------------------------------------------------------------------------------------
# AXPY, MEMSET
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3, 4, 5, 1023, 1027, 2048 * 256 * 4 + 7])
def test_axpy_exact(count):
    """Y[:COUNT] += X[:COUNT] as one f32 add; the float4 loop (COUNT / 4 vectors), the scalar tail (COUNT % 4) and, at the last size,
    the float4 loop's second grid-stride trip; the elements behind COUNT stay.  Operands are 16-byte aligned (arena allocations)."""
    gen = np.random.default_rng(count)
    c = ByteCase(count)
    x = c.t("x", (count + 9,), torch.from_numpy(gen.standard_normal(count + 9).astype(np.float32)))
    y = c.t("y", (count + 9,), torch.from_numpy(gen.standard_normal(count + 9).astype(np.float32)))
    assert x.off % 16 == 0 and y.off % 16 == 0
    c.launch("AXPY", X=x, Y=y, COUNT=count)
    want = c.sent.copy()
    xs, ys = (c.sent[r.off:r.off + r.nbytes].view(np.float32) for r in (x, y))
    out = ys.copy()
    out[:count] = ys[:count] + xs[:count]
    c.put(want, y, out)
    c.same(want, f"AXPY {count}")


@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("nbytes", [1, 3, 4, 2000, 4097])
def test_memset_exact(nbytes, offset):
    gen = np.random.default_rng(nbytes)
    c = ByteCase(nbytes)
    z = c.t("z", (8192,), torch.from_numpy(gen.integers(1, 256, 8192).astype(np.uint8)), "u8")
    c.launch("MEMSET", DST=z.at(offset), BYTES=nbytes)
    want = c.sent.copy()
    want[z.off + offset:z.off + offset + nbytes] = 0
    c.same(want, f"MEMSET {nbytes} bytes at {offset}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# SPACE_TO_DEPTH, IM2COL
# ---------------------------------------------------------------------------------------------------------------------------------------
def s2d_kernel(W) -> str:
    """launch_space_to_depth: rows of whole float4s go to space_to_depth_kernel, every other width to the grid-stride scalar kernel"""
    return "float4" if W % 4 == 0 else "scalar"


S2D = [(B, C, H, W, k) for W, k in [(4, "float4"), (8, "float4"), (12, "float4"), (1, "scalar"), (5, "scalar"), (6, "scalar"), (7, "scalar")]
       for H in (1, 3) for B, C in ((1, 1), (2, 3))]
S2D.append((2, 8, 512, 513, "scalar"))      # 16.8 M output elements > 65536 x 256: the scalar kernel's grid stride loops


@pytest.mark.parametrize("B,C,H,W,kernel", S2D, ids=["-".join(str(v) for v in r) for r in S2D])
def test_space_to_depth_exact_both_kernels(B, C, H, W, kernel):
    assert s2d_kernel(W) == kernel
    n = B * C * 4 * H * W
    if n > 65536 * 256:
        xv = (np.arange(n, dtype=np.uint32) + np.uint32(0x3f800000)).view(np.float32)      # distinct finite bit patterns
    else:
        xv = distinct(n, np.random.default_rng(n)).numpy()
    c = ByteCase(n % 1000)
    x = c.t("x", (B, C, 2 * H, 2 * W), torch.from_numpy(xv))
    y = c.t("y", (B, 4 * C, H, W), "nan")
    c.launch("SPACE_TO_DEPTH", X=x, Y=y, B=B, C=C, H=H, W=W)
    want = c.sent.copy()
    c.put(want, y, PR.space_to_depth(xv.reshape(B, C, 2 * H, 2 * W)))
    c.same(want, f"SPACE_TO_DEPTH {kernel} kernel")


def _same_pads(n, k, s):
    from s2lc_amd.plan.unet_plan import same_pads

    return same_pads(n, k, s)


def _tf_same(B, C, H, W, k, s):
    (Ho, pt), (Wo, pl) = _same_pads(H, k, s), _same_pads(W, k, s)
    return (B, C, H, W, k, s, pt, pl, Ho, Wo)


IM2COL = [_tf_same(2, 13, 32, 32, 3, 2), _tf_same(1, 3, 15, 22, 3, 2), _tf_same(2, 4, 17, 17, 5, 2), _tf_same(1, 2, 12, 20, 3, 3),   # tests/test_ops_gpu
          # stride 1, symmetric padding; WO % 4 = 0, 1, 2, 3; 9 and 25 taps
          (2, 3, 8, 8, 3, 1, 1, 1, 8, 8), (1, 2, 7, 9, 3, 1, 1, 1, 7, 9), (2, 2, 6, 10, 5, 1, 2, 2, 6, 10), (1, 3, 5, 11, 5, 1, 2, 2, 5, 11),
          (1, 2, 9, 7, 3, 1, 1, 1, 9, 7), (1, 2, 6, 12, 5, 1, 2, 2, 6, 12)]


def test_im2col_cases_cover_every_store_form():
    s1 = [r for r in IM2COL if r[5] == 1]
    assert all(r[6] == (r[4] - 1) // 2 == r[7] and r[8] == r[2] and r[9] == r[3] for r in s1)
    assert {r[9] % 4 for r in s1} == {0, 1, 2, 3} and {r[4] ** 2 for r in s1} == {9, 25}
    assert {(r[9] % 4 == 0, r[4] ** 2) for r in s1} >= {(True, 9), (True, 25), (False, 9), (False, 25)}


@pytest.mark.parametrize("B,C,H,W,k,s,pt,pl,HO,WO", IM2COL, ids=["-".join(str(v) for v in r) for r in IM2COL])
def test_im2col_exact_whole_arena(B, C, H, W, k, s, pt, pl, HO, WO):
    """distinct non-zero values, padded taps exactly +0.0, the arena outside Y as uploaded; WO % 4 == 0: one float4 store per thread,
    otherwise guarded scalar stores"""
    n = B * C * H * W
    xv = distinct(n, np.random.default_rng(n)).numpy()
    c = ByteCase(n % 1000)
    x = c.t("x", (B, C, H, W), torch.from_numpy(xv))
    y = c.t("y", (B, C * k * k, HO, WO), "nan")
    c.launch("IM2COL", X=x, Y=y, B=B, C=C, H=H, W=W, KH=k, KW=k, STRIDE=s, PAD_T=pt, PAD_L=pl, HO=HO, WO=WO)
    ref = PR.im2col(xv.reshape(B, C, H, W), k, k, s, pt, pl, HO, WO)
    if pt or pl:
        assert (ref.view(np.uint32) == 0).any()            # some taps are padding: +0.0, bit for bit
    want = c.sent.copy()
    c.put(want, y, ref)
    c.same(want, f"IM2COL {'float4' if WO % 4 == 0 else 'ragged'} stores")
