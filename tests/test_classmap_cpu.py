"""CPU: `s2k_classmap_filter` is exported (and the stage table and the ABI version did not move), it validates every argument on the host
before anything is launched, the numpy restatement (tests/classmap_ref.py) agrees with a per-pixel loop written from the definition and
with hand cases, and `classmap.majority_filter` / `boundary_to_ignore`, the `TilePredictor` arguments and
`GpuTilePipeline.ignore_label_boundaries` raise ValueError for bad arguments before they refuse to run off the GPU.  The entry is never
called with valid arguments here: there is no device to launch on."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd import _lib, classmap
from s2lc_amd import predict as P
from s2lc_amd.data.gpu_pipeline import GpuTilePipeline
from s2lc_amd.metrics import SegMetrics
from s2lc_amd.plan import opdefs as D
from tests import classmap_ref as R

ROOT = Path(__file__).resolve().parents[1]
S2K_EINVAL, S2K_EFAULT = -22, -14


def test_entry_is_exported_and_the_stage_table_is_unchanged():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g

    g.build()
    L = _lib.lib()
    assert hasattr(ctypes.CDLL(str(g.LIB)), "s2k_classmap_filter")
    assert L.s2k_abi_version() == 2 and len(D.OPS) == 55
    assert "classmap.hip" in g.SOURCES
    hdr = (ROOT / "include" / "s2k.h").read_text()
    assert re.search(r"\bint s2k_classmap_filter\s*\(", hdr) and "#define S2K_ABI_VERSION 2" in hdr
    assert _lib.CLASSMAP_MODES == {"majority": 0, "boundary": 1}
    assert (classmap.STRIP, classmap.BAND, classmap.MAX_CLASSES) == (64, 16, 32)
    assert [classmap.strip_outputs(s) for s in (3, 5, 7, 15)] == [62, 60, 58, 50]


# a valid call over CPU tensors (never made): M, H, W, K = 2, 8, 8, 4, majority, int64 -> int64, with hist and changed
GOOD = dict(M=2, H=8, W=8, K=4, size=3, mode=0, votes=0b1111, fixed=0b0001, ignore=0, nsrc=3, src_bytes=8, dst_bytes=8)
TENSORS = dict(src=torch.zeros(2, 8, 8, dtype=torch.int64), dst=torch.zeros(2, 8, 8, dtype=torch.int64), src_lut=None,
               labels=torch.zeros(3, 8, 8, dtype=torch.uint8), index=torch.zeros(2, dtype=torch.int32), lut=torch.zeros(256, dtype=torch.int32),
               hist=torch.zeros(4, 4, dtype=torch.int64), changed=torch.zeros(2, dtype=torch.int64))


def _call(**change):
    a = {**GOOD, **{k: v for k, v in change.items() if k in GOOD}}
    t = {**TENSORS, **{k: v for k, v in change.items() if k in TENSORS}}
    rc = _lib.classmap_filter(t["src"], t["src_lut"], t["dst"], (a["M"], a["H"], a["W"], a["K"]), a["size"], a["mode"], a["votes"], a["fixed"],
                              a["ignore"], t["labels"], t["index"], t["lut"], a["nsrc"], t["hist"], t["changed"], 0,
                              src_bytes=a["src_bytes"], dst_bytes=a["dst_bytes"])
    return rc, _lib.lib().s2k_last_error().decode()


LUT = torch.zeros(256, dtype=torch.int32)
BOUNDARY = dict(mode=1, votes=0, fixed=0)
BAD = [
    # element widths, the source table, aliasing
    dict(src_bytes=4), dict(src_bytes=0), dict(dst_bytes=2), dict(dst_bytes=16), dict(src_lut=LUT), dict(dst=TENSORS["src"]),
    # K, size, mode
    dict(K=0, votes=0, fixed=0), dict(K=33), dict(K=-1, votes=0, fixed=0), dict(size=1), dict(size=4), dict(size=2), dict(size=17), dict(size=16),
    dict(size=-3), dict(mode=2), dict(mode=-1),
    # mask bits at K and above (majority); any bit, and ignore outside [0, K), in boundary mode
    dict(votes=0b10000), dict(fixed=0b10000), dict(K=2, votes=0b100, fixed=0), dict(votes=0x80000000, fixed=0),
    dict(mode=1, votes=1, fixed=0), dict(mode=1, votes=0, fixed=1), dict(**BOUNDARY, ignore=4), dict(**BOUNDARY, ignore=-1),
    # dims: positive, H * W below 2^31, the grid
    dict(M=0), dict(M=-2), dict(H=0), dict(W=0), dict(H=-8), dict(W=-1), dict(H=65536, W=32768), dict(H=1 << 20, W=1 << 20),
    dict(M=1 << 24), dict(M=1 << 10, H=1 << 14, W=1 << 14),
    # hist needs its three companions and nsrc >= 1
    dict(labels=None), dict(index=None), dict(lut=None), dict(nsrc=0), dict(nsrc=-1),
]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={'t' if isinstance(v, torch.Tensor) else v}" for k, v in b.items()) for b in BAD])
def test_entry_rejects_invalid_arguments_on_the_host(bad):
    rc, msg = _call(**bad)
    assert rc == S2K_EINVAL and msg.startswith("classmap_filter: ") and len(msg) > 25, (rc, msg)


@pytest.mark.parametrize("name", ["src", "dst"])
def test_entry_rejects_a_null_required_pointer(name):
    rc, msg = _call(**{name: None})
    assert rc == S2K_EFAULT and msg.startswith("classmap_filter: null pointer"), (rc, msg)
    with pytest.raises(_lib.S2kError, match="null pointer"):
        _lib.check(rc)


# ---- the restatement against a per-pixel loop over the definition ---------------------------------------------------------------------
def _loop(cls, K, size, mode, votes=None, fixed=(), ignore=0):
    H, W = cls.shape
    r = size // 2
    votes = set(range(K)) if votes is None else set(votes)
    out = cls.copy()
    for y in range(H):
        for x in range(W):
            c = int(cls[y, x])
            if not 0 <= c < K:
                continue
            win = [int(v) for v in cls[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].reshape(-1) if 0 <= v < K]
            if mode == 0:
                n = [sum(1 for v in win if v == k) if k in votes else 0 for k in range(K)]
                best = max(n)
                if not (n[c] == best or best == 0 or c in fixed):
                    out[y, x] = min(k for k in range(K) if n[k] == best)
            elif c != ignore and any(v != c and v != ignore for v in win):
                out[y, x] = ignore
    return out


@pytest.mark.parametrize("case", [(12, 12, 4, 3), (12, 11, 5, 5), (7, 12, 9, 7), (12, 12, 3, 15), (1, 9, 2, 3), (9, 1, 4, 5), (5, 6, 32, 3)],
                         ids=lambda c: "x".join(str(v) for v in c))
def test_restatement_is_the_definition(case):
    H, W, K, size = case
    rng = np.random.default_rng(H * 100 + W)
    cls = rng.integers(0, K, (H, W))
    cls[rng.random((H, W)) < 0.1] = rng.choice([-1, K + 2, 255])
    assert np.array_equal(R.majority(cls, K, size), _loop(cls, K, size, 0))
    votes, fixed = list(range(1, K)), (0,)
    assert np.array_equal(R.majority(cls, K, size, votes, fixed), _loop(cls, K, size, 0, votes, fixed))
    for ignore in {0, K - 1}:
        assert np.array_equal(R.boundary(cls, K, size, ignore), _loop(cls, K, size, 1, ignore=ignore))
    twice = _loop(_loop(cls, K, size, 0), K, size, 0)
    assert np.array_equal(R.majority(cls, K, size, iterations=2), twice)
    assert R.changed(cls, twice).tolist() == [int((cls != twice).sum())]
    stacked = np.stack([cls, cls.T[:H, :W] if H == W else cls[::-1]])
    assert np.array_equal(R.majority(stacked, K, size)[1], _loop(stacked[1], K, size, 0))      # maps never see each other


def test_hand_cases():
    board = np.indices((9, 10)).sum(0) % 2
    assert np.array_equal(R.majority(board, 2, 3), board)                      # the centre wins the 4 : 5 and the edge ties
    salt = np.full((7, 7), 2)
    salt[3, 3] = 1
    assert np.array_equal(R.majority(salt, 4, 3), np.full((7, 7), 2)) and R.changed(salt, R.majority(salt, 4, 3)).tolist() == [1]
    const = np.full((15, 15), 31)
    assert R.window_counts(const, 32, 15)[31, 7, 7] == 225 and np.array_equal(R.majority(const, 32, 15), const)
    rng = np.random.default_rng(3)
    m = rng.integers(0, 4, (16, 16))
    out = R.majority(m, 4, 5, votes=(1, 2, 3), fixed=(0,))
    assert np.array_equal(out == 0, m == 0) and (out != m).any()                # the zero set exactly as it was
    # a pixel touching only the ignored class is no boundary; one touching another class is; the ignored class never changes
    lab = np.array([[0, 0, 0, 0, 0, 0], [0, 1, 1, 1, 2, 2], [0, 1, 1, 1, 2, 2], [0, 0, 0, 0, 0, 0]])
    want = np.array([[0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 2], [0, 1, 1, 0, 0, 2], [0, 0, 0, 0, 0, 0]])
    assert np.array_equal(R.boundary(lab, 3, 3, 0), want)
    assert R.confusion([0, 1, 5, 2, -1], [1, 1, 1, 9, 0], 3).tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 0]]


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def _cpu_pipe(labels=True, label_map="cnes-multiclass"):
    p = GpuTilePipeline([0.1] * 4, [0.2] * 4, random_crop_size=8, label_map=label_map, device="cpu")
    g = torch.Generator().manual_seed(0)
    p.load(torch.randint(-100, 100, (3, 4, 16, 16), generator=g, dtype=torch.int32).to(torch.int16),
           torch.randint(0, 24, (3, 16, 16), generator=g, dtype=torch.int32).to(torch.uint8) if labels else None)
    return p


def test_validators_raise_before_the_gpu_refusal():
    m = torch.zeros(2, 8, 8, dtype=torch.int64)
    pipe = _cpu_pipe()
    pred = P.TilePredictor(lambda x: x, pipe, 4)
    metrics = SegMetrics(4, device="cpu")
    pal = torch.zeros(4, 3, dtype=torch.uint8)
    bad = [
        lambda: classmap.majority_filter(m, 4, size=4), lambda: classmap.majority_filter(m, 4, size=1), lambda: classmap.majority_filter(m, 4, size=17),
        lambda: classmap.majority_filter(m, 4, size=3.0), lambda: classmap.majority_filter(m, 0), lambda: classmap.majority_filter(m, 33),
        lambda: classmap.majority_filter(m, 4, votes=(1, 4)), lambda: classmap.majority_filter(m, 4, fixed=(4,)),
        lambda: classmap.majority_filter(m, 4, votes=(-1,)), lambda: classmap.majority_filter(m, 4, iterations=0),
        lambda: classmap.majority_filter(m, 4, iterations=-2), lambda: classmap.majority_filter(m.float(), 4),
        lambda: classmap.majority_filter(m.int(), 4), lambda: classmap.majority_filter(m[0, 0], 4), lambda: classmap.majority_filter(m[:0], 4),
        lambda: classmap.majority_filter(m.numpy(), 4),
        lambda: classmap.boundary_to_ignore(m, 4, size=2), lambda: classmap.boundary_to_ignore(m, 4, size=1), lambda: classmap.boundary_to_ignore(m, 4, size=17),
        lambda: classmap.boundary_to_ignore(m, 0), lambda: classmap.boundary_to_ignore(m, 33), lambda: classmap.boundary_to_ignore(m, 4, ignore_index=4),
        lambda: classmap.boundary_to_ignore(m, 4, ignore_index=-1), lambda: classmap.boundary_to_ignore(m.double(), 4),
        lambda: pred.predict(majority=4), lambda: pred.predict(majority=1), lambda: pred.predict(majority=17), lambda: pred.predict(majority=3, iterations=0),
        lambda: pred.evaluate(metrics, majority=6), lambda: pred.evaluate(metrics, majority=3, iterations=0),
        lambda: pred.evaluate(metrics, [7], majority=3), lambda: pred.render([0], pal, majority=8), lambda: pred.render([0], pal, majority=3, iterations=-1),
        lambda: P.TilePredictor(lambda x: x, _cpu_pipe(labels=False), 4).evaluate(metrics, majority=3),
        lambda: pipe.ignore_label_boundaries(size=4), lambda: pipe.ignore_label_boundaries(size=1), lambda: pipe.ignore_label_boundaries(size=17),
        lambda: pipe.ignore_label_boundaries(ignore_index=4), lambda: pipe.ignore_label_boundaries(ignore_index=-1),
        lambda: _cpu_pipe(labels=False).ignore_label_boundaries(),
        lambda: _cpu_pipe(label_map="osm-multiclass").ignore_label_boundaries(),      # an identity map names 256 classes: beyond the filter's 32
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} did not raise")


def test_the_new_functions_refuse_the_cpu():
    m = torch.zeros(2, 8, 8, dtype=torch.int64)
    pipe = _cpu_pipe()
    pred = P.TilePredictor(lambda x: x, pipe, 4)
    pal = torch.zeros(4, 3, dtype=torch.uint8)
    calls = (lambda: classmap.majority_filter(m, 4), lambda: classmap.majority_filter(m[0].to(torch.uint8), 32, 15, 3, (1, 2), (0,), True),
             lambda: classmap.boundary_to_ignore(m, 4), lambda: classmap.boundary_to_ignore(m.to(torch.uint8), 2, 7, 1),
             lambda: pred.predict(majority=5, iterations=2), lambda: pred.evaluate(SegMetrics(4, device="cpu"), [0, 2], majority=3),
             lambda: pred.render([1], pal, majority=3), lambda: pipe.ignore_label_boundaries(), lambda: pipe.ignore_label_boundaries(5, 3))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert pipe.label_classes == 4 and int(pipe.lut.max()) == 3      # nothing was rewritten
