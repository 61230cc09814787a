"""CPU: what the cases of tests/test_vit_stages_gpu.py cover, and that its comparison works - no GPU involved.

The stage test runs small plans (cheap, every kind of record, padded token rows) and two full-width shallow ones.  Here the restated
launchers (tests/conv_dispatch.py, wgrad_dispatch.py, vit_dispatch.py) show that the f32 cases together reach every (kind, family,
instantiation) of CONV / WGRAD and every (kind, family) of CHAN_LN_FWD / MAE_LOSS_* that the production plans launch - MAE batch 64,
segmentation batch 16 frozen and unfrozen, built as tests/test_conv_dispatch_cpu.py::_plan_conv_records builds them.  The GPU test
asserts per record that the predicted family is the one that ran.  Change a configuration and this test names what was lost."""
import functools

import pytest
import torch

import s2lc_amd  # noqa: F401
from s2lc_amd.plan import opdefs as D
from tests import plan_harness as H

F32_CASES = [n for n, o in H.STAGE_CASES.items() if o.get("precision", "f32") == "f32"]
# production entries no case reaches, each with the reason it cannot be reached below production size: none for these configurations
UNREACHABLE: dict = {}


@functools.lru_cache(maxsize=None)
def _production_plan(which):
    from s2lc_amd.modules.prithvi import MaskedAutoencoderViT
    from s2lc_amd.modules.prithvi_segmentation import PrithviSegmentationNet, PrithviSegmentationNetConfig
    from s2lc_amd.utils import _prithvi_model_args, load_untrained_prithvi

    if which == "mae":          # Prithvi-100M MAE pre-training, batch 64, mask 0.75
        return load_untrained_prithvi(1)._make_plan(64, True, 0.75, True)
    bb = MaskedAutoencoderViT(**_prithvi_model_args(1), _decoder=False, _flat=False)       # segmentation fine-tuning, batch 16
    return PrithviSegmentationNet(PrithviSegmentationNetConfig(1, 4, 256, 1, 0.1, which == "seg_frozen"), backbone=bb)._make_plan(16, True, 0.0, True)


@functools.lru_cache(maxsize=None)
def _case_plan(name):
    return H.stage_plan(H.stage_case(name))


def _production_set():
    return set().union(*(H.launch_set(_production_plan(w)) for w in ("mae", "seg_frozen", "seg_unfrozen")))


def test_the_f32_cases_reach_every_launch_of_the_production_plans():
    prod = _production_set()
    assert {k for k, *_ in prod} == {"CONV", "WGRAD", "CHAN_LN_FWD", "MAE_LOSS_FWD", "MAE_LOSS_BWD"}
    have = set().union(*(H.launch_set(_case_plan(n)) for n in F32_CASES))
    missing = prod - have
    assert missing == set(UNREACHABLE), f"production launches no stage case reaches: {sorted(missing - set(UNREACHABLE), key=str)}; stale: {sorted(set(UNREACHABLE) - missing, key=str)}"
    assert not UNREACHABLE


def test_the_two_full_width_cases_alone_reach_it():
    """the claim of the configurations themselves: B = 8 for the MAE, B = 1 for the segmentation net (smaller batches of the MAE and
    B = 2 of the segmentation net miss production instantiations)"""
    have = H.launch_set(_case_plan("mae_full_b8")) | H.launch_set(_case_plan("seg_full_b1"))
    assert _production_set() <= have, sorted(_production_set() - have, key=str)
    # ... which the small fixtures do not: every CONV of theirs is the generic kernel
    small = set().union(*(H.launch_set(_case_plan(n)) for n in F32_CASES if "small" in n))
    assert {e[2][0] for e in small if e[0] == "CONV"} == {"conv_igemm_kernel"}


def test_the_full_width_mae_case_reaches_both_layernorm_families():
    fams = {e[1] for e in H.launch_set(_case_plan("mae_full_b8")) if e[0] == "CHAN_LN_FWD"}
    assert fams == {0, 8}


def test_the_small_cases_reach_padded_token_rows_in_encoder_and_decoder():
    plan = _case_plan("mae_small_bs2")
    spec = plan.spec
    rows = {(f["HEADS"] * f["HD"], f["L"], f["LS"]) for prog in (plan.fwd, plan.bwd) for k, f in prog.ops if k in ("ATTN_FWD", "ATTN_BWD")}
    for dim in (spec.embed_dim, spec.decoder_embed_dim):
        assert any(d == dim and ls > l for d, l, ls in rows), (dim, rows)
    seg = _case_plan("seg_small_train_unfrozen")
    assert any(f["LS"] > f["L"] for k, f in seg.fwd.ops if k == "ATTN_FWD")


@pytest.mark.parametrize("name", list(H.STAGE_CASES))
def test_nothing_reads_what_a_contract_leaves_open(name):
    """the two allowances of the comparison (plan_harness.UNSPECIFIED, REPLICATED): no record reads split-K scratch, and statistics
    replicas are read only through the slots that sum them"""
    plan = _case_plan(name)
    for prog in (plan.fwd, plan.bwd):
        if prog is not None:
            assert H.unspecified_reads(prog, plan.const_table) == []


def test_split_cases_flag_what_the_router_routes():
    n = {name: sum(bool(int(f.get("_flags", 0)) & D.FLAG_SPLIT) for prog in (p.fwd, p.bwd) for _, f in prog.ops)
         for name in ("mae_full_b8_split", "seg_full_b1_split") for p in [_case_plan(name)]}
    assert n["seg_full_b1_split"] > 0, n
    assert all(not int(f.get("_flags", 0)) & D.FLAG_SPLIT for name in F32_CASES for p in [_case_plan(name)]
               for prog in (p.fwd, p.bwd) if prog is not None for _, f in prog.ops)


@pytest.mark.parametrize("name,nonfinite", [("mae_small_bs2_dx", []), ("seg_small_train_unfrozen", []), ("seg_small_eval_bwd", []),
                                            ("mae_small_r0_bs2", [("MAE_LOSS_FWD", "LOSS")])])
def test_the_comparison_passes_a_plan_against_itself(name, nonfinite):
    """the GPU test's comparison with the f32 emulation standing in for the GPU: every written range compared, nothing partly
    written (finite exactly where the emulators are), nothing changed outside the written ranges, every error against the f32
    emulator 0"""
    c = H.stage_case(name)
    plan = H.stage_plan(c)
    rf, rb, grads = H.cpu_half(c, plan)
    rf.check(name + " fwd")
    assert rf.nonfinite == nonfinite and rf.compared >= len(plan.fwd.ops)
    assert all(v[0] == 0.0 for v in rf.worst.values())
    if plan.bwd is not None:
        rb.check(name + " bwd")
        assert rb.nonfinite == [] and all(v[0] == 0.0 for v in rb.worst.values())
        assert set(grads) <= set(plan.layout.params) and all(v[0] == 0.0 for v in grads.values())


def test_widen_keeps_integers_and_doubles_floats():
    from s2lc_amd.plan.program import TRef

    img = torch.zeros(64, dtype=torch.uint8)
    img[:16].view(torch.float32).copy_(torch.tensor([1.5, -2.0, float("nan"), 3.0]))
    img[16:32].view(torch.int64).copy_(torch.tensor([7, -9]))
    w = H.widen({0: img}, [TRef(0, 16, (2,), "i64")])[0]
    f = w[:32].view(torch.float64)
    assert f[0] == 1.5 and f[1] == -2.0 and torch.isnan(f[2]) and f[3] == 3.0
    assert w[32:48].view(torch.int64).tolist() == [7, -9]
