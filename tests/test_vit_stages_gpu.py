"""The planned Prithvi programs (plan/vit_plan.py: plan_mae, plan_seg and the four method plans) on the GPU, stage by stage, against
the CPU emulation of the same program (oracle/ops_ref.py) - what tests/test_unet_gpu.py::test_programs_stage_by_stage_vs_emulator is
to the U-Net plans, but strict: every byte range a program writes is compared (row padding L..LS-1 included, by byte range, nothing
skipped because "the oracle is not finite"), and every other byte of the workspace, the outputs, the gradients, the buffers and the
packs must still be what it was - the NaN poison, the uploaded value or the forward's result.

A. Whole programs (test_whole_programs, test_method_programs).  Forward over a NaN-poisoned workspace; then both emulators (f32 and
   float64) continue from the GPU's post-forward state and the backward is compared the same way, GRADS parameter by parameter
   against the parameter's own max |ref|.  Every case also asserts, record by record, that the kernel family the library reports
   (profiled on a second copy of the buffers) is the one the restated launchers predict - tests/test_vit_stage_cover_cpu.py proves on
   the CPU that these cases reach every instantiation of the production plans; here it is shown that they ran.
B. One record at a time (test_one_record_at_a_time), on the small MAE (norm_pix_loss) and segmentation (unfrozen, train) plans:
   each record runs alone through the library AND through both emulators from the GPU's state before it, so an early error cannot
   excuse a later one.  No record of these plans is bound to its neighbours (no FLAG_CHAIN: asserted), so every step is one record.

Bars (tests/plan_harness.py, OP_BAR - nothing new, each number is the kind's own op-test bar: tests/test_vit_kernels_gpu.py's
docstring for LayerNorm 2e-5 / 1e-4, attention 1e-4 / 2e-4, MAE loss 2e-5, activations 1e-5; tests/test_ops_gpu.py for CONV 1e-4,
WGRAD 2e-4, CHANNEL_SUM and the head's BatchNorm stages 1e-4; index outputs and data movement bit for bit):
   B: the op bar, against the f32 and the float64 emulator;
   A: max(op bar, 8 E) per range and per parameter gradient, E = the f32 emulator's own distance from the float64 emulator there
      (the `stress` rule of tests/test_vit_kernels_gpu.py::_check); a stage that only moves values or adds once inherits the bar of
      the tensor it moves.  A parameter whose float64 gradient is below 1e-7 of the network's largest is held to 1e-5 of that largest
      gradient (the U-Net stage test's rule); frozen / absent gradients and head.net.0.bias are exactly 0.
No tensor is exempt.  Two contracts leave content open and are handled by name in plan_harness (UNSPECIFIED, REPLICATED): a CONV's
split-K SCRATCH (no ViT plan has one) and the [NREP][2][C] statistics replicas, compared as their sum.

The full-width segmentation case (940 MB workspace) is compared against both emulators like every other case.
f32-split: the same two full-width cases at the same bars (tests/test_f32_split_ops_gpu.py holds the split kernels to the f32 op
tolerance; the emulator computes flagged stages in exact f32); every FLAG_SPLIT record must have run family 5.

Measured worst figures (records, not bars) are printed per kind and passed to record_property.  First green run on an MI355X, the
larger of the two errors, worst case of all:
   A: CONV 5.4e-6, WGRAD 1.8e-6, CHAN_LN_FWD 1.7e-6, CHAN_LN_BWD 2.7e-6, ATTN_FWD 1.4e-6, ATTN_BWD 2.1e-6, ACT_FWD 2.1e-6, ACT_BWD
      2.6e-6, MAE_LOSS_FWD 3.8e-8, MAE_LOSS_BWD 9.7e-8, BN_FINALIZE 3.1e-7, BN_BWD_REDUCE / _APPLY 2.0e-7, TOKEN_GATHER 1.5e-6,
      TOKEN_SCATTER 2.7e-6, WGRAD_FINALIZE 7.1e-7, AXPY 9.7e-8, PATCHIFY (inverse) 4.9e-7; index stages, MEMSET, WEIGHT_PACK (quad and
      split copies included) and DROP_GATE bit for bit.  CHANNEL_SUM 2.4e-5 in f32 plans; 1.8e-4 in seg_full_b1_split, where the bar
      is 8 E = 2.3e-4: neck.feature_pyramid_net.7.bias, 50,176 gradients per channel of the split 3x3 data gradient summed to a
      value 1e-4 of their magnitude - the closest figure of the file, and the worst parameter gradient; every other one < 3e-6.
   B: CONV 8.8e-7, WGRAD 4.4e-7, CHAN_LN_FWD 2.2e-7, CHAN_LN_BWD 2.7e-7, ATTN_FWD 2.3e-7, ATTN_BWD 3.1e-7, ACT_FWD 2.0e-7, ACT_BWD
      1.2e-7, MAE_LOSS 9.7e-8, CHANNEL_SUM 1.2e-6, BN stages 1.3e-7, TOKEN_SCATTER 5.5e-8; everything else bit for bit.
What it found: TOKEN_GATHER without FILL writes 0 for a negative index (plan_random_masking's cls slot), the emulator copied token
0 - oracle/ops_ref.py and the contract line in opdefs.py now say 0; tests/test_vit_kernels_gpu.py has the single-record case."""
import pytest
import torch

import s2lc_amd  # noqa: F401
from oracle import ops_ref
from oracle import prithvi_ref as P
from s2lc_amd.plan import opdefs as D
from s2lc_amd.plan import vit_plan as V
from tests import plan_harness as H
from tests.helpers import mae_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


# ---- images ------------------------------------------------------------------------------------------------------------------------
def _download(bases, names=H.MUTABLE) -> dict:
    """{base id: flat uint8 CPU copy} of the named bases of a _lib.Bases"""
    torch.cuda.synchronize()
    return {D.BASE[n]: bases.keep[n].contiguous().reshape(-1).view(torch.uint8).cpu() for n in names if bases.keep.get(n) is not None}


def _second_copy(bases):
    """the same bases with every writable buffer cloned: the profiled pass executes the stages again"""
    from s2lc_amd import _lib

    b2 = _lib.Bases()
    for n, t in bases.keep.items():
        if t is not None:
            b2.set(n, t.clone() if n in H.MUTABLE else t)
    return b2


def _adopt(emu: dict, image: dict, refs=None) -> None:
    """the emulator continues from the GPU's state: `image` replaces the writable bases (refs: widened first)"""
    src = H.widen(image, refs) if refs is not None else image
    for b, img in src.items():
        n = min(img.numel(), emu[b].numel())
        emu[b][:n].copy_(img[:n])


def _families(prog, packed, bases, what):
    """every CONV / WGRAD / CHAN_LN_FWD / MAE_LOSS_* record ran the kernel family the restated launchers predict"""
    from s2lc_amd import _lib

    _, var = _lib.profile_variants(packed, bases, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n_split = 0
    for i, (kind, f) in enumerate(prog.ops):
        want = H.predicted_family(kind, f)
        if want is not None:
            assert int(var[i]) == want[0], f"{what} #{i} {kind}: ran family {int(var[i])}, the restated launcher predicts {want}"
        n_split += bool(int(f.get("_flags", 0)) & D.FLAG_SPLIT)
    return n_split


def _report(rep, what, record_property, grads=None):
    for kind, (e32, e64, bar, E) in sorted(rep.worst.items()):
        print(f"{what} {kind}: worst {e32:.2e} (f32 emulator) {e64 if e64 is None else format(e64, '.2e')} (float64), "
              f"bar {bar:.1e}, E {E if E is None else format(E, '.1e')}")
    record_property(what, {k: [float(v[0]), None if v[1] is None else float(v[1]), float(v[2])] for k, v in rep.worst.items()})
    if grads:
        name, (e32, e64, bar) = max(grads.items(), key=lambda kv: max(kv[1][0], kv[1][1] or 0.0))
        print(f"{what} gradients: worst {name} {e32:.2e} (f32 emulator) {e64 if e64 is None else format(e64, '.2e')} (float64), bar {bar:.1e}")
        record_property(what + " grads", [name, float(e32), None if e64 is None else float(e64), float(bar)])
    rep.check(what)


def _run_programs(plan, eng, bases, emu32, emu64, set_dout, what, record_property, nonfinite_fwd=(), exact_zero=()):
    """A: forward from the poisoned workspace, then the backward from the GPU's forward state, each against both emulators."""
    from s2lc_amd import _lib

    refs = H.typed_refs(plan)
    blob = plan.const_table
    st = torch.cuda.current_stream().cuda_stream
    before = _download(bases)
    prof = _second_copy(bases)
    _lib.run(eng.fwd, bases, st)
    gpu = _download(bases, H.MUTABLE + ("PARAMS",))
    H.emulate(eng.fwd, emu32, False)
    H.emulate(eng.fwd, emu64, True)
    rep = H.compare_written(plan.fwd, blob, gpu, emu32, emu64, before=before, whole=True)
    assert rep.nonfinite == list(nonfinite_fwd), rep.nonfinite
    assert rep.compared >= len(plan.fwd.ops)
    _report(rep, what + " fwd", record_property)
    n_split = _families(plan.fwd, eng.fwd, prof, what + " fwd")
    if plan.bwd is None:
        return n_split
    set_dout(emu32)
    before = _download(bases)
    _adopt(emu32, before)
    _adopt(emu64, before, refs)
    prof = _second_copy(bases)
    _lib.run(eng.bwd, bases, st)
    gpu = _download(bases, H.MUTABLE + ("PARAMS",))
    H.emulate(eng.bwd, emu32, False)
    H.emulate(eng.bwd, emu64, True)
    rep = H.compare_written(plan.bwd, blob, gpu, emu32, emu64, before=before, whole=True)
    assert rep.nonfinite == [], rep.nonfinite
    grads = H.compare_grads(plan, rep, gpu, emu32, emu64, exact_zero=exact_zero)
    _report(rep, what + " bwd", record_property, grads)
    return n_split + _families(plan.bwd, eng.bwd, prof, what + " bwd")


def _engine_buffers(eng, plan, dev, n_params):
    """NaN over the workspace AND over the accumulators an engine reuses from step to step without clearing them (AUX, WGS: a program
    must MEMSET what it accumulates into); zeroed outputs and gradients.  The emulator's bases start the same (poison_accumulators)."""
    eng.ws.view(torch.float32).fill_(NAN)
    eng.aux.view(torch.float32).fill_(NAN)
    eng.wpack.zero_()
    if eng.wgs is not None:
        eng.wgs.fill_(NAN)
    out = torch.zeros(plan.out_bytes + 256, dtype=torch.uint8, device=dev)
    grads = torch.zeros(n_params, dtype=torch.float32, device=dev)
    return out, grads


# ---- A. whole programs of the two modules ----------------------------------------------------------------------------------------
def _whole_setup(name):
    from s2lc_amd.engine import fill_noise
    from s2lc_amd.vit_engine import VitEngine

    c = H.stage_case(name)
    fp, fb = c.module._flat_params.detach().clone(), c.module._flat_bufs.detach().clone()
    dev = torch.device(DEV)
    c.module.to(dev)
    eng = VitEngine(c.module, c.B, c.training, c.ratio, dev, c.want_bwd, c.want_dx)
    plan = eng.plan
    out, grads = _engine_buffers(eng, plan, dev, plan.layout.n_params)
    noise = fill_noise(plan, {"noise": c.noise, "drop_u": c.drop_u}, dev)
    dout = dx = None
    if plan.bwd is not None:
        dout = (torch.zeros(plan.dout_bytes + 256, dtype=torch.uint8, device=dev) if plan.douts
                else torch.zeros(plan.dout_shape, dtype=torch.float32, device=dev))
        dx = torch.zeros_like(c.x, device=dev) if c.want_dx else None
    bases = eng.bases(c.module, c.x.to(dev), out, noise, dout=dout, grads=grads, dx=dx)
    nz = H.stage_noise(c, plan)
    emu32 = H.make_bases_vit(plan, fp, fb, c.x, nz, False)
    emu64 = H.make_bases_vit(plan, fp, fb, c.x, nz, True)
    H.poison_accumulators(emu32)
    H.poison_accumulators(emu64, True)

    def set_dout(e32):
        """MAE: d loss = 1 (no gradient on pred).  Segmentation: d cross_entropy / d logits of the emulated logits, ignore_index 0."""
        g = H.stage_dout(c, plan, e32)
        dout.view(-1).view(torch.float32)[: g.numel()].copy_(g)
        H.fview(emu32, "DOUT")[: g.numel()].copy_(g)
        H.fview(emu64, "DOUT", True)[: g.numel()].copy_(g)

    return c, plan, eng, bases, emu32, emu64, set_dout


@pytest.mark.parametrize("name", list(H.STAGE_CASES))
def test_whole_programs(name, record_property):
    c, plan, eng, bases, emu32, emu64, set_dout = _whole_setup(name)
    assert (plan.bwd is not None) == c.want_bwd and bool(plan.want_dx) == c.want_dx
    # mask ratio 0: nothing is masked, the loss is 0 / 0 - NaN in the emulators and on the GPU alike, everything else finite
    nonfinite = [("MAE_LOSS_FWD", "LOSS")] if c.net == "mae" and c.ratio == 0.0 else []
    n_split = _run_programs(plan, eng, bases, emu32, emu64, set_dout, name, record_property, nonfinite_fwd=nonfinite,
                            exact_zero=("head.net.0.bias",) if c.training else ())
    flagged = sum(bool(int(f.get("_flags", 0)) & D.FLAG_SPLIT) for prog in (plan.fwd, plan.bwd) if prog is not None for _, f in prog.ops)
    assert n_split == flagged and (flagged > 0 if name == "seg_full_b1_split" else True) and (flagged == 0 or c.precision == "f32-split")
    if c.want_dx:
        kinds = [(k, f.get("INVERSE", 0)) for k, f in plan.bwd.ops if k == "PATCHIFY"]
        assert len(kinds) == 2 and all(inv for _, inv in kinds), kinds
    if name == "seg_small_eval_bwd":
        assert any(k == "BN_BWD_APPLY" and f.get("EVAL") for k, f in plan.bwd.ops)


# ---- A. the four method plans -----------------------------------------------------------------------------------------------------
def _method_cases():
    """name -> (plan, inputs, noise, upstream gradients by output name) at the small_bs2 geometry"""
    from tests.test_vit_plan_cpu import _mae_spec

    cfg, sd, x, noise, ratio = mae_inputs("small_bs2")
    B = x.shape[0]
    spec = _mae_spec(cfg)
    layout = V.mae_layout(spec)
    with torch.no_grad():
        lat, mask, ids = P.forward_encoder(sd, cfg, x, ratio, noise)
        pred = P.forward_decoder(sd, cfg, lat, ids)
    rnd = lambda shape, seed: torch.randn(shape, generator=torch.Generator().manual_seed(seed))      # noqa: E731
    xt = rnd((B, cfg.num_patches, 12), 3)
    keep = int(cfg.num_patches * 0.5)
    spec_np = _mae_spec(cfg)
    spec_np.norm_pix_loss = True
    return sd, layout, {
        "encoder": (V.plan_mae_encoder(spec, B, ratio, True, layout), {"x": x}, {"noise": noise}, {"latent": rnd(lat.shape, 1)}),
        "encoder_dx": (V.plan_mae_encoder(spec, B, ratio, True, layout, want_dx=True), {"x": x}, {"noise": noise}, {"latent": rnd(lat.shape, 1)}),
        "decoder": (V.plan_mae_decoder(spec, B, lat.shape[1], True, layout), {"x": lat, "ids_restore": ids}, {}, {"pred": rnd(pred.shape, 2)}),
        "loss": (V.plan_mae_loss(spec, B, True, layout), {"imgs": x, "pred": pred, "mask": mask}, {}, {"loss": torch.ones(1)}),
        "loss_norm_pix": (V.plan_mae_loss(spec_np, B, True, layout), {"imgs": x, "pred": pred, "mask": mask}, {}, {"loss": torch.ones(1)}),
        "random_masking": (V.plan_random_masking(spec, B, cfg.num_patches, 12, 0.5, True, layout), {"x": xt}, {"noise": noise},
                           {"x_masked": rnd((B, keep, 12), 4)}),
    }


@pytest.mark.parametrize("name", ["encoder", "encoder_dx", "decoder", "loss", "loss_norm_pix", "random_masking"])
def test_method_programs(name, record_property):
    """X / DOUT / NOISE packed as vit_engine._MethodFunction packs them; OUT, DX and GRADS against the emulator."""
    from s2lc_amd.engine import _TORCH_DT, _view, fill_noise
    from s2lc_amd.modules.prithvi import MaskedAutoencoderViT
    from s2lc_amd.vit_engine import MethodEngine
    from tests.helpers import PRITHVI_SMALL

    sd, layout, cases = _method_cases()
    plan, inputs, noise, gouts = cases[name]
    module = MaskedAutoencoderViT(**PRITHVI_SMALL)
    module.load_state_dict(sd)
    fp, fb = module._flat_params.detach().clone(), module._flat_bufs.detach().clone()
    dev = torch.device(DEV)
    module.to(dev)
    eng = MethodEngine(plan, dev)
    out, grads = _engine_buffers(eng, plan, dev, layout.n_params)
    xbuf = torch.zeros(plan.x_bytes + 256, dtype=torch.uint8, device=dev)
    for n, t in inputs.items():
        ref = plan.inputs[n]
        _view(xbuf, ref).copy_(t.to(device=dev, dtype=_TORCH_DT[ref.dtype]).reshape(ref.shape))
    dout = torch.zeros(plan.dout_bytes + 256, dtype=torch.uint8, device=dev)
    dx = torch.zeros(plan.dx_bytes + 256, dtype=torch.uint8, device=dev)
    bases = eng.bases(module, xbuf, out, fill_noise(plan, noise, dev), dout=dout, grads=grads, dx=dx)
    emu32, m32 = H.method_bases(plan, fp, fb, inputs, noise, False)
    emu64, m64 = H.method_bases(plan, fp, fb, inputs, noise, True)
    H.poison_accumulators(emu32)
    H.poison_accumulators(emu64, True)

    def set_dout(_):
        for n, g in gouts.items():
            ref = plan.douts[n]
            _view(dout, ref).copy_(g.to(dev).reshape(ref.shape))
            m32.view(ref.ref, ref.shape).copy_(g.reshape(ref.shape))
            m64.view(ref.ref, ref.shape).copy_(g.reshape(ref.shape))

    _run_programs(plan, eng, bases, emu32, emu64, set_dout, "method " + name, record_property)
    written = H.written_ranges(plan.bwd, plan.const_table)
    for t in plan.dins.values():        # every planned input gradient is written whole
        iv = written[D.BASE["DX"]]
        assert bool(((iv[:, 0] <= t.off) & (iv[:, 1] >= t.off + t.nbytes)).any()), t


# ---- B. one record at a time --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mae_small_bs2_norm_pix", "seg_small_train_unfrozen"])
def test_one_record_at_a_time(name, record_property):
    from s2lc_amd import _lib

    c, plan, eng, bases, emu32, emu64, set_dout = _whole_setup(name)
    refs, blob = H.typed_refs(plan), plan.const_table
    st = torch.cuda.current_stream().cuda_stream
    fixed = [b for b in emu32 if D.BASES[b] not in H.MUTABLE]
    cur = _download(bases)
    for prog, packed, what in ((plan.fwd, eng.fwd, "fwd"), (plan.bwd, eng.bwd, "bwd")):
        assert not any(int(f.get("_flags", 0)) & D.FLAG_CHAIN for _, f in prog.ops)      # no record is bound to its successors
        if what == "bwd":
            _adopt(emu32, cur)
            set_dout(emu32)          # from the logits the forward left (the GPU's: emu32 has just adopted them)
        rep = H.StageReport()
        for i in range(len(prog.ops)):
            _lib.run(packed, bases, st, i, i + 1)
            now = _download(bases, H.MUTABLE + ("PARAMS",))
            # the same single record through both emulators, from the GPU's state before it
            e32 = {b: (emu32[b] if b in fixed else cur[b].clone()) for b in emu32 if b in fixed or b in cur}
            e64 = {b: emu64[b] for b in fixed}
            e64.update(H.widen(cur, refs))
            ops_ref.run_program(packed[i:i + 1], e32, D, narrow_bases=H.NARROW)
            ops_ref.run_program(packed[i:i + 1], e64, D, wide=True, narrow_bases=H.NARROW)
            H.compare_written(prog, blob, now, e32, e64, before=cur, whole=False, begin=i, end=i + 1, rep=rep)
            cur = {b: now[b] for b in cur}
        assert rep.nonfinite == [], rep.nonfinite
        _report(rep, f"{name} {what} per record", record_property)
