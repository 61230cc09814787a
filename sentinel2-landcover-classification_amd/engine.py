"""Runtime glue: owns the device buffers of a planned network and runs its stage programs.

PyTorch supplies device memory, the current HIP stream and the autograd *edge* (one
`autograd.Function` for the whole network: forward = one `s2k_program_run`, backward = one more).
The reference's equivalent is `self.net(x)` + `loss.backward()` in
/root/reference/src/train_segmentation.py:129-147 dispatching ~1,000 ATen ops per step.

One of each, for every model family and both entry points (eager autograd nodes; the torch.compile custom ops of compile_ops.py):
`Engine` (buffers + packed programs; `UnetEngine` here, `VitEngine` / `MethodEngine` in vit_engine.py only say how their plan is
made), `preflight`, `fill_noise`, `run_backward` (how a backward meets the data-parallel reducer) and `backward_into_grads` (the
gradient target around it).  The U-Net's step is `unet_prepare` + `Engine.run_forward` + `unet_backward_raw`, as the ViTs' is
`vit_engine.vit_prepare` / `vit_backward_raw`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


class Workspace:
    """The per-forward device state of a planned network: activation arena + statistics accumulators.  A training
    forward LEASES one until its backward has run (or its autograd node dies), so fwd, fwd, bwd, bwd — two micro-batches,
    two losses, a logging forward between forward and backward — never overwrite each other's saved activations."""

    def __init__(self, ws_bytes: int, aux_bytes: int, device: torch.device):
        pad = 256
        self.ws = torch.empty(ws_bytes + pad, dtype=torch.uint8, device=device)
        self.aux = torch.zeros(max(aux_bytes, 8) + pad, dtype=torch.uint8, device=device)


class WorkspaceLease:
    """Returns the workspace to its engine's pool when released or garbage-collected with the autograd node."""

    def __init__(self, pool: list, space: Workspace):
        self.pool, self.space = pool, space

    def release(self) -> None:
        if self.space is not None:
            self.pool.append(self.space)
            self.space = None

    def __del__(self):
        self.release()


class WorkspacePool:
    def __init__(self, ws_bytes: int, aux_bytes: int, device: torch.device):
        self.args = (ws_bytes, aux_bytes, device)
        self.free: list[Workspace] = [Workspace(*self.args)]
        self.allocated = 1

    def lease(self) -> WorkspaceLease:
        if not self.free:       # an earlier forward still owns the last one (its backward is outstanding)
            self.free.append(Workspace(*self.args))
            self.allocated += 1
        return WorkspaceLease(self.free, self.free.pop())

    def peek(self) -> Workspace:
        if not self.free:
            self.free.append(Workspace(*self.args))
            self.allocated += 1
        return self.free[-1]


_TORCH_DT = {"f32": torch.float32, "i64": torch.int64, "i32": torch.int32}


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _view(buf: torch.Tensor, t) -> torch.Tensor:
    """The tensor a TRef names inside a packed byte buffer (OUT / X / DOUT / DX)."""
    return buf[t.off:t.off + t.nbytes].view(_TORCH_DT[t.dtype]).view(t.shape)


class Engine:
    """Buffers + packed programs of one planned network for one cache key of one module.  The subclasses only say how their
    plan is made and keep what is particular to their family."""

    def __init__(self, plan, device: torch.device):
        self.plan = plan
        self.fwd = plan.fwd.pack()
        self.bwd = plan.bwd.pack() if plan.bwd is not None else None
        self.device = device
        self.spaces = WorkspacePool(plan.ws_bytes, plan.aux_bytes, device)
        self.const = torch.tensor(plan.const_table if plan.const_table else [0] * 8, dtype=torch.int32, device=device)
        self.wpack = torch.zeros(plan.wpack_bytes // 4 + 65536, dtype=torch.float32, device=device)  # + slack: A-tile loads may overrun
        self.wgs = torch.empty(plan.layout.n_params, dtype=torch.float32, device=device) if plan.bwd is not None else None
        self.bwd_marks = plan.bwd_param_marks
        self.want_dx = getattr(plan, "want_dx", False)     # the backward program also writes the input's gradient into DX

    @property
    def resident(self) -> Workspace:
        """The workspace a fresh forward would take (tests / profilers that drive the programs by hand)."""
        return self.spaces.peek()

    @property
    def ws(self) -> torch.Tensor:
        return self.resident.ws

    @property
    def aux(self) -> torch.Tensor:
        return self.resident.aux

    def bases(self, module, x, out, noise=None, dout=None, grads=None, space: Workspace | None = None, dx=None,
              dout_need: int | None = None) -> _lib.Bases:
        space = space or self.resident
        b = _lib.Bases()
        b.set("WS", space.ws).set("AUX", space.aux).set("CONST", self.const).set("WPACK", self.wpack)
        b.set("PARAMS", module._flat_params).set("BUFS", module._flat_bufs)
        b.set("X", x).set("OUT", out)
        if self.wgs is not None:
            b.set("WGS", self.wgs)
        if dout is not None:
            plan, need = self.plan, dout_need     # dout_need: the stages reading the rest of the packed buffer are skipped by the caller
            if need is None:
                need = getattr(plan, "dout_bytes", 0) or 4 * int(torch.Size(getattr(plan, "dout_shape", None) or plan.logits_shape).numel())
            if dout.numel() * dout.element_size() < need:      # the backward program reads DOUT unchecked on the device
                raise ValueError(f"DOUT holds {dout.numel() * dout.element_size()} bytes, the backward program reads {need}")
            b.set("DOUT", dout)
        if noise is not None:
            b.set("NOISE", noise)
        if grads is not None:
            b.set("GRADS", grads)
        if dx is not None:
            b.set("DX", dx)
        return b

    def views(self, out: torch.Tensor) -> dict:
        return {name: _view(out, t) for name, t in self.plan.outputs.items()}

    def run_forward(self, module, x, out, noise) -> WorkspaceLease:
        """Enqueue the forward program on a leased workspace; the caller keeps the lease until the backward has run, or releases
        it at once (stream-ordered: the next forward that takes this workspace is enqueued behind this one)."""
        lease = self.spaces.lease()
        _lib.run(self.fwd, self.bases(module, x, out, noise, space=lease.space), _stream(x.device))
        return lease


class UnetEngine(Engine):
    """One (B, H, W, training) shape of an EfficientnetUnet."""

    def __init__(self, module, B: int, H: int, W: int, training: bool, device: torch.device, want_bwd: bool | None = None,
                 want_dx: bool = False):
        super().__init__(module._make_plan(B, H, W, training, want_bwd, want_dx), device)
        self.want_dx, self.B, self.n_noise_rows = want_dx, B, self.plan.n_noise_rows


def _engine(module, x: torch.Tensor, training: bool, want_bwd: bool, want_dx: bool = False) -> UnetEngine:
    key = (tuple(x.shape), training, want_bwd, want_dx, x.device)
    eng = module._engines.get(key)
    if eng is None:
        B, _, H, W = x.shape
        eng = UnetEngine(module, B, H, W, training, x.device, want_bwd, want_dx)
        module._engines[key] = eng
    return eng


def preflight(module, x) -> None:
    """What every whole-network forward checks before it plans or launches anything."""
    if not x.is_cuda:
        raise RuntimeError(f"{type(module).__name__} runs on the HIP engine only: move the module and the input to the GPU "
                           "(there is no CPU fallback; the CPU restatement lives under oracle/ for tests)")
    _lib.lib()
    if x.dtype != torch.float32:
        raise TypeError("the parity path computes in fp32; got " + str(x.dtype))
    if module._flat_params.device != x.device:
        raise RuntimeError("module and input are on different devices")


def fill_noise(plan, injected: dict | None, device) -> torch.Tensor:
    """The NOISE buffer of a plan: fresh uniforms, or the tensors injected by name (parity tests)."""
    noise = torch.empty(max(plan.noise_bytes // 4, 1), dtype=torch.float32, device=device)
    for name, t in plan.noise.items():
        n = int(np.prod(t.shape))
        dst = noise[t.off // 4:t.off // 4 + n]
        src = (injected or {}).get(name)
        if src is None:
            dst.uniform_(0.0, 1.0)     # torch.rand semantics: U[0, 1)
        else:
            if tuple(src.shape) != tuple(t.shape):
                raise ValueError(f"{name} must have shape {tuple(t.shape)}, got {tuple(src.shape)}")
            dst.copy_(src.to(device=device, dtype=torch.float32).reshape(-1))
    return noise


class _UnetFunction(torch.autograd.Function):
    """Whole-network autograd node.  Parameter gradients are written straight into the module's
    flat gradient buffer by the backward program (never returned through autograd: 900+
    per-tensor accumulations would cost more host time than the GPU step)."""

    @staticmethod
    def forward(ctx, x, anchor, module, eng, noise):
        out = torch.empty(eng.plan.logits_shape, dtype=torch.float32, device=x.device)
        ctx.module, ctx.eng, ctx.noise, ctx.lease = module, eng, noise, eng.run_forward(module, x, out, noise)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        return unet_backward_raw(ctx.module, ctx.eng, ctx.lease, ctx.noise, x, dout), None, None, None, None


def unet_backward_raw(module, eng, lease, noise, x, dout):
    """The backward program of a UnetEngine forward.  Parameter gradients go into the module's flat gradient buffer; returns dX
    or None.  Shared by the autograd node above and the torch.compile custom op (compile_ops.py)."""
    if lease.space is None:
        raise RuntimeError("backward through the same forward a second time: the saved activations have been released "
                           "(the s2k engine keeps them for one backward, like autograd without retain_graph)")
    dout = dout.contiguous()
    scale = getattr(module, "_grad_scale", 1.0)
    if scale != 1.0:
        dout = dout * scale   # data-parallel mean folded into the upstream gradient
    return backward_into_grads(module, eng, lease, x, None, noise, dout, scale)


def backward_into_grads(module, eng, lease, x, out, noise, dout, scale: float, skip=(), dout_need: int | None = None):
    """A whole-network backward program and its gradient target (the U-Net's and the ViTs').  Gradients that are live (a second
    backward before zero_grad) are accumulated: the program writes the scratch buffer, which is then added to the flat gradient
    buffer; otherwise the program overwrites the flat buffer, and parameters that had no `.grad` yet get theirs published.
    `skip`: sorted stage ranges [s0, s1) left out of the program.  Returns dX (planned only when x.requires_grad) or None."""
    live = module._grads_live()
    accumulate = live and not getattr(module, "_overwrite_next", False)
    module._overwrite_next = False
    grads = module._grad_scratch() if accumulate else module._grad_buffer()
    grads.zero_()
    dx = torch.empty_like(x) if eng.want_dx else None
    bases = eng.bases(module, x, out, noise, dout=dout, grads=grads, space=lease.space, dx=dx, dout_need=dout_need)
    st = _stream(x.device)

    def run_range(a, b):        # stages [a, b) of the backward program minus the skipped ranges
        for (s0, s1) in skip:
            if a < s1 and s0 < b:
                if a < s0:
                    _lib.run(eng.bwd, bases, st, a, s0)
                a = max(a, s1)
        if a < b:
            _lib.run(eng.bwd, bases, st, a, b)

    with torch.cuda.device(x.device):
        run_backward(module, eng.bwd_marks, len(eng.bwd), run_range, grads, accumulate, lo_min=getattr(eng.plan, "trainable_lo", 0))
    lease.release()     # stream-ordered: the next forward that takes this workspace is enqueued behind this backward
    if accumulate:
        module._grad_buffer().add_(grads)
    if not live:
        module._publish_grads(module._no_grad_params)
    if dx is not None and scale != 1.0:
        # the 1/world of the data-parallel mean belongs to the PARAMETER gradients only: whatever sits in front of the
        # module (an input adapter under its own DDP, a saliency map) must see d loss_rank / d x, as with torch DDP
        dx.mul_(1.0 / scale)
    return dx


def _note_bucket_reduction(module) -> None:
    """Bookkeeping for ddp.FlatGradReducer: this backward hands its gradients to the bucket hook segment by segment.  The
    separately callable methods (vit_engine._MethodFunction) instead ADD local gradients to the flat buffer and leave the
    reduction to FlatGradReducer.finish(); both in one backward would reduce the bucketed part twice."""
    if getattr(module, "_method_grads_unreduced", False):
        raise RuntimeError("one backward mixes the fused forward with separately called methods under a data-parallel reducer: "
                           "call ddp.finish() between them, or use one of the two paths per step")
    module._bucket_reduced = True


def run_backward(module, marks, n_ops: int, run_range, grads: torch.Tensor, accumulate: bool, lo_min: int = 0) -> None:
    """Enqueue a whole-network backward program, with or without the data-parallel reducer (shared by the eager autograd nodes of
    engine.py / vit_engine.py and the torch.compile custom ops, so their checks cannot drift apart).

      no reducer, or inside `FlatGradReducer.no_sync()`   the program runs in one go; under no_sync the module is marked: its flat
                                                          buffer holds LOCAL gradients that a later backward / finish() reduces
      reducer, fresh gradients                            segment by segment, each final suffix bucket handed to the hook
      reducer, accumulating onto live gradients           (gradient accumulation: the last micro-batch of a no_sync sequence) the
                                                          program runs in one go into the scratch buffer, the caller adds it to the
                                                          flat buffer, and finish() reduces the SUM in one collective - torch DDP's
                                                          semantics: one reduction of the accumulated gradients per optimiser step
    `run_range(a, b)` enqueues stages [a, b); `marks` = (a, b, lo, hi) backward segments (plan.bwd_param_marks)."""
    hook = getattr(module, "_bwd_segment_hook", None)
    if hook is None or getattr(module, "_no_sync", False):
        if hook is not None:
            module._method_grads_unreduced = True      # local gradients: reduced as a whole by finish()
        run_range(0, n_ops)
        return
    if accumulate or getattr(module, "_method_grads_unreduced", False):
        if getattr(module, "_bucket_reduced", False):
            raise RuntimeError("a second backward accumulates onto gradients that were already all-reduced bucket by bucket in this "
                               "step: run every micro-batch but the last inside `with reducer.no_sync():` (as with torch DDP)")
        module._method_grads_unreduced = True
        run_range(0, n_ops)
        return
    _note_bucket_reduction(module)
    for (a, b, lo, hi) in marks:
        run_range(a, b)
        hook(max(lo, lo_min), hi, grads)


def unet_prepare(module, x: torch.Tensor, want_bwd: bool, want_dx: bool):
    """(engine, drop-connect noise or None) for one forward of the U-Net on a contiguous `x` (shared by run_unet and the
    torch.compile custom op).  train() plans always carry the backward program; eval() plans only when autograd wants one (torch
    differentiates an eval-mode module just the same: BatchNorm on its running statistics, no drop-connect)."""
    preflight(module, x)
    training = module.training
    eng = _engine(module, x, training, training or want_bwd, want_dx)
    noise = None
    if training:
        noise = module.drop_connect_noise
        if noise is None:
            noise = torch.rand(eng.n_noise_rows, x.shape[0], device=x.device, dtype=torch.float32)
        else:
            if tuple(noise.shape) != (eng.n_noise_rows, x.shape[0]):      # the device program reads NOISE unchecked
                raise ValueError(f"drop_connect_noise must be [{eng.n_noise_rows}, {x.shape[0]}]")
            noise = noise.to(device=x.device, dtype=torch.float32).contiguous()
        module._flat_nbt += 1  # every BatchNorm's num_batches_tracked (one fused add over the flat view)
    return eng, noise


def run_unet(module, x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    want_dx = torch.is_grad_enabled() and x.requires_grad
    differentiate = torch.is_grad_enabled() and (want_dx or any(p.requires_grad for p in module.parameters()))
    eng, noise = unet_prepare(module, x, differentiate, want_dx)
    if differentiate:
        return _UnetFunction.apply(x, module._anchor(x.device), module, eng, noise)
    out = torch.empty(eng.plan.logits_shape, dtype=torch.float32, device=x.device)
    eng.run_forward(module, x, out, noise).release()
    return out
