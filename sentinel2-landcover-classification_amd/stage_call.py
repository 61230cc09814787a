"""One standalone stage call: the records, the tensors they refer to and the launch, tied together.

    call = StageCall()
    call.add("ARGMAX", LOGITS=call.t(logits, (B, C, HW)), MASK=call.t(mask, (B, HW)), B=B, C=C, HW=HW)
    call.run()

`t` binds a tensor to the next free base slot and returns the `TRef` that names it, with the tensor's own dtype and (unless a reshaped
one is given) shape - the kernels only ever see `bases[slot] + offset`, so any slot serves and no name out of `opdefs.BASES` is needed.
`const` / `scratch` lay small host tables and zeroed results out in one upload and one device allocation.  A call is built (`t`,
`const`, `scratch`, `add`), then packed (`pack`, or the first `run` / `view`); a packed call only swaps tensors (`rebind`) and runs,
which is what `cached` does for the wrappers that launch every step.  Everything up to `pack()` works on CPU tensors (tests interpret
the packed records with oracle/ops_ref.py); only `run()` needs the GPU and the built library.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .plan import opdefs as D
from .plan.program import ALIGN, ITEMSIZE, Program, TRef

_TORCH = {"f32": torch.float32, "f64": torch.float64, "i64": torch.int64, "i32": torch.int32, "i16": torch.int16, "u8": torch.uint8,
          "bf16": torch.bfloat16}
_NAME = {v: k for k, v in _TORCH.items()}


class StageCall:
    def __init__(self):
        self.prog, self.bases, self.packed = Program(), _lib.Bases(), None
        self.tensors = []          # slot -> tensor: kept alive across the launch
        self.device = None         # of the first bound tensor; every other one must match
        self.per_use = ()          # slots whose tensors `run()` lets go of after the launch (`cached`)
        self._slots = {}           # id(tensor) -> slot, while the call is built: a packed call takes no further tensor
        self._need = []            # slot -> (torch dtype, bytes) of the tensor first bound: what `rebind` asks of another one
        self._arena = {}           # "const" / "scratch" -> [slot, top]: their tensors exist from pack() on
        self._parts = []           # (offset, bytes) of the constants

    # ---- tensors ---------------------------------------------------------------------------------------------------------------
    def _check(self, tensor) -> None:
        """contiguous and on the call's device: decided before any data_ptr()"""
        if not tensor.is_contiguous():
            raise ValueError("a stage operand must be contiguous")
        if self.device is None:
            self.device = tensor.device
            if tensor.is_cuda:
                self.bases.device = tensor.device      # made current around the launch (_lib.run)
        elif tensor.device != self.device:
            raise ValueError(f"stage operands on different devices: {tensor.device} and {self.device}")

    def _building(self) -> None:
        if self.packed is not None:
            raise RuntimeError("the call is packed: records, tensors, constants and scratch come before")

    def _new_slot(self, need=None) -> int:
        self._building()
        if len(self.tensors) == len(D.BASES):
            raise ValueError(f"a stage call binds at most {len(D.BASES)} tensors")
        self.tensors.append(None)
        self._need.append(need)
        return len(self.tensors) - 1

    def t(self, tensor, shape=None, dtype: str | None = None, byte_off: int = 0) -> TRef | None:
        """The ref of `tensor` (None: the NULL operand) at its own data_ptr(): the same tensor object always gets the same slot.
        `shape` defaults to the tensor's; a uint8 tensor may be read as `dtype` from `byte_off` on."""
        if tensor is None:
            return None
        self._check(tensor)
        own = _NAME.get(tensor.dtype)
        if own is None:
            raise ValueError(f"no stage operand has the dtype {tensor.dtype}")
        if shape is None and dtype is None and not byte_off:
            shape, dtype = tuple(tensor.shape), own
        else:
            shape, dtype = tuple(tensor.shape if shape is None else shape), own if dtype is None else dtype
            if dtype not in ITEMSIZE or (dtype != own and own != "u8"):               # a uint8 tensor is raw bytes of any dtype
                raise ValueError(f"no stage operand of dtype {dtype} from a {tensor.dtype} tensor")
            if byte_off < 0 or byte_off % ITEMSIZE[dtype] or byte_off + math.prod(shape) * ITEMSIZE[dtype] > tensor.nbytes:
                raise ValueError(f"{dtype} {shape} at byte {byte_off} does not fit a tensor of {tensor.nbytes} bytes")
        slot = self._slots.get(id(tensor))
        if slot is None:
            slot = self._slots[id(tensor)] = self._new_slot((tensor.dtype, tensor.nbytes))
            self.tensors[slot] = tensor
            self.bases.arr[slot] = tensor.data_ptr()
        return TRef(slot, byte_off, shape, dtype)

    def rebind(self, ref: TRef | int, tensor) -> None:
        """Another tensor behind a slot (or behind `ref`'s) of the packed call - the dtype of the first one, at least as many bytes -
        without repacking."""
        slot = ref if isinstance(ref, int) else ref.base
        if tensor is self.tensors[slot]:
            return
        self._check(tensor)
        dtype, nbytes = self._need[slot]
        if self.packed is None or tensor.dtype != dtype or tensor.nbytes < nbytes:
            raise ValueError(f"rebind needs a packed call and a {dtype} tensor of at least {nbytes} bytes")
        self.tensors[slot] = tensor
        self.bases.arr[slot] = tensor.data_ptr()

    # ---- packed constants and zeroed scratch -----------------------------------------------------------------------------------
    def _alloc(self, arena: str, shape, dtype: str) -> TRef:
        self._building()
        a = self._arena.get(arena)
        if a is None:
            a = self._arena[arena] = [self._new_slot(), 0]
        ref = TRef(a[0], a[1], tuple(int(s) for s in shape), dtype)
        a[1] += (ref.nbytes + ALIGN - 1) // ALIGN * ALIGN
        return ref

    def const(self, values, dtype: str, shape=None) -> TRef:
        """Host data for the one byte image that `pack()` uploads, on an ALIGN boundary."""
        data = torch.as_tensor(values, dtype=_TORCH[dtype]).contiguous()
        if shape is not None and int(np.prod(shape)) != data.numel():
            raise ValueError(f"{data.numel()} values for a constant of shape {tuple(shape)}")
        ref = self._alloc("const", data.shape if shape is None else shape, dtype)
        self._parts.append((ref.off, data.reshape(-1).view(torch.uint8)))
        return ref

    def scratch(self, shape, dtype: str) -> TRef:
        """Room in the one zeroed device allocation that `pack()` makes, on an ALIGN boundary."""
        return self._alloc("scratch", shape, dtype)

    def image(self) -> torch.Tensor:
        """The constants as one uint8 host tensor (at least ALIGN bytes)."""
        img = torch.zeros(max(self._arena.get("const", (0, 0))[1], ALIGN), dtype=torch.uint8)
        for off, b in self._parts:
            img[off:off + b.numel()] = b
        return img

    def view(self, ref: TRef) -> torch.Tensor:
        """What `ref` names inside the (packed) constants or scratch, as a tensor of its shape and dtype."""
        self.pack()
        return self.tensors[ref.base][ref.off:ref.off + ref.nbytes].view(_TORCH[ref.dtype]).view(ref.shape)

    # ---- records and launch ----------------------------------------------------------------------------------------------------
    def add(self, kind: str, **fields) -> None:
        self._building()
        self.prog.add(kind, **fields)

    def pack(self) -> np.ndarray:
        """The packed records; the first call uploads the constants and zeroes the scratch on the bound tensors' device."""
        if self.packed is None:
            for arena, (slot, top) in self._arena.items():
                self.tensors[slot] = self.image().to(self.device) if arena == "const" else \
                    torch.zeros(max(top, ALIGN), dtype=torch.uint8, device=self.device)
                self.bases.arr[slot] = self.tensors[slot].data_ptr()
            self.packed = self.prog.pack()
        return self.packed

    def run(self, stream: int | None = None) -> None:
        """Launch the records on `stream` (default: the current stream of the bound tensors' device), that device current."""
        packed = self.packed if self.packed is not None else self.pack()
        try:
            if self.bases.device is None:
                raise RuntimeError("standalone stages run on the GPU (there is no CPU fallback)")
            _lib.run(packed, self.bases, torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream)
        finally:
            for slot in self.per_use:
                self.tensors[slot] = None


def cached(cache: dict, build, *tensors, **scalars) -> StageCall:
    """The packed call `build(*tensors, **scalars)`, built once per device, tensor shapes and scalars and kept in `cache`; every later
    use only puts its own tensors behind the slots the first ones took (`rebind`: no record is rebuilt or repacked) and `run()` lets go
    of them again, so the cache keeps none of them alive.  For wrappers that run every step.  A cached call is one object: not for
    threads that launch the same stage on the same device at the same time."""
    key = (build, tensors[0].device, tuple([None if t is None else t.shape for t in tensors]), tuple(scalars.values()))
    hit = cache.get(key)
    if hit is None:
        call = build(*tensors, **scalars)
        call.pack()
        slots = [None if t is None else call._slots.get(id(t)) for t in tensors]
        bound = [s for s in slots if s is not None]
        if len(set(bound)) == len(bound):          # one tensor given twice shares a slot: that call serves this use only
            call.per_use = tuple(bound)
            cache[key] = call, slots
        return call
    call, slots = hit
    for slot, tensor in zip(slots, tensors):
        if slot is not None:
            call.rebind(slot, tensor)
    return call
