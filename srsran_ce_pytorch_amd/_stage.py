"""What the stage wrappers behind the channel estimate (dmrs, equalizer, demod, ratematch) share: the mapping of the
library's error codes to exceptions, the lazily created device plan, and the argument checks they have in common."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib


def raise_for(code: int, assertions=()):
    """Raise what the library's error `code` stands for, with its ``ce_last_error()`` text; an invalid-argument text
    listed in `assertions` is an ``AssertionError`` (the estimator: what the reference asserts)."""
    msg = _lib.last_error()
    if code == _lib.CE_ERR_INVALID:
        raise (AssertionError if msg in assertions else ValueError)(msg)
    if code == _lib.CE_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(f"libce_hip: {msg} (code {code})")


def derive_host(entry: str, desc, view):
    """Fill `view` through the host-only ``ce_*_derive_host`` entry point `entry`; works without a GPU."""
    rc = getattr(_lib.load(), entry)(C.byref(desc), C.byref(view))
    if rc != 0:
        raise_for(rc)
    return view


def check_dense(name: str, t, dtype, shape, dev, dtype_name=None):
    """`t` is a dense `dtype` tensor of `shape` on `dev` (an ``out=`` or a kept buffer), or ``ValueError``."""
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()
            or t.device != dev):
        raise ValueError(f"{name} must be a dense {dtype_name or dtype} tensor of shape {shape} on {dev}")


def check_aligned(*named):
    """Every ``(name, tensor)`` pair (a ``None`` tensor is skipped) starts on 16 bytes, as the kernels' 16-byte accesses need."""
    for name, t in named:
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"{name} must be 16-byte aligned")


def batch_param(name: str, value, B: int, dev, lo: int, hi: int, int_text: str = "an int") -> torch.Tensor:
    """A per-slot parameter -> an int32 tensor of 1 or `B` elements on `dev`: a host int is range-checked against
    `lo`..`hi` and holds for the whole batch, a device tensor is taken as it is."""
    if isinstance(value, torch.Tensor):
        if value.dtype != torch.int32 or value.dim() != 1 or value.shape[0] != B or value.device != dev:
            raise ValueError(f"{name}: a tensor must be int32 of shape [{B}] on {dev}, got {value.dtype} {tuple(value.shape)} on {value.device}")
        if value.stride(0) < 0:
            raise ValueError("negative strides are not supported")
        return value
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name}: expected {int_text} or an int32 device tensor of shape [{B}]")
    if not lo <= int(value) <= hi:
        raise ValueError(f"{name}={int(value)} outside {lo}..{hi}")
    return torch.tensor([int(value)], dtype=torch.int32).to(dev)      # on the current stream, like the launch that reads it


def batch_stride(t: torch.Tensor) -> int:
    """Element stride between slots of a per-slot parameter tensor: 0 where one element holds for the whole batch."""
    return 0 if t.shape[0] == 1 else int(t.stride(0))


class Stage:
    """Validated on construction (no GPU needed); the device plan is created at the first launch.

    A subclass names its entry points (``_CREATE``, ``_DESTROY``, ``_LAUNCH``), the subject of its "runs on a ROCm GPU
    only" message (``_NOUN``) and builds its descriptor for a device index in ``_build_desc()``."""

    _CREATE = _DESTROY = _LAUNCH = _NOUN = ""

    def __init__(self, device=None):
        self._lib = _lib.load()
        self._handle = None
        self._device_arg = device
        self.device: Optional[torch.device] = None

    def _build_desc(self, device_index: int):
        raise NotImplementedError

    def _create(self, device_index: int, handle) -> int:
        """The library's return code of plan creation into `handle`; a stage whose entry point takes no descriptor overrides it."""
        desc = self._build_desc(device_index)                  # (and whatever host memory it points to) alive across the call
        return getattr(self._lib, self._CREATE)(C.byref(desc), C.byref(handle))

    def _plan(self):
        if self._handle is None:
            device = self._device_arg
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise RuntimeError(f"{self._NOUN} runs on a ROCm GPU only (no CPU fallback)")
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            handle = C.c_void_p()
            with torch.cuda.device(device):
                rc = self._create(device.index, handle)
            if rc != 0:
                raise_for(rc)
            self._handle, self.device = handle, device
        return self._handle

    def _launch(self, *args):
        """The stage's launch entry point on the current stream of the plan's device: ``(plan, *args, stream)``."""
        dev = self.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            rc = getattr(self._lib, self._LAUNCH)(self._handle, *args, C.c_void_p(stream))
        if rc != 0:
            raise_for(rc)

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            getattr(self._lib, self._DESTROY)(h)
