"""The one place a libthzdoe entry point is called from Python.

``call`` runs an entry on a device's current stream, ``workspace`` allocates what a ``*_workspace_size``
entry asks for, ``_launch`` is the two together for the entries that take (workspace, bytes) last.
Every module of the package goes through these; host-only queries that launch nothing
(thz_asm_band, thz_abi_version, the timing entries of _lib) call the library directly.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def _require_device(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the MI355X path needs a ROCm device tensor (got device {t.device}); "
                           "this framework has no CPU compute path")


def _stream_handle():
    """torch.cuda.current_stream().cuda_stream of the current device, read without building the Stream object
    (about a microsecond of every eager call; torch's own generated code reads the handle the same way)."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _fptr(arr):
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_float))


def convert(args, _tensor=torch.Tensor, _struct=ctypes.Structure, _ptr=ctypes.c_void_p, _ref=ctypes.byref):
    """The arguments as ctypes takes them: a tensor is its data pointer, a descriptor (ctypes.Structure) goes
    by reference, and anything else is unchanged: ints, floats, a byref'd object, a ctypes array, and None --
    which ctypes passes as NULL for every pointer type, c_void_p and POINTER(desc) alike.  One expression per
    argument and no call of our own: this runs on every eager launch."""
    return [_ptr(a.data_ptr()) if isinstance(a, _tensor) else _ref(a) if isinstance(a, _struct) else a for a in args]


def call(fn, *args, device):
    """fn(*args, stream) on ``device``'s current stream, the arguments converted by ``convert``; a status
    other than THZ_OK raises ThzError."""
    with torch.cuda.device(device):
        _lib.check(fn(*convert(args), _stream_handle()))


def workspace(size_fn, *size_args, device):
    """The uint8 device tensor size_fn(*size_args, &bytes) asks for, at least one byte so that its pointer is
    never NULL (no entry is reached with a zero size, and every entry takes (ptr, 1) where
    it would take (NULL, 0)).  A failing size call raises ThzError before the device is touched."""
    nbytes = ctypes.c_size_t(0)
    _lib.check(size_fn(*convert(size_args), ctypes.byref(nbytes)))
    return torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=device)


def _launch(size_fn, run_fn, d, device, *args):
    """One call of a workspace-taking entry point on ``device``'s current stream:
    run_fn(&d, *args, workspace, bytes, stream) with the workspace size_fn(&d) asks for."""
    ws = workspace(size_fn, d, device=device)
    call(run_fn, d, *args, ws, ws.numel(), device=device)


def loss_stats(ld, device):
    """The float32 statistics buffer of the intensity-MSE entries for the LossDesc ``ld``:
    thz_intensity_mse_workspace_size is the one size entry that returns its size (0 for a descriptor the
    entries refuse), and the buffer is saved for the backward, so it is sized exactly."""
    nbytes = _lib.lib().thz_intensity_mse_workspace_size(ctypes.byref(ld))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)
