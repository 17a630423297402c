"""IFTA / Gerchberg-Saxton designer of a quantised DOE on the fused projection kernels (csrc/thz_ifta.hip).

The classical baseline of every quantisation-aware method and the usual initialiser of gradient training:
iterate between the DOE plane and the target planes, imposing the target amplitude there and the level table
here, with the share of cells snapped to the table growing over the run (stepwise quantisation).  The
reference has no such module.  One iteration is

  1. the height map's transmission times the incident field, fused into ``ASM_prop.propagate_planes``;
  2. ``optics.ifta_target_stats``: the planes' sums against the target, written into the history row;
  3. the amplitude scale: each plane's own (``scale="plane"``) or one for all planes (``"joint"``);
  4. ``optics.ifta_target_project`` in place on the planes;
  5. the Z-summing ASM adjoint back to the DOE plane;
  6. ``optics.ifta_doe_project`` with this iteration's snap fraction ``q``.

Nothing in the loop reads the device, so the whole run is one captured graph replayed per design.
"""
from __future__ import annotations

import torch

from . import _lib, optics
from . import doe as _doe
from . import propagation as _prop
from .DataType.ElectricField import ElectricField
from .Props.ASM_Prop import ASM_prop
from .Props._zx import _z_host

_CAPTURE_MODE = "thread_local"  # as qat.py: other threads' HIP calls do not break the capture


def default_q_schedule(iters):
    """The snap fraction per iteration: a linear ramp from 0 to 1 over the first 80 % of the run, 1 after."""
    ramp = max(1, int(round(0.8 * iters)))
    return [min(1.0, it / (ramp - 1)) if ramp > 1 else 1.0 for it in range(iters)]


class IFTAResult:
    """A finished run: ``height`` [hs, ws] float32, ``idx`` [hs, ws] int64 (the level, -1 where a cell is off
    the table), ``history`` [iters, Z, 6] float64 on the device (``optics.IFTA_STATS`` of every iteration's
    planes before their projection)."""

    def __init__(self, height, idx, history, material, device):
        self.height, self.idx, self.history = height, idx, history
        self._material, self._device = material, device

    def as_element(self, thick=None):
        """The map as a ``FixDOEElement`` with no fabrication tolerance, for the propagators and utils.metrics.
        ``thick=dict(thickness=..., slices=...)`` (and any other ``ThickDOEElement`` keyword): the map as a
        ``ThickDOEElement`` instead, the split-step model of the relief."""
        if thick is not None:
            from .Components.ThickDOE import ThickDOEElement
            return ThickDOEElement(self.height, material=list(self._material), device=self._device, **thick)
        from .Components.QuantizedDOE import FixDOEElement
        return FixDOEElement(self.height, tolerance=0.0, material=list(self._material), device=self._device)


class IFTA:
    """``IFTA(asm, z_list, wavelength, spacing, eps, tand, lut, doe_shape, incident=None, window=None, alpha=1.0,
    beta=1.0, scale="plane")``.

    ``asm``: an ``ASM_prop`` whose output has the field's size (cropped after padding, or unpadded).  ``z_list``: the
    target planes, at most THZ_MAX_Z.  ``lut``: the height table, ascending in [0, h_max), h_max = wavelength /
    (sqrt(eps) - 1); a list or CPU tensor (a device tensor is read back here, which a graph capture refuses).
    ``doe_shape`` = (hs, ws): the field must be a whole number of pixels per cell.  ``incident``: the field on the
    DOE, complex64 [H, W] (or [1, 1, H, W]); None: a unit plane wave.  ``window``: bool [H, W], the signal window of
    the target planes; None: every pixel.  ``alpha``, ``beta``: ``optics.ifta_target_project``.  ``tand`` enters the
    forward model only; the projections fit the phase.  One batch item and one wavelength: the kernels compute in
    complex64.  CZT and RSC propagators are not served."""

    def __init__(self, asm, z_list, wavelength, spacing, eps, tand, lut, doe_shape, incident=None, window=None,
                 alpha=1.0, beta=1.0, scale="plane", seed=0):
        if not isinstance(asm, ASM_prop):
            raise TypeError(f"IFTA: the propagator must be an ASM_prop; got {type(asm).__name__} (CZT and RSC "
                            "designers are not built)")
        if asm.do_padding and not asm.do_unpad_after_pad:
            raise ValueError("IFTA: the ASM_prop must crop its output to the field's H x W "
                             "(do_unpad_after_pad=True): the target planes have the DOE plane's size")
        self.asm = asm
        self.zs = _z_host(z_list)
        if not 1 <= len(self.zs) <= _lib.THZ_MAX_Z:
            raise ValueError(f"IFTA: {len(self.zs)} planes; one call takes 1 .. {_lib.THZ_MAX_Z} (THZ_MAX_Z)")
        if scale not in ("plane", "joint"):
            raise ValueError(f"IFTA: scale must be 'plane' or 'joint'; got {scale!r}")
        self.alpha, self.beta, self.scale = float(alpha), float(beta), scale
        if not 0.0 < self.alpha <= 2.0:
            raise ValueError(f"IFTA: alpha must lie in (0, 2]; got {alpha}")
        if not 0.0 <= self.beta <= 1.0:
            raise ValueError(f"IFTA: beta must lie in [0, 1]; got {beta}")
        self.wavelength, self.eps, self.tand = float(wavelength), float(eps), float(tand)
        self.spacing = spacing
        self.kappa = _doe.phase_scale(self.wavelength, self.eps)
        self.h_max = 2.0 * torch.pi / self.kappa
        self.lut = optics.heightmap.host_table(lut, "IFTA", torch.float32)
        if not 1 <= len(self.lut) <= _lib.THZ_MAX_LUT:
            raise ValueError(f"IFTA: {len(self.lut)} levels; the kernels take 1 .. {_lib.THZ_MAX_LUT} (THZ_MAX_LUT)")
        self.doe_shape = (int(doe_shape[0]), int(doe_shape[1]))
        self.device = torch.device(asm.device)
        self.incident = None
        if incident is not None:
            self.incident = self._plane(incident, "incident field", complex_=True)
            self._check_cells(*self.incident.shape)
        self.window = None
        if window is not None:
            if not torch.is_tensor(window) or window.dtype not in (torch.bool, torch.uint8) or window.dim() != 2:
                raise TypeError("IFTA: the window must be a bool / uint8 [H, W] tensor")
            self.window = window.to(self.device).contiguous()
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))
        self._state = None  # the buffers (and graph) of the last shapes run
        self.captures = 0   # graphs captured so far

    # -- arguments -----------------------------------------------------------------------------
    def _plane(self, t, what, complex_):
        """``t`` as [H, W]: one batch item, one wavelength."""
        if not torch.is_tensor(t):
            raise TypeError(f"IFTA: the {what} must be a tensor")
        if t.dtype in (torch.complex128, torch.float64):
            raise TypeError(f"IFTA: the kernels compute in complex64 / float32; got a {t.dtype} {what}")
        if complex_ and t.dtype != torch.complex64:
            raise TypeError(f"IFTA: the {what} must be complex64; got {t.dtype}")
        if t.dim() < 2 or t.numel() != t.shape[-2] * t.shape[-1]:
            raise ValueError(f"IFTA: one batch item and one wavelength (B = C = 1); got a {what} of "
                             f"{tuple(t.shape)}")
        return t.detach().reshape(t.shape[-2:]).to(self.device).contiguous()

    def _check_cells(self, H, W):
        hs, ws = self.doe_shape
        if hs < 1 or ws < 1 or H % hs or W % ws:
            raise ValueError(f"IFTA: a {H} x {W} field over doe_shape {self.doe_shape}: every cell must be a whole "
                             "number of field pixels")

    def _target(self, target):
        """The target amplitude as float32 [H, W] or [Z, H, W]."""
        if not torch.is_tensor(target):
            raise TypeError("IFTA: the target amplitude must be a tensor")
        if target.is_complex() or target.dtype == torch.float64:
            raise TypeError(f"IFTA: the kernels compute in float32; got a {target.dtype} target amplitude")
        if target.dim() < 2:
            raise ValueError(f"IFTA: target amplitude {tuple(target.shape)}: [H, W] or [Z, H, W]")
        H, W = target.shape[-2:]
        Z, lead = len(self.zs), target.numel() // (H * W)
        if lead == 1:
            t = target.reshape(H, W)
        elif lead == Z and target.shape[0] == Z:
            t = target.reshape(Z, H, W)
        else:
            raise ValueError(f"IFTA: target amplitude {tuple(target.shape)} for {Z} planes: one batch item and one "
                             "wavelength (B = C = 1), [H, W] or [Z, H, W]")
        return t.detach().to(device=self.device, dtype=torch.float32)

    # -- the loop ------------------------------------------------------------------------------
    def _buffers(self, H, W, t_shape, iters):
        key = (H, W, tuple(t_shape), iters)
        if self._state is None or self._state["key"] != key:
            dev, (hs, ws), Z = self.device, self.doe_shape, len(self.zs)
            inc = self.incident if self.incident is not None else torch.ones((H, W), dtype=torch.complex64, device=dev)
            field = ElectricField(inc.reshape(1, 1, H, W), wavelengths=self.wavelength, spacing=self.spacing,
                                  device=dev)
            field.wavelengths_host, field.spacing_host  # the host mirrors, read here once
            self._state = dict(key=key, field=field, graph=None,
                               init=torch.zeros((hs, ws), dtype=torch.float32, device=dev),
                               target=torch.zeros(t_shape, dtype=torch.float32, device=dev),
                               q=torch.zeros(iters, dtype=torch.float32, device=dev),
                               history=torch.zeros((iters, Z, 6), dtype=torch.float64, device=dev),
                               height=torch.zeros((hs, ws), dtype=torch.float32, device=dev),
                               idx=torch.zeros((hs, ws), dtype=torch.int32, device=dev))
        return self._state

    def _loop(self, st, iters):
        """All iterations on the state's buffers; every launch is on the current stream."""
        field, asm = st["field"], self.asm
        data = field._data
        _, _, H, W = data.shape
        Z = len(self.zs)
        ph, pw = asm.compute_padding(H, W, return_size_of_padding=True)
        wl, sp, bl = field.wavelengths_host, field.spacing_host, asm._bandlimit_code()
        h, idx = st["init"], None
        for it in range(iters):
            field._pending = _doe.PendingModulation(data, h, wl, self.eps, self.tand, tolerance=None)
            planes = asm.propagate_planes(field, self.zs).reshape(Z, H, W)
            row = optics.ifta_target_stats(planes, st["target"], self.window, out=st["history"][it])
            if self.scale == "plane":
                s = row[:, 4].contiguous()
            else:
                tu, tt = row[:, 2].sum(), row[:, 3].sum()
                s = torch.where(tt == 0, torch.zeros_like(tt), tu / tt).expand(Z).contiguous()
            optics.ifta_target_project(planes, st["target"], s, self.window, self.alpha, self.beta, out=planes)
            back = _prop.asm_apply(planes.reshape(Z, 1, 1, H, W), wl, sp, self.zs, ph, pw, True, bl, adjoint=True)
            h, idx = optics.ifta_doe_project(back.reshape(H, W), self.doe_shape, self.wavelength, self.eps, self.lut,
                                             q=st["q"][it:it + 1], incident=self.incident)
        field._pending = None
        st["height"].copy_(h)
        st["idx"].copy_(idx)

    def _capture(self, st, iters):
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):  # plans, workspaces and the allocator's pools are made outside the capture
            self._loop(st, min(iters, 2))
        torch.cuda.current_stream(self.device).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode=_CAPTURE_MODE):
            self._loop(st, iters)
        self.captures += 1
        return g

    def run(self, target_amplitude, iters=50, q_schedule=None, init=None, graph=True):
        """Design a map for ``target_amplitude`` ([H, W] for every plane or [Z, H, W], non-negative).

        ``q_schedule``: ``iters`` snap fractions in [0, 1], copied once to the device; None: a linear ramp from 0 to 1
        over the first 80 % of the run, then 1.  A schedule that ends below 1 leaves cells off the table (idx -1).
        ``init``: a height map [hs, ws]; None: a uniform draw in [0, h_max) from the designer's seeded generator.
        ``graph=True``: the loop is captured once per (field size, target shape, iters) and replayed on every later
        run, whatever the target, init and schedule hold.  Nothing here waits for the device; read ``history`` when
        you choose to."""
        iters = int(iters)
        if iters < 1:
            raise ValueError(f"IFTA.run: iters must be at least 1; got {iters}")
        target = self._target(target_amplitude)
        H, W = target.shape[-2:]
        if self.incident is not None and tuple(self.incident.shape) != (H, W):
            raise ValueError(f"IFTA.run: target planes of {(H, W)} for an incident field of "
                             f"{tuple(self.incident.shape)}")
        if self.window is not None and tuple(self.window.shape) != (H, W):
            raise ValueError(f"IFTA.run: target planes of {(H, W)} for a window of {tuple(self.window.shape)}")
        self._check_cells(H, W)
        qs = default_q_schedule(iters) if q_schedule is None else [float(v) for v in q_schedule]
        if len(qs) != iters or not all(0.0 <= v <= 1.0 for v in qs):
            raise ValueError(f"IFTA.run: q_schedule needs {iters} values in [0, 1]")
        with torch.no_grad(), torch.cuda.device(self.device):
            st = self._buffers(H, W, target.shape, iters)
            st["target"].copy_(target)
            st["q"].copy_(torch.tensor(qs, dtype=torch.float32))
            if init is None:
                st["init"].uniform_(0.0, self.h_max, generator=self._gen)
            else:
                if (not torch.is_tensor(init) or tuple(init.shape[-2:]) != self.doe_shape
                        or init.numel() != st["init"].numel()):
                    raise ValueError(f"IFTA.run: init must be a height map of {self.doe_shape}")
                st["init"].copy_(init.detach().reshape(self.doe_shape).to(torch.float32))
            if graph:
                if st["graph"] is None:
                    st["graph"] = self._capture(st, iters)
                st["graph"].replay()
            else:
                self._loop(st, iters)
            return IFTAResult(st["height"].clone(), st["idx"].to(torch.int64), st["history"].clone(),
                              (self.eps, self.tand), self.device)
