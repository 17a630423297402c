"""Rayleigh-Sommerfeld convolution, RSC_prop / VRS_prop -- drop-in for Props/RSC_Prop.py.

Same constructor (``z_distance, device``; :17-45), ``z`` property (:47-57),
``compute_padding`` (:60-77, padding scale 1), once-per-instance minimum-distance diagnostic
(:89-127) and ``forward(field) -> ElectricField`` (:170-215, :265-321).  As in the
reference, RSC_prop takes a single field (B == 1, :198-200) and the output window is
ifft2(...)[..., H:, W:] (so an odd N returns N-1 samples, :207); VRS_prop forms Ez from the
field's Ex/Ey planes and returns 3 planes.  One documented difference: where the reference's
diagnostic crashes (z_min1 = 0 is an int without ``.detach``, :112-117) this mirror prints
0.000 mm and continues.  The math runs in libthzdoe's gfx950 kernels (the spatial-kernel
FFT and the convolution passes of thz_asm.hip; the z-x slice of thz_rsc.hip).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
from quantizationawarethzdoe_amd import propagation as _prop
from quantizationawarethzdoe_amd.Props import _zx
from quantizationawarethzdoe_amd.Props._zx import _f, _z_host

mm = 1e-3


class RSC_prop(nn.Module):
    _vectorial = False

    def __init__(self, z_distance: float = 0.0, device: str = None) -> None:
        super().__init__()
        self.do_padding = True
        self.DEFAULT_PADDING_SCALE = torch.tensor([1, 1])
        self.device = device or torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self._z = torch.tensor(z_distance, device=self.device)
        self._zh = _f(z_distance)
        self.shape = None
        self.check_Zc = True

    @property
    def z(self):
        return self._z

    @z.setter
    def z(self, z) -> None:
        if isinstance(z, torch.Tensor) and z.device != torch.device(self.device):
            z = z.to(self.device)
        self._z = z
        self._zh = _f(z)

    def compute_padding(self, H, W, return_size_of_padding=False):
        """Props/RSC_Prop.py:60-77."""
        ph, pw = (int(np.floor(H / 2)), int(np.floor(W / 2))) if self.do_padding else (0, 0)
        if return_size_of_padding:
            return ph, pw
        return H + 2 * ph, W + 2 * pw

    def check_RS_minimum_z(self, quality_factor=1, dx=None, dy=None, wavelength=None, Ph=None):
        """Energy-conservation / sampling minimum distances, printed (Props/RSC_Prop.py:89-127)."""
        f32 = np.float32
        dx, dy, lam = f32(dx), f32(dy), f32(wavelength)
        range_x, range_y = f32(self.shape[-2]) * dx, f32(self.shape[-1]) * dy
        dr = np.sqrt(dx ** 2 + dy ** 2)
        rmax = np.sqrt(range_x ** 2 + range_y ** 2)
        factor = (((f32(quality_factor) * dr + rmax) ** 2 - lam ** 2 - rmax ** 2) / (f32(2) * lam)) ** 2 - rmax ** 2
        z_min1 = np.sqrt(factor) if factor > 0 else f32(0)
        print("Minimum propagation distance to satisfy energy conservation: {:.3f} mm".format(z_min1 / mm))
        with np.errstate(invalid="ignore"):
            z_min2 = f32(Ph) * dx ** 2 / lam * np.sqrt(f32(1) - (lam / (f32(2) * dx)) ** 2)
        print("Minimum propagation distance to satisfy sampling for FT: {:.3f} mm".format(z_min2 / mm))
        if self._zh > min(z_min1, z_min2):
            print("The simulation will be accurate !")
        else:
            print("The propagation distance should be larger than minimum propagation distance to keep "
                  "simulation accurate!")

    def create_spatial_grid(self, H, W, dx, dy):
        """linspace(-N dx/2, N dx/2, N) on both axes WITH dx (Props/RSC_Prop.py:79-87, the
        reference's y grid uses dx too), meshgrid 'ij', on the module's device."""
        def grid(n):
            e = (np.float32(-n) * np.float32(_f(dx))) / np.float32(2), (np.float32(n) * np.float32(_f(dx))) / np.float32(2)
            return torch.linspace(float(e[0]), float(e[1]), int(n))
        meshx, meshy = torch.meshgrid(grid(H), grid(W), indexing="ij")
        return meshx.to(device=self.device), meshy.to(device=self.device)

    def _kernel_grid(self, H, W, dx):
        """The grid the convolution kernels evaluate the RS kernel on: the same end points as
        create_spatial_grid, each coordinate as ONE fp32 expression, start + step i below the middle
        and end + step (i - (n - 1)) from it on (csrc/thz_dev.hpp lin()).  torch.linspace on the CPU
        (the reference's meshes) adds the step per SIMD lane onto a rounded vector base, a second
        rounding: about 40 % of its coordinates differ from these by one ulp, k ulp = 7.5e-4 rad at
        the far end of a 16384-point line."""
        def grid(n):
            lo, hi = (np.float32(-n) * np.float32(_f(dx))) / np.float32(2), (np.float32(n) * np.float32(_f(dx))) / np.float32(2)
            if n == 1:
                return torch.tensor([float(lo)])
            step = (hi - lo) / np.float32(n - 1)
            i = np.arange(n)
            low = i < n // 2
            k = np.where(low, i, i - (n - 1)).astype(np.float32)
            return torch.from_numpy(np.where(low, lo, hi).astype(np.float32) + step * k)
        meshx, meshy = torch.meshgrid(grid(H), grid(W), indexing="ij")
        return meshx.to(device=self.device), meshy.to(device=self.device)

    def create_kernel(self, field: ElectricField) -> torch.Tensor:
        """The spatial RS kernel exp(ikr) z/(2 pi r^2)(1/r - ik) on the padded grid, [1, C, Ph, Pw]
        (Props/RSC_Prop.py:129-167), with the once-per-instance minimum-distance print.  The
        convolution kernels take FFT2 of the same values in-kernel; this materialises them with
        thz_rs_kernel for inspection, on the kernels' own grid (_kernel_grid), so the table is what
        the propagation applies (tests/test_table_parity_gpu.py), and sets ``meshx`` / ``meshy`` as
        the reference does (torch.linspace: equal to the kernels' grid to one ulp)."""
        B, C, H, W = field.shape
        Ph, Pw = self.compute_padding(H, W)
        sp, wl = field.spacing_host, field.wavelengths_host
        self.meshx, self.meshy = self.create_spatial_grid(Ph, Pw, sp[0], sp[1])
        if self.check_Zc:
            self.shape = field.shape
            self.check_RS_minimum_z(1, sp[0], sp[1], min(wl), Ph=Ph)
            self.check_Zc = False
        return _prop.rs_kernel(*self._kernel_grid(Ph, Pw, sp[0]), self._zh, wl)

    def _single_field(self, B):
        if not self._vectorial and B != 1:
            raise RuntimeError(f"RSC_prop convolves a single field (B == 1) as the reference does "
                               f"(Props/RSC_Prop.py:198-200); got B={B}")

    def forward(self, field: ElectricField) -> ElectricField:
        data = field.data
        B, C, H, W = self.shape = data.shape
        self._single_field(B)
        sp = field.spacing_host
        wl = field.wavelengths_host
        if self.check_Zc:
            self.check_RS_minimum_z(1, sp[0], sp[1], min(wl), Ph=H + 2 * (H // 2))
            self.check_Zc = False
        x = _prop.kernel_dtype(data, "RSC_prop", field.wavelengths)
        out = _RscFunction.apply(x, tuple(wl), tuple(sp), self._zh, self._vectorial)
        Eout = ElectricField(data=out, wavelengths=field.wavelengths, spacing=field.spacing, device=field.device)
        return Eout._adopt_host(field)

    def propagate_planes(self, field: ElectricField, z_list) -> torch.Tensor:
        """Additive API: the planes of ``z_list`` -> [Z, Bo, C, Ho, Wo], ``forward`` per plane (the same
        kernels, differentiable) stacked; the instance's own ``z`` is not touched.  The counterpart of
        ASM_prop / CZT_prop.propagate_planes, and the fallback and yardstick of propagate_zx."""
        self._single_field(field.data.shape[0])
        x = _prop.kernel_dtype(field.data, "RSC_prop", field.wavelengths)
        wl, sp = tuple(field.wavelengths_host), tuple(field.spacing_host)
        return torch.stack([_RscFunction.apply(x, wl, sp, zh, self._vectorial) for zh in _z_host(z_list)])

    def propagate_zx(self, field: ElectricField, z_list, row=None, axis="x", grad="planes") -> torch.Tensor:
        """Additive API: one output row of every plane of ``z_list`` -> [Z, Bo, C, Wo], equal to
        ``propagate_planes(field, z_list)[..., row, :]`` -- the x-z cross-section of a focal region on
        the Rayleigh-Sommerfeld convolution, which otherwise costs one ``forward`` per plane.  ``row``
        indexes the Ho = 2 (H // 2) output rows; None is the centre row Ho // 2.  ``axis="y"`` returns
        ``planes[..., :, row]`` instead, [Z, Bo, C, Ho], ``row`` then indexing the Wo output columns.
        ``z_list`` may have any length (chunks of THZ_MAX_Z planes).

        A complex64 device field that does not require grad (or under ``no_grad``) runs the slice
        kernels (thz_rsc_slice_forward): the input rows' spectra once, then per plane H kernel rows
        evaluated, transformed and accumulated, and one inverse line per (z, b, c) -- no transform
        along H, no Ph x Pw kernel table.  ``axis="y"`` runs them on the transposed field with the
        spacing unchanged: the kernel's grid takes dx on both axes (Props/RSC_Prop.py:83-84) and
        dx dy is symmetric, so the exchange is exact; for VRS the Ex / Ey planes are exchanged going in
        and output planes 0 / 1 coming out (Ez = Ex x / r + Ey y / r is symmetric under the exchange).
        A complex128 field or an input that requires grad propagates the full planes in z-chunks whose
        temporary stays under 10 GiB and slices each chunk (Props/_zx.py sliced_planes, as ASM_prop and
        CZT_prop do), which keeps the fp64 kernels and autograd.

        ``grad`` chooses what serves a differentiated call, as on ASM_prop / CZT_prop.propagate_zx.
        ``"planes"`` (the default) is the behaviour above.  ``"slice"``: the slice kernels serve a
        complex64 device field whether or not it requires grad, and the backward is their own adjoint
        (thz_rsc_slice_adjoint: one cotangent line transform per (z, b, c), the kernel rows' conjugated
        spectra summed over the planes in the spectrum, one inverse row per (b, c, i); nothing of a
        plane's size per z in either direction); ``axis="y"`` transposes and exchanges Ex / Ey outside
        the slice (torch differentiates both).  A complex128 field still takes the full planes.  Any
        other value is a ValueError."""
        _zx.check_axis_grad(axis, grad)
        B, C, H, W = field.data.shape
        Ho, Wo = 2 * (H // 2), 2 * (W // 2)
        row = _zx.output_row(row, Ho if axis == "x" else Wo, axis)
        self._single_field(B)
        zs = _z_host(z_list)
        x = _prop.kernel_dtype(field.data, "RSC_prop", field.wavelengths)
        diff = torch.is_grad_enabled() and x.requires_grad
        if x.dtype == torch.complex64 and x.is_cuda and not (diff and grad == "planes"):
            swap = axis == "y" and self._vectorial  # Ex / Ey exchanged going in, planes 0 / 1 coming out
            xs = x.transpose(-1, -2) if axis == "y" else x
            out = _zx.native_sweep("rsc", xs[[1, 0]] if swap else xs, tuple(field.wavelengths_host),
                                   tuple(field.spacing_host), zs, row, (self._vectorial,))
            return out[:, [1, 0, 2]] if swap else out
        plane_bytes = (3 if self._vectorial else B) * C * Ho * Wo * (16 if x.dtype == torch.complex128 else 8)
        return _zx.sliced_planes(lambda chunk: self.propagate_planes(field, chunk), zs, plane_bytes, row, axis)


class VRS_prop(RSC_prop):
    """Vectorial RS: Ez = (Ex x + Ey y) / r, then the scalar convolution per component (:218-321)."""
    _vectorial = True


class _RscFunction(torch.autograd.Function):
    """Forward on the HIP convolution; backward = the adjoint convolution (conj FFT2(K), windows
    exchanged).  VRS: out = [RSC(Ex), RSC(Ey), RSC(Ez)], Ez = Ex x/r + Ey y/r, so
    dEx = RSC^H(g0) + x/r RSC^H(g2) and dEy = RSC^H(g1) + y/r RSC^H(g2) on the unpadded grid."""

    @staticmethod
    def forward(ctx, data, wavelengths, spacing, z, vectorial):
        ctx.cfg = (wavelengths, spacing, z, vectorial, tuple(data.shape))
        return _prop.rsc_apply(data, wavelengths, spacing, z, vectorial)

    @staticmethod
    def backward(ctx, g):
        wavelengths, spacing, z, vectorial, shape = ctx.cfg
        B, C, H, W = shape
        adj = _prop.rsc_apply(g.contiguous(), wavelengths, spacing, z, adjoint=True, field_hw=(H, W))
        if not vectorial:
            return adj, None, None, None, None
        # the Ez grid in the field's precision (fp32 for complex64, fp64 for complex128)
        rdt = torch.float64 if adj.dtype == torch.complex128 else torch.float32
        dx = torch.tensor(spacing[0], dtype=rdt)
        x = torch.linspace(float(-dx * H / 2), float(dx * H / 2), H, device=g.device, dtype=rdt)
        y = torch.linspace(float(-dx * W / 2), float(dx * W / 2), W, device=g.device, dtype=rdt)
        X, Y = torch.meshgrid(x, y, indexing="ij")
        r = torch.sqrt(X ** 2 + Y ** 2 + torch.tensor(z, dtype=rdt) ** 2)
        gin = torch.zeros(shape, dtype=adj.dtype, device=g.device)
        gin[0] = adj[0] + adj[2] * (X / r)
        gin[1] = adj[1] + adj[2] * (Y / r)
        return gin, None, None, None, None
