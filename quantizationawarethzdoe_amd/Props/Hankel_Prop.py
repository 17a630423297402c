"""Hankel propagator of rotationally symmetric fields, Hankel_prop -- an addition of this port (the reference
propagates every field on a 2-D grid).

A symmetric field is its profile on N rings, and the quasi-discrete Hankel transform carries it to any plane with
two products by one N x N table (hankel.py, csrc/thz_hankel.hip) instead of three passes over a
padded P x P grid.  The rings are the transform's nodes ``.r`` (proportional to the zeros of J0, nearly uniform);
``sample_rings`` brings a uniform radial profile, such as a RotationallySymmetric*DOELayer's, onto them.

A design step of a lens-like element, on-axis intensity over a focal range::

    prop = Hankel_prop(z_distance=0.1, num_rings=2048, r_max=0.2, device=dev)
    beam = torch.exp(-(prop.r / 40e-3) ** 2).to(torch.complex64).view(1, 1, 1, -1)          # [B, C, 1, N]
    height = prop.sample_rings(profile, dx).float().view(1, -1)                             # [1, N], from [R] bins
    field, _ = doe.modulate(beam, height, [lam], eps, tand)                                 # the thin element
    axis = prop.propagate_zr(field.view(1, 1, -1), [lam], z_list, keep=1)                   # [Z, 1, 1, 1]
    loss = -(axis.abs() ** 2).sum()
    loss.backward()                                                                         # to profile

The thin-element screen needs no kernel of its own: ``doe.modulate`` on a one-row field is it.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from quantizationawarethzdoe_amd import hankel


class Hankel_prop(nn.Module):
    """``Hankel_prop(z_distance, num_rings, r_max, device=None)``: ``num_rings`` rings (1 .. 8192) on the aperture
    radius ``r_max``.  The field vanishes at r = r_max, the transform's boundary, so ``r_max`` is chosen larger
    than the element -- the counterpart of ASM_prop's ``padding_scale``."""

    def __init__(self, z_distance: float = 0.0, num_rings: int = 1024, r_max: float = 1.0, device=None) -> None:
        super().__init__()
        self.device = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
        self.z = float(z_distance)
        self.num_rings = int(num_rings)
        self.r_max = float(r_max)
        if self.num_rings < 1 or not self.r_max > 0:
            raise ValueError(f"Hankel_prop: num_rings = {num_rings} >= 1 and r_max = {r_max} > 0 are required")

    @property
    def r(self):
        """the nodes r_n, float64 [N]"""
        return hankel.hankel_nodes(self.num_rings, self.r_max, self.device)[0]

    @property
    def kappa(self):
        """the radial frequencies kappa_m, float64 [N]"""
        return hankel.hankel_nodes(self.num_rings, self.r_max, self.device)[1]

    def forward(self, profile, wavelengths):
        """``profile`` complex64 [B, C, N] on ``.r`` -> the profile at ``.z``, [B, C, N]"""
        return self.propagate_zr(profile, wavelengths, [self.z])[0]

    def propagate_zr(self, profile, wavelengths, z_list, keep=None):
        """-> complex64 [Z, B, C, keep]: the first ``keep`` rings (default all) of every plane of ``z_list`` in one
        call; ``keep=1`` is the near-axis sample alone, which an extended-depth-of-focus loss reads.  Equal to Z
        one-plane calls bit for bit for N <= 128, to rounding above (``hankel.hankel_propagate``)."""
        if profile.shape[-1] != self.num_rings:
            raise ValueError(f"Hankel_prop: a profile of {profile.shape[-1]} rings for num_rings = {self.num_rings}")
        return hankel.hankel_propagate(profile, wavelengths, self.r_max, z_list, keep=keep)

    def create_kernel(self, wavelengths, z_list=None):
        """H complex64 [Z, C, N] as the kernels form it, for inspection (``z_list`` default: ``[.z]``)"""
        return hankel.hankel_transfer_function(wavelengths, self.r_max, [self.z] if z_list is None else z_list,
                                               self.num_rings, self.device)

    def sample_rings(self, values, dx):
        """A uniform radial profile ``values`` [..., R] of ring pitch ``dx`` on the nodes: bin floor(r_n / dx), the
        continuous form of ``radial_bin``, and 0 beyond the last bin.  A torch gather: differentiable, off the hot
        path."""
        R = values.shape[-1]
        idx = torch.floor(self.r / float(dx)).to(torch.int64)
        inside = idx < R
        picked = values.index_select(-1, idx.clamp(max=R - 1).to(values.device))
        return picked * inside.to(values.device).to(picked.dtype)
