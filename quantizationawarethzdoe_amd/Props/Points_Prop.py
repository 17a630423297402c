"""Propagation to arbitrary detector points, Points_prop -- an addition of this port (the reference propagates every
field to a grid parallel to the element).

The Rayleigh-Sommerfeld integral is summed directly from the source pixels to a list of 3-D points (points.py,
csrc/thz_points.hip): a scan path, a tilted camera, an arc of diffraction orders, a few loss points.  The
kernel function is RSC_prop's, so the result is also an independent check of the FFT propagators at any point.

A camera tilted by 20 degrees, 60 mm behind the element, and a loss on what it sees::

    from quantizationawarethzdoe_amd import points
    cam = Points_prop(points.tilted_plane((64, 64), 0.5e-3, center=(0, 0, 60e-3), tilt_y=math.radians(20)))
    seen = cam(field)                       # complex64 [B, C, 64, 64]
    (-(seen.abs() ** 2)[..., 32, 32].sum()).backward()
"""
from __future__ import annotations

import torch
import torch.nn as nn

from quantizationawarethzdoe_amd import points as _points


class Points_prop(nn.Module):
    """``Points_prop(points, origin=(0, 0))``: ``points`` [..., 3] in metres with z > 0, host data (checked here, uploaded
    once per device) or a device tensor (taken as it is); ``origin`` the (x, y) of the field's centre."""

    def __init__(self, points, origin=(0.0, 0.0)) -> None:
        super().__init__()
        on_device = torch.is_tensor(points) and points.is_cuda
        self.points = points if on_device else _points.host_points(points, "Points_prop")
        self.origin = (float(origin[0]), float(origin[1]))
        self._uploaded = {}

    def forward(self, field, chunks=None) -> torch.Tensor:
        """``field`` an ElectricField -> complex64 [B, C, *points.shape[:-1]]"""
        pts = self.points
        if not pts.is_cuda:
            dev = field.data.device
            if dev not in self._uploaded:
                self._uploaded[dev] = pts.to(dev)
            pts = self._uploaded[dev]
        return _points.rs_points(field, pts, origin=self.origin, chunks=chunks)
