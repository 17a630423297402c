"""A DOE of finite thickness: split-step (multi-slice) propagation through the relief.

MI355X addition with no counterpart in the reference, whose layers (Components/QuantizedDOE.py) apply
the thin-element screen and leave the field in the plane it entered; its FDTDval/ notebooks check
designs against a full-wave solver instead.  ``ThickDOEElement`` takes a fixed height map, as
``FixDOEElement`` does, and returns the field in the plane ``thickness`` above the base plate
(optics.thick_doe: the model, the sign conventions and the supported geometries).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from quantizationawarethzdoe_amd import optics
from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField


class ThickDOEElement(nn.Module):
    """``ThickDOEElement(height_map, thickness, slices, material, padding_scale=1, convention="reference",
    device=None)``: ``material`` = [epsilon, tan delta]; ``padding_scale`` and the "exact" band limit are
    those of the ASM step between slabs.  ``method`` ("auto", "fused", "compose") may be set on the
    instance; "auto" runs the fused kernels unless a gradient is asked for.  ``grad="fused"`` (optics.thick_doe)
    keeps gradients on the fused kernels' native backward; a ``height_map`` handed in as a tensor that requires
    grad (or an ``nn.Parameter``) is then kept as it is, attached, so the map can be designed on the thick model."""

    def __init__(self, height_map, thickness: float, slices: int, material: list = None, padding_scale=1,
                 convention: str = "reference", device: torch.device = None, grad: str = None) -> None:
        super().__init__()
        self.device = device if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if grad not in (None, "fused"):
            raise ValueError(f"ThickDOEElement: grad must be None or 'fused'; got {grad!r}")
        self.grad = grad
        if grad == "fused" and torch.is_tensor(height_map) and height_map.requires_grad:
            # the map under design: the caller's parameter (registered), or their graph's tensor
            self.height_map = height_map
        else:
            h = height_map.detach().clone() if torch.is_tensor(height_map) else torch.tensor(np.asarray(height_map))
            # a fixed map: no gradient unless the caller asks for one (height_map.requires_grad_(True) sends
            # "auto" down the differentiable compose path)
            self.height_map = nn.parameter.Parameter(h.to(device=self.device, dtype=torch.float32),
                                                     requires_grad=False)
        if convention not in optics.THICK_CONVENTIONS:
            raise ValueError(f"ThickDOEElement: convention must be 'reference' or 'physical'; got {convention!r}")
        if int(slices) < 1 or not float(thickness) > 0.0:
            raise ValueError(f"ThickDOEElement: thickness > 0 and slices >= 1; got {thickness}, {slices}")
        self.thickness, self.slices = float(thickness), int(slices)
        self.material = torch.tensor(material, device=self.device)
        self.epsilon = self.material[0]
        self.tand = self.material[1]
        self._eps_tand = (float(material[0]), float(material[1]))
        self.padding_scale = padding_scale
        self.bandlimit = "exact"
        self.convention = convention
        self.method = "auto"

    def forward(self, field: ElectricField) -> ElectricField:
        data = field.data
        if data.dtype == torch.complex128:
            raise TypeError("ThickDOEElement: the DOE kernels compute in complex64; got a complex128 field -- cast "
                            "the field to complex64 before the DOE layer")
        out = optics.thick_doe(data, self.height_map, field.wavelengths_host, field.spacing_host,
                               self._eps_tand[0], self._eps_tand[1], self.thickness, self.slices,
                               padding_scale=self.padding_scale, bandlimit=self.bandlimit,
                               convention=self.convention, method=self.method, grad=self.grad)
        Eout = ElectricField(data=out, wavelengths=field.wavelengths, spacing=field.spacing, device=field.device)
        return Eout._adopt_host(field)
