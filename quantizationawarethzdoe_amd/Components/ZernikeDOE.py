"""A DOE whose height map is a Zernike series over a circular pupil.

The reference's Components/Hologram*.py and PhaseHologram.py parameterise their maps by Zernike coefficients; this
element brings that parameterisation to the DOE layers of this port: a smooth map with at most 120 degrees of freedom,
the usual well-conditioned start before a quantizer or the IFTA take over.  The map is synthesised by
``zernike.synthesize`` (csrc/thz_zernike.hip) and applied exactly as ``FixDOEElement`` applies its map.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from quantizationawarethzdoe_amd import zernike
from quantizationawarethzdoe_amd.Components.QuantizedDOE import DOELayer
from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField


class ZernikeDOEElement(DOELayer):
    """``ZernikeDOEElement(coeffs, pupil, shape, spacing, material, wrap=None, base=0.0)``: the height map is
    ``base + zernike.synthesize(coeffs, shape, spacing, pupil)`` in metres (``base`` alone outside the pupil), taken
    modulo ``wrap`` when one is given (a kinoform of that depth; the gradient is 1 almost everywhere).  ``coeffs`` is
    float32 [K], K a full set of orders; an ``nn.Parameter`` is kept as it is and trained (its gradient arrives through
    thz_zernike_project), anything else is stored as a fixed buffer.  ``material`` = [epsilon, tan delta]."""

    def __init__(self, coeffs, pupil, shape, spacing, material: list, wrap: float = None, base: float = 0.0,
                 device: torch.device = None) -> None:
        super().__init__()
        self.device = device if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if isinstance(coeffs, nn.Parameter):
            self.coeffs = coeffs
        else:
            self.register_buffer("coeffs", torch.as_tensor(coeffs, dtype=torch.float32).detach().clone().to(self.device))
        if self.coeffs.dim() != 1:
            raise ValueError(f"ZernikeDOEElement: coeffs are [K]; got {tuple(self.coeffs.shape)}")
        if wrap is not None and not float(wrap) > 0.0:
            raise ValueError(f"ZernikeDOEElement: wrap = {wrap} must be positive")
        n, m = zernike.orders(self.coeffs.shape[0] - 1)
        zernike._geometry(shape, spacing, pupil, n, "ZernikeDOEElement")  # the argument errors, at construction
        self.pupil, self.shape, self.spacing = tuple(float(v) for v in pupil), (int(shape[-2]), int(shape[-1])), spacing
        self.wrap, self.base = None if wrap is None else float(wrap), float(base)
        self.material = torch.tensor(material, device=self.device)
        self.epsilon = self.material[0]
        self.tand = self.material[1]

    def build_height_map(self):
        h = zernike.synthesize(self.coeffs, self.shape, self.spacing, self.pupil) + self.base
        return h if self.wrap is None else torch.remainder(h, self.wrap)

    @property
    def height_map(self):
        return self.build_height_map()

    def forward(self, field: ElectricField) -> ElectricField:
        return self.modulate(field, self.build_height_map(), None, self.epsilon, self.tand)
