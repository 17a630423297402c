"""Fabrication-tolerance Monte Carlo: how much of a designed relief survives fabrication.

The reference puts ``tolerance`` into every DOE layer -- ``add_height_map_noise``, one U(-tol, tol) draw per pixel
(Components/QuantizedDOE.py:82-87) -- and compares its quantizers on the nominal map only.  This module answers the
yield question for a multi-level element: the efficiency and uniformity of the focal spots under

* a depth-scale error (print shrinkage, etch rate): every height times ``1 + g``, ``g ~ N(0, sigma_scale)``;
* a depth error per level: each of the L levels off by its own ``e_l ~ N(0, sigma_level[l])`` on every pixel of
  that level (``sigma_level[0] = 0`` models an unetched top level) -- a term the layers' ``tolerance`` cannot state;
* per-pixel roughness, the reference's uniform draw or a normal one.

``optics.tolerance_modulate`` forms K realisations of the modulated field in one streaming kernel from one read of
the map and the incident field (csrc/thz_tolerance.hip); the K fields ride the batch axis of the propagator and of
``optics.region_stats``.  Nothing is read from the device inside a run.

    fab = FabricationModel(sigma_scale=0.02, sigma_level=[0, 5e-6, 5e-6, 5e-6], roughness=("normal", 2e-6))
    report = ToleranceAnalysis(element, asm, regions, fab, incident, lut=lut).run(K=256)
    report.summary()["efficiency"]["q05"], report.yield_fraction(min_efficiency=0.6)
"""
import collections
import math

import torch

from . import _lib, optics
from .DataType.ElectricField import ElectricField


class FabricationModel:
    """``FabricationModel(sigma_scale=0.0, sigma_level=0.0, roughness=None, clamp=(0.0, None))``.

    ``sigma_scale``: std of the relative depth-scale error.  ``sigma_level``: std of the per-level depth error in
    metres, one number for every level or a list of up to 16, one per level.  ``roughness``: None, ``("uniform", a)``
    for ``(u - 0.5) 2 a`` (the reference's formula) or ``("normal", s)``.  ``clamp = (lo, hi)``: the realised height
    is held inside it; None switches a side off."""

    def __init__(self, sigma_scale=0.0, sigma_level=0.0, roughness=None, clamp=(0.0, None)):
        who = "FabricationModel"
        self.sigma_scale = self._sigma(sigma_scale, "sigma_scale", who)
        if isinstance(sigma_level, (int, float)):
            self.sigma_level = self._sigma(sigma_level, "sigma_level", who)
        else:
            levels = tuple(self._sigma(v, "sigma_level", who) for v in sigma_level)
            if not 1 <= len(levels) <= _lib.THZ_MAX_LUT:
                raise ValueError(f"{who}: sigma_level has {len(levels)} entries; one number or 1 .. {_lib.THZ_MAX_LUT}")
            self.sigma_level = levels
        if roughness is not None:
            if not isinstance(roughness, (tuple, list)) or len(roughness) != 2 or roughness[0] not in optics.TOLERANCE_ROUGHNESS:
                raise ValueError(f"{who}: roughness must be None, ('uniform', a) or ('normal', s); got {roughness!r}")
            roughness = (roughness[0], self._sigma(roughness[1], "roughness", who))
        self.roughness = roughness
        if not isinstance(clamp, (tuple, list)) or len(clamp) != 2:
            raise ValueError(f"{who}: clamp must be (lo, hi), None for an open side; got {clamp!r}")
        lo, hi = (None if v is None else float(v) for v in clamp)
        if any(v is not None and math.isnan(v) for v in (lo, hi)) or (lo is not None and hi is not None and lo > hi):
            raise ValueError(f"{who}: clamp = {clamp!r} needs lo <= hi")
        self.clamp = (lo, hi)

    @staticmethod
    def _sigma(v, name, who):
        v = float(v)
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError(f"{who}: {name} = {v} must be finite and >= 0")
        return v

    @property
    def has_level_term(self):
        s = self.sigma_level
        return s != 0.0 if isinstance(s, float) else any(v != 0.0 for v in s)

    def for_levels(self, L):
        """The model with ``sigma_level`` spelled out for an L-level table."""
        s = self.sigma_level
        if not isinstance(s, float) and len(s) != L:
            raise ValueError(f"FabricationModel: {len(s)} level sigmas for a table of {L} levels")
        levels = (s,) * L if isinstance(s, float) else s
        return FabricationModel(self.sigma_scale, levels, self.roughness, self.clamp)

    def __repr__(self):
        return (f"FabricationModel(sigma_scale={self.sigma_scale}, sigma_level={self.sigma_level}, "
                f"roughness={self.roughness}, clamp={self.clamp})")


_Q = (("q05", 0.05), ("q50", 0.50), ("q95", 0.95))


class ToleranceReport:
    """``efficiency`` [K, R] and ``uniformity`` [K] (float64, on the device) of the K realisations, with the
    definitions of ``utils.metrics.diffraction_efficiency`` / ``spot_uniformity``, and ``nominal``, a dict of the
    same two for the unperturbed map ([R] and a scalar)."""

    def __init__(self, efficiency, uniformity, nominal):
        self.efficiency, self.uniformity, self.nominal = efficiency, uniformity, nominal

    @staticmethod
    def _stats(x):
        q = torch.quantile(x, torch.tensor([v for _, v in _Q], dtype=x.dtype, device=x.device), dim=0)
        out = {"mean": x.mean(dim=0), "std": x.std(dim=0, unbiased=False)}
        out.update({name: q[i] for i, (name, _) in enumerate(_Q)})
        return out

    def summary(self):
        """mean, std and the 5 / 50 / 95 % quantiles over the realisations of ``efficiency`` (per region),
        ``total_efficiency`` (the regions summed) and ``uniformity``."""
        return {"efficiency": self._stats(self.efficiency), "total_efficiency": self._stats(self.efficiency.sum(dim=-1)),
                "uniformity": self._stats(self.uniformity)}

    def yield_fraction(self, min_efficiency=None, max_uniformity=None):
        """The fraction of realisations whose summed region efficiency is at least ``min_efficiency`` and whose
        uniformity is at most ``max_uniformity`` (None: not asked), as a float."""
        ok = torch.ones(self.efficiency.shape[0], dtype=torch.bool, device=self.efficiency.device)
        if min_efficiency is not None:
            ok &= self.efficiency.sum(dim=-1) >= float(min_efficiency)
        if max_uniformity is not None:
            ok &= self.uniformity <= float(max_uniformity)
        return float(ok.double().mean())


_Element = collections.namedtuple("_Element", "height eps tand")


def _element_parts(element, who):
    """Height map [hs, ws] float32 and material of a ``FixDOEElement``, a trained layer or an ``IFTAResult``."""
    if hasattr(element, "as_element") and hasattr(element, "_material"):  # IFTAResult
        h, (eps, tand) = element.height, element._material
    else:
        h = getattr(element, "height_map", None)
        if h is None or getattr(element, "epsilon", None) is None:
            raise TypeError(f"{who}: the element needs a height_map and a material; got a {type(element).__name__}")
        eps, tand = element.epsilon, getattr(element, "tand", 0.0)
    if not torch.is_tensor(h) or h.numel() != h.shape[-2] * h.shape[-1]:
        raise ValueError(f"{who}: one height map [hs, ws]; got {tuple(getattr(h, 'shape', ()))}")
    return _Element(h.detach().reshape(h.shape[-2:]).to(torch.float32).contiguous(), float(eps), float(tand))


class ToleranceAnalysis:
    """``ToleranceAnalysis(element, propagator, regions, fab, field, *, lut=None, kind="circ", reference=None)``.

    ``element``: anything with a ``height_map`` and a material -- a ``FixDOEElement``, a trained layer, an
    ``IFTAResult``.  ``propagator``: a module mapping ``ElectricField -> ElectricField`` (ASM / CZT / RSC) that carries
    the field from the element to the plane the ``regions`` (rows of ``optics.region_stats``, with ``kind``) lie in.
    ``field``: the incident ``ElectricField`` ([1, C, H, W]).  ``lut``: the element's levels; every map pixel's level
    is ``optics.lut_quantize(height, lut, mode="argmin")``, required when ``fab`` has a per-level term.
    ``reference``: the field whose whole-plane power the efficiencies are taken over (as in
    ``diffraction_efficiency``); None: each realisation's own output plane."""

    def __init__(self, element, propagator, regions, fab, field, *, lut=None, kind="circ", reference=None):
        who = "ToleranceAnalysis"
        if not isinstance(fab, FabricationModel):
            raise TypeError(f"{who}: fab must be a FabricationModel; got a {type(fab).__name__}")
        if not isinstance(field, ElectricField):
            raise TypeError(f"{who}: the incident field must be an ElectricField; got a {type(field).__name__}")
        if not callable(propagator):
            raise TypeError(f"{who}: the propagator must map an ElectricField to an ElectricField")
        if field.shape[0] != 1:
            raise ValueError(f"{who}: one incident field [1, C, H, W]; got {tuple(field.shape)}")
        self.height, self.eps, self.tand = _element_parts(element, who)
        if fab.has_level_term and lut is None:
            raise ValueError(f"{who}: a per-level error needs lut, the element's levels")
        self.idx = None
        if lut is not None:
            levels = [float(v) for v in (lut.detach().cpu().reshape(-1) if torch.is_tensor(lut) else lut)]
            fab = fab.for_levels(len(levels))
            self.idx = optics.lut_quantize(self.height, levels, mode="argmin", surrogate=None)[1].to(torch.int32)
        self.fab, self.field, self.propagator = fab, field, propagator
        self.regions, self.kind, self.reference = regions, kind, reference
        R = len(regions)
        if R < 1:
            raise ValueError(f"{who}: at least one region")

    def _powers(self, data):
        """Region powers [N, R + 1] (the whole plane last, the channels summed) of the fields ``data`` [N, C, H, W]
        after the propagator."""
        f = self.field
        out = self.propagator(ElectricField(data=data, wavelengths=f.wavelengths, spacing=f.spacing, device=f.device))
        return optics.region_stats(out.data, self.regions, self.kind).power.sum(dim=1)

    def _grade(self, power):
        """(efficiency [N, R], uniformity [N]) of region powers [N, R + 1]."""
        if self.reference is None:
            total = power[:, -1:]
        else:
            ref = self.reference.data if isinstance(self.reference, ElectricField) else self.reference
            total = optics.region_stats(ref, [], "circ").power.sum().reshape(1, 1)
        eff = power[:, :-1] / total
        hi, lo = eff.amax(dim=-1), eff.amin(dim=-1)
        return eff, (hi - lo) / (hi + lo)

    def nominal(self):
        """Efficiency [R] and uniformity of the unperturbed map, through the same kernels (all sigmas 0)."""
        none = FabricationModel(clamp=(None, None))
        data = optics.tolerance_modulate(self.field.data, self.height, self.field.wavelengths_host, self.eps, self.tand,
                                         none, 1)
        eff, uni = self._grade(self._powers(data))
        return {"efficiency": eff[0], "uniformity": uni[0]}

    def run(self, K, chunk=32, rng=None):
        """K realisations in chunks of ``chunk``: per chunk one ``tolerance_modulate``, one propagator call and one
        ``region_stats`` on a batch of ``chunk`` fields, ``first`` advancing, so the table does not depend on
        ``chunk``.  ``rng = (state, stream)`` as in ``optics.add_noise``; None draws a state once for the run."""
        K, chunk = int(K), int(chunk)
        if K < 1 or chunk < 1:
            raise ValueError(f"ToleranceAnalysis.run: K = {K} and chunk = {chunk} must be >= 1")
        data = self.field.data
        rng = optics.noise.noise_state(data, rng)
        power = torch.empty((K, len(self.regions) + 1), dtype=torch.float64, device=data.device)  # all a run keeps
        with torch.no_grad():
            for first in range(0, K, chunk):
                n = min(chunk, K - first)
                mod = optics.tolerance_modulate(data, self.height, self.field.wavelengths_host, self.eps, self.tand,
                                                self.fab, n, idx=self.idx, rng=rng, first=first)
                power[first:first + n] = self._powers(mod)
            return ToleranceReport(*self._grade(power), self.nominal())
