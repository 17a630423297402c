"""Full-wave validator: a 3-D Yee-grid FDTD run of a DOE relief on the fused step kernels (csrc/thz_fdtd.hip).

The scalar models of this package -- the thin-element map of ``FixDOEElement`` and the multi-slice map of
``ThickDOEElement`` -- are one-way.  This module answers whether a design survives Maxwell's equations: the relief
(one dielectric on air, a base plate under it) stands in a grid of cubic cells, periodic in x and y (the circular
convolution of ``ASM_prop(do_padding=False)``, so the two compare without edge effects) and closed by CPML along z;
a current sheet in the front air gap sends Re{A(y, x) exp(-i w0 t)} toward +z, and the running DFT at w0 gives
complex phasors on transverse planes and on one x-z and one y-z slice.  The sheet also radiates backward into the
front PML and the grid's plane wave has not exactly unit amplitude, so every result is read against an empty run
(``element=False``: same grid, no dielectric).

Conventions: axes (z, y, x); time dependence exp(-i w0 t), a wave toward +z has the phasor
exp(+i k z) as in the ASM; ``res.z`` is in metres above the top of the base plate.  The three E components are
reported where the Yee grid holds them (Ex half a cell along x, Ey along y, Ez along z from the cell's corner).
``settle_periods=None`` waits ``ramp_periods`` plus three transits of the domain, one to fill it and two of margin,
a transit being (air cells + sqrt(eps) element cells) / courant steps, rounded up to whole periods.

A worked example -- a design from ``ifta.py``, its thin-element and its thick-element z-x map, each against the
full-wave x-z slice.  The designers work in the reference's sign, exp(-i kappa h), while a
dielectric delays: exp(+i kappa h) under the ASM's exp(+i k z), which is what the grid computes.  The relief that
realises the designed phase is therefore the mirrored map (h_max - h) mod h_max; run as designed, the full-wave
field is that of the conjugate element (a lens diverges)::

    import torch
    from quantizationawarethzdoe_amd import fdtd, ifta
    from quantizationawarethzdoe_amd.Components.ThickDOE import ThickDOEElement
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop

    dev, lam, px, eps, tand, T = torch.device("cuda:0"), 1e-3, 1e-3, 2.66, 0.03, 4e-3
    W, z_focus = 32, 20e-3
    asm = ASM_prop(do_padding=False, bandlimit_kernel=False, device=dev)
    target = torch.zeros(W, W)
    target[W // 2, W // 2] = 1.0                                   # a focal spot
    h_max = lam / (eps ** 0.5 - 1)
    lut = [h_max * l / 8 for l in range(8)]
    design = ifta.IFTA(asm, [z_focus], lam, px, eps, tand, lut, (W, W)).run(target, iters=30)
    relief = torch.remainder(h_max - design.height, h_max)         # the map to fabricate
    z_list = [2e-3 * (i + 1) for i in range(15)]
    field = ElectricField(torch.ones(1, 1, W, W, dtype=torch.complex64, device=dev), wavelengths=lam, spacing=px,
                          device=dev)
    thin = asm.propagate_zx(design.as_element()(field), z_list)[:, 0, 0]
    thick_el = ThickDOEElement(relief, T, 8, [eps, tand], padding_scale=0, convention="physical", device=dev)
    thick = asm.propagate_zx(thick_el(field), z_list)[:, 0, 0]
    sim = fdtd.FDTDValidator(relief, pixel=px, wavelength=lam, material=[eps, tand], thickness=T, base=2e-3,
                             cells_per_wavelength=10, gap_back=34e-3, device=dev)
    res, empty = sim.run(row=sim.Ny // 2), sim.run(element=False, row=sim.Ny // 2)
    for name, model in (("thin", thin), ("thick", thick)):
        print(name, fdtd.compare_zx(res, empty, model, z_list))
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._call import _require_device, call, workspace

CPML_ORDER = 3
CPML_SIGMA = 0.8     # sigma_max = CPML_SIGMA (CPML_ORDER + 1) / (eta0 Delta)
CPML_ALPHA = 0.05    # alpha at the inner face over sigma_max, falling linearly to 0 at the wall
STEP_COLS = 5
COURANT_MAX = 1.0 / math.sqrt(3.0)


# -- the host tables (tests/fdtd_ref.py restates them; tests/test_fdtd_cpu.py compares the bits) ------------------
def cpml_tables(npml, courant):
    """float32 [8, npml]: (b, c) at the E planes and at the H planes of the front slab, then of the back slab."""
    l = np.arange(npml, dtype=np.float64)
    smax = CPML_SIGMA * (CPML_ORDER + 1)
    amax = CPML_ALPHA * smax
    rows = []
    for rhos in (((npml - l) / npml, (npml - l - 0.5) / npml), (l / npml, (l + 0.5) / npml)):
        for rho in rhos:
            sig = smax * rho ** CPML_ORDER
            alp = amax * (1.0 - rho)
            b = np.exp(-(sig + alp) * courant)
            rows += [b, sig / (sig + alp) * (b - 1.0)]
    return np.ascontiguousarray(np.stack(rows).astype(np.float32))


def cacb_table(eps, tand, courant, cpw):
    """float32 [10]: Ca[n], Cb[n] for n = 0 .. 4 dielectric cells of the four around an edge: eps and
    sigma = w0 eps0 eps tand at the design frequency, both averaged arithmetically."""
    f = np.arange(5, dtype=np.float64) / 4.0
    e = 1.0 + f * (float(eps) - 1.0)
    s = f * (2.0 * np.pi / cpw * float(eps) * float(tand))
    half = 0.5 * s * courant
    return np.ascontiguousarray(np.concatenate([(e - half) / (e + half), courant / (e + half)]).astype(np.float32))


def _cos_sin(periods):
    ph = 2.0 * np.pi * (periods - np.floor(periods))
    return np.cos(ph), np.sin(ph)


def step_table(n_steps, courant, cpw, ramp_periods, settle_steps, acc_steps):
    """fp64 [n_steps, 5]: the source's cos and sin times its raised-cosine ramp at t = (n + 1/2) dt (float32
    values), the DFT's cos and sin at t = (n + 1) dt, 1 where the step is accumulated."""
    n = np.arange(n_steps, dtype=np.float64)
    per = float(cpw) / float(courant)
    ts = (n + 0.5) / per
    ramp = 0.5 * (1.0 - np.cos(np.pi * np.minimum(ts / ramp_periods, 1.0))) if ramp_periods > 0 else np.ones_like(ts)
    c, s = _cos_sin(ts)
    dc, ds = _cos_sin((n + 1.0) / per)
    flag = ((n >= settle_steps) & (n < settle_steps + acc_steps)).astype(np.float64)
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(np.stack([f32(c * ramp), f32(s * ramp), dc, ds, flag], axis=1))


class FDTDResult:
    """``planes`` [n, 3, Ny, Nx], ``zx`` [3, Nz, Nx], ``zy`` [3, Nz, Ny] complex64 phasors of (Ex, Ey, Ez) (None
    where not asked for); ``z`` [Nz] float64, metres above the top of the base plate; ``plane_z`` the planes'
    positions; ``grid`` = (Nz, Ny, Nx); ``steps``; ``base_rounded`` (metres)."""

    def __init__(self, sim, planes, zx, zy, plane_k, steps):
        self.sim, self.planes, self.zx, self.zy, self.steps = sim, planes, zx, zy, steps
        self.grid = (sim.Nz, sim.Ny, sim.Nx)
        self.z = (np.arange(sim.Nz, dtype=np.float64) - sim.k_top) * sim.delta
        self.plane_z = [float(self.z[k]) for k in plane_k]
        self.base_rounded = sim.base_rounded
        self.pol = sim.pol

    def to_pixels(self, a, kind=None):
        """Cell values averaged over each pixel's ppc cells.  ``kind``: "zx" [..., Nz, Nx] -> [..., Nz, W] (the grid
        of ``propagate_zx``), "zy" [..., Nz, Ny] -> [..., Nz, H], "planes" [..., Ny, Nx] -> [..., H, W]; None: a
        4-D array is planes, ``res.zy`` itself is "zy", anything else "zx"."""
        s, p = self.sim, self.sim.ppc
        if kind is None:
            kind = "planes" if a.dim() == 4 else "zy" if a is self.zy else "zx"
        if kind not in ("planes", "zx", "zy"):
            raise ValueError(f"to_pixels: kind must be 'planes', 'zx' or 'zy'; got {kind!r}")
        if kind == "zy" or kind == "planes":
            ax = -1 if kind == "zy" else -2
            if s.H > 1:   # one row of pixels: y carries no pixel grid
                a = a.movedim(ax, -1)
                a = a.reshape(*a.shape[:-1], s.H, p).mean(-1).movedim(-1, ax)
            if kind == "zy":
                return a
        return a.reshape(*a.shape[:-1], s.W, p).mean(-1)


class FDTDState:
    """One prepared run: the workspace, the tables and the descriptor.  ``advance(n)`` enqueues n time steps on the
    current stream (no host sync; capturable in ``torch.cuda.graph``); the table holds ``n_table`` steps."""

    def __init__(self, sim, plan, incident):
        self.sim, self.plan = sim, plan
        self.tab = step_table(plan["n_table"], sim.courant, sim.cpw, plan["ramp_periods"], plan["settle_steps"],
                              plan["acc_steps"])
        self.cpml = cpml_tables(sim.npml, sim.courant)
        self.cacb = cacb_table(sim.eps, sim.tand, sim.courant, sim.cpw)
        d = self.desc = sim._desc(plan, self.tab, self.cpml, self.cacb)
        self.ws = workspace(_lib.lib().thz_fdtd_workspace_size, d, device=sim.device)
        self.enqueued = 0
        call(_lib.lib().thz_fdtd_setup, d, sim.height, incident, self.ws, self.ws.numel(), device=sim.device)
        # the tables are host arrays of this object: copied by now
        torch.cuda.current_stream(sim.device).synchronize()

    def advance(self, n):
        n = int(n)
        if n < 0 or self.enqueued + n > self.plan["n_table"]:
            raise ValueError(f"FDTD: {self.enqueued} + {n} steps for a step table of {self.plan['n_table']}")
        call(_lib.lib().thz_fdtd_run, self.desc, self.ws, self.ws.numel(), n, device=self.sim.device)
        self.enqueued += n   # a captured call counts once: the steps of its first replay
        return self

    def fields(self):
        """[6, Nz, Ny, Nx] float32: Ex, Ey, Ez, Hx, Hy, Hz (H times eta0) as they stand."""
        s = self.sim
        out = torch.empty((6, s.Nz, s.Ny, s.Nx), dtype=torch.float32, device=s.device)
        call(_lib.lib().thz_fdtd_fields, self.desc, self.ws, self.ws.numel(), out, device=s.device)
        return out

    def material(self):
        """[Nz, Ny, Nx] int32: the rasterised word nx | ny << 3 | nz << 6 of edge counts."""
        s = self.sim
        out = torch.empty((s.Nz, s.Ny, s.Nx), dtype=torch.int16, device=s.device)
        call(_lib.lib().thz_fdtd_material, self.desc, self.ws, self.ws.numel(), out, device=s.device)
        return out.to(torch.int32) & 0xffff

    def monitors(self):
        """(planes, zx, zy) complex64 phasors; None where not monitored."""
        s, p = self.sim, self.plan
        dev, c64 = s.device, torch.complex64
        planes = torch.empty((len(p["planes"]), 3, s.Ny, s.Nx), dtype=c64, device=dev) if p["planes"] else None
        zx = torch.empty((3, s.Nz, s.Nx), dtype=c64, device=dev) if p["row"] is not None else None
        zy = torch.empty((3, s.Nz, s.Ny), dtype=c64, device=dev) if p["col"] is not None else None
        call(_lib.lib().thz_fdtd_monitors, self.desc, self.ws, self.ws.numel(), planes, zx, zy, device=dev)
        return planes, zx, zy


class FDTDValidator:
    """``FDTDValidator(height_map, pixel=1e-3, wavelength=1e-3, material=[2.66, 0.03], thickness=4e-3, base=2e-3,
    cells_per_wavelength=15, gap_front=3e-3, gap_back=40e-3, npml=12, courant=0.5, polarization="x", device=...)``.

    ``height_map``: float32 [H, W] (metres), clamped to [0, thickness] and staircased to whole cells on a base plate
    of ``base`` metres (rounded to whole cells: ``base_rounded``).  A pixel must be a whole number of cells
    (``pixel`` cells_per_wavelength / wavelength an integer).  ``ny_cells``: for H = 1 only, the cells along y of
    the y-invariant problem (default one pixel; 1 is the 2-D problem exactly).  ``courant`` <= 1 / sqrt(3).  The
    kernels compute in float32; there is no CPU path."""

    def __init__(self, height_map, pixel=1e-3, wavelength=1e-3, material=(2.66, 0.03), thickness=4e-3, base=2e-3,
                 cells_per_wavelength=15, gap_front=3e-3, gap_back=40e-3, npml=12, courant=0.5, polarization="x",
                 ny_cells=None, device=None):
        who = "FDTDValidator"
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if not torch.is_tensor(height_map):
            raise TypeError(f"{who}: the height map must be a tensor")
        if self.device.type != "cuda":
            raise RuntimeError(f"{who}: the MI355X path needs a ROCm device (got device {self.device}); this "
                               "framework has no CPU compute path")
        if height_map.dtype != torch.float32:
            raise TypeError(f"{who}: the kernels compute in float32; got a {height_map.dtype} height map")
        if height_map.dim() < 2 or height_map.numel() != height_map.shape[-2] * height_map.shape[-1]:
            raise ValueError(f"{who}: one height map [H, W]; got {tuple(height_map.shape)}")
        if polarization not in ("x", "y"):
            raise ValueError(f"{who}: polarization must be 'x' or 'y'; got {polarization!r}")
        self.H, self.W = (int(v) for v in height_map.shape[-2:])
        self.pixel, self.wavelength = float(pixel), float(wavelength)
        self.eps, self.tand = float(material[0]), float(material[1])
        self.cpw, self.courant, self.npml = float(cells_per_wavelength), float(courant), int(npml)
        self.pol = 0 if polarization == "x" else 1
        self.delta = self.wavelength / self.cpw
        ratio = self.pixel / self.delta
        self.ppc = int(math.floor(ratio + 0.5))
        if self.ppc < 1 or abs(ratio - self.ppc) > 1e-9 * ratio:
            raise ValueError(f"{who}: a pixel of {self.pixel} over cells of {self.delta} is {ratio:.9g} cells: a pixel "
                             "must be a whole number of cells")
        if not 0.0 < self.courant <= COURANT_MAX:
            raise ValueError(f"{who}: courant {courant} outside (0, 1 / sqrt(3)]")
        cells = lambda v: int(math.floor(float(v) / self.delta + 0.5))
        self.thickness = float(np.float32(thickness))
        self.n_base, self.n_relief = cells(base), int(math.floor(self.thickness / self.delta + 0.5))
        self.base_rounded = self.n_base * self.delta
        self.n_front, self.n_back = cells(gap_front), cells(gap_back)
        if self.n_front < 4 or self.n_back < 2:
            raise ValueError(f"{who}: gaps of {self.n_front} and {self.n_back} cells; the front gap holds the source "
                             "(at least 4 cells), the back gap at least 2")
        self.Nx = self.W * self.ppc
        if ny_cells is not None and self.H != 1:
            raise ValueError(f"{who}: ny_cells is for a height map of one row")
        self.Ny = self.H * self.ppc if ny_cells is None else int(ny_cells)
        self.Nz = 2 * self.npml + self.n_front + self.n_base + self.n_relief + self.n_back
        self.k_elem = self.npml + self.n_front
        self.k_top = self.k_elem + self.n_base      # the plane of res.z = 0
        self.k_src = self.npml + 2
        self.steps_per_period = self.cpw / self.courant
        self.height = height_map.detach().reshape(self.H, self.W).to(self.device).contiguous()

    @classmethod
    def from_element(cls, element, **kw):
        """From a ``FixDOEElement``, a ``ThickDOEElement`` or an ``IFTAResult``: height map, material and, where the
        element carries them, pixel (``doe_dxy``) and thickness."""
        if hasattr(element, "as_element") and hasattr(element, "_material"):   # IFTAResult
            kw.setdefault("material", list(element._material))
            return cls(element.height, **kw)
        h = getattr(element, "height_map", None)
        if h is None:
            raise TypeError(f"FDTDValidator.from_element: no height map on a {type(element).__name__}")
        for name, key in (("thickness", "thickness"), ("doe_dxy", "pixel")):
            v = getattr(element, name, None)
            if v is not None and key not in kw:
                kw[key] = float(v)
        if "material" not in kw and getattr(element, "epsilon", None) is not None:
            kw["material"] = [float(element.epsilon), float(getattr(element, "tand", 0.0))]
        kw.setdefault("device", h.device)
        return cls(h.detach().to(torch.float32), **kw)

    # -- planning ------------------------------------------------------------------------------
    def transit_steps(self):
        """Steps a wavefront needs through the domain: (air cells + sqrt(eps) element cells) / courant."""
        elem = self.n_base + self.n_relief
        return ((self.Nz - elem) + math.sqrt(self.eps) * elem) / self.courant

    def default_settle_periods(self, ramp_periods):
        """``ramp_periods`` + three transits (one to fill the domain, two of margin), in whole periods."""
        return ramp_periods + math.ceil(3.0 * self.transit_steps() / self.steps_per_period)

    def k_of(self, z):
        """The plane nearest to ``z`` metres above the top of the base plate."""
        return self.k_top + int(math.floor(float(z) / self.delta + 0.5))

    def plan(self, element=True, planes=(), row=None, col=None, settle_periods=None, acc_periods=4, ramp_periods=3,
             n_table=None):
        """The run's integers (the dict ``tests/fdtd_ref.Sim`` takes).  ``planes``: metres above the base plate's
        top; ``n_table``: steps the table holds (default: settle + accumulate)."""
        per = self.steps_per_period
        acc = acc_periods * per
        if abs(acc - round(acc)) > 1e-9 * acc or round(acc) < 1:
            raise ValueError(f"FDTD: {acc_periods} periods of {per:g} steps: the DFT needs a whole number of steps "
                             "over a whole number of periods")
        if settle_periods is None:
            settle_periods = self.default_settle_periods(ramp_periods)
        settle = int(math.ceil(settle_periods * per - 1e-9))
        planes_k = [self.k_of(z) for z in planes]
        if len(planes_k) > _lib.THZ_FDTD_MAX_PLANES:
            raise ValueError(f"FDTD: {len(planes_k)} monitor planes; one run takes {_lib.THZ_FDTD_MAX_PLANES}")
        return dict(Nz=self.Nz, Ny=self.Ny, Nx=self.Nx, ppc=self.ppc, npml=self.npml, k_elem=self.k_elem,
                    n_base=self.n_base, thickness=self.thickness, delta=self.delta, courant=self.courant, cpw=self.cpw,
                    eps=self.eps, tand=self.tand, k_src=self.k_src, pol=self.pol, planes=planes_k,
                    row=None if row is None else int(row), col=None if col is None else int(col),
                    n_table=int(n_table) if n_table is not None else settle + int(round(acc)),
                    ramp_periods=float(ramp_periods), settle_steps=settle, acc_steps=int(round(acc)),
                    element=bool(element))

    def _desc(self, plan, tab, cpml, cacb):
        d = _lib.FdtdDesc(Nz=self.Nz, Ny=self.Ny, Nx=self.Nx, H=self.H, W=self.W, pixel=self.pixel, delta=self.delta,
                          courant=self.courant, npml=self.npml, k_elem=self.k_elem, n_base=self.n_base,
                          element=int(plan["element"]), thickness=self.thickness, k_src=plan["k_src"],
                          polarization=plan["pol"], n_planes=len(plan["planes"]),
                          row=-1 if plan["row"] is None else plan["row"], col=-1 if plan["col"] is None else plan["col"],
                          n_table=plan["n_table"], n_acc=plan["acc_steps"],
                          step_table=tab.ctypes.data, cpml=cpml.ctypes.data, cacb=cacb.ctypes.data)
        for q, k in enumerate(plan["planes"]):
            d.plane_k[q] = k
        return d

    def _incident(self, incident):
        if incident is None:
            return None
        if not torch.is_tensor(incident):
            raise TypeError("FDTD: the incident amplitude must be a tensor")
        _require_device(incident, "FDTD incident amplitude")
        if incident.dtype != torch.complex64:
            raise TypeError(f"FDTD: the incident amplitude must be complex64; got {incident.dtype}")
        if incident.numel() != self.H * self.W or tuple(incident.shape[-2:]) != (self.H, self.W):
            raise ValueError(f"FDTD: incident amplitude {tuple(incident.shape)} for a map of {(self.H, self.W)}")
        return incident.detach().reshape(self.H, self.W).to(self.device).resolve_conj().contiguous()

    def start(self, incident=None, **plan_kw):
        """A prepared run (``FDTDState``): rasterised, fields cleared, tables on the device."""
        return FDTDState(self, self.plan(**plan_kw), self._incident(incident))

    def run(self, incident=None, element=True, settle_periods=None, acc_periods=4, planes=(), row=None, col=None,
            ramp_periods=3):
        """Settle, accumulate the DFT over ``acc_periods`` periods, return the phasors (``FDTDResult``).
        ``incident``: complex64 [H, W] on the device (None: a plane wave of amplitude 1).  ``planes``: up to 8
        positions in metres above the base plate's top; ``row`` / ``col``: the cell row of the x-z slice and the
        cell column of the y-z slice.  ``element=False``: the normalisation run."""
        st = self.start(incident, element=element, planes=planes, row=row, col=col, settle_periods=settle_periods,
                        acc_periods=acc_periods, ramp_periods=ramp_periods)
        st.advance(st.plan["n_table"])
        p, zx, zy = st.monitors()
        return FDTDResult(self, p, zx, zy, st.plan["planes"], st.plan["n_table"])


def compare_zx(res, empty, model_zx, z_list, origin="top"):
    """|E_pol|^2 of the full-wave x-z slice against a scalar z-x map (``propagate_zx`` of a unit-amplitude field
    behind a thin or thick element, [Z, W] or [Z, 1, 1, W]) on the planes ``z_list``.

    ``origin``: where the scalar model's z = 0 lies -- ``"top"``, the plane ``thickness`` above the base plate (the
    exit plane of both element models), or ``"base"``.  The FDTD slice is averaged over each pixel's cells and
    divided by the empty run's mean intensity on the same plane.  Returns a dict: ``rel_l2`` of the two intensity
    maps, ``scale`` and ``rel_l2_scaled`` after the least-squares scale of the model (what Fresnel losses at the
    faces, which the scalar models leave out, account for), and peak position (metres) and width at the peak plane
    of both (``utils.metrics.focal_sweep``)."""
    from .utils import metrics
    sim = res.sim
    if res.zx is None or empty.zx is None:
        raise ValueError("compare_zx: both runs need the x-z slice (row=...)")
    m = model_zx.detach()
    m = m.reshape(m.shape[0], -1)
    if m.shape[0] != len(z_list) or m.shape[1] != sim.W:
        raise ValueError(f"compare_zx: a model map of {tuple(model_zx.shape)} for {len(z_list)} planes of {sim.W} pixels")
    k0 = sim.k_top + (sim.n_relief if origin == "top" else 0)
    ks = [k0 + int(math.floor(float(z) / sim.delta + 0.5)) for z in z_list]
    if min(ks) < sim.npml or max(ks) >= sim.Nz - sim.npml:
        raise ValueError("compare_zx: a plane of z_list lies outside the domain's free planes")
    idx = torch.tensor(ks, device=res.zx.device)
    f = res.to_pixels(res.zx)[res.pol].index_select(0, idx)
    e = empty.to_pixels(empty.zx)[res.pol].index_select(0, idx)
    If = (f.abs().double() ** 2) / (e.abs().double() ** 2).mean(dim=-1, keepdim=True)
    Im = (m.abs().double() ** 2).to(If.device)
    scale = float((If * Im).sum() / (Im * Im).sum())
    out = dict(rel_l2=float((If - Im).norm() / If.norm()), scale=scale,
               rel_l2_scaled=float((If - scale * Im).norm() / If.norm()))
    for name, I in (("fdtd", If), ("model", Im)):
        sw = metrics.focal_sweep(I.contiguous(), z_list, sim.pixel)
        kz = int(sw.peak.argmax())
        out[f"{name}_peak_z"] = float(z_list[kz])
        out[f"{name}_peak"] = float(sw.peak[kz])
        out[f"{name}_width"] = float(sw.width[kz])
    return out
