"""Numpy restatement of the Yee-grid FDTD validator (csrc/thz_fdtd.hip, quantizationawarethzdoe_amd/fdtd.py).

The same scheme, one function per pass, every cell's expression in the operation order of the kernels (which
compile with contraction off), so ``dtype=np.float32`` gives the kernels' bits and ``dtype=np.float64`` the truth
the parity tests compare against.  Both runs use the same float32 coefficient tables: the difference between them
is the rounding of the field arithmetic alone.

Model.  Cubic cells of side Delta, axes (z, y, x), x and y periodic, z closed by a wall behind
``npml`` cells of CPML on each side.  Units: c = 1, lengths in cells, H times eta0, dt = ``courant`` cells.  Yee
placement of index (k, j, i):  Ex (i+1/2, j, k), Ey (i, j+1/2, k), Ez (i, j, k+1/2), Hx (i, j+1/2, k+1/2),
Hy (i+1/2, j, k+1/2), Hz (i+1/2, j+1/2, k).  Step n (from 0): H^{n+1/2} from E^n, then E^{n+1} from H^{n+1/2}, the
current sheet at t = (n + 1/2) dt, the running DFT of E^{n+1} at t = (n + 1) dt.  Time dependence exp(-i w t), so a
wave toward +z has the phasor exp(+i k z), as the angular-spectrum propagators have it.

The CPML recipe (kappa = 1), written here once.  With rho the depth into a slab over the slab's thickness (0 at
the inner face, 1 at the wall), in units of 1 / Delta with eta0 absorbed:
  sigma(rho) = sigma_max rho^3,  sigma_max = 0.8 * 4         (0.8 (m + 1) / (eta0 Delta), m = 3)
  alpha(rho) = 0.05 sigma_max (1 - rho)
  b = exp(-(sigma + alpha) courant),  c = sigma / (sigma + alpha) (b - 1)
evaluated at the E planes (rho = l / npml from the inner face) and at the H planes (half a cell further), fp64,
rounded to float32.  psi <- b psi + c d for the raw z-difference d, and d + psi replaces d in the update.
"""
import numpy as np

CPML_ORDER = 3
CPML_SIGMA = 0.8
CPML_ALPHA = 0.05
STEP_COLS = 5


def cpml_tables(npml, courant):
    """float32 [8, npml]: (bE, cE, bH, cH) of the front slab (plane l), then of the back slab (plane Nz - npml + l)."""
    l = np.arange(npml, dtype=np.float64)
    smax = CPML_SIGMA * (CPML_ORDER + 1)
    amax = CPML_ALPHA * smax

    def bc(rho):
        sig = smax * rho ** CPML_ORDER
        alp = amax * (1.0 - rho)
        b = np.exp(-(sig + alp) * courant)
        return b, sig / (sig + alp) * (b - 1.0)

    rows = []
    for rho_e, rho_h in (((npml - l) / npml, (npml - l - 0.5) / npml), (l / npml, (l + 0.5) / npml)):
        rows += [*bc(rho_e), *bc(rho_h)]
    return np.stack(rows).astype(np.float32)


def cacb_table(eps, tand, courant, cpw):
    """float32 [10]: Ca[n], Cb[n] for n = 0 .. 4 dielectric cells of the four around an edge (arithmetic mean of
    eps and of sigma = w0 eps0 eps tand, in these units w0 eps tand with w0 = 2 pi / cpw)."""
    f = np.arange(5, dtype=np.float64) / 4.0
    e = 1.0 + f * (float(eps) - 1.0)
    s = f * (2.0 * np.pi / cpw * float(eps) * float(tand))
    half = 0.5 * s * courant
    return np.concatenate([(e - half) / (e + half), courant / (e + half)]).astype(np.float32)


def _cos_sin(periods):
    """cos and sin of 2 pi ``periods``, the argument reduced to one period first."""
    ph = 2.0 * np.pi * (periods - np.floor(periods))
    return np.cos(ph), np.sin(ph)


def step_table(n_steps, courant, cpw, ramp_periods, settle_steps, acc_steps):
    """fp64 [n_steps, 5]: source cos and sin times the raised-cosine ramp at t = (n + 1/2) dt (float32 values), the
    DFT's cos and sin at t = (n + 1) dt, and 1 where the step is accumulated."""
    n = np.arange(n_steps, dtype=np.float64)
    per = float(cpw) / float(courant)  # steps per period
    ts = (n + 0.5) / per
    ramp = 0.5 * (1.0 - np.cos(np.pi * np.minimum(ts / ramp_periods, 1.0))) if ramp_periods > 0 else np.ones_like(ts)
    c, s = _cos_sin(ts)
    dc, ds = _cos_sin((n + 1.0) / per)
    flag = ((n >= settle_steps) & (n < settle_steps + acc_steps)).astype(np.float64)
    return np.stack([(c * ramp).astype(np.float32).astype(np.float64), (s * ramp).astype(np.float32).astype(np.float64),
                     dc, ds, flag], axis=1)


def relief_cells(h, thickness, delta):
    """Whole cells of relief per pixel: floor(clamp(h, 0, T) / Delta + 1/2), the clamp in float32."""
    hc = np.minimum(np.maximum(np.asarray(h, np.float32), np.float32(0)), np.float32(thickness))
    return np.floor(hc.astype(np.float64) / float(delta) + 0.5).astype(np.int64)


def cell_mask(h, ppc, Nz, Ny, Nx, k_elem, n_base, thickness, delta, element=True):
    """bool [Nz, Ny, Nx]: the dielectric cells."""
    h = np.asarray(h, np.float32)
    H, W = h.shape
    top = k_elem + n_base + relief_cells(h, thickness, delta)
    rows = np.zeros(Ny, np.int64) if H == 1 else np.arange(Ny) // ppc
    top = top[rows][:, np.arange(Nx) // ppc]
    k = np.arange(Nz)[:, None, None]
    return (k >= k_elem) & (k < top[None]) & bool(element)


def rasterise(h, ppc, Nz, Ny, Nx, k_elem, n_base, thickness, delta, element=True):
    """uint16 [Nz, Ny, Nx]: nx | ny << 3 | nz << 6, how many of the four cells around the cell's Ex / Ey / Ez edge
    are dielectric (x, y periodic; below plane 0 air)."""
    m = cell_mask(h, ppc, Nz, Ny, Nx, k_elem, n_base, thickness, delta, element).astype(np.int64)
    zm = np.concatenate([np.zeros_like(m[:1]), m[:-1]])
    ym, xm = (lambda a: np.roll(a, 1, 1)), (lambda a: np.roll(a, 1, 2))
    nx = m + zm + ym(m) + ym(zm)
    ny = m + zm + xm(m) + xm(zm)
    nz = m + ym(m) + xm(m) + xm(ym(m))
    return (nx | (ny << 3) | (nz << 6)).astype(np.uint16)


class Sim:
    """One run.  ``plan``: dict(Nz, Ny, Nx, ppc, npml, k_elem, n_base, thickness, delta, courant, cpw, eps, tand,
    k_src, pol (0 x, 1 y), planes (k indices), row, col (or None), n_table, ramp_periods, settle_steps, acc_steps,
    element).  ``incident``: complex64 [H, W] or None."""

    def __init__(self, plan, height, incident=None, dtype=np.float64):
        p = self.p = dict(plan)
        self.dt = dtype
        Nz, Ny, Nx = p["Nz"], p["Ny"], p["Nx"]
        self.mat = rasterise(height, p["ppc"], Nz, Ny, Nx, p["k_elem"], p["n_base"], p["thickness"], p["delta"],
                             p.get("element", True))
        cacb = cacb_table(p["eps"], p["tand"], p["courant"], p["cpw"]).astype(dtype)
        m = self.mat.astype(np.int64)
        self.ca = [cacb[:5][(m >> s) & 7] for s in (0, 3, 6)]
        self.cb = [cacb[5:][(m >> s) & 7] for s in (0, 3, 6)]
        self.cpml = cpml_tables(p["npml"], p["courant"]).astype(dtype)
        self.table = step_table(p["n_table"], p["courant"], p["cpw"], p["ramp_periods"], p["settle_steps"],
                                p["acc_steps"])
        H, W = np.asarray(height).shape
        A = np.ones((H, W), np.complex64) if incident is None else np.asarray(incident, np.complex64)
        rows = np.zeros(Ny, np.int64) if H == 1 else np.arange(Ny) // p["ppc"]
        A = A[rows][:, np.arange(Nx) // p["ppc"]]
        self.Ar, self.Ai = A.real.astype(dtype), A.imag.astype(dtype)
        self.S = dtype(np.float32(p["courant"]))
        self.amp = dtype(np.float32(2.0) * np.float32(p["courant"]))
        z = lambda: np.zeros((Nz, Ny, Nx), dtype)
        self.ex, self.ey, self.ez, self.hx, self.hy, self.hz = z(), z(), z(), z(), z(), z()
        ps = lambda: np.zeros((2, p["npml"], Ny, Nx), dtype)
        self.psi_hx, self.psi_hy, self.psi_ex, self.psi_ey = ps(), ps(), ps(), ps()
        self.n = 0
        self.acc_p = np.zeros((len(p["planes"]), 3, Ny, Nx), np.complex128)
        self.acc_zx = np.zeros((3, Nz, Nx), np.complex128)
        self.acc_zy = np.zeros((3, Nz, Ny), np.complex128)

    def _slabs(self):
        npml, Nz = self.p["npml"], self.p["Nz"]
        return ((0, slice(0, npml)), (1, slice(Nz - npml, Nz)))

    def step_h(self):
        ex, ey, ez, S = self.ex, self.ey, self.ez, self.S
        up = lambda a: np.concatenate([a[1:], np.zeros_like(a[:1])])  # plane k + 1; beyond the last: the wall
        yp, xp = (lambda a: np.roll(a, -1, 1)), (lambda a: np.roll(a, -1, 2))
        dzey, dzex = up(ey) - ey, up(ex) - ex
        for s, sl in self._slabs():
            b, c = self.cpml[s * 4 + 2][:, None, None], self.cpml[s * 4 + 3][:, None, None]
            self.psi_hx[s] = b * self.psi_hx[s] + c * dzey[sl]
            self.psi_hy[s] = b * self.psi_hy[s] + c * dzex[sl]
            dzey[sl] = dzey[sl] + self.psi_hx[s]
            dzex[sl] = dzex[sl] + self.psi_hy[s]
        self.hx = self.hx - S * ((yp(ez) - ez) - dzey)
        self.hy = self.hy - S * (dzex - (xp(ez) - ez))
        self.hz = self.hz - S * ((xp(ey) - ey) - (yp(ex) - ex))

    def step_e(self):
        p, hx, hy, hz, dt = self.p, self.hx, self.hy, self.hz, self.dt
        row = self.table[self.n] if self.n < len(self.table) else np.zeros(STEP_COLS)
        down = lambda a: np.concatenate([np.zeros_like(a[:1]), a[:-1]])
        ym, xm = (lambda a: np.roll(a, 1, 1)), (lambda a: np.roll(a, 1, 2))
        dzhy, dzhx = hy - down(hy), hx - down(hx)
        for s, sl in self._slabs():
            b, c = self.cpml[s * 4 + 0][:, None, None], self.cpml[s * 4 + 1][:, None, None]
            self.psi_ex[s] = b * self.psi_ex[s] + c * dzhy[sl]
            self.psi_ey[s] = b * self.psi_ey[s] + c * dzhx[sl]
            dzhy[sl] = dzhy[sl] + self.psi_ex[s]
            dzhx[sl] = dzhx[sl] + self.psi_ey[s]
        ex = self.ca[0] * self.ex + self.cb[0] * ((hz - ym(hz)) - dzhy)
        ey = self.ca[1] * self.ey + self.cb[1] * (dzhx - (hz - xm(hz)))
        ex[0], ey[0] = self.ex[0], self.ey[0]  # plane 0 is the wall
        self.ez = self.ca[2] * self.ez + self.cb[2] * ((hy - xm(hy)) - (hx - ym(hx)))
        v = self.amp * (self.Ar * dt(row[0]) + self.Ai * dt(row[1]))
        tgt = ex if p["pol"] == 0 else ey
        tgt[p["k_src"]] = tgt[p["k_src"]] + v
        self.ex, self.ey = ex, ey
        if row[4] != 0.0:
            dc, ds = row[2], row[3]
            E = (self.ex, self.ey, self.ez)
            acc = lambda a, v: (a.real + v.astype(np.float64) * dc) + 1j * (a.imag + v.astype(np.float64) * ds)
            for q, k in enumerate(p["planes"]):
                for c in range(3):
                    self.acc_p[q, c] = acc(self.acc_p[q, c], E[c][k])
            if p.get("row") is not None:
                for c in range(3):
                    self.acc_zx[c] = acc(self.acc_zx[c], E[c][:, p["row"], :])
            if p.get("col") is not None:
                for c in range(3):
                    self.acc_zy[c] = acc(self.acc_zy[c], E[c][:, :, p["col"]])
        self.n += 1

    def run(self, n_steps):
        for _ in range(n_steps):
            self.step_h()
            self.step_e()
        return self

    def fields(self):
        return np.stack([self.ex, self.ey, self.ez, self.hx, self.hy, self.hz])

    def monitors(self):
        """(planes, zx, zy) phasors, complex128: the sums times 2 / acc_steps."""
        s = 2.0 / self.p["acc_steps"]
        return self.acc_p * s, self.acc_zx * s, self.acc_zy * s


def yee_wavenumber(cpw, courant):
    """k~ Delta of the Yee relation sin(w dt / 2) / dt = sin(k~ Delta / 2) / Delta in vacuum."""
    return 2.0 * np.arcsin(np.sin(np.pi * courant / cpw) / courant)


def yee_wavenumber_medium(cpw, courant, eps, tand):
    """The complex k~ Delta of the scheme inside the uniform lossy dielectric.  A wave exp(i (k~ z - w t)) in the H
    update gives Hy = S sin(k~ / 2) / sin(w dt / 2) Ex, and in the E update with the full cell's (Ca, Cb)
    sin^2(k~ / 2) = (e^{-i w dt / 2} - Ca e^{+i w dt / 2}) 2 i sin(w dt / 2) / (4 S Cb), which is the vacuum relation
    for Ca = 1, Cb = S."""
    w = 2.0 * np.pi * courant / cpw  # w dt
    e, s = float(eps), 2.0 * np.pi / cpw * float(eps) * float(tand)
    half = 0.5 * s * courant
    ca, cb = (e - half) / (e + half), courant / (e + half)
    s2 = (np.exp(-0.5j * w) - ca * np.exp(0.5j * w)) * (2j * np.sin(0.5 * w)) / (4.0 * courant * cb)
    return 2.0 * np.arcsin(np.sqrt(s2 + 0j))


def yee_impedance_ratio(cpw, courant, kd):
    """Hy / Ex of a wave of numerical wavenumber ``kd`` (k~ Delta): S sin(k~ / 2) / sin(w dt / 2), the admittance the
    interface conditions of the grid see (1 in the continuum's vacuum)."""
    return courant * np.sin(0.5 * kd) / np.sin(np.pi * courant / cpw)


def airy_transmission(cpw, courant, eps, tand, n_cells):
    """Transmitted over incident phasor (same plane behind the plate, plate over no plate) of a plate of ``n_cells``
    whole cells, from the numerical wavenumbers and admittances: t = t12 t21 e^{i k1 d} / (1 - r21^2 e^{2 i k1 d})
    over e^{i k0 d}."""
    k0, k1 = yee_wavenumber(cpw, courant), yee_wavenumber_medium(cpw, courant, eps, tand)
    y0, y1 = yee_impedance_ratio(cpw, courant, k0), yee_impedance_ratio(cpw, courant, k1)
    r = (y0 - y1) / (y0 + y1)
    t = (1.0 - r * r) * np.exp(1j * k1 * n_cells) / (1.0 - r * r * np.exp(2j * k1 * n_cells))
    return t / np.exp(1j * k0 * n_cells)
