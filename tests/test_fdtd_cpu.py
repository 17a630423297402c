"""The FDTD validator without a GPU: the numpy restatement (tests/fdtd_ref.py) pinned to physics, and the host
logic of csrc/thz_fdtd.hip and quantizationawarethzdoe_amd/fdtd.py.

Dispersion and slab run the 1 x 1 transverse problem (periodic: the 1-D problem) in fp64.  The bounds: a CPML
reflection plus settle residue below 1 % of the amplitude at 20 cells per wavelength (a condition on the absorber
and on the default settle time), and second-order convergence of the slab's transmission (the error falls by at
least 3 from 20 to 40 cells per wavelength; the scheme promises 4)."""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import fdtd_ref as fr

EPS = 2.66
S = 0.5
NPML = 12


def _plan_1d(cpw, n_plate, tand, element):
    """One wavelength of air, the plate, one wavelength of air between the slabs; the settle time by the formula
    of fdtd.FDTDValidator.default_settle_periods (ramp + three transits, in whole periods)."""
    Nz = 2 * NPML + cpw + n_plate + cpw
    per = int(cpw / S)
    transit = ((Nz - n_plate) + math.sqrt(EPS) * n_plate) / S
    settle = (3 + math.ceil(3.0 * transit / per)) * per
    acc = 2 * per
    return dict(Nz=Nz, Ny=1, Nx=1, ppc=1, npml=NPML, k_elem=NPML + cpw, n_base=n_plate, thickness=0.0, delta=1.0 / cpw,
                courant=S, cpw=cpw, eps=EPS, tand=tand, k_src=NPML + 2, pol=0, planes=[Nz - NPML - 3], row=0, col=None,
                n_table=settle + acc, ramp_periods=3.0, settle_steps=settle, acc_steps=acc, element=element)


@functools.lru_cache(maxsize=None)
def _run_1d(cpw, n_plate, tand, element):
    plan = _plan_1d(cpw, n_plate, tand, element)
    sim = fr.Sim(plan, np.zeros((1, 1), np.float32), None, np.float64).run(plan["n_table"])
    planes, zx, _ = sim.monitors()
    return plan, planes[0, 0, 0, 0], zx[0, :, 0]


@pytest.mark.parametrize("cpw", [20, 40])
def test_dispersion_and_flatness_of_a_plane_wave(cpw):
    plan, _, e = _run_1d(cpw, 0, 0.0, False)
    line = e[plan["k_src"] + 2: plan["Nz"] - NPML]
    amp = np.abs(line)
    flat = float((amp.max() - amp.min()) / (2.0 * amp.mean()))
    phase = np.angle(line[1:] / line[:-1])
    kd = fr.yee_wavenumber(cpw, S)
    dev = float(np.abs(phase - kd).max())
    print(f"fdtd-dispersion cpw {cpw}: |E| ripple {flat:.3e} of the amplitude, phase per cell off k~ Delta = {kd:.6f} by "
          f"{dev:.3e}")
    assert flat < 0.01 and dev < 0.01 * kd
    assert kd > 2.0 * np.pi / cpw  # the grid's wave is slower than light


@pytest.mark.parametrize("tand", [0.0, 0.03])
def test_slab_transmission_is_the_airy_value_to_second_order(tand):
    err = {}
    for cpw in (20, 40):
        n_plate = 2 * cpw  # two wavelengths, faces on cell boundaries
        _, with_plate, _ = _run_1d(cpw, n_plate, tand, True)
        _, without, _ = _run_1d(cpw, n_plate, tand, False)
        want = fr.airy_transmission(cpw, S, EPS, tand, n_plate)
        err[cpw] = abs(with_plate / without - want)
        print(f"fdtd-slab tand {tand} cpw {cpw}: t = {with_plate / without:.5f}, Airy {want:.5f}, error {err[cpw]:.3e}")
    assert err[20] < 0.02 and err[40] * 3.0 <= err[20]


def _brute_raster(h, ppc, Nz, Ny, Nx, k_elem, n_base, T, delta):
    H, W = h.shape
    out = np.zeros((Nz, Ny, Nx), np.uint16)

    def solid(k, j, i):
        if k < 0:
            return 0
        v = float(min(max(np.float32(h[0 if H == 1 else (j % Ny) // ppc, (i % Nx) // ppc]), np.float32(0)),
                      np.float32(T)))
        return int(k_elem <= k < k_elem + n_base + math.floor(v / delta + 0.5))

    for k in range(Nz):
        for j in range(Ny):
            for i in range(Nx):
                nx = solid(k, j, i) + solid(k - 1, j, i) + solid(k, j - 1, i) + solid(k - 1, j - 1, i)
                ny = solid(k, j, i) + solid(k - 1, j, i) + solid(k, j, i - 1) + solid(k - 1, j, i - 1)
                nz = solid(k, j, i) + solid(k, j - 1, i) + solid(k, j, i - 1) + solid(k, j - 1, i - 1)
                out[k, j, i] = nx | (ny << 3) | (nz << 6)
    return out


@pytest.mark.parametrize("ppc", [1, 5])
def test_rasteriser_against_a_brute_force_loop(ppc):
    delta, ncell = 0.125e-3, 6
    T = ncell * delta
    faces = [np.float32(m * delta) for m in range(ncell + 1)]
    vals = [0.0, -1e-4, T, 2 * T, 0.4 * delta, 0.6 * delta, 2.5 * delta] + faces
    h = np.resize(np.array(vals, np.float32), (3, 5))
    Nz, Ny, Nx = 14, 3 * ppc, 5 * ppc
    got = fr.rasterise(h, ppc, Nz, Ny, Nx, 3, 2, T, delta)
    assert np.array_equal(got, _brute_raster(h, ppc, Nz, Ny, Nx, 3, 2, T, delta))
    cells = fr.relief_cells(np.array(faces, np.float32), T, delta)
    assert cells.tolist() == list(range(ncell + 1))
    assert fr.relief_cells(np.array([-1.0, 2 * T], np.float32), T, delta).tolist() == [0, ncell]
    assert not fr.rasterise(h, ppc, Nz, Ny, Nx, 3, 2, T, delta, element=False).any()
    # one row, Ny = 1: the y neighbour is the cell itself (the 2-D problem)
    row = fr.rasterise(h[:1], ppc, Nz, 1, Nx, 3, 2, T, delta)
    assert np.array_equal(row, _brute_raster(h[:1], ppc, Nz, 1, Nx, 3, 2, T, delta))


def _desc(**over):
    from quantizationawarethzdoe_amd import _lib, fdtd
    tab = fdtd.step_table(40, 0.5, 8.0, 3.0, 8, 32)
    cpml, cacb = fdtd.cpml_tables(4, 0.5), fdtd.cacb_table(EPS, 0.03, 0.5, 8.0)
    kw = dict(Nz=40, Ny=8, Nx=16, H=1, W=2, pixel=1e-3, delta=0.125e-3, courant=0.5, npml=4, k_elem=12, n_base=4,
              element=1, thickness=1e-3, k_src=6, polarization=0, n_planes=1, row=0, col=-1, n_table=40, n_acc=32,
              step_table=tab.ctypes.data, cpml=cpml.ctypes.data, cacb=cacb.ctypes.data)
    planes = over.pop("planes", [30])
    kw.update(over)
    d = _lib.FdtdDesc(**kw)
    for q, k in enumerate(planes):
        d.plane_k[q] = k
    return d, (tab, cpml, cacb)


def test_host_refusals_without_a_gpu():
    from quantizationawarethzdoe_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    d, keep = _desc()
    assert L.thz_fdtd_workspace_size(ctypes.byref(d), ctypes.byref(n)) == _lib.THZ_OK and n.value > 6 * 4 * 40 * 8 * 16
    need = n.value
    for over, code, word in ((dict(delta=0.13e-3), _lib.THZ_E_UNSUPPORTED, b"whole number of cells"),
                             (dict(courant=0.6), _lib.THZ_E_ARG, b"Courant"),
                             (dict(planes=[37]), _lib.THZ_E_ARG, b"inside a PML slab"),
                             (dict(planes=[3]), _lib.THZ_E_ARG, b"inside a PML slab"),
                             (dict(k_src=2), _lib.THZ_E_ARG, b"source plane"),
                             (dict(Nx=17), _lib.THZ_E_ARG, b"pixels"),
                             (dict(H=2), _lib.THZ_E_ARG, b"pixels"),
                             (dict(n_planes=9), _lib.THZ_E_ARG, b"monitor planes"),
                             (dict(k_elem=30), _lib.THZ_E_ARG, b"reaches into a PML slab"),
                             (dict(row=8), _lib.THZ_E_ARG, b"slice row")):
        bad, keep2 = _desc(**over)
        assert L.thz_fdtd_workspace_size(ctypes.byref(bad), ctypes.byref(n)) == code, over
        assert word in L.thz_last_error(), (over, L.thz_last_error())
    null, ws = ctypes.c_void_p(0), ctypes.c_void_p(256 * 1024)
    assert L.thz_fdtd_run(ctypes.byref(d), ws, need - 1, 1, null) == _lib.THZ_E_WORKSPACE
    assert L.thz_fdtd_run(ctypes.byref(d), null, need, 1, null) == _lib.THZ_E_WORKSPACE
    assert L.thz_fdtd_run(ctypes.byref(d), ctypes.c_void_p(256 * 1024 + 16), need, 1, null) == _lib.THZ_E_ARG
    assert L.thz_fdtd_setup(ctypes.byref(d), null, null, ws, need, null) == _lib.THZ_E_ARG
    assert L.thz_fdtd_setup(ctypes.byref(d), ctypes.c_void_p(4096), null, ws, need - 1, null) == _lib.THZ_E_WORKSPACE
    assert L.thz_fdtd_monitors(ctypes.byref(d), ws, need, null, ws, null, null) == _lib.THZ_E_ARG
    assert L.thz_fdtd_fields(ctypes.byref(d), ws, need, null, null) == _lib.THZ_E_ARG
    assert L.thz_fdtd_workspace_size(None, ctypes.byref(n)) == _lib.THZ_E_ARG


def test_python_refusals_without_a_gpu():
    import torch
    from quantizationawarethzdoe_amd import fdtd
    h = torch.zeros(4, 4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        fdtd.FDTDValidator(h, device="cpu")
    with pytest.raises(TypeError, match="float32"):
        fdtd.FDTDValidator(h.double(), device="cuda:0")
    with pytest.raises(ValueError, match="whole number of cells"):
        fdtd.FDTDValidator(h, pixel=1e-3, wavelength=1.1e-3, device="cuda:0")
    with pytest.raises(ValueError, match="courant"):
        fdtd.FDTDValidator(h, courant=0.6, device="cuda:0")


@pytest.mark.parametrize("cpw,courant,npml", [(8.0, 0.5, 8), (15.0, 0.5, 12), (12.0, 0.4, 10)])
def test_host_tables_are_bit_equal_to_the_restatement(cpw, courant, npml):
    from quantizationawarethzdoe_amd import fdtd
    a, b = fdtd.cpml_tables(npml, courant), fr.cpml_tables(npml, courant)
    assert a.dtype == np.float32 and a.shape == (8, npml) and a.tobytes() == b.tobytes()
    per = cpw / courant
    settle, acc = int(7 * per), int(round(2 * per))
    a, b = fdtd.step_table(settle + acc + 5, courant, cpw, 3.0, settle, acc), fr.step_table(settle + acc + 5, courant,
                                                                                         cpw, 3.0, settle, acc)
    assert a.dtype == np.float64 and a.shape == (settle + acc + 5, 5) and a.tobytes() == b.tobytes()
    assert a[:, 4].sum() == acc and a[settle - 1, 4] == 0 and a[settle, 4] == 1
    assert (fdtd.cacb_table(EPS, 0.03, courant, cpw).tobytes() == fr.cacb_table(EPS, 0.03, courant, cpw).tobytes())
    ca = fdtd.cacb_table(EPS, 0.0, courant, cpw)
    assert ca[0] == 1.0 and ca[5] == np.float32(courant) and ca[4] == 1.0 and ca[9] == np.float32(courant / EPS)
    assert fdtd.CPML_ORDER == fr.CPML_ORDER and fdtd.CPML_SIGMA == fr.CPML_SIGMA and fdtd.CPML_ALPHA == fr.CPML_ALPHA
