"""The Hankel propagator without a GPU: the host-built table against scipy, the model's algebra at the library's
zeros, and the host refusals of the entry points (include/thzdoe.h: thz_hankel_*)."""
import ctypes

import numpy as np
import pytest

from tests import hankel_ref


def _host_table(N):
    from quantizationawarethzdoe_amd import _lib
    T, w, zeros = np.empty((N, N), np.float32), np.empty(N, np.float32), np.empty(N + 1)
    assert _lib.lib().thz_hankel_table_host(N, T.ctypes.data, w.ctypes.data, zeros.ctypes.data) == _lib.THZ_OK
    return T, w, zeros


@pytest.mark.parametrize("N", [1, 2, 33, 256])
def test_table_against_scipy(N):
    """zeros to 2 fp64 ulp; T (and w) to 1 fp32 ulp of the fp32 rounding of the scipy table"""
    T, w, zeros = _host_table(N)
    T64, w64, z64 = hankel_ref.scipy_table(N)
    assert np.all(np.abs(zeros - z64) <= 2 * np.spacing(z64))
    for got, ref in ((T, T64.astype(np.float32)), (w, w64.astype(np.float32))):
        assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))
    assert np.array_equal(T, T.T)


def test_model_in_fp64_at_the_library_zeros():
    """T T = I to 10 x 3.1e-11 (N = 256) and the Gaussian's spectrum to 1e-12 of its peak (N = 512, r_max = 0.1 m,
    w0 = 8 mm).  Both bounds are figures of the fp64 algebra, so they are held on the table as the library forms it
    before its one rounding: the model in fp64 at the exported zeros.

    The exported fp32 T and w are then held to what one rounding u = 2^-24 of every entry allows.  Rows of T have
    unit norm (T T = I), so |(T + dT)(T + dT) - T T| <= (2 u + u^2) max_ij sum_k |T_ik| |T_kj| <= 2 u + u^2 by
    Cauchy-Schwarz; the spectrum, a sum of products T_mn w_n f_n divided by w_m, moves by at most 3 u + O(u^2) of
    sum_n |T_mn| w_n f_n / w_m per entry (T, w_n and w_m rounded once each).  Measured: 1.1e-8 and 2.5e-8 of the
    peak."""
    u = 2.0 ** -24
    T32, _, zeros = _host_table(256)
    T, _ = hankel_ref.table_at(zeros)
    assert np.abs(T @ T - np.eye(256)).max() <= 10 * 3.1e-11
    assert np.abs(T32.astype(np.float64) @ T32.astype(np.float64) - np.eye(256)).max() <= 2 * u + u * u + 10 * 3.1e-11
    T32, w32, zeros = (a.astype(np.float64) for a in _host_table(512))
    T, w = hankel_ref.table_at(zeros)
    r_max, w0 = 0.1, 8e-3
    r, kappa = zeros[:-1] * r_max / zeros[-1], zeros[:-1] / r_max
    f, scale = np.exp(-r ** 2 / w0 ** 2), r_max ** 2 / zeros[-1]
    exact = (w0 ** 2 / 2) * np.exp(-kappa ** 2 * w0 ** 2 / 4)
    assert np.abs((T @ (w * f)) / w * scale - exact).max() <= 1e-12 * exact.max()
    allowed = 3.1 * u * (np.abs(T) @ (w * f)) / w * scale + 1e-12 * exact.max()
    assert np.all(np.abs((T32 @ (w32 * f)) / w32 * scale - exact) <= allowed)


GOOD = dict(N=64, keep=64, Z=2, B=1, C=1, r_max=0.1)
PTR = ctypes.c_void_p(256)  # a non-null, aligned pointer that a refused call never follows


@pytest.mark.parametrize("change, ptrs, text", [
    (dict(N=0), None, "N = 0"), (dict(N=8193, keep=8193), None, "N = 8193"),
    (dict(keep=0), None, "keep = 0"), (dict(keep=65), None, "keep = 65"),
    (dict(Z=0), None, "bad shape"), (dict(B=0), None, "bad shape"), (dict(C=0), None, "bad shape"),
    (dict(r_max=0.0), None, "r_max"), (dict(r_max=-1.0), None, "r_max"),
    (dict(lam=0.0), None, "wavelength"), (dict(lam=None), None, "null wavelengths"), (dict(z=None), None, "null z"),
    ({}, (None, PTR, PTR), "null pointer"), ({}, (PTR, None, PTR), "null pointer"),
    ({}, (PTR, PTR, None), "workspace"), ({}, (PTR, PTR, PTR), "workspace"),
])
def test_host_refusals(change, ptrs, text):
    """every refusal is made on the host, before any device call, and reports through thz_last_error; a short or
    null workspace answers THZ_E_WORKSPACE, the library's code for it, everything else THZ_E_ARG"""
    from quantizationawarethzdoe_amd import _lib
    L = _lib.lib()
    cfg = {**GOOD, "lam": 1e-3, "z": (0.05, 0.1), **change}
    lam, z = cfg.pop("lam"), cfg.pop("z")
    wl, zs = _lib.float_array([lam or 0.0]), _lib.float_array(z or ())
    fptr = ctypes.POINTER(ctypes.c_float)
    d = _lib.HankelDesc(**cfg, wavelengths=ctypes.cast(wl, fptr) if lam is not None else None,
                        z=ctypes.cast(zs, fptr) if z is not None else None)
    want = _lib.THZ_E_WORKSPACE if text == "workspace" else _lib.THZ_E_ARG
    for fn in (L.thz_hankel_forward, L.thz_hankel_adjoint):
        a, b, ws = ptrs or (PTR, PTR, PTR)
        assert fn(ctypes.byref(d), a, b, ws, 1, None) == want
        assert text in L.thz_last_error().decode()
    if ptrs is None and z is not None:  # the size entry reads no z
        assert L.thz_hankel_workspace_size(ctypes.byref(d), ctypes.byref(ctypes.c_size_t(0))) == _lib.THZ_E_ARG
        assert text in L.thz_last_error().decode()
    if ptrs is None:
        assert L.thz_hankel_transfer_function(ctypes.byref(d), PTR, None) == _lib.THZ_E_ARG
    assert L.thz_hankel_forward(None, PTR, PTR, PTR, 1, None) == _lib.THZ_E_ARG
    assert L.thz_hankel_table_host(0, PTR, PTR, PTR) == _lib.THZ_E_ARG
    assert L.thz_hankel_table(8193, PTR, PTR, PTR, None) == _lib.THZ_E_ARG
