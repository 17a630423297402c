"""Time-domain pulses without a GPU: the restatement (tests/pulse_ref.py) and the host helpers of pulse.py against a
closed form, and the host refusals of the entries (include/thzdoe.h: thz_pulse_*)."""
import ctypes
import math

import pytest
import torch

from tests import pulse_ref


def test_closed_form():
    """A Gaussian amplitude spectrum exp(-(f - f0)^2 / (2 s^2)) delayed by tau through U_c = exp(+i 2 pi f_c tau): the
    intensity is a Gaussian about tau with t_rms = 1 / (2 sqrt(2) pi s), and the window energy is the Parseval sum
    sum_c |q_c S_c|^2 / df.  256 channels over f0 +- 6 s and 512 samples over tau +- 1.5 / s (13 t_rms, inside the period
    1 / df = 21 / s): the spectrum is cut at exp(-18) of its peak and both trapezoid rules sample a Gaussian 20 or more
    times per width, where their error is far below fp64 rounding, so what is left is rounding -- measured 9e-17 of
    t_rms for t_mean, 2e-15 for t_rms and 3e-15 for the energy, held to 1e-12."""
    from quantizationawarethzdoe_amd import pulse
    s, f0, tau = 0.1e12, 1.0e12, 0.7e-12
    f = torch.linspace(f0 - 6 * s, f0 + 6 * s, 256, dtype=torch.float64)
    S = pulse.gaussian_spectrum(pulse.C0 / f, f0, 2 * s * math.sqrt(math.log(2)))
    t = tau + torch.linspace(-1.5 / s, 1.5 / s, 512, dtype=torch.float64)
    q, dt = pulse.trapezoid_weights(f), pulse.trapezoid_weights(t)
    table = (q * S)[None, :] * torch.exp(-2j * math.pi * t[:, None] * f[None, :])
    U = torch.exp(2j * math.pi * f * tau)[None, :, None, None]
    W, _, _, t_mean, t_rms = (float(m) for m in pulse_ref.maps(table, t, dt, U)[0].flatten())
    want = 1 / (2 * math.sqrt(2) * math.pi * s)
    assert abs(t_mean - tau) <= 1e-12 * want and abs(t_rms - want) <= 1e-12 * want
    parseval = float(((q * S.abs()) ** 2).sum() / (f[1] - f[0]))
    assert abs(W - parseval) <= 1e-12 * parseval


PTR = ctypes.c_void_p(256)  # a non-null, aligned pointer that a refused call never follows


@pytest.mark.parametrize("change, code, text", [
    (dict(C=0), "THZ_E_UNSUPPORTED", "C = 0"), (dict(C=65), "THZ_E_UNSUPPORTED", "C = 65"),
    (dict(T=0), "THZ_E_UNSUPPORTED", "T = 0"), (dict(T=4097), "THZ_E_UNSUPPORTED", "T = 4097"),
    (dict(H=65536, W=32768), "THZ_E_UNSUPPORTED", "H W"), (dict(B=0), "THZ_E_ARG", "bad shape"),
    (dict(table=None), "THZ_E_ARG", "null pointer"), (dict(table=ctypes.c_void_p(260)), "THZ_E_ARG", "8-byte"),
])
def test_host_refusals(change, code, text):
    """every refusal is made on the host, before any device call, and reports through thz_last_error"""
    from quantizationawarethzdoe_amd import _lib
    L = _lib.lib()
    cfg = {**dict(B=1, C=4, T=8, H=8, W=8, table=PTR), **change}
    table = cfg.pop("table")
    d = ctypes.byref(_lib.PulseDesc(**cfg))
    for status in (L.thz_pulse_synthesize(d, PTR, table, PTR, None), L.thz_pulse_adjoint(d, PTR, table, PTR, None),
                   L.thz_pulse_maps(d, PTR, table, PTR, PTR, PTR, None),
                   L.thz_pulse_maps_backward(d, PTR, table, PTR, PTR, PTR, PTR, PTR, None)):
        assert status == getattr(_lib, code) and text in L.thz_last_error().decode()
    assert L.thz_pulse_maps(None, PTR, PTR, PTR, PTR, PTR, None) == _lib.THZ_E_ARG
