"""The four noise formulas of the reference (Addons/Noise.py:27, 58-61, 87-89, 112; utils/Noise.py:28-32)
restated on GIVEN draws and a GIVEN Poisson sample, in torch ops on the inputs' device and dtype, in
the reference's operation order.  tests/test_noise_cpu.py pins it to the reference's own outputs
(tests/golden/noise_golden.npz) bit for bit; tests/test_noise_gpu.py then holds the kernels to it on
the kernels' exported draws."""
import math

import torch


def _t(v, like):
    """A scalar parameter as the reference holds it: a 0-dim float32 tensor."""
    return torch.tensor(float(v), dtype=torch.float32, device=like.device)


def gauss(x, n, sigma):
    """x + n * sigma; sigma a float or a 0-dim / [1] float32 tensor (the SNR form's scale)."""
    s = sigma.reshape(()) if torch.is_tensor(sigma) else _t(sigma, x)
    return x + n * s


def snr_scale(x, snr_db):
    """sqrt(mean(|x|^2) / 10^(snr_db / 10)) in the input's precision (utils/Noise.py:28-31)."""
    return torch.sqrt(torch.mean(x.abs() ** 2) / (10 ** (snr_db / 10)))


def snr_scale_fp64(x, snr_db):
    """The same value from fp64 arithmetic on the fp32 data, as a Python float."""
    return math.sqrt(float(torch.mean(x.to(torch.complex128 if x.is_complex() else torch.float64).abs() ** 2))
                     / (10 ** (snr_db / 10)))


def uniform(x, u, a):
    return x + (u - 0.5) * 2 * _t(a, x)


def poisson(x, sample, gain, normalize):
    """sample = the Poisson draw of x / gain."""
    return sample * _t(gain, x) if normalize else sample


def poisson_gauss(x, sample, n, gain, sigma):
    y = sample * _t(gain, x)
    y = y + n * _t(sigma, x)
    return y
