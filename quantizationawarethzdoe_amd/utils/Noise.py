"""The reference's utils/Noise.py (:4-116): the noise models of ``Addons.Noise``, except that
``GaussianNoise(SNR_dB)`` scales the noise to the signal power,
y = x + n sqrt(mean(|x|^2) / 10^(SNR_dB / 10)) (:28-32).  The scale is computed on the device
(thz_signal_scale) and the gradient includes its dependence on x (thz_snr_noise_backward)."""
import torch

from quantizationawarethzdoe_amd import optics
from quantizationawarethzdoe_amd.Addons.Noise import PoissonGaussianNoise, PoissonNoise, UniformNoise  # noqa: F401


class GaussianNoise(torch.nn.Module):
    def __init__(self, SNR_dB):
        super().__init__()
        self.SNR = SNR_dB

    def forward(self, x, rng=None):
        return optics.add_noise(x, "gauss", snr_db=self.SNR, rng=rng)

    def measure(self, field, rng=None):
        """forward(|field|^2).  The scale needs the mean of the whole intensity before the first pixel
        is written, so the intensity is formed first; the noise pass is the same kernel."""
        data = field if torch.is_tensor(field) else field.data
        return self.forward(data.abs() ** 2, rng=rng)
