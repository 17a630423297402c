"""Detector noise models with the reference's names and constructor arguments (Addons/Noise.py:4-112),
computed by the fused noise kernel (``optics.add_noise`` / ``optics.detect``, thz_noise.hip).

``sigma``, ``gain``, ``normalize`` and ``a`` are non-trainable ``nn.Parameter``s as in the reference,
so state dicts interchange.  ``forward(x, rng=None)`` is the reference's forward on a measurement;
``measure(field, rng=None)`` is the same model on |field|^2 in one pass from the complex field.
``rng = (state, stream)`` as in ``optics.add_noise``; without it the state comes from torch's
generator.  The Poisson kinds have a zero gradient (torch's derivative of ``poisson``).
"""
import torch

from quantizationawarethzdoe_amd import optics


class _NoiseModel(torch.nn.Module):
    """Host copies of the scalar parameters for the kernel's descriptor.  A parameter that lives on
    the host is read directly; one moved to a device is read once per value (keyed on its storage
    and version), so repeated calls do not sync.  The first call after ``.to(device)``,
    ``load_state_dict`` or an in-place update of such a parameter does sync: it must not be the
    call a graph captures (make one warm-up call first, or leave the module on the host)."""
    kind = None

    def _host(self, name):
        p = getattr(self, name)
        if p.device.type == "cpu":
            return p.item()
        key = (p.data_ptr(), p._version)
        cache = self.__dict__.setdefault("_host_cache", {})
        if cache.get(name, (None, None))[0] != key:
            cache[name] = (key, p.item())
        return cache[name][1]

    def _params(self):
        return {n: self._host(n) for n in ("sigma", "a", "gain", "normalize") if n in self._parameters}

    def forward(self, x, rng=None):
        return optics.add_noise(x, self.kind, rng=rng, **self._params())

    def measure(self, field, rng=None):
        """The noisy intensity of a complex field (tensor or ElectricField): forward(|field|^2), fused."""
        return optics.detect(field, self.kind, rng=rng, **self._params())


class GaussianNoise(_NoiseModel):
    r"""y = x + eps, eps ~ N(0, sigma^2) (:27); complex x gets complex noise of total variance sigma^2."""
    kind = "gauss"

    def __init__(self, sigma=0.1):
        super().__init__()
        self.sigma = torch.nn.Parameter(torch.tensor(sigma), requires_grad=False)


class PoissonNoise(_NoiseModel):
    r"""y = P(x / gain), times gain if ``normalize`` (:58-61)."""
    kind = "poisson"

    def __init__(self, gain=1.0, normalize=True):
        super().__init__()
        self.normalize = torch.nn.Parameter(torch.tensor(normalize), requires_grad=False)
        self.gain = torch.nn.Parameter(torch.tensor(gain), requires_grad=False)


class PoissonGaussianNoise(_NoiseModel):
    r"""y = gain z + eps, z ~ P(x / gain), eps ~ N(0, sigma^2) (:87-89)."""
    kind = "poisson_gauss"

    def __init__(self, gain=1.0, sigma=0.1):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.tensor(gain), requires_grad=False)
        self.sigma = torch.nn.Parameter(torch.tensor(sigma), requires_grad=False)


class UniformNoise(_NoiseModel):
    r"""y = x + eps, eps ~ U(-a, a) (:112).  Real measurements only."""
    kind = "uniform"

    def __init__(self, a=0.1):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(a), requires_grad=False)
