"""Fixture of the detector noise models: the reference's classes on seeded CPU draws.

Run once, on the CPU, where the reference tree is present:

    python tests/golden/gen_noise_golden.py

Writes tests/golden/noise_golden.npz:
  classes                     the "<module>.<class>" names, in the order of the sd_* entries below
  sd_<module>_<class>_keys / _values / _dtypes   the state dict of the class built with ARGS below, for
                              the four classes of each of Addons.Noise, utils.Noise and
                              utils.Helper_Functions (utils.Noise.GaussianNoise has no state)
  x_real [7, 9] float32, x_cplx [7, 9] complex64   seeded inputs (generator seed 1)
  n_real, n_cplx, u_real      torch.randn_like(x_real), randn_like(x_cplx), rand_like(x_real) right after
                              torch.manual_seed(0): the draws the reference's forward consumes there
  gauss_sigma_{real,cplx}     Addons.Noise.GaussianNoise(0.25)(x) after manual_seed(0)
  gauss_snr_{real,cplx}       utils.Noise.GaussianNoise(12.0)(x) after manual_seed(0)
  uniform_real                Addons.Noise.UniformNoise(0.3)(x_real) after manual_seed(0)
  scale_{real,cplx}           sqrt(mean(x.abs() ** 2) / 10 ** (snr_db / 10)) as the reference's forward forms it (float32, on
                              the generating machine: a mean's last bit depends on the CPU's summation order)
  sigma, snr_db, a            the three parameters above
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _refimport import import_reference  # noqa: E402

ARGS = {"GaussianNoise": dict(sigma=0.25), "PoissonNoise": dict(gain=0.5, normalize=False),
        "PoissonGaussianNoise": dict(gain=2.0, sigma=0.05), "UniformNoise": dict(a=0.3)}
SNR_DB = 12.0


def main():
    ref = import_reference()
    mods = {m: ref.import_module(m) for m in ("Addons.Noise", "utils.Noise", "utils.Helper_Functions")}
    out, classes = {}, []
    for m, mod in mods.items():
        for cls, kw in ARGS.items():
            snr_form = m == "utils.Noise" and cls == "GaussianNoise"
            obj = getattr(mod, cls)(SNR_DB) if snr_form else getattr(mod, cls)(**kw)
            sd = obj.state_dict()
            tag = f"sd_{m.replace('.', '_')}_{cls}"
            out[tag + "_keys"] = np.array(list(sd.keys()), dtype="U32")
            out[tag + "_values"] = np.array([float(v) for v in sd.values()], dtype=np.float64)
            out[tag + "_dtypes"] = np.array([str(v.dtype) for v in sd.values()], dtype="U32")
            classes.append(f"{m}.{cls}")
    out["classes"] = np.array(classes, dtype="U64")

    g = torch.Generator().manual_seed(1)
    x_real = torch.randn(7, 9, generator=g)
    x_cplx = torch.view_as_complex(torch.randn(7, 9, 2, generator=g))
    out["x_real"], out["x_cplx"] = x_real.numpy(), x_cplx.numpy()

    def seeded(fn, *a):
        torch.manual_seed(0)
        return fn(*a).numpy()

    out["n_real"] = seeded(torch.randn_like, x_real)
    out["n_cplx"] = seeded(torch.randn_like, x_cplx)
    out["u_real"] = seeded(torch.rand_like, x_real)
    A, U = mods["Addons.Noise"], mods["utils.Noise"]
    out["gauss_sigma_real"] = seeded(A.GaussianNoise(ARGS["GaussianNoise"]["sigma"]), x_real)
    out["gauss_sigma_cplx"] = seeded(A.GaussianNoise(ARGS["GaussianNoise"]["sigma"]), x_cplx)
    out["gauss_snr_real"] = seeded(U.GaussianNoise(SNR_DB), x_real)
    out["gauss_snr_cplx"] = seeded(U.GaussianNoise(SNR_DB), x_cplx)
    for tag, x in (("real", x_real), ("cplx", x_cplx)):
        scale = torch.sqrt(torch.mean(x.abs() ** 2) / 10 ** (SNR_DB / 10))  # utils/Noise.py:28-32
        assert np.array_equal((x + torch.from_numpy(out["n_" + tag]) * scale).numpy(), out["gauss_snr_" + tag])
        out["scale_" + tag] = scale.numpy()
    out["uniform_real"] = seeded(A.UniformNoise(ARGS["UniformNoise"]["a"]), x_real)
    out["sigma"] = np.float64(ARGS["GaussianNoise"]["sigma"])
    out["snr_db"] = np.float64(SNR_DB)
    out["a"] = np.float64(ARGS["UniformNoise"]["a"])
    path = os.path.join(HERE, "noise_golden.npz")
    np.savez_compressed(path, **out)
    print("classes", len(classes), "wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
