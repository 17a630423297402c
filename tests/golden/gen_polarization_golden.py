"""Fixture of the polarization analysis: the reference's PolarizationAnalyser on a seeded field.

Run once, on the CPU, where the reference tree is present:

    python tests/golden/gen_polarization_golden.py

Writes tests/golden/polarization_golden.npz:
  x            [3, 2, 24, 20] complex64, torch.view_as_complex(torch.randn(3, 2, 24, 20, 2, seed 0))
  wavelengths  [1e-3, 0.9e-3] (float32), spacing 1 mm
  {I,Q,U,V,A,B,theta,h}{32,64}   [2, 24, 20]: the reference's polarization_state / polarization_ellipse
               per wavelength on the complex64 data and on the same values cast to complex128
  err_{I,Q,U,V}      the reference's own fp32 error against its fp64 values, max over pixels of
                     |x32 - x64| / I64, per wavelength
  err_{A,B}          max |x32 - x64| per wavelength
  err_theta          max |exp(2i theta32) - exp(2i theta64)| per wavelength (the doubled-angle phasor
                     the test compares on); err_theta_raw the plain max |theta32 - theta64|
  h_mismatch         pixels where h32 != h64, min_abs_v_eps = min |V64 + eps|
  dcp_jones          sum V / sum I of the reference's VectorialGuassian_beam (64 x 64, 4 mm waists,
                     jones_vector [1, 1 - 1j], 220 and 330 GHz, 1 mm) per wavelength: pins the sign of
                     the degree of circular polarization the propagated beam is compared with
"""
import os
import sys

import matplotlib

matplotlib.use("Agg")

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _refimport import import_reference  # noqa: E402


def main():
    ref = import_reference()
    PA = ref.import_module("Addons.Polarization").PolarizationAnalyser
    g = torch.Generator().manual_seed(0)
    x = torch.view_as_complex(torch.randn(3, 2, 24, 20, 2, generator=g))
    wavelengths = [1e-3, 0.9e-3]
    field = ref.ElectricField(data=x, wavelengths=wavelengths, spacing=1e-3, device=torch.device("cpu"))
    pa = PA(field, device=torch.device("cpu"))
    names = ("I", "Q", "U", "V", "A", "B", "theta", "h")
    out = {n + p: [] for n in names for p in ("32", "64")}
    for wl in field.wavelengths:
        d32 = field._get_data_for_wavelength(wl)
        for tag, d in (("32", d32), ("64", d32.to(torch.complex128))):
            vals = pa.polarization_state(d, numpy=True) + pa.polarization_ellipse(d, numpy=True)
            for n, v in zip(names, vals):
                out[n + tag].append(np.asarray(v))
    out = {k: np.stack(v) for k, v in out.items()}
    assert all(np.isfinite(v).all() for v in out.values()), "a reference value is not finite"
    assert out["I32"].dtype == np.float32 and out["I64"].dtype == np.float64
    ax = (1, 2)
    for n in "IQUV":
        out["err_" + n] = (np.abs(out[n + "32"] - out[n + "64"]) / out["I64"]).max(axis=ax)
    for n in "AB":
        out["err_" + n] = np.abs(out[n + "32"] - out[n + "64"]).max(axis=ax)
    out["err_theta"] = np.abs(np.exp(2j * out["theta32"].astype(np.float64)) - np.exp(2j * out["theta64"])).max(axis=ax)
    out["err_theta_raw"] = np.abs(out["theta32"] - out["theta64"]).max(axis=ax)
    out["h_mismatch"] = (out["h32"] != out["h64"]).sum(axis=ax)
    out["min_abs_v_eps"] = np.abs(out["V64"] + 1e-6).min(axis=ax)

    c0 = 299792458.0
    beam_wl = [c0 / 220e9, c0 / 330e9]
    beam = ref.GB.VectorialGuassian_beam(height=64, width=64, beam_waist_x=4e-3, beam_waist_y=4e-3,
                                         jones_vector=[1, 1 - 1j], wavelengths=beam_wl, spacing=1e-3,
                                         device=torch.device("cpu"))()
    pb = PA(beam, device=torch.device("cpu"))
    dcp = []
    for wl in beam.wavelengths:
        I, _, _, V = pb.polarization_state(beam._get_data_for_wavelength(wl), numpy=True)
        dcp.append(float(V.sum() / I.sum()))
    out["dcp_jones"] = np.array(dcp)
    out["beam_wavelengths"] = np.array(beam_wl)

    out["x"] = x.numpy()
    out["wavelengths"] = field.wavelengths.numpy()
    out["spacing"] = np.float32(1e-3)
    path = os.path.join(HERE, "polarization_golden.npz")
    np.savez_compressed(path, **out)
    for k in ("err_I", "err_Q", "err_U", "err_V", "err_A", "err_B", "err_theta", "err_theta_raw", "h_mismatch",
              "min_abs_v_eps", "dcp_jones"):
        print(f"{k:14s}", out[k])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
