"""The reference's inspection API on the HIP path vs the reference's own outputs
(tests/golden/introspect_golden.npz, made by tests/golden/gen_golden.py --only introspect):

* ASM_prop.create_kernel / Kx / Ky / shape (Props/ASM_Prop.py:138-311) -> thz_asm_transfer_function;
* RSC_prop.create_kernel / create_spatial_grid (Props/RSC_Prop.py:79-167) and CZT_prop.RS_kernel /
  build_CZT_grid (Props/CZT_Prop.py:44-118) -> thz_rs_kernel;
* ApertureElement.add_circ_aperture_to_field / add_rect_aperture_to_field / .aperture
  (Components/Aperture.py:44-123) -> thz_aperture on a unit field.

Tolerances: the transfer function evaluates the reference's fp32 angle z sqrt(k^2 - K^2) with the
same operations, so its masks must match exactly and its values must equal exp(i angle) of that
fp32 angle to the sin/cos rounding (1e-6); against the reference's own fp32 table (whose complex64
exp adds ~|angle| 1.5e-7) the bound is 1.25 x the reference's fp32-vs-fp64 error.
The RS kernel forms its phase k r with k |z| in double; the reference's fp32 k r carries an error
of up to ~|k r| 6e-8 rad (1e-4 here), so it is compared with the reference's kernel expression
evaluated in fp64 on the same fp32 meshes and z (bound: _rs_tol, from the fp32 part of its phase),
and with the fp32 output within 1.25 x the reference's own fp32 error.
"""
import json
import os

import numpy as np
import pytest
import torch

from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
from quantizationawarethzdoe_amd.Props.CZT_Prop import CZT_prop
from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop
from quantizationawarethzdoe_amd.Components.Aperture import ApertureElement

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C0 = 2.998e8
MM = 1e-3


def _rs_tol(meshx, meshy, z, freqs_ghz):
    """Relative bound of thz_rs_kernel vs the fp64 kernel expression: the fp32 part of its phase,
    k rho^2 / (r + |z|) = k (r - |z|), rounds at ~2.4e-7 of its size (three fp32 roundings), on top
    of 2e-6 for the amplitude and the double-reduced k |z| mod 2 pi."""
    lam = C0 / (np.array(freqs_ghz, dtype=np.float64) * 1e9)
    r = np.sqrt(meshx.astype(np.float64) ** 2 + meshy.astype(np.float64) ** 2 + z * z)
    return 2e-6 + (2 * np.pi / lam.min()) * float((r - abs(z)).max()) * 3e-7


@pytest.fixture(scope="module")
def G():
    with np.load(os.path.join(GOLDEN, "introspect_golden.npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "manifest.json")) as fh:
        cases = {c["name"]: c for c in json.load(fh)["introspect"]}
    return arrays, cases


def _field(c, dev):
    wl = [C0 / (g * 1e9) for g in c["f"]]
    x = torch.ones((1, len(wl), c["H"], c["W"]), dtype=torch.complex64, device=dev)
    return ElectricField(x, wavelengths=wl if len(wl) > 1 else wl[0], spacing=[c["dx"] * MM, c["dy"] * MM], device=dev)


@pytest.mark.parametrize("name", ["tf_exact_s1", "tf_approx_s15_2wl", "tf_nobl_negz", "tf_nopad"])
def test_asm_create_kernel_matches_reference(G, name, capsys):
    A, cases = G
    c = cases[name]
    dev = torch.device("cuda:0")
    prop = ASM_prop(z_distance=c["z"], do_padding=c.get("do_padding", True), padding_scale=c["s"],
                    bandlimit_kernel=c["bl"], bandlimit_type=c["t"], device=dev)
    H = prop.create_kernel(_field(c, dev))
    torch.cuda.synchronize()
    assert capsys.readouterr().out == c["print"]  # the critical-distance print, once per instance
    ref32, ref64 = A[f"{name}__H32"], A[f"{name}__H64"]
    got = H.cpu().numpy()
    assert got.shape == ref32.shape and H.dtype == torch.complex64 and H.is_cuda
    np.testing.assert_array_equal(got == 0, ref32 == 0)  # evanescent and band-limit masks
    # the reference's own fp32 angle, exactly: every op of Props/ASM_Prop.py:141-253 in numpy fp32
    f32 = np.float32
    Ph, Pw = ref32.shape[-2:]
    lam = np.array([C0 / (g * 1e9) for g in c["f"]], dtype=f32)[:, None, None]
    kx = (f32(2 * np.pi) * ((np.arange(Ph, dtype=f32) - f32(Ph // 2)) / f32(Ph))) / f32(c["dx"] * MM)
    ky = (f32(2 * np.pi) * ((np.arange(Pw, dtype=f32) - f32(Pw // 2)) / f32(Pw))) / f32(c["dy"] * MM)
    k = f32(2 * np.pi) / lam
    with np.errstate(invalid="ignore"):
        ang = f32(c["z"]) * np.sqrt(k * k - (kx[:, None] * kx[:, None] + ky[None, :] * ky[None, :]))
    exact = np.where(ref32 != 0, np.exp(1j * np.nan_to_num(ang).astype(np.float64)), 0)
    assert np.abs(got - exact).max() <= 1e-6
    # the reference's complex64 exp adds up to ~|angle| 1.5e-7 of its own on top (3e-5 at 210 rad
    # here), so against its outputs the bound is its fp32 error
    err32 = np.abs(ref32 - ref64).max()
    assert np.abs(got - ref32).max() <= 1.25 * err32 + 2e-6
    assert np.abs(got - ref64).max() <= 1.25 * err32 + 2e-6
    np.testing.assert_array_equal(prop.Kx.numpy(), A[f"{name}__Kx"])
    np.testing.assert_array_equal(prop.Ky.numpy(), A[f"{name}__Ky"])
    assert tuple(prop.shape[-2:]) == ref32.shape[-2:]
    prop.create_kernel(_field(c, dev))
    assert capsys.readouterr().out == ""


def _np_angle(H, W, s, dx, dy, lam, z, do_padding=True):
    """The reference's fp32 angle z sqrt(k^2 - K^2) on the centred padded grid, op by op in numpy fp32
    (Props/ASM_Prop.py:141-145, 244-253)."""
    f32 = np.float32
    ph, pw = (int(np.floor(s * H / 2)), int(np.floor(s * W / 2))) if do_padding else (0, 0)
    Ph, Pw = H + 2 * ph, W + 2 * pw
    kx = (f32(2 * np.pi) * ((np.arange(Ph, dtype=f32) - f32(Ph // 2)) / f32(Ph))) / f32(dx)
    ky = (f32(2 * np.pi) * ((np.arange(Pw, dtype=f32) - f32(Pw // 2)) / f32(Pw))) / f32(dy)
    k = f32(2 * np.pi) / np.asarray(lam, dtype=f32)[:, None, None]
    with np.errstate(invalid="ignore"):
        return f32(z) * np.sqrt(k * k - (kx[:, None] * kx[:, None] + ky[None, :] * ky[None, :]))


def test_asm_create_kernel_random_geometries_vs_oracle_masks():
    """create_kernel on seeded random geometries (sizes 8-160, padding 0-2.5, 1-3 wavelengths,
    |z| up to 0.4 m, every band-limit setting): the masks equal the oracle's
    (oracle.asm_transfer_function, pinned to the reference's create_kernel by the CPU tests) exactly,
    and the values equal exp(i angle) of the reference's fp32 angle to 1e-6."""
    from oracle import thz_oracle as orc
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    for _ in range(24):
        H, W = int(rng.integers(8, 161)), int(rng.integers(8, 161))
        s = float(rng.choice([0.0, 0.5, 1.0, 1.5, 2.0, 2.5]))
        nl = int(rng.integers(1, 4))
        freqs = [float(f) for f in rng.uniform(150, 450, nl)]
        dx, dy = float(rng.uniform(0.2, 1.5)) * MM, float(rng.uniform(0.2, 1.5)) * MM
        z = float(rng.uniform(-0.4, 0.4))
        bl, bt = [(True, "exact"), (True, "approx"), (False, "exact")][int(rng.integers(0, 3))]
        wl = [C0 / (f * 1e9) for f in freqs]
        f = ElectricField(torch.ones((1, nl, H, W), dtype=torch.complex64, device=dev),
                          wavelengths=wl if nl > 1 else wl[0], spacing=[dx, dy], device=dev)
        prop = ASM_prop(z_distance=z, padding_scale=s, bandlimit_kernel=bl, bandlimit_type=bt, device=dev)
        prop.check_Zc = False
        got = prop.create_kernel(f).cpu().numpy()
        lam = torch.tensor(wl, dtype=torch.float32)
        Ph, Pw = got.shape[-2:]
        ref = orc.asm_transfer_function(Ph, Pw, lam, torch.tensor(dx, dtype=torch.float32),
                                        torch.tensor(dy, dtype=torch.float32), z, bl, bt).numpy()
        np.testing.assert_array_equal(got == 0, ref == 0, err_msg=f"{H}x{W} s={s} z={z} {bl} {bt}")
        ang = _np_angle(H, W, s, dx, dy, np.array(wl, dtype=np.float32), z)
        exact = np.where(ref != 0, np.exp(1j * np.nan_to_num(ang).astype(np.float64)), 0)[None]
        assert np.abs(got - exact).max() <= 1e-6, (H, W, s, z, bl, bt)


def test_asm_kernel_is_what_forward_applies():
    """The exported table is the transfer function the propagation kernels apply on the fly:
    crop(ifft2(fft2(pad x) * ifftshift(H))) with torch's FFT on the exported H equals forward(x).
    One field on the runtime plan against an fp32 GPU FFT; tests/test_table_parity_gpu.py builds this
    comparison out (every plan family and entry point, fp64 CPU algebra, the fp32 FFT floor as bound)."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 2, 48, 48, dtype=torch.complex64, generator=g).to(dev)
    f = ElectricField(x, wavelengths=[C0 / 280e9, C0 / 320e9], spacing=[0.5 * MM, 0.5 * MM], device=dev)
    prop = ASM_prop(z_distance=0.07, padding_scale=1, bandlimit_type="exact", device=dev)
    out = prop(f).data
    Hc = prop.create_kernel(f)
    xp = torch.nn.functional.pad(x, (24, 24, 24, 24))
    ref = torch.fft.ifft2(torch.fft.fft2(xp) * torch.fft.ifftshift(Hc, dim=(-2, -1)))[..., 24:72, 24:72]
    assert float((out - ref).abs().max() / ref.abs().max()) < 1e-5


def test_rsc_create_kernel_matches_reference(G, capsys):
    A, cases = G
    c = cases["rsc_k"]
    dev = torch.device("cuda:0")
    prop = RSC_prop(z_distance=c["z"], device=dev)
    K = prop.create_kernel(_field(c, dev))
    torch.cuda.synchronize()
    assert capsys.readouterr().out == c["print"]
    np.testing.assert_array_equal(prop.meshx.cpu().numpy(), A["rsc_k__meshx"])
    np.testing.assert_array_equal(prop.meshy.cpu().numpy(), A["rsc_k__meshy"])
    got, r32, r64 = K.cpu().numpy(), A["rsc_k__K32"], A["rsc_k__K64on32"]
    assert got.shape == r32.shape
    tol = _rs_tol(A["rsc_k__meshx"], A["rsc_k__meshy"], c["z"], c["f"])
    assert np.abs(got - r64).max() <= tol * np.abs(r64).max()
    assert np.abs(got - r32).max() <= 1.25 * np.abs(r32 - r64).max() + tol * np.abs(r64).max()


def test_czt_grid_and_rs_kernel_match_reference(G):
    A, cases = G
    c = cases["czt_grid"]
    dev = torch.device("cuda:0")
    f = _field(c, dev)
    prop = CZT_prop(z_distance=c["z"], device=dev)
    g = prop.build_CZT_grid(prop.z, f.wavelengths, c["H"], c["W"], f.spacing[0], f.spacing[1], c["outH"], c["outW"],
                            c["odx"] * MM, c["ody"] * MM)
    names = ("Inmeshx", "Inmeshy", "Outmeshx", "Outmeshy", "Dm", "fx_1", "fx_2", "fy_1", "fy_2")
    for k, v in zip(names, g):
        ref = A[f"czt_grid__{k}"]
        # torch's CUDA linspace rounds a few grid points an ulp away from its CPU kernel
        np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=3e-7, atol=1e-9, err_msg=k)
    for key, which in (("F", "In"), ("F0", "Out")):
        # on the reference's own meshes, so only the kernel is compared
        mx = torch.from_numpy(A[f"czt_grid__{which}meshx"]).to(dev)
        my = torch.from_numpy(A[f"czt_grid__{which}meshy"]).to(dev)
        got = prop.RS_kernel(prop.z, mx, my, f.wavelengths).cpu().numpy()
        r32, r64 = A[f"czt_grid__{key}32"], A[f"czt_grid__{key}64on32"]
        assert got.shape == r32.shape
        tol = _rs_tol(A[f"czt_grid__{which}meshx"], A[f"czt_grid__{which}meshy"], c["z"], c["f"])
        assert np.abs(got - r64).max() <= tol * np.abs(r64).max(), key
        assert np.abs(got - r32).max() <= 1.25 * np.abs(r32 - r64).max() + tol * np.abs(r64).max(), key


def test_aperture_masks_match_reference(G):
    A, cases = G
    c = cases["ap"]
    dev = torch.device("cuda:0")
    x = torch.ones((1, 1, c["H"], c["W"]), dtype=torch.complex64, device=dev)
    f = ElectricField(x, wavelengths=C0 / 300e9, spacing=[c["dx"], c["dy"]], device=dev)
    el = ApertureElement(aperture_type="circ", aperture_size=c["circ"])
    m = el.add_circ_aperture_to_field(f, radius=c["circ"])
    assert m.dtype == torch.int64 and m.is_cuda
    np.testing.assert_array_equal(m.cpu().numpy(), A["ap__circ"])
    np.testing.assert_array_equal(el.add_rect_aperture_to_field(f).cpu().numpy(), A["ap__rect_default"])
    np.testing.assert_array_equal(el.add_rect_aperture_to_field(f, rect_width=c["rect_w"], rect_height=c["rect_h"])
                                  .cpu().numpy(), A["ap__rect_wh"])
    with pytest.raises(AttributeError):
        el.aperture
    out = el(f)
    np.testing.assert_array_equal(el.aperture.cpu().numpy(), A["ap__circ"])
    np.testing.assert_array_equal(out.data.real.cpu().numpy(), A["ap__circ"][0, 0][None, None].astype(np.float32))
