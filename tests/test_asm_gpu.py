"""ASM parity on the GPU: HIP kernels (via the ASM_prop mirror and the C-ABI) vs the
reference-generated golden fixtures and the pinned CPU oracle.

Tolerance (complex fp32, stated in BASELINE.json north_star): rel-L2 against the fp64
golden <= max(1e-4, 1.25 x the reference's own fp32 error on that case) -- the reference's
fp32 error is 9e-6 .. 1.4e-4 on these cases (manifest "rel32vs64"; the unlimited-band case
is the 1.4e-4 one) -- and <= 2 x the reference's own fp32 error + 2e-5 against the
reference's fp32 output.
"""
import numpy as np
import pytest
import torch

from oracle import thz_oracle as orc
from tests.golden_io import GOLDEN, arrays, manifest, rel_l2, spacing, wavelengths
from tests.gpu_util import dev as _dev

pytestmark = pytest.mark.gpu
M = manifest()
C0 = 2.998e8


def _prop_cls():
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    return ElectricField, ASM_prop


def _run_case(case, x, grad=None):
    EF, ASM = _prop_cls()
    dev = _dev()
    wl = [C0 / (f * 1e9) for f in case["f"]]
    data = torch.from_numpy(x).to(dev)
    if grad is not None:
        data.requires_grad_(True)
    field = EF(data, wavelengths=wl if len(wl) > 1 else wl[0], spacing=[case["dx"] * 1e-3, case["dy"] * 1e-3],
               device=dev)
    prop = ASM(z_distance=case["z"], do_padding=case.get("do_padding", True),
               do_unpad_after_pad=case.get("unpad", True), padding_scale=case["s"], bandlimit_kernel=case["bl"],
               bandlimit_type=case["t"], device=dev)
    out = prop(field)
    gin = None
    if grad is not None:
        out.data.backward(torch.from_numpy(grad).to(dev))
        gin = data.grad.detach().cpu().numpy()
    return out.data.detach().cpu().numpy(), gin


@pytest.mark.parametrize("case", M["asm"], ids=[c["name"] for c in M["asm"]])
def test_asm_forward_vs_golden(case):
    A = arrays("asm")
    k = case["name"]
    out, _ = _run_case(case, A[f"{k}__in"])
    assert out.shape == A[f"{k}__out64"].shape
    e64 = rel_l2(out, A[f"{k}__out64"])
    e32 = rel_l2(out, A[f"{k}__out32"])
    assert e64 <= max(1e-4, 1.25 * case["rel32vs64"]), (e64, case["rel32vs64"])
    assert e32 <= 2 * case["rel32vs64"] + 2e-5, (e32, case["rel32vs64"])


@pytest.mark.parametrize("case", [c for c in M["asm"] if c["grad"]], ids=lambda c: c["name"])
def test_asm_backward_vs_reference_autograd(case):
    A = arrays("asm")
    k = case["name"]
    _, gin = _run_case(case, A[f"{k}__in"], grad=A[f"{k}__gout"])
    assert rel_l2(gin, A[f"{k}__gin64"]) <= 1e-4


def test_asm_cfg1_checksum():
    """cfg1: 1024^2 ones-field, z=0.2 m, dx=0.5 mm, 300 GHz, s=1 (P=2048), exact."""
    c = M["asm_cfg1"]
    G = arrays("asm_cfg1")
    out, _ = _run_case(c, np.ones((1, 1, 1024, 1024), np.complex64))
    e = float(np.sum(np.abs(out.astype(np.complex128)) ** 2))
    assert abs(e - c["energy64"]) / c["energy64"] < 2e-5
    assert rel_l2(out[0, 0, ::32, ::32], G["cfg1__sub64"]) <= 1e-4
    assert rel_l2(out[0, 0, 512, :], G["cfg1__row512_64"]) <= 1e-4


def test_asm_multi_z_matches_oracle():
    EF, ASM = _prop_cls()
    dev = _dev()
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((2, 2, 80, 72)) + 1j * rng.standard_normal((2, 2, 80, 72))).astype(np.complex64)
    wl = [C0 / 250e9, C0 / 330e9]
    zs = [0.02, 0.07, -0.03, 0.15, 0.3]
    field = EF(torch.from_numpy(x).to(dev), wavelengths=wl, spacing=[0.5e-3, 0.6e-3], device=dev)
    prop = ASM(z_distance=zs[0], padding_scale=1.5, bandlimit_type="approx", device=dev)
    planes = prop.propagate_planes(field, zs).cpu().numpy()
    assert planes.shape == (5, 2, 2, 80, 72)
    for k, z in enumerate(zs):
        ref = orc.asm_forward(torch.from_numpy(x).to(torch.complex128), wavelengths([250, 330], True),
                              spacing(0.5, 0.6, True), z, 1.5, bandlimit_type="approx").numpy()
        # the reference op sequence in fp32 sets the floor (phase z*k ~ 2e3 rad at z = 0.3 m)
        ref32 = orc.asm_forward(torch.from_numpy(x), wavelengths([250, 330]), spacing(0.5, 0.6), z, 1.5,
                                bandlimit_type="approx").numpy()
        floor = rel_l2(ref32, ref)
        assert rel_l2(planes[k], ref) <= max(1e-4, 1.5 * floor), (k, z, floor)


@pytest.mark.parametrize("n", list(range(1, 65)) + [67, 100, 101, 128, 201, 243, 250, 251, 300, 303, 500, 1000,
                                                    1024, 2048, 3000, 4096, 6144, 8192, 12288, 16384])
def test_fft_rows_vs_numpy(n):
    from quantizationawarethzdoe_amd.propagation import fft_rows
    rng = np.random.default_rng(n)
    rows = 3
    x = (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))).astype(np.complex64)
    xt = torch.from_numpy(x).to(_dev())
    f = fft_rows(xt).cpu().numpy()
    b = fft_rows(xt, inverse=True).cpu().numpy()
    ref_f = np.fft.fft(x.astype(np.complex128), axis=-1)
    ref_b = np.fft.ifft(x.astype(np.complex128), axis=-1) * n
    tol = 2e-6 * max(1.0, np.log2(n))
    assert rel_l2(f, ref_f) <= tol
    assert rel_l2(b, ref_b) <= tol


def test_asm_full_size_properties():
    """cfg2 geometry (4096^2 Gaussian, P=8192, dx=0.25 mm, 300 GHz): one plane vs the fp32 oracle,
    plus linearity and the adjoint identity <A x, y> = <x, A^H y> at full size."""
    EF, ASM = _prop_cls()
    dev = _dev()
    N = 4096
    dx = 0.25e-3
    lam = C0 / 300e9
    xs = (torch.arange(N, dtype=torch.float32) - N / 2) * dx
    X, Y = torch.meshgrid(xs, xs, indexing="ij")
    g = torch.exp(-(X ** 2 + Y ** 2) / (50e-3) ** 2).to(torch.complex64)[None, None]
    prop = ASM(z_distance=0.05, padding_scale=1, device=dev)
    f1 = EF(g.to(dev), wavelengths=lam, spacing=dx, device=dev)
    o1 = prop(f1).data
    with torch.no_grad():
        torch.set_num_threads(max(1, torch.get_num_threads()))
        ref = orc.asm_forward(g, torch.tensor([lam], dtype=torch.float32), torch.tensor([dx, dx]), 0.05, 1)
    assert rel_l2(o1.cpu().numpy(), ref.numpy()) <= 1e-4
    gen = torch.Generator(device=dev).manual_seed(0)
    r = torch.randn(1, 1, N, N, dtype=torch.complex64, device=dev, generator=gen)
    o2 = prop(EF(r, wavelengths=lam, spacing=dx, device=dev)).data
    o3 = prop(EF(2.0 * g.to(dev) - 1j * r, wavelengths=lam, spacing=dx, device=dev)).data
    lin = float((o3 - (2.0 * o1 - 1j * o2)).norm() / o3.norm())
    assert lin <= 1e-5
    from quantizationawarethzdoe_amd.propagation import asm_apply
    y = torch.randn(1, 1, 1, N, N, dtype=torch.complex64, device=dev, generator=gen)
    Ax = asm_apply(r, [lam], [dx, dx], [0.05], N // 2, N // 2, True, 1)
    AHy = asm_apply(y, [lam], [dx, dx], [0.05], N // 2, N // 2, True, 1, adjoint=True)
    lhs = torch.vdot(y.reshape(-1).to(torch.complex128), Ax.reshape(-1).to(torch.complex128))
    rhs = torch.vdot(AHy.reshape(-1).to(torch.complex128), r.reshape(-1).to(torch.complex128))
    assert abs(complex(lhs - rhs)) / abs(complex(lhs)) <= 1e-4
    e_in = float((r.abs().double() ** 2).sum())
    e_out = float((o2.abs().double() ** 2).sum())
    assert e_out <= e_in * (1 + 1e-5)


def _cfg2_input(dev):
    """The bench.py cfg2 input: a 4096^2 Gaussian beam (w 50 mm, 300 GHz, dx 0.25 mm) made by the
    device kernel (LightSource/Gaussian_beam.py:88-160)."""
    from quantizationawarethzdoe_amd.optics import gaussian_beam
    lam = float(torch.tensor(C0 / 300e9, dtype=torch.float32))
    return gaussian_beam(4096, 4096, 0.25e-3, 0.25e-3, [lam], [50e-3], [50e-3], device=dev), lam


def test_asm_cfg2_timed_path_vs_oracle():
    """The headline kernels over several z-chunks: asm_cols<8192> with a 32-plane z-chunk (spectrum
    reused across z in registers, per-z kept-row bisection), the kfull / kparts z-range split of
    the last dispatch round, and a tail chunk of 8 planes.  40 planes over 20-120 mm (the bench
    sweep's range, experiment_extend_depth_of_focus.ipynb:229); the first and last plane of each
    chunk vs the fp32 oracle (<= 1e-4 rel-L2), and the sweep's end planes (z = 20 mm and 120 mm
    exactly) vs the REFERENCE's own fp64 output signature (tests/golden/cfg2_check.npz: energy,
    E[::64, ::64], row 2048; <= 1e-4, the reference's own fp32 error there is 4e-6 / 2.3e-5)."""
    from quantizationawarethzdoe_amd.propagation import asm_apply, asm_plan_info
    dev = _dev()
    x, lam = _cfg2_input(dev)
    sp = [float(torch.tensor(0.25e-3, dtype=torch.float32))] * 2
    zs = [float(v) for v in torch.linspace(20e-3, 120e-3, 40, dtype=torch.float64)]
    ncols, zc = asm_plan_info(1, 1, 4096, 4096, 2048, 2048, True, 1, [lam], sp, zs, 32)
    assert zc == 32 and ncols < 8192
    out = asm_apply(x, [lam], sp, zs, 2048, 2048, True, 1, z_chunk=32)
    assert out.shape == (40, 1, 1, 4096, 4096)
    check = [0, 31, 32, 39]
    got = {k: out[k, 0, 0].cpu().numpy() for k in check}
    del out
    xc = x.cpu()
    with torch.no_grad():
        refs = orc.asm_forward_planes(xc, torch.tensor([lam], dtype=torch.float32), torch.tensor(sp),
                                      [zs[k] for k in check], 1)
        for k, (_, ref) in zip(check, refs):
            e = rel_l2(got[k], ref[0, 0].numpy())
            assert e <= 1e-4, (k, zs[k], e)
    G = np.load(f"{GOLDEN}/cfg2_check.npz")
    for k, p in ((0, 0), (39, 1)):
        g = got[k].astype(np.complex128)
        assert rel_l2(g[::64, ::64], G[f"p{p}__sub64"]) <= 1e-4
        assert rel_l2(g[2048], G[f"p{p}__row64"]) <= 1e-4
        assert abs(float(np.sum(np.abs(g) ** 2)) - float(G[f"p{p}__energy64"])) <= 1e-5 * float(G[f"p{p}__energy64"])


def test_asm_cfg2_default_chunk_vs_oracle():
    """The bench's own launch: 64 planes of the cfg2 sweep at the library's default z_chunk (one
    64-plane column pass and one row pass); planes 0, 31, 32 and 63 vs the fp32 oracle (<= 1e-4)."""
    from quantizationawarethzdoe_amd.propagation import asm_apply, asm_plan_info
    dev = _dev()
    x, lam = _cfg2_input(dev)
    sp = [float(torch.tensor(0.25e-3, dtype=torch.float32))] * 2
    zs = [float(v) for v in torch.linspace(20e-3, 120e-3, 64, dtype=torch.float64)]
    ncols, zc = asm_plan_info(1, 1, 4096, 4096, 2048, 2048, True, 1, [lam], sp, zs)
    assert zc == 64
    out = asm_apply(x, [lam], sp, zs, 2048, 2048, True, 1)
    check = [0, 31, 32, 63]
    got = {k: out[k, 0, 0].cpu().numpy() for k in check}
    del out
    with torch.no_grad():
        refs = orc.asm_forward_planes(x.cpu(), torch.tensor([lam], dtype=torch.float32), torch.tensor(sp),
                                      [zs[k] for k in check], 1)
        for k, (_, ref) in zip(check, refs):
            e = rel_l2(got[k], ref[0, 0].numpy())
            assert e <= 1e-4, (k, zs[k], e)


def test_asm_middle_crop_row_pass_bit_identical_to_the_generic_one():
    """cfg2's row pass, asm_rows_inv_mid<8192> (the middle-half crop of padding scale 1 as a
    compile-time window, so the last stage's outputs outside it and their store tests fold away),
    against the generic asm_rows_inv<8192> that the same call runs when the padded plane is kept
    (unpad=False: every output column stored), cropped afterwards: BIT-identical planes.  Round 4
    found 10 % of the elements an ulp apart: with a * b + c * d left to contraction the compiler kept
    a different product rounded in the two instantiations (the same FMA count, another pairing; ISA
    diff of the two kernels).  The complex products are now written as explicit fmaf
    (csrc/thz_fft.hpp cmul / cmulc), so every instantiation rounds each butterfly the same way.
    Both calls run the same K1 and K2 (the crop changes only which rows K2 stores)."""
    from quantizationawarethzdoe_amd.propagation import asm_apply
    dev = _dev()
    x, lam = _cfg2_input(dev)
    sp = [float(torch.tensor(0.25e-3, dtype=torch.float32))] * 2
    zs = [0.02, 0.07]
    mid = asm_apply(x, [lam], sp, zs, 2048, 2048, True, 1)
    full = asm_apply(x, [lam], sp, zs, 2048, 2048, False, 1)
    assert full.shape[-2:] == (8192, 8192)
    assert torch.equal(mid, full[..., 2048:6144, 2048:6144])


@pytest.mark.parametrize("geom", ["p300", "p500", "p2048"])
def test_asm_device_resident_planes_bit_identical(geom):
    """thz_asm_desc.z_dev (ABI 6: the kernels read the plane distances from device memory, so a
    captured graph replays with planes rewritten between replays) gives the same planes, bit for
    bit, as the host z: the same fp32 values reach the same arithmetic; the band is sized for any z
    (the evanescent bound), and its extra columns carry zeros through the column pass.  Forward over
    three planes and the Z-summing adjoint; the compile-time 300-point plan (P = 300), the runtime
    mixed-radix plan (P = 500, the extended-DOF geometry) and a power of two."""
    from quantizationawarethzdoe_amd.propagation import asm_apply
    dev = _dev()
    H, pad, dx = {"p300": (100, 100, 1e-3), "p500": (100, 200, 1e-3), "p2048": (1024, 512, 0.5e-3)}[geom]
    g = torch.Generator(device=dev).manual_seed(8)
    x = torch.randn(1, 1, H, H, dtype=torch.complex64, device=dev, generator=g)
    lam = [float(torch.tensor(C0 / 300e9, dtype=torch.float32))]
    zs = [0.052, 0.061, 0.089]
    zd = torch.tensor(zs, dtype=torch.float32, device=dev)
    a = asm_apply(x, lam, [dx, dx], zs, pad, pad, True, 1)
    b = asm_apply(x, lam, [dx, dx], zs, pad, pad, True, 1, z_dev=zd)
    assert torch.equal(a, b)
    ga = asm_apply(a, lam, [dx, dx], zs, pad, pad, True, 1, adjoint=True)
    gb = asm_apply(a, lam, [dx, dx], zs, pad, pad, True, 1, adjoint=True, z_dev=zd)
    assert torch.equal(ga, gb)
    # the planes really come from the device buffer: other values there, other planes
    zd2 = torch.tensor([0.06, 0.07, 0.08], dtype=torch.float32, device=dev)
    c = asm_apply(x, lam, [dx, dx], zs, pad, pad, True, 1, z_dev=zd2)
    d = asm_apply(x, lam, [dx, dx], [0.06, 0.07, 0.08], pad, pad, True, 1)
    assert torch.equal(c, d)


def test_asm_p2048_64_planes_every_plane_vs_oracle():
    """asm_cols<2048> over 64 planes in two full 32-plane chunks (the kparts split of each chunk's
    last dispatch round included): every plane vs the fp64 oracle, <= max(1e-4, 1.5 x the oracle's
    own fp32 error on that plane)."""
    from quantizationawarethzdoe_amd.propagation import asm_apply
    dev = _dev()
    rng = np.random.default_rng(21)
    x = (rng.standard_normal((1, 1, 1024, 1024)) + 1j * rng.standard_normal((1, 1, 1024, 1024))).astype(np.complex64)
    lam = wavelengths([300])
    sp = spacing(0.5, 0.5)
    zs = [float(v) for v in torch.linspace(0.01, 0.25, 64, dtype=torch.float64)]
    out = asm_apply(torch.from_numpy(x).to(dev), [float(lam[0])], [float(sp[0]), float(sp[1])], zs, 512, 512, True,
                    1, z_chunk=32).cpu().numpy()
    xt = torch.from_numpy(x)
    with torch.no_grad():
        r64 = orc.asm_forward_planes(xt.to(torch.complex128), lam.double(), sp.double(), zs, 1)
        r32 = orc.asm_forward_planes(xt, lam, sp, zs, 1)
        for k, ((_, a), (_, b)) in enumerate(zip(r64, r32)):
            a = a.numpy()
            floor = rel_l2(b.numpy(), a)
            e = rel_l2(out[k], a)
            assert e <= max(1e-4, 1.5 * floor), (k, zs[k], e, floor)


def test_asm_p1024_z_chunk_beyond_workgroup():
    """P = 1024 runs 64-thread column workgroups; a z_chunk of 100 planes must still find every
    plane's kept-row bound (the per-z bisection is strided over the workgroup)."""
    from quantizationawarethzdoe_amd.propagation import asm_apply, asm_plan_info
    dev = _dev()
    rng = np.random.default_rng(22)
    x = (rng.standard_normal((1, 1, 512, 512)) + 1j * rng.standard_normal((1, 1, 512, 512))).astype(np.complex64)
    lam = wavelengths([300])
    sp = spacing(0.5, 0.5)
    zs = [float(v) for v in torch.linspace(0.01, 0.3, 100, dtype=torch.float64)]
    lamf, spf = [float(lam[0])], [float(sp[0]), float(sp[1])]
    assert asm_plan_info(1, 1, 512, 512, 256, 256, True, 1, lamf, spf, zs, 100)[1] == 100
    out = asm_apply(torch.from_numpy(x).to(dev), lamf, spf, zs, 256, 256, True, 1, z_chunk=100).cpu().numpy()
    check = [0, 63, 64, 99]
    xt = torch.from_numpy(x)
    with torch.no_grad():
        r64 = orc.asm_forward_planes(xt.to(torch.complex128), lam.double(), sp.double(), [zs[k] for k in check], 1)
        r32 = orc.asm_forward_planes(xt, lam, sp, [zs[k] for k in check], 1)
        for k, (_, a), (_, b) in zip(check, r64, r32):
            a = a.numpy()
            floor = rel_l2(b.numpy(), a)
            assert rel_l2(out[k], a) <= max(1e-4, 1.5 * floor), (k, zs[k], floor)


@pytest.mark.parametrize("zs,bl,H,W", [([0.02, 0.07, -0.03, 0.15, 0.3], "approx", 100, 100),
                                      ([0.1], "exact", 100, 100),
                                      ([0.05, 0.2, 0.1], "exact", 100, 80),
                                      ([0.1], "approx", 80, 100)],
                         ids=["5z_approx", "1z_exact", "rows240_cols300", "rows300_cols240"])
def test_asm_p300_mixed_radix_vs_oracle(zs, bl, H, W):
    """P = 300 (the cfg4 / cfg5 grid) runs the compile-time mixed-radix kernels and the per-
    (wavelength, column) tables of asm_tf_tables: two wavelengths and two planes per
    wavelength, 5 planes (the tables' bisection branch) and 1 plane (their lane-parallel branch),
    vs the fp64 oracle; plus the adjoint identity <A x, y> = <x, A^H y> through the C-ABI."""
    EF, ASM = _prop_cls()
    dev = _dev()
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((2, 2, H, W)) + 1j * rng.standard_normal((2, 2, H, W))).astype(np.complex64)
    wl = [C0 / 250e9, C0 / 330e9]
    field = EF(torch.from_numpy(x).to(dev), wavelengths=wl, spacing=[0.5e-3, 0.6e-3], device=dev)
    prop = ASM(z_distance=zs[0], padding_scale=2, bandlimit_type=bl, device=dev)
    planes = prop.propagate_planes(field, zs).cpu().numpy()
    assert planes.shape == (len(zs), 2, 2, H, W)
    for k, z in enumerate(zs):
        ref = orc.asm_forward(torch.from_numpy(x).to(torch.complex128), wavelengths([250, 330], True),
                              spacing(0.5, 0.6, True), z, 2, bandlimit_type=bl).numpy()
        ref32 = orc.asm_forward(torch.from_numpy(x), wavelengths([250, 330]), spacing(0.5, 0.6), z, 2,
                                bandlimit_type=bl).numpy()
        floor = rel_l2(ref32, ref)
        assert rel_l2(planes[k], ref) <= max(1e-4, 1.5 * floor), (k, z, floor)
    from quantizationawarethzdoe_amd.propagation import asm_apply
    gen = torch.Generator(device=dev).manual_seed(5)
    r = torch.randn(2, 2, H, W, dtype=torch.complex64, device=dev, generator=gen)
    y = torch.randn(1, 2, 2, H, W, dtype=torch.complex64, device=dev, generator=gen)
    code = 1 if bl == "exact" else 2
    Ax = asm_apply(r, wl, [0.5e-3, 0.6e-3], [zs[-1]], H, W, True, code)
    AHy = asm_apply(y, wl, [0.5e-3, 0.6e-3], [zs[-1]], H, W, True, code, adjoint=True)
    lhs = torch.vdot(y.reshape(-1).to(torch.complex128), Ax.reshape(-1).to(torch.complex128))
    rhs = torch.vdot(AHy.reshape(-1).to(torch.complex128), r.reshape(-1).to(torch.complex128))
    assert abs(complex(lhs - rhs)) / abs(complex(lhs)) <= 1e-4


@pytest.mark.parametrize("zs,bl", [([0.05, 0.06, 0.07, 0.08, 0.09], "exact"), ([0.052], "exact"),
                                   ([0.03, 0.11, -0.04], "approx")], ids=["edof_5z", "1z", "3z_approx"])
def test_asm_p500_compile_time_plan_vs_oracle(zs, bl):
    """P = 500 (the extended-DOF grid: 100 x 100, padding scale 4) on the compile-time mixed-radix
    plan 5 4 5 5 (Mx500: two-wave transforms in K1, K2, the Z-summing K2 and K3) vs the fp64
    oracle, every plane at <= max(1e-4, 1.5 x the fp32 oracle's own error); plus the adjoint
    identity <A x, y> = <x, A^H y> of the Z-plane forward and its one-launch Z-summing adjoint."""
    EF, ASM = _prop_cls()
    dev = _dev()
    rng = np.random.default_rng(50)
    x = (rng.standard_normal((2, 1, 100, 100)) + 1j * rng.standard_normal((2, 1, 100, 100))).astype(np.complex64)
    wl = C0 / 300e9
    field = EF(torch.from_numpy(x).to(dev), wavelengths=wl, spacing=[1e-3, 1e-3], device=dev)
    prop = ASM(z_distance=zs[0], padding_scale=4, bandlimit_type=bl, device=dev)
    planes = prop.propagate_planes(field, zs).cpu().numpy()
    assert planes.shape == (len(zs), 2, 1, 100, 100)
    for k, z in enumerate(zs):
        ref = orc.asm_forward(torch.from_numpy(x).to(torch.complex128), wavelengths([300], True),
                              spacing(1.0, 1.0, True), z, 4, bandlimit_type=bl).numpy()
        ref32 = orc.asm_forward(torch.from_numpy(x), wavelengths([300]), spacing(1.0, 1.0), z, 4,
                                bandlimit_type=bl).numpy()
        floor = rel_l2(ref32, ref)
        assert rel_l2(planes[k], ref) <= max(1e-4, 1.5 * floor), (k, z, floor)
    from quantizationawarethzdoe_amd.propagation import asm_apply
    gen = torch.Generator(device=dev).manual_seed(9)
    r = torch.randn(2, 1, 100, 100, dtype=torch.complex64, device=dev, generator=gen)
    y = torch.randn(len(zs), 2, 1, 100, 100, dtype=torch.complex64, device=dev, generator=gen)
    code = 1 if bl == "exact" else 2
    Ax = asm_apply(r, [wl], [1e-3, 1e-3], zs, 200, 200, True, code)
    AHy = asm_apply(y, [wl], [1e-3, 1e-3], zs, 200, 200, True, code, adjoint=True)
    lhs = torch.vdot(y.reshape(-1).to(torch.complex128), Ax.reshape(-1).to(torch.complex128))
    rhs = torch.vdot(AHy.reshape(-1).to(torch.complex128), r.reshape(-1).to(torch.complex128))
    assert abs(complex(lhs - rhs)) / abs(complex(lhs)) <= 1e-4


def test_asm_max_planes_per_call():
    """THZ_MAX_Z = 256 planes in one call (8 default z-chunks of 32, P = 1024): every 32nd plane
    and both chunk edges vs the fp64 oracle at <= max(1e-4, 1.5 x the fp32 oracle's error)."""
    from quantizationawarethzdoe_amd.propagation import asm_apply
    dev = _dev()
    rng = np.random.default_rng(31)
    x = (rng.standard_normal((1, 1, 512, 512)) + 1j * rng.standard_normal((1, 1, 512, 512))).astype(np.complex64)
    lam = wavelengths([300])
    sp = spacing(0.5, 0.5)
    zs = [float(v) for v in torch.linspace(0.01, 0.3, 256, dtype=torch.float64)]
    lamf, spf = [float(lam[0])], [float(sp[0]), float(sp[1])]
    out = asm_apply(torch.from_numpy(x).to(dev), lamf, spf, zs, 256, 256, True, 1).cpu().numpy()
    assert out.shape == (256, 1, 1, 512, 512)
    check = [0, 31, 32, 127, 128, 224, 255]
    xt = torch.from_numpy(x)
    with torch.no_grad():
        r64 = orc.asm_forward_planes(xt.to(torch.complex128), lam.double(), sp.double(), [zs[k] for k in check], 1)
        r32 = orc.asm_forward_planes(xt, lam, sp, [zs[k] for k in check], 1)
        for k, (_, a), (_, b) in zip(check, r64, r32):
            a = a.numpy()
            floor = rel_l2(b.numpy(), a)
            assert rel_l2(out[k], a) <= max(1e-4, 1.5 * floor), (k, zs[k], floor)


def test_asm_largest_transform_p16384_properties():
    """The largest compile-time transform (8192^2 field, padding 1 -> P = 16384; 1024-thread
    workgroups), checked by size-independent properties (an fp64 oracle plane of 16384^2 is out
    of reach of the CPU tests): the adjoint identity <A x, y> = <x, A^H y> to 1e-5 relative, and
    energy never grows under the band-limited transfer function (|H| <= 1)."""
    from quantizationawarethzdoe_amd.propagation import asm_apply
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(5)
    N = 8192
    x = torch.randn((1, 1, N, N), dtype=torch.complex64, device=dev, generator=g)
    y = torch.randn((1, 1, 1, N, N), dtype=torch.complex64, device=dev, generator=g)
    lam = [float(torch.tensor(C0 / 300e9, dtype=torch.float32))]
    sp = [float(torch.tensor(0.5e-3, dtype=torch.float32))] * 2
    ax = asm_apply(x, lam, sp, [0.3], N // 2, N // 2, True, 1)
    ahy = asm_apply(y, lam, sp, [0.3], N // 2, N // 2, True, 1, adjoint=True)
    lhs = torch.vdot(ax.reshape(-1).to(torch.complex128), y.reshape(-1).to(torch.complex128))
    rhs = torch.vdot(x.reshape(-1).to(torch.complex128), ahy.reshape(-1).to(torch.complex128))
    scale = float(torch.linalg.vector_norm(ax.abs().double())) * float(torch.linalg.vector_norm(y.abs().double()))
    assert abs(complex(lhs - rhs)) <= 1e-5 * scale, (complex(lhs), complex(rhs), scale)
    ex = float((x.abs().double() ** 2).sum())
    eax = float((ax.abs().double() ** 2).sum())
    assert 0.0 < eax <= ex * (1 + 1e-5), (eax, ex)


@pytest.mark.parametrize("H,W,s,bl,C,Z,zc", [
    (80, 72, 1.5, "approx", 2, 5, 0),       # runtime plan (P = 200 / 180), one chunk
    (100, 100, 2, "exact", 1, 4, 0),        # P = 300: the mixed-radix column pass
    (100, 100, 2, "exact", 1, 7, 3),        # P = 300, three chunks (the later ones add into U)
    (100, 100, 4, "exact", 1, 5, 0),        # P = 500: the compile-time 5 4 5 5 plan (extended DOF)
    (100, 100, 4, "exact", 2, 5, 2),        # P = 500, two wavelengths, three chunks
    (512, 512, 1, "exact", 2, 5, 2),        # P = 1024: the power-of-two column pass, three chunks
    (1024, 1024, 1, "exact", 1, 3, 0),      # P = 2048
    (60, 70, 1, "none", 1, 3, 0),           # no band limit
])
def test_asm_multi_plane_backward_one_adjoint_vs_oracle(H, W, s, bl, C, Z, zc):
    """The backward of a Z-plane forward is ONE adjoint launch that sums the planes' spectra in the
    column pass (thz_asm_forward, adjoint = 1, Z > 1) -- vs autograd through the fp64 oracle's
    per-plane forwards (rel-L2 <= 1e-4), through propagate_planes and through the raw C-ABI call
    (with an explicit z_chunk so later chunks accumulate into U)."""
    from quantizationawarethzdoe_amd.propagation import asm_apply, asm_padding
    EF, ASM = _prop_cls()
    dev = _dev()
    rng = np.random.default_rng(H + Z + zc)
    x = (rng.standard_normal((1, C, H, W)) + 1j * rng.standard_normal((1, C, H, W))).astype(np.complex64)
    freqs = [300] if C == 1 else [260, 320]
    wl = [C0 / (f * 1e9) for f in freqs]
    dxy = 1.0 if H <= 100 else 0.5
    zs = list(np.linspace(0.02, 0.12, Z) * (1 if H != 60 else 3))
    g = (rng.standard_normal((Z, 1, C, H, W)) + 1j * rng.standard_normal((Z, 1, C, H, W))).astype(np.complex64)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    field = EF(xd, wavelengths=wl if C > 1 else wl[0], spacing=[dxy * 1e-3, dxy * 1e-3], device=dev)
    prop = ASM(z_distance=zs[0], padding_scale=s, bandlimit_type="exact" if bl == "none" else bl,
               bandlimit_kernel=bl != "none", device=dev)
    planes = prop.propagate_planes(field, zs)
    gx, = torch.autograd.grad(planes, xd, grad_outputs=torch.from_numpy(g).to(dev))
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        xo = torch.from_numpy(x).to(torch.complex128).requires_grad_(True)
        lam = wavelengths(freqs, True)
        sp = spacing(dxy, dxy, True)
        outs = [orc.asm_forward(xo, lam, sp, z, s, bandlimit=bl != "none",
                                bandlimit_type="exact" if bl == "none" else bl) for z in zs]
        ref, = torch.autograd.grad(torch.stack(outs), xo, grad_outputs=torch.from_numpy(g).to(torch.complex128))
    finally:
        torch.set_default_dtype(old)
    assert rel_l2(gx.cpu().numpy(), ref.numpy()) <= 1e-4, rel_l2(gx.cpu().numpy(), ref.numpy())
    # the raw entry with an explicit chunk size: the same sum
    ph, pw = asm_padding(H, W, (s, s))
    code = {"exact": 1, "approx": 2, "none": 0}[bl]
    sp32 = [float(np.float32(dxy * 1e-3))] * 2
    wl32 = [float(np.float32(w)) for w in wl]
    raw = asm_apply(torch.from_numpy(g).to(dev), wl32, sp32, zs, ph, pw, True, code, adjoint=True, z_chunk=zc)
    assert raw.shape == (1, C, H, W)
    assert rel_l2(raw.cpu().numpy(), ref.numpy()) <= 1e-4
