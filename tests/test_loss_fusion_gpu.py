"""Fused ASM -> QAT loss (thz_asm_forward_loss): the row-inverse pass of the last
propagation accumulates mean((normalize(|E|^2) - target)^2) over the rows it stores.

Checked against the separate path (asm_propagate -> intensity_mse, the two-kernel loss) and the
fp64 oracle (oracle/thz_oracle.py intensity_mse of the oracle ASM, Props/ASM_Prop.py:314-378 +
experiment_four_focal_spots.ipynb:336-370).  The output field is the same K1/K2/K3 pipeline, so
it matches the separate path bit for bit; the loss is a one-pass fp64 sum against fp32 two-pass
sums, rel <= 1e-5; gradients rel-L2 <= 1e-5 (same kernels, the loss statistics agree to fp32
rounding).  Against the fp64 oracle: rel <= 1e-4 (fp32 propagation).
"""
import numpy as np
import pytest
import torch

from oracle import thz_oracle as orc
from tests.golden_io import rel_l2
from tests.gpu_util import dev as _dev

pytestmark = pytest.mark.gpu
C0 = 2.998e8


# (B, C, H, W, padding_scale, target broadcast): P = 300 mixed-radix (cfg4 / cfg5), power of two,
# runtime plan; targets broadcast over B and / or C as the notebooks' do
CASES = [
    ((1, 1, 100, 100), 2, (1, 1)),
    ((3, 1, 100, 100), 2, (3, 1)),
    ((2, 2, 100, 100), 2, (1, 2)),
    ((1, 1, 512, 512), 2, (1, 1)),
    ((2, 1, 256, 256), 2, (1, 1)),
    ((2, 2, 60, 70), 2, (2, 2)),
]


def _wl(C):
    return [C0 / 300e9, C0 / 250e9][:C]


@pytest.mark.parametrize("shape,ps,tb", CASES)
def test_asm_loss_fused_equals_separate(shape, ps, tb):
    from quantizationawarethzdoe_amd import optics, propagation as P
    dev = _dev()
    B, C, H, W = shape
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(shape, generator=g) + 1j * torch.randn(shape, generator=g)).to(torch.complex64).to(dev)
    tgt = torch.rand((tb[0], tb[1], H, W), generator=g).to(dev)
    wl, sp, z = _wl(C), (1e-3, 1e-3), 0.12
    ph, pw = P.asm_padding(H, W, (ps, ps))
    res = []
    for fused in (True, False):
        xd = x.clone().requires_grad_(True)
        if fused:
            out, loss = P.asm_propagate_loss(xd, tgt, wl, sp, z, ph, pw)
        else:
            out = P.asm_propagate(xd, wl, sp, [z], ph, pw)
            loss = optics.intensity_mse(out[0], tgt)
        loss.backward()
        res.append((out.detach().cpu(), float(loss.detach()), xd.grad.cpu()))
    (o1, l1, g1), (o2, l2, g2) = res
    assert rel_l2(o1.numpy(), o2.numpy()) <= 1e-7  # same pipeline (the K3 variant only adds the sums)
    assert abs(l1 - l2) <= 1e-5 * abs(l2)
    assert rel_l2(g1.numpy(), g2.numpy()) <= 1e-5
    # the fp64 oracle: propagate, then the loss
    xo = x.cpu().to(torch.complex128)
    oo = orc.asm_forward(xo, wl, sp, z, padding_scale=ps)
    lo = float(orc.intensity_mse(oo, tgt.cpu().double()))
    assert abs(l1 - lo) <= 1e-4 * abs(lo)


def test_asm_loss_out_cotangent_adds():
    """When the fused output field is used besides the loss, its cotangent adds to the loss's."""
    from quantizationawarethzdoe_amd import optics, propagation as P
    dev = _dev()
    shape = (2, 1, 100, 100)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, dtype=torch.complex64, generator=g).to(dev)
    tgt = torch.rand((1, 1, 100, 100), generator=g).to(dev)
    ph, pw = P.asm_padding(100, 100, (2, 2))
    res = []
    for fused in (True, False):
        xd = x.clone().requires_grad_(True)
        if fused:
            out, loss = P.asm_propagate_loss(xd, tgt, _wl(1), (1e-3, 1e-3), 0.2, ph, pw)
        else:
            out = P.asm_propagate(xd, _wl(1), (1e-3, 1e-3), [0.2], ph, pw)
            loss = optics.intensity_mse(out[0], tgt)
        (loss + 0.3 * out.abs().pow(2).sum()).backward()
        res.append(xd.grad.cpu())
    assert rel_l2(res[0].numpy(), res[1].numpy()) <= 1e-5


def test_intensity_mse_argmax_tie_and_vs_oracle():
    """The one-pass loss kernel: a tied maximum takes the first index (torch.max), the loss and
    the field gradient match the fp64 oracle / autograd of the reference formula."""
    from quantizationawarethzdoe_amd import optics
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    f = torch.randn((3, 2, 33, 47), dtype=torch.complex64, generator=g)
    f[1, 0, 4, 5] = 10.0
    f[1, 1, 20, 7] = -10.0  # same |E|^2, later index: the gradient's max path stays at the first
    t = torch.rand((1, 2, 33, 47), generator=g)
    fd = f.to(dev).requires_grad_(True)
    loss = optics.intensity_mse(fd, t.to(dev))
    loss.backward()
    fr = f.to(torch.complex128).requires_grad_(True)
    inten = fr.abs() ** 2
    m = inten.reshape(3, -1).max(1, keepdim=True)[0].reshape(3, 1, 1, 1)
    lr = ((inten / m - t.double()) ** 2).mean()
    lr.backward()
    loss, lr = float(loss.detach()), float(lr.detach())
    assert abs(loss - lr) <= 1e-5 * lr
    assert abs(loss - float(orc.intensity_mse(f.to(torch.complex128), t.double()))) <= 1e-5 * lr
    assert rel_l2(fd.grad.cpu().numpy(), fr.grad.numpy().astype(np.complex64)) <= 1e-5


def test_trainers_default_loss_is_fused_and_matches():
    """QATTrainer with the default loss runs the fused pipeline; a loss_fn that is not the default
    object runs the separate kernels.  Same seeds -> same loss trajectory and weights."""
    from quantizationawarethzdoe_amd import optics, qat
    dev = _dev()
    traj = []
    for fused in (True, False):
        torch.manual_seed(0)
        system = qat.FourFocalSpotsSystem(device=dev)
        lf = None if fused else (lambda d, t: optics.intensity_mse(d, t))
        tr = qat.QATTrainer(system, qat.four_focal_spots_target(device=dev), max_itrs=20, loss_fn=lf)
        torch.manual_seed(11)
        losses = [float(tr.step(f)) for f in (0.1, 0.2, 0.5, 0.9)]
        traj.append((losses, [p.detach().cpu() for p in system.parameters() if p.requires_grad]))
    (la, wa), (lb, wb) = traj
    assert np.allclose(la, lb, rtol=2e-5, atol=0)
    for a, b in zip(wa, wb):
        assert rel_l2(a.numpy(), b.numpy()) <= 1e-4


def test_donn_default_loss_fused_matches():
    from quantizationawarethzdoe_amd import donn, optics
    dev = _dev()
    g = torch.Generator().manual_seed(2)
    u = torch.rand(8, 1, 100, 100, generator=g).to(dev)
    labels = torch.randint(0, 10, (8,), generator=g).to(dev)
    out = []
    for fused in (True, False):
        torch.manual_seed(4)
        model = donn.DONN(device=dev)
        lf = None if fused else (lambda d, t: optics.intensity_mse(d, t))
        tr = donn.DONNTrainer(model, donn.detector_targets(device=dev), loss_fn=lf)
        torch.manual_seed(6)
        out.append(([float(tr.step(u, labels)) for _ in range(3)], [p.detach().cpu() for p in tr.params]))
    (la, pa), (lb, pb) = out
    assert np.allclose(la, lb, rtol=2e-5, atol=0)
    for a, b in zip(pa, pb):
        assert rel_l2(a.numpy(), b.numpy()) <= 1e-4


@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
def test_loss_near_convergence_vs_fp64_oracle(fused):
    """A near-converged field (normalised intensity = target up to ~1e-4): the loss kernels form
    sum (I/m - T)^2 as S_II/m^2 - 2 S_IT/m + S_TT from one-pass fp64 sums (ADVICE round 2 asked
    whether that cancels catastrophically).  In fp64 the cancellation costs ~1e-16 S_TT / loss
    ~ 1e-9 relative here; what remains is the fp32 rounding of |E|^2 itself (~6e-8 of I against
    residuals of ~1e-4), so the bound vs the fp64 oracle of the same fp32 field is 1e-2 relative
    -- a cancelling fp32 form would be off by O(1).  The loss is ~1e-8 against S_TT / n ~ 0.3.

    Gradient (2 E dL/dI), two references.  (a) fp64 arithmetic on the fp32 intensities the
    reference itself forms (torch.abs(E) ** 2 of the complex64 field, on the device): rel-L2 <= 5e-3
    (the kernels' fp32 residual r = I/m - T carries ~1e-7 of T against r ~ 1e-4 T).  (b) the fp64
    oracle (|E|^2 in fp64): the max intensity m then differs by the fp32 rounding of I_max
    (delta ~ 6e-8), which shifts every residual coherently by -(I/m) delta; the argmax element's
    term S / m^2 (S = sum_i r_i I_i, a random-sign sum of n = 10^4 residuals of ~1e-4) moves by
    ~delta sqrt(n) / 1e-4 ~ 6 %, and that element carries ~40 % of the gradient's norm here
    (measured on the box: 1.5e-2 rel-L2, all of it at the two argmax elements).  Bound 0.1 on the whole
    gradient; with the two argmax elements masked the old bound, 1e-2, and at each argmax element
    0.25 relative."""
    from quantizationawarethzdoe_amd import optics, propagation as P
    dev = _dev()
    g = torch.Generator().manual_seed(8)
    shape = (2, 1, 100, 100)
    x = (torch.randn(shape, generator=g) + 1j * torch.randn(shape, generator=g)).to(torch.complex64)
    wl, sp, z = _wl(1), (1e-3, 1e-3), 0.12
    ph, pw = P.asm_padding(100, 100, (2, 2))
    with torch.no_grad():
        E = P.asm_propagate(x.to(dev), wl, sp, [z], ph, pw)[0]
        I = E.abs().double() ** 2
        I = I / I.amax(dim=(1, 2, 3), keepdim=True)
        tgt = (I * (1 + 1e-4 * torch.randn(I.shape, generator=g).to(dev).double())).float()
    xd = x.to(dev).requires_grad_(True)
    if fused:
        # the loss of the field the fused pipeline stored, in fp64 (isolates the loss arithmetic from
        # the fp32 propagation); the gradient vs the separate path's through the same kernels
        out, loss = P.asm_propagate_loss(xd, tgt, wl, sp, z, ph, pw)
        loss.backward()
        gx = xd.grad
        ref = orc.intensity_mse(out[0].detach().cpu().to(torch.complex128), tgt.cpu().double())
        xs = x.to(dev).requires_grad_(True)
        optics.intensity_mse(P.asm_propagate(xs, wl, sp, [z], ph, pw)[0], tgt).backward()
        rg = xs.grad.cpu()
    else:
        Ed = E.clone().requires_grad_(True)
        loss = optics.intensity_mse(Ed, tgt)
        loss.backward()
        gx = Ed.grad
        Eo = E.cpu().to(torch.complex128).requires_grad_(True)
        ref = orc.intensity_mse(Eo, tgt.cpu().double())
        ref.backward()
        rg = Eo.grad
        # (a): dL/dE = 2 E g (r / m - [argmax] S / m^2), g = 2 / N, in fp64 from the fp32 intensities
        I32 = (E.abs() ** 2).double().cpu()
        flat = I32.reshape(2, -1)
        m = flat.max(dim=1).values
        am = flat.argmax(dim=1)
        r = flat / m[:, None] - tgt.cpu().double().reshape(2, -1)
        S = (r * flat).sum(dim=1)
        gI = (2.0 / flat.numel()) * r / m[:, None]
        gI[torch.arange(2), am] -= (2.0 / flat.numel()) * S / m ** 2
        rg32 = (2.0 * E.cpu().to(torch.complex128).reshape(2, -1) * gI).reshape(E.shape)
        assert rel_l2(gx.cpu().numpy(), rg32.numpy()) <= 5e-3
    lv, rv = float(loss.detach()), float(ref.detach())
    assert 1e-10 < rv < 1e-6, rv  # near convergence: the loss is ~1e-8 of the target's scale
    assert abs(lv - rv) <= 1e-2 * rv, (lv, rv)
    assert rel_l2(gx.cpu().numpy(), rg.numpy()) <= (1e-2 if fused else 0.1)
    if not fused:
        # (b) at the old bound with the argmax elements masked: everywhere
        # else the fp64 oracle's gradient is met to 1e-2; at the argmax element itself the coherent
        # S / m^2 shift (~6 %, above) is bounded separately
        Io = (Eo.detach().abs() ** 2).reshape(2, -1)
        amo = Io.argmax(dim=1)
        ga, gr = gx.cpu().reshape(2, -1).clone(), rg.reshape(2, -1).clone()
        at_max = [(ga[b, amo[b]], gr[b, amo[b]]) for b in range(2)]
        ga[torch.arange(2), amo] = 0
        gr[torch.arange(2), amo] = 0
        assert rel_l2(ga.numpy(), gr.numpy()) <= 1e-2, rel_l2(ga.numpy(), gr.numpy())
        for a, b_ in at_max:
            assert abs(complex(a) - complex(b_)) <= 0.25 * abs(complex(b_)), (complex(a), complex(b_))


@pytest.mark.parametrize("how", ["wavelength_f64", "data_c128"])
def test_deferred_loss_refuses_complex128_like_the_unfused_path(how):
    """A complex128 propagation (float64 wavelength tensor or complex128 data) under
    deferred_output() must not reach the complex64 fused-loss kernel: field_intensity_mse raises the
    TypeError the unfused intensity_mse raises for a complex128 field, and the
    same system in complex64 runs."""
    from quantizationawarethzdoe_amd import optics
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    from quantizationawarethzdoe_amd.propagation import deferred_output
    dev = _dev()
    x = torch.randn(1, 1, 64, 64, dtype=torch.complex64, device=dev)
    lam = torch.tensor([C0 / 300e9], dtype=torch.float64 if how == "wavelength_f64" else torch.float32)
    data = x.to(torch.complex128) if how == "data_c128" else x
    prop = ASM_prop(z_distance=0.05, padding_scale=2, device=dev)
    target = torch.rand(1, 1, 64, 64, device=dev)
    f = ElectricField(data=data, wavelengths=lam, spacing=1e-3, device=dev)
    with deferred_output():
        out = prop(f)
        with pytest.raises(TypeError, match="complex64"):
            optics.field_intensity_mse(out, target)
    f32 = ElectricField(data=x, wavelengths=lam.float(), spacing=1e-3, device=dev)
    with deferred_output():
        loss = optics.field_intensity_mse(prop(f32), target)
    assert torch.isfinite(loss)
