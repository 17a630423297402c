"""The Hermite-Gauss kernels (csrc/thz_modes.hip) against the fp64 restatement of the model on their own exported
tables (tests/modes_ref.py), held to parity.MARGIN x the fp32 floor of the same algebra."""
import functools

import pytest
import torch

from tests import gpu_util, modes_ref, parity

pytestmark = pytest.mark.gpu
LOG = "THZ_MODES_PARITY_LOG"
C64, C128 = torch.complex64, torch.complex128
PITCH = 0.5e-3

# (B, C, H, W, M, N).  One pixel; tails on both axes of one tile (MD_BM = 128 rows, MD_BK = 32 columns: W = 33 is the
# second LDS step); two channels, a second wave (H = 33) and partial mode tiles; two batches, a second workgroup tile
# (H = 130 > MD_BM) with full mode tiles; three per-channel waists and nine LDS steps with a one-column tail; a second
# workgroup tile with a one-row tail and N < M.
CASES = [(1, 1, 1, 1, 1, 1), (1, 1, 31, 33, 1, 1), (1, 2, 33, 40, 4, 3), (2, 1, 130, 100, 32, 32),
         (1, 3, 64, 257, 7, 32), (1, 1, 129, 64, 32, 5)]


def _geometry(case):
    B, C, H, W, M, N = case
    waist = ([(0.15 + 0.02 * c) * W * PITCH for c in range(C)], [(0.15 + 0.02 * c) * H * PITCH for c in range(C)])
    return waist, (-0.3 * PITCH, 0.1 * PITCH)


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs, the exported tables, the fp64 restatements and their fp32 floors -- computed once per case"""
    from quantizationawarethzdoe_amd import modes
    B, C, H, W, M, N = case
    dev = gpu_util.dev()
    (wx, wy), (x0, y0) = _geometry(case)
    Gx = modes.hg_table(N, W, PITCH, wx, x0, dev).cpu()
    Gy = modes.hg_table(M, H, PITCH, wy, y0, dev).cpu()
    U, c = gpu_util.white_cpu((B, C, H, W), seed=H + W), gpu_util.white_cpu((B, C, M, N), seed=M + N)
    s = PITCH * PITCH
    ana, syn = modes_ref.decompose(Gy, U, Gx, s), modes_ref.synthesize(Gy, c, Gx, 1.0)
    # With one mode the fp32 run rounds two or three times per number and can land below one rounding: on one CPU 2.7e-8
    # for the coefficient and 3.6e-8 (two roundings, u / sqrt(3) each) for the field of 31 x 33 pixels, 4.4e-8 for the
    # one pixel.  Such a floor is clamped up to 2^-24, as the Hankel test does for N = 1.
    caps = dict(rel_cap=1e-5, max_cap=1e-3, at_least_u32=M * N == 1)
    return dict(dev=dev, Gx=Gx, Gy=Gy, U=U, c=c, ana=ana, syn=syn,
                ana_floor=parity.floor_of(modes_ref.decompose(Gy, U, Gx, s, C64), ana, **caps),
                syn_floor=parity.floor_of(modes_ref.synthesize(Gy, c, Gx, 1.0, C64), syn, **caps))


def _decompose(case, U):
    from quantizationawarethzdoe_amd import modes
    waist, centre = _geometry(case)
    return modes.hg_decompose(U, PITCH, waist, orders=case[4:], center=centre)


def _synthesize(case, c):
    from quantizationawarethzdoe_amd import modes
    waist, centre = _geometry(case)
    return modes.hg_synthesize(c, case[2:4], PITCH, waist, center=centre)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_parity(case):
    c = _case(case)
    parity.judge(LOG, "modes", "analyze", str(case), _decompose(case, c["U"].to(c["dev"])).cpu(), c["ana"], c["ana_floor"])
    parity.judge(LOG, "modes", "synthesize", str(case), _synthesize(case, c["c"].to(c["dev"])).cpu(), c["syn"],
                 c["syn_floor"])


@pytest.mark.parametrize("case", [CASES[2], CASES[3]], ids=str)
def test_backward(case):
    """the gradients of sum |out|^2 mask through both directions against fp64 autograd of the restatement, within
    MARGIN x the error of the complex64 CPU autograd; the adjoint identity <A x, y> = <x, A^H y> in fp64 to 1e-5"""
    c = _case(case)
    s = PITCH * PITCH
    for name, gpu_fn, ref_fn, x0, scale in (("analyze", _decompose, modes_ref.decompose, c["U"], s),
                                            ("synthesize", _synthesize, modes_ref.synthesize, c["c"], 1.0)):
        out_shape = c["ana" if name == "analyze" else "syn"].shape
        mask = torch.rand(out_shape, generator=torch.Generator().manual_seed(7))

        def cpu_grad(cdtype):
            x = x0.clone().to(cdtype).requires_grad_(True)  # a leaf of its own: the case is shared
            out = ref_fn(c["Gy"], x, c["Gx"], scale, cdtype)
            (out.abs().pow(2) * mask.to(out.real.dtype)).sum().backward()
            return x.grad.to(C128)

        x = x0.to(c["dev"]).requires_grad_(True)
        (gpu_fn(case, x).abs().pow(2) * mask.to(c["dev"])).sum().backward()
        g64, g32 = cpu_grad(C128), cpu_grad(C64)
        e32 = float((g32 - g64).norm() / g64.norm())
        err = float((x.grad.cpu().to(C128) - g64).norm() / g64.norm())
        parity.emit(LOG, f"modes backward {name} {case}: e32 {e32:.3e} err {err:.3e} ratio {err / e32:.2f}")
        assert err <= parity.MARGIN * e32

        y = gpu_util.white_cpu(tuple(out_shape), seed=11)
        x2 = x0.to(c["dev"]).requires_grad_(True)
        ax = gpu_fn(case, x2)
        ax.backward(y.to(c["dev"]))
        lhs = torch.vdot(ax.detach().cpu().to(C128).flatten(), y.to(C128).flatten())
        rhs = torch.vdot(x0.to(C128).flatten(), x2.grad.cpu().to(C128).flatten())
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_bitwise():
    """a repeated call, graph replays against eager, B x C planes in one call against the planes one at a time"""
    from quantizationawarethzdoe_amd import modes
    case = (2, 2, 130, 100, 7, 5)
    (wx, wy), centre = _geometry(case)
    dev = gpu_util.dev()
    U, c = gpu_util.white_cpu(case[:4], seed=3).to(dev), gpu_util.white_cpu(case[:2] + case[4:], seed=4).to(dev)
    eager = _decompose(case, U), _synthesize(case, c)
    assert gpu_util.bits(eager[0], _decompose(case, U)) and gpu_util.bits(eager[1], _synthesize(case, c))
    for b in range(2):
        for ch in range(2):
            w = ([wx[ch]], [wy[ch]])
            one = modes.hg_decompose(U[b:b + 1, ch:ch + 1].contiguous(), PITCH, w, orders=case[4:], center=centre)
            assert gpu_util.bits(eager[0][b, ch], one[0, 0])
            one = modes.hg_synthesize(c[b:b + 1, ch:ch + 1].contiguous(), case[2:4], PITCH, w, center=centre)
            assert gpu_util.bits(eager[1][b, ch], one[0, 0])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = _decompose(case, U), _synthesize(case, c)  # the tables exist: the capture only launches
    for _ in range(3):
        out[0].zero_(), out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert gpu_util.bits(eager[0], out[0]) and gpu_util.bits(eager[1], out[1])


def test_physics():
    """gaussicity of a displaced and of a waist-mismatched Gaussian, and mode_filter with every mode kept on a field
    of 4 x 4 random coefficients, against the fp64 restatement by the Ratios.value rule (tests/test_modes_cpu.py ties
    the restatement to the closed forms); a complex128 field is refused by name"""
    from quantizationawarethzdoe_amd.utils import metrics
    dev = gpu_util.dev()
    n, p, w, d, w2 = 256, 0.25e-3, 8e-3, 3e-3, 6e-3
    ratios = parity.Ratios(LOG, "")

    def table(k, waist, centre, dtype):
        return modes_ref.table(k, n, p, [waist], centre).to(dtype)

    beams = torch.cat([torch.einsum("cmi,cnj->cmnij", table(1, wy, 0.0, torch.float64), table(1, wx, x0, torch.float64))
                       for wy, wx, x0 in ((w, w, d), (w2, w2, 0.0))]).reshape(2, 1, n, n).to(C64)

    def gaussicity(dtype):
        cdtype = C128 if dtype == torch.float64 else C64
        G = table(1, w, 0.0, dtype)
        c = modes_ref.decompose(G, beams, G, p * p, cdtype)[:, :, 0, 0]
        return c.abs() ** 2 / ((beams.to(cdtype).abs() ** 2).sum((-2, -1)) * p * p)

    ratios.value("gaussicity", "displaced 3 mm, waist 6 mm on 8 mm", metrics.gaussicity(beams.to(dev), p, w), gaussicity)

    coeffs = gpu_util.white_cpu((1, 1, 4, 4), seed=5)
    G4 = table(4, w, 0.0, torch.float64)
    field = modes_ref.synthesize(G4, coeffs, G4, 1.0).to(C64)

    def filtered(dtype):
        cdtype = C128 if dtype == torch.float64 else C64
        G = table(4, w, 0.0, dtype)
        out = modes_ref.synthesize(G, modes_ref.decompose(G, field, G, p * p, cdtype), G, 1.0, cdtype)
        return torch.view_as_real(out)

    kept = metrics.mode_filter(field.to(dev), torch.ones(4, 4), p, w)
    ratios.value("mode_filter", "4 x 4 kept", torch.view_as_real(kept), filtered)
    for what, (ratio, name) in sorted(ratios.worst.items()):
        parity.emit(LOG, f"modes {what:<12s} {name:<34s} err / bound {ratio:.4f}")
    with pytest.raises(TypeError, match="complex128"):
        metrics.gaussicity(beams.to(dev).to(C128), p, w)
