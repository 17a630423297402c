"""The point-propagation kernels (csrc/thz_points.hip) against the fp64 restatement of the sum (tests/points_ref.py),
held to parity.MARGIN x the fp32 floor of the contract's own algebra; the gradient by the rule of parity.Ratios."""
import functools

import pytest
import torch

from tests import gpu_util, parity, points_ref

pytestmark = pytest.mark.gpu
LOG = "THZ_POINTS_PARITY_LOG"
C64, C128 = torch.complex64, torch.complex128
RATIOS = parity.Ratios(LOG, "")
SP = (0.5e-3, 0.4e-3)

# (B, C, H, W, M, chunks, origin).  A workgroup owns 512 owners, slot k of thread t being owner 256 k + t, so a wave
# fills 64 consecutive owners of a slot; a streamed tile is 256 items; 4 channels x 2 batch entries are in a lane.
# One element; a three-term sum; B = 2 with C = 3 on 25 x 41 = 1025 pixels cut into chunks = 3 (342, 342, 341) for
# 65 points (a second wave of one) about a shifted origin; C = 5 (a second channel tile of one) with 257 pixels (a second
# streamed tile of one), 257 points (a second slot of one) and chunks = 50 clamped to the 2 streamed tiles; B = 3 (a
# second batch tile of one) with 513 points (a second workgroup of one) on the library's own split.
CASES = [(1, 1, 1, 1, 1, None, (0.0, 0.0)), (1, 1, 1, 3, 2, None, (0.0, 0.0)), (2, 3, 25, 41, 65, 3, (1.3e-3, -0.7e-3)),
         (1, 5, 1, 257, 257, 50, (0.0, 0.0)), (3, 1, 16, 20, 513, None, (-2.1e-3, 0.9e-3))]


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs, the fp64 restatements and their fp32 floors -- computed once per case"""
    B, C, H, W, M, chunks, origin = case
    g = torch.Generator().manual_seed(B + C + H + W + M)
    lam = torch.tensor([gpu_util.f32(v) for v in torch.linspace(0.8e-3, 1.5e-3, C).tolist()], dtype=torch.float64)
    lo = torch.tensor([-20e-3, -15e-3, 5e-3], dtype=torch.float64)
    pts = lo + torch.rand(M, 3, dtype=torch.float64, generator=g) * (torch.tensor([20e-3, 15e-3, 40e-3], dtype=torch.float64) - lo)
    U, gr = gpu_util.white_cpu((B, C, H, W), seed=M + W), gpu_util.white_cpu((B, C, M), seed=M + H)
    fwd = points_ref.rs_points(U, pts, lam, SP, origin)
    adj = points_ref.adjoint(gr, pts, lam, SP, (H, W), origin)
    caps = dict(rel_cap=1e-5, max_cap=1e-3)
    return dict(dev=gpu_util.dev(), lam=lam, pts=pts, U=U, g=gr, fwd=fwd, adj=adj, chunks=chunks, origin=origin,
                fwd_floor=parity.floor_of(points_ref.rs_points(U, pts, lam, SP, origin, torch.float32), fwd,
                                          at_least_u32=H * W <= 3, **caps),
                adj_floor=parity.floor_of(points_ref.adjoint(gr, pts, lam, SP, (H, W), origin, torch.float32), adj,
                                          at_least_u32=M <= 3, **caps))


def _run(c, U, pts=None, chunks=-1):
    from quantizationawarethzdoe_amd import points
    return points.rs_points(U, c["pts"] if pts is None else pts, wavelengths=c["lam"].tolist(), spacing=SP,
                            origin=c["origin"], chunks=c["chunks"] if chunks == -1 else chunks)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_parity(case):
    c = _case(case)
    U = c["U"].to(c["dev"]).requires_grad_(True)
    out = _run(c, U)
    parity.judge(LOG, "points", "forward", str(case), out.detach().cpu(), c["fwd"], c["fwd_floor"], widths=(8, 52))
    out.backward(c["g"].to(c["dev"]))
    parity.judge(LOG, "points", "adjoint", str(case), U.grad.cpu(), c["adj"], c["adj_floor"], widths=(8, 52))


def _grad(fn, x0, dtype):
    """view_as_real of the gradient of the real scalar fn(x, dtype) at x0 cast to the complex type of ``dtype``"""
    x = x0.clone().to(C128 if dtype == torch.float64 else C64).requires_grad_(True)
    fn(x, dtype).backward()
    return torch.view_as_real(x.grad)


@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=str)
def test_backward(case):
    """the gradient of sum mask |out|^2, and the adjoint identity <A x, y> = <x, A^H y> in complex128 to 1e-5"""
    c = _case(case)
    mask = torch.rand(c["fwd"].shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)

    def loss(x, dtype):
        return (points_ref.rs_points(x, c["pts"], c["lam"], SP, c["origin"], dtype).abs().pow(2) * mask.to(dtype)).sum()

    x = c["U"].to(c["dev"]).requires_grad_(True)
    (_run(c, x).abs().pow(2) * mask.float().to(c["dev"])).sum().backward()
    RATIOS.grad("rs_points", str(case), torch.view_as_real(x.grad), lambda dtype: _grad(loss, c["U"], dtype))

    x2 = c["U"].to(c["dev"]).requires_grad_(True)
    ax = _run(c, x2)
    ax.backward(c["g"].to(c["dev"]))
    lhs = torch.vdot(ax.detach().cpu().to(C128).flatten(), c["g"].to(C128).flatten())
    rhs = torch.vdot(c["U"].to(C128).flatten(), x2.grad.cpu().to(C128).flatten())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_bitwise():
    """a repeated call, three graph replays against eager, and B = 2 against the entries one at a time at a fixed split"""
    c = _case(CASES[2])
    U, pts = c["U"].to(c["dev"]), c["pts"].to(c["dev"])
    eager = _run(c, U, pts)
    assert gpu_util.bits(eager, _run(c, U, pts)) and gpu_util.bits(eager, _run(c, U))
    for b in range(2):
        assert gpu_util.bits(eager[b], _run(c, U[b:b + 1].contiguous(), pts)[0])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = _run(c, U, pts)  # device points: the capture only launches
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert gpu_util.bits(eager, out)
    for what, (ratio, name) in sorted(RATIOS.worst.items()):
        parity.emit(LOG, f"points {what:<16s} {name:<52s} err / bound {ratio:.4f}")


def test_public_path():
    """Points_prop on a tilted plane is rs_points on the same inputs bit for bit, in the plane's own shape"""
    from quantizationawarethzdoe_amd import points
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props import Points_prop
    c = _case(CASES[2])
    plane = points.tilted_plane((6, 9), 0.7e-3, (2e-3, -1e-3, 30e-3), tilt_x=0.1, tilt_y=-0.35)
    field = ElectricField(c["U"].to(c["dev"]), wavelengths=c["lam"].float(), spacing=list(SP), device=c["dev"])
    got = Points_prop(plane, origin=c["origin"])(field)
    assert got.shape == (2, 3, 6, 9)
    assert gpu_util.bits(got, points.rs_points(field.data, plane, wavelengths=field.wavelengths_host,
                                               spacing=field.spacing_host, origin=c["origin"]))
