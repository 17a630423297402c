"""Propagation to points without a GPU: the restatement (tests/points_ref.py) pinned to the oracle's kernel function, the
geometry helpers of points.py and the host refusals."""
import math

import pytest
import torch

from oracle import thz_oracle as orc
from tests import points_ref

LAM = torch.tensor([0.9e-3, 1.4e-3], dtype=torch.float64)
PTS = torch.tensor([[3.1e-3, -2.2e-3, 7e-3], [-11e-3, 4.5e-3, 19e-3], [0.4e-3, 9e-3, 33e-3]], dtype=torch.float64)
SP = (0.5e-3, 0.4e-3)


@pytest.mark.parametrize("pixel", [(0, 0), (3, 5)])
def test_restatement_is_the_oracle_kernel(pixel):
    """a field that is one unit pixel gives dx dy G at the offsets to that pixel, to 1e-12 in fp64; and the sum is linear"""
    H, W, origin = 5, 7, (0.6e-3, -0.3e-3)
    i, j = pixel
    U = torch.zeros(1, 2, H, W, dtype=torch.complex128)
    U[0, :, i, j] = 1
    x, y = origin[0] + (j - (W - 1) / 2) * SP[0], origin[1] + (i - (H - 1) / 2) * SP[1]
    want = SP[0] * SP[1] * orc._rs_kernel(PTS[:, 2].view(1, 1, 1, 3), (PTS[:, 0] - x).view(1, 1, 1, 3),
                                           (PTS[:, 1] - y).view(1, 1, 1, 3), LAM)[:, :, 0, :]
    got = points_ref.rs_points(U, PTS, LAM, SP, origin)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12
    V = torch.randn(1, 2, H, W, dtype=torch.complex128, generator=torch.Generator().manual_seed(1))
    both = points_ref.rs_points(2 * U + 1j * V, PTS, LAM, SP, origin)
    assert float((both - (2 * got + 1j * points_ref.rs_points(V, PTS, LAM, SP, origin))).abs().max()) <= 1e-12 * float(both.abs().max())


def test_geometry_helpers():
    from quantizationawarethzdoe_amd import points
    c = (1e-3, -2e-3, 50e-3)
    flat = points.tilted_plane((3, 4), (0.5e-3, 0.25e-3), c)
    assert flat.shape == (3, 4, 3) and flat.dtype == torch.float64
    assert torch.allclose(flat[1, :, 0], c[0] + (torch.arange(4, dtype=torch.float64) - 1.5) * 0.5e-3, rtol=0, atol=1e-18)
    assert torch.allclose(flat[:, 2, 1], c[1] + (torch.arange(3, dtype=torch.float64) - 1.0) * 0.25e-3, rtol=0, atol=1e-18)
    assert bool((flat[..., 2] == c[2]).all())
    tilt = points.tilted_plane((3, 5), 0.5e-3, c, tilt_x=0.2, tilt_y=math.radians(30))
    assert torch.allclose(tilt[1, 2], torch.tensor(c, dtype=torch.float64), rtol=0, atol=1e-18)       # about the centre
    for d in (tilt[:, 1:] - tilt[:, :-1], tilt[1:] - tilt[:-1]):                                        # the pitch stays
        assert torch.allclose(d.norm(dim=-1), torch.full(d.shape[:-1], 0.5e-3, dtype=torch.float64), rtol=1e-12, atol=0)
    assert abs(float(tilt[1, 4, 2] - tilt[1, 0, 2]) + 4 * 0.5e-3 * math.sin(math.radians(30))) <= 1e-15  # about y: z falls with x
    line = points.scan_line((0, 0, 1e-2), (4e-3, 0, 2e-2), 5)
    assert line.shape == (5, 3) and torch.allclose(line[:, 0], torch.arange(5, dtype=torch.float64) * 1e-3, rtol=0, atol=1e-18)
    assert line[-1].tolist() == [4e-3, 0.0, 2e-2]


@pytest.mark.parametrize("pts, dtype, error, text", [
    ([[0.0, 0.0, 0.0]], torch.complex64, ValueError, "z > 0"),
    ([[0.0, 0.0, -1e-3]], torch.complex64, ValueError, "z > 0"),
    ([[0.0, float("nan"), 1e-3]], torch.complex64, ValueError, "finite"),
    ([[0.0, 0.0, 1e-3]], torch.complex128, TypeError, "complex128"),
])
def test_host_refusals(pts, dtype, error, text):
    from quantizationawarethzdoe_amd import points
    with pytest.raises(error, match=text):
        points.rs_points(torch.zeros(1, 1, 4, 4, dtype=dtype), pts, wavelengths=[1e-3], spacing=0.5e-3)
