"""Zernike analysis without a GPU: the restatement (tests/zernike_ref.py) against known polynomials and
orthonormality, and the argument errors of quantizationawarethzdoe_amd.zernike, raised before a device is touched."""
import math

import pytest
import torch

from tests import zernike_ref


def test_known_polynomials_and_index():
    from quantizationawarethzdoe_amd import zernike
    for k, (n, m) in enumerate(zernike_ref.orders(14)):
        assert zernike.index(n, m) == k and zernike.orders(k) == (n, m)
    assert zernike.num_modes(14) == 120 and zernike.num_modes(0) == 1
    # a row of pixels along +x with rho = 0, 0.25, 0.5, 0.75, 1 (pitch 1, R = 4, the centre on pixel 0)
    shape, spacing, pupil = (1, 5), (1.0, 1.0), (-2.0, 0.0, 4.0)
    rho = torch.arange(5, dtype=torch.float64) / 4
    for Z in (zernike_ref.closed_form(shape, spacing, pupil, 14),
              zernike_ref.recurrence(shape, spacing, pupil, 14, torch.float64)):
        assert float((Z[4, 0] - math.sqrt(3) * (2 * rho * rho - 1)).abs().max()) <= 1e-14
        assert abs(float(Z[zernike.index(14, 0), 0, 4]) - math.sqrt(15)) <= 1e-10


def test_recurrence_is_the_closed_form_and_orthonormal():
    """the fp64 recurrence within 1e-9 of the explicit sum at n = 14; G / N_pix -> I on a fine grid: a disk of radius
    R pixels is summed with a relative error of about R^-1.5 (the Gauss circle problem) times the integrand's edge
    value, at most 2 (n + 1): 0.03 at n = 14 and 0.015 up to n = 6 for R = 99"""
    shape, spacing, pupil = (201, 201), (1.0, 1.0), (0.3, -0.2, 99.0)
    Z = zernike_ref.recurrence(shape, spacing, pupil, 14, torch.float64)
    assert float((Z - zernike_ref.closed_form(shape, spacing, pupil, 14)).abs().max()) <= 1e-9
    G = zernike_ref.gram(Z) / float((Z[0] != 0).sum())
    eye = torch.eye(120, dtype=torch.float64)
    assert float((G - eye).abs().max()) <= 0.03 and float((G[:28, :28] - eye[:28, :28]).abs().max()) <= 0.015


@pytest.mark.parametrize("kw, text", [
    (dict(max_order=15), "max_order"), (dict(max_order=-1), "max_order"), (dict(pupil=(0.0, 0.0, 0.0)), "radius"),
    (dict(pupil=(0.0, 0.0, -1e-3)), "radius"), (dict(pupil=(0.0, 0.0, 1.4e-3), max_order=3), "fewer pixels"),
])
def test_argument_errors_before_the_device(kw, text, monkeypatch):
    from quantizationawarethzdoe_amd import _call, zernike

    def no_device(*a, **k):
        raise AssertionError("a device call was made although the arguments are wrong")

    monkeypatch.setattr(_call, "call", no_device)
    monkeypatch.setattr(zernike, "call", no_device)
    cfg = {**dict(spacing=1e-3, pupil=(0.0, 0.0, 3e-3), max_order=2), **kw}
    with pytest.raises(ValueError, match=text):
        zernike.fit(torch.zeros(1, 8, 8), **cfg)
    with pytest.raises(ValueError, match=text):
        zernike.gram((8, 8), device="cuda:0", **cfg)
    with pytest.raises(TypeError, match="float64"):
        zernike.project(torch.zeros(1, 8, 8, dtype=torch.float64), 1e-3, (0.0, 0.0, 3e-3), 2)
