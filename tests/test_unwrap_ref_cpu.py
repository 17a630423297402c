"""The CPU restatement of the unwrapping model (tests/unwrap_ref.py) recovers a known phase."""
import pytest
import torch

from tests import unwrap_ref as R


@pytest.mark.parametrize("shape", [(64, 64), (64, 256), (128, 64)])
def test_restatement_recovers_the_phase(shape):
    """fp64 direct solve of a smooth field with a largest difference of 2.5 rad: the error left is that of rounding the
    field to complex64 (4 - 6e-8 rad), held to 1e-6 rad."""
    U, s = R.smooth_field(*shape)
    phi, _ = R.unwrap(U, dtype=torch.float64)
    err = float(((phi - phi.mean()) - (s - s.mean())).abs().max())
    print(shape, "range", float(s.max() - s.min()), "err", err)
    assert err < 1e-6


def test_public_module_checks_on_the_host():
    from quantizationawarethzdoe_amd import _lib, unwrap
    assert {"thz_unwrap_workspace_size", "thz_unwrap_phase", "thz_unwrap_residues"} <= set(_lib.EXPORTED)
    with pytest.raises(RuntimeError, match="ROCm device"):
        unwrap.unwrap_phase(torch.ones(64, 64, dtype=torch.complex64))
