"""The Python glue the three propagate_zx share (Props/_zx.py, propagation._SLICE_FAMILIES), without a
GPU: the z-sweep as host floats, the argument checks (raised before any device check, the same
strings from every propagator), the family table's entry names against the library, and a plain text
search of the package source for the pieces that must exist once.
"""
import os
import re

import numpy as np
import pytest
import torch

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quantizationawarethzdoe_amd")
ZS = [0.25, 0.5, 0.75, 1.0]  # exact in every float format


@pytest.mark.parametrize("z", [
    torch.tensor(ZS),
    torch.tensor(ZS).reshape(2, 2),
    list(ZS),
    [torch.tensor(v) for v in ZS],
    np.array(ZS).reshape(2, 2),
], ids=["tensor_1d", "tensor_2d", "floats", "tensors_0d", "numpy_2d"])
def test_z_host_gives_the_flat_list_of_floats(z):
    from quantizationawarethzdoe_amd.Props._zx import _z_host
    got = _z_host(z)
    assert got == ZS and all(type(v) is float for v in got)


def test_z_host_of_a_scalar():
    from quantizationawarethzdoe_amd.Props._zx import _z_host
    for z in (0.5, np.float32(0.5), torch.tensor(0.5)):
        got = _z_host(z)
        assert got == [0.5] and type(got[0]) is float


def _props():
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    from quantizationawarethzdoe_amd.Props.CZT_Prop import CZT_prop
    from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop, VRS_prop
    return {"asm": ASM_prop, "czt": CZT_prop, "rsc": RSC_prop, "vrs": VRS_prop}


# a 16 x 16 CPU field: ASM (padding scale 1, cropped) and CZT (output grid = input grid) have 16 output
# rows, RSC / VRS 2 (16 // 2) = 16
N_ROWS = 16
BAD = {
    "axis": (dict(axis="z"), "propagate_zx: axis must be 'x' or 'y', got 'z'"),
    "grad": (dict(grad="both"), "propagate_zx: grad must be 'planes' or 'slice', got 'both'"),
    "row_negative": (dict(row=-1), f"propagate_zx: row -1 outside the valid range [0, {N_ROWS}) of the output rows"),
    "row_n": (dict(row=N_ROWS), f"propagate_zx: row {N_ROWS} outside the valid range [0, {N_ROWS}) of the output rows"),
}


@pytest.mark.parametrize("case", list(BAD))
@pytest.mark.parametrize("name", ["asm", "czt", "rsc", "vrs"])
def test_argument_errors_come_before_the_device_check_with_one_text(name, case):
    """On a CPU field the launch would raise RuntimeError ("needs a ROCm device tensor"); these raise
    ValueError first, with the same string from every propagator."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    B = 2 if name == "vrs" else 1
    field = ElectricField(torch.ones(B, 1, 16, 16, dtype=torch.complex64), wavelengths=1e-3, spacing=[1e-3, 1e-3],
                          device="cpu")
    prop = _props()[name](z_distance=0.1, device="cpu")
    prop.check_Zc = False
    kw, text = BAD[case]
    with pytest.raises(ValueError) as err:
        prop.propagate_zx(field, [0.1, 0.2], **kw)
    assert str(err.value) == text


def test_family_entry_names_are_exported_and_bound():
    from quantizationawarethzdoe_amd import _lib, propagation as P
    assert sorted(P._SLICE_FAMILIES) == ["asm", "czt", "rsc"]
    h = _lib.lib()
    for tag, fam in P._SLICE_FAMILIES.items():
        assert len(fam.entries) == 4 and len(set(fam.entries)) == 4
        for name in fam.entries:
            assert tag in name and name in _lib.EXPORTED and hasattr(h, name), name


def _package_source():
    text = []
    for root, _, files in os.walk(PKG):
        for f in sorted(files):
            if f.endswith(".py"):
                with open(os.path.join(root, f), encoding="utf-8") as fh:
                    text.append(fh.read())
    return "\n".join(text)


def test_shared_pieces_exist_once_in_the_package_source():
    src = _package_source()
    for once in ("axis must be 'x' or 'y'", "10240 * 1024 * 1024", "def _z_host"):
        assert src.count(once) == 1, (once, src.count(once))
    functions = re.findall(r"^class (\w+)\(torch\.autograd\.Function\):", src, flags=re.M)
    assert [n for n in functions if "Slice" in n] == ["_SliceFunction"], functions
