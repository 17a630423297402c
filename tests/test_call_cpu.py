"""quantizationawarethzdoe_amd._call, the one call path of the Python glue, and the optics package's re-exports
(DESIGN section 36).  Needs the built library and no GPU."""
import ctypes

import pytest
import torch

# optics.NAME is optics.<module>.NAME: the public names of each module, written out
OPTICS_PUBLIC = {
    "elements": ("gaussian_beam", "thin_lens", "aperture", "intensity_mse", "field_intensity_mse", "resample"),
    "polarization": ("stokes", "polarization_ellipse", "POLARIZATION_EPS"),
    "noise": ("add_noise", "detect", "signal_scale", "noise_draws", "NOISE_KINDS"),
    "tolerance": ("tolerance_modulate", "TOLERANCE_ROUGHNESS"),
    "losses": ("dice_loss", "bce_with_logits", "ssim", "hierarchy_loss"),
    "heightmap": ("lut_quantize", "center_difference", "total_variation"),
    "metrics": ("region_stats", "line_widths", "RegionStats", "LineWidths"),
    "ifta": ("ifta_target_stats", "ifta_target_project", "ifta_doe_project", "IFTA_STATS"),
    "thick": ("thick_doe", "thick_doe_native", "THICK_CONVENTIONS"),
}


def test_arg_conversion():
    from quantizationawarethzdoe_amd import _call, _lib
    t = torch.arange(6, dtype=torch.float32)
    d = _lib.AsmDesc(B=3, C=1, H=4, W=4, Z=1)
    arr, ref = (ctypes.c_float * 2)(1.0, 2.0), ctypes.byref(d)
    given = (d, t, None, 7, -1, 0.25, True, arr, ref)
    got = _call.convert(given)
    assert len(got) == len(given)
    assert type(got[0]) is type(ref) and got[0]._obj is d
    assert ctypes.POINTER(_lib.AsmDesc).from_param(got[0]) is got[0]
    assert isinstance(got[1], ctypes.c_void_p) and got[1].value == t.data_ptr() != 0
    # None is what ctypes passes as NULL for c_void_p and POINTER(desc) parameters alike
    assert got[2] is None
    assert ctypes.c_void_p.from_param(got[2]) is None
    assert ctypes.POINTER(_lib.DoeDesc).from_param(got[2]) is None
    for a, b in zip(given[3:], got[3:]):
        assert a is b
    assert _call.convert(()) == []


def test_workspace_raises_before_the_device(monkeypatch):
    from quantizationawarethzdoe_amd import _call, _lib

    def no_device(*a, **kw):
        raise AssertionError("workspace() allocated although the size call failed")

    monkeypatch.setattr(_call.torch, "empty", no_device)
    monkeypatch.setattr(_call.torch.cuda, "device", no_device)
    with pytest.raises(_lib.ThzError) as e:
        _call.workspace(_lib.lib().thz_asm_workspace_size, _lib.AsmDesc(B=0, C=1, H=4, W=4, Z=1), device="cuda:0")
    assert e.value.code == _lib.THZ_E_ARG and "bad shape" in str(e.value)
    with pytest.raises(_lib.ThzError) as e:  # the scalar-first form
        _call.workspace(_lib.lib().thz_tv_workspace_size, 0, 4, 4, device="cuda:0")
    assert e.value.code == _lib.THZ_E_ARG and "bad shape" in str(e.value)


def test_workspace_size_forms_on_the_host():
    """Descriptor-first and scalar-first size calls through workspace(), allocated on the CPU: the bytes are the
    entry's own."""
    from quantizationawarethzdoe_amd import _call, _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.thz_tv_workspace_size(3, 5, 7, ctypes.byref(n)) == _lib.THZ_OK
    ws = _call.workspace(L.thz_tv_workspace_size, 3, 5, 7, device="cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == n.value > 0
    d = _lib.DiceBceDesc(N=2, M=9, p=2.0, smooth=1.0, terms=_lib.LOSS_TERM_DICE)
    assert L.thz_dice_bce_sums_workspace_size(ctypes.byref(d), ctypes.byref(n)) == _lib.THZ_OK
    assert _call.workspace(L.thz_dice_bce_sums_workspace_size, d, device="cpu").numel() == n.value > 0
    # the one size entry that returns its size: the float32 statistics of the intensity MSE
    ld = _lib.LossDesc(B=2, C=1, H=4, W=4, tB=1, tC=1)
    stats = _call.loss_stats(ld, "cpu")
    assert stats.dtype == torch.float32 and 4 * stats.numel() == L.thz_intensity_mse_workspace_size(ctypes.byref(ld)) > 0
    # a size of zero (the region statistics of planes without a pixel) still gives a pointer
    rd = _lib.RegionStatsDesc(N=1, H=0, W=4, dtype=_lib.METRICS_F32, K=0)
    assert L.thz_region_stats_workspace_size(ctypes.byref(rd), ctypes.byref(n)) == _lib.THZ_OK and n.value == 0
    assert _call.workspace(L.thz_region_stats_workspace_size, rd, device="cpu").numel() == 1


@pytest.mark.parametrize("module", sorted(OPTICS_PUBLIC))
def test_optics_reexports(module):
    from quantizationawarethzdoe_amd import optics
    mod = getattr(optics, module)
    assert mod.__doc__ and "csrc/thz_" in mod.__doc__ and "DESIGN" in mod.__doc__
    for name in OPTICS_PUBLIC[module]:
        assert getattr(optics, name) is getattr(mod, name), name


def test_optics_reexports_no_private_name():
    from quantizationawarethzdoe_amd import optics
    listed = {n for names in OPTICS_PUBLIC.values() for n in names} | set(OPTICS_PUBLIC)
    assert {n for n in vars(optics) if not n.startswith("__")} == listed
