"""ctypes binding of libthzdoe.so (include/thzdoe.h).

The shared library is built in-tree by ``quantizationawarethzdoe_amd/csrc/Makefile``
(``__graft_entry__.build()``).  There is NO fallback: if the library is missing or a
symbol is absent, every product entry point raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("THZDOE_LIB", os.path.join(_HERE, "libthzdoe.so"))

THZ_OK = 0
THZ_E_ARG = 1
THZ_E_UNSUPPORTED = 2
THZ_E_WORKSPACE = 3
THZ_E_HIP = 4
THZ_MAX_WAVELENGTHS = 64
THZ_MAX_Z = 256
THZ_ABI_VERSION = 9  # include/thzdoe.h: the descriptor layouts below

BANDLIMIT = {None: 0, False: 0, "none": 0, "exact": 1, "approx": 2}

# every symbol include/thzdoe.h declares (checked by tests/test_abi.py)
EXPORTED = [
    "thz_version", "thz_last_error", "thz_abi_version",
    "thz_asm_workspace_size", "thz_asm_forward", "thz_asm_band", "thz_asm_row_pairs", "thz_asm_forward_modulated",
    "thz_asm_forward_loss", "thz_asm_adjoint_loss", "thz_asm_transfer_function", "thz_rs_kernel",
    "thz_asm_slice_workspace_size", "thz_asm_slice_forward",
    "thz_asm_slice_adjoint_workspace_size", "thz_asm_slice_adjoint",
    "thz_czt_workspace_size", "thz_czt_forward",
    "thz_czt_slice_workspace_size", "thz_czt_slice_forward",
    "thz_czt_slice_adjoint_workspace_size", "thz_czt_slice_adjoint",
    "thz_rsc_workspace_size", "thz_rsc_forward",
    "thz_rsc_slice_workspace_size", "thz_rsc_slice_forward",
    "thz_rsc_slice_adjoint_workspace_size", "thz_rsc_slice_adjoint",
    "thz_thick_workspace_size", "thz_thick_forward",
    "thz_thick_forward_saved", "thz_thick_backward_workspace_size", "thz_thick_backward",
    "thz_doe_modulate_forward", "thz_doe_modulate_backward", "thz_quant_forward", "thz_quant_backward",
    "thz_doe_quant_backward", "thz_radial_quant_backward",
    "thz_radial_forward", "thz_radial_backward",
    "thz_gaussian_beam", "thz_thin_lens", "thz_aperture",
    "thz_intensity_mse_workspace_size", "thz_intensity_mse_forward", "thz_intensity_mse_backward",
    "thz_resample_forward", "thz_resample_backward",
    "thz_stokes_forward", "thz_stokes_backward", "thz_polarization_ellipse",
    "thz_stokes64_forward", "thz_polarization_ellipse64",
    "thz_noise_apply", "thz_noise_draws", "thz_signal_scale_workspace_size", "thz_signal_scale",
    "thz_snr_noise_backward",
    "thz_dice_bce_sums_workspace_size", "thz_dice_bce_sums", "thz_dice_bce_backward",
    "thz_ssim_workspace_size", "thz_ssim_forward", "thz_ssim_backward",
    "thz_lut_quantize_forward", "thz_lut_quantize_backward",
    "thz_tv_workspace_size", "thz_tv_forward", "thz_tv_backward",
    "thz_region_stats_workspace_size", "thz_region_stats_forward", "thz_region_stats_backward", "thz_line_widths",
    "thz_ifta_target_stats_workspace_size", "thz_ifta_target_stats", "thz_ifta_target_project", "thz_ifta_doe_project",
    "thz_fdtd_workspace_size", "thz_fdtd_setup", "thz_fdtd_run", "thz_fdtd_monitors", "thz_fdtd_fields",
    "thz_fdtd_material",
    "thz_tolerance_modulate_forward", "thz_tolerance_modulate_backward",
    "thz_fft_rows",
    "thz_asm64_workspace_size", "thz_asm64_forward", "thz_czt64_workspace_size", "thz_czt64_forward",
    "thz_rsc64_workspace_size", "thz_rsc64_forward", "thz_fft64_rows",
    "thz_step_fetch", "thz_adam_step",
    "thz_timing_enable", "thz_timing_reset", "thz_timing_read",
]


class ThzError(RuntimeError):
    """A libthzdoe call failed; carries the THZ_E_* code."""

    def __init__(self, code, msg):
        super().__init__(f"libthzdoe error {code}: {msg}")
        self.code = code


class AsmDesc(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("pad_h", ctypes.c_int), ("pad_w", ctypes.c_int),
        ("unpad", ctypes.c_int), ("bandlimit", ctypes.c_int), ("Z", ctypes.c_int),
        ("adjoint", ctypes.c_int), ("z_chunk", ctypes.c_int),
        ("dx", ctypes.c_float), ("dy", ctypes.c_float),
        ("wavelengths", ctypes.POINTER(ctypes.c_float)), ("z", ctypes.POINTER(ctypes.c_float)),
        ("window_mask", ctypes.c_void_p),  # const thz_aperture_desc* (ABI 5), NULL = none
        ("z_dev", ctypes.c_void_p),  # const float* device [Z] (ABI 6), NULL = the host z
    ]


class CztDesc(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("outH", ctypes.c_int), ("outW", ctypes.c_int),
        ("dx", ctypes.c_float), ("dy", ctypes.c_float), ("odx", ctypes.c_float), ("ody", ctypes.c_float),
        ("z", ctypes.c_float), ("wavelengths", ctypes.POINTER(ctypes.c_float)), ("adjoint", ctypes.c_int),
    ]


class CztSliceDesc(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("outH", ctypes.c_int), ("outW", ctypes.c_int),
        ("dx", ctypes.c_float), ("dy", ctypes.c_float), ("odx", ctypes.c_float), ("ody", ctypes.c_float),
        ("Z", ctypes.c_int), ("z", ctypes.POINTER(ctypes.c_float)),
        ("wavelengths", ctypes.POINTER(ctypes.c_float)), ("row", ctypes.c_int),
    ]


class RscDesc(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("vectorial", ctypes.c_int), ("dx", ctypes.c_float), ("dy", ctypes.c_float), ("z", ctypes.c_float),
        ("wavelengths", ctypes.POINTER(ctypes.c_float)), ("adjoint", ctypes.c_int),
    ]


class RscSliceDesc(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("vectorial", ctypes.c_int), ("dx", ctypes.c_float), ("dy", ctypes.c_float),
        ("Z", ctypes.c_int), ("z", ctypes.POINTER(ctypes.c_float)),
        ("wavelengths", ctypes.POINTER(ctypes.c_float)), ("row", ctypes.c_int),
    ]


class AsmDesc64(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("pad_h", ctypes.c_int), ("pad_w", ctypes.c_int),
        ("unpad", ctypes.c_int), ("bandlimit", ctypes.c_int), ("Z", ctypes.c_int), ("adjoint", ctypes.c_int),
        ("dx", ctypes.c_double), ("dy", ctypes.c_double),
        ("wavelengths", ctypes.POINTER(ctypes.c_double)), ("z", ctypes.POINTER(ctypes.c_double)),
    ]


class CztDesc64(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("outH", ctypes.c_int), ("outW", ctypes.c_int),
        ("dx", ctypes.c_double), ("dy", ctypes.c_double), ("odx", ctypes.c_double), ("ody", ctypes.c_double),
        ("z", ctypes.c_double), ("wavelengths", ctypes.POINTER(ctypes.c_double)), ("adjoint", ctypes.c_int),
    ]


class RscDesc64(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("vectorial", ctypes.c_int), ("dx", ctypes.c_double), ("dy", ctypes.c_double), ("z", ctypes.c_double),
        ("wavelengths", ctypes.POINTER(ctypes.c_double)), ("adjoint", ctypes.c_int),
    ]


class DoeDesc(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("hs", ctypes.c_int), ("ws", ctypes.c_int),
        ("tolerance", ctypes.c_float), ("epsilon", ctypes.c_float), ("tand", ctypes.c_float),
        ("wavelengths", ctypes.POINTER(ctypes.c_float)),
        ("rng", ctypes.c_void_p), ("rng_stream", ctypes.c_uint),
    ]


class ThickDesc(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("pad_h", ctypes.c_int), ("pad_w", ctypes.c_int), ("bandlimit", ctypes.c_int),
        ("hs", ctypes.c_int), ("ws", ctypes.c_int), ("slices", ctypes.c_int),
        ("thickness", ctypes.c_float), ("dx", ctypes.c_float), ("dy", ctypes.c_float),
        ("epsilon", ctypes.c_float), ("tand", ctypes.c_float), ("phase_sign", ctypes.c_float),
        ("wavelengths", ctypes.POINTER(ctypes.c_float)),
    ]


class QuantDesc(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int), ("hq", ctypes.c_int), ("wq", ctypes.c_int), ("mirror", ctypes.c_int),
        ("L", ctypes.c_int), ("lut", ctypes.POINTER(ctypes.c_float)),
        ("hmax", ctypes.c_float), ("clamp", ctypes.c_float), ("tau", ctypes.c_float),
        ("iter_frac", ctypes.c_float), ("c_s", ctypes.c_float), ("s", ctypes.c_float),
        ("beta", ctypes.c_float), ("phase_scale", ctypes.c_float), ("dyn", ctypes.c_void_p),
        ("rng", ctypes.c_void_p), ("rng_stream", ctypes.c_uint),
    ]


class GaussDesc(ctypes.Structure):
    _fields_ = [
        ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("dx", ctypes.c_float), ("dy", ctypes.c_float),
        ("wavelengths", ctypes.POINTER(ctypes.c_float)), ("waist_x", ctypes.POINTER(ctypes.c_float)),
        ("waist_y", ctypes.POINTER(ctypes.c_float)),
        ("x0", ctypes.c_float), ("y0", ctypes.c_float), ("z_w0x", ctypes.c_float), ("z_w0y", ctypes.c_float),
        ("alpha", ctypes.c_float),
    ]


class LensDesc(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("dx", ctypes.c_float), ("dy", ctypes.c_float), ("focal_length", ctypes.c_float),
        ("wavelengths", ctypes.POINTER(ctypes.c_float)),
    ]


class ApertureDesc(ctypes.Structure):
    _fields_ = [
        ("BC", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("kind", ctypes.c_int),
        ("dx", ctypes.c_float), ("dy", ctypes.c_float), ("half_w", ctypes.c_float), ("half_h", ctypes.c_float),
        ("radius", ctypes.c_float),
    ]


class LossDesc(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("tB", ctypes.c_int), ("tC", ctypes.c_int)]


class ResampleDesc(ctypes.Structure):
    _fields_ = [("BC", ctypes.c_int), ("Hin", ctypes.c_int), ("Win", ctypes.c_int), ("Hout", ctypes.c_int),
                ("Wout", ctypes.c_int), ("dx_in", ctypes.c_float), ("dy_in", ctypes.c_float),
                ("dx_out", ctypes.c_float), ("dy_out", ctypes.c_float)]


class NoiseDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("input", ctypes.c_int),
                ("sigma", ctypes.c_float), ("a", ctypes.c_float), ("gain", ctypes.c_float),
                ("normalize", ctypes.c_int),
                ("sigma_dev", ctypes.c_void_p),  # const float* device [1], NULL = the host sigma
                ("rng", ctypes.c_void_p), ("stream", ctypes.c_uint)]


class DiceBceDesc(ctypes.Structure):
    _fields_ = [("N", ctypes.c_longlong), ("M", ctypes.c_longlong),
                ("p", ctypes.c_float), ("smooth", ctypes.c_float),
                ("terms", ctypes.c_int), ("bce_grad_elementwise", ctypes.c_int),
                ("weight", ctypes.c_void_p), ("pos_weight", ctypes.c_void_p)]  # const float* device [N M] or NULL


SSIM_MAX_WIN = 33


class SsimDesc(ctypes.Structure):
    _fields_ = [("NC", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("ws", ctypes.c_int),
                ("window", ctypes.c_float * SSIM_MAX_WIN),
                ("C1", ctypes.c_double), ("C2", ctypes.c_double),
                ("nonnegative", ctypes.c_int), ("accumulate", ctypes.c_int)]


LOSS_TERM_DICE, LOSS_TERM_BCE = 1, 2

LUTQ_BUCKETIZE, LUTQ_ARGMIN = 0, 1
LUTQ_GRAD_IDENTITY, LUTQ_GRAD_POLY, LUTQ_GRAD_SIGMOID = 0, 1, 2

NOISE_GAUSS, NOISE_UNIFORM, NOISE_POISSON, NOISE_POISSON_GAUSS = 0, 1, 2, 3
NOISE_IN_REAL32, NOISE_IN_FIELD_INTENSITY, NOISE_IN_COMPLEX64 = 0, 1, 2
DRAW_NORMAL, DRAW_UNIFORM, DRAW_COMPLEX_NORMAL = 0, 1, 2

THZ_MAX_ADAM_PARAMS = 16


class AdamParam(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("step", ctypes.c_void_p), ("n", ctypes.c_longlong)]


class AdamDesc(ctypes.Structure):
    _fields_ = [("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double), ("decoupled", ctypes.c_int),
                ("nparams", ctypes.c_int),
                ("done", ctypes.c_void_p)]


APERTURE_RECT, APERTURE_CIRC = 1, 2

Q_FP, Q_STE, Q_PSQ, Q_SGV3, Q_NGS, Q_SGV1 = 0, 1, 2, 3, 4, 5
THZ_MAX_LUT = 16


class LutQuantizeDesc(ctypes.Structure):
    _fields_ = [("n", ctypes.c_longlong), ("mode", ctypes.c_int), ("wrap", ctypes.c_int), ("kind", ctypes.c_int),
                ("L", ctypes.c_int), ("T", ctypes.c_int),
                ("lut", ctypes.c_float * THZ_MAX_LUT), ("thresholds", ctypes.c_float * THZ_MAX_LUT)]


THZ_MAX_REGIONS = 16
REGION_CIRC, REGION_RECT = 0, 1
METRICS_C64, METRICS_C128, METRICS_F32, METRICS_F64 = 0, 1, 2, 3


class Region(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("cr", ctypes.c_float), ("cc", ctypes.c_float),
                ("a", ctypes.c_float), ("b", ctypes.c_float)]


class RegionStatsDesc(ctypes.Structure):
    _fields_ = [("N", ctypes.c_longlong), ("H", ctypes.c_int), ("W", ctypes.c_int), ("dtype", ctypes.c_int),
                ("K", ctypes.c_int), ("regions", ctypes.c_void_p),  # const thz_region* [K], host or device
                ("regions_on_device", ctypes.c_int)]


class IftaDesc(ctypes.Structure):
    _fields_ = [("N", ctypes.c_longlong), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("target_planes", ctypes.c_longlong),  # 1: T [H, W]; N: T [N, H, W]
                ("alpha", ctypes.c_double), ("beta", ctypes.c_double)]


class IftaDoeDesc(ctypes.Structure):
    _fields_ = [("N", ctypes.c_longlong), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("hs", ctypes.c_int), ("ws", ctypes.c_int),
                ("incident_planes", ctypes.c_longlong),  # 0: none; 1: A [H, W]; N: A [N, H, W]
                ("wavelength", ctypes.c_float), ("epsilon", ctypes.c_float),
                ("L", ctypes.c_int), ("lut", ctypes.c_float * THZ_MAX_LUT)]


THZ_FDTD_MAX_PLANES = 8


class FdtdDesc(ctypes.Structure):
    _fields_ = [("Nz", ctypes.c_int), ("Ny", ctypes.c_int), ("Nx", ctypes.c_int),
                ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("pixel", ctypes.c_double), ("delta", ctypes.c_double), ("courant", ctypes.c_double),
                ("npml", ctypes.c_int), ("k_elem", ctypes.c_int), ("n_base", ctypes.c_int), ("element", ctypes.c_int),
                ("thickness", ctypes.c_float), ("k_src", ctypes.c_int), ("polarization", ctypes.c_int),
                ("n_planes", ctypes.c_int), ("plane_k", ctypes.c_int * THZ_FDTD_MAX_PLANES),
                ("row", ctypes.c_int), ("col", ctypes.c_int),
                ("n_table", ctypes.c_longlong), ("n_acc", ctypes.c_int),
                ("step_table", ctypes.c_void_p),  # const double* host [n_table][5]
                ("cpml", ctypes.c_void_p),        # const float* host [8][npml]
                ("cacb", ctypes.c_void_p)]        # const float* host [10]


TOL_TAG_SCALE, TOL_TAG_LEVEL, TOL_TAG_ROUGH = 0x5343414C, 0x4C45564C, 0x524F5547  # "SCAL", "LEVL", "ROUG"
TOL_ROUGH_NONE, TOL_ROUGH_UNIFORM, TOL_ROUGH_NORMAL = 0, 1, 2


class ToleranceDesc(ctypes.Structure):
    _fields_ = [("K", ctypes.c_int), ("first", ctypes.c_longlong), ("Bf", ctypes.c_int),
                ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("hs", ctypes.c_int), ("ws", ctypes.c_int),
                ("L", ctypes.c_int), ("sigma_level", ctypes.c_float * THZ_MAX_LUT),
                ("sigma_scale", ctypes.c_float), ("rough_kind", ctypes.c_int), ("rough", ctypes.c_float),
                ("lo", ctypes.c_float), ("hi", ctypes.c_float),
                ("epsilon", ctypes.c_float), ("tand", ctypes.c_float),
                ("wavelengths", ctypes.POINTER(ctypes.c_float)),  # host [C]
                ("rng", ctypes.c_void_p), ("stream", ctypes.c_uint)]


_lib = None
_lock = threading.Lock()


def _declare(lib):
    c_int, c_void_p, c_size_t = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    lib.thz_version.restype = ctypes.c_char_p
    lib.thz_last_error.restype = ctypes.c_char_p
    lib.thz_asm_workspace_size.argtypes = [ctypes.POINTER(AsmDesc), ctypes.POINTER(c_size_t)]
    lib.thz_asm_forward.argtypes = [ctypes.POINTER(AsmDesc), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.thz_asm_slice_workspace_size.argtypes = [ctypes.POINTER(AsmDesc), ctypes.POINTER(c_size_t)]
    lib.thz_asm_slice_forward.argtypes = [ctypes.POINTER(AsmDesc), c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                          c_void_p]
    lib.thz_asm_slice_adjoint_workspace_size.argtypes = [ctypes.POINTER(AsmDesc), ctypes.POINTER(c_size_t)]
    lib.thz_asm_slice_adjoint.argtypes = [ctypes.POINTER(AsmDesc), c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                          c_void_p]
    lib.thz_asm_band.argtypes = [ctypes.POINTER(AsmDesc), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    lib.thz_asm_forward_modulated.argtypes = [ctypes.POINTER(AsmDesc), ctypes.POINTER(DoeDesc), c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.thz_asm_forward_loss.argtypes = [ctypes.POINTER(AsmDesc), ctypes.POINTER(DoeDesc), c_void_p, c_void_p,
                                         c_void_p, c_void_p, ctypes.POINTER(LossDesc), c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_size_t, c_void_p]
    lib.thz_asm_adjoint_loss.argtypes = [ctypes.POINTER(AsmDesc), ctypes.POINTER(LossDesc), c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.thz_fft_rows.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]
    lib.thz_rsc_workspace_size.argtypes = [ctypes.POINTER(RscDesc), ctypes.POINTER(c_size_t)]
    lib.thz_rsc_forward.argtypes = [ctypes.POINTER(RscDesc), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.thz_rsc_slice_workspace_size.argtypes = [ctypes.POINTER(RscSliceDesc), ctypes.POINTER(c_size_t)]
    lib.thz_rsc_slice_forward.argtypes = [ctypes.POINTER(RscSliceDesc), c_void_p, c_void_p, c_void_p, c_size_t,
                                          c_void_p]
    lib.thz_rsc_slice_adjoint_workspace_size.argtypes = [ctypes.POINTER(RscSliceDesc), ctypes.POINTER(c_size_t)]
    lib.thz_rsc_slice_adjoint.argtypes = [ctypes.POINTER(RscSliceDesc), c_void_p, c_void_p, c_void_p, c_size_t,
                                          c_void_p]
    lib.thz_thick_workspace_size.argtypes = [ctypes.POINTER(ThickDesc), ctypes.POINTER(c_size_t)]
    lib.thz_thick_forward.argtypes = [ctypes.POINTER(ThickDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p]
    lib.thz_thick_forward_saved.argtypes = [ctypes.POINTER(ThickDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_size_t, c_void_p]
    lib.thz_thick_backward_workspace_size.argtypes = [ctypes.POINTER(ThickDesc), ctypes.POINTER(c_size_t)]
    lib.thz_thick_backward.argtypes = [ctypes.POINTER(ThickDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_size_t, c_void_p]
    lib.thz_doe_modulate_forward.argtypes = [ctypes.POINTER(DoeDesc), c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p]
    lib.thz_doe_modulate_backward.argtypes = [ctypes.POINTER(DoeDesc), c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p]
    lib.thz_quant_forward.argtypes = [ctypes.POINTER(QuantDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.thz_quant_backward.argtypes = [ctypes.POINTER(QuantDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.thz_doe_quant_backward.argtypes = [ctypes.POINTER(DoeDesc), ctypes.POINTER(QuantDesc), c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.thz_radial_quant_backward.argtypes = [ctypes.POINTER(QuantDesc), c_void_p, c_int, c_int, c_int, c_void_p,
                                              c_void_p, c_void_p, c_void_p]
    lib.thz_radial_forward.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.thz_radial_backward.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.thz_czt_workspace_size.argtypes = [ctypes.POINTER(CztDesc), ctypes.POINTER(c_size_t)]
    lib.thz_czt_forward.argtypes = [ctypes.POINTER(CztDesc), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.thz_czt_slice_workspace_size.argtypes = [ctypes.POINTER(CztSliceDesc), ctypes.POINTER(c_size_t)]
    lib.thz_czt_slice_forward.argtypes = [ctypes.POINTER(CztSliceDesc), c_void_p, c_void_p, c_void_p, c_size_t,
                                          c_void_p]
    lib.thz_czt_slice_adjoint_workspace_size.argtypes = [ctypes.POINTER(CztSliceDesc), ctypes.POINTER(c_size_t)]
    lib.thz_czt_slice_adjoint.argtypes = [ctypes.POINTER(CztSliceDesc), c_void_p, c_void_p, c_void_p, c_size_t,
                                          c_void_p]
    lib.thz_gaussian_beam.argtypes = [ctypes.POINTER(GaussDesc), c_void_p, c_void_p]
    lib.thz_thin_lens.argtypes = [ctypes.POINTER(LensDesc), c_void_p, c_void_p, c_void_p]
    lib.thz_aperture.argtypes = [ctypes.POINTER(ApertureDesc), c_void_p, c_void_p, c_void_p]
    lib.thz_asm_transfer_function.argtypes = [ctypes.POINTER(AsmDesc), c_void_p, c_void_p]
    lib.thz_rs_kernel.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_void_p, c_int, c_void_p, c_void_p]
    lib.thz_intensity_mse_workspace_size.argtypes = [ctypes.POINTER(LossDesc)]
    lib.thz_intensity_mse_forward.argtypes = [ctypes.POINTER(LossDesc), c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p]
    lib.thz_intensity_mse_backward.argtypes = [ctypes.POINTER(LossDesc), c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p]
    lib.thz_resample_forward.argtypes = [ctypes.POINTER(ResampleDesc), c_void_p, c_void_p, c_void_p]
    lib.thz_resample_backward.argtypes = [ctypes.POINTER(ResampleDesc), c_void_p, c_void_p, c_void_p]
    for name in ("thz_stokes_forward", "thz_polarization_ellipse", "thz_stokes64_forward",
                 "thz_polarization_ellipse64"):  # ex, ey, n, out, stream
        getattr(lib, name).argtypes = [c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p]
    lib.thz_stokes_backward.argtypes = [c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p]
    c_ll, c_uint, c_float = ctypes.c_longlong, ctypes.c_uint, ctypes.c_float
    lib.thz_noise_apply.argtypes = [ctypes.POINTER(NoiseDesc), c_void_p, c_void_p, c_ll, c_void_p]
    lib.thz_noise_draws.argtypes = [c_int, c_void_p, c_uint, c_ll, c_void_p, c_void_p]
    lib.thz_signal_scale_workspace_size.argtypes = [c_ll, ctypes.POINTER(c_size_t)]
    lib.thz_signal_scale.argtypes = [c_void_p, c_ll, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.thz_snr_noise_backward.argtypes = [c_void_p, c_void_p, c_ll, c_int, c_float, c_void_p, c_void_p, c_uint,
                                           c_void_p, c_void_p, c_size_t, c_void_p]
    lib.thz_dice_bce_sums_workspace_size.argtypes = [ctypes.POINTER(DiceBceDesc), ctypes.POINTER(c_size_t)]
    lib.thz_dice_bce_sums.argtypes = [ctypes.POINTER(DiceBceDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_size_t, c_void_p]
    lib.thz_dice_bce_backward.argtypes = [ctypes.POINTER(DiceBceDesc), c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p]
    lib.thz_ssim_workspace_size.argtypes = [ctypes.POINTER(SsimDesc), ctypes.POINTER(c_size_t)]
    lib.thz_ssim_forward.argtypes = [ctypes.POINTER(SsimDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_size_t, c_void_p]
    lib.thz_ssim_backward.argtypes = [ctypes.POINTER(SsimDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p]
    lib.thz_lut_quantize_forward.argtypes = [ctypes.POINTER(LutQuantizeDesc), c_void_p, c_void_p, c_void_p, c_void_p]
    lib.thz_lut_quantize_backward.argtypes = [ctypes.POINTER(LutQuantizeDesc), c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p]
    lib.thz_tv_workspace_size.argtypes = [c_ll, c_int, c_int, ctypes.POINTER(c_size_t)]
    lib.thz_tv_forward.argtypes = [c_void_p, c_ll, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                   c_void_p]
    lib.thz_tv_backward.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int, c_void_p, c_void_p]
    lib.thz_region_stats_workspace_size.argtypes = [ctypes.POINTER(RegionStatsDesc), ctypes.POINTER(c_size_t)]
    lib.thz_region_stats_forward.argtypes = [ctypes.POINTER(RegionStatsDesc), c_void_p, c_void_p, c_void_p, c_size_t,
                                             c_void_p]
    lib.thz_region_stats_backward.argtypes = [ctypes.POINTER(RegionStatsDesc), c_void_p, c_void_p, c_void_p, c_void_p]
    lib.thz_line_widths.argtypes = [c_void_p, c_int, c_ll, c_int, ctypes.c_double, c_void_p, c_void_p]
    lib.thz_ifta_target_stats_workspace_size.argtypes = [ctypes.POINTER(IftaDesc), ctypes.POINTER(c_size_t)]
    lib.thz_ifta_target_stats.argtypes = [ctypes.POINTER(IftaDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_size_t, c_void_p]
    lib.thz_ifta_target_project.argtypes = [ctypes.POINTER(IftaDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p]
    lib.thz_ifta_doe_project.argtypes = [ctypes.POINTER(IftaDoeDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p]
    fd = ctypes.POINTER(FdtdDesc)
    lib.thz_fdtd_workspace_size.argtypes = [fd, ctypes.POINTER(c_size_t)]
    lib.thz_fdtd_setup.argtypes = [fd, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.thz_fdtd_run.argtypes = [fd, c_void_p, c_size_t, c_ll, c_void_p]
    lib.thz_fdtd_monitors.argtypes = [fd, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.thz_fdtd_fields.argtypes = [fd, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.thz_fdtd_material.argtypes = [fd, c_void_p, c_size_t, c_void_p, c_void_p]
    td = ctypes.POINTER(ToleranceDesc)
    lib.thz_tolerance_modulate_forward.argtypes = [td, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.thz_tolerance_modulate_backward.argtypes = [td, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_size_t, c_void_p]
    for tag, desc in (("asm64", AsmDesc64), ("czt64", CztDesc64), ("rsc64", RscDesc64)):
        getattr(lib, f"thz_{tag}_workspace_size").argtypes = [ctypes.POINTER(desc), ctypes.POINTER(c_size_t)]
        getattr(lib, f"thz_{tag}_forward").argtypes = [ctypes.POINTER(desc), c_void_p, c_void_p, c_void_p, c_size_t,
                                                       c_void_p]
    lib.thz_fft64_rows.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]
    lib.thz_step_fetch.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.thz_adam_step.argtypes = [ctypes.POINTER(AdamDesc), ctypes.POINTER(AdamParam), c_void_p]
    lib.thz_asm_row_pairs.argtypes = [c_int]
    lib.thz_timing_enable.argtypes = [c_int]
    lib.thz_timing_reset.argtypes = []
    lib.thz_timing_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
    for name in EXPORTED[2:]:
        getattr(lib, name).restype = c_int
    lib.thz_intensity_mse_workspace_size.restype = c_size_t


def lib():
    """Load (once) and return the ctypes handle; raise loudly if it cannot be loaded."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise ThzError(-1, f"{LIB_PATH} not built: run __graft_entry__.build() "
                                       "(make -C quantizationawarethzdoe_amd/csrc)")
                h = ctypes.CDLL(LIB_PATH)
                _declare(h)
                abi = h.thz_abi_version()
                if abi != THZ_ABI_VERSION:
                    raise ThzError(-1, f"{LIB_PATH} has ABI {abi}, these bindings describe ABI {THZ_ABI_VERSION}: "
                                       "rebuild the library (make -C quantizationawarethzdoe_amd/csrc)")
                _lib = h
    return _lib


def check(code):
    if code != THZ_OK:
        raise ThzError(code, lib().thz_last_error().decode())


def version():
    return lib().thz_version().decode()


def timing_enable(on=True):
    check(lib().thz_timing_enable(int(bool(on))))


def asm_row_pairs(mode=-1):
    """Form of the ASM inverse row pass: -1 the library's choice, 0 one row, 1 two rows per workgroup."""
    check(lib().thz_asm_row_pairs(int(mode)))


def timing_reset():
    check(lib().thz_timing_reset())


def timing_read(kernel):
    """(total_ms, launches) of one kernel since the last reset; synchronises pending events."""
    ms, n = ctypes.c_double(0), ctypes.c_long(0)
    check(lib().thz_timing_read(kernel.encode(), ctypes.byref(ms), ctypes.byref(n)))
    return ms.value, n.value


def double_array(values):
    return (ctypes.c_double * max(1, len(values)))(*[float(v) for v in values])


def float_array(values):
    arr = (ctypes.c_float * max(1, len(values)))(*[float(v) for v in values])
    return arr
