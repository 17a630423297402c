"""Device entry points of everything that is not a propagator or a DOE layer, one module per csrc unit (the map
is in DESIGN §36).  The public names are re-exported here: ``optics.NAME`` is ``optics.<module>.NAME``.  Helpers
that sibling modules, tests and timing scripts share (``heightmap.lut_desc``, ``metrics.region_table``, ...) are
reached by their module's path.
"""
from . import elements, heightmap, ifta, losses, metrics, noise, polarization, thick, tolerance
from .elements import aperture, field_intensity_mse, gaussian_beam, intensity_mse, resample, thin_lens
from .heightmap import center_difference, lut_quantize, total_variation
from .ifta import IFTA_STATS, ifta_doe_project, ifta_target_project, ifta_target_stats
from .losses import bce_with_logits, dice_loss, hierarchy_loss, ssim
from .metrics import LineWidths, RegionStats, line_widths, region_stats
from .noise import NOISE_KINDS, add_noise, detect, noise_draws, signal_scale
from .polarization import POLARIZATION_EPS, polarization_ellipse, stokes
from .thick import THICK_CONVENTIONS, thick_doe, thick_doe_native
from .tolerance import TOLERANCE_ROUGHNESS, tolerance_modulate
