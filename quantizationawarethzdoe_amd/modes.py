"""Gaussian-mode analysis: Hermite-Gauss decomposition and synthesis of a field, a module of this port alone like
hankel.py and ifta.py (csrc/thz_modes.hip).  The overlap integrals of every plane with M x N modes are two
chained products with one real table per axis on the fp32 matrix cores; the field is read once and the intermediate
never leaves the chip.  The model is stated in include/thzdoe.h; utils/metrics.py builds Gaussicity, the modal power
spectrum and the mode filter on it.

Conventions, those of ``ElectricField`` and ``Guassian_beam``: ``spacing`` is a scalar or (dx, dy), ``center`` is
(x0, y0) in metres from the plane's centre pixel, x runs along the last dimension.  Pixel j of n sits at
(j - (n - 1) / 2) pitch, the coordinates of utils/metrics.py -- not the linspace(-L / 2, L / 2, n) of ``Guassian_beam``,
whose pitch is L / (n - 1).  ``waist`` is a scalar, a list / tensor [C] (one per wavelength channel, both axes) or a
tuple (wx, wy) of scalars or [C] sequences; they are host numbers (a device tensor would be read back).  The modes
are those of a beam at its waist: remove a field's curvature first (``optics.thin_lens``).
"""
import torch

from . import _lib
from ._call import _require_device, call, workspace

_TABLES = {}  # (n_modes, n_pix, pitch, centre, waists, device index) -> G: what the kernels use, exported once


def _seq(v, C, who):
    vals = [float(x) for x in torch.as_tensor(v, dtype=torch.float64).reshape(-1).tolist()]
    if len(vals) == 1:
        vals = vals * C
    if len(vals) != C:
        raise ValueError(f"{who}: {len(vals)} waists for {C} channels")
    if not all(x > 0 for x in vals):
        raise ValueError(f"{who}: waists must be positive; got {vals}")
    return tuple(vals)


def _waists(waist, C, who):
    """(wx [C], wy [C]) as tuples of floats"""
    if waist is None:
        raise ValueError(f"{who}: the modes need a waist")
    if isinstance(waist, tuple):
        if len(waist) != 2:
            raise ValueError(f"{who}: a tuple waist is (wx, wy)")
        return _seq(waist[0], C, who), _seq(waist[1], C, who)
    w = _seq(waist, C, who)
    return w, w


def _pair(v, who, what):
    vals = [float(x) for x in torch.as_tensor(v, dtype=torch.float64).reshape(-1).tolist()]
    if len(vals) not in (1, 2):
        raise ValueError(f"{who}: {what} is a scalar or a pair; got {v!r}")
    return vals[0], vals[-1]


def _orders(orders, who):
    M, N = (int(orders), int(orders)) if isinstance(orders, int) else (int(orders[0]), int(orders[1]))
    if not (1 <= M <= _lib.HG_MAX_ORDER and 1 <= N <= _lib.HG_MAX_ORDER):
        raise ValueError(f"{who}: orders (M, N) = ({M}, {N}) outside 1 .. {_lib.HG_MAX_ORDER}")
    return M, N


def as_field(field, spacing, who):
    """(complex64 [B, C, H, W] tensor, (dx, dy)) of a tensor or an ElectricField (whose spacing serves when none is
    given)"""
    if not torch.is_tensor(field) and hasattr(field, "data"):
        spacing = field.spacing_host if spacing is None else spacing
        field = field.data
    if not torch.is_tensor(field):
        raise TypeError(f"{who}: the field must be a tensor or an ElectricField")
    _require_device(field, who)
    if field.dtype == torch.complex128:
        raise TypeError(f"{who}: the kernels compute in complex64; got a complex128 field -- cast it, an fp64 "
                        "variant does not exist")
    if field.dtype != torch.complex64 or field.dim() != 4:
        raise TypeError(f"{who}: the field is complex64 [B, C, H, W]; got {field.dtype} {tuple(field.shape)}")
    if spacing is None:
        raise ValueError(f"{who}: a tensor needs its spacing")
    return field, _pair(spacing, who, "spacing")


def hg_table(n_modes, n_pix, pitch, waists, centre, device):
    """G float32 [C, n_modes, n_pix], the modes u_k(x_j) of one axis at ``waists`` [C] as the kernels hold them on
    ``device`` (thz_hg_table).  The first call for a key builds the table on the host in extended precision -- a
    blocking step -- and every later call, of the transforms too, only launches."""
    who = "hg_table"
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who}: the MI355X path needs a ROCm device (got device {device}); "
                           "this framework has no CPU compute path")
    n_modes, n_pix, pitch, centre = int(n_modes), int(n_pix), float(pitch), float(centre)
    ws = tuple(float(w) for w in waists)
    key = (n_modes, n_pix, pitch, centre, ws, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _TABLES:
        _orders((n_modes, n_modes), who)
        if n_pix < 1:
            raise ValueError(f"{who}: n_pix = {n_pix}")
        G = torch.empty(len(ws), n_modes, n_pix, dtype=torch.float32, device=device)
        call(_lib.lib().thz_hg_table, n_modes, n_pix, pitch, centre, _lib.double_array(ws), len(ws), G, device=device)
        _TABLES[key] = G
    return _TABLES[key]


def _desc(cfg, scale):
    (B, C, H, W), (M, N), (dx, dy), (x0, y0), (wx, wy) = cfg
    ax, ay = _lib.double_array(wx), _lib.double_array(wy)
    d = _lib.HgDesc(B=B, C=C, H=H, W=W, M=M, N=N, dx=dx, dy=dy, x0=x0, y0=y0, waist_x=ax, waist_y=ay, scale=scale)
    d._keep = (ax, ay)
    return d


def _analyze(field, cfg, scale):
    (B, C, _, _), (M, N) = cfg[0], cfg[1]
    d = _desc(cfg, scale)
    out = torch.empty(B, C, M, N, dtype=torch.complex64, device=field.device)
    ws = workspace(_lib.lib().thz_hg_workspace_size, d, device=field.device)
    call(_lib.lib().thz_hg_analyze, d, field.contiguous(), out, ws, ws.numel(), device=field.device)
    return out


def _synthesize(coeffs, cfg, scale):
    B, C, H, W = cfg[0]
    out = torch.empty(B, C, H, W, dtype=torch.complex64, device=coeffs.device)
    call(_lib.lib().thz_hg_synthesize, _desc(cfg, scale), coeffs.contiguous(), out, device=coeffs.device)
    return out


class _Decompose(torch.autograd.Function):
    """c of thz_hg_analyze; the tables are real, so the backward is thz_hg_synthesize at the same scale."""

    @staticmethod
    def forward(ctx, field, cfg, scale):
        ctx.cfg = (cfg, scale)
        return _analyze(field, cfg, scale)

    @staticmethod
    def backward(ctx, g):
        return _Synthesize.apply(g.resolve_conj(), *ctx.cfg), None, None


class _Synthesize(torch.autograd.Function):
    """U of thz_hg_synthesize; the backward is thz_hg_analyze at the same scale."""

    @staticmethod
    def forward(ctx, coeffs, cfg, scale):
        ctx.cfg = (cfg, scale)
        return _synthesize(coeffs, cfg, scale)

    @staticmethod
    def backward(ctx, g):
        return _Decompose.apply(g.resolve_conj(), *ctx.cfg), None, None


def _cfg(shape, orders, spacing, waist, center, who):
    B, C, H, W = (int(v) for v in shape)
    return ((B, C, H, W), _orders(orders, who), _pair(spacing, who, "spacing"), _pair(center, who, "center"),
            _waists(waist, C, who))


def hg_decompose(field, spacing=None, waist=None, orders=(1, 1), center=(0.0, 0.0)):
    """The Hermite-Gauss coefficients of every plane: ``field`` complex64 [B, C, H, W] (or an ElectricField, whose
    spacing serves when none is given) -> complex64 [B, C, M, N], c[m, n] = dx dy sum_ij u_m(y_i) U[i, j] u_n(x_j), the
    overlap integral with the normalised mode of order m along y and n along x (thz_hg_analyze).  |c|^2 summed over
    all modes is the field's power dx dy sum |U|^2 once M x N modes hold it.  Conventions in the module's docstring.

    Gradients flow to ``field`` (thz_hg_synthesize).  The first call for a geometry builds two tables on the host and
    copies them: that call blocks and cannot be captured.  Every later call has no host sync and is capturable in
    torch.cuda.graph.  A repeated call gives the same bits, and B x C planes in one call the bits of the planes one
    at a time."""
    who = "hg_decompose"
    x, spacing = as_field(field, spacing, who)
    cfg = _cfg(x.shape, orders, spacing, waist, center, who)
    return _Decompose.apply(x.resolve_conj(), cfg, cfg[2][0] * cfg[2][1])


def hg_synthesize(coeffs, shape, spacing, waist, center=(0.0, 0.0)):
    """The field of a set of Hermite-Gauss coefficients: ``coeffs`` complex64 [B, C, M, N] -> complex64 [B, C, H, W]
    with ``shape`` = (H, W), U[i, j] = sum_mn c[m, n] u_m(y_i) u_n(x_j) (thz_hg_synthesize): a higher-order-mode
    source, and with ``hg_decompose`` a mode filter.  Gradients flow to ``coeffs`` (thz_hg_analyze).  Blocking first
    call, capture and bits as for ``hg_decompose``."""
    who = "hg_synthesize"
    if not torch.is_tensor(coeffs):
        raise TypeError(f"{who}: coeffs must be a tensor")
    _require_device(coeffs, who)
    if coeffs.dtype == torch.complex128:
        raise TypeError(f"{who}: the kernels compute in complex64; got complex128 coefficients -- cast them, an fp64 "
                        "variant does not exist")
    if coeffs.dtype != torch.complex64 or coeffs.dim() != 4:
        raise TypeError(f"{who}: coeffs are complex64 [B, C, M, N]; got {coeffs.dtype} {tuple(coeffs.shape)}")
    B, C, M, N = coeffs.shape
    H, W = int(shape[-2]), int(shape[-1])
    if H < 1 or W < 1:
        raise ValueError(f"{who}: shape (H, W) = ({H}, {W})")
    cfg = _cfg((B, C, H, W), (M, N), spacing, waist, center, who)
    return _Synthesize.apply(coeffs.resolve_conj(), cfg, 1.0)
