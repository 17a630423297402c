"""Zernike wavefront analysis over a circular pupil: projection, least-squares fit, form removal and synthesis of
float32 maps, a module of this port alone like modes.py and hankel.py (csrc/thz_zernike.hip).  The basis
is never stored: the kernels generate every pixel's K values, hold them in LDS and multiply on the fp32 matrix cores.
The model (OSA / ANSI index, orthonormal on the unit disk, the recurrences and their precisions) is stated in
include/thzdoe.h; utils/metrics.py builds ``wavefront_rms`` and Components/ZernikeDOE.py a Zernike-parameterised
element on it.

Conventions, those of modes.py: ``spacing`` is a scalar or (dx, dy), ``pupil`` is (x0, y0, R) in metres from the
plane's centre pixel, x runs along the last dimension, pixel j of n sits at (j - (n - 1) / 2) pitch.  Maps are float32
[B, H, W] (or [H, W], returned as given); ``max_order`` is the largest radial order n, 0 ... 14, and
K = (n + 1) (n + 2) / 2 modes are numbered k = (n (n + 2) + m) / 2.  Pupil and spacing are host numbers.
"""
import torch

from . import _lib
from ._call import _require_device, call, workspace

_GRAMS = {}   # (H, W, dx, dy, pupil, max_order, device index) -> (G float32 [K, K], its fp64 Cholesky factor)
_FULL = set()  # geometries whose pupil was counted on the host and holds at least K pixels
_MASKS = {}   # (H, W, dx, dy, pupil, device index) -> Z_0, float32 [H, W]: 1 inside the pupil, 0 outside


def index(n, m):
    """The OSA / ANSI index k = (n (n + 2) + m) / 2 of radial order n and azimuthal order m."""
    n, m = int(n), int(m)
    if n < 0 or abs(m) > n or (n - m) % 2:
        raise ValueError(f"zernike.index: no mode (n, m) = ({n}, {m})")
    return (n * (n + 2) + m) // 2


def orders(k):
    """(n, m) of the OSA / ANSI index k."""
    k = int(k)
    if k < 0:
        raise ValueError(f"zernike.orders: k = {k}")
    n = 0
    while (n + 1) * (n + 2) // 2 <= k:
        n += 1
    return n, 2 * k - n * (n + 2)


def num_modes(max_order):
    """K = (n + 1) (n + 2) / 2 modes up to radial order ``max_order``."""
    n = int(max_order)
    if not 0 <= n <= _lib.ZERNIKE_MAX_ORDER:
        raise ValueError(f"zernike: max_order = {n} outside 0 .. {_lib.ZERNIKE_MAX_ORDER}")
    return (n + 1) * (n + 2) // 2


def _pair(v, who):
    vals = [float(x) for x in torch.as_tensor(v, dtype=torch.float64).reshape(-1).tolist()]
    if len(vals) not in (1, 2):
        raise ValueError(f"{who}: spacing is a scalar or (dx, dy); got {v!r}")
    if not all(0 < x < float("inf") for x in vals):
        raise ValueError(f"{who}: spacing must be positive; got {v!r}")
    return vals[0], vals[-1]


def _geometry(shape, spacing, pupil, max_order, who):
    """(H, W, dx, dy, x0, y0, R, max_order): checked host numbers, the cache key of a geometry"""
    H, W = int(shape[-2]), int(shape[-1])
    if H < 1 or W < 1:
        raise ValueError(f"{who}: shape (H, W) = ({H}, {W})")
    num_modes(max_order)
    x0, y0, R = (float(v) for v in pupil)
    if not 0 < R < float("inf"):
        raise ValueError(f"{who}: the pupil radius R = {R} must be positive")
    return (H, W) + _pair(spacing, who) + (x0, y0, R, int(max_order))


def pupil_pixels(shape, spacing, pupil):
    """How many pixels the pupil holds, counted on the host (row by row: no H x W array)."""
    H, W, dx, dy, x0, y0, R, _ = _geometry(shape, spacing, pupil, 0, "pupil_pixels")
    x = (torch.arange(W, dtype=torch.float64) - (W - 1) / 2) * dx - x0
    y = (torch.arange(H, dtype=torch.float64) - (H - 1) / 2) * dy - y0
    return int(torch.searchsorted((x * x).sort().values, R * R - y * y, right=True).sum())


def _desc(geo, B):
    H, W, dx, dy, x0, y0, R, n = geo
    return _lib.ZernikeDesc(B=B, H=H, W=W, max_order=n, dx=dx, dy=dy, x0=x0, y0=y0, R=R)


def _dev_index(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"zernike: the MI355X path needs a ROCm device (got device {device}); "
                           "this framework has no CPU compute path")
    return device, device.index if device.index is not None else torch.cuda.current_device()


def _maps(w, who):
    """(float32 [B, H, W] view, whether the caller's map was [H, W])"""
    if not torch.is_tensor(w):
        raise TypeError(f"{who}: the maps must be a tensor")
    if w.dtype == torch.float64:
        raise TypeError(f"{who}: the kernels compute in float32; got a float64 map -- cast it, an fp64 variant "
                        "does not exist")
    if w.dtype != torch.float32 or w.dim() not in (2, 3):
        raise TypeError(f"{who}: the maps are float32 [B, H, W] or [H, W]; got {w.dtype} {tuple(w.shape)}")
    return (w[None], True) if w.dim() == 2 else (w, False)


def _project(w, geo, device, gram=False):
    """S [B, K] of the maps ``w`` (or None) and, with ``gram``, G [K, K]; one entry call"""
    K = num_modes(geo[-1])
    d = _desc(geo, 1 if w is None else w.shape[0])
    out = None if w is None else torch.empty(w.shape[0], K, dtype=torch.float32, device=device)
    G = torch.empty(K, K, dtype=torch.float32, device=device) if gram else None
    ws = workspace(_lib.lib().thz_zernike_workspace_size, d, int(G is not None), device=device)
    call(_lib.lib().thz_zernike_project, d, None if w is None else w.contiguous(), out, G, ws, ws.numel(), device=device)
    return out, G


def _synthesize(coeffs, geo):
    out = torch.empty(coeffs.shape[0], geo[0], geo[1], dtype=torch.float32, device=coeffs.device)
    call(_lib.lib().thz_zernike_synthesize, _desc(geo, coeffs.shape[0]), coeffs.contiguous(), out, device=coeffs.device)
    return out


class _Project(torch.autograd.Function):
    """S of thz_zernike_project; Z is real, so the backward is thz_zernike_synthesize."""

    @staticmethod
    def forward(ctx, w, geo):
        ctx.geo = geo
        return _project(w, geo, w.device)[0]

    @staticmethod
    def backward(ctx, g):
        return _Synthesize.apply(g, ctx.geo), None


class _Synthesize(torch.autograd.Function):
    """w of thz_zernike_synthesize; the backward is thz_zernike_project."""

    @staticmethod
    def forward(ctx, coeffs, geo):
        ctx.geo = geo
        return _synthesize(coeffs, geo)

    @staticmethod
    def backward(ctx, g):
        return _Project.apply(g, ctx.geo), None


def zernike_table(shape, spacing, pupil, max_order, device):
    """Z float32 [K, H, W] exactly as the kernels generate it (thz_zernike_table): for tests and plots, never for the
    hot path -- at K = 120 and 2048^2 it is 2 GB."""
    geo = _geometry(shape, spacing, pupil, max_order, "zernike_table")
    device, _ = _dev_index(device)
    out = torch.empty(num_modes(max_order), geo[0], geo[1], dtype=torch.float32, device=device)
    call(_lib.lib().thz_zernike_table, _desc(geo, 1), out, device=device)
    return out


def project(w, spacing, pupil, max_order):
    """S[b, k] = sum over the pupil's pixels of Z_k w[b], float32 [B, K] (thz_zernike_project): inner products, not
    yet coefficients -- on a pixel grid the modes are only approximately orthogonal (``fit``).  Gradients flow to
    ``w`` (thz_zernike_synthesize).  No host sync, capturable; a repeated call gives the same bits, and B planes in
    one call the bits of the planes one at a time."""
    x, single = _maps(w, "zernike.project")
    geo = _geometry(x.shape, spacing, pupil, max_order, "zernike.project")
    _require_device(x, "zernike.project")
    out = _Project.apply(x, geo)
    return out[0] if single else out


def synthesize(coeffs, shape, spacing, pupil):
    """w[b] = sum_k coeffs[b, k] Z_k inside the pupil and 0 outside, float32 [B, H, W] with ``shape`` = (H, W)
    (thz_zernike_synthesize); ``coeffs`` float32 [B, K] (or [K], giving [H, W]) with K a full set of orders.
    Gradients flow to ``coeffs`` (thz_zernike_project).  Sync, capture and bits as for ``project``."""
    who = "zernike.synthesize"
    if not torch.is_tensor(coeffs):
        raise TypeError(f"{who}: coeffs must be a tensor")
    _require_device(coeffs, who)
    if coeffs.dtype == torch.float64:
        raise TypeError(f"{who}: the kernels compute in float32; got float64 coefficients -- cast them, an fp64 "
                        "variant does not exist")
    if coeffs.dtype != torch.float32 or coeffs.dim() not in (1, 2):
        raise TypeError(f"{who}: coeffs are float32 [B, K] or [K]; got {coeffs.dtype} {tuple(coeffs.shape)}")
    c = coeffs[None] if coeffs.dim() == 1 else coeffs
    n, m = orders(c.shape[1] - 1)
    if m != n:
        raise ValueError(f"{who}: K = {c.shape[1]} is not a full set of orders (n + 1) (n + 2) / 2")
    out = _Synthesize.apply(c, _geometry(shape, spacing, pupil, n, who))
    return out[0] if coeffs.dim() == 1 else out


def _gram(geo, device, who):
    """(G, its fp64 Cholesky factor) of a geometry, computed once per device; the pupil must hold K pixels"""
    K = num_modes(geo[-1])
    if geo not in _FULL:
        if pupil_pixels(geo[:2], geo[2:4], geo[4:7]) < K:
            raise ValueError(f"{who}: the pupil holds fewer pixels than the {K} modes of max_order = {geo[-1]}")
        _FULL.add(geo)
    device, idx = _dev_index(device)
    key = geo + (idx,)
    if key not in _GRAMS:
        G = _project(None, geo, device, gram=True)[1]
        L = torch.linalg.cholesky_ex(G.double(), check_errors=False).L
        _GRAMS[key] = (G, L)
    return _GRAMS[key]


def gram(shape, spacing, pupil, max_order, device):
    """G[k, k'] = sum over the pupil's pixels of Z_k Z_k', float32 [K, K], exactly symmetric (thz_zernike_project);
    about N_pix times the identity on a fine grid.  Cached per geometry and device.  ValueError (before any launch) when
    the pupil holds fewer pixels than K."""
    return _gram(_geometry(shape, spacing, pupil, max_order, "zernike.gram"), device, "zernike.gram")[0]


def fit(w, spacing, pupil, max_order):
    """The least-squares Zernike coefficients of every map over the pupil, float32 [B, K]: the solution of G a = S
    with S = ``project(w)`` and G = ``gram(...)``, solved on the device in fp64 with G's cached Cholesky factor.
    No host sync; the first call for a pupil computes and factors G, later calls only project and solve.  Gradients
    flow to ``w``.  ValueError (before any launch) when the pupil holds fewer pixels than K."""
    who = "zernike.fit"
    x, single = _maps(w, who)
    geo = _geometry(x.shape, spacing, pupil, max_order, who)
    L = _gram(geo, x.device, who)[1]
    a = torch.cholesky_solve(_Project.apply(x, geo).double().T, L).T.float()
    return a[0] if single else a


def _mask(geo, device):
    device, idx = _dev_index(device)
    key = geo[:-1] + (idx,)
    if key not in _MASKS:
        _MASKS[key] = _synthesize(torch.ones(1, 1, dtype=torch.float32, device=device), geo[:-1] + (0,))[0]
    return _MASKS[key]


def residual(w, spacing, pupil, max_order=2, keep=None):
    """Form removal: ``w`` minus the synthesis of its fit up to ``max_order`` inside the pupil, 0 outside; the default
    takes out piston, tilt, defocus and astigmatism (n <= 2).  ``keep`` lists mode indices k whose fitted term stays
    in the result.  float32, the shape of ``w``; differentiable in ``w``."""
    x, single = _maps(w, "zernike.residual")
    a = fit(x, spacing, pupil, max_order)
    if keep is not None:
        drop = torch.ones(a.shape[1], dtype=torch.float32)
        drop[[int(k) for k in keep]] = 0.0
        a = a * drop.to(a.device)
    geo = _geometry(x.shape, spacing, pupil, max_order, "zernike.residual")
    out = (x - synthesize(a, x.shape[-2:], spacing, pupil)) * _mask(geo, x.device)
    return out[0] if single else out
