"""What ASM_prop, CZT_prop and RSC_prop / VRS_prop.propagate_zx share: the z-sweep as host floats,
the checks of ``axis`` / ``grad`` / ``row``, the sweep on the slice kernels and the fallback that
slices full planes.  Which inputs the slice kernels serve, and each propagator's geometry, stay in the
propagators."""
from __future__ import annotations

import numpy as np
import torch

from quantizationawarethzdoe_amd import propagation as _prop


def _f(v):
    return float(v.detach().cpu()) if torch.is_tensor(v) else float(v)


def _z_host(z):
    """The plane distances of a z-sweep as a flat list of host floats: a tensor or numpy array of any
    shape, a (nested) sequence of floats or 0-d tensors on any device, any other iterable, or one value."""
    if torch.is_tensor(z):
        return [float(v) for v in z.detach().reshape(-1).cpu().tolist()]
    if not isinstance(z, np.ndarray):
        try:
            return [_f(v) for v in z]  # the usual sweep: a flat sequence of floats or 0-d tensors
        except TypeError:
            if not isinstance(z, (list, tuple)):
                return [float(z)]
    return [float(v) for v in np.asarray(z).reshape(-1)]  # an array, or a nested sequence


def check_axis_grad(axis, grad):
    if axis not in ("x", "y"):
        raise ValueError(f"propagate_zx: axis must be 'x' or 'y', got {axis!r}")
    if grad not in ("planes", "slice"):
        raise ValueError(f"propagate_zx: grad must be 'planes' or 'slice', got {grad!r}")


def output_row(row, n, axis):
    """``row`` as an index of the ``n`` output rows (axis "x") or columns ("y"); None is the centre n // 2."""
    row = n // 2 if row is None else int(row)
    if not 0 <= row < n:
        raise ValueError(f"propagate_zx: row {row} outside the valid range [0, {n}) of the output "
                         f"{'rows' if axis == 'x' else 'columns'}")
    return row


def native_sweep(family, x, wavelengths, spacing, zs, row, geo):
    """Row ``row`` of every plane of ``zs`` on the slice kernels of ``family`` ("asm" / "czt" / "rsc");
    ``x`` is the complex64 device field as the kernels take it (transposed for ``axis="y"``) and ``geo``
    the family's geometry tuple (propagation._SLICE_FAMILIES).  An input that requires grad goes
    through the autograd Function per chunk of THZ_MAX_Z planes (backward: the slice adjoint); any
    other is detached and every chunk written into one [Z, ...] result."""
    return _prop._slice_sweep(_prop._SLICE_FAMILIES[family], x, wavelengths, spacing, zs, row, geo,
                              torch.is_grad_enabled() and x.requires_grad)


def sliced_planes(planes_of, zs, plane_bytes, row, axis):
    """The fallback: ``planes_of(z chunk)`` -> the full planes [z, ..., rows, columns] of the chunk,
    differentiably, in chunks of at most THZ_MAX_Z planes whose temporary (``plane_bytes`` each) stays
    under 10 GiB -- the library's own cap on its per-chunk intermediate -- each chunk sliced at ``row``."""
    step = int(max(1, min(_prop._lib.THZ_MAX_Z, (10240 * 1024 * 1024) // max(1, plane_bytes))))
    outs = []
    for k in range(0, len(zs), step):
        planes = planes_of(zs[k:k + step])
        outs.append(planes[..., row, :] if axis == "x" else planes[..., :, row])
    return outs[0] if len(outs) == 1 else torch.cat(outs, 0)
