"""Polarization analyser -- drop-in for the reference's Addons/Polarization.py.

``PolarizationAnalyser`` reads the polarization state out of a vectorial field ([3, C, H, W]: Ex, Ey,
Ez on the batch axis), as test_new_features.ipynb cells 0-6 do after VRS_prop.  The Stokes vector
(:45-65) and the ellipse parameters (:67-92) are each one fused pass over the Ex and Ey planes on the
device (optics.stokes / optics.polarization_ellipse -> thz_stokes_forward,
thz_polarization_ellipse); the Ez plane is never read.  The ``visualize_*`` methods are host
matplotlib on those outputs, with the reference's titles, colour limits and extents.

One deliberate deviation: B's radicand is clamped at 0, where the reference returns NaN on exactly
linear polarization (optics.polarization_ellipse).  The plotting keeps two quirks of the reference,
cited where they occur.
"""
from __future__ import annotations

import numpy as np
import torch

from quantizationawarethzdoe_amd import optics as _optics

eps = _optics.POLARIZATION_EPS


def _host(t, numpy):
    return t.detach().cpu().numpy() if numpy else t


class PolarizationAnalyser:
    def __init__(self, field, device=None):
        self.device = device or torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if field.field_type != 'vectorial':
            raise ValueError("The polarization analyser is only valid for vectorial field")
        self.field = field

    # -- the two analyses (device kernels) ----------------------------------------------------------
    def polarization_state(self, field, numpy=False):
        """(I, Q, U, V) of ``field`` ([>= 2, ...] complex, Ex and Ey first), each squeezed as the
        reference squeezes its component planes (:49-50): [H, W] for [3, 1, H, W]."""
        s = _optics.stokes(field, comp_dim=0)
        return tuple(_host(s[k].squeeze(), numpy) for k in range(4))

    def polarization_ellipse(self, field, numpy=True):
        """(A, B, theta, h): semi-axes, orientation and handedness of the polarization ellipse."""
        e = _optics.polarization_ellipse(field, comp_dim=0)
        return tuple(_host(e[k].squeeze(), numpy) for k in range(4))

    # -- plotting (host) ----------------------------------------------------------------------------
    def _frame(self, wavelength):
        """Half-sizes of the field in its display unit, that unit's name, and the wavelength as
        (value, unit) for the titles (:109-117)."""
        from quantizationawarethzdoe_amd.utils.Visualization_Helper import float_to_unit_identifier
        sp = self.field.spacing_host
        half_x, half_y = sp[0] / 2.0 * self.field.height, sp[1] / 2.0 * self.field.width
        scale, axis_unit = float_to_unit_identifier(max(half_x, half_y))
        wl_scale, wl_unit = float_to_unit_identifier(float(wavelength))
        return half_x / scale, half_y / scale, axis_unit, str(round(float(wavelength) / wl_scale, 2)) + str(wl_unit)

    def _four_panels(self, planes, names, limits, wavelength, figsize, cmap):
        import matplotlib.pyplot as plt
        from quantizationawarethzdoe_amd.utils.Visualization_Helper import add_colorbar
        hx, hy, axis_unit, wl_text = self._frame(wavelength)
        if figsize is not None:
            plt.figure(figsize=figsize)
        images = []
        for k, (plane, name, (lo, hi)) in enumerate(zip(planes, names, limits)):
            plt.subplot(2, 2, k + 1)
            images.append(plt.imshow(plane, cmap=cmap, extent=[-hy, hy, -hx, hx], vmin=lo, vmax=hi))
            plt.title(name + " | wavelength = " + wl_text)
            plt.xlabel("Position (" + axis_unit + ")")
            plt.ylabel("Position (" + axis_unit + ")")
        for im in images:
            add_colorbar(im)
        plt.axis("on")
        plt.tight_layout()

    def visualize_param_stokes(self, wavelength, normalize=False, figsize=(8, 8), cmap=None):
        """S1 ... S4 in a 2 x 2 figure: S1 on [0, max S1], the others on +-max S1 (:94-149)."""
        from matplotlib import cm
        planes = self.polarization_state(self.field._get_data_for_wavelength(wavelength), numpy=True)
        if normalize:
            planes = tuple(p / (np.abs(p).max() + eps) for p in planes)
        top = planes[0].max()
        self._four_panels(planes, ("S1", "S2", "S3", "S4"), [(0, top)] + [(-top, top)] * 3, wavelength, figsize,
                          cm.seismic if cmap is None else cmap)

    def visualize_param_ellipse(self, wavelength, figsize=(8, 8), cmap=None):
        """A and B on [0, max(A, B)], theta on +-pi, h autoscaled (:152-202)."""
        from matplotlib import cm
        planes = self.polarization_ellipse(self.field._get_data_for_wavelength(wavelength), numpy=True)
        top = max(planes[0].max(), planes[1].max())
        self._four_panels(planes, ("A", "B", "theta", "h"), [(0, top), (0, top), (-np.pi, np.pi), (None, None)],
                          wavelength, figsize, cm.seismic if cmap is None else cmap)

    def visualize_ellipse_field(self, wavelength, percentage_intensity=0.005, num_ellipses=(21, 21), figsize=(8, 8),
                                cm_intensity=None, amplification=0.75, color_line='w', line_width=0.75):
        """The local polarization ellipses on a num_ellipses grid over an intensity map (:204-305)."""
        import matplotlib.pyplot as plt
        from matplotlib import cm
        data = self.field._get_data_for_wavelength(wavelength)
        I, Q, _, _ = self.polarization_state(data, numpy=True)
        Ex, Ey = (data[k].squeeze().detach().cpu().numpy() for k in (0, 1))
        H, W = self.field.height, self.field.width
        hx, hy, axis_unit, wl_text = self._frame(wavelength)
        if figsize is not None:
            plt.figure(figsize=figsize)
        # the reference's background sums |Ey|^2 twice (Polarization.py:266): |Ex|^2 + 2 |Ey|^2, with
        # |Ey|^2 = (I - Q) / 2 from the Stokes planes; the drawing threshold uses I itself (:220)
        back = I + 0.5 * (I - Q)
        plt.imshow(back, cmap=cm.gist_heat if cm_intensity is None else cm_intensity, extent=[-hy, hy, -hx, hx],
                   vmax=back.max(), vmin=back.min())
        plt.title("Intensity | wavelength = " + wl_text)
        plt.xlabel("Position (" + axis_unit + ")")
        plt.ylabel("Position (" + axis_unit + ")")
        ax = plt.gca()

        x, y = np.linspace(-hx, hx, H), np.linspace(-hy, hy, W)
        # both cell sizes come from the height extent Dx in the reference (Polarization.py:239)
        cell = min(2 * hx / num_ellipses[0], 2 * hx / num_ellipses[1])
        # cell-centre indices: the first set is spaced over the height and clipped to the width, the
        # second the other way round, and the first indexes the last axis (Polarization.py:243-261)
        sx, sy = H / num_ellipses[0], W / num_ellipses[1]
        ix = np.round(sx / 2 + sx * np.arange(num_ellipses[0])).astype(int)
        iy = np.round(sy / 2 + sy * np.arange(num_ellipses[1])).astype(int)
        ix, iy = np.clip(ix, 0, Ex.shape[-1] - 1), np.clip(iy, 0, Ey.shape[-2] - 1)
        turn = np.exp(1j * np.linspace(0, 2 * np.pi, 64))
        for i in ix:
            for j in iy:
                px, py = np.real(Ex[j, i] * turn), np.real(Ey[j, i] * turn)
                r = np.sqrt(px ** 2 + py ** 2).max()
                if r > 0 and r ** 2 > percentage_intensity * I.max():
                    px = px / r * cell * amplification / 2 + x[i]
                    py = py / r * cell * amplification / 2 + y[j]
                    ax.plot(px, py, color_line, lw=line_width)
                    ax.arrow(px[0], py[0], px[0] - px[1], py[0] - py[1], width=0, head_width=1, fc=color_line,
                             ec=color_line, length_includes_head=False)
        plt.show()

    def analyze(self, wavelength, type='ellipse_field', percentage_intensity=0.005, figsize=(8, 8),
                num_ellipses=(21, 21), color_line='w', line_width=0.75):
        if type == 'stokes':
            self.visualize_param_stokes(wavelength, figsize=figsize)
        elif type == 'param_ellipse':
            self.visualize_param_ellipse(wavelength, figsize=figsize)
        elif type == 'ellipse_field':
            self.visualize_ellipse_field(wavelength, figsize=figsize, percentage_intensity=percentage_intensity,
                                         num_ellipses=num_ellipses, color_line=color_line, line_width=line_width)
        else:
            raise ValueError("No existing analysis type in vector field")
