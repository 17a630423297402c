"""DiscreteDOE -- drop-in for the reference's Components/discrete_doe.py: the holder of the level
table that the nearest-neighbour quantizers of Components/quantization.py read.

Interface kept from the reference (:6-35): the class attributes ``_lut``, ``_lut_midvals`` and
``prev_idx``, and the two properties.  On an instance, assigning ``lut`` stores a detached copy of the
table as a tensor together with the midpoints of neighbouring levels (``lut_mid``); assigning None
clears only the table; assigning ``lut_midvals`` stores the thresholds alone.  The quantizers read
``DiscreteDOE.lut`` and ``DiscreteDOE.lut_midvals`` on the *class* (Components/quantization.py:64-65),
where a property is the property object itself, so a user of the reference assigns both on the class
(``DiscreteDOE.lut = table; DiscreteDOE.lut_midvals = torch.tensor(lut_mid(table))``); that works
here the same way.  Tables kept as lists or CPU tensors cost the quantizers nothing; a device tensor
is read back to the host on every call (optics.lut_quantize).
"""
import torch

from quantizationawarethzdoe_amd.utils.Helper_Functions import lut_mid


def _as_table(values):
    return values.clone().detach() if torch.is_tensor(values) else torch.tensor(values)


class DiscreteDOE:
    """Level table (``lut``) and thresholds between levels (``lut_midvals``) of a discrete DOE."""
    _lut = None
    _lut_midvals = None
    prev_idx = 0.

    def _get_lut(self):
        return self._lut

    def _set_lut(self, table):
        if table is not None:
            self.lut_midvals = lut_mid(table)
            table = _as_table(table)
        self._lut = table

    def _get_midvals(self):
        return self._lut_midvals

    def _set_midvals(self, thresholds):
        self._lut_midvals = torch.tensor(thresholds)

    lut = property(_get_lut, _set_lut)
    lut_midvals = property(_get_midvals, _set_midvals)
