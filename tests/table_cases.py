"""The ASM geometries of the table-parity tests (tests/test_table_parity_gpu.py, tests/test_asm_rows_pair_b64_gpu.py)
and the family's judge: tests/parity.judge on the table-parity log.

Plain helper module: no test, no fixture.
"""
import functools

from oracle import thz_oracle as orc
from tests import parity
from tests.gpu_util import C0, C64, dev, f32, white_cpu

DX = 0.4e-3
GHZ = (300, 340)
PLANE_KERNELS = ("asm_rows_fwd", "asm_cols", "asm_rows_inv")

# One table-parity line, then the assertion: both metrics within the margin of the fp32 floor.
judge = functools.partial(parity.judge, "THZ_TABLE_PARITY_LOG", "table-parity")


class AsmCase:
    """One ASM geometry: the device field, the propagator and the exported tables on the CPU."""

    def __init__(self, H, W, s=1, bl="exact", B=1, C=1, z=None, unpad=True, pad=True, dx=DX, seed=0):
        from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
        from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
        self.ph, self.pw, self.Ph, self.Pw = orc.asm_padding(H, W, s, pad)
        self.unpad = unpad or not pad
        self.bl = bl
        self.z = min(0.4 * self.Ph * dx, 0.12) if z is None else z
        self.x = white_cpu((B, C, H, W), 1000 * H + W + seed)
        wl = [f32(C0 / (f * 1e9)) for f in GHZ[:C]]
        self.field = ElectricField(self.x.to(dev()), wavelengths=wl, spacing=[dx, dx], device=dev())
        self.prop = ASM_prop(z_distance=self.z, do_padding=pad, do_unpad_after_pad=unpad,
                             padding_scale=list(s) if isinstance(s, tuple) else s, bandlimit_kernel=bl is not None,
                             bandlimit_type=bl or "exact", device=dev())
        self.prop.check_Zc = False
        assert self.prop.compute_padding(H, W, True) == (self.ph, self.pw)

    def table(self, z=None):
        """create_kernel's table for plane z on the CPU, with the band-limit condition: a band-limited
        case keeps at least 25 % of its table."""
        keep = self.prop.z
        if z is not None:
            self.prop.z = z
        try:
            Hc = self.prop.create_kernel(self.field).cpu()
        finally:
            self.prop.z = keep
        assert tuple(Hc.shape[-2:]) == (self.Ph, self.Pw) and Hc.dtype == C64
        frac = float((Hc != 0).float().mean())
        if self.bl is not None:
            assert frac >= 0.25, f"band-limited table keeps {frac:.3f} of its entries"
        return Hc

    def code(self):
        return self.prop._bandlimit_code()

    def args(self):
        """(wavelengths, spacing) as every launch of this field receives them"""
        return self.field.wavelengths_host, self.field.spacing_host
