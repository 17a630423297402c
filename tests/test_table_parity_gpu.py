"""Table parity: the HIP propagators against fp64 algebra on their own exported fp32 tables.

Every other parity test of the suite compares with the fp64 oracle, which recomputes the transfer
function (ASM) or the spatial kernel (RSC) in fp64, so its bound is the fp32 rounding of the phase
argument (1e-5 ... 1.4e-4 relative L2): the reference's own error, not an error of the FFT, band, crop
or accumulation code.  Here each case exports the table from the device with exactly the fp32
wavelengths, spacings and z the launch receives (ASM_prop.create_kernel, RSC_prop.create_kernel) and
runs pad -> FFT -> multiply -> IFFT -> crop around it in complex128 on the CPU (tests/table_ref.py,
pinned by tests/test_table_ref_cpu.py).  The phase rounding cancels; what is left is the kernels' own
arithmetic.

Two metrics per plane: relative L2, and max|err| / rms(ref) -- elementwise, the one a single wrong
element of a large plane cannot hide in.

Bound, on both: err <= MARGIN x floor32(case), floor32 being the identical algebra in complex64 with
torch's CPU FFT on the same table and input against the complex128 result (measured 1.5e-7 ... 3.7e-7
rel-L2, 0.26e-6 ... 1.4e-6 max/rms).  MARGIN = 4 allows a different but equally valid fp32 FFT (radix-16 / 8 /
5 / 4 / 3 / 2 Stockham stages with table twiddles against pocketfft's factorisation, explicit-fmaf
complex products, split partial sums in the slice kernels): error constants of fp32 FFT variants
differ by small factors, never by an order of magnitude.  The measured ratios are recorded in
profiles/table_parity_ratios.txt (every case prints its line; THZ_TABLE_PARITY_LOG=<file> appends
them to a file).

Inputs are seeded complex white noise.  dx = dy = 0.4 mm at 300 GHz unless a case says otherwise: the
propagating disc is then 0.8 of the frequency square across (half of its area), so the kept-columns
band of the column pass is narrower than the plane, and a band limit at z = min(0.4 Ph dx, 0.12 m)
still leaves far more than the 25 % of non-zero table entries every band-limited case asserts.  (The
reference's band limit takes the padded HEIGHT for both axes, so a thin-H field with a band limit
keeps only a few columns: the thin row-pass carriers run without one.)

Uniform sweeps that take the plane recurrence are not here: they advance H by a product, on purpose,
and tests/test_asm_recurrence_gpu.py owns their 2e-5 bound.  The CZT forms its chirps in-kernel and
exports no table: tests/test_czt_parity_gpu.py holds it to the same margin against tests/czt_ref.py.
"""
import functools
import os

import pytest
import torch

from oracle import thz_oracle as orc
from tests import table_ref as tr
from tests import test_rsc_zx_gpu as zx

pytestmark = pytest.mark.gpu

MARGIN = 4.0
C0 = 2.998e8
DX = 0.4e-3
GHZ = (300, 340)
C64 = torch.complex64


def _dev():
    return torch.device("cuda:0")


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _white(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, dtype=torch.complex128, generator=g).to(C64)


def _launches(fn, names):
    """(result of fn(), launches of each timed kernel family of ``names``)"""
    from quantizationawarethzdoe_amd import _lib
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        out = fn()
        return out, tuple(_lib.timing_read(n)[1] for n in names)
    finally:
        _lib.timing_enable(False)


# The one family with a margin of its own: runtime plans whose largest prime factor R exceeds 256 run
# that factor as a generic DFT stage (csrc/thz_fft.hpp stage_generic), every output a sequential fp32
# sum of R table products -- a documented trade, any length is served.  A sequential sum of R random
# terms of size a has partial sums of size a sqrt(j), so its round-off is u a sqrt(sum j) / sqrt(3) =
# u a R / sqrt(6) against an output of size a sqrt(R): relative u sqrt(R / 6), u = 2^-24, once in the
# forward and once in the inverse transform: sqrt(2) u sqrt(R / 6) = 1.0e-6 at R = 853 (Pw = 1706), by
# itself about four times the floor pocketfft reaches there (2.6e-7), where a register stage adds
# about u.  MARGIN times that share is above the cap the project sets for a family margin, 10, so the
# cap it is.  For R <= 256 the same share is at most twice the floor and MARGIN covers it.
TABLE_DFT_MARGIN = 10.0


def _largest_prime_factor(n):
    p, best = 2, 1
    while p * p <= n:
        while n % p == 0:
            best, n = p, n // p
        p += 1
    return max(best, n) if n > 1 else best


def _margin(P):
    return TABLE_DFT_MARGIN if _largest_prime_factor(P) > 256 else MARGIN


def _judge(family, name, got, ref, floor, MARGIN=MARGIN):
    """One table-parity line, then the assertion: both metrics within MARGIN of the fp32 floor."""
    rel, mx = tr.errors(got, ref)
    line = (f"table-parity {family:<12s} {name:<34s} floor32 {floor[0]:.3e} {floor[1]:.3e}  err {rel:.3e} {mx:.3e}"
            f"  ratio {rel / floor[0]:5.2f} {mx / floor[1]:5.2f}")
    print(line)
    log = os.environ.get("THZ_TABLE_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")
    assert rel <= MARGIN * floor[0] and mx <= MARGIN * floor[1], line
    return rel / floor[0], mx / floor[1]


def _judge_planes(family, name, got, ref, lo):
    """[Z, ...] results plane by plane: ``lo`` is the complex64 run of the algebra that gave ``ref``"""
    for k in range(ref.shape[0]):
        _judge(family, f"{name} z{k}" if ref.shape[0] > 1 else name, got[k], ref[k], tr.floor_of(lo[k], ref[k]))


# ---------------------------------------------------------------------------------------------
# ASM
# ---------------------------------------------------------------------------------------------
PLANE_KERNELS = ("asm_rows_fwd", "asm_cols", "asm_rows_inv")


class _Asm:
    """One ASM geometry: the device field, the propagator and the exported tables on the CPU."""

    def __init__(self, H, W, s=1, bl="exact", B=1, C=1, z=None, unpad=True, pad=True, dx=DX, seed=0):
        from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
        from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
        self.ph, self.pw, self.Ph, self.Pw = orc.asm_padding(H, W, s, pad)
        self.unpad = unpad or not pad
        self.bl = bl
        self.z = min(0.4 * self.Ph * dx, 0.12) if z is None else z
        self.x = _white((B, C, H, W), 1000 * H + W + seed)
        wl = [_f32(C0 / (f * 1e9)) for f in GHZ[:C]]
        self.field = ElectricField(self.x.to(_dev()), wavelengths=wl, spacing=[dx, dx], device=_dev())
        self.prop = ASM_prop(z_distance=self.z, do_padding=pad, do_unpad_after_pad=unpad,
                             padding_scale=list(s) if isinstance(s, tuple) else s, bandlimit_kernel=bl is not None,
                             bandlimit_type=bl or "exact", device=_dev())
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


def _asm_forward_case(family, name, P_axis, P, **kw):
    """One plane through ASM_prop.forward against asm_from_table; the padded length of the axis under
    test is the plan the case is meant for, and the planes' three kernels served it once each."""
    a = _Asm(**kw)
    assert (a.Pw if P_axis == "w" else a.Ph) == P, (a.Ph, a.Pw, P)
    out, n = _launches(lambda: a.prop(a.field).data.cpu(), PLANE_KERNELS)
    assert n == (1, 1, 1), n
    Hc = a.table()
    ref = tr.asm_from_table(a.x, Hc, a.ph, a.pw, a.unpad)
    assert out.shape == ref.shape
    floor = tr.floor32(tr.asm_from_table, a.x, Hc, a.ph, a.pw, a.unpad, ref=ref)
    return _judge(family, name, out, ref, floor, _margin(P))


# (P, N, padding scale): the compile-time plans 300 and 500 (mixed radix), 1024 ... 16384 (powers of
# two), and the runtime plans 180, 201 (odd), 251 (prime), 600 and 1706 = 2 x 853 (table DFT);
# P = N + 2 floor(s N / 2)
LINES = [(300, 100, 2), (500, 100, 4), (1024, 512, 1), (2048, 1024, 1), (4096, 2048, 1), (8192, 4096, 1),
         (16384, 8192, 1), (180, 90, 1), (201, 101, 1), (251, 125, 1.01), (600, 300, 1), (1706, 854, 0.999)]


@pytest.mark.parametrize("P, N, s", LINES, ids=[f"Pw{p[0]}" for p in LINES])
def test_asm_row_pass(P, N, s):
    """The row passes K1 / K3 on a thin field H = 8, W = N; no band limit (see the module docstring)."""
    _asm_forward_case("asm-rows", f"8x{N} s{s} Pw{P} none", "w", P, H=8, W=N, s=s, bl=None, z=0.05)


COL_BL = {300: "approx", 2048: "approx", 600: None, 8192: None}


@pytest.mark.parametrize("P, N, s", LINES, ids=[f"Ph{p[0]}" for p in LINES])
def test_asm_column_pass(P, N, s):
    """The column pass K2 on the transposed carriers H = N, W = 8 (the power-of-two column kernels
    with the pruned first stage live here); band limits as COL_BL, else exact."""
    bl = COL_BL.get(P, "exact")
    _asm_forward_case("asm-cols", f"{N}x8 s{s} Ph{P} {bl or 'none'}", "h", P, H=N, W=8, s=s, bl=bl)


# (id, P, kw)
SQUARES = [
    ("64_s1_exact", 128, dict(H=64, W=64, s=1)),
    ("64_s1_approx", 128, dict(H=64, W=64, s=1, bl="approx")),
    ("64_s1_none", 128, dict(H=64, W=64, s=1, bl=None)),
    ("64_s1.5_padded_out", 160, dict(H=64, W=64, s=1.5, unpad=False)),
    ("64_s2_negative_z", 192, dict(H=64, W=64, s=2, z=-0.03)),
    ("64_s1_B2C2", 128, dict(H=64, W=64, s=1, B=2, C=2)),
    ("64_s1_fullband", 128, dict(H=64, W=64, s=1, dx=0.5e-3)),
    ("101_s1", 201, dict(H=101, W=101, s=1)),
    ("101_nopad", 101, dict(H=101, W=101, pad=False)),
    ("100_s2", 300, dict(H=100, W=100, s=2)),
    ("100_s2_B2C2", 300, dict(H=100, W=100, s=2, B=2, C=2)),
    ("300_nopad", 300, dict(H=300, W=300, pad=False)),
    ("100_s4", 500, dict(H=100, W=100, s=4)),
    ("512_s1", 1024, dict(H=512, W=512, s=1)),
    ("1024_s1", 2048, dict(H=1024, W=1024, s=1)),
]


@pytest.mark.parametrize("name, P, kw", SQUARES, ids=[s[0] for s in SQUARES])
def test_asm_square(name, P, kw):
    kw = dict(kw)
    kw.setdefault("bl", "exact")
    _asm_forward_case("asm-square", name, "h", P, **kw)
    assert orc.asm_padding(kw["H"], kw["W"], kw.get("s", 1), kw.get("pad", True))[3] == P


# five planes, not uniformly spaced (no step of the list repeats: the per-plane form, not the plane
# recurrence), as fractions of the geometry's default z
ZFRAC = (0.45, 0.6, 0.72, 1.0, 1.31)
MULTI = [(300, 100, 2), (500, 100, 4), (1024, 512, 1), (2048, 1024, 1)]


@functools.lru_cache(maxsize=None)
def _multi(P):
    """The square geometry of padded size P, its five planes, their tables, and the fp64 / fp32 planes
    from those tables (computed once per size, only read)."""
    _, N, s = next(m for m in MULTI if m[0] == P)
    a = _Asm(H=N, W=N, s=s, seed=5)
    zs = [_f32(f * a.z) for f in ZFRAC]
    Hcs = [a.table(z) for z in zs]
    ref = tr.asm_planes_from_tables(a.x, Hcs, a.ph, a.pw)
    lo = tr.asm_planes_from_tables(a.x, Hcs, a.ph, a.pw, dtype=C64)
    return a, zs, Hcs, ref, lo


@pytest.mark.parametrize("P, how", [(300, "planes"), (300, "z_chunk2"), (500, "planes"), (1024, "planes"),
                                    (1024, "z_dev"), (2048, "planes")], ids=lambda v: str(v))
def test_asm_planes(P, how):
    """Z = 5 planes of one call, each against its own exported table."""
    from quantizationawarethzdoe_amd import propagation as Pr
    a, zs, Hcs, ref, lo = _multi(P)
    wl, sp = a.args()
    if how == "z_chunk2":
        run = lambda: Pr.asm_propagate(a.field.data, wl, sp, zs, a.ph, a.pw, True, a.code(), z_chunk=2)
        chunks = 3
    elif how == "z_dev":
        zd = torch.tensor(zs, dtype=torch.float32, device=_dev())
        run = lambda: a.prop.propagate_planes(a.field, zs, z_dev=zd)
        chunks = 1
    else:
        run = lambda: a.prop.propagate_planes(a.field, zs)
        chunks = 1
    with torch.no_grad():
        out, n = _launches(lambda: run().cpu(), PLANE_KERNELS)
    assert n == (1, chunks, chunks), n
    _judge_planes("asm-planes", f"P{P} {how}", out, ref, lo)


@pytest.mark.parametrize("P", [m[0] for m in MULTI])
def test_asm_adjoint_sums_the_planes(P):
    from quantizationawarethzdoe_amd import propagation as Pr
    a, zs, Hcs, ref, _ = _multi(P)
    wl, sp = a.args()
    g = _white(tuple(ref.shape), 77 + P)
    out, n = _launches(lambda: Pr.asm_apply(g.to(_dev()), wl, sp, zs, a.ph, a.pw, True, a.code(), adjoint=True).cpu(),
                       PLANE_KERNELS)
    assert n == (1, 1, 1), n
    want = tr.asm_adjoint_from_table(g, Hcs, a.ph, a.pw)
    _judge("asm-adjoint", f"P{P} Z5", out, want, tr.floor32(tr.asm_adjoint_from_table, g, Hcs, a.ph, a.pw, ref=want))


def _modulated(x, t, Hc, ph, pw, dtype=tr.C128):
    return tr.asm_from_table(x.to(dtype) * t.to(dtype), Hc, ph, pw, dtype=dtype)


def test_asm_fused_doe_modulation():
    """thz_asm_forward_modulated at P = 300: the row pass's loader applies t_c(h).  The CPU side
    modulates in fp64 with the fp32 transmission the unfused modulate kernel produces (a field of
    ones through it), then applies the table."""
    from quantizationawarethzdoe_amd import doe
    from quantizationawarethzdoe_amd import propagation as Pr
    a = _Asm(H=100, W=100, s=2, C=2, seed=9)
    wl, sp = a.args()
    h = (torch.rand(100, 100, generator=torch.Generator().manual_seed(4)) * 1e-3).to(_dev())
    with torch.no_grad():
        t = doe.modulate(torch.ones_like(a.field.data), h, wl, 2.66, 0.03)[0].cpu()
        pend = doe.PendingModulation(a.field.data, h, wl, 2.66, 0.03)
        out, n = _launches(lambda: Pr.asm_propagate_modulated(pend, wl, sp, [a.z], a.ph, a.pw, True, a.code()).cpu(),
                           PLANE_KERNELS)
    assert n == (1, 1, 1) and pend.out is None, n   # the modulated field was never formed
    Hc = a.table()
    ref = _modulated(a.x, t, Hc, a.ph, a.pw)
    _judge("asm-fused", "100 s2 P300 DOE->ASM", out[0], ref, tr.floor32(_modulated, a.x, t, Hc, a.ph, a.pw, ref=ref))


def _rows(n):
    return (0, n // 2, n - 1)


def test_asm_slice_forward_and_adjoint():
    """The z-x slice kernels on 512^2 -> P = 1024, rows 0, n // 2, n - 1 of the five planes."""
    from quantizationawarethzdoe_amd import propagation as Pr
    a, zs, Hcs, ref, lo = _multi(1024)
    wl, sp = a.args()
    xd = a.field.data
    N = a.x.shape[-1]
    for row in _rows(N):
        got, n = _launches(lambda: Pr.asm_slice_apply(xd, wl, sp, zs, row, a.ph, a.pw, True, a.code()).cpu(),
                           ("asm_cols_slice", "asm_rows_slice"))
        assert n == (1, 1), n
        _judge_planes("asm-slice", f"P1024 row {row}", got, ref[..., row, :], lo[..., row, :])
        g = _white(tuple(got.shape), 300 + row)
        gin, n = _launches(lambda: Pr.asm_slice_adjoint(g.to(_dev()), wl, sp, zs, row, a.ph, a.pw, True, a.code(),
                                                        N).cpu(), ("asm_cols_slice_adj",))
        assert n == (1,), n
        G = torch.zeros(tuple(ref.shape), dtype=C64)
        G[..., row, :] = g
        want = tr.asm_adjoint_from_table(G, Hcs, a.ph, a.pw)
        _judge("asm-slice-adj", f"P1024 row {row}", gin, want,
               tr.floor32(tr.asm_adjoint_from_table, G, Hcs, a.ph, a.pw, ref=want))


# ---------------------------------------------------------------------------------------------
# RSC / VRS
# ---------------------------------------------------------------------------------------------
# (H, W, C, B, (dx, dy)) as tests/test_rsc_zx_gpu.py; the thin long lines are its PLANS
RSC_FIELDS = [(64, 64, 1, 1, (0.25e-3, 0.25e-3)), (48, 40, 2, 1, (0.25e-3, 0.3e-3)), (33, 47, 1, 1, (0.25e-3, 0.25e-3)),
              (20, 24, 1, 1, (0.5e-3, 0.5e-3))] + zx.PLANS


@functools.lru_cache(maxsize=None)
def _rsc(geo, zs, vectorial=False):
    """The device field of a zx geometry, the exported kernel table of every plane of ``zs`` and the
    fp64 / fp32 planes from them [Z, Bo, C, Ho, Wo] (computed once, only read)."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop
    H, W, C, B, spacing = geo
    x = zx._input(geo)
    field = ElectricField(x.to(_dev()), wavelengths=zx._lam(C), spacing=list(spacing), device=_dev())
    dx, dy = field.spacing_host
    Ks, ref, lo = [], [], []
    for z in zs:
        prop = RSC_prop(z_distance=z, device=_dev())
        prop.check_Zc = False
        K = prop.create_kernel(field).cpu()
        assert tuple(K.shape) == (1, C, H + 2 * (H // 2), W + 2 * (W // 2)) and K.dtype == C64
        Ks.append(K)
        if vectorial:
            ref.append(tr.vrs_from_table(x, K, dx, dy, _f32(z)))
            lo.append(tr.vrs_from_table(x, K, dx, dy, _f32(z), dtype=C64))
        else:
            ref.append(tr.rsc_from_table(x, K, dx, dy))
            lo.append(tr.rsc_from_table(x, K, dx, dy, dtype=C64))
    return field, Ks, torch.stack(ref), torch.stack(lo)


@pytest.mark.parametrize("geo", RSC_FIELDS, ids=zx._id)
def test_rsc_forward_and_adjoint(geo):
    from quantizationawarethzdoe_amd import propagation as Pr
    H, W, C, B, _ = geo
    z = 0.05
    field, (K,), ref, lo = _rsc(geo, (z,))
    wl, sp = field.wavelengths_host, field.spacing_host
    out, n = _launches(lambda: Pr.rsc_apply(field.data, wl, sp, z).cpu(), ("rsc_kernel_fft",) + PLANE_KERNELS)
    assert n == (1, 1, 1, 1), n
    _judge("rsc", f"{H}x{W} C{C}", out, ref[0], tr.floor_of(lo[0], ref[0]))
    g = _white(tuple(out.shape), 500 + H)
    gin = Pr.rsc_apply(g.to(_dev()), wl, sp, z, adjoint=True, field_hw=(H, W)).cpu()
    want = tr.rsc_adjoint_from_table(g, K, sp[0], sp[1], H, W)
    _judge("rsc-adjoint", f"{H}x{W} C{C}", gin, want,
           tr.floor32(tr.rsc_adjoint_from_table, g, K, sp[0], sp[1], H, W, ref=want))


def test_vrs_three_planes():
    from quantizationawarethzdoe_amd import propagation as Pr
    geo, z = (40, 48, 2, 2, (0.25e-3, 0.3e-3)), 0.05
    field, _, ref, lo = _rsc(geo, (z,), True)
    out = Pr.rsc_apply(field.data, field.wavelengths_host, field.spacing_host, z, vectorial=True).cpu()
    assert out.shape == ref[0].shape == (3, 2, 40, 48)
    for b, nm in enumerate(("Ex", "Ey", "Ez")):
        _judge("vrs", f"40x48 C2 {nm}", out[b], ref[0][b], tr.floor_of(lo[0][b], ref[0][b]))


SLICES = [(g, False) for g in zx.GEOMETRIES + zx.PLANS + zx.BATCHES] + [(zx.VRS, True), (zx.VRS_4096, True)]


@pytest.mark.parametrize("geo, vec", SLICES, ids=[zx._id(g) + ("_vrs" if v else "") for g, v in SLICES])
def test_rsc_slice_forward_and_adjoint(geo, vec):
    """rsc_slice_apply / rsc_slice_adjoint on the zx file's geometries and its non-uniform ZS, rows 0,
    n // 2, n - 1, against the fp64 planes from each plane's own exported table."""
    from quantizationawarethzdoe_amd import propagation as Pr
    H, W, C, B, _ = geo
    field, Ks, ref, lo = _rsc(geo, zx.ZS, vec)
    wl, sp = field.wavelengths_host, field.spacing_host
    name = f"{H}x{W} C{C} B{B}" + (" vrs" if vec else "")
    for row in _rows(2 * (H // 2)):
        got, n = _launches(lambda: Pr.rsc_slice_apply(field.data, wl, sp, list(zx.ZS), row, vec).cpu(),
                           ("rsc_slice_acc",))
        assert n == (1,), n
        _judge_planes("rsc-slice", f"{name} row {row}", got, ref[..., row, :], lo[..., row, :])
        g = _white(tuple(got.shape), 700 + row)
        gin, n = _launches(lambda: Pr.rsc_slice_adjoint(g.to(_dev()), wl, sp, list(zx.ZS), row, (B, C, H, W), vec).cpu(),
                           ("rsc_slice_acc_adj",))
        assert n == (1,), n

        def adjoint(g, Ks, dtype=tr.C128):
            """the sum over the planes of each plane's adjoint of g[k] at row ``row`` of a zero plane"""
            total = 0
            for k, K in enumerate(Ks):
                G = torch.zeros(tuple(ref.shape[1:]), dtype=dtype)
                G[..., row, :] = g[k].to(dtype)
                if vec:
                    total = total + tr.vrs_adjoint_from_table(G, K, sp[0], sp[1], _f32(zx.ZS[k]), H, W, dtype=dtype)
                else:
                    total = total + tr.rsc_adjoint_from_table(G, K, sp[0], sp[1], H, W, dtype=dtype)
            return total

        want = adjoint(g, Ks)
        _judge("rsc-slice-adj", f"{name} row {row}", gin, want, tr.floor32(adjoint, g, Ks, ref=want))
