"""The project's parity rule, once: the metrics, the fp32 floor, the margin, and the two harness shapes.

A kernel family is compared with an fp64 restatement of its algebra, and its allowed error is MARGIN times the error
the same algebra makes in fp32 on the CPU ("floor32", "e32").  Floor-based families (``judge``) hold both metrics of
``errors`` to MARGIN x floor32 and append one line per case to a log; bound-based families (``Ratios``) hold a value
to 4 max(e32, 2^-24 |value|) in the maximum norm and a gradient to 4 max(e32, 1e-6) in relative L2, and rewrite a
summary of the largest err / bound per quantity at the end of their module.

Plain helper module: no test, no fixture, torch only.  tests/test_parity_toolkit_cpu.py pins it.
"""
import os

import torch

C128 = torch.complex128
U32 = 2.0 ** -24   # one fp32 rounding, relative

# floor32 is the identical algebra in complex64 with torch's CPU FFT against its complex128 run.  MARGIN = 4 allows a
# different but equally valid fp32 pipeline (radix-16 / 8 / 5 / 4 / 3 / 2 Stockham stages with table twiddles against
# pocketfft's factorisation, explicit-fmaf complex products, split partial sums in the slice kernels): error constants
# of fp32 FFT variants differ by small factors, never by an order of magnitude.
MARGIN = 4.0


def errors(got, ref):
    """(relative L2, max|err| / rms(ref)) of ``got`` against ``ref``, both taken in complex128.  The second is
    elementwise: one wrong element of n carries 1 / sqrt(n) of a relative L2 and all of this one."""
    got, ref = got.to(C128), ref.to(C128)
    err = (got - ref).abs()
    rms = float(ref.abs().pow(2).mean().sqrt())
    return float(err.pow(2).sum().sqrt() / ref.abs().pow(2).sum().sqrt()), float(err.max()) / rms


def floor_of(lo, ref, *, rel_cap, max_cap, at_least_u32=False):
    """errors() of the low-precision run ``lo`` against ``ref``, checked to be what a bound may rest on: rel-L2 within
    ``rel_cap`` and max/rms within ``max_cap``.  By default no run is better than one fp32 rounding and max/rms is no
    smaller than rel-L2; with ``at_least_u32`` both only have to be positive and are clamped up to U32."""
    rel, mx = errors(lo, ref)
    if at_least_u32:
        ok = 0 < rel < rel_cap and 0 < mx < max_cap
    else:
        ok = U32 <= rel <= rel_cap and rel <= mx <= max_cap
    assert ok, f"floor32 {rel:.3e} {mx:.3e} is not an fp32 pipeline's error (caps {rel_cap:.1e} {max_cap:.1e})"
    return (max(rel, U32), max(mx, U32)) if at_least_u32 else (rel, mx)


def emit(log_env, line):
    """Print ``line`` and append it to the file the environment variable ``log_env`` names, if it names one."""
    print(line)
    log = os.environ.get(log_env)
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


def judge(log_env, prefix, family, name, got, ref, floor, margin=MARGIN, widths=(12, 34)):
    """One parity line (``widths``: the family and name columns, a family's own), then the assertion: both metrics
    within ``margin`` of the fp32 floor.  -> (rel-L2 ratio, max/rms ratio)"""
    rel, mx = errors(got, ref)
    assert floor[0] > 0 and floor[1] > 0, floor
    line = (f"{prefix} {family:<{widths[0]}s} {name:<{widths[1]}s} floor32 {floor[0]:.3e} {floor[1]:.3e}"
            f"  err {rel:.3e} {mx:.3e}  ratio {rel / floor[0]:5.2f} {mx / floor[1]:5.2f}")
    emit(log_env, line)
    assert rel <= margin * floor[0] and mx <= margin * floor[1], line
    return rel / floor[0], mx / floor[1]


class Ratios:
    """The largest err / bound per quantity of a bound-based family; ``write()`` rewrites the summary file that
    ``log_env`` names.  ``widths``: the quantity and case columns of the printed line and the key column of the file."""

    def __init__(self, log_env, header, widths=(26, 60, 28)):
        self.log_env, self.header, self.widths = log_env, header, widths
        self.worst, self.values = {}, {}

    def note(self, what, case, ratio):
        print(f"{what:{self.widths[0]}s} {case:{self.widths[1]}s} err / bound = {ratio:.4f}")
        if what not in self.worst or ratio > self.worst[what][0]:
            self.worst[what] = (ratio, case)

    def value(self, what, case, got, fn):
        """fn(dtype) -> the restatement on the CPU.  |got - fp64| <= 4 max(e32, 2^-24 |value|), err, e32 and |value|
        the maxima over the quantity's elements."""
        r64, r32 = fn(torch.float64), fn(torch.float32)
        got = got.detach().cpu().double()
        assert got.shape == r64.shape, (got.shape, r64.shape)
        assert bool(torch.isfinite(got).all())
        err = float((got - r64).abs().max())
        e32 = float((r32.double() - r64).abs().max())
        bound = MARGIN * max(e32, U32 * float(r64.abs().max()))
        self.note(what, case, err / bound if bound else float(err > 0))
        assert err <= bound, (what, case, err, e32, bound)

    def grad(self, what, case, got, fn):
        """fn(dtype) -> the gradient of the restatement by autograd on the CPU.  Relative L2 <= 4 max(e32, 1e-6); a
        zero fp64 gradient demands an exactly zero one."""
        g64, g32 = fn(torch.float64), fn(torch.float32)
        got = got.detach().cpu().double()
        assert got.shape == g64.shape and bool(torch.isfinite(got).all())
        nrm = float(g64.norm())
        if nrm == 0:
            assert float(got.abs().max()) == 0
            return
        err, e32 = float((got - g64).norm()) / nrm, float((g32.double() - g64).norm()) / nrm
        bound = MARGIN * max(e32, 1e-6)
        self.note(what + " grad", case, err / bound)
        assert err <= bound, (what, case, err, e32, bound)

    def write(self):
        path = os.environ.get(self.log_env)
        if path:
            with open(path, "w") as fh:
                fh.write(self.header)
                for k in sorted(self.worst):
                    fh.write(f"{k:{self.widths[2]}s} {self.worst[k][0]:.4f}   ({self.worst[k][1]})\n")
                for k in sorted(self.values):
                    fh.write(f"{k:{self.widths[2]}s} {self.values[k]}\n")
