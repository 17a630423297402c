#!/usr/bin/env python
"""Time the fused polarization kernels against the reference's torch op sequence on the same
device and tensors: a [3, 32, 2048, 2048] complex64 field (seeded), one MI355X.

Three pairs, alternated --reps times after --warmup rounds, each call timed with HIP events:
  stokes   : optics.stokes(x)               (thz_stokes_forward)       vs  Addons/Polarization.py:49-56
  ellipse  : optics.polarization_ellipse(x) (thz_polarization_ellipse) vs  :72-84 on top of :49-56
  fwd+bwd  : sum(w * stokes(x)).backward()  (thz_stokes_backward)      vs  torch differentiating :49-56
The torch sequence is the yardstick (there was no such function before).  Then, in a pass of its own,
the kernels' own HIP-event times (thz_timing_*), with the byte model: Stokes and ellipse read 16 B and
write 16 B per pixel (32 B), the backward reads 32 B and writes 16 B (48 B); achieved GB/s and the
fraction of the 8.0 TB/s HBM3E peak.  Outputs of both sides are compared at the timed size.  Plain
text to --out.

    python scripts/polarization_timing.py --out profiles/polarization_timing.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12
EPS = 1e-6


def ref_stokes(field):
    """The yardstick: as many elementwise torch ops, on plane-sized temporaries, as the reference's
    polarization_state spends (Addons/Polarization.py:49-56) -- |Ex|^2 and |Ey|^2 formed twice each
    (for I and for Q) and the product Ex conj(Ey) twice (for U and for V); 18 ops."""
    ex, ey = field[0].squeeze(), field[1].squeeze()
    s0 = ex.abs().pow(2).add(ey.abs().pow(2))
    s1 = ex.abs().pow(2).sub(ey.abs().pow(2))
    s2 = ex.mul(ey.conj()).real.mul(2)
    s3 = ex.mul(ey.conj()).imag.mul(2)
    return s0, s1, s2, s3


def ref_ellipse(field):
    """The reference's polarization_ellipse op for op (:72-84) on top of ref_stokes: a complex L,
    |L| taken twice, complex-free square roots, angle and sign; no clamp, so B can be NaN."""
    _, s1, s2, s3 = ref_stokes(field)
    pol = s1.pow(2).add(s2.pow(2)).add(s3.pow(2)).sqrt()
    lin = s1.add(s2.mul(1j)).add(EPS)
    major = pol.add(lin.abs()).add(EPS).mul(0.5).sqrt().real
    minor = pol.sub(lin.abs()).add(EPS).mul(0.5).sqrt().real
    return major, minor, lin.angle().mul(0.5), s3.add(EPS).sign()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/polarization_timing.txt")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--n", type=int, default=2048)
    args = ap.parse_args()

    from quantizationawarethzdoe_amd import _lib, optics

    if not torch.cuda.is_available():
        sys.exit("polarization_timing: needs a ROCm GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    C, N = args.channels, args.n
    torch.manual_seed(4000)
    x = torch.randn(3, C, N, N, dtype=torch.complex64, device=dev)
    w = torch.randn(4, C, N, N, device=dev)
    pixels = C * N * N

    def fused_fb():
        xr = x.detach().requires_grad_(True)
        (w * optics.stokes(xr)).sum().backward()
        return xr.grad

    def torch_fb():
        xr = x.detach().requires_grad_(True)
        (w * torch.stack(ref_stokes(xr))).sum().backward()
        return xr.grad

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn(x)
        return run

    pairs = [
        ("stokes", nograd(optics.stokes), nograd(ref_stokes)),
        ("ellipse", nograd(optics.polarization_ellipse), nograd(ref_ellipse)),
        ("stokes fwd+bwd", fused_fb, torch_fb),
    ]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        del out
        return ms

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = [
        f"Polarization timing: [3, {C}, {N}, {N}] complex64 field ({pixels / 1e6:.1f} M pixels per component plane)",
        f"device {torch.cuda.get_device_name(0)}, library {_lib.version()}, {args.reps} alternated reps after "
        f"{args.warmup} warm-up rounds, HIP events around each call",
    ]
    for name, fused, ref in pairs:
        for _ in range(args.warmup):
            fused()
            ref()
        torch.cuda.synchronize()
        tf, tr = [], []
        for _ in range(args.reps):
            tf.append(timed(fused))
            tr.append(timed(ref))
        lines += [
            f"{name}:",
            f"  fused kernel(s)       : median {med(tf):9.3f} ms  (min {min(tf):.3f}, max {max(tf):.3f})",
            f"  torch op sequence     : median {med(tr):9.3f} ms  (min {min(tr):.3f}, max {max(tr):.3f})",
            f"  ratio torch / fused   : {med(tr) / med(tf):.2f}   slowest fused rep faster than the fastest torch rep: "
            f"{max(tf) < min(tr)}",
        ]
        torch.cuda.empty_cache()

    # same results at the timed size (a reordered fp32 sum differs in the last bits)
    with torch.no_grad():
        s, r = optics.stokes(x), torch.stack(ref_stokes(x))
        lines.append(f"stokes fused vs torch: max |diff| / I = {float(((s - r).abs() / r[0]).max()):.3e}")
        del s, r
        e, r = optics.polarization_ellipse(x), ref_ellipse(x)
        lines.append(f"ellipse fused vs torch: max |dA| = {float((e[0] - r[0]).abs().max()):.3e}, "
                     f"torch NaN pixels in B = {int(torch.isnan(r[1]).sum())}, fused NaN pixels = "
                     f"{int(torch.isnan(e).sum())}")
        del e, r
    ga, gb = fused_fb(), torch_fb()
    lines.append(f"backward fused vs torch: relative L2 = {float((ga - gb).norm() / gb.norm()):.3e}")
    del ga, gb
    torch.cuda.empty_cache()

    kernels = [("stokes_fwd", 32), ("polarization_ellipse", 32), ("stokes_bwd", 48)]
    _lib.timing_enable(True)
    _lib.timing_reset()
    for _ in range(args.reps):
        with torch.no_grad():
            optics.stokes(x)
            optics.polarization_ellipse(x)
        fused_fb()
    per = {k: _lib.timing_read(k) for k, _ in kernels}
    _lib.timing_enable(False)
    lines.append("kernels' own HIP-event time per launch (separate pass) and the byte model:")
    for k, bpp in kernels:
        ms, n = per[k]
        t = ms / n * 1e-3
        bw = bpp * pixels / t
        lines.append(f"  {k:22s} {ms / n:8.3f} ms  ({n} launches)  {bpp} B/pixel = {bpp * pixels / 2 ** 30:.2f} GiB -> "
                     f"{bw / 1e9:7.1f} GB/s = {100 * bw / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
