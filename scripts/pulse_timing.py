#!/usr/bin/env python
"""Time the pulse kernels (pulse.synthesize, pulse.pulse_maps and their backwards) on the current GPU and write
profiles/pulse_timing.txt.

Shapes [1, 32, 2048, 2048] and [3, 32, 1024, 1024] at T = 64 and 128, against two yardsticks on the same exported table:
``real``, torch.matmul on the real-stacked form ([2T, 2C] x [2C, pixels], the stacking and the return to complex
included) -- the fair one; and ``einsum``, torch.einsum with the complex64 table, followed by the torch reductions for
the maps.  HIP events around each call, every contender warmed up and alternated round by round; medians and the spread
over the rounds, peak memory above the inputs per contender.  Kernel time is the library's own event pair around each
launch (thz_timing_read), taken in a pass of its own; ``--trace B,C,H,W,T`` runs one shape alone for
``rocprofv3 --kernel-trace --stats -- python scripts/pulse_timing.py --trace ...``.  No counter is read.

The model: 8 T C flop per pixel, 8 C bytes read, 8 T (synthesize) or 20 (maps) bytes written.

Asserted once: a pulse_maps call allocates the five maps and nothing else, and forward + backward the five maps, their
gradient as autograd hands it over ([B, 5, H, W]) and the field-sized gradient -- no [B, T, H, W] tensor.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import _lib, pulse  # noqa: E402

C0 = pulse.C0


def axes(C, T):
    f = torch.linspace(0.2e12, 1.0e12, C, dtype=torch.float64)
    return (C0 / f).tolist(), ((torch.arange(T, dtype=torch.float64) - T / 2) * (30e-12 / T)).tolist()


def rounds(fns, n):
    """the contenders alternated round by round -> per contender (milliseconds per round, peak bytes above the start)"""
    peaks = []
    for f in fns:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
    ms = [[] for _ in fns]
    for _ in range(n):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return ms, peaks


def fmt(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} .. {max(v):.3f})"


def contenders(U, lam, times):
    """{name: (hand, real, einsum)} closures on one field"""
    dev = U.device
    table = pulse.time_table(lam, times, device=dev)
    t, dt = pulse.time_samples(lam, times, device=dev)
    A = torch.cat([torch.cat([table.real, -table.imag], 1), torch.cat([table.imag, table.real], 1)])  # [2T, 2C]
    T = table.shape[0]
    B, C, H, W = U.shape
    w5 = torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0], device=dev)[None, :, None, None]

    def syn_real(x):
        out = A @ torch.cat([x.real, x.imag], 1).reshape(B, 2 * C, H * W)
        return torch.complex(out[:, :T], out[:, T:]).reshape(B, T, H, W)

    def syn_einsum(x):
        return torch.einsum("jc,bchw->bjhw", table, x)

    def reduce(E):
        I = E.real ** 2 + E.imag ** 2
        tt, ww = t[None, :, None, None], dt[None, :, None, None]
        Wm = (I * ww).sum(1)
        peak, j = I.max(1)
        tm = (tt * I * ww).sum(1) / Wm
        return torch.stack([Wm, peak, t[j], tm, torch.sqrt((((tt - tm[:, None]) ** 2) * I * ww).sum(1) / Wm)], 1)

    def bwd(fn, loss):
        def run():
            x = U.detach().requires_grad_(True)
            loss(fn(x)).backward()
            return x.grad
        return run

    sq = lambda E: (E.real ** 2 + E.imag ** 2).sum()  # noqa: E731
    wsum = lambda m: (m * w5).sum()  # noqa: E731
    hand_syn = lambda x: pulse.synthesize(x, times, wavelengths=lam)  # noqa: E731
    hand_maps = lambda x: pulse.pulse_maps_tensor(x, times, wavelengths=lam)  # noqa: E731
    return {
        "synthesize": (lambda: hand_syn(U), lambda: syn_real(U), lambda: syn_einsum(U)),
        "synthesize fwd+bwd": (bwd(hand_syn, sq), bwd(syn_real, sq), bwd(syn_einsum, sq)),
        "pulse_maps": (lambda: hand_maps(U), lambda: reduce(syn_real(U)), lambda: reduce(syn_einsum(U))),
        "pulse_maps fwd+bwd": (bwd(hand_maps, wsum), bwd(lambda x: reduce(syn_real(x)), wsum),
                               bwd(lambda x: reduce(syn_einsum(x)), wsum)),
    }


def kernel_ms(fn, names, calls=5):
    """per call, the summed event time of the named kernel families"""
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return sum(_lib.timing_read(n)[0] for n in names) / calls
    finally:
        _lib.timing_enable(False)
        _lib.timing_reset()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pulse_timing.txt"))
    ap.add_argument("--trace", help="B,C,H,W,T: run this shape's four hand paths alone (under the profiler)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.trace:
        B, C, H, W, T = (int(v) for v in args.trace.split(","))
        lam, times = axes(C, T)
        for run in [c[0] for c in contenders(torch.randn(B, C, H, W, dtype=torch.complex64, device=dev), lam, times).values()]:
            for _ in range(5):
                run()
        return torch.cuda.synchronize()
    lines = [f"pulse timing on {torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min .. max); "
             "peak = peak memory above the inputs; a hand kernel that loses to a yardstick is marked **", ""]
    for shape in ((1, 32, 2048, 2048), (3, 32, 1024, 1024)):
        for T in (64, 128):
            B, C, H, W = shape
            lam, times = axes(C, T)
            U = torch.randn(*shape, dtype=torch.complex64, device=dev)
            cs = contenders(U, lam, times)
            pix, maps_b, field_b = B * H * W, B * 5 * H * W * 4, U.numel() * 8
            lines.append(f"[{B}, {C}, {H}, {W}] T = {T}")
            for name, fns in cs.items():
                ms, peaks = rounds(fns, args.rounds)
                med = [statistics.median(m) for m in ms]
                lose = "**" if med[0] > min(med[1:]) else "  "
                lines.append(f"  {lose}{name:<20s} hand {fmt(ms[0])} peak {peaks[0] / 2**20:8.0f} MiB | real {fmt(ms[1])} "
                             f"peak {peaks[1] / 2**20:8.0f} MiB  x{med[1] / med[0]:5.2f} | einsum {fmt(ms[2])} "
                             f"peak {peaks[2] / 2**20:8.0f} MiB  x{med[2] / med[0]:5.2f}")
                if name == "pulse_maps":
                    assert peaks[0] <= maps_b + 2**20, (peaks[0], maps_b)
                if name == "pulse_maps fwd+bwd":
                    assert peaks[0] <= 2 * maps_b + field_b + 2**21, (peaks[0], maps_b, field_b)
            flop, rd = 8.0 * T * C * pix, 8.0 * C * pix
            for name, fams, wr in (("synthesize", ["pulse_synthesize"], 8.0 * T * pix), ("pulse_maps", ["pulse_maps"], 20.0 * pix)):
                k = kernel_ms(cs[name][0], fams) * 1e-3
                lines.append(f"    kernel {name:<12s} {k * 1e3:8.3f} ms  {flop / k / 1e12:6.1f} TFLOP/s  "
                             f"{(rd + wr) / k / 1e9:7.0f} GB/s  ({flop / (rd + wr):5.1f} flop/B)")
            for name, fams in (("adjoint", ["pulse_adjoint"]), ("maps_bwd", ["pulse_maps_bwd"])):
                which = "synthesize fwd+bwd" if name == "adjoint" else "pulse_maps fwd+bwd"
                k = kernel_ms(cs[which][0], fams) * 1e-3
                lines.append(f"    kernel {name:<12s} {k * 1e3:8.3f} ms  {(2 if name == 'maps_bwd' else 1) * flop / k / 1e12:6.1f} TFLOP/s")
            lines.append("")
            del U, cs
            torch.cuda.empty_cache()
    lines.append("memory asserted: pulse_maps allocates the five maps; forward + backward the five maps, their [B, 5, H, W] "
                 "gradient and the field-sized gradient; no [B, T, H, W] tensor.  Traffic counters: not read.")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
