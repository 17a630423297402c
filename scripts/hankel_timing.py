#!/usr/bin/env python
"""Time the Hankel propagator (hankel.hankel_propagate) on the current GPU and write profiles/hankel_timing.txt.

  (a) propagate_zr at N in {512, 2048, 4096}, B C in {1, 32}, Z = 64, keep = N and keep = 1
  (b) the same algebra as torch ops on the same card: torch.matmul on the exported fp32 T with a materialised H, as
      real products (re and im stacked as two right-hand sides, the stacking and the return to complex included) --
      the yardstick; and, for the record, the same with T cast to complex64, which does twice the real arithmetic
  (c) ASM_prop.propagate_zx on the 2-D field of the same aperture and sampling (N = 2048 against 4096^2, P = 8192)
  (d) forward + backward of the design step of Props/Hankel_Prop.py's docstring

HIP events around each call, every shape warmed up, the contenders of a shape alternated round by round; medians
and the spread (min .. max) over the rounds.  The event time of a call includes its five launches.

Kernel time comes from a profiler run of its own (scripts/hankel_trace.sh): ``--trace N,BC,keep`` runs one shape
under ``rocprofv3 --kernel-trace --stats``, and ``--trace-summary DIR`` turns the kernel statistics of those runs
into kernel time per call and achieved FLOP/s and bytes/s on the operation and byte model below.  No counter is read.
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import doe, hankel  # noqa: E402
from quantizationawarethzdoe_amd.Props.Hankel_Prop import Hankel_prop  # noqa: E402

LAM = 1e-3


def model(N, BC, Z, keep):
    """(flop, bytes) of one forward: two real products on 2 BC and 2 Z BC real columns; T read once per product
    (once per column block of 128), H, the profile, F and the output once"""
    flop = 2.0 * N * N * 2 * BC + 2.0 * keep * N * 2 * Z * BC
    blocks = -(-2 * Z * BC // 128)
    byts = 4.0 * N * N + 4.0 * keep * N * blocks + 8.0 * (Z * N + 2 * BC * N + Z * BC * keep)
    return flop, byts


def rounds(fns, n):
    """the contenders alternated round by round -> per contender the list of milliseconds"""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(n):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return ms


def fmt(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} .. {max(v):.3f})"


def trace_shape(spec, calls):
    """one shape, ``calls`` forwards after 3 warm-up calls, for a profiler run of its own"""
    N, BC, keep = (int(v) for v in spec.split(","))
    dev = torch.device("cuda:0")
    f = torch.randn(1, BC, N, dtype=torch.complex64, device=dev)
    zs = [0.05 + 0.002 * i for i in range(64)]
    for _ in range(3 + calls):
        hankel.hankel_propagate(f, [LAM] * BC, N * LAM, zs, keep=keep)
    torch.cuda.synchronize()


def trace_summary(root, out):
    """DIR/<N>_<BC>_<keep>/**/*kernel_stats.csv -> kernel time per forward call (every hankel_* kernel; a call
    launches hankel_tf once) and the model's rates over it"""
    lines = ["", "kernel time per forward call, rocprofv3 --kernel-trace --stats, one run per shape (Z = 64):"]
    for d in sorted(glob.glob(os.path.join(root, "*_*_*")), key=lambda p: [int(v) for v in os.path.basename(p).split("_")]):
        N, BC, keep = (int(v) for v in os.path.basename(d).split("_"))
        ns = {"hankel_tf": 0.0, "hankel_gemm": 0.0, "hankel_finish": 0.0}
        calls = 0
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in ns:
                    if k + "_kernel" in row["Name"]:
                        ns[k] += float(row["TotalDurationNs"])
                        calls += int(row["Calls"]) if k == "hankel_tf" else 0
        if not calls:
            continue
        t = sum(ns.values()) / calls * 1e-9
        flop, byts = model(N, BC, 64, keep)
        lines.append(f"N {N:5d} BC {BC:3d} keep {keep:5d}: {t * 1e6:8.1f} us (tf {ns['hankel_tf'] / calls / 1e3:6.1f} "
                     f"gemm {ns['hankel_gemm'] / calls / 1e3:7.1f} finish {ns['hankel_finish'] / calls / 1e3:7.1f})  "
                     f"{flop / t / 1e12:6.2f} TFLOP/s {byts / t / 1e9:7.1f} GB/s  {flop / byts:6.1f} flop/B")
    with open(out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hankel_timing.txt"))
    ap.add_argument("--trace", help="N,BC,keep: run this shape alone (under the profiler)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--trace-summary", help="directory of the profiler runs: append kernel times to --out")
    args = ap.parse_args()
    if args.trace:
        return trace_shape(args.trace, args.calls)
    if args.trace_summary:
        return trace_summary(args.trace_summary, args.out)
    dev = torch.device("cuda:0")
    lines = [f"Hankel propagator timing on {torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min .. max)", ""]
    Z = 64
    zs = [0.05 + 0.002 * i for i in range(Z)]
    for N in (512, 2048, 4096):
        t0 = time.perf_counter()
        T, w, _ = hankel.hankel_table(N, dev)
        torch.cuda.synchronize()
        lines.append(f"table N = {N}: built and exported in {time.perf_counter() - t0:.2f} s (host, extended precision)")
        r_max = N * LAM
        for BC in (1, 32):
            f = torch.randn(1, BC, N, dtype=torch.complex64, device=dev)
            lams = [LAM] * BC
            H = hankel.hankel_transfer_function(lams, r_max, zs, N, dev)
            Tc = T.to(torch.complex64)
            for keep in (N, 1):
                def hand():
                    return hankel.hankel_propagate(f, lams, r_max, zs, keep=keep)

                def torch_real():  # T is real: re and im are two right-hand sides of a real product
                    x = w * f
                    F = torch.stack((x.real, x.imag)) @ T.T
                    G = H[:, None] * torch.complex(F[0], F[1])[None]
                    out = torch.stack((G.real, G.imag)) @ T[:keep].T
                    return torch.complex(out[0], out[1]) / w[:keep]

                def torch_cast():  # T cast to complex64: twice the real arithmetic
                    F = (w * f) @ Tc.T
                    return ((H[:, None] * F[None]) @ Tc[:keep].T) / w[:keep]

                err = float((hand() - torch_real()).norm() / torch_real().norm())
                mh, mt, mc = rounds([hand, torch_real, torch_cast], args.rounds)
                flop, byts = model(N, BC, Z, keep)
                t = statistics.median(mh) * 1e-3
                lines.append(f"N {N:5d} BC {BC:3d} Z {Z} keep {keep:5d}: hand {fmt(mh)}  torch real {fmt(mt)}  "
                             f"torch / hand {statistics.median(mt) / statistics.median(mh):5.2f}  "
                             f"(T as complex64 {fmt(mc)})  over the call: {flop / t / 1e12:6.2f} TFLOP/s "
                             f"{byts / t / 1e9:7.1f} GB/s  rel diff {err:.1e}")
    # (d) the design step: profile -> sample_rings -> modulate -> propagate_zr -> on-axis intensity -> backward
    N, r_max = 2048, 2048 * LAM
    prop = Hankel_prop(0.1, N, r_max, device=dev)
    beam = torch.exp(-(prop.r / (0.2 * r_max)) ** 2).to(torch.complex64).view(1, 1, 1, -1)
    profile = (torch.rand(1024, device=dev) * 1e-3).requires_grad_(True)

    def step():
        profile.grad = None
        height = prop.sample_rings(profile, r_max / 1024).float().view(1, -1)
        field, _ = doe.modulate(beam, height, [LAM], 2.66, 0.03)
        axis = prop.propagate_zr(field.view(1, 1, -1), [LAM], zs, keep=1)
        (-(axis.abs() ** 2).sum()).backward()

    lines += ["", f"design step N = 2048, Z = 64, keep = 1, forward + backward: {fmt(rounds([step], args.rounds)[0])}"]
    # (c) the 2-D path on the same aperture and sampling
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    x = torch.randn(1, 1, 4096, 4096, dtype=torch.complex64, device=dev)
    field = ElectricField(x, wavelengths=LAM, spacing=[LAM / 2, LAM / 2], device=dev)
    asm = ASM_prop(z_distance=0.05, padding_scale=1, device=dev)
    f1 = torch.randn(1, 1, N, dtype=torch.complex64, device=dev)
    m2, m1 = rounds([lambda: asm.propagate_zx(field, zs), lambda: hankel.hankel_propagate(f1, [LAM], r_max, zs)],
                    max(5, args.rounds // 2))
    lines.append(f"ASM_prop.propagate_zx 4096^2 (P = 8192), 64 planes: {fmt(m2)};  Hankel N = 2048, 64 planes: {fmt(m1)}"
                 f"  ratio {statistics.median(m2) / statistics.median(m1):.1f}")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
