#!/usr/bin/env python
"""Time forward plus backward of RSC_prop.propagate_zx(grad="slice") against grad="planes" on the
workload of scripts/rsc_zx_timing.py (a 1024^2 field, lambda = 1 mm, dx = 0.25 mm, seeded white input)
over Z = 64 planes in 20 ... 120 mm, centre row, loss out.abs().square().sum().  grad="planes" is what
a field that requires grad took before the slice had a backward, and still takes by default.

The two forms are alternated --reps times after --warmup rounds, each step (forward, loss, backward
to the field) timed with HIP events around the whole step.  Then, in passes of their own, each
form's torch.cuda.max_memory_allocated over one step and the native form's per-kernel HIP-event
times (thz_timing_*), and the relative L2 between the two gradients.  Plain text to --out.

    python scripts/rsc_zx_grad_timing.py --out profiles/rsc_zx_grad_timing.txt
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rsc_zx_grad_timing.txt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--vectorial", action="store_true", help="VRS_prop on an Ex / Ey pair")
    args = ap.parse_args()

    from quantizationawarethzdoe_amd import _lib
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop, VRS_prop

    if not torch.cuda.is_available():
        sys.exit("rsc_zx_grad_timing: needs a ROCm GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    N, Z, vec = args.n, args.planes, args.vectorial
    B, Bo = (2, 3) if vec else (1, 1)
    torch.manual_seed(3000)
    x = torch.randn(B, 1, N, N, dtype=torch.complex64, device=dev).requires_grad_(True)
    field = ElectricField(x, wavelengths=1e-3, spacing=[0.25e-3, 0.25e-3], device=dev)
    zs = [float(v) for v in torch.linspace(20e-3, 120e-3, Z, dtype=torch.float64)]
    Ho = Wo = 2 * (N // 2)
    row = Ho // 2
    prop = (VRS_prop if vec else RSC_prop)(z_distance=zs[0], device=dev)
    prop.check_Zc = False   # no minimum-distance print in the timed region

    def step(mode):
        out = prop.propagate_zx(field, zs, row=row, grad=mode)
        gx, = torch.autograd.grad(out.abs().square().sum(), x)
        return gx

    def timed(mode):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        gx = step(mode)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), gx

    def peak(mode):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(mode)
        torch.cuda.synchronize()
        return base, torch.cuda.max_memory_allocated()

    for _ in range(args.warmup):
        step("slice")
        step("planes")
    torch.cuda.synchronize()
    ts, tp = [], []
    for _ in range(args.reps):
        t, gs = timed("slice")
        ts.append(t)
        t, gp = timed("planes")
        tp.append(t)
    rel = float((gs - gp).norm() / gp.norm())
    del gs, gp
    mem = {mode: peak(mode) for mode in ("slice", "planes")}
    kernels = ["rsc_slice_rows", "rsc_slice_acc", "rsc_slice_line", "rsc_slice_line_adj", "rsc_slice_acc_adj",
               "rsc_slice_rows_adj"]
    _lib.timing_enable(True)
    _lib.timing_reset()
    for _ in range(args.reps):
        step("slice")
    per = {k: _lib.timing_read(k) for k in kernels}
    _lib.timing_enable(False)

    ksum = sum(ms for ms, _ in per.values())
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    gib = 2.0 ** 30
    lines = [
        f"{'VRS' if vec else 'RSC'} z-x slice, forward + backward: {N}^2 field, lambda 1 mm, dx 0.25 mm, Z = {Z} planes "
        f"in 20 ... 120 mm, row {row}, loss sum |zx|^2",
        f"device {torch.cuda.get_device_name(0)}, library {_lib.version()}, {args.reps} alternated reps after "
        f"{args.warmup} warm-up rounds, HIP events around the whole step",
        f"grad='slice'  (native)   : median {med(ts):9.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f})  "
        f"reps {' '.join(f'{t:.3f}' for t in ts)}",
        f"grad='planes' (full)     : median {med(tp):9.3f} ms  (min {min(tp):.3f}, max {max(tp):.3f})  "
        f"reps {' '.join(f'{t:.3f}' for t in tp)}",
        f"ratio planes / slice     : {med(tp) / med(ts):.2f}",
        f"every native rep faster than every planes rep: {max(ts) < min(tp)}",
        f"relative L2 of the field gradient, slice vs planes: {rel:.3e}",
    ]
    stack = 8.0 * Z * Bo * Ho * Wo
    lines.append(f"one plane stack [Z, Bo, C, Ho, Wo] complex64: {stack / gib:.3f} GiB; grad='slice' peaks below it: "
                 f"{mem['slice'][1] - mem['slice'][0] < stack}")
    for mode in ("slice", "planes"):
        base, pk = mem[mode]
        lines.append(f"max_memory_allocated over one step, grad='{mode}': {pk / gib:8.3f} GiB "
                     f"({(pk - base) / gib:.3f} GiB above the {base / gib:.3f} GiB held before it)")
    lines.append("native per-kernel HIP-event time per step (separate pass):")
    for k in kernels:
        ms, n = per[k]
        lines.append(f"  {k:20s} {ms / args.reps:9.3f} ms  ({n / args.reps:.0f} launches, "
                     f"{100 * ms / ksum:.1f} % of the kernel time)")
    rows = float(Z) * N   # kernel rows evaluated and transformed, per direction
    for k in ("rsc_slice_acc", "rsc_slice_acc_adj"):
        ms = per[k][0] / args.reps
        lines.append(f"{k}: {rows:.0f} kernel rows of {N + 2 * (N // 2)} points per step, "
                     f"{rows / (ms * 1e-3) / 1e6:.2f} M rows/s")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
