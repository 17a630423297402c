#!/usr/bin/env python
"""Time RSC_prop.propagate_zx against Z calls of RSC_prop.forward: a 1024^2 field (seeded white
input), lambda = 1 mm, dx = 0.25 mm, Z = 64 planes in 20 ... 120 mm, centre row.

Two ways to the same [Z, 1, 1, 1024] map, alternated --reps times after --warmup rounds, each timed
with HIP events around the whole map:
  native : prop.propagate_zx(field, zs)                  (thz_rsc_slice_forward)
  loop   : prop.z = z; prop(field).data[..., row, :]     per plane -- all there was before
then, in a pass of its own, the native path's per-kernel HIP-event times (thz_timing_*), the
relative L2 between the two maps, and the slice kernels' register / scratch / occupancy lines from
the compiler's resource summary (--resources FILE: lines collected beforehand with
`hipcc -Rpass-analysis=kernel-resource-usage`; without it the script compiles csrc/thz_rsc.hip for
the summary itself).  Plain text to --out.

    python scripts/rsc_zx_timing.py --out profiles/rsc_zx_timing.txt
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def resource_lines(path=None):
    """One line per rsc_slice_* kernel: VGPRs, SGPRs, scratch bytes per lane, waves per SIMD."""
    if path:
        with open(path) as fh:
            text = fh.read()
    else:
        src = os.path.join(ROOT, "quantizationawarethzdoe_amd", "csrc", "thz_rsc.hip")
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        text = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize",
                               "-munsafe-fp-atomics", "-c", "-Rpass-analysis=kernel-resource-usage", src, "-o",
                               os.devnull], capture_output=True, text=True).stderr
    out = []
    for block in re.split(r"(?=remark: Function Name)", text):
        m = re.search(r"Function Name: _ZN3thz\d+(rsc_slice_\w+?)ILi(\d+)E(?:Li(\d+)E)?E", block)
        if not m:
            continue

        def val(key):
            return int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        name = f"{m.group(1)}<{m.group(2)}{', ' + m.group(3) if m.group(3) else ''}>"
        out.append(f"  {name:26s} {val('VGPRs'):4d} VGPRs {val('TotalSGPRs'):4d} SGPRs  scratch "
                   f"{val('ScratchSize [bytes/lane]'):3d} B/lane  {val('Occupancy [waves/SIMD]')} waves/SIMD")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rsc_zx_timing.txt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()

    from quantizationawarethzdoe_amd import _lib
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop

    if not torch.cuda.is_available():
        sys.exit("rsc_zx_timing: needs a ROCm GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    N, Z = args.n, args.planes
    torch.manual_seed(3000)
    x = torch.randn(1, 1, N, N, dtype=torch.complex64, device=dev)
    field = ElectricField(x, wavelengths=1e-3, spacing=[0.25e-3, 0.25e-3], device=dev)
    zs = [float(v) for v in torch.linspace(20e-3, 120e-3, Z, dtype=torch.float64)]
    row = N // 2
    prop, stepper = RSC_prop(z_distance=zs[0], device=dev), RSC_prop(z_distance=zs[0], device=dev)
    prop.check_Zc = stepper.check_Zc = False   # no minimum-distance print in the timed loop

    def native():
        return prop.propagate_zx(field, zs, row=row)

    def loop():
        rows = []
        for z in zs:
            stepper.z = z
            rows.append(stepper(field).data[..., row, :])
        return torch.stack(rows)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    with torch.no_grad():
        for _ in range(args.warmup):
            native()
            loop()
        torch.cuda.synchronize()
        tn, tl = [], []
        for _ in range(args.reps):
            t, a = timed(native)
            tn.append(t)
            t, b = timed(loop)
            tl.append(t)
        rel = float((a - b).norm() / b.norm())
        kernels = ["rsc_slice_rows", "rsc_slice_acc", "rsc_slice_line"]
        _lib.timing_enable(True)
        _lib.timing_reset()
        for _ in range(args.reps):
            native()
        per = {k: _lib.timing_read(k) for k in kernels}
        _lib.timing_enable(False)

    ksum = sum(ms for ms, _ in per.values())
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = [
        f"RSC z-x slice timing: {N}^2 field, lambda 1 mm, dx 0.25 mm, Z = {Z} planes in 20 ... 120 mm, row {row}",
        f"device {torch.cuda.get_device_name(0)}, library {_lib.version()}, {args.reps} alternated reps after "
        f"{args.warmup} warm-up rounds, HIP events around the whole map",
        f"native propagate_zx      : median {med(tn):9.3f} ms  (min {min(tn):.3f}, max {max(tn):.3f})",
        f"Z x forward, sliced      : median {med(tl):9.3f} ms  (min {min(tl):.3f}, max {max(tl):.3f})",
        f"ratio loop / native      : {med(tl) / med(tn):.2f}",
        f"slowest native rep faster than the fastest loop rep: {max(tn) < min(tl)}",
        f"relative L2 native vs loop: {rel:.3e}",
        "native per-kernel HIP-event time per map (separate pass):",
    ]
    for k in kernels:
        ms, n = per[k]
        lines.append(f"  {k:20s} {ms / args.reps:9.3f} ms  ({n / args.reps:.0f} launches, "
                     f"{100 * ms / ksum:.1f} % of the kernel time)")
    P = 2 * N
    evals = float(Z) * N * P
    ms_acc = per["rsc_slice_acc"][0] / args.reps
    lines.append(f"accumulate kernel: {Z * N} kernel rows of {P} points per map = {evals:.3e} RS-kernel evaluations "
                 f"and {Z * N} transforms, {evals / (ms_acc * 1e-3) / 1e9:.1f} G evaluations/s; Uh read once per plane "
                 f"{Z * N * P * 8 / 2 ** 30:.2f} GiB -> {Z * N * P * 8 / (ms_acc * 1e-3) / 1e12:.2f} TB/s")
    lines.append("slice kernels' resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
    lines += resource_lines(args.resources)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
