#!/usr/bin/env python
"""Time a differentiated ASM_prop.propagate_zx at cfg2 geometry (4096^2 Gaussian beam, P = 8192,
dx 0.25 mm, 300 GHz, 64 planes of the 20-120 mm sweep) under its two ``grad`` forms:

  grad="slice"   forward  asm_rows_fwd + asm_cols_slice + asm_rows_slice
                 backward asm_rows_fwd (the cotangent rows) + asm_cols_slice_adj + asm_rows_inv
  grad="planes"  forward  asm_rows_fwd + asm_cols + asm_rows_inv (the full planes, sliced)
                 backward the full path's Z-summing adjoint of the zero-embedded cotangent

Per-kernel HIP-event times (thz_timing_*), forward and backward read separately, warm-up calls
first, then --calls timed forward+backward calls of each form in one run, and the peak device memory
each allocates above the input field.  One JSON document to --out.

Expectation (the slice-adjoint section): forward+backward under grad="slice" takes less
kernel time than the grad="planes" forward alone, and its peak memory is under one tenth of the
planes form's.

    python scripts/zx_slice_grad_timing.py --out profiles/zx_slice_grad_timing.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

C0 = 2.998e8
FWD = {"slice": ["asm_rows_fwd", "asm_cols_slice", "asm_rows_slice"], "planes": ["asm_rows_fwd", "asm_cols", "asm_rows_inv"]}
BWD = {"slice": ["asm_rows_fwd", "asm_cols_slice_adj", "asm_rows_inv"], "planes": ["asm_rows_fwd", "asm_cols", "asm_rows_inv"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/zx_slice_grad_timing.json")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=4096, help="field size (padded to 2 n)")
    ap.add_argument("--planes", type=int, default=64)
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls must be at least 10")

    from quantizationawarethzdoe_amd import _lib, propagation as P
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    from quantizationawarethzdoe_amd.optics import gaussian_beam

    dev = torch.device("cuda:0")
    N, Z = args.n, args.planes
    lam = float(torch.tensor(C0 / 300e9, dtype=torch.float32))
    dx = float(torch.tensor(0.25e-3, dtype=torch.float32))
    x = gaussian_beam(N, N, dx, dx, [lam], [50e-3], [50e-3], device=dev).reshape(1, 1, N, N).requires_grad_(True)
    field = ElectricField(x, wavelengths=lam, spacing=[dx, dx], device=dev)
    prop = ASM_prop(z_distance=0.02, padding_scale=1, device=dev)
    prop.check_Zc = False
    zs = [float(v) for v in torch.linspace(20e-3, 120e-3, Z, dtype=torch.float64)]
    gen = torch.Generator(device=dev).manual_seed(1)
    g = torch.randn(Z, 1, 1, N, dtype=torch.complex64, device=dev, generator=gen)
    ncols, zc = P.asm_plan_info(1, 1, N, N, N // 2, N // 2, True, 1, [lam], [dx, dx], zs)

    def read(names, into):
        for k in names:
            ms, n = _lib.timing_read(k)  # synchronises on the pending events
            into.setdefault(k, [0.0, 0])
            into[k][0] += ms
            into[k][1] += n

    def measure(form):
        def step(fwd=None, bwd=None):
            if fwd is not None:
                _lib.timing_reset()
            zx = prop.propagate_zx(field, zs, row=N // 2, grad=form)
            if fwd is not None:
                read(FWD[form], fwd)
                _lib.timing_reset()
            gx, = torch.autograd.grad(zx, x, grad_outputs=g)
            if bwd is not None:
                read(BWD[form], bwd)
            return gx

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            step()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.calls * 1e3
        peak = torch.cuda.max_memory_allocated() - base
        fwd, bwd = {}, {}
        _lib.timing_enable(True)
        for _ in range(args.calls):
            step(fwd, bwd)
        _lib.timing_enable(False)

        def per(d):
            return {k: {"ms_per_call": v[0] / args.calls, "launches_per_call": v[1] / args.calls} for k, v in d.items()}

        f, b = per(fwd), per(bwd)
        fms, bms = (sum(v["ms_per_call"] for v in d.values()) for d in (f, b))
        return {"forward_kernels": f, "backward_kernels": b, "forward_kernel_ms": fms, "backward_kernel_ms": bms,
                "kernel_ms_per_call": fms + bms, "wall_ms_per_call_untimed": wall, "peak_bytes_above_input": peak}

    res = {
        "geometry": {"n": N, "padded": 2 * N, "planes": Z, "dx": dx, "wavelength": lam, "band_columns": ncols,
                     "full_path_z_chunk": zc},
        "calls": args.calls, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "library": _lib.version(),
        "slice": measure("slice"),
        "planes": measure("planes"),
    }
    s, p = res["slice"], res["planes"]
    res["expectation"] = {
        "slice_forward_plus_backward_kernel_ms": s["kernel_ms_per_call"],
        "planes_forward_kernel_ms": p["forward_kernel_ms"],
        "time_met": s["kernel_ms_per_call"] < p["forward_kernel_ms"],
        "slice_peak_bytes": s["peak_bytes_above_input"], "planes_peak_bytes": p["peak_bytes_above_input"],
        "memory_met": s["peak_bytes_above_input"] < p["peak_bytes_above_input"] / 10,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res["expectation"]))


if __name__ == "__main__":
    main()
