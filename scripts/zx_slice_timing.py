#!/usr/bin/env python
"""Time ASM_prop.propagate_zx against propagate_planes at cfg2 geometry (4096^2 Gaussian beam,
P = 8192, dx 0.25 mm, 300 GHz, the 20-120 mm sweep of experiment_extend_depth_of_focus.ipynb:229).

Per-kernel HIP-event times (thz_timing_*), warm-up calls first, then --calls timed calls of
  propagate_zx, 64 planes      (asm_rows_fwd + asm_cols_slice + asm_rows_slice)
  propagate_zx, 200 planes     (the notebook's prop_range)
  propagate_planes, 64 planes  (asm_rows_fwd + asm_cols + asm_rows_inv), same run
and the peak device memory each allocates above the input field.  One JSON document to --out.

Expectation (the z-x slice section): the 64-plane slice takes less than the full path's
asm_cols time of the same run, and its peak memory stays under T + 64 MB.

    python scripts/zx_slice_timing.py --out profiles/zx_slice_timing.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

C0 = 2.998e8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/zx_slice_timing.json")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=4096, help="field size (padded to 2 n)")
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls must be at least 10")

    from quantizationawarethzdoe_amd import _lib, propagation as P
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    from quantizationawarethzdoe_amd.optics import gaussian_beam

    dev = torch.device("cuda:0")
    N = args.n
    lam = float(torch.tensor(C0 / 300e9, dtype=torch.float32))
    dx = float(torch.tensor(0.25e-3, dtype=torch.float32))
    x = gaussian_beam(N, N, dx, dx, [lam], [50e-3], [50e-3], device=dev)
    field = ElectricField(x, wavelengths=lam, spacing=[dx, dx], device=dev)
    prop = ASM_prop(z_distance=0.02, padding_scale=1, device=dev)
    prop.check_Zc = False
    z64 = [float(v) for v in torch.linspace(20e-3, 120e-3, 64, dtype=torch.float64)]
    z200 = [float(v) for v in np.linspace(20e-3, 120e-3, num=200)]
    ncols, zc = P.asm_plan_info(1, 1, N, N, N // 2, N // 2, True, 1, [lam], [dx, dx], z64)
    t_bytes = (ncols + 15) // 16 * 16 * N * 8

    def measure(fn, kernels):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        _lib.timing_enable(True)
        _lib.timing_reset()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.calls * 1e3
        per = {}
        for k in kernels:
            ms, n = _lib.timing_read(k)
            per[k] = {"ms_per_call": ms / args.calls, "launches_per_call": n / args.calls}
        _lib.timing_enable(False)
        return {"kernels": per, "kernel_ms_per_call": sum(v["ms_per_call"] for v in per.values()),
                "wall_ms_per_call": wall, "peak_bytes_above_input": torch.cuda.max_memory_allocated() - base}

    slice_k = ["asm_rows_fwd", "asm_cols_slice", "asm_rows_slice"]
    res = {
        "geometry": {"n": N, "padded": 2 * N, "dx": dx, "wavelength": lam, "band_columns": ncols,
                     "full_path_z_chunk": zc, "T_bytes": t_bytes},
        "calls": args.calls, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0), "library": _lib.version(),
        "zx_64": measure(lambda: prop.propagate_zx(field, z64), slice_k),
        "zx_200": measure(lambda: prop.propagate_zx(field, z200), slice_k),
        "planes_64": measure(lambda: prop.propagate_planes(field, z64), ["asm_rows_fwd", "asm_cols", "asm_rows_inv"]),
    }
    k2 = res["planes_64"]["kernels"]["asm_cols"]["ms_per_call"]
    res["expectation"] = {
        "zx_64_kernel_ms": res["zx_64"]["kernel_ms_per_call"], "full_path_asm_cols_ms": k2,
        "time_met": res["zx_64"]["kernel_ms_per_call"] < k2,
        "zx_64_peak_bytes": res["zx_64"]["peak_bytes_above_input"], "T_plus_64MB": t_bytes + (64 << 20),
        "memory_met": res["zx_64"]["peak_bytes_above_input"] < t_bytes + (64 << 20),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res["expectation"]))


if __name__ == "__main__":
    main()
