"""Timings of the FDTD validator (profiles/fdtd_timing.txt): time per step and the byte-model rate of the two step
kernels, the same two passes written with torch ops as the baseline, and one run at the reference's scale.

    python scripts/fdtd_timing.py [--out profiles/fdtd_timing.txt]      every case, each a child under its own timeout
    python scripts/fdtd_timing.py --case NAME                            one case, its lines on stdout

HIP events around 20 steps, 5 warm-ups, the median of 5.  Byte model: 76 B per cell and step (H pass 36, E pass 36
plus the material word, rounded as the design states it) against 8.0 TB/s.  Traffic counters were not read.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAM, CPW, STEPS = 1e-3, 8, 20
CASES = {"256x256x512": (512, 256, 256), "512x512x1024": (1024, 512, 512), "2d-4096x4096": (4096, 1, 4096)}
LIMITS = {"256x256x512": 240, "512x512x1024": 300, "2d-4096x4096": 240, "reference-scale": 900}


def _median_ms(fn):
    import torch
    for _ in range(5):
        fn()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / STEPS)
    return statistics.median(out)


def _torch_steps(f, S):
    """The two passes as torch ops: roll differences, periodic in every direction, no CPML, vacuum."""
    import torch
    ex, ey, ez, hx, hy, hz = f
    d = lambda a, ax: torch.roll(a, -1, ax) - a
    b = lambda a, ax: a - torch.roll(a, 1, ax)
    for _ in range(STEPS):
        hx -= S * (d(ez, 1) - d(ey, 0))
        hy -= S * (d(ex, 0) - d(ez, 2))
        hz -= S * (d(ey, 2) - d(ex, 1))
        ex += S * (b(hz, 1) - b(hy, 0))
        ey += S * (b(hx, 0) - b(hz, 2))
        ez += S * (b(hy, 2) - b(hx, 1))


def case_grid(name):
    import torch
    from quantizationawarethzdoe_amd import fdtd
    Nz, Ny, Nx = CASES[name]
    dev = torch.device("cuda:0")
    delta = LAM / CPW
    g = torch.Generator().manual_seed(0)
    H = 1 if Ny == 1 else Ny
    h = torch.rand(H, Nx, generator=g) * 32 * delta
    back = Nz - 2 * 12 - 8 - 16 - 32
    sim = fdtd.FDTDValidator(h, pixel=delta, wavelength=LAM, thickness=32 * delta, base=16 * delta,
                             cells_per_wavelength=CPW, gap_front=8 * delta, gap_back=back * delta,
                             ny_cells=1 if Ny == 1 else None, device=dev)
    assert (sim.Nz, sim.Ny, sim.Nx) == (Nz, Ny, Nx)
    st = sim.start(planes=[40 * delta], row=0, settle_periods=2, acc_periods=2, n_table=11 * STEPS)
    ms = _median_ms(lambda: st.advance(STEPS))
    cells = Nz * Ny * Nx
    rate = 76.0 * cells / (ms * 1e-3) / 1e12
    print(f"fdtd-timing {name:<16s} kernels  {ms * 1e3:9.1f} us/step  {cells / ms / 1e6:8.1f} Gcell/s  byte model "
          f"{rate:5.2f} TB/s = {100 * rate / 8.0:4.1f} % of 8.0 TB/s")
    f = [torch.zeros(Nz, Ny, Nx, device=dev) for _ in range(6)]
    f[0][Nz // 2] = 1.0
    tms = _median_ms(lambda: _torch_steps(f, 0.5))
    print(f"fdtd-timing {name:<16s} torch    {tms * 1e3:9.1f} us/step  (roll differences, no CPML, no material)  "
          f"kernels faster by {tms / ms:5.2f} x")


def case_reference():
    import numpy as np
    import torch
    from quantizationawarethzdoe_amd import fdtd
    dev = torch.device("cuda:0")
    h = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "fdtd_beam_splitter_height.npy")))
    # the recorded map has four levels, 0 .. 0.75 mm, so the relief is 1 mm thick (not the 4 mm of a general
    # element); the back gap is chosen so that the domain is 50 wavelengths deep as the reference's is:
    # 2 x 12 PML cells + (3 + 2 + 1 + 42.4) mm at 15 cells per mm = 750 planes
    sim = fdtd.FDTDValidator(h, pixel=1e-3, wavelength=1e-3, material=[2.66, 0.03], thickness=1e-3, base=2e-3,
                             cells_per_wavelength=15, gap_front=3e-3, gap_back=42.4e-3, device=dev)
    cells = sim.Nz * sim.Ny * sim.Nx
    torch.cuda.reset_peak_memory_stats(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = sim.run(row=sim.Ny // 2, planes=[40e-3])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    amp = float(res.zx[0].abs().max())
    print(f"fdtd-timing reference-scale  80 x 80 beam splitter, 15 cells per wavelength: grid {res.grid} = {cells / 1e9:.3f}e9 "
          f"cells, {res.steps} steps, wall {wall:.1f} s = {wall / res.steps * 1e3:.2f} ms/step (byte model "
          f"{76.0 * cells * res.steps / wall / 1e12:.2f} TB/s), peak memory {peak:.1f} GiB, max |Ex| on the slice {amp:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fdtd_timing.txt"))
    ap.add_argument("--skip", nargs="*", default=[])
    a = ap.parse_args()
    if a.case:
        case_reference() if a.case == "reference-scale" else case_grid(a.case)
        return 0
    lines = ["# scripts/fdtd_timing.py: HIP events around 20 steps, 5 warm-ups, median of 5; traffic counters not read"]
    for name in list(CASES) + ["reference-scale"]:
        if name in a.skip:
            continue
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--case",
                            name], capture_output=True, text=True)
        got = [l for l in r.stdout.splitlines() if l.startswith("fdtd-timing")]
        print("\n".join(got) if got else r.stdout + r.stderr, flush=True)
        if r.returncode != 0:   # nothing more on the GPU after a failure
            print(f"fdtd-timing {name}: exit status {r.returncode}; stopping", flush=True)
            print(r.stderr[-2000:])
            return r.returncode
        lines += got
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
