"""Timing of the IFTA projections (optics.ifta_target_stats / ifta_target_project / ifta_doe_project) and of a
whole designer iteration (ifta.IFTA) against the same iteration written with torch ops on the same propagator.

A 2048^2 field (padding_scale 1: P = 4096), a 1024^2 DOE (2 x 2 pixels per cell), four levels, one plane and four
planes.  Per kernel: device events around `reps` calls on a ring of inputs larger than the 256 MB last-level
cache, the median of `rounds` rounds.  Per iteration: a run of `iters` iterations, eager and as one graph replay,
over `iters`.  Byte model: stats 12 B / pixel read (13 with a window); project 12 B read (13 with a
window) + 8 B written; doe 8 B / pixel read (16 with an incident field) + 8 B / cell written.  The TB/s figures
divide the model's bytes by the time; traffic counters were not read.

    python scripts/ifta_timing.py [--out profiles/ifta_timing.txt]
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import doe as _doe  # noqa: E402
from quantizationawarethzdoe_amd import ifta, optics  # noqa: E402
from quantizationawarethzdoe_amd import propagation as _prop  # noqa: E402
from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop  # noqa: E402

LAM, EPS, TAND = 2.998e8 / 300e9, 2.66, 0.03


def timed(fn, inputs, reps, rounds):
    for x in inputs:
        fn(x)
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r in range(reps):
            fn(inputs[r % len(inputs)])
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def torch_iteration(des, st, h, q, T, window):
    """One iteration with torch ops between the same fused forward and the same adjoint."""
    field, asm = st["field"], des.asm
    data = field._data
    _, _, H, W = data.shape
    Z = len(des.zs)
    hs, ws = des.doe_shape
    ph, pw = asm.compute_padding(H, W, return_size_of_padding=True)
    wl, sp, bl = field.wavelengths_host, field.spacing_host, asm._bandlimit_code()
    field._pending = _doe.PendingModulation(data, h, wl, des.eps, des.tand, tolerance=None)
    U = asm.propagate_planes(field, des.zs).reshape(Z, H, W)
    a = U.abs()
    w = torch.ones((), device=U.device) if window is None else window.float()
    s_tu = (T * a * w).double().sum((-2, -1))
    s_tt = (T * T * w).double().sum((-2, -1)).expand(Z)
    s_all, s_in = (a * a).double().sum((-2, -1)), (a * a * w).double().sum((-2, -1))
    s = torch.where(s_tt == 0, torch.zeros_like(s_tu), s_tu / s_tt)
    row = torch.stack((s_all, s_in, s_tu, s_tt, s, s_in / s_all), dim=-1)
    new = torch.clamp(des.alpha * s.float().reshape(Z, 1, 1) * T + (1 - des.alpha) * a, min=0)
    unit = torch.where(a == 0, torch.ones_like(U), U / a)
    P = new * unit if window is None else torch.where(window.bool(), new * unit, des.beta * U)
    back = _prop.asm_apply(P.reshape(Z, 1, 1, H, W).contiguous(), wl, sp, des.zs, ph, pw, True, bl, adjoint=True)
    g = back.reshape(hs, H // hs, ws, W // ws).sum((1, 3))
    hc = torch.remainder(-torch.angle(g) / des.kappa - 2e-3, des.h_max)
    lut = torch.tensor(des.lut, device=U.device)
    d_all = torch.remainder(hc[..., None] - lut, des.h_max)
    d_all = torch.minimum(d_all, des.h_max - d_all)
    d, best = d_all.min(-1)
    level = lut[best]
    L = lut.numel()
    off = torch.remainder(hc - level + des.h_max / 2, des.h_max) - des.h_max / 2
    up = lut[(best + 1) % L] + (best == L - 1) * des.h_max - level
    down = level - (lut[(best - 1) % L] - (best == 0) * des.h_max)
    take = (q >= 1) | (d <= q * torch.where(off >= 0, up, down) / 2)
    return torch.where(take, level, hc), row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ifta_timing.txt"))
    ap.add_argument("--field", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ifta_timing: needs the ROCm device; nothing is measured without it")
    dev = torch.device("cuda:0")
    H = W = args.field
    hs = ws = args.cells
    lut = [(2 * math.pi / _doe.phase_scale(LAM, EPS)) * i / 4 for i in range(4)]
    gen = torch.Generator(device=dev).manual_seed(0)
    log = [f"# {torch.cuda.get_device_name(0)}; field {H} x {W} complex64, padding_scale 1 (P = {2 * H}), DOE {hs} x "
           f"{ws}, {len(lut)} levels; kernels: median (min .. max) of {args.rounds} rounds of {args.reps} calls on a ring "
           f"of inputs beyond the 256 MB last-level cache; iterations: a run of {args.iters}, per iteration",
           "# TB/s = the byte model's bytes over the time; traffic counters were not read", ""]
    T = torch.rand(H, W, device=dev, generator=gen)
    for Z in (1, 4):
        px = Z * H * W
        ring = max(2, math.ceil(600e6 / (8 * px)))
        planes = [torch.view_as_complex(torch.randn(Z, H, W, 2, device=dev, generator=gen)) for _ in range(ring)]
        scale = torch.ones(Z, dtype=torch.float64, device=dev)
        t = timed(lambda u: optics.ifta_target_stats(u, T), planes, args.reps, args.rounds)
        log.append(f"Z = {Z}  ifta_target_stats    {t[0]:8.4f} ms ({t[1]:.4f} .. {t[2]:.4f})  {12 * px / t[0] / 1e9:6.3f} TB/s")
        t = timed(lambda u: optics.ifta_target_project(u, T, scale, out=u), planes, args.reps, args.rounds)
        log.append(f"Z = {Z}  ifta_target_project  {t[0]:8.4f} ms ({t[1]:.4f} .. {t[2]:.4f})  {20 * px / t[0] / 1e9:6.3f} TB/s "
                   "(in place)")
        if Z == 1:
            backs = [torch.view_as_complex(torch.randn(H, W, 2, device=dev, generator=gen)) for _ in range(20)]
            q = torch.full((1,), 0.5, device=dev)
            t = timed(lambda u: optics.ifta_doe_project(u, (hs, ws), LAM, EPS, lut, q=q), backs, args.reps, args.rounds)
            log.append(f"       ifta_doe_project     {t[0]:8.4f} ms ({t[1]:.4f} .. {t[2]:.4f})  "
                       f"{(8 * H * W + 8 * hs * ws) / t[0] / 1e9:6.3f} TB/s (no incident field)")
        zs = [0.2 + 0.05 * k for k in range(Z)]
        asm = ASM_prop(z_distance=zs[0], padding_scale=1, bandlimit_type="exact", device=dev)
        asm.check_Zc = False
        des = ifta.IFTA(asm, zs, LAM, 1e-3, EPS, TAND, lut, (hs, ws))
        out = {}
        for name, graph in (("eager", False), ("graph replay", True)):
            t = timed(lambda _: des.run(T, iters=args.iters, graph=graph), [None], 1, args.rounds)
            out[name] = t[0] / args.iters
            log.append(f"Z = {Z}  iteration, {name:13s} {t[0] / args.iters:8.4f} ms ({t[1] / args.iters:.4f} .. "
                       f"{t[2] / args.iters:.4f})")
        st = des._state
        qs = [torch.tensor(v, device=dev) for v in ifta.default_q_schedule(args.iters)]

        def torch_run(_):
            with torch.no_grad():
                h = st["init"]
                for it in range(args.iters):
                    h, _row = torch_iteration(des, st, h, qs[it], T, None)
            return h

        t = timed(torch_run, [None], 1, args.rounds)
        log.append(f"Z = {Z}  iteration, torch ops     {t[0] / args.iters:8.4f} ms ({t[1] / args.iters:.4f} .. "
                   f"{t[2] / args.iters:.4f})  x{t[0] / args.iters / out['eager']:.2f} the eager iteration, "
                   f"x{t[0] / args.iters / out['graph replay']:.2f} the replayed one")
        print("\n".join(log[-7:]), flush=True)
        del planes
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(log) + "\n")


if __name__ == "__main__":
    main()
