#!/usr/bin/env python
"""Time the unwrapping kernels (unwrap.unwrap_phase, unwrap.residues) on the current GPU and write
profiles/unwrap_timing.txt.

  shapes     [1, 1, 1024, 1024] and [1, 8, 2048, 2048] band-limited speckle
  calls      the direct solve, a 20-iteration amplitude-weighted solve (tol = 0: no step is frozen), residues
  opponent   the same algorithm in torch ops on the same card: wrapped differences from the field, the cosine
             transforms by the FFT of the mirrored 2N extension, PCG with its scalars kept on the device
  memory     peak allocation above the input

HIP events around each whole call, every shape warmed up, the two contenders alternated round by round; medians and
the spread (min .. max).  The TB/s figure is a byte model over the event time of the whole call, not a measurement:
per plane element, the direct solve reads the field with its four neighbours from cache (8 B counted once), moves the
coefficient plane six times (write, column read + write, row read + write, closing read: 24 B) and writes the
result (4 B); a PCG step adds the planes its five kernels touch (r, Qp, phi, p read and r, phi written: 24 B; the
solve: 20 B; z, p_old read and p, Qp written, w read: 20 B).  No traffic counter is read.
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import unwrap  # noqa: E402


def dct(x, dim):
    x = x.movedim(dim, -1)
    N = x.shape[-1]
    Y = torch.fft.fft(torch.cat([x, x.flip(-1)], -1), dim=-1)[..., :N]
    ph = torch.polar(torch.ones(N, device=x.device), -math.pi * torch.arange(N, device=x.device) / (2 * N))
    return ((Y * ph).real / 2).movedim(-1, dim)


def idct(X, dim):
    X = X.movedim(dim, -1)
    N = X.shape[-1]
    ph = torch.polar(torch.full((N,), 2.0, device=X.device), math.pi * torch.arange(N, device=X.device) / (2 * N))
    Y = torch.cat([X * ph, torch.zeros_like(X[..., :1], dtype=torch.complex64)], -1)
    return torch.fft.irfft(Y, n=2 * N, dim=-1)[..., :N].movedim(-1, dim)


def torch_unwrap(U, weights=None, iters=0):
    """the model of include/thzdoe.h in torch ops (power-of-two planes), anchor None, not congruent"""
    H, W = U.shape[-2:]
    dx = torch.angle(U[..., :, 1:] * U[..., :, :-1].conj())
    dy = torch.angle(U[..., 1:, :] * U[..., :-1, :].conj())
    if weights is None:
        wx = wy = None
    else:
        a = U.abs()
        w = a / a.amax((-2, -1), keepdim=True)
        wx, wy = torch.minimum(w[..., :, :-1], w[..., :, 1:]), torch.minimum(w[..., :-1, :], w[..., 1:, :])
        dx, dy = wx * dx, wy * dy

    def div(ex, ey):
        q = torch.zeros(U.shape, dtype=torch.float32, device=U.device)
        q[..., :, :-1] += ex
        q[..., :, 1:] -= ex
        q[..., :-1, :] += ey
        q[..., 1:, :] -= ey
        return q
    s = lambda n: (4 * torch.sin(math.pi * torch.arange(n, dtype=torch.float64) / (2 * n)) ** 2).float().to(U.device)
    lam = -(s(H)[:, None] + s(W)[None, :])
    lam[0, 0] = 1

    def pinv(r):
        c = dct(dct(r, -1), -2) / lam
        c[..., 0, 0] = 0
        return idct(idct(c, -2), -1)
    rho = div(dx, dy)
    if iters == 0:
        return pinv(rho)
    dot = lambda a, b: -(a.double() * b.double()).sum((-2, -1), keepdim=True)
    phi, r, p, rz_old = torch.zeros_like(rho), rho, torch.zeros_like(rho), None
    for k in range(iters):
        z = pinv(r)
        rz = dot(r, z)
        p = z if k == 0 else z + (rz / rz_old).float() * p
        qp = div(wx * (p[..., :, 1:] - p[..., :, :-1]), wy * (p[..., 1:, :] - p[..., :-1, :]))
        alpha = (rz / dot(p, qp)).float()
        phi, r, rz_old = phi + alpha * p, r - alpha * qp, rz
    return phi


def torch_residues(U):
    dx = torch.angle(U[..., :, 1:] * U[..., :, :-1].conj())
    dy = torch.angle(U[..., 1:, :] * U[..., :-1, :].conj())
    return torch.round((dx[..., :-1, :] + dy[..., :, 1:] - dx[..., 1:, :] - dy[..., :, :-1]) / (2 * math.pi)).to(torch.int8)


def rounds(fns, n):
    for f in fns:
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms, peak = [[] for _ in fns], [0 for _ in fns]
    for _ in range(n):
        for i, f in enumerate(fns):
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = f()
            b.record()
            b.synchronize()
            del out
            ms[i].append(a.elapsed_time(b))
            peak[i] = max(peak[i], torch.cuda.max_memory_allocated() - base)
    return ms, peak


def fmt(v):
    return f"{statistics.median(v):9.3f} ms ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unwrap_timing.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"unwrap kernels on {torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min .. max); hand = the "
             "kernels, torch = the same algorithm in torch ops (mirrored-FFT DCT, device-side PCG scalars); peak = "
             "allocation above the input; TB/s = the byte model of the script's head over the event time (no counter read)"]
    for shape in [(1, 1, 1024, 1024), (1, 8, 2048, 2048)]:
        g = torch.Generator(device=dev).manual_seed(3)
        n = torch.randn(*shape, dtype=torch.complex64, device=dev, generator=g)
        fy, fx = torch.fft.fftfreq(shape[-2], device=dev), torch.fft.fftfreq(shape[-1], device=dev)
        U = torch.fft.ifft2(torch.fft.fft2(n) * torch.exp(-(fy[:, None] ** 2 + fx[None, :] ** 2) / (2 * 0.08 ** 2)))
        px = U.numel()
        cases = [
            ("direct", lambda: unwrap.unwrap_phase(U, anchor=None), lambda: torch_unwrap(U), 36 * px),
            ("pcg 20", lambda: unwrap.unwrap_phase(U, weights="amplitude", iters=20, tol=0.0, anchor=None),
             lambda: torch_unwrap(U, "amplitude", 20), (16 + 20 * 64) * px),
            ("residues", lambda: unwrap.residues(U), lambda: torch_residues(U), 9 * px),
        ]
        lines.append(f"--- {list(shape)}")
        for name, hand, ref, nbytes in cases:
            a, b = hand().float(), ref().float()
            diff = float((a - b).norm() / b.norm().clamp_min(1e-30))
            ms, peak = rounds([hand, ref], args.rounds)
            h, t = statistics.median(ms[0]), statistics.median(ms[1])
            lines.append(f"{name:9s}: hand {fmt(ms[0])} peak {peak[0] / 2 ** 20:8.1f} MiB   torch {fmt(ms[1])} peak "
                         f"{peak[1] / 2 ** 20:8.1f} MiB   torch / hand {t / h:6.2f}{'  (hand LOSES)' if t < h else ''}   "
                         f"model {nbytes / h / 1e9:6.3f} TB/s   rel diff {diff:.1e}")
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
