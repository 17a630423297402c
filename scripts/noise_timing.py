#!/usr/bin/env python
"""Time the fused detector-noise kernel against the reference's torch op sequence on the same device
and tensors: a [3, 32, 2048, 2048] complex64 field (seeded, mean |E|^2 = 3) and its float32 intensity,
one MI355X.

Pairs, alternated --reps times after --warmup rounds, each call timed with HIP events:
  detect <kind>     : optics.detect(field, kind)      vs  field.abs() ** 2 followed by the model's ops
  add_noise <kind>  : optics.add_noise(intensity, kind) vs the model's ops (Addons/Noise.py:27, 58-61, 87-89, 112)
  poisson at a rate of 3, of 50, and on a 0 ... 200 ramp (shuffled, so every wave mixes both samplers)
for the four kinds gauss, uniform, poisson, poisson_gauss.  The torch sequence is the yardstick (the
reference's forward, op for op, on torch's generator).  Then, in a pass of its own per case, the
kernel's own HIP-event time (thz_timing_*, "noise_apply") with the byte model: detect reads 8 B and
writes 4 B per element (12 B), add_noise reads 4 B and writes 4 B (8 B); achieved TB/s and the
fraction of the 8.0 TB/s HBM3E peak.  The two sides draw different samples, so their outputs are
compared by mean and variance at the timed size.  Plain text to --out.

    python scripts/noise_timing.py --out profiles/noise_timing.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12
SIGMA, AMP, GAIN = 0.1, 0.1, 1.0


def ref_model(x, kind):
    """The reference's forward, op for op."""
    if kind == "gauss":
        return x + torch.randn_like(x) * SIGMA
    if kind == "uniform":
        return x + (torch.rand_like(x) - 0.5) * 2 * AMP
    y = torch.poisson(x / GAIN)
    if kind == "poisson":
        y *= GAIN
        return y
    y = y * GAIN
    y += torch.randn_like(x) * SIGMA
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/noise_timing.txt")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--n", type=int, default=2048)
    args = ap.parse_args()

    from quantizationawarethzdoe_amd import _lib, optics

    if not torch.cuda.is_available():
        sys.exit("noise_timing: needs a ROCm GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    C, N = args.channels, args.n
    torch.manual_seed(4100)
    field = torch.randn(3, C, N, N, dtype=torch.complex64, device=dev) * (3.0 ** 0.5)
    inten = field.abs() ** 2
    elems = field.numel()
    state = torch.tensor([4100, 0], dtype=torch.int32, device=dev)
    one = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    kinds = ("gauss", "uniform", "poisson", "poisson_gauss")
    kw = dict(sigma=SIGMA, a=AMP, gain=GAIN, normalize=True)

    def fused(fn, x, kind):
        def run():
            state.add_(one)
            return fn(x, kind, rng=(state, 0), **kw)
        return run

    cases = [(f"detect {k}", 12, fused(optics.detect, field, k), (lambda k=k: ref_model(field.abs() ** 2, k)))
             for k in kinds]
    cases += [(f"add_noise {k}", 8, fused(optics.add_noise, inten, k), (lambda k=k: ref_model(inten, k)))
              for k in kinds]

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
        f"Noise timing: [3, {C}, {N}, {N}] complex64 field, mean |E|^2 = 3 ({elems / 1e6:.1f} M elements), "
        f"sigma = {SIGMA}, a = {AMP}, gain = {GAIN}",
        f"device {torch.cuda.get_device_name(0)}, library {_lib.version()}, {args.reps} alternated reps after "
        f"{args.warmup} warm-up rounds, HIP events around each call; kernel time from the library's own events in a "
        f"separate pass",
    ]

    def run_case(name, bpe, fn, ref, x_desc=""):
        with torch.no_grad():
            for _ in range(args.warmup):
                fn()
                ref()
            torch.cuda.synchronize()
            tf, tr = [], []
            for _ in range(args.reps):
                tf.append(timed(fn))
                tr.append(timed(ref))
            a, b = fn().double(), ref().double()
            stats = (f"mean {float(a.mean()):.5f} / {float(b.mean()):.5f}, var {float(a.var()):.5f} / "
                     f"{float(b.var()):.5f} (fused / torch)")
            del a, b
            _lib.timing_enable(True)
            _lib.timing_reset()
            for _ in range(args.reps):
                fn()
            ms, n = _lib.timing_read("noise_apply")
            _lib.timing_enable(False)
        t = ms / n * 1e-3
        bw = bpe * elems / t
        lines.extend([
            f"{name}{x_desc}:",
            f"  fused call            : median {med(tf):9.3f} ms  (min {min(tf):.3f}, max {max(tf):.3f})",
            f"  torch op sequence     : median {med(tr):9.3f} ms  (min {min(tr):.3f}, max {max(tr):.3f})",
            f"  ratio torch / fused   : {med(tr) / med(tf):.2f}   slowest fused rep faster than the fastest torch rep: "
            f"{max(tf) < min(tr)}",
            f"  kernel noise_apply    : {ms / n:9.3f} ms  ({n} launches)  {bpe} B/element = {bpe * elems / 2 ** 30:.2f} GiB"
            f" -> {bw / 1e12:.3f} TB/s = {100 * bw / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak",
            f"  samples               : {stats}",
        ])
        print("\n".join(lines[-6:]), flush=True)
        torch.cuda.empty_cache()

    for name, bpe, fn, ref in cases:
        run_case(name, bpe, fn, ref)

    # the Poisson kernel by rate: inversion only, rejection only, and both in every wave
    del field
    torch.cuda.empty_cache()
    for label, fill in (("rate 3", lambda t: t.fill_(3.0)), ("rate 50", lambda t: t.fill_(50.0)),
                        ("rates 0 ... 200, shuffled", lambda t: t.uniform_(0.0, 200.0))):
        fill(inten)
        run_case("add_noise poisson", 8, fused(optics.add_noise, inten, "poisson"),
                 (lambda: ref_model(inten, "poisson")), f" at {label}")

    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
