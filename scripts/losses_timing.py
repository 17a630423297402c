"""Times the fused losses (optics.dice_loss / bce_with_logits / ssim / hierarchy_loss) against the same
losses as torch ops on the same device, forward and forward + backward, on [8, 1, 2048, 2048], and
writes profiles/losses_timing.txt.

The torch forms are tests/losses_ref.py (SSIM as the grouped-convolution sequence).  Each pair is
timed in alternated repetitions with HIP events around the call; the kernels' own times come from the
library's events in a separate pass, with the achieved fraction of the 8.0 TB/s HBM peak on each
kernel's byte model.  Peak device memory of SSIM forward + backward is read
from torch.cuda.max_memory_allocated.

    python scripts/losses_timing.py [--out profiles/losses_timing.txt] [--reps 10]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import _lib, optics  # noqa: E402
from tests import losses_ref as lr  # noqa: E402

SHAPE = (8, 1, 2048, 2048)
HBM_PEAK = 8.0e12
WS = 11


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def fwd(f, x, t):
    def run():
        with torch.no_grad():
            f(x, t)
    return run


def fwd_bwd(f, x, t):
    def run():
        xa = x.detach().requires_grad_(True)
        torch.autograd.grad(f(xa, t), xa)
    return run


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "losses_timing.txt"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    t = (torch.rand(SHAPE, device=dev, generator=g) > 0.6).float()
    x = 0.7 * t + 0.3 * torch.rand(SHAPE, device=dev, generator=g)
    n = x.numel()
    N, C, H, W = SHAPE
    pos = (H - WS + 1) * (W - WS + 1) * N * C
    tiles = -(-(H - WS + 1) // 32) * -(-(W - WS + 1) // 32) * N * C
    halo = tiles * (32 + WS - 1) ** 2  # staged pixels per plane pair, halo re-reads included
    pairs = [("dice_loss", optics.dice_loss, lr.dice), ("bce_with_logits", optics.bce_with_logits, lr.bce),
             ("ssim", optics.ssim, lr.ssim), ("hierarchy_loss", optics.hierarchy_loss, lr.hierarchy)]
    # bytes per kernel: the streaming passes 8 B per element forward, 12 B backward; the SSIM forward
    # 8 B per staged pixel (+ 12 B per position with the coefficient planes), its backward 12 B per
    # staged position + 8 B read (x, y) + 4 B written per pixel (+ 4 B read when it accumulates)
    model = {"dice_bce_sums": lambda k: 8 * n, "dice_bce_bwd": lambda k: 12 * n,
             "ssim_fwd": lambda k: 8 * halo + (12 * pos if k else 0),
             "ssim_bwd": lambda k: 12 * halo + 12 * n + (4 * n if k == 2 else 0)}
    lines = [f"Loss timing: pred, target {list(SHAPE)} float32 ({n / 1e6:.1f} M elements), SSIM window {WS} taps",
             f"device {torch.cuda.get_device_name(0)}, library {_lib.version()}, {args.reps} alternated reps after 3 "
             "warm-up rounds, HIP events around each call; kernel time from the library's own events in a separate pass"]
    ok = True
    for name, fused, ref in pairs:
        for mode, wrap in (("forward", fwd), ("forward + backward", fwd_bwd)):
            f, r = wrap(fused, x, t), wrap(ref, x, t)
            for _ in range(3):
                f(), r()
            tf, tr = [], []
            for _ in range(args.reps):
                tf.append(timed(f))
                tr.append(timed(r))
            mf, mr = statistics.median(tf), statistics.median(tr)
            ok = ok and mf <= mr
            lines += [f"{name} {mode}:",
                      f"  fused call            : median {mf:9.3f} ms  (min {min(tf):.3f}, max {max(tf):.3f})",
                      f"  torch op sequence     : median {mr:9.3f} ms  (min {min(tr):.3f}, max {max(tr):.3f})",
                      f"  ratio torch / fused   : {mr / mf:.2f}   slowest fused rep faster than the fastest torch rep: "
                      f"{max(tf) < min(tr)}"]
            _lib.timing_enable(True)
            _lib.timing_reset()
            for _ in range(args.reps):
                f()
            torch.cuda.synchronize()
            for k in ("dice_bce_sums", "dice_bce_finish", "dice_bce_bwd", "ssim_fwd", "ssim_finish", "ssim_bwd"):
                ms, cnt = _lib.timing_read(k)
                if not cnt:
                    continue
                line = f"  kernel {k:15s}: {ms / cnt:9.3f} ms  ({cnt} launches)"
                if k in model:
                    kind = (2 if name == "hierarchy_loss" else 1) if mode != "forward" else 0
                    nbytes = model[k](kind)
                    tbs = nbytes / (ms / cnt * 1e-3) / 1e12
                    line += (f"  {nbytes / 2 ** 30:.2f} GiB -> {tbs:.3f} TB/s = {100 * tbs * 1e12 / HBM_PEAK:.1f} % "
                             "of the 8.0 TB/s HBM peak")
                lines.append(line)
            _lib.timing_enable(False)
    pf, pr = peak_bytes(fwd_bwd(optics.ssim, x, t)), peak_bytes(fwd_bwd(lr.ssim, x, t))
    ok = ok and pf < pr
    lines += ["ssim forward + backward, torch.cuda.max_memory_allocated above the inputs:",
              f"  fused                 : {pf / 2 ** 20:9.1f} MiB   ({pf / (4 * n):.2f} planes of the input's size)",
              f"  torch op sequence     : {pr / 2 ** 20:9.1f} MiB   ({pr / (4 * n):.2f} planes)",
              f"every fused loss no slower than its torch sequence, SSIM peak memory below: {ok}"]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
