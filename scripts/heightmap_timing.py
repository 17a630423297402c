"""Times the height-map entries (optics.lut_quantize forward and its surrogate backwards, center_difference,
total_variation forward and backward) against the reference's torch op sequence on the same device, on
a [8, 1, 2048, 2048] float32 map, and writes profiles/heightmap_timing.txt.

Each call is bracketed by HIP events: 5 warm-ups, then the median of 20 runs, fused and torch
alternated.  The torch forms are the op sequences the float64 path of the same functions runs
(optics.heightmap.lut_forward_torch / lut_slope_torch / center_difference_torch), here in float32.  The
argmin snap runs with the notebooks' 10-level table on both sides; the bucketize forms with its nine
midpoints and the reference's modulo.  Every call takes the next of three input maps (403 MB in all,
more than the 256 MB last-level cache), so no call finds its input resident from the call before;
what a call writes may still be absorbed by that cache, so the TB/s figures are an effective
bandwidth on the byte model, not counted HBM traffic.  One case runs the snap on a view one float past
16-byte alignment (a contiguous slice like x[1:]), which takes the element-width form of the kernel.
The kernels' own times come from the library's events in a separate pass, with the effective TB/s on
each kernel's byte model set against the 8.0 TB/s HBM peak.  Peak device memory
above the inputs is read from torch.cuda.max_memory_allocated.

    python scripts/heightmap_timing.py [--out profiles/heightmap_timing.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import _lib, optics  # noqa: E402

SHAPE = (8, 1, 2048, 2048)
HBM_PEAK = 8.0e12
WARMUP, RUNS = 5, 20
LUT = tuple(torch.tensor([float(v) for v in (torch.arange(0, 10) * (1e-3 / 10))], dtype=torch.float32).tolist())
MID = optics.heightmap.lut_mid(LUT, torch.float32)
S = 2.5
# bytes per element of each kernel
MODEL = {"lut_quantize_fwd": 12, "lut_quantize_bwd": 16, "tv_fwd": 4, "center_difference": 12, "tv_bwd": 8,
         "center_difference_bwd": 12}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def torch_quantize(x, mode, kind):
    """The reference's sequence as one autograd function would run it: forward, then grad_out * slope."""
    wrap = mode == _lib.LUTQ_BUCKETIZE
    q, idx = optics.heightmap.lut_forward_torch(x, LUT, MID, mode, wrap)
    if kind is None:
        return q
    g = torch.ones_like(x)
    return g if kind == _lib.LUTQ_GRAD_IDENTITY else g * optics.heightmap.lut_slope_torch(x, idx, LUT, kind, S)


def torch_tv(x):
    dx, dy = optics.heightmap.center_difference_torch(x.reshape(-1, *x.shape[-2:]))
    return dx.abs().mean() + dy.abs().mean()


class Rotation:
    """The next of several equal maps on every call."""

    def __init__(self, maps):
        self.maps, self.i = maps, 0

    def __call__(self):
        self.i = (self.i + 1) % len(self.maps)
        return self.maps[self.i]


def cases(nxt, nxt_off, up):
    s = torch.tensor(S, device=up.device)

    def fused_q(mode, surrogate):
        def run():
            x = nxt()
            if surrogate is None:
                optics.lut_quantize(x, LUT, mode=mode, wrap=mode == "bucketize", midvals=MID if mode == "bucketize" else None,
                                    surrogate=None)
            else:
                xa = x.detach().requires_grad_(True)
                q, _ = optics.lut_quantize(xa, LUT, wrap=True, midvals=MID, surrogate=surrogate, s=s)
                torch.autograd.grad(q, xa, up)
        return run

    def torch_q(mode, kind):
        def run():
            with torch.no_grad():
                torch_quantize(nxt(), mode, kind)
        return run

    def fused_tv_fb():
        xa = nxt().detach().requires_grad_(True)
        torch.autograd.grad(optics.total_variation(xa), xa)

    def torch_tv_fb():
        xa = nxt().detach().requires_grad_(True)
        torch.autograd.grad(torch_tv(xa), xa)

    def nograd(f, source=nxt):
        def run():
            with torch.no_grad():
                f(source())
        return run

    def snap(t):
        return optics.lut_quantize(t, LUT, mode="argmin", surrogate=None)

    return [
        ("lut_quantize argmin snap, 10 levels (forward)", fused_q("argmin", None), torch_q(_lib.LUTQ_ARGMIN, None)),
        ("lut_quantize argmin snap on a view one float past alignment (element-width form)", nograd(snap, nxt_off),
         nograd(lambda t: torch_quantize(t, _lib.LUTQ_ARGMIN, None), nxt_off)),
        ("lut_quantize bucketize + modulo, 10 levels (forward)", fused_q("bucketize", None),
         torch_q(_lib.LUTQ_BUCKETIZE, None)),
        ("nns_poly forward + backward, s = 2.5", fused_q("bucketize", "poly"), torch_q(_lib.LUTQ_BUCKETIZE, _lib.LUTQ_GRAD_POLY)),
        ("nns_sigmoid forward + backward, s = 2.5", fused_q("bucketize", "sigmoid"),
         torch_q(_lib.LUTQ_BUCKETIZE, _lib.LUTQ_GRAD_SIGMOID)),
        ("center_difference (forward)", nograd(optics.center_difference),
         nograd(lambda t: optics.heightmap.center_difference_torch(t.reshape(-1, *t.shape[-2:])))),
        ("total_variation (forward)", nograd(optics.total_variation), nograd(torch_tv)),
        ("total_variation forward + backward", fused_tv_fb, torch_tv_fb),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heightmap_timing.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2] * SHAPE[3]
    flat = [torch.rand(n + 4, device=dev, generator=g) * 1.2e-3 - 0.1e-3 for _ in range(3)]
    nxt = Rotation([f[:n].view(SHAPE) for f in flat])
    nxt_off = Rotation([f[1:n + 1].view(SHAPE) for f in flat])
    assert all(m.data_ptr() % 16 == 0 for m in nxt.maps) and all(m.data_ptr() % 16 == 4 for m in nxt_off.maps)
    up = torch.randn(SHAPE, device=dev, generator=g)
    lines = [f"Height-map timing: {list(SHAPE)} float32 ({n / 1e6:.1f} M elements), 10-level table",
             f"device {torch.cuda.get_device_name(0)}, library {_lib.version()}, {WARMUP} warm-ups, median of {RUNS} "
             "alternated runs, HIP events around each call; kernel time from the library's own events in a separate pass",
             f"inputs rotate over three maps ({3 * 4 * n / 1e6:.0f} MB, above the 256 MB last-level cache); outputs may still "
             "be absorbed by that cache, so TB/s is an effective figure on the byte model, not counted HBM traffic"]
    ok = True
    for name, fused, ref in cases(nxt, nxt_off, up):
        for _ in range(WARMUP):
            fused(), ref()
        tf, tr = [], []
        for _ in range(RUNS):
            tf.append(timed(fused))
            tr.append(timed(ref))
        mf, mr = statistics.median(tf), statistics.median(tr)
        pf, pr = peak_bytes(fused), peak_bytes(ref)
        ok = ok and mf <= mr
        lines += [f"{name}:",
                  f"  fused call            : median {mf:9.3f} ms  (min {min(tf):.3f}, max {max(tf):.3f})   peak memory "
                  f"{pf / 2 ** 20:8.1f} MiB ({pf / (4 * n):.2f} maps)",
                  f"  torch op sequence     : median {mr:9.3f} ms  (min {min(tr):.3f}, max {max(tr):.3f})   peak memory "
                  f"{pr / 2 ** 20:8.1f} MiB ({pr / (4 * n):.2f} maps)",
                  f"  ratio torch / fused   : {mr / mf:.2f}"]
        _lib.timing_enable(True)
        _lib.timing_reset()
        for _ in range(RUNS):
            fused()
        torch.cuda.synchronize()
        for k in ("lut_quantize_fwd", "lut_quantize_bwd", "center_difference", "tv_fwd", "tv_finish", "tv_bwd"):
            ms, cnt = _lib.timing_read(k)
            if not cnt:
                continue
            line = f"  kernel {k:18s}: {ms / cnt:9.3f} ms  ({cnt} launches)"
            if k in MODEL:
                tbs = MODEL[k] * n / (ms / cnt * 1e-3) / 1e12
                line += (f"  {MODEL[k]} B per element -> effective {tbs:.3f} TB/s = {100 * tbs * 1e12 / HBM_PEAK:.1f} % of "
                         "the 8.0 TB/s HBM peak")
            lines.append(line)
        _lib.timing_enable(False)
    lines.append(f"every fused call no slower than its torch sequence: {ok}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
