"""The unwrapping kernels (csrc/thz_unwrap.hip) against the fp64 restatement of tests/unwrap_ref.py: parity of the
direct solve and of the PCG iteration under the project's floor rule, exact integer maps, the freeze, residues and
bit determinism.  THZ_UNWRAP_PARITY_LOG collects the parity lines (profiles/unwrap_parity_ratios.txt)."""
import functools
import math

import pytest
import torch

from tests import parity
from tests import unwrap_ref as R
from tests.gpu_util import bits, dev

pytestmark = pytest.mark.gpu
LOG = "THZ_UNWRAP_PARITY_LOG"
CAPS = dict(rel_cap=1e-4, max_cap=1e-3)
SHAPES = [(64, 64), (64, 256), (128, 64)]


def _uw():
    from quantizationawarethzdoe_amd import unwrap
    return unwrap


@functools.lru_cache(maxsize=None)
def _holed():
    return R.holed_field()


# the last two cross the threshold between the runtime plan (64 .. 512 points) and the compile-time transforms, on
# the row passes and on the column pass
@pytest.mark.parametrize("shape", [(1, 64, 64), (1, 64, 256), (3, 256, 128), (1, 64, 1024), (1, 1024, 64)])
def test_direct_solve_parity(shape):
    U = R.speckle(shape)
    ref, _ = R.unwrap(U, dtype=torch.float64)
    floor = parity.floor_of(R.unwrap(U, dtype=torch.float32)[0], ref, **CAPS)
    got = _uw().unwrap_phase(U.to(dev()), anchor=None).cpu()
    parity.judge(LOG, "unwrap", "direct", "x".join(map(str, shape)), got, ref, floor)


@pytest.mark.parametrize("as_phase", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_congruent_solution_is_exact(shape, as_phase):
    """Smooth fields, congruent and anchored at the centre: the integer map equals the true phase's at every pixel and
    the values are float32(psi + 2 pi k) to 4 ulp."""
    U, s = R.smooth_field(*shape)
    psi = torch.angle(U.to(torch.complex128))
    x = psi.to(torch.float32) if as_phase else U
    psi = x.double() if as_phase else psi
    out = _uw().unwrap_phase(x.to(dev()), congruent=True, anchor="center").cpu().double()
    k_true = torch.round((s - psi) / R.TWO_PI)
    k_true = k_true - k_true[shape[0] // 2, shape[1] // 2]
    assert torch.equal(torch.round((out - psi) / R.TWO_PI), k_true)
    err = (out - (psi + R.TWO_PI * k_true).to(torch.float32).double()).abs()
    assert bool((err <= 4 * 2.0 ** -23 * out.abs()).all()), float((err / out.abs()).max())


def test_weighted_embedded_solve():
    """80 x 96 with a garbage-filled hole of weight 0: exact integer map on the weighted pixels after 20 steps, a
    history that ends below 1e-5, and the same answer after 80 steps (the freeze)."""
    U, s, w = _holed()
    H, W = s.shape
    keep = w > 0
    d = dev()
    psi = torch.angle(U.to(torch.complex128))
    out, hist = _uw().unwrap_phase(U.to(d), weights=w.to(d), iters=20, tol=1e-6, congruent=True, anchor="center",
                                   return_history=True)
    k_true = torch.round((s - psi) / R.TWO_PI)
    k_true = k_true - k_true[H // 2, W // 2]
    assert torch.equal(torch.round((out.cpu().double() - psi) / R.TWO_PI)[keep], k_true[keep])
    h = hist.cpu()[:, 0]
    print("hist", " ".join(f"{v:.2e}" for v in h.tolist()))
    low = h[h < 1e-3]
    assert float(h[-1]) < 1e-5 and bool((low[1:] <= low[:-1]).all())
    p20 = _uw().unwrap_phase(U.to(d), weights=w.to(d), iters=20, tol=1e-6).cpu()
    p80 = _uw().unwrap_phase(U.to(d), weights=w.to(d), iters=80, tol=1e-6).cpu()
    print("80 vs 20", float((p80 - p20)[keep].abs().max()))
    assert float((p80 - p20)[keep].abs().max()) <= 1e-3


@pytest.mark.parametrize("case", ["80x96 hole", "64x1024 amplitude"])
def test_pcg_iteration_parity(case):
    """Three steps against three steps of the restatement; the second case runs the compile-time row passes and the
    amplitude weights formed on the device."""
    U, w = (_holed()[0], _holed()[2]) if "hole" in case else (R.smooth_field(64, 1024)[0], "amplitude")
    ref, _ = R.unwrap(U, weights=w, iters=3, dtype=torch.float64)
    floor = parity.floor_of(R.unwrap(U, weights=w, iters=3, dtype=torch.float32)[0], ref, **CAPS)
    wd = w if isinstance(w, str) else w.to(dev())
    got = _uw().unwrap_phase(U.to(dev()), weights=wd, iters=3, anchor=None).cpu()
    parity.judge(LOG, "unwrap", "pcg", case + " iters=3", got, ref, floor)


def test_residues_of_two_vortices():
    y, x = torch.meshgrid(torch.arange(64.0), torch.arange(64.0), indexing="ij")
    U = (torch.complex(x - 20.5, y - 30.5) * torch.complex(x - 40.5, -(y - 12.5))).to(torch.complex64)
    q = _uw().residues(U.to(dev())).cpu()
    want = torch.zeros(63, 63, dtype=torch.int8)
    want[30, 20], want[12, 40] = 1, -1
    assert q.dtype == torch.int8 and torch.equal(q, want)


def test_bits_repeat_graph_and_batch():
    U, _, w = _holed()
    d = dev()
    Ud, wd = U.to(d), w.to(d)
    run = lambda: _uw().unwrap_phase(Ud, weights=wd, iters=5)
    eager = run()
    assert bits(run(), eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    for _ in range(3):
        captured.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert bits(captured, eager)
    S = R.speckle((3, 64, 128)).to(d)
    for kw in (dict(), dict(weights="amplitude", iters=4)):
        whole = _uw().unwrap_phase(S, **kw)
        assert all(bits(whole[b], _uw().unwrap_phase(S[b:b + 1], **kw)[0]) for b in range(3))
