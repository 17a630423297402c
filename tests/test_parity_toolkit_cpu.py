"""The parity and device toolkit itself (tests/parity.py, tests/gpu_util.py) on hand-made cases, no GPU."""
import math

import pytest
import torch

from tests import parity as P
from tests.gpu_util import bits

N = 64


def _pair(delta=1.0):
    """ref: N ones; got: ref with one element off by ``delta``"""
    ref = torch.ones(N, dtype=torch.complex128)
    got = ref.clone()
    got[5] += delta
    return got, ref


def test_errors_of_one_wrong_element():
    rel, mx = P.errors(*_pair(0.5))
    assert rel == pytest.approx(0.5 / math.sqrt(N), rel=1e-15) and mx == pytest.approx(0.5, rel=1e-15)
    assert P.errors(torch.ones(N, dtype=torch.complex64), torch.ones(N)) == (0.0, 0.0)


def test_floor_of_windows_and_clamp():
    caps = dict(rel_cap=2e-6, max_cap=2e-5)
    ok, ref = _pair(8e-6)    # rel 1e-6, max/rms 8e-6
    assert P.floor_of(ok, ref, **caps) == P.errors(ok, ref)
    with pytest.raises(AssertionError, match="floor32"):
        P.floor_of(ref.clone(), ref, **caps)              # an exact run is no fp32 run
    with pytest.raises(AssertionError, match="floor32"):
        P.floor_of(ref.clone(), ref, at_least_u32=True, **caps)
    with pytest.raises(AssertionError, match="floor32"):
        P.floor_of(_pair(8e-5)[0], ref, **caps)           # above both caps
    tiny, _ = _pair(1e-8)    # under one rounding on both metrics: refused, or clamped up
    with pytest.raises(AssertionError, match="floor32"):
        P.floor_of(tiny, ref, **caps)
    assert P.floor_of(tiny, ref, at_least_u32=True, **caps) == (P.U32, P.U32)
    rel, mx = P.floor_of(ok, ref, at_least_u32=True, **caps)
    assert (rel, mx) == P.errors(ok, ref)


@pytest.mark.parametrize("metric", [0, 1])
def test_judge_passes_at_3p9_and_raises_at_4p1(metric, monkeypatch, tmp_path, capsys):
    log = tmp_path / "parity.log"
    monkeypatch.setenv("THZ_TOOLKIT_TEST_LOG", str(log))
    got, ref = _pair(1e-6)
    rel, mx = P.errors(got, ref)

    def floor(ratio):   # the judged metric at ``ratio`` times its floor, the other at its floor
        return tuple(v / (ratio if k == metric else 1.0) for k, v in enumerate((rel, mx)))

    r = P.judge("THZ_TOOLKIT_TEST_LOG", "toolkit-parity", "fam", "case", got, ref, floor(3.9), widths=(6, 8))
    assert r[metric] == pytest.approx(3.9) and r[1 - metric] == pytest.approx(1.0)
    printed = capsys.readouterr().out
    assert printed == log.read_text() and printed.startswith("toolkit-parity fam    case     floor32 ")
    assert printed.rstrip("\n").endswith("ratio  3.90  1.00" if metric == 0 else "ratio  1.00  3.90")
    with pytest.raises(AssertionError, match="toolkit-parity"):
        P.judge("THZ_TOOLKIT_TEST_LOG", "toolkit-parity", "fam", "case", got, ref, floor(4.1), widths=(6, 8))
    assert len(log.read_text().splitlines()) == 2      # the failing line is logged before the assertion
    P.judge("THZ_TOOLKIT_TEST_LOG", "toolkit-parity", "fam", "case", got, ref, floor(4.1), margin=10.0)
    monkeypatch.delenv("THZ_TOOLKIT_TEST_LOG")
    P.judge("THZ_TOOLKIT_TEST_LOG", "toolkit-parity", "fam", "case", got, ref, floor(1.0))
    assert len(log.read_text().splitlines()) == 3


def test_ratios_value_grad_and_write(monkeypatch, tmp_path):
    log = tmp_path / "ratios.txt"
    monkeypatch.setenv("THZ_TOOLKIT_TEST_LOG", str(log))
    R = P.Ratios("THZ_TOOLKIT_TEST_LOG", "# header\n", widths=(10, 12, 14))
    r64 = torch.tensor([1.0, -8.0], dtype=torch.float64)

    def fn(e32):
        return {torch.float64: r64, torch.float32: (r64 + torch.tensor([e32, 0.0])).float()}.get

    # the floor decides: e32 = 0, bound = 4 x 2^-24 x 8
    floor = 4 * 2.0 ** -24 * 8.0
    R.value("v", "floor", r64 + torch.tensor([0.0, 0.5 * floor]), fn(0.0))
    assert R.worst["v"] == (pytest.approx(0.5), "floor")
    with pytest.raises(AssertionError):
        R.value("v", "floor over", r64 + torch.tensor([0.0, 1.01 * floor]), fn(0.0))
    # e32 decides: 2^-10 is exact in float32
    R.value("w", "e32", r64 + torch.tensor([3.0 * 2.0 ** -10, 0.0]), fn(2.0 ** -10))
    assert R.worst["w"] == (pytest.approx(0.75), "e32")
    # bound == 0: only an exact result passes, and it is noted as ratio 0
    zero = {torch.float64: torch.zeros(2, dtype=torch.float64), torch.float32: torch.zeros(2)}.get
    R.value("z", "zero", torch.zeros(2), zero)
    assert R.worst["z"] == (0.0, "zero")
    with pytest.raises(AssertionError):
        R.value("z", "zero off", torch.tensor([0.0, 1e-30]), zero)
    with pytest.raises(AssertionError):
        R.value("v", "shape", torch.zeros(3), fn(0.0))
    with pytest.raises(AssertionError):
        R.value("v", "nan", torch.tensor([1.0, float("nan")]), fn(0.0))
    # gradients: relative L2 against 4 max(e32, 1e-6); g64 has norm 5
    g64 = torch.tensor([3.0, 4.0], dtype=torch.float64)
    gfn = {torch.float64: g64, torch.float32: g64.float()}.get
    R.grad("v", "floor", g64 + torch.tensor([0.0, 5 * 2e-6]), gfn)
    assert R.worst["v grad"] == (pytest.approx(0.5), "floor")
    with pytest.raises(AssertionError):
        R.grad("v", "over", g64 + torch.tensor([0.0, 5 * 4.1e-6]), gfn)
    R.grad("z", "zero norm", torch.zeros(2), zero)        # exact zero passes and notes nothing
    assert "z grad" not in R.worst
    with pytest.raises(AssertionError):
        R.grad("z", "zero norm off", torch.tensor([0.0, 1e-30]), zero)
    R.note("v", "smaller", 0.25)                           # the largest ratio is kept
    assert R.worst["v"][1] == "floor over"
    R.values["a value"] = "text"
    R.write()
    lines = log.read_text().splitlines()
    assert lines[0] == "# header" and [ln.split()[0] for ln in lines[1:]] == ["v", "v", "w", "z", "a"]
    assert lines[2] == f"{'v grad':14s} {R.worst['v grad'][0]:.4f}   (over)" and lines[-1] == f"{'a value':14s} text"
    R.write()                                              # rewritten, not appended
    assert log.read_text().splitlines() == lines


def test_bits():
    z = torch.zeros(3)
    assert bits(z, z.clone()) and not bits(z, -z) and bool((z == -z).all())
    nan = torch.tensor([float("nan")])
    assert bits(nan, nan.clone())
    assert not bits(z, z.double()) and not bits(z, torch.zeros(4))
    for dtype in (torch.complex64, torch.float64, torch.complex128):
        a = torch.ones(5, dtype=dtype)
        b = a.clone()
        real = torch.view_as_real(b) if dtype.is_complex else b
        flat = real.reshape(-1)
        flat[-1] = torch.nextafter(flat[-1], flat[-1] + 1)  # one bit, in the last (imaginary) part
        assert bits(a, a.clone()) and not bits(a, b), dtype
    assert bits(torch.tensor([True, False]), torch.tensor([True, False]))
