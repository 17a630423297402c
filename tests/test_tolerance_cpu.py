"""The fabrication-tolerance Monte Carlo without a GPU: host-side validation of the two C entries (nothing touches a
device before it), the argument errors of FabricationModel / ToleranceAnalysis / optics.tolerance_modulate, the
restatement tests/tolerance_ref.py on trivial models, ToleranceReport on a made-up table, and the vetting of the
fixed seed of the statistical GPU test on the float64 restatement of the generator."""
import ctypes
import math

import numpy as np
import pytest
import torch

from quantizationawarethzdoe_amd import _lib, optics, tolerance
from tests import tolerance_ref as tr

OK, NULL = ctypes.c_void_p(4096), ctypes.c_void_p(0)  # OK is never dereferenced: validation precedes any device call
WL = _lib.float_array([1e-3])


def _desc(**kw):
    base = dict(K=3, first=0, Bf=1, C=1, H=8, W=8, hs=8, ws=8, L=4, sigma_scale=0.02, rough_kind=_lib.TOL_ROUGH_NORMAL,
                rough=1e-6, lo=0.0, hi=math.inf, epsilon=2.66, tand=0.03,
                wavelengths=ctypes.cast(WL, ctypes.POINTER(ctypes.c_float)), rng=4096, stream=0)
    levels = kw.pop("levels", (0.0, 1e-6, 1e-6, 1e-6))
    base.update(kw)
    return _lib.ToleranceDesc(sigma_level=(ctypes.c_float * _lib.THZ_MAX_LUT)(*levels), **base)


def _fwd(d, field=OK, height=OK, idx=OK, out=OK, hout=NULL):
    return _lib.lib().thz_tolerance_modulate_forward(ctypes.byref(d) if d is not None else None, field, height, idx, out,
                                                     hout, NULL)


def _bwd(d, g=OK, field=OK, height=OK, idx=OK, gf=OK, gh=OK):
    return _lib.lib().thz_tolerance_modulate_backward(ctypes.byref(d) if d is not None else None, g, field, height, idx,
                                                      gf, gh, NULL, 0, NULL)


def _refused(code, word):
    return code == _lib.THZ_E_ARG and word in _lib.lib().thz_last_error()


def test_entries_are_exported():
    assert {"thz_tolerance_modulate_forward", "thz_tolerance_modulate_backward"} <= set(_lib.EXPORTED)
    assert _lib.lib().thz_abi_version() == 9  # additive: detected by symbol


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_entry_refuses_on_the_host(call):
    assert _refused(call(None), b"null")
    for hole in ("field", "height"):
        assert _refused(call(_desc(), **{hole: NULL}), b"null"), hole
    assert _refused(call(_desc(rng=0)), b"null")
    assert _refused(call(_desc(wavelengths=None)), b"null")
    assert _refused(call(_desc(L=17)), b"L = 17")
    assert _refused(call(_desc(sigma_scale=-0.1)), b"sigma_scale")
    assert _refused(call(_desc(levels=(0.0, -1e-6, 0.0, 0.0))), b"sigma_level[1]")
    assert _refused(call(_desc(rough=-1e-6)), b"roughness")
    assert _refused(call(_desc(rough=float("nan"))), b"roughness")
    assert _refused(call(_desc(rough_kind=3)), b"roughness kind")
    assert _refused(call(_desc(lo=1.0, hi=0.5)), b"lo")
    assert _refused(call(_desc(first=-1)), b"first")
    assert _refused(call(_desc(Bf=2)), b"Bf")
    assert _refused(call(_desc(K=0)), b"shape")
    # the two limits of the generator's 32-bit index: (first + K) 16 and (first + K) hs ws
    assert _refused(call(_desc(first=2 ** 28 - 2)), b"16 > 2^32")
    assert _refused(call(_desc(first=2 ** 26 - 2)), b"hs ws")
    assert _refused(call(_desc(first=2 ** 62)), b"2^32")
    # idx may be absent only without a level term
    assert _refused(call(_desc(), idx=NULL), b"null idx")
    assert _refused(call(_desc(), idx=ctypes.c_void_p(4098)), b"aligned")
    assert _refused(call(_desc(), field=ctypes.c_void_p(4100)), b"aligned")
    assert call(_desc(C=_lib.THZ_MAX_WAVELENGTHS + 1)) == _lib.THZ_E_UNSUPPORTED


def test_forward_needs_out_and_backward_takes_optional_gradients():
    assert _refused(_fwd(_desc(), out=NULL), b"null")
    assert _refused(_bwd(_desc(), g=NULL), b"null")
    assert _bwd(_desc(), gf=NULL, gh=NULL) == _lib.THZ_OK  # nothing asked for: launches nothing
    assert _refused(_bwd(_desc(), gf=ctypes.c_void_p(4100)), b"aligned")


def test_fabrication_model_validation():
    F = tolerance.FabricationModel
    m = F(0.02, [0, 1e-6, 2e-6], ("uniform", 1e-6), (0.0, 2e-3))
    assert m.sigma_level == (0.0, 1e-6, 2e-6) and m.has_level_term and m.clamp == (0.0, 2e-3)
    assert not F().has_level_term and F().clamp == (0.0, None) and F().roughness is None
    assert F(sigma_level=3e-6).for_levels(4).sigma_level == (3e-6,) * 4
    for bad in (dict(sigma_scale=-1), dict(sigma_level=[1e-6, -1e-6]), dict(sigma_level=[0.0] * 17), dict(sigma_level=[]),
                dict(roughness=("pink", 1e-6)), dict(roughness=("normal", -1.0)), dict(roughness=1e-6),
                dict(clamp=(1.0, 0.0)), dict(clamp=0.0), dict(sigma_scale=float("nan"))):
        with pytest.raises(ValueError):
            F(**bad)
    with pytest.raises(ValueError):
        F(sigma_level=[1e-6, 1e-6]).for_levels(4)
    # what optics hands the kernel: a scalar level sigma serves every index, none means an empty table
    assert optics.tolerance.tolerance_cfg(F(sigma_level=2e-6), "t")[1] == (2e-6,) * 16
    assert optics.tolerance.tolerance_cfg(F(), "t") == (0.0, (), _lib.TOL_ROUGH_NONE, 0.0, 0.0, math.inf)


def test_tolerance_modulate_argument_errors():
    F = tolerance.FabricationModel
    x, h = torch.ones(1, 1, 4, 4, dtype=torch.complex64), torch.zeros(4, 4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        optics.tolerance_modulate(x, h, [1e-3], 2.66, 0.03, F(), 2)
    with pytest.raises(TypeError):
        optics.tolerance_modulate(None, h, [1e-3], 2.66, 0.03, F(), 2)


def test_tolerance_analysis_argument_errors():
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    F, A = tolerance.FabricationModel, tolerance.ToleranceAnalysis
    cpu = torch.device("cpu")
    field = ElectricField(torch.ones(1, 1, 4, 4, dtype=torch.complex64), wavelengths=1e-3, spacing=1e-3, device=cpu)

    class El:
        height_map, epsilon, tand = torch.zeros(4, 4), 2.66, 0.03
    prop, regions = (lambda f: f), [[2.0, 2.0, 1.0]]
    with pytest.raises(TypeError, match="FabricationModel"):
        A(El, prop, regions, 0.02, field)
    with pytest.raises(TypeError, match="ElectricField"):
        A(El, prop, regions, F(), field.data)
    with pytest.raises(TypeError, match="propagator"):
        A(El, None, regions, F(), field)
    with pytest.raises(TypeError, match="height_map"):
        A(object(), prop, regions, F(), field)
    with pytest.raises(ValueError, match="lut"):
        A(El, prop, regions, F(sigma_level=1e-6), field)
    with pytest.raises(ValueError, match="region"):
        A(El, prop, [], F(), field)
    a = A(El, prop, regions, F(0.02), field)
    with pytest.raises(ValueError):
        a.run(0)
    with pytest.raises(ValueError):
        a.run(4, chunk=0)


def test_restatement_without_errors_is_the_clamped_map():
    g = np.random.default_rng(0)
    h = g.uniform(-1e-4, 1.2e-3, (5, 7)).astype(np.float32)
    idx = g.integers(0, 5, (5, 7))
    draws = g.standard_normal((3, 16)).astype(np.float32)
    out = tr.heights(h, idx, 0.0, [0.0] * 4, None, 0.0, 1e-3, draws[:, 0], draws, g.standard_normal((3, 5, 7)))
    want = np.clip(h, np.float32(0.0), np.float32(1e-3))
    assert out.dtype == np.float32 and all(np.array_equal(out[k], want) for k in range(3))
    same = tr.heights(h, idx, 0.0, [0.0] * 4, ("uniform", 0.0), -math.inf, math.inf, draws[:, 0], draws, None)
    assert np.array_equal(same[1], h)
    ht = tr.heights_torch(torch.from_numpy(h).double(), torch.from_numpy(idx), 0.0, [0.0] * 4, None, 0.0, 1e-3,
                          torch.from_numpy(draws[:, 0]), torch.from_numpy(draws), None)
    assert np.array_equal(ht.numpy(), np.broadcast_to(np.clip(h.astype(np.float64), 0.0, 1e-3), (3, 5, 7)))


def test_restatement_terms():
    """Each term alone on draws of 1: scale, the level of the pixel (an index outside the table takes none),
    uniform and normal roughness."""
    h = np.full((1, 3), 1e-3, dtype=np.float32)
    idx = np.array([[0, 2, 4]])
    one, ones = np.ones(1, dtype=np.float32), np.ones((1, 16), dtype=np.float32)
    f = np.float32
    out = tr.heights(h, idx, 0.5, [1e-4, 2e-4, 3e-4, 4e-4], None, -math.inf, math.inf, one, ones, None)[0, 0]
    base = (f(1) + f(0.5)) * f(1e-3)
    assert out.tolist() == [base + f(1e-4), base + f(3e-4), base]
    d = np.array([[[0.0, 0.5, 0.75]]], dtype=np.float32)
    uni = tr.heights(h, None, 0.0, [], ("uniform", 1e-4), -math.inf, math.inf, one, ones, d)[0, 0]
    assert uni.tolist() == [f(1e-3) - f(1e-4), f(1e-3), f(1e-3) + f(0.5) * f(1e-4)]
    nor = tr.heights(h, None, 0.0, [], ("normal", 1e-4), -math.inf, math.inf, one, ones, d)[0, 0]
    assert nor.tolist() == [f(1e-3), f(1e-3) + f(1e-4) * f(0.5), f(1e-3) + f(1e-4) * f(0.75)]


def test_generator_restatement_known_words():
    """splitmix64 finalisation of the packed counter: state (0, 0), stream 0, index 0 is mix(golden gamma)."""
    assert int(tr.rng_bits(0, 0, 0, [0])[0]) == 0xE220A8397B1DCDAF  # the first output of splitmix64 seeded with 0
    a, b = tr.rng_bits(1, 2, 3, np.arange(8)), tr.rng_bits(1, 2, 3 ^ tr.TAG_SCALE, np.arange(8))
    assert len(set(a.tolist()) | set(b.tolist())) == 16
    u = tr.u01(1, 2, 3, np.arange(1000))
    assert u.dtype == np.float32 and 0.0 <= u.min() and u.max() < 1.0 and np.all(u * 2 ** 24 == np.floor(u * 2 ** 24))


def test_yield_fraction_is_monotone():
    g = torch.Generator().manual_seed(0)
    eff = torch.rand(200, 3, generator=g, dtype=torch.float64) * 0.3
    hi, lo = eff.amax(dim=-1), eff.amin(dim=-1)
    rep = tolerance.ToleranceReport(eff, (hi - lo) / (hi + lo), {"efficiency": eff[0], "uniformity": 0.0})
    assert rep.yield_fraction() == 1.0
    prev = 1.0
    for t in np.linspace(0.0, 0.9, 19):  # a tighter efficiency floor never admits more
        y = rep.yield_fraction(min_efficiency=float(t))
        assert y <= prev
        prev = y
    assert prev == 0.0
    prev = 1.0
    for t in np.linspace(1.0, 0.0, 21):  # nor does a tighter uniformity ceiling
        y = rep.yield_fraction(min_efficiency=0.3, max_uniformity=float(t))
        assert y <= prev
        prev = y
    total = eff.sum(dim=-1)
    assert rep.yield_fraction(min_efficiency=0.45) == float((total >= 0.45).double().mean())
    s = rep.summary()
    assert s["efficiency"]["mean"].shape == (3,) and s["uniformity"]["q50"].shape == ()
    assert bool((s["total_efficiency"]["q05"] <= s["total_efficiency"]["q50"]).item())
    assert torch.allclose(s["total_efficiency"]["mean"], total.mean())


def test_statistical_seed_is_inside_its_bounds():
    """The seed of tests/test_tolerance_gpu.py::test_statistics on the float64 restatement (the device normals
    differ from it by float32 rounding only): every check holds, with its margin printed."""
    c = tr.STAT
    K, k = c["K"], np.arange(c["K"], dtype=np.uint64)
    g = c["sigma_scale"] * tr.normal64(c["seed"], c["step"], c["stream"] ^ tr.TAG_SCALE, k)
    e = np.stack([s * tr.normal64(c["seed"], c["step"], c["stream"] ^ tr.TAG_LEVEL, 16 * k + l)
                  for l, s in enumerate(c["sigma_level"])], axis=1)
    u = tr.u01(c["seed"], c["step"], c["stream"] ^ tr.TAG_ROUGH, np.arange(K * c["pixels"]))
    r = (((u - np.float32(0.5)) * np.float32(2.0)) * np.float32(c["a"])).astype(np.float64).reshape(K, c["pixels"])
    checks = tr.stat_checks(g, e, r)
    for name, (v, b) in checks.items():
        print(f"{name:16s} value {v:.3e} bound {b:.3e} margin {v / b if b else 0.0:.2f}")
    assert not tr.stat_failures(checks)
    # the checks do reject a wrong sampler: a 10 % wider scale error, and two levels sharing their draw
    assert "g.std" in tr.stat_failures(tr.stat_checks(1.1 * g, e, r))
    shared = e.copy()
    shared[:, 1] = 2 * e[:, 0]
    assert "corr(e0,e1)" in tr.stat_failures(tr.stat_checks(g, shared, r))
