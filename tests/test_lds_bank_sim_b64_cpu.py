"""The two-line (row pair) exchange image under the 8-byte LDS rules (scripts/lds_bank_sim.py): every
exchange of every power-of-two size the pair kernel is instantiated for costs no bank-conflict cycle,
on the store pattern (ds_write_b64: four groups of 16 contiguous lanes over 32 dword banks) and on the
load pattern (ds_read_b64: two groups of 32 lanes over 64 dword banks); the per-r address offsets do
not depend on the thread, and the layout fits the image.  pair_lay there mirrors csrc/thz_fft.hpp.
"""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    spec = importlib.util.spec_from_file_location("lds_bank_sim", os.path.join(ROOT, "scripts", "lds_bank_sim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_b64_rules_on_known_patterns(sim):
    """The rules themselves, on patterns whose cost is known by hand."""
    lanes = np.arange(64)
    assert sim.cyc_b64_write(lanes) == 4 and sim.cyc_b64_read(lanes) == 2      # consecutive float2
    assert sim.cyc_b64_write(16 * lanes) == 4 * 16                              # one bank pair for all
    assert sim.cyc_b64_read(32 * lanes) == 2 * 32
    assert sim.cyc_b64_write(0 * lanes) == 4 and sim.cyc_b64_read(0 * lanes) == 2  # broadcast
    # distinct mod 32 in a 32-lane group, yet 2-way in each 16-lane group: the case the b32 search misses
    p = 16 * lanes + (lanes >> 1)
    assert sim.cyc_b64_read(np.concatenate([np.arange(32), np.arange(32)])) == 2
    assert len(set(int(v) % 32 for v in p[:32])) == 32 and sim.cyc_b64_write(p) == 8


@pytest.mark.parametrize("n", [1024, 2048, 4096, 8192, 16384])
def test_pair_image_has_no_conflict_cycles(sim, n):
    rows = sim.pair_exchange_table(n)
    assert [r["L"] for r in rows] == [1, 16, 256][:len(rows)] and len(rows) == (3 if n >= 8192 else 2)
    for r in rows:
        assert r["st_cyc"] == r["st_ideal"] > 0, r
        assert r["ld_cyc"] == r["ld_ideal"] > 0, r
        assert r["const_offsets"], r
        assert r["footprint"] <= sim.pair_image_f2(n), r


def test_one_float_layout_conflicts_under_the_store_rule(sim):
    """What the search was for: split_lay<1>, free of conflicts for 4-byte accesses, is 2-way on ds_write_b64."""
    first = sim.pair_exchange_table(8192, sim.split_lay)[0]
    assert first["L"] == 1 and first["st_cyc"] == 2 * first["st_ideal"] and first["ld_cyc"] == first["ld_ideal"]
