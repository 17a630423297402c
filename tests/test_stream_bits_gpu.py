"""The streaming add-on kernels give the bits they gave before they moved onto the shared toolkit
(csrc/thz_stream.hpp): every output of every case of tests/stream_bits_cases.py against
tests/golden/stream_bits.npz, which tests/golden/gen_stream_bits.py wrote with a library built from the commit
before the move, and the element-width form of every kernel against its 16-byte form.

The toolkit's contract is an order of operations ("The streaming toolkit"): per field, the xor
butterfly 32 .. 1 inside a wave, the waves in index order, a finish thread's slots in ascending stride order.
Nothing is compared within a tolerance: torch.equal on the integer views.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import stream_bits_cases as sb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_bits.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files if k != "__lib__"}


@functools.lru_cache(maxsize=None)
def _run(name):
    return sb.run_case(name)


def test_fixture_covers_the_cases():
    want = {k.split("/")[0] for k in _golden()}
    assert want == set(sb.CASES)


@pytest.mark.parametrize("name", list(sb.CASES))
def test_bits_match_the_parent(name):
    got = _run(name)
    want = {k.split("/", 1)[1]: v for k, v in _golden().items() if k.startswith(name + "/")}
    assert set(got) == set(want)
    for k, v in got.items():
        w = torch.from_numpy(want[k])
        assert v.dtype == w.dtype and v.shape == w.shape, (name, k, v.dtype, w.dtype, v.shape, w.shape)
        assert torch.equal(v, w), f"{name}/{k}: {int((v != w).sum())} of {v.numel()} values differ"


@pytest.mark.parametrize("aligned, twin", sb.PAIRS)
def test_element_width_form_matches_the_16_byte_form(aligned, twin):
    a, b = _run(aligned), _run(twin)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{twin}/{k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} values differ"
