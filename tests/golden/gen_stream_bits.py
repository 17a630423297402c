"""Fixture of tests/test_stream_bits_gpu.py: the bits the streaming add-on kernels produced BEFORE they moved
onto the shared toolkit (csrc/thz_stream.hpp), so that the refactor -- and any later change to the toolkit --
is held to them.

Run once on an MI355X with a library built from the commit whose bits are to be pinned:

    THZDOE_LIB=/path/to/parent/libthzdoe.so python tests/golden/gen_stream_bits.py

Writes tests/golden/stream_bits.npz: one entry "<case>/<output>" per output of every case of
tests/stream_bits_cases.py, as the integer view of its bits (int32 for float32 and complex64, int64 for
float64), and "__lib__", the library path it ran.  Only outputs are stored; the test regenerates the inputs
from the cases' seeds.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from quantizationawarethzdoe_amd import _lib  # noqa: E402
from tests import stream_bits_cases as sb  # noqa: E402


def main():
    out = {"__lib__": np.array(os.path.basename(_lib.LIB_PATH))}
    for name in sb.CASES:
        for k, v in sb.run_case(name).items():
            out[f"{name}/{k}"] = v.numpy()
    for a, b in sb.PAIRS:
        same = all(np.array_equal(out[k], out[b + k[len(a):]]) for k in out if k.startswith(a + "/"))
        print(f"{a} == {b}: {same}")
    path = os.path.join(HERE, "stream_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out) - 1} arrays, {os.path.getsize(path)} bytes, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
