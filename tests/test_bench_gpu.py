"""bench.py as a program on the GPU: a plain run prints the headline line alone, and
``--dump-outputs`` writes the seeded sample of the planes its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """``bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR``: exit 0, one JSON line with the
    headline fields, 2 timed steps, and none of what --full adds (output checks, secondaries, CPU
    baseline).  DIR/cfg2_planes.npy is float32 [64, DUMP_POINTS, 2] within 64 MB and equals, bit
    for bit, the planes of the same 64-plane asm_apply call made here at bench.dump_pixels(): the
    forward pass is deterministic (no atomics, a fixed reduction order), so the same kernels on the
    same input leave no rounding to allow for, and a dump of another buffer, of other pixels or of
    a step that had not finished differs.  This checks that the file is what the timed path
    computed; tests/test_asm_gpu.py checks those values against the oracle and the reference."""
    import bench
    from quantizationawarethzdoe_amd.propagation import asm_apply
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "propagations/s" and line["higher_is_better"] is True
    assert line["dtype"] == "complex64 (fp32)" and line["steps"] == 2 and line["warmup"] == 1
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 64 / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    assert line["kernels"]["asm_cols"]["launches"] == 2  # the timers saw exactly the timed steps
    assert line["output_check"] is None and "secondary" not in line and "cpu_baseline" not in line

    assert os.listdir(tmp_path) == ["cfg2_planes.npy"]
    got = np.load(tmp_path / "cfg2_planes.npy")
    assert got.dtype == np.float32 and got.shape == (64, bench.DUMP_POINTS, 2) and got.nbytes <= 64e6

    dev = torch.device("cuda:0")
    x = bench.gaussian(bench.N_FIELD, bench.DX, bench.WAIST, dev)
    lam = [float(torch.tensor(bench.C0 / bench.FREQ, dtype=torch.float32))]
    sp = [float(torch.tensor(bench.DX, dtype=torch.float32))] * 2
    pad = bench.N_FIELD // 2
    out = asm_apply(x, lam, sp, bench.z_planes(0, 1), pad, pad, True, 1)
    idx = bench.dump_pixels()
    assert idx.unique().numel() == bench.DUMP_POINTS and 0 <= int(idx.min()) and int(idx.max()) < bench.N_FIELD ** 2
    ref = torch.view_as_real(out.reshape(64, -1)[:, idx.to(dev)]).cpu().numpy()
    del out
    assert np.abs(ref).max() > 0
    differ = [k for k in range(64) if not np.array_equal(got[k], ref[k])]
    assert not differ, differ
