"""Multi-process paths on CPU (gloo, world_size 2): the QAT gradient all-reduce and the
independent-plane sharding used by bench.py."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _allreduce_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from quantizationawarethzdoe_amd.qat import GradientAllReduce
        torch.manual_seed(0)
        params = [torch.nn.Parameter(torch.zeros(50, 50)), torch.nn.Parameter(torch.zeros(3, 7)),
                  torch.nn.Parameter(torch.zeros(4), requires_grad=False)]
        g = torch.Generator().manual_seed(100 + rank)  # each rank: its own noise sample
        for p in params[:2]:
            p.grad = torch.randn(p.shape, generator=g)
        local = [p.grad.clone() for p in params[:2]]
        ar = GradientAllReduce(params)
        assert ar.world == world and len(ar.params) == 2
        ar()
        gathered = [[torch.zeros_like(t) for _ in range(world)] for t in local]
        for t, out in zip(local, gathered):
            dist.all_gather(out, t)
        ok = all(torch.allclose(p.grad, torch.stack(out).mean(0), atol=1e-7)
                 for p, out in zip(params[:2], gathered))
        # a parameter without a gradient contributes zeros and receives the average
        params[1].grad = None
        ar()
        q.put((rank, ok, params[1].grad is not None))
    finally:
        dist.destroy_process_group()


def test_gradient_allreduce_gloo_world2():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_allreduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok and has for _, ok, has in res), res


def _slot_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from quantizationawarethzdoe_amd import doe
        from quantizationawarethzdoe_amd.qat import GradientAllReduce
        params = [torch.nn.Parameter(torch.zeros(5, 6)), torch.nn.Parameter(torch.zeros(7))]
        ar = GradientAllReduce(params)
        g = torch.Generator().manual_seed(10 + rank)
        vals = [torch.randn(p.shape, generator=g) for p in params]
        # what a fused backward kernel does: take the parameter's slot, write the gradient into it;
        # autograd then adopts the tensor as .grad (here: assigned)
        slot = doe.grad_slot(params[0], params[0])
        slot.copy_(vals[0])
        params[0].grad = slot
        in_bucket = ar._in_bucket(params[0], ar._offsets[0])
        # a second contribution in the same backward does not get the slot again
        second = doe.grad_slot(params[0], params[0])
        fresh = second.data_ptr() != slot.data_ptr()
        params[1].grad = vals[1].clone()  # an ordinary gradient is packed by a copy
        ar()
        out = [torch.zeros_like(v) for v in vals]
        ok = True
        for v, o, p in zip(vals, out, params):
            got = [torch.zeros_like(v) for _ in range(world)]
            dist.all_gather(got, v)
            ok &= torch.allclose(p.grad, torch.stack(got).mean(0), atol=1e-7)
        # after pack the slots are free again
        again = doe.grad_slot(params[0], torch.empty(0)) if params[0].grad is None else None
        q.put((rank, bool(in_bucket), bool(fresh), bool(ok), params[0].grad.data_ptr() == slot.data_ptr(),
               again is None))
    finally:
        dist.destroy_process_group()


def test_gradient_slots_in_the_allreduce_bucket_gloo_world2():
    """The fused DOE backward kernels write a weight's gradient straight into its slice of the
    all-reduce bucket (doe.grad_slot): pack then copies nothing for it, the average lands in the
    same tensor, a second request in one backward gets a fresh buffer, and ordinary gradients are
    still packed and unpacked by copies."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_slot_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(all(r[1:]) for r in res), res


def _agree_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import warnings
        from quantizationawarethzdoe_amd.qat import GradientAllReduce, agreed_capture
        ar = GradientAllReduce([torch.nn.Parameter(torch.zeros(4))])

        def fails_on_rank1():
            if rank == 1:
                raise RuntimeError("capture refused on this rank")
            return "graph", 1.0

        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            mixed = agreed_capture(ar, fails_on_rank1)
            both = agreed_capture(ar, lambda: ("graph", 2.0))
        q.put((rank, mixed, both))
    finally:
        dist.destroy_process_group()


def _guard_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    # rank 0's environment makes the capture safe, rank 1's does not (the variable unset)
    if rank == 0:
        os.environ["TORCH_NCCL_CUDA_EVENT_CACHE"] = "0"
    else:
        os.environ.pop("TORCH_NCCL_CUDA_EVENT_CACHE", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import warnings
        from quantizationawarethzdoe_amd.qat import GradientAllReduce, agreed_capture, collective_capture_safe
        ar = GradientAllReduce([torch.nn.Parameter(torch.zeros(4))])
        ar.capturable = True  # as on RCCL: the collective would be captured into the graph
        called = []

        def capture():
            called.append(rank)
            return "graph", 1.0

        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            res = agreed_capture(ar, capture)
        warned = any("TORCH_NCCL_CUDA_EVENT_CACHE" in str(w.message) for w in rec)
        q.put((rank, collective_capture_safe(), res, bool(called), warned))
    finally:
        dist.destroy_process_group()


def test_collective_capture_guard_falls_back_on_every_rank_gloo_world2():
    """the library itself refuses to capture the all-reduce where
    TORCH_NCCL_CUDA_EVENT_CACHE is not 0 (qat.collective_capture_safe).  The rank without the
    variable does not attempt the capture and votes for the split form, so BOTH ranks fall back
    (agreed_capture's MIN), with the variable named in the warning."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_guard_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, safe0, res0, called0, _), (r1, safe1, res1, called1, warned1) = res
    assert safe0 and not safe1
    assert res0 is None and res1 is None          # every rank takes the split form
    assert called0 and not called1                # rank 1 never attempted the capture
    assert warned1


def test_agreed_capture_falls_back_on_every_rank_gloo_world2():
    """a capture failure on ONE rank makes every rank take the split form (the
    eager MIN of a success flag after the attempt); a capture that succeeds everywhere is kept."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_agree_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [r[1] for r in res] == [None, None]
    assert [r[2] for r in res] == [("graph", 2.0), ("graph", 2.0)]


def test_donn_detector_targets_and_cpu_refusal():
    """cfg5: ten disjoint det x det detector targets; the trainer refuses a CPU model loudly."""
    from quantizationawarethzdoe_amd import donn
    t = donn.detector_targets(device=torch.device("cpu"))
    assert t.shape == (10, 1, 100, 100)
    assert all(float(t[k].sum()) == 100.0 for k in range(10))
    assert float(t.sum(0).max()) == 1.0
    model = donn.DONN(device=torch.device("cpu"))
    tr = donn.DONNTrainer(model, t)
    assert tr.allreduce.world == 1 and sum(p.numel() for p in tr.params) == 3 * 100 * 100
    with pytest.raises(RuntimeError, match="ROCm device"):
        tr.step(torch.rand(2, 1, 100, 100), torch.tensor([1, 2]))


def test_plane_sharding_covers_every_plane_once():
    from bench import shard_planes
    for n_planes in (1, 7, 64, 512):
        for world in (1, 2, 3, 8):
            seen = []
            for r in range(world):
                seen.extend(shard_planes(n_planes, r, world))
            assert sorted(seen) == list(range(n_planes))


class _FakeSystem(torch.nn.Module):
    """A CPU stand-in for FourFocalSpotsSystem: out = w * x_rank (each rank its own 'noise sample')."""

    def __init__(self, x):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(-1.0, 1.0, x.numel()).reshape(x.shape))
        self.x = x
        self.device = torch.device("cpu")

    def forward(self, frac):
        import types
        return types.SimpleNamespace(data=self.w * self.x * (1.0 + frac))


def _mse(out, tgt):
    return ((out - tgt) ** 2).mean()


def _trainer_worker(rank, world, port, q):
    """QATTrainer's eager step runs the same fwd/bwd+pack | all-reduce | unpack+Adam phases the
    HIP-graph replay is split into; after 3 steps every rank must hold the weights of one Adam
    trajectory driven by the rank-averaged gradient."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from quantizationawarethzdoe_amd.qat import QATTrainer
        xs = [torch.randn(6, 5, generator=torch.Generator().manual_seed(10 + r)) for r in range(world)]
        tgt = torch.randn(6, 5, generator=torch.Generator().manual_seed(99))
        sysm = _FakeSystem(xs[rank])
        tr = QATTrainer(sysm, tgt, lr=0.05, max_itrs=10, loss_fn=_mse)
        assert tr.allreduce.world == world
        for _ in range(3):
            tr.step()
        w = sysm.w.detach().clone()
        allw = [torch.zeros_like(w) for _ in range(world)]
        dist.all_gather(allw, w)
        # single-process replay of the same trajectory with the averaged gradient
        ref = torch.nn.Parameter(torch.linspace(-1.0, 1.0, 30).reshape(6, 5))
        opt = torch.optim.Adam([ref], lr=0.05)
        for it in range(3):
            frac = it / 10
            opt.zero_grad()
            loss = sum(_mse(ref * x * (1.0 + frac), tgt) for x in xs) / world
            loss.backward()
            opt.step()
        ok_same = all(torch.equal(a, allw[0]) for a in allw)
        ok_ref = torch.allclose(w, ref.detach(), atol=1e-6)
        q.put((rank, ok_same, ok_ref))
    finally:
        dist.destroy_process_group()


def test_trainer_phased_allreduce_gloo_world2():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_trainer_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(a and b for _, a, b in res), res


def test_bench_two_ranks_dry_run_gloo():
    """``bench.py --gpus 2`` without a launcher starts two ranks itself (torch.distributed.run child);
    the dry run rehearses the orchestration on the CPU over gloo: n_gpus 2, every plane of the
    128-plane global sweep exactly once, the cfg3 wavelengths and the cfg5 batch likewise."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-run", "--steps", "3",
                        "--warmup", "1"], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["steps"] == 3
    assert line["planes_covered"] == list(range(128))
    assert line["wavelengths_covered"] == list(range(32))
    assert line["samples_covered"] == list(range(256))
    assert line["value"] == round(2 * 64 * 3 / line["elapsed_max_s"], 2)


def test_bench_refuses_gpus_world_mismatch():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--dry-run"],
                       capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


def test_bench_dump_outputs_refuses_the_dry_run_and_zero_steps():
    """--dump-outputs writes what the GPU path computed, so the CPU rehearsal refuses it; --steps
    sets the number of timed steps, so it must be at least 1 (argparse usage errors, exit 2)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra, word in ((["--dump-outputs", "unused_dir"], "--dump-outputs"), (["--steps", "0"], "--steps")):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--dry-run"] + extra,
                           capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 2 and word in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(os.path.join(root, "unused_dir"))


def test_bench_secondary_watchdog_prints_the_line_and_exits_nonzero():
    """A secondary that hangs (e.g. in a collective) must not cost the headline line: the watchdog
    prints the line with the finished secondaries (the snapshot the main thread published) and the
    rest marked as timed out, reports a finished secondary's failed output check on stderr, and
    exits with WATCHDOG_EXIT (a hang is not a success)."""
    import json
    import subprocess
    import sys
    code = ("import json, time, bench\n"
            "line = {'metric': 'm', 'value': 1.0}\n"
            "snap = [{}]\n"
            "bench._secondary_watchdog(line, ['cfg3_czt', 'cfg4_qat'], 0, 0.5, snap)\n"
            "snap[0] = {'cfg3_czt': {'value': 2.0, 'output_check': {'ok': False, 'why': 'x'}}}\n"
            "time.sleep(60)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    import bench
    assert r.returncode == bench.WATCHDOG_EXIT != 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["value"] == 1.0 and out["secondary"]["cfg3_czt"]["value"] == 2.0
    assert "timed out" in out["secondary"]["cfg4_qat"]["error"]
    assert "output check FAILED" in r.stderr and "cfg3_czt" in r.stderr


def test_bench_failed_checks_helper():
    import bench
    sec = {"a": {"output_check": {"ok": True}}, "b": {"error": "boom"},
           "c": {"modes": {"x": {"output_check": {"ok": False}}, "y": {"output_check": {"ok": True}}}}}
    f = bench._failed_checks(sec)
    assert len(f) == 1 and f[0].startswith("c.modes.x:")
