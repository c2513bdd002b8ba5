"""-m gpu: the HIP path with MORE THAN ONE RANK. The GPU boxes this repo is developed on have one device and RCCL refuses
two ranks on one device, so the ranks SHARE cuda:0 and talk over gloo -- the whole control flow of the view-sharded path
(replicated parameters, every rank renders its views of the step through the HIP rasterizer into
its GradArena, one GradExchange per step, identical replicas afterwards) runs for real; only the wire is not xGMI.
The reference sums the C_batch_size = 4 views of a step in one process (training/object_trainer.py:302-382): the
exchanged arena must equal that single-process sum."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.util import rel_scale

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, K, D, RES, NV = 20_000, 16, 3, 256, 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _scene(dev):
    from dreamscene_amd import synth
    g = synth.g_object(P, seed=3, K=K)
    cams = synth.object_cameras(NV, RES, RES)
    params = {k: torch.tensor(v, device=dev) for k, v in g.items()}
    ups = [tuple(torch.tensor(x, device=dev) for x in synth.upstream_grads(RES, RES, i)) for i in range(NV)]
    return params, cams, ups


def _render_into_arena(params, cams, ups, which, arena, dev):
    """fwd+bwd of the views `which` through ONE GaussianRasterizerViews call; their summed gradients land in the arena."""
    from dreamscene_amd.rasterizer import RasterContext
    from dreamscene_amd.views import GaussianRasterizerViews
    from tests.util import settings_for
    sl = [settings_for(cams[i], np.ones(3, np.float32), D, dev) for i in which]
    rast = GaussianRasterizerViews(sl, context=RasterContext(grad_arena=arena))
    m2d = torch.zeros((len(which), P, 3), device=dev, requires_grad=True)
    pr = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    outs = rast(means3D=pr["means3D"], means2D=m2d, opacities=pr["opacities"], shs=pr["shs"], scales=pr["scales"],
                rotations=pr["rotations"])
    ts, gs = [], []
    for (img, _, da), i in zip(outs, which):
        ts += [img, da]
        gs += [ups[i][0], ups[i][1]]
    (g2d,) = torch.autograd.grad(ts, [m2d], gs)
    torch.cuda.synchronize(dev)
    return outs, g2d


def _worker(rank, world, port, mode, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from dreamscene_amd import _lib, multiview
    _lib.load()
    params, cams, ups = _scene(dev)
    arena = multiview.GradArena(P, K, dev)
    lazy = mode.endswith("_lazy_async")    # the device forms without any host read, on the exchange's own stream
    ex = multiview.GradExchange(arena, sh_degree=D, mode=mode.replace("_lazy_async", ""), strict=not lazy)
    mine = multiview.shard_views(NV, rank, world)
    for step in range(3 if lazy else 2):   # (the second one runs the batched launches; lazy sparse_rs learns two capacities)
        outs, g2d = _render_into_arena(params, cams, ups, mine, arena, dev)
        own = arena.flat.clone()
        if step > 0:
            # the arena went through an exchange: K8 may only skip the rows the union bitmap does not name (GsrGrads.zero_outside
            # behind the message forms), and must have cleared everything after the others -- same bits as into a fresh arena
            fresh = multiview.GradArena(P, K, dev)
            fresh.flat.fill_(3.0)
            _render_into_arena(params, cams, ups, mine, fresh, dev)
            assert torch.equal(own, fresh.flat), f"step {step}: this rank's gradients differ from a backward into a fresh arena"
        if lazy:
            # the statistics all-reduce on the caller's stream beside the exchange on its own (multiview.reduce_step)
            radii = outs[-1][1]
            norm, vis, maxr = multiview.reduce_step(ex, g2d[-1], radii)
            ref_norm, ref_vis, ref_maxr = multiview.reduce_view_stats(g2d[-1], radii)
            assert torch.equal(norm, ref_norm) and torch.equal(vis, ref_vis) and torch.equal(maxr, ref_maxr)
            fitted = ex.finish()
            # (the first step may find the speculated capacity -- P / 4 rows -- too small for this small, dense scene: that step's
            #  arena then stays un-reduced, BY CONTRACT of strict=False, and the capacity follows the largest count seen)
            assert fitted or step < (1 if mode.startswith("rows") else 2), "a message overflowed after the capacities had been learnt"
            assert ex.last.get("device") and ex.last.get("host_reads") == 0, ex.last
        else:
            ex.reduce()
        torch.cuda.synchronize(dev)
        if arena.zero_outside_ok():       # (the message forms leave the union bitmap: the invariant must hold for the SUM as well)
            assert arena.verify_zero_outside(), f"step {step}: rows outside the union bitmap are not zero after the exchange"
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), flat=arena.flat.cpu().numpy(), own=own.cpu().numpy(),
             img0=outs[0][0].detach().cpu().numpy(), last=json.dumps(ex.last))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["dense", "rows", "rows_lazy_async", "direct", "sparse_rs", "sparse_rs_lazy_async", "auto"])
def test_two_ranks_share_the_gpu(built_lib, tmp_path, mode):
    """Every wire format of GradExchange with the arena ON THE DEVICE (round 5: `direct` and `sparse_rs` too -- their device
    halves, searchsorted / index_add_ / the strided packs on GPU tensors, ran on CPU tensors only until now; the collectives
    themselves are staged through the host under gloo)."""
    from dreamscene_amd import multiview
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), mode, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert np.array_equal(r0["flat"], r1["flat"]), "the replicas disagree after the exchange"
    assert not np.array_equal(r0["own"], r1["own"]), "the ranks rendered the same views"
    # the single-process sum over the same four views (what the reference's trainer accumulates)
    dev = torch.device("cuda", 0)
    params, cams, ups = _scene(dev)
    arena = multiview.GradArena(P, K, dev)
    for _ in range(2):
        outs, _ = _render_into_arena(params, cams, ups, list(range(NV)), arena, dev)
    ref = arena.flat.cpu().numpy().astype(np.float64)
    scale = rel_scale(ref)
    assert np.abs(ref).max() > 0
    e = float(np.abs(r0["flat"].astype(np.float64) - ref).max())
    assert e <= 1e-5 * scale, f"exchanged sum differs from the single-process 4-view sum by {e:.3e} (scale {scale:.3e})"
    # per-view outputs do not depend on how the views are grouped into calls: rank 0's first view is view 0
    assert np.array_equal(r0["img0"], outs[0][0].detach().cpu().numpy()), "view 0 rendered differently in the sharded run"
    fmt = json.loads(str(r0["last"]))["format"]
    assert fmt in ("sparse_rs", "dense") if mode == "auto" else fmt == mode.replace("_lazy_async", "")


def test_bench_two_ranks_one_gpu(built_lib, tmp_path):
    """bench.py's own N > 1 path (init, view sharding, exchange every step, barrier-bracketed timing, max over ranks,
    one JSON line from rank 0), two ranks on the one GPU over gloo."""
    env = dict(os.environ, GSR_BENCH_BACKEND="gloo", GSR_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4",
           "--warmup", "2", "--gaussians", "20000", "--res", "256", "--no-cpu-baseline", "--capture", "off", "--exchange", "dense",
           "--sustain-seconds", "0", "--rotate-seconds", "0", "--train-seconds", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["scaling"] == "weak"
    assert "dense" in line["config"]["parallelism"]


def test_bench_gpus_flag_launches_the_ranks_itself(built_lib):
    """`python bench.py --gpus 2` with NO launcher around it (the flag was parsed and ignored, the run
    measured one GPU): the script starts itself under torch.distributed.run, two ranks come up, rank 0 prints one line with
    n_gpus = 2, the all-reduce of the real arena is timed (`rccl`) and the exchange format is measured, then chosen."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(GSR_BENCH_BACKEND="gloo", GSR_BENCH_SHARE_GPU="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--gaussians",
           "20000", "--res", "256", "--full", "--no-cpu-baseline", "--capture", "off", "--sustain-seconds", "0",
           "--rotate-seconds", "0", "--train-seconds", "0", "--exchange-probe-steps", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["gpus_requested"] == 2 and line["value"] > 0
    assert line["rccl"]["ranks"] == 2 and line["rccl"]["allreduce_ms"] > 0 and line["rccl"]["arena_bytes"] >= 236 * 20000
    probe = line["exchange"]["probe_ms_per_step"]
    assert set(probe) == {"dense", "rows"} and all(v["ms_per_step"] > 0 for v in probe.values())
    assert line["exchange"]["format"] == min(probe, key=lambda f: probe[f]["ms_per_step"])


def _legacy_rows_worker(rank, world, port, out_dir):
    """render_views_data_parallel with a FOUR-argument callback (overwrites the arena, K8 accumulate = 0 per view) in the
    `rows` wire format: ADVICE r3 -- the reached-row bitmap K8 leaves describes the last view only; if it stayed valid the
    exchange would drop the rows only earlier views reached."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from dreamscene_amd import _lib, multiview
    from dreamscene_amd.rasterizer import GaussianRasterizer, RasterContext
    from tests.util import settings_for
    _lib.load()
    params, cams, ups = _scene(dev)
    arena = multiview.GradArena(P, K, dev)
    ex = multiview.GradExchange(arena, sh_degree=D, mode="rows")

    def legacy(prm, cam, grad_out, up):
        rast = GaussianRasterizer(settings_for(cam, np.ones(3, np.float32), D, dev), context=RasterContext(grad_arena=arena))
        m2d = torch.zeros((P, 3), device=dev, requires_grad=True)
        pr = {k: v.clone().requires_grad_(True) for k, v in prm.items()}
        img, radii, da = rast(means3D=pr["means3D"], means2D=m2d, opacities=pr["opacities"], shs=pr["shs"],
                              scales=pr["scales"], rotations=pr["rotations"])
        torch.autograd.grad([img, da], [m2d], [up[0], up[1]])
        return radii

    multiview.render_views_data_parallel(legacy, params, cams, ups, arena, exchange=ex)
    torch.cuda.synchronize(dev)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), flat=arena.flat.cpu().numpy(), last=json.dumps(ex.last))
    dist.barrier()
    dist.destroy_process_group()


def test_rows_exchange_with_a_four_argument_callback(built_lib, tmp_path):
    from dreamscene_amd import multiview
    world = 2
    mp.spawn(_legacy_rows_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert np.array_equal(r0["flat"], r1["flat"])
    assert json.loads(str(r0["last"]))["format"] == "rows"
    dev = torch.device("cuda", 0)
    params, cams, ups = _scene(dev)
    arena = multiview.GradArena(P, K, dev)
    for _ in range(2):
        _render_into_arena(params, cams, ups, list(range(NV)), arena, dev)
    ref = arena.flat.cpu().numpy().astype(np.float64)
    scale = rel_scale(ref)
    e = float(np.abs(r0["flat"].astype(np.float64) - ref).max())
    assert e <= 1e-5 * scale, f"rows exchange after a host-side view sum lost gradient rows: {e:.3e} (scale {scale:.3e})"
