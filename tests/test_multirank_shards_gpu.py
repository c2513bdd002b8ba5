"""-m gpu: the view-sharded step with EMPTY and UNEVEN shards. The trainers render C_batch_size = 4 views per step:
with more ranks than views some ranks render nothing, and with 3 views on 2 ranks one rank renders two views and the other one.
Every rank must still speak the same wire protocol (GradExchange: the plan is a function of rank-invariant state only) and end up
with the same bits.

Ranks share cuda:0 and talk over gloo (as tests/test_multirank_gpu.py). One spawn per (world, mode) runs a schedule of steps on ONE
arena and ONE GradExchange: the number of views per step changes, and so does the callback style (keyword `accumulate=`, five
positional arguments, the four-argument overwrite contract), so empty, single-view and multi-view shards meet every style, and a
rank that was empty in one step has views in the next. Collectives are bounded (60 s): a protocol mismatch fails, it does not hang.

After every exchange the workers check that the plan (format, device form, learnt capacities) and the arena bits agree on all
ranks. The parent checks every step against an independent float64 reference: the step's views rendered one at a time through
the plain GaussianRasterizer (ordinary autograd .grad tensors, no arena, no accumulate), summed in float64 in view order."""
import hashlib
import json
import os
import socket
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.util import rel_scale

pytestmark = pytest.mark.gpu

P, K, RES, POOL = 12_001, 16, 192, 5        # P: no multiple of 2, 3 or 64 -- uneven owner slices, a partial bitmap word
SCHEDULE = {2: [1, 3, 4, 1, 2], 3: [1, 2, 4, 5, 1]}
STYLES = ("keyword", "positional", "four")
REGIONS = ("means3D", "scales", "rotations", "opacities", "shs")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _scene(dev):
    from dreamscene_amd import synth
    g = synth.g_object(P, seed=4, K=K)
    g["means3D"][::8, 2] = 30.0             # far above every orbit camera: rows that no view reaches
    cams = synth.object_cameras(POOL, RES, RES)
    params = {k: torch.tensor(v, device=dev) for k, v in g.items()}
    ups = [tuple(torch.tensor(x, device=dev) for x in synth.upstream_grads(RES, RES, i)) for i in range(POOL)]
    return params, cams, ups


def _callbacks(arena, D, dev):
    from dreamscene_amd.rasterizer import GaussianRasterizer, RasterContext
    from tests.util import settings_for

    def run(prm, cam, up, accumulate):
        rast = GaussianRasterizer(settings_for(cam, np.ones(3, np.float32), D, dev),
                                  context=RasterContext(grad_arena=arena, accumulate=accumulate))
        m2d = torch.zeros((P, 3), device=dev, requires_grad=True)
        pr = {k: v.clone().requires_grad_(True) for k, v in prm.items()}
        img, radii, da = rast(means3D=pr["means3D"], means2D=m2d, opacities=pr["opacities"], shs=pr["shs"],
                              scales=pr["scales"], rotations=pr["rotations"])
        torch.autograd.grad([img, da], [m2d], [up[0], up[1]])
        return radii

    def keyword(prm, cam, grad_out, up, accumulate=False):
        return run(prm, cam, up, accumulate)

    def positional(prm, cam, grad_out, up, acc):
        return run(prm, cam, up, acc)

    def four(prm, cam, grad_out, up):
        return run(prm, cam, up, False)
    return dict(keyword=keyword, positional=positional, four=four)


def _expected_formats(mode):
    return ("sparse_rs", "dense") if mode == "auto" else (mode,)


def _worker(rank, world, port, mode, strict, D, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from dreamscene_amd import _lib, multiview
    _lib.load()
    params, cams, ups = _scene(dev)
    arena = multiview.GradArena(P, K, dev)
    ex = multiview.GradExchange(arena, sh_degree=D, mode=mode, strict=strict)
    cbs = _callbacks(arena, D, dev)
    warm = [] if strict else [4, 4]         # strict=False: learn the capacities first (a warm-up step may overflow, by contract)
    flats, fmts = [], []
    for s, n in enumerate(warm + SCHEDULE[world]):
        scheduled = s >= len(warm)
        style = STYLES[(s - len(warm)) % 3] if scheduled else "keyword"
        multiview.render_views_data_parallel(cbs[style], params, cams[:n], ups[:n], arena, exchange=ex)
        fitted = ex.finish()
        torch.cuda.synchronize(dev)
        flat = arena.flat.cpu().numpy()
        info = dict(format=ex.last.get("format"), device=ex.last.get("device"), rows_cap=ex._rows_cap,
                    rs_caps=list(ex._rs_caps), fitted=fitted,
                    sha=hashlib.sha256(flat.tobytes()).hexdigest() if scheduled else None)
        seen = [None] * world
        dist.all_gather_object(seen, info)
        what = f"step {s} (n={n}, {style}, rank {rank})"
        for k in ("format", "device", "rows_cap", "rs_caps"):
            assert all(x[k] == seen[0][k] for x in seen), f"{what}: ranks disagree on {k}: {[x[k] for x in seen]}"
        assert info["format"] in _expected_formats(mode), f"{what}: format {info['format']}"
        if mode in ("rows", "sparse_rs"):
            assert info["device"], f"{what}: a cuda arena took the host-count form: {ex.last}"
        if scheduled:
            assert all(x["fitted"] for x in seen), f"{what}: a message overflowed after the warm-up: {seen}"
            assert all(x["sha"] == seen[0]["sha"] for x in seen), f"{what}: the replicas differ after the exchange"
            if not strict:
                assert ex.last.get("host_reads") == 0, f"{what}: {ex.last}"
            flats.append(flat)
            fmts.append(info["format"])
        if arena.zero_outside_ok():
            assert arena.verify_zero_outside(), f"{what}: rows outside the bitmap are not zero after the exchange"
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), flats=np.stack(flats), fmts=json.dumps(fmts))
    dist.barrier()
    dist.destroy_process_group()


_REF = {}


def _per_view_reference(D):
    """float64 parameter gradients of every view of the pool, one plain GaussianRasterizer call per view."""
    if D in _REF:
        return _REF[D]
    from dreamscene_amd.rasterizer import GaussianRasterizer
    from tests.util import settings_for
    dev = torch.device("cuda", 0)
    params, cams, ups = _scene(dev)
    views = []
    for i in range(POOL):
        pr = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        m2d = torch.zeros((P, 3), device=dev, requires_grad=True)
        img, _, da = GaussianRasterizer(settings_for(cams[i], np.ones(3, np.float32), D, dev))(
            means3D=pr["means3D"], means2D=m2d, opacities=pr["opacities"], shs=pr["shs"], scales=pr["scales"],
            rotations=pr["rotations"])
        torch.autograd.backward([img, da], [ups[i][0], ups[i][1]])
        views.append({k: pr[k].grad.detach().cpu().numpy().astype(np.float64).reshape(P, -1) for k in REGIONS})
    _REF[D] = views
    return views


CASES = [(2, "dense", True, 3), (2, "rows", True, 1), (2, "direct", True, 1), (2, "sparse_rs", True, 3), (2, "auto", True, 1),
         (2, "rows", False, 3), (2, "sparse_rs", False, 1),
         (3, "auto", True, 3), (3, "rows", True, 1), (3, "sparse_rs", True, 2)]


@pytest.mark.parametrize("world,mode,strict,D", CASES,
                         ids=[f"w{w}-{m}{'' if s else '-lazy'}-D{d}" for w, m, s, d in CASES])
def test_sharded_steps_equal_the_float64_per_view_sum(built_lib, tmp_path, world, mode, strict, D):
    from dreamscene_amd import multiview
    mp.spawn(_worker, args=(world, _free_port(), mode, strict, D, str(tmp_path)), nprocs=world, join=True)
    rs = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    fmts = json.loads(str(rs[0]["fmts"]))
    assert all(json.loads(str(r["fmts"])) == fmts for r in rs) and all(f in _expected_formats(mode) for f in fmts), fmts
    per_view = _per_view_reference(D)
    nb = (D + 1) ** 2
    layout = multiview.GradArena(P, K, "cpu")
    for s, n in enumerate(SCHEDULE[world]):
        what = f"step {s} (n={n}, {STYLES[s % 3]}, format {fmts[s]})"
        for r in rs[1:]:
            assert np.array_equal(rs[0]["flats"][s], r["flats"][s]), f"{what}: the replicas differ"
        layout.flat.copy_(torch.from_numpy(rs[0]["flats"][s]))
        got = {k: layout.views[k].numpy().astype(np.float64).reshape(P, -1) for k in REGIONS}
        ref = {k: np.zeros((P, per_view[0][k].shape[1])) for k in REGIONS}
        for i in range(n):                                  # view order, float64
            for k in REGIONS:
                ref[k] += per_view[i][k]
        sh = got["shs"].reshape(P, K, 3)
        assert not sh[:, nb:, :].any(), f"{what}: SH columns above the active degree {D} are not zero"
        for k in REGIONS:
            g, e = (sh[:, :nb, :].reshape(P, -1), ref[k].reshape(P, K, 3)[:, :nb, :].reshape(P, -1)) if k == "shs" \
                else (got[k], ref[k])
            scale = rel_scale(e)
            assert np.abs(e).max() > 0, f"{what}: {k}: the reference is zero"
            err = float(np.abs(g - e).max())
            assert err <= 1e-5 * scale, f"{what}: {k} differs from the float64 per-view sum by {err:.3e} (scale {scale:.3e})"
        ref_zero = np.logical_and.reduce([~ref[k].any(1) for k in REGIONS])
        assert ref_zero.sum() >= P // 8, f"{what}: only {int(ref_zero.sum())} rows nobody reached"
        for k in REGIONS:
            assert not got[k][ref_zero].any(), f"{what}: {k}: rows that no view reached are not exactly zero"
