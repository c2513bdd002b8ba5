"""-m gpu: the K7 -> K8 scratch contract of the C ABI (include/gsrast.h, GsrGrads.reach / .scratch_clean). With
scratch_clean the caller keeps `partials` + `reach` between calls, hands them over ALL ZERO and gets them back all zero --
no clear is launched; without it the library clears whatever it is given. Both protocols give the same gradients, for
every form of K8 (the sparse and dense views kernels restore the scratch themselves; the scene forms and the single-view
kernel get it cleared behind them). K >= 9 reaches the dense views kernel only under GSR_K8_SPARSE=0, which the library
reads once per load: that case runs in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import rel_scale, same_bits, settings_for, small_scene, tol_ok

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_scratch_zero(R):
    n = 0
    for sc in R._SCRATCH.values():
        assert not sc.dirty
        assert int(torch.count_nonzero(sc.partials)) == 0, "partials not restored to zero"
        assert int(torch.count_nonzero(sc.reach)) == 0, "reach marks not restored to zero"
        n += 1
    return n


def _legacy_bind(gr, sc, k=0):
    """the protocol without the contract: garbage in, the library clears (and may leave anything behind)"""
    sc.partials[k].fill_(float("nan"))
    gr.partials = sc.partials[k].data_ptr()
    gr.reach = None
    gr.scratch_clean = 0


def _legacy_bind_reach(gr, sc, k=0):
    """reach given, but no promise: the library clears both first"""
    sc.partials[k].fill_(float("nan"))
    sc.reach[k].fill_(7)
    gr.partials = sc.partials[k].data_ptr()
    gr.reach = sc.reach[k].data_ptr()
    gr.scratch_clean = 0


def _protocols_agree(K, D, V, cam_grads):
    """K, D, V views of one scene, three calls per protocol: the scratch comes back all zero, and the two protocols
    without the contract give the same gradients. Returns the contract's gradients (leaves, means2D[, viewmatrix])."""
    from dreamscene_amd import rasterizer as R, synth
    from dreamscene_amd.views import GaussianRasterizerViews
    dev = torch.device(DEV)
    P, H, W = 2500, 112, 144
    g, _ = small_scene(P=P, H=H, W=W, K=K, seed=13)
    cams = synth.object_cameras(V + 1, H, W, radius=3.0)[1:]
    t = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in g.items()}
    leaves = [t[k] for k in ("means3D", "shs", "opacities", "scales", "rotations")]
    gis = [torch.tensor(synth.upstream_grads(H, W, seed=k)[0], device=dev) for k in range(V)]
    gdas = [torch.tensor(synth.upstream_grads(H, W, seed=k)[1], device=dev) for k in range(V)]
    sets = [settings_for(c, [1, 1, 1], D, dev) for c in cams]
    if cam_grads:      # camera tensors that require grad: the single-view kernel that does not restore the scratch itself
        sets = [s._replace(viewmatrix=s.viewmatrix.clone().requires_grad_(True)) for s in sets]

    def run():
        R._SCRATCH.clear()
        res = None
        for rep in range(3):       # (first call of the views path runs view by view; the later ones batched)
            if V == 1:
                m2d = torch.zeros((P, 3), device=dev, requires_grad=True)
                img, radii, da = R.GaussianRasterizer(sets[0])(means3D=t["means3D"], means2D=m2d, shs=t["shs"],
                                                                opacities=t["opacities"], scales=t["scales"],
                                                                rotations=t["rotations"])
                extra = [sets[0].viewmatrix] if cam_grads else []
                res = torch.autograd.grad([img, da], leaves + [m2d] + extra, [gis[0], gdas[0]])
            else:
                m2d = torch.zeros((V, P, 3), device=dev, requires_grad=True)
                outs = GaussianRasterizerViews(sets)(means3D=t["means3D"], means2D=m2d, shs=t["shs"],
                                                     opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
                res = torch.autograd.grad([x for (img, _, da) in outs for x in (img, da)], leaves + [m2d],
                                          [y for k in range(V) for y in (gis[k], gdas[k])])
            torch.cuda.synchronize()
        return [x.detach().cpu().numpy() for x in res]

    clean = run()
    assert _all_scratch_zero(R) >= 1
    assert sum(float(np.abs(x).sum()) for x in clean) > 0
    bind = R._bind_scratch
    try:
        R._bind_scratch = _legacy_bind
        legacy = run()
        R._bind_scratch = _legacy_bind_reach
        legacy_reach = run()
    finally:
        R._bind_scratch = bind
    for a, b, c in zip(clean, legacy, legacy_reach):
        assert np.isfinite(b).all() and np.isfinite(c).all()
        assert tol_ok(a, b, atol=2e-6) and tol_ok(a, c, atol=2e-6)      # (fp32 atomics: order varies run to run)
    return clean


@pytest.mark.parametrize("K,D,V,cam_grads", [(16, 3, 3, False), (4, 1, 2, False), (16, 3, 1, False), (16, 3, 1, True),
                                             (9, 2, 4, False)])
def test_scratch_is_returned_clean_and_protocols_agree(built_lib, K, D, V, cam_grads):
    _protocols_agree(K, D, V, cam_grads)


DENSE_CASES = [(16, 3, 3, False), (16, 3, 1, False)]


def _dense_child(path):
    """the child of the test below, started with GSR_K8_SPARSE=0: the scenarios above, gradients to `path`"""
    np.savez(path, **{f"c{c}_{i}": x for c, case in enumerate(DENSE_CASES) for i, x in enumerate(_protocols_agree(*case))})


def test_dense_forms_keep_the_contract(built_lib, tmp_path):
    """GSR_K8_SPARSE=0 (read once per library load, hence a fresh process): K = 16 then takes the dense views kernel for
    3 views and the single-view kernel for one. Each keeps the contract and gives the gradients of the default form."""
    path = tmp_path / "dense.npz"
    cmd = [sys.executable, "-c", "import sys; from tests.test_scratch import _dense_child; _dense_child(sys.argv[1])",
           str(path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, GSR_K8_SPARSE="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    dense = np.load(path)
    for c, case in enumerate(DENSE_CASES):
        for i, a in enumerate(_protocols_agree(*case)):
            assert tol_ok(dense[f"c{c}_{i}"], a, atol=2e-6), (case, i)


def test_scene_forms_clear_the_scratch_behind_them(built_lib):
    """raw-leaf scene input (dreamscene_amd/scene.py): K8's scene kernels read the sums directly; the library clears the
    scratch after them, so the contract holds for the next call on the same buffers."""
    from dreamscene_amd import rasterizer as R, scene
    from tests.test_golden import _cam_from_fixture, load
    from tests.test_scene import _models_from_fixture, _loss
    d = load("scene_render.npz")
    dev = torch.device(DEV)
    R._SCRATCH.clear()
    ref = None
    for rep in range(2):
        models = _models_from_fixture(d, device=dev)
        out = scene.scene_render(models, _cam_from_fixture(d), torch.tensor(d["bg"], device=dev), int(d["active_sh_degree"]),
                                 test=True)
        _loss(out, d, dev).backward()
        torch.cuda.synchronize()
        grads = [t.grad.detach().cpu().numpy() for m in models for t in m]
        assert _all_scratch_zero(R) >= 1
        if ref is None:
            ref = grads
        else:
            for a, b in zip(grads, ref):      # (run-to-run: the order of K7's fp32 atomics)
                assert float(np.abs(a - b).max()) <= 1e-5 * rel_scale(b)


@pytest.mark.parametrize("door", ["raw", "raw_scene", "views", "views_scene"])
def test_a_failed_enqueue_releases_the_scratch_and_the_next_call_rezeroes_it(built_lib, monkeypatch, door):
    """the persistent K7 -> K8 scratch is locked for the length of one enqueue (two host threads on a stream must
    not interleave K7(A), K7(B), K8(A)); a call that raises half-way releases the lock, leaves the scratch flagged dirty, and
    the next call zeroes it before use. For every entry point of the backward: rasterize_backward_raw on a plain and on a scene
    state, the two views functions (two views). The two that take a GradArena write into one, which must not trust its
    reached-row bitmap after the failure."""
    from dreamscene_amd import multiview, rasterizer as R, _lib as L
    from tests.test_backward_doors import P, forward, gaussians, raw_model, views_setup
    dev = torch.device(DEV)
    K, D = 16, 3
    scene, V = door.endswith("scene"), (2 if door.startswith("views") else 1)
    t = gaussians(K, seed=17)
    model = raw_model(t) if scene else None
    sets, gis, gdas = views_setup(D, V)
    arena = None if scene else multiview.GradArena(P, K, dev)

    def backward():
        sts = [forward(R, s, t, model)[1] for s in sets]
        if door == "views":
            o = R.rasterize_backward_views_raw(sts, gis, gdas, arena=arena)
        elif door == "views_scene":
            o = R.rasterize_backward_views_scene_raw(sts, gis, gdas)
        else:
            o = R.rasterize_backward_raw(sts[0], gis[0], gdas[0], arena=arena)
        torch.cuda.synchronize()
        res = {f"leaf {j}": x for j, x in enumerate(o["model_grads"][0])} if scene else \
            {k: o[k] for k in ("dL_dmeans3D", "dL_dshs", "dL_dscales", "dL_drotations", "dL_dopacities")}
        res["dL_dmeans2D"] = o["dL_dmeans2D"]
        return {k: x.clone() for k, x in res.items()}       # (with an arena every call returns the same memory)
    ref = backward()
    assert sum(float(x.abs().sum()) for x in ref.values()) > 0
    sc = list(R._SCRATCH.values())[-1]              # (most recently used: this call's)
    assert sc.partials.shape[:2] == (V, P)
    assert arena is None or arena.reached_valid
    real_check = L.check
    failed = []

    def failing_check(code, what):
        if what == ("gsr_backward_views" if V > 1 else "gsr_backward"):
            sc.partials.fill_(3.0)              # (what a half-enqueued K7 would leave behind)
            failed.append(what)
            raise L.GsrError("injected failure")
        return real_check(code, what)
    monkeypatch.setattr(R.L, "check", failing_check)
    with pytest.raises(L.GsrError):
        backward()
    monkeypatch.setattr(R.L, "check", real_check)
    assert len(failed) == 1
    assert sc.dirty and not sc.lock.locked()
    assert arena is None or not arena.reached_valid
    again = backward()
    assert not sc.dirty and not sc.lock.locked()
    assert arena is None or arena.reached_valid
    for k in ref:
        same_bits(ref[k], again[k], k)
    assert int(torch.count_nonzero(sc.partials)) == 0
