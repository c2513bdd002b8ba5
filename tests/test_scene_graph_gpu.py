"""-m gpu: the captured raw-leaf step -- dreamscene_amd/scene_graph.py -- against `scene.rasterize_models_views` given the same
inputs, step by step: images, depth_alpha, radii and the returned scales bit-identical (the same kernels run in the same order
within a view), gradients at the bar tests/test_graph.py holds captured against eager to (fp32 atomics order), the
densification statistics at tests/test_graph.py's bar as well.

The scene: models of 1 800 + 1 200 (+ 7) rows built as tests/test_noise_gpu.py builds its own (small splats, cameras inside
the cloud: every view culls some Gaussians and has some behind it), 112 x 144 pixels (7 x 9 tiles, not multiples of 16)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.util import settings_for, tol_ok

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 112, 144
SEED = 0x9E3779B97F4A7C15


def _model(n, mi, K, seed=70, scale=0.5):
    """Raw leaves of one model, tests/test_noise_gpu.py's recipe."""
    from dreamscene_amd import synth
    g = synth.g_object(max(n, 64), seed=seed + mi, K=K)     # (kNN scales need neighbours)
    g = {k: v[:n] for k, v in g.items()}
    sc = (g["scales"] * scale).astype(np.float32)
    op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
    off = np.array([[0.4 * (mi - 1), 0.15 * mi, 0.0]], dtype=np.float32)
    raw = (g["means3D"] * 0.8 + off, np.log(sc), g["rotations"] * (0.6 + 0.5 * mi), np.log(op / (1 - op)),
           g["shs"][:, :1, :], g["shs"][:, 1:, :])
    return tuple(torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV, requires_grad=True) for a in raw)


def _models(K, sizes=(1800, 1200, 7)):
    return [_model(n, mi, K) for mi, n in enumerate(sizes)]


def _leaves(models):
    return [t for m in models for t in m]


def _P(models):
    return sum(int(m[0].shape[0]) for m in models)


_CAMS, _UP = {}, {}


def _cams(h=H, w=W, radius=0.45):
    from dreamscene_amd import synth
    if (h, w, radius) not in _CAMS:
        _CAMS[h, w, radius] = synth.object_cameras(8, h, w, radius=radius, fovx=0.46)
    return _CAMS[h, w, radius]


def _upstream(k, h=H, w=W):
    from dreamscene_amd import synth
    if (k, h, w) not in _UP:
        gi, gda = synth.upstream_grads(h, w, seed=k)
        _UP[k, h, w] = (torch.tensor(gi, device=DEV), torch.tensor(gda, device=DEV))
    return _UP[k, h, w]


def _sets(step, V, D, h=H, w=W, radius=0.45):
    """Cameras, backgrounds and active SH degree that change with the step; another field of view at step 4."""
    sets = []
    for k in range(V):
        s = settings_for(_cams(h, w, radius)[(step + 2 * k) % 8], [0.1 * step, 0.4, 1.0 - 0.2 * k],
                         D if (step + k) % 3 else 0, DEV)
        if step == 4:
            s = s._replace(tanfovx=s.tanfovx * 1.25, tanfovy=s.tanfovy * 1.25)
        sets.append(s)
    return sets


def _loss(outs, scale_views=None):
    h, w = outs[0][0].shape[1:]
    loss = 0.0
    for k, (img, _, da, sc) in enumerate(outs):
        gi, gda = _upstream(k, h, w)
        loss = loss + (img * gi).sum() + (da * gda).sum()
        if scale_views is None or k in scale_views:
            loss = loss + 0.01 * (k + 1) * sc.mean()
    return loss


def _prime(sets, models):
    """One throwaway eager step: the first multi-view call of a (P, H, W) runs view by view (no capacity hint yet); every
    eager call after it is the batched one."""
    from dreamscene_amd import scene
    with torch.no_grad():
        scene.rasterize_models_views(sets, models, torch.zeros((len(sets), _P(models), 3), device=DEV))


def _run(call, sets, models, scale_views=None, leaves=True, **noise):
    """One step forward + backward through `call` (the module or the eager function). -> (outputs, gradients), cloned."""
    V = len(sets)
    m2d = torch.zeros((V, _P(models), 3), device=DEV, requires_grad=True)
    outs = call(sets, models, m2d, **noise)
    grads = torch.autograd.grad(_loss(outs, scale_views), [m2d] + (_leaves(models) if leaves else []), allow_unused=True)
    return [tuple(x.clone() for x in o) for o in outs], [None if x is None else x.clone() for x in grads]


def _same_outputs(got, ref, what):
    for k, (a, b) in enumerate(zip(got, ref)):
        for name, x, y in zip(("image", "radii", "depth_alpha", "scales"), a, b):
            assert torch.equal(x, y), f"{what}: view {k} {name}: {(x != y).sum().item()} of {x.numel()} entries differ"


def _close_grads(got, ref, what):
    assert len(got) == len(ref)
    for j, (a, b) in enumerate(zip(got, ref)):
        if a is None or b is None:
            assert a is None and b is None, (what, j)
        elif b.numel():
            assert tol_ok(a.reshape(b.shape), b, atol=2e-6), f"{what}: gradient {j}"      # (fp32 atomics order)


def _eager_call(context=None):
    from dreamscene_amd import scene
    return lambda sets, models, m2d, **noise: scene.rasterize_models_views(sets, models, m2d, context=context, **noise)


@pytest.mark.parametrize("V,K,D,form", [(4, 16, 3, "int"), (1, 4, 1, "none"), (3, 9, 2, "tensors"), (2, 16, 3, "words")])
def test_captured_step_equals_eager_and_follows_the_cameras(built_lib, V, K, D, form):
    """Five steps with different cameras, bg, SH degree (FoV at the last) and a new stream id each; a leaf moves in place
    after every step. Steps 0-1 run eagerly, step 2 captures, 3-4 replay."""
    from dreamscene_amd import scene
    from dreamscene_amd.scene_graph import CapturedModelsViews
    models = _models(K, (1800, 1200, 7) if V != 1 else (1800, 1200))
    P = _P(models)
    rast = CapturedModelsViews()
    gen = torch.Generator().manual_seed(11)
    words = torch.zeros(V, dtype=torch.int32, device=DEV)           # the caller's stream tensor ("words")
    _prime(_sets(0, V, D), models)
    ids = lambda step: 1000 + 17 * step

    def noise_of(step, sid=None):
        sid = ids(step) if sid is None else sid
        if form == "int":
            return dict(noise=scene.NoiseSpec(SEED, sid))
        if form == "words":
            words.copy_(torch.arange(sid, sid + V, dtype=torch.int32))
            return dict(noise=scene.NoiseSpec(SEED, words, shs=False))
        return {}
    for step in range(5):
        sets = _sets(step, V, D)
        noise = noise_of(step)
        if form == "tensors":
            noise = dict(scale_noise=torch.randn((V, P, 3), generator=gen).to(DEV),
                         sh_noise=torch.randn((V, P, K, 3), generator=gen).to(DEV))
        ref = _run(_eager_call(), sets, models, **noise)
        got = _run(rast, sets, models, **noise)
        _same_outputs(got[0], ref[0], f"step {step}")
        _close_grads(got[1], ref[1], f"step {step}")
        if step == 4 and form in ("int", "words"):
            # the ids are read when the kernels run, not baked into the graph: step 3's id gives another image
            with torch.no_grad():
                stale = scene.rasterize_models_views(sets, models, torch.zeros((V, P, 3), device=DEV), **noise_of(4, ids(3)))
            assert not torch.equal(stale[0][0], got[0][0][0]) and not torch.equal(stale[0][3], got[0][0][3])
        with torch.no_grad():                    # a zero-copy capture must see this
            models[step % len(models)][step % 4].add_(1e-3)
    assert rast.stats["captures"] == 1 and rast.stats["replays"] == 3 and rast.stats["eager_steps"] == 2, rast.stats
    assert rast.stats["overflows"] == 0


@pytest.mark.parametrize("V", [1, 16])
def test_pack_views_streams_writes_the_block_and_the_words(built_lib, V):
    from dreamscene_amd import _lib as L
    from dreamscene_amd.graph import user_view
    from dreamscene_amd.rasterizer import RasterContext
    lib = built_lib
    sets = [_sets(k, 1, 3)[0]._replace(tanfovx=0.3 + 0.01 * k, sh_degree=k % 4) for k in range(V)]
    structs = (L.GsrView * V)(*[user_view(s, 100, 16, RasterContext()) for s in sets])
    ids = ([0, 2 ** 32 - 1] + [(2654435761 * k) % 2 ** 32 for k in range(2, 16)])[:V] if V > 1 else [2 ** 32 - 1]
    a = torch.full((V, L.GSR_PACKED_VIEW_FLOATS), -7.0, device=DEV)
    b, c = a.clone(), a.clone()
    words = torch.full((V + 1,), 0x55555555, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.gsr_pack_views(V, structs, a.data_ptr(), st), "gsr_pack_views")
    L.check(lib.gsr_pack_views_streams(V, structs, (C.c_uint32 * V)(*ids), b.data_ptr(), words.data_ptr(), st), "streams")
    L.check(lib.gsr_pack_views_streams(V, structs, None, c.data_ptr(), None, st), "streams (NULL)")
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and not bool((a == -7.0).any())
    assert a[0, 40].item() == np.float32(0.3) and a[V - 1, 42].item() == float((V - 1) % 4)
    got = [int(x) & 0xFFFFFFFF for x in words.cpu().tolist()]
    assert got[:V] == ids and got[V] == 0x55555555          # the ids, and nothing past them


def test_captured_step_in_the_trainers_configuration(built_lib):
    """Gradients ADDED into model_grad_buffers, densification statistics of the last view, seeded scale noise, a loss on the
    returned scales of views 0 and 2 only (the others must get what the eager path gives them: no gradient pointer)."""
    from dreamscene_amd import densify, scene
    from dreamscene_amd.scene_graph import CapturedModelsViews
    V, K, D = 4, 16, 3
    models = _models(K)
    P = _P(models)
    dev = torch.device(DEV)
    zeros = lambda: [tuple(torch.zeros_like(t) for t in m) for m in models]
    bufs_c, bufs_e = zeros(), zeros()
    stats_c, stats_e = densify.DensifyStats(P, dev), densify.DensifyStats(P, dev)
    rast = CapturedModelsViews(context=scene.SceneContext(model_grad_buffers=bufs_c, densify_stats=stats_c.tensors()))
    eager = _eager_call(scene.SceneContext(model_grad_buffers=bufs_e, densify_stats=stats_e.tensors()))
    _prime(_sets(0, V, D), models)
    for step in range(5):
        sets = _sets(step, V, D)
        noise = dict(noise=scene.NoiseSpec(SEED, 4 * step, shs=False))
        ref = _run(eager, sets, models, scale_views=(0, 2), leaves=False, **noise)
        got = _run(rast, sets, models, scale_views=(0, 2), leaves=False, **noise)
        _same_outputs(got[0], ref[0], f"step {step}")
        _close_grads(got[1], ref[1], f"step {step}")
        for m, (rc_, re_) in enumerate(zip(bufs_c, bufs_e)):
            for j, (a, b) in enumerate(zip(rc_, re_)):
                if b.numel():
                    assert m == 2 or bool(b.abs().max() > 0), (step, m, j)       # (the 7-row model may be culled whole)
                    assert tol_ok(a, b, atol=2e-6), f"step {step}: buffer of model {m} leaf {j}"
        assert torch.equal(stats_c.denom, stats_e.denom) and torch.equal(stats_c.max_radii2D, stats_e.max_radii2D), step
        np.testing.assert_allclose(stats_c.xyz_gradient_accum.cpu().numpy(), stats_e.xyz_gradient_accum.cpu().numpy(),
                                   rtol=1e-5, atol=1e-9)
    assert int(stats_c.denom.max()) == 5
    assert rast.stats["captures"] == 1 and rast.stats["replays"] == 3, rast.stats


def test_grad_never_aliases_the_static_tensors(built_lib):
    """Without buffers autograd receives the capture's static tensors; loss.backward() must COPY them into .grad."""
    from dreamscene_amd import scene
    from dreamscene_amd.scene_graph import CapturedModelsViews
    V, K, D = 2, 4, 1
    models = _models(K, (1800, 1200))
    leaves = _leaves(models)
    rast = CapturedModelsViews()
    kept = None
    for step in range(5):
        sets = _sets(step, V, D)
        m2d = torch.zeros((V, _P(models), 3), device=DEV, requires_grad=True)
        for t in leaves:
            t.grad = None                       # (zero_grad(set_to_none=True))
        _loss(rast(sets, models, m2d, noise=scene.NoiseSpec(SEED, step))).backward()
        mine = [m2d.grad] + [t.grad for t in leaves]
        assert all(g is not None for g in mine)
        if step >= 3:
            cap = rast._cap
            static = {cap.bwd["_m2d"].data_ptr()} | {g.data_ptr() for row in cap.bwd["model_grads"] for g in row if g.numel()}
            assert not any(g.data_ptr() in static for g in mine if g.numel()), "a .grad aliases the capture's static tensors"
        if step == 3:
            kept = [(g, g.clone()) for g in mine]
        if step == 4:
            torch.cuda.synchronize()
            for (g, c), now in zip(kept, mine):
                assert torch.equal(g, c), "step 3's .grad changed when step 4 ran"
                if g.numel():
                    assert g.data_ptr() != now.data_ptr()
                    assert not torch.equal(g, now)
    assert rast.stats["replays"] == 3 and rast.stats["captures"] == 1, rast.stats


def test_overflow_falls_back_and_recaptures(built_lib):
    """2 000 rows, 192 x 256, headroom 1.0: the splats grow twelvefold after four steps, a view's pair count exceeds the
    captured capacity, that step is redone eagerly (exact) and the next one captures again with more room."""
    from dreamscene_amd import synth
    from dreamscene_amd.scene_graph import CapturedModelsViews
    V, P, h, w, K, D = 2, 2000, 192, 256, 4, 1
    g = synth.g_object(P, seed=41, K=K)
    op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
    raw = (g["means3D"], np.log(g["scales"]), g["rotations"], np.log(op / (1 - op)), g["shs"][:, :1, :], g["shs"][:, 1:, :])
    models = [tuple(torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV, requires_grad=True) for a in raw)]
    sets = [settings_for(_cams(h, w, 3.0)[k + 1], [0, 0, 0], D, DEV) for k in range(V)]
    _prime(sets, models)
    rast = CapturedModelsViews(headroom=1.0)
    cap_before = None
    for step in range(8):
        if step == 4:
            with torch.no_grad():
                models[0][1].add_(float(np.log(12.0)))
        ref = _run(_eager_call(), sets, models)
        got = _run(rast, sets, models)
        _same_outputs(got[0], ref[0], f"step {step}")
        _close_grads(got[1], ref[1], f"step {step}")
        if step == 3:
            cap_before = rast._cap.cap
    assert rast.stats["overflows"] == 1 and rast.stats["captures"] == 2, rast.stats
    assert rast.stats["eager_steps"] == 3 and rast._cap.cap > cap_before, (rast.stats, rast._cap.cap, cap_before)


def test_densified_model_warms_up_and_captures_again(built_lib):
    from dreamscene_amd import scene
    from dreamscene_amd.scene_graph import CapturedModelsViews
    V, K, D = 2, 4, 1
    models = _models(K, (1800, 1200))
    rast = CapturedModelsViews()
    for step in range(8):
        if step == 4:
            models[1] = _model(900, 5, K)        # another row count: new tensors, a new step shape
        sets = _sets(step, V, D)
        if step in (0, 4):
            _prime(sets, models)
        noise = dict(noise=scene.NoiseSpec(SEED, step))
        ref = _run(_eager_call(), sets, models, **noise)
        got = _run(rast, sets, models, **noise)
        _same_outputs(got[0], ref[0], f"step {step}")
        _close_grads(got[1], ref[1], f"step {step}")
        expect = dict(captures=(step >= 2) + (step >= 6), eager_steps=min(step + 1, 2) + (min(step - 3, 2) if step >= 4 else 0),
                      replays=max(0, min(step - 1, 2)) + max(0, step - 5), overflows=0)
        assert {k: rast.stats[k] for k in expect} == expect, (step, rast.stats, expect)


def test_pending_backward_and_overwritten_replay(built_lib):
    """An eval render under no_grad between a step's forward and its backward runs eagerly and leaves the capture alone; a
    backward of a replay that a later forward has overwritten raises."""
    from dreamscene_amd import scene
    from dreamscene_amd.graph import WARM_CALLS
    from dreamscene_amd.scene_graph import CapturedModelsViews
    V, K, D = 2, 4, 1
    models = _models(K, (1800, 1200))
    P = _P(models)
    leaves = _leaves(models)
    rast = CapturedModelsViews()
    spec = scene.NoiseSpec(SEED, 5, shs=False)

    def fwd(step):
        m2d = torch.zeros((V, P, 3), device=DEV, requires_grad=True)
        return rast(_sets(step, V, D), models, m2d, noise=spec)
    for step in range(WARM_CALLS + 2):          # warm-up, capture, one replay -- each with its own backward
        _loss(fwd(step)).backward()
    for t in leaves:
        t.grad = None
    _loss(fwd(20)).backward()                   # reference: step 20 with nothing in between
    ref = [t.grad.clone() for t in leaves]
    for t in leaves:
        t.grad = None
    loss = _loss(fwd(20))
    replays, eager_steps = rast.stats["replays"], rast.stats["eager_steps"]
    with torch.no_grad():                       # the eval render: other cameras, forward only
        ev = rast(_sets(3, V, D), models, torch.zeros((V, P, 3), device=DEV), noise=spec)
        ev_ref = scene.rasterize_models_views(_sets(3, V, D), models, torch.zeros((V, P, 3), device=DEV), noise=spec)
    assert rast.stats["replays"] == replays and rast.stats["eager_steps"] == eager_steps + 1
    _same_outputs(ev, ev_ref, "eval render")
    loss.backward()                             # no "overwritten by a later forward"
    for t, r in zip(leaves, ref):
        if r.numel():
            assert tol_ok(t.grad, r, atol=2e-6)
    with torch.no_grad():                       # nothing pending any more: forward-only calls replay again
        rast(_sets(4, V, D), models, torch.zeros((V, P, 3), device=DEV), noise=spec)
    assert rast.stats["replays"] == replays + 1
    first = _loss(fwd(10))
    second = _loss(fwd(11))                     # overwrites the static state `first` refers to
    with pytest.raises(RuntimeError, match="overwritten by a later forward"):
        first.backward()
    second.backward()                           # the latest forward still differentiates
    assert rast.stats["captures"] == 1 and rast.stats["overflows"] == 0


@pytest.mark.parametrize("direct", [True, False])
def test_backward_graph_over_the_callers_gradient_tensors(built_lib, monkeypatch, direct):
    """Upstream gradients that are contiguous fp32 tensors at addresses that repeat (what a loss produces): the backward graph is
    captured over them and nothing is copied; with no direct graphs left they are copied into the static buffers. Scale
    gradients for views 0 and 2 only, either way equal to the eager call given the same gradients."""
    from dreamscene_amd import graph, scene
    from dreamscene_amd.scene_graph import CapturedModelsViews
    if not direct:
        monkeypatch.setattr(graph, "MAX_DIRECT_GRAPHS", 0)
    V, K, D = 3, 9, 2
    models = _models(K)
    P = _P(models)
    leaves = _leaves(models)
    gen = torch.Generator().manual_seed(3)
    g_sc = [torch.randn((P, 3), generator=gen).to(DEV) * 1e-3 if k != 1 else None for k in range(V)]
    rast = CapturedModelsViews()
    _prime(_sets(0, V, D), models)

    def run(call, sets, noise):
        m2d = torch.zeros((V, P, 3), device=DEV, requires_grad=True)
        outs = call(sets, models, m2d, **noise)
        ys, gs = [], []
        for k, (img, _, da, sc) in enumerate(outs):
            ys += [img, da] + ([sc] if g_sc[k] is not None else [])
            gs += list(_upstream(k)) + ([g_sc[k]] if g_sc[k] is not None else [])
        grads = torch.autograd.grad(ys, [m2d] + leaves, gs, allow_unused=True)
        return [tuple(x.clone() for x in o) for o in outs], [None if x is None else x.clone() for x in grads]
    for step in range(5):
        sets = _sets(step, V, D)
        noise = dict(noise=scene.NoiseSpec(SEED, 3 * step))
        ref = run(_eager_call(), sets, noise)
        got = run(rast, sets, noise)
        _same_outputs(got[0], ref[0], f"step {step}")
        _close_grads(got[1], ref[1], f"step {step}")
    assert rast.stats["replays"] == 3 and rast.stats.get("captures_bwd_direct", 0) == (1 if direct else 0), rast.stats
