"""-m gpu: the four entry points of the backward (rasterizer.rasterize_backward_raw for plain and scene states,
rasterize_backward_views_raw, rasterize_backward_views_scene_raw) hand their work to the library through one host driver.
One view gives the same gradients through the single-view and the views door, and the densification statistics count
exactly the views `stats_views` names.

Shapes: P = 321 (more than one 256-Gaussian workgroup; the last wave and the last 64-bit reach word both partial), a 48 x 48
image, K = 16 with D = 3 (the sparse views form of K8) and K = 4 with D = 1 (the dense one)."""
import numpy as np
import pytest
import torch

from tests.util import rel_scale, settings_for, small_scene, tol_ok

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, H, W = 321, 48, 48
FORMS = [(16, 3), (4, 1)]
LEAF_GRADS = ("dL_dmeans3D", "dL_dshs", "dL_dopacities", "dL_dscales", "dL_drotations")


def gaussians(K, seed=29):
    g, _ = small_scene(P=P, H=H, W=W, K=K, seed=seed)
    return {k: torch.tensor(v, device=DEV) for k, v in g.items()}


def raw_model(t):
    """The Gaussians `t` as ONE model of a scene: the raw leaves whose activations (exp, sigmoid; the rotation is normalised by
    the kernel) give them back."""
    op = t["opacities"].clamp(1e-4, 1 - 1e-4)
    return tuple(x.contiguous() for x in (t["means3D"], t["scales"].log(), t["rotations"], (op / (1 - op)).log(),
                                          t["shs"][:, :1], t["shs"][:, 1:]))


def forward(R, s, t, model=None):
    """(outputs, state) of one view: of the Gaussians `t`, or with `model` (raw_model(t); the views of one call share the leaf
    tensors) of the one-model scene."""
    if model is not None:
        return R.rasterize_forward_raw(s, None, None, None, None, None, None, None, want_aux=False,
                                       scene=dict(models=[model], scale_noise=None, sh_noise=None, want_act=False))
    return R.rasterize_forward_raw(s, t["means3D"], t["opacities"], t["shs"], None, t["scales"], t["rotations"], None,
                                   want_aux=False)


def views_setup(D, V, radius=3.0):
    """V cameras around the object, one upstream gradient pair per view."""
    from dreamscene_amd import synth
    cams = synth.object_cameras(V + 1, H, W, radius=radius)[1:]
    sets = [settings_for(c, [1, 1, 1], D, DEV) for c in cams]
    ups = [tuple(torch.tensor(x, device=DEV) for x in synth.upstream_grads(H, W, seed=k)) for k in range(V)]
    return sets, [u[0] for u in ups], [u[1] for u in ups]


@pytest.mark.parametrize("scene", [False, True], ids=["plain", "scene"])
@pytest.mark.parametrize("K,D", FORMS)
def test_one_view_through_both_doors(built_lib, K, D, scene):
    """ONE forward state through rasterize_backward_raw (gsr_backward) and through the views function of its kind with a list
    of one (gsr_backward_views): the same leaf gradients and dL_dmeans2D, to the 2e-6 of max|.| that tests/test_scratch.py
    allows between runs that differ in the order of K7's fp32 atomics."""
    from dreamscene_amd import rasterizer as R
    t = gaussians(K)
    sets, gis, gdas = views_setup(D, 1)
    _, st = forward(R, sets[0], t, raw_model(t) if scene else None)
    one = R.rasterize_backward_raw(st, gis[0], gdas[0])
    if scene:
        many = R.rasterize_backward_views_scene_raw([st], gis, gdas)
        pairs = [(f"leaf {j}", a, b) for j, (a, b) in enumerate(zip(one["model_grads"][0], many["model_grads"][0]))]
    else:
        many = R.rasterize_backward_views_raw([st], gis, gdas)
        pairs = [(k, one[k], many[k]) for k in LEAF_GRADS]
    torch.cuda.synchronize()
    assert many["dL_dmeans2D"].shape == (1, P, 3)
    pairs.append(("dL_dmeans2D", one["dL_dmeans2D"], many["dL_dmeans2D"][0]))
    assert sum(float(a.abs().sum()) for _, a, _ in pairs) > 0
    for name, a, b in pairs:
        e = float((a - b).abs().max()) if a.numel() else 0.0
        print(f"[both doors] K={K} {'scene' if scene else 'plain'} {name}: {e / rel_scale(a):.2e} of max|.| = {rel_scale(a):.2e}")
    for name, a, b in pairs:
        assert a.shape == b.shape and tol_ok(b, a, atol=2e-6), name


@pytest.mark.parametrize("stats_views,counted", [(None, [2]), ("all", [0, 1, 2]), ([0], [0])], ids=["last", "all", "first"])
@pytest.mark.parametrize("scene", [False, True], ids=["plain", "scene"])
@pytest.mark.parametrize("K,D", FORMS)
def test_stats_views_counts_the_named_views(built_lib, K, D, scene, stats_views, counted):
    """Densification statistics of a 3-view call (GsrGrads.stat_*, include/gsrast.h), from zeroed tensors: for the views that
    count -- the last one by default -- and their visible Gaussians (radii > 0): denom = how many such views, max_radii2D = the
    largest of their radii (both exact), xyz_gradient_accum = the sum of ||dL_dmeans2D[:2]|| of the call's own per-view
    gradients, to 1e-5 of its largest entry. The eye sits at the rim of the cloud (radius 0.6): every view culls a few
    Gaussians, 22 of the 321 are visible in some views and not in others."""
    from dreamscene_amd import rasterizer as R
    V = 3
    t = gaussians(K)
    sets, gis, gdas = views_setup(D, V, radius=0.6)
    model = raw_model(t) if scene else None
    outs, states = zip(*[forward(R, s, t, model) for s in sets])
    stats = tuple(torch.zeros(P, device=DEV) for _ in range(3))       # (max_radii2D, xyz_gradient_accum, denom)
    door = R.rasterize_backward_views_scene_raw if scene else R.rasterize_backward_views_raw
    o = door(list(states), gis, gdas, stats=stats, stats_views=stats_views)
    torch.cuda.synchronize()
    radii = np.stack([out["radii"].cpu().numpy() for out in outs])
    m2d = o["dL_dmeans2D"].cpu().numpy().astype(np.float64)
    assert radii.shape == (V, P) and m2d.shape == (V, P, 3)
    vis = radii[counted] > 0
    assert vis.any() and not vis.all()
    want_denom = vis.sum(0).astype(np.float32)
    want_maxr = np.where(vis, radii[counted], 0).max(0).astype(np.float32)
    want_accum = (np.sqrt(m2d[counted, :, 0] ** 2 + m2d[counted, :, 1] ** 2) * vis).sum(0)
    maxr, accum, denom = (x.cpu().numpy() for x in stats)
    assert np.array_equal(denom, want_denom)
    assert np.array_equal(maxr, want_maxr)
    assert want_accum.max() > 0
    e = float(np.abs(accum - want_accum).max())
    print(f"[stats_views] K={K} {'scene' if scene else 'plain'} {stats_views}: xyz_gradient_accum {e / rel_scale(want_accum):.2e} "
          f"of max|expected| = {rel_scale(want_accum):.2e}")
    assert e <= 1e-5 * rel_scale(want_accum)
