"""-m gpu: camera and settings space. tests/test_fuzz.py and the parity suite move in Gaussian space under three orbit poses
(no roll, tanfov < 1, tanfovy tied to tanfovx by the reference's rule, scale_modifier 1.0); here the Gaussians stay ordinary and
the camera rolls, looks past the object from anywhere on a sphere, fovx and fovy take 0.2 ... 2.2 independently, and
scale_modifier takes 0.25 ... 3 -- through every form of K1 / K8: single view, precomputed covariance, batched views (dense,
sparse, per-view scales), the scene table and the captured step. Same bars as the suites these forms already have
(TOL, CAM_GRAD_SLACK, bit-exact integer artefacts), held against the C oracle, which tests/test_oracle_consistency.py holds
against float64 autograd on the same seeds."""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import _check_forward, _grad_check, _run_hip
from tests.test_k8_sparse import D as D_B, H as H_B, K as K_B, P as P_B, W as W_B, _scene, assert_every_kind_of_block
from tests.util import (CAMERA_FUZZ_SEEDS, err, oracle_view, random_camera, random_settings_config, rel_scale, settings_for,
                        tol_ok)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def _report(what, rep):
    print(f"[{what}] " + " ".join(f"{k} {e / max(m, 1e-30):.1e}" for k, (e, m) in rep.items()))


# ------------------------------------------------------------------------------------------------------------- (a) single view
@pytest.mark.parametrize("seed", CAMERA_FUZZ_SEEDS)
def test_single_view(built_lib, c_oracle, seed):
    g, cam, bg, P, K, D, mod = random_settings_config(seed)
    out, _ = _run_hip(g, cam, bg, D, scale_modifier=mod)
    v = oracle_view(c_oracle, cam, P, K, D, bg, scale_modifier=mod)
    f = c_oracle.forward(v, g["means3D"], g["opacities"], shs=g["shs"], scales=g["scales"], rotations=g["rotations"])
    _check_forward(out, f, P)
    _report(f"single view, seed {seed}", _grad_check(g, cam, bg, D, c_oracle, seed=seed, tol=1e-5, scale_modifier=mod))


# ------------------------------------------------------------------------------------------- (b) precomputed covariance / colours
@pytest.mark.parametrize("seed", [0, 3, 5, 7, 8, 15])
def test_precomputed_inputs(built_lib, c_oracle, seed):
    """cov3D_precomp = what the reference hands over as get_covariance(scaling_modifier): the modifier is already inside, and
    the settings carry the same modifier -- which must not be applied a second time (SEMANTICS.md section 3)."""
    from oracle import torch_oracle as TO
    g, cam, bg, P, K, D, mod = random_settings_config(seed)
    assert mod != 1.0 and P >= 65
    cov = TO.cov3d_from_scale_rot(torch.tensor(g["scales"]), mod, torch.tensor(g["rotations"])).numpy().astype(np.float32)
    g2 = dict(means3D=g["means3D"], opacities=g["opacities"], cov3D_precomp=cov,
              colors_precomp=np.random.default_rng(seed).uniform(size=(P, 3)).astype(np.float32))
    out, _ = _run_hip(g2, cam, bg, 0, scale_modifier=mod)
    v = oracle_view(c_oracle, cam, P, 0, 0, bg, scale_modifier=mod)
    f = c_oracle.forward(v, g2["means3D"], g2["opacities"], colors_precomp=g2["colors_precomp"], cov3D_precomp=cov)
    # the same Gaussians through scales + rotations + the modifier: the same footprints (one rounding apart at the most)
    f_sr = c_oracle.forward(v, g["means3D"], g["opacities"], colors_precomp=g2["colors_precomp"], scales=g["scales"],
                            rotations=g["rotations"])
    assert np.abs(f["radii"].astype(np.int64) - f_sr["radii"]).max() <= 1 and int((f["radii"] > 0).sum()) >= 16
    _check_forward(out, f, P)
    rep = _grad_check(g2, cam, bg, 0, c_oracle, seed=seed, tol=1e-5, scale_modifier=mod)
    assert "dL_dcov3D" in rep and "dL_dcolors" in rep
    _report(f"precomputed inputs, seed {seed}", rep)


# ------------------------------------------------------------------------------------------------------------ (c) batched views
PVS_FACTORS = (1.0, 1.01, 0.99, 1.02)
# (V, scale_modifier, form, seed of the cameras); the seeds are chosen so that every case reaches all three kinds of workgroup
BATCHED_CASES = [(1, 1.7, "sparse", 2), (2, 0.5, "sparse", 0), (4, 1.7, "sparse", 0),
                 (1, 0.5, "pvs", 2), (2, 1.7, "pvs", 0), (4, 0.5, "pvs", 0)]


def _batched_cameras(seed, V):
    rng = np.random.default_rng(7000 + seed)
    return [random_camera(rng, H_B, W_B) for _ in range(V)]


def _batched_oracle(c_oracle, g, cams, bg, ups, mod, pvs):
    names = ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dshs")
    ref = {k: 0.0 for k in names}
    per_view, reached = [], np.zeros(P_B, bool)
    for j, (cam, (gi, gda)) in enumerate(zip(cams, ups)):
        sc = (g["scales"] * np.float32(PVS_FACTORS[j])).astype(np.float32) if pvs else g["scales"]
        v = oracle_view(c_oracle, cam, P_B, K_B, D_B, bg, scale_modifier=mod)
        f = c_oracle.forward(v, g["means3D"], g["opacities"], shs=g["shs"], scales=sc, rotations=g["rotations"])
        b = c_oracle.backward(v, f, gi, gda, g["means3D"], shs=g["shs"], scales=sc, rotations=g["rotations"])
        for k in names:
            ref[k] = ref[k] + np.asarray(b[k], dtype=np.float64)
        per_view.append((f, b))
        reached |= (np.abs(np.asarray(b["dL_dopacity"]).reshape(P_B, -1)).sum(1) +
                    np.abs(np.asarray(b["dL_dshs"]).reshape(P_B, -1)).sum(1)) > 0
    return ref, per_view, reached


@pytest.mark.parametrize("V,mod,form,cam_seed", BATCHED_CASES)
def test_batched_views(built_lib, c_oracle, V, mod, form, cam_seed):
    """GaussianRasterizerViews into a GradArena: parameter gradients = the sum of the per-view C-oracle gradients. `sparse`:
    the opacity pattern of test_k8_sparse (full, mixed and unreached workgroups side by side); `pvs`: scales [V,P,3], every
    view's scale gradient against its own oracle view. Two calls: the first projects view by view (no pair-count hint yet),
    the second through the batched K1."""
    from dreamscene_amd import multiview, rasterizer as R, synth
    from dreamscene_amd.views import GaussianRasterizerViews
    pvs = form == "pvs"
    g = _scene()
    cams = _batched_cameras(cam_seed, V)
    bg = np.array([0.1, 0.3, 0.9], np.float32)
    ups = [synth.upstream_grads(H_B, W_B, seed=k) for k in range(V)]
    ref, per_view, reached = _batched_oracle(c_oracle, g, cams, bg, ups, mod, pvs)
    assert_every_kind_of_block(reached)      # (under the kernel's real layout: tests/k8_layout.py)
    dev = torch.device(DEV)
    t = {k: torch.tensor(v, device=DEV) for k, v in g.items()}
    sets = [settings_for(c, bg, D_B, dev, scale_modifier=mod) for c in cams]
    up_t = [torch.tensor(y, device=dev) for k in range(V) for y in ups[k]]
    for call in range(2):
        arena = multiview.GradArena(P_B, K_B, dev)
        arena.flat.fill_(-3.0 - call)              # stale contents: the call must overwrite every row it owns
        tt = {k: v.clone().requires_grad_(True) for k, v in t.items()}
        if pvs:
            tt["scales"] = (t["scales"].unsqueeze(0) * torch.tensor(PVS_FACTORS[:V], device=dev).view(V, 1, 1)).requires_grad_(True)
        rast = GaussianRasterizerViews(sets, context=R.RasterContext(grad_arena=arena))
        m2d = torch.zeros((V, P_B, 3), device=dev, requires_grad=True)
        outs = rast(means3D=tt["means3D"], means2D=m2d, shs=tt["shs"], opacities=tt["opacities"], scales=tt["scales"],
                    rotations=tt["rotations"])
        grads = torch.autograd.grad([x for (img, _, da) in outs for x in (img, da)], [m2d] + ([tt["scales"]] if pvs else []),
                                    up_t)
        torch.cuda.synchronize()
        for j, ((img, radii, da), (f, b)) in enumerate(zip(outs, per_view)):
            assert np.array_equal(radii.cpu().numpy(), f["radii"]), (call, j)
            assert err(img.detach().cpu().numpy(), f["image"]) <= TOL, (call, j)
            assert err(da.detach().cpu().numpy(), f["depth_alpha"]) <= TOL * rel_scale(f["depth_alpha"]), (call, j)
            a, r = grads[0][j].cpu().numpy().reshape(-1), np.asarray(b["dL_dmeans2D"]).reshape(-1)
            assert err(a, r) <= TOL * rel_scale(r), ("dL_dmeans2D", call, j, err(a, r) / rel_scale(r))
            if pvs:
                a, r = grads[1][j].cpu().numpy().reshape(-1), np.asarray(b["dL_dscales"]).reshape(-1)
                assert err(a, r) <= TOL * rel_scale(r), ("dL_dscales of the view", call, j, err(a, r) / rel_scale(r))
        for ak, rk in [("means3D", "dL_dmeans3D"), ("rotations", "dL_drotations"), ("opacities", "dL_dopacity"),
                       ("shs", "dL_dshs")] + ([] if pvs else [("scales", "dL_dscales")]):
            a, r = arena.views[ak].cpu().numpy().reshape(-1), np.asarray(ref[rk]).reshape(-1)
            print(f"[batched V {V} mod {mod} {form} call {call}] {ak} {err(a, r) / rel_scale(r):.1e}")
            assert err(a, r) <= TOL * rel_scale(r), (ak, call)


# --------------------------------------------------------------------------------------------------------------- (d) scene form
def _two_models(dev):
    """Raw leaves (the way test_epilogue.test_densify_stats_fused_into_backward makes them) of two models side by side."""
    from dreamscene_amd import synth
    models = []
    for mi, (n, seed, off) in enumerate([(300, 9, -0.25), (257, 10, 0.3)]):
        g = synth.g_object(n, seed=seed, K=16)
        op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
        raw = (g["means3D"] * 0.8 + np.array([[off, 0.1 * mi, 0.0]], np.float32), np.log(g["scales"] * 4.0),
               g["rotations"] * (0.7 + 0.6 * mi), np.log(op / (1 - op)), g["shs"][:, :1], g["shs"][:, 1:])
        models.append(tuple(torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev, requires_grad=True)
                            for a in raw))
    return models


def test_scene_form(built_lib):
    """scene.rasterize_models / rasterize_models_views (raw leaves of two models into K1 / K8) with scale_modifier 1.7 under
    rolled cameras, against the C oracle fed with the activations the kernel exported and chained to the raw leaves by autograd
    through oracle/scene_oracle.py -- the scheme and the bars of test_scene.test_fused_scene_vs_oracle."""
    from dreamscene_amd import rasterizer as R, scene, synth
    from oracle import c_oracle as CO, scene_oracle as SO
    from tests.test_scene import LEAVES
    dev = torch.device(DEV)
    K, D, H, W, V, mod = 16, 3, 88, 104, 2, 1.7
    models = _two_models(dev)
    leaves = [t for m in models for t in m]
    P = sum(int(m[0].shape[0]) for m in models)
    rng = np.random.default_rng(7100)
    cams = [random_camera(rng, H, W) for _ in range(V)]
    bg = [0.3, 0.6, 0.9]
    sets = [settings_for(c, bg, D, dev, scale_modifier=mod) for c in cams]
    ups = [synth.upstream_grads(H, W, seed=4 + k) for k in range(V)]
    gen = torch.Generator().manual_seed(5)
    gss = [torch.randn((P, 3), generator=gen) * 1e-3 for _ in range(V)]
    # the activations as the kernel computes them (exp / sigmoid differ by an ulp between libm and the GPU)
    out, _ = R.rasterize_forward_raw(sets[0], None, None, None, None, None, None, None,
                                     scene=dict(models=models, scale_noise=None, sh_noise=None, want_act=True))
    cpu_models = [tuple(t.detach().cpu().requires_grad_(True) for t in m) for m in models]
    a = SO.activate_and_cat(cpu_models)
    np.testing.assert_allclose(out["act_scales"].cpu().numpy(), a["scales"].detach().numpy(), rtol=4e-7)
    np.testing.assert_allclose(out["act_rotations"].cpu().numpy(), a["rotations"].detach().numpy(), rtol=0, atol=2.5e-7)
    np.testing.assert_allclose(out["act_opacities"].cpu().numpy(), a["opacities"].detach().numpy().reshape(-1), rtol=4e-7)
    act = dict(means3D=a["means3D"].detach().numpy(), shs=a["shs"].detach().numpy(), scales=out["act_scales"].cpu().numpy(),
               rotations=out["act_rotations"].cpu().numpy(), opacities=out["act_opacities"].cpu().numpy())

    def oracle(k):
        ov = oracle_view(CO, cams[k], P, K, D, bg, scale_modifier=mod)
        f = CO.forward(ov, act["means3D"], act["opacities"], shs=act["shs"], scales=act["scales"], rotations=act["rotations"])
        b = CO.backward(ov, f, ups[k][0], ups[k][1], act["means3D"], shs=act["shs"], scales=act["scales"],
                        rotations=act["rotations"])
        assert int((f["radii"] > 0).sum()) >= 64 and f["N"] >= 1000, (k, f["N"])
        return f, b

    def leaf_grads(bs, gs_sum):
        """Autograd through the oracle glue: dL/d(activated inputs) summed over the views -> dL/d(raw leaves)."""
        for row in cpu_models:
            for t in row:
                t.grad = None
        s = lambda key: torch.tensor(sum(np.asarray(b[key], dtype=np.float64) for b in bs).astype(np.float32))
        torch.autograd.backward(
            [a["means3D"], a["scales"], a["rotations"], a["opacities"], a["shs"]],
            [s("dL_dmeans3D"), s("dL_dscales") + gs_sum, s("dL_drotations"), s("dL_dopacity").reshape(a["opacities"].shape),
             s("dL_dshs")], retain_graph=True)
        return [t.grad.numpy().copy() if t.grad is not None else np.zeros(t.shape, np.float32) for row in cpu_models for t in row]

    def loss_of(outs):
        return sum((img * torch.tensor(ups[k][0], device=dev)).sum() + (da * torch.tensor(ups[k][1], device=dev)).sum() +
                   (sc * gss[k].to(dev)).sum() for k, (img, _, da, sc) in outs)

    def compare(what, got_leaves, ref_leaves):
        for i, (hg, rg) in enumerate(zip(got_leaves, ref_leaves)):
            name = f"{what}: model {i // 6} {LEAVES[i % 6]}"
            print(f"[scene form] {name} {err(hg.cpu().numpy(), rg) / rel_scale(rg):.1e}")
            assert tol_ok(hg.cpu().numpy(), rg), name

    refs = [oracle(k) for k in range(V)]
    # one view at a time
    for k in range(V):
        f, b = refs[k]
        m2d = torch.zeros((P, 3), device=dev, requires_grad=True)
        img, radii, da, sc = scene.rasterize_models(sets[k], models, m2d)
        grads = torch.autograd.grad(loss_of([(k, (img, radii, da, sc))]), leaves + [m2d])
        assert np.array_equal(radii.cpu().numpy(), f["radii"])
        assert torch.equal(sc, out["act_scales"])             # the scales handed back carry no modifier
        assert tol_ok(img.detach().cpu().numpy(), f["image"]) and tol_ok(da.detach().cpu().numpy(), f["depth_alpha"])
        assert tol_ok(grads[-1].cpu().numpy(), b["dL_dmeans2D"]), f"view {k}: dL_dmeans2D"
        compare(f"view {k}", grads[:-1], leaf_grads([b], gss[k]))
    # both views through one call (the first call of this (P, H, W) still projects view by view: no hint yet)
    ref_sum = leaf_grads([b for _, b in refs], gss[0] + gss[1])
    for call in range(2):
        m2d = torch.zeros((V, P, 3), device=dev, requires_grad=True)
        outs = scene.rasterize_models_views(sets, models, m2d)
        grads = torch.autograd.grad(loss_of(list(enumerate(outs))), leaves + [m2d])
        for k, ((img, radii, da, sc), (f, b)) in enumerate(zip(outs, refs)):
            assert np.array_equal(radii.cpu().numpy(), f["radii"]), (call, k)
            assert tol_ok(img.detach().cpu().numpy(), f["image"]) and tol_ok(da.detach().cpu().numpy(), f["depth_alpha"])
            assert tol_ok(grads[-1][k].cpu().numpy(), b["dL_dmeans2D"]), f"call {call} view {k}: dL_dmeans2D"
        compare(f"views call {call}", grads[:-1], ref_sum)


# ------------------------------------------------------------------------------------------------------------ (e) captured step
def test_captured_step_follows_fov_and_roll(built_lib):
    """graph.CapturedViews: captured under one camera set, replayed under one whose tanfovx, tanfovy, roll and SH degree all
    differ (the packed camera block is rewritten, nothing else): outputs and gradients are the eager call's, bit for bit.
    Another scale_modifier is baked into the captured structs: it must force a new capture, not a stale replay."""
    from dreamscene_amd import synth
    from dreamscene_amd.graph import CapturedViews, WARM_CALLS
    from tests.test_graph import _eager, _setup
    V, P, H, W, K = 2, 1500, 96, 112, 16
    g, t = _setup(P, H, W, K, seed=19, scale_mul=1.5)
    leaves = [t[k] for k in ("means3D", "shs", "opacities", "scales", "rotations")]
    gis = [torch.tensor(synth.upstream_grads(H, W, seed=k)[0], device=DEV) for k in range(V)]
    gdas = [torch.tensor(synth.upstream_grads(H, W, seed=k)[1], device=DEV) for k in range(V)]
    orbit = synth.object_cameras(V, H, W, radius=3.0)                 # what the capture is made under: no roll, tanfov 0.23
    rng = np.random.default_rng(7220)
    rolled = [random_camera(rng, H, W) for _ in range(V)]
    for a, b in zip(orbit, rolled):                                   # (tanfov 1.96 x 0.23 and 0.10 x 0.12)
        assert abs(a.tanfovx - b.tanfovx) > 1e-3 and abs(a.tanfovy - b.tanfovy) > 1e-3
    rast = CapturedViews()

    def step(cams, D, mod, what):
        sets = [settings_for(c, [0.2, 0.4, 0.9], D, DEV, scale_modifier=mod) for c in cams]
        ref_outs, ref_grads = _eager(sets, t, gis, gdas)
        m2d = torch.zeros((V, P, 3), device=DEV, requires_grad=True)
        outs = rast(sets, means3D=t["means3D"], means2D=m2d, opacities=t["opacities"], shs=t["shs"], scales=t["scales"],
                    rotations=t["rotations"])
        grads = torch.autograd.grad([x for (img, _, da) in outs for x in (img, da)], leaves + [m2d],
                                    [y for k in range(V) for y in (gis[k], gdas[k])])
        torch.cuda.synchronize()
        for (img, radii, da), (rimg, rradii, rda) in zip(outs, ref_outs):
            assert int((radii > 0).sum()) >= 64, what
            assert torch.equal(radii, rradii), what
            assert torch.equal(img, rimg) and torch.equal(da, rda), what
        for name, x, y in zip(("means3D", "shs", "opacities", "scales", "rotations", "means2D"), grads, ref_grads):
            d = (x.reshape(y.shape) - y).abs().max().item()
            print(f"[captured, {what}] dL/d{name}: max |captured - eager| {d:.3e} (max|eager| {y.abs().max().item():.3e})")
            assert torch.equal(x.reshape(y.shape), y), (what, name, d)

    for k in range(WARM_CALLS):
        step(orbit, 3, 1.0, f"eager warm-up {k}")
    step(orbit, 3, 1.0, "capture")
    assert rast.stats["captures"] == 1 and rast.stats["replays"] == 1 and rast.stats["eager_steps"] == WARM_CALLS, rast.stats
    step(rolled, 1, 1.0, "replay: rolled cameras, other tanfovx / tanfovy / SH degree")
    assert rast.stats["captures"] == 1 and rast.stats["replays"] == 2 and rast.stats["overflows"] == 0, rast.stats
    step(rolled, 1, 1.7, "scale_modifier 1.7")
    assert rast.stats["captures"] == 2 and rast.stats["replays"] == 3 and rast.stats["overflows"] == 0, rast.stats
    step(orbit, 3, 1.7, "replay of the second capture")
    assert rast.stats["captures"] == 2 and rast.stats["replays"] == 4 and rast.stats["overflows"] == 0, rast.stats
