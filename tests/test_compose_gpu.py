"""-m gpu: csrc/compose.hip through dreamscene_amd.compose against tests/compose_ref.py (float64) with DERIVED forward-error bounds,
the box / ground / no-compounding behaviour, the render invariance of a placement on the HIP rasterizer against the fp32 oracle's
own figure for the same pair, the scene pipeline and graph capture. Every test runs under its own time limit."""
import ctypes
import faulthandler

import numpy as np
import pytest
import torch

from tests import compose_ref as CR
from tests.test_compose import CASE_Q, CASE_T

U = 2.0 ** -24                       # fp32 unit roundoff
TEST_SECONDS = 420


@pytest.fixture(autouse=True)
def _time_limit():
    """A hung kernel does not return to Python: the watchdog thread ends the process with a traceback instead."""
    faulthandler.dump_traceback_later(TEST_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def random_leaves(P, K, seed, dev="cpu"):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    lv = (r(P, 3), -3.0 + 0.5 * r(P, 3), r(P, 4), 1.5 * r(P, 1), r(P, 1, 3), 0.3 * r(P, K - 1, 3))
    return tuple(t.to(dev).contiguous() for t in lv)


def assert_within(out, ref, mag, n, what):
    """|out - ref64| <= (n + 2) u sum|terms| for EVERY entry: n products, each rounded once, summed in sequence (at most n more
    roundings on any term, the last add of the translation included); no outliers."""
    out = out.detach().cpu().double()
    bound = (n + 2) * U * mag
    over = (out - ref).abs() > bound
    worst = float(((out - ref).abs() / bound.clamp_min(1e-300)).max()) if out.numel() else 0.0
    print(f"[place vs ref] {what}: worst error {worst:.3f} of its bound")
    assert not bool(over.any()), f"{what}: {int(over.sum())} entries beyond (n+2) u sum|terms|, worst {worst:.3f} of the bound"


GENERIC_Q = (0.9, -0.35, 0.2, 0.55)                       # not normalised on purpose
CENTER = (1.25, -0.75, 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 255, 256, 257, 100_003])
@pytest.mark.parametrize("K", [1, 4, 9, 16])
def test_kernel_matches_the_float64_definition(built_lib, K, P):
    from dreamscene_amd import compose
    dev = torch.device("cuda:0")
    cpu = random_leaves(P, K, seed=1000 * K + P)
    model = tuple(t.to(dev) for t in cpu)
    keep = tuple(t.clone() for t in model)
    for scale in ([1.0], [0.37], [0.5, 1.0, 2.0]):
        for ground in (True, False):
            what = f"K={K} P={P} scale={scale} ground={ground}"
            po = compose.place(model, GENERIC_Q, scale, CENTER, ground=ground)
            po2 = compose.place(model, GENERIC_Q, scale, CENTER, ground=ground)
            torch.cuda.synchronize()
            for a, b in zip(model, keep):
                assert torch.equal(a, b), what + ": the model was written"
            for name, a, b in zip(compose.LEAVES, po, po2):
                assert torch.equal(a, b), f"{what}: two runs differ in {name}"
                assert a.is_leaf and not a.requires_grad
            assert torch.equal(po.bbox, po2.bbox) and torch.equal(po.t_effective, po2.t_effective)
            assert torch.equal(po._opacity, model[3]) and torch.equal(po._features_dc, model[4])
            assert po._opacity.data_ptr() != model[3].data_ptr()
            c32 = compose.placement_constants(GENERIC_Q, scale, CENTER)
            assert torch.equal(po._scaling.cpu(), cpu[1] + torch.tensor(c32.log_scale)[None, :]), what + ": scaling bits"
            c = CR.constants(GENERIC_Q, scale, CENTER)
            ref = CR.place_ref(cpu[0], cpu[1], cpu[2], cpu[5], c, ground=ground, t_effective=po.t_effective.cpu())
            assert_within(po._xyz, ref["xyz"], ref["mag_xyz"], 3, what + " xyz")
            assert_within(po._rotation, ref["rotation"], ref["mag_rotation"], 4, what + " rotation")
            fr = po._features_rest
            assert fr.shape == model[5].shape
            for first, n, _ in CR.BANDS:
                if K - 1 >= first + n:
                    assert_within(fr[:, first:first + n], ref["f_rest"][:, first:first + n], ref["mag_f_rest"][:, first:first + n],
                                  n, f"{what} band {n}")
            # the box: the bits of amin / amax of what was written
            assert torch.equal(po.bbox, torch.cat((po._xyz.amin(0), po._xyz.amax(0)))), what + ": bbox"
            # T: the centre; with ground one fp32 subtraction of the minimum of fl32(R S x).z, which a placement at the origin shows
            te = po.t_effective.cpu()
            assert te[0] == np.float32(CENTER[0]) and te[1] == np.float32(CENTER[1])
            if ground:
                zmin = compose.place(model, GENERIC_Q, scale, (0, 0, 0), ground=False).bbox[2].cpu()
                assert te[2] == torch.tensor(CENTER[2], dtype=torch.float32) - zmin, what + ": t_effective"
                low = float(po._xyz[:, 2].min())
                ulp = 2.0 ** -23 * max(abs(CENTER[2]), abs(float(zmin)))
                print(f"[place ground] {what}: lowest z {low!r} for centre z {CENTER[2]}, {abs(low - CENTER[2]) / ulp:.2f} ulp")
                assert abs(low - CENTER[2]) <= 2 * ulp, what + ": the object does not stand on center.z"
                # the float64 definition's own T agrees up to the error of the minimum and the subtraction
                t64 = CR.place_ref(cpu[0], cpu[1], cpu[2], cpu[5], c, ground=True)["t_effective"]
                assert abs(float(te[2]) - float(t64[2])) <= 5 * U * float(ref["mag_xyz"][:, 2].max())
            else:
                assert te[2] == np.float32(CENTER[2])


@pytest.mark.gpu
def test_copy_false_shares_the_untouched_storage_and_models_work(built_lib):
    from dreamscene_amd import compose

    class M:
        pass
    dev = torch.device("cuda:0")
    m = M()
    for n, t in zip(compose.LEAVES, random_leaves(300, 16, 4, dev)):
        setattr(m, n, torch.nn.Parameter(t))
    m.max_radii2D, m.xyz_gradient_accum, m.denom = torch.rand(300, device=dev), torch.rand(300, device=dev), torch.ones(300, device=dev)
    a = compose.place(m, (10, 20, 30), [1.0], (0, 0, 0), copy=False)
    b = compose.place(m, (10, 20, 30), [1.0], (0, 0, 0), copy=True)
    assert a._opacity.data_ptr() == m._opacity.data_ptr() and a._features_dc.data_ptr() == m._features_dc.data_ptr()
    assert b._opacity.data_ptr() != m._opacity.data_ptr() and torch.equal(b._opacity, m._opacity)
    assert a.stats[0].data_ptr() == m.max_radii2D.data_ptr() and torch.equal(b.stats[2], m.denom)
    for x, y in zip(a, b):
        assert torch.equal(x, y) and not x.requires_grad
    assert a.affine["T"] is a.t_effective and a.affine["R"].tolist() == [10.0, 20.0, 30.0] and a.affine["S"].tolist() == [1.0]
    leaves, stats = compose.combine([a, b])
    assert leaves[0].shape == (600, 3) and torch.equal(leaves[5][300:], b._features_rest) and stats[1].shape == (600,)
    assert compose.combine([tuple(a), b])[1] is None


@pytest.mark.gpu
def test_placing_an_object_twice_does_not_compound(built_lib):
    from dreamscene_amd import compose
    dev = torch.device("cuda:0")
    model = random_leaves(5000, 16, 8, dev)
    other = random_leaves(700, 16, 9, dev)
    keep = tuple(t.clone() for t in model)
    p1 = dict(rotation=(0.0, 0.0, 90.0), scale=[1.2], center=[3.0, 1.0, 0.0])
    p2 = dict(rotation=list(GENERIC_Q), scale=[0.5, 1.0, 2.0], center=[-4.0, 2.0, 0.25])
    start = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    placed, box = compose.add_objects_to_scene([(model, [p1, p2]), (other, [p1])], scene_box=start)
    assert len(placed) == 3 and box.device.type == "cuda"
    for po, (m, prm) in zip(placed, ((model, p1), (model, p2), (other, p1))):
        single = compose.place(m, prm["rotation"], prm["scale"], prm["center"])
        for name, a, b in zip(compose.LEAVES, po, single):
            assert torch.equal(a, b), name
        assert torch.equal(po.bbox, single.bbox)
    for a, b in zip(model, keep):
        assert torch.equal(a, b)
    assert p1["center"] == [3.0, 1.0, 0.0]                      # the reference subtracts z_min from the caller's list
    boxes = torch.stack([po.bbox for po in placed] + [start.to(dev)])
    assert torch.equal(box, torch.cat((boxes[:, :3].amin(0), boxes[:, 3:].amax(0))))
    _, box2 = compose.add_objects_to_scene([(model, [p1, p2])])
    assert torch.equal(box2, torch.cat((torch.minimum(placed[0].bbox[:3], placed[1].bbox[:3]),
                                        torch.maximum(placed[0].bbox[3:], placed[1].bbox[3:]))))


# ---- the render invariance on the HIP rasterizer ---------------------------------------------------------------------------------

def _seeded_q(seed):
    return tuple(float(v) for v in np.random.default_rng(seed).normal(size=4))


# a similarity p' = s R p + t and the scene it is tried on. At C2 size (100 k Gaussians @512^2: ~2e4 saturated pixels, each with a
# transmittance that crosses T_MIN somewhere in a stack of hundreds) the fp32 oracle ALONE takes a gate differently, or swaps two
# Gaussians of nearly equal depth at the end of a pixel's list, on a few pixels for most placements: with the translation of the
# small case 8 ... 23 of 262 144 pixels change n_contrib for every one of 400 seeded rotations (radii never differ). The error
# that flips them grows with |p'|, so the C2 placements use a small translation (exact in fp32) and seeded rotations for which
# the oracle alone holds, found by search on the CPU oracle: seed 69 of 92 tried at scale 1. At scale 1.7 none of 750 seeded
# rotations passed at C2 size (1 ... 10 pixels each), so the similarity with a scale is tried on the small scene only.
C2_T = (0.125, -0.25, 0.0625)
SIM_CASES = {
    "case400": dict(P=400, seed=3, res=64, n_cams=4, cam_idx=1, rotation=CASE_Q, scale=1.0, t=CASE_T),
    "case400_scaled": dict(P=400, seed=3, res=64, n_cams=4, cam_idx=1, rotation=CASE_Q, scale=1.7, t=CASE_T),
    "c2": dict(P=100_000, seed=1, res=512, n_cams=1, cam_idx=0, rotation=_seeded_q(69), scale=1.0, t=C2_T),
}


def sim_scene(P, seed, res, n_cams, cam_idx, **_):
    """fp32 raw leaves (numpy, scene.LEAVES order) of synth's G-object, and the camera."""
    from dreamscene_amd import synth
    g = synth.g_object(P, seed=seed, K=16)
    raw = CR.raw_leaves(g)
    leaves = tuple(np.ascontiguousarray(raw[k], dtype=np.float32) for k in ("xyz", "scaling", "rotation", "opacity", "f_dc", "f_rest"))
    return leaves, synth.object_cameras(n_cams, res, res)[cam_idx]


def activate(leaves) -> dict:
    """GaussianModel's activations (gs_renderer.py:464-488) in fp32 torch, on whatever device the leaves are."""
    xyz, scaling, rot, opacity, f_dc, f_rest = (torch.as_tensor(t) for t in leaves)
    return dict(means3D=xyz, scales=torch.exp(scaling), rotations=torch.nn.functional.normalize(rot),
                opacities=torch.sigmoid(opacity), shs=torch.cat((f_dc, f_rest), dim=1).contiguous())


def oracle_pair_c(CO, P, seed, res, n_cams, cam_idx, rotation, scale, t) -> dict:
    """The fp32 C oracle on (object, camera) and on (object placed by the float64 definition and rounded to fp32, moved camera):
    a, b = its outputs; near_margin = the least |z / 0.2 - 1| of a view-space depth in either configuration."""
    leaves, cam = sim_scene(P, seed, res, n_cams, cam_idx)
    c = CR.constants(rotation, [scale], t)
    ref = CR.place_ref(leaves[0], leaves[1], leaves[2], leaves[5], c, ground=False)
    placed = (ref["xyz"].float().numpy(), ref["scaling64"].float().numpy(), ref["rotation"].float().numpy(), leaves[3], leaves[4],
              ref["f_rest"].float().numpy())
    moved = CR.moved_camera(cam, rotation, scale, np.asarray(c["t"]))
    views = (dict(viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center), moved)
    outs, margin = [], np.inf
    for lv, v in zip((leaves, placed), views):
        act = {k: x.numpy() for k, x in activate(lv).items()}
        ov = CO.make_view(P, 16, 3, res, res, cam.tanfovx, cam.tanfovy, [1, 1, 1], v["viewmatrix"], v["projmatrix"], v["campos"])
        outs.append(CO.forward(ov, act["means3D"], act["opacities"], shs=act["shs"], scales=act["scales"], rotations=act["rotations"],
                               omp=P > 10_000))
        z = act["means3D"].astype(np.float64) @ np.asarray(v["viewmatrix"], dtype=np.float64)[:3, 2] + float(v["viewmatrix"][3][2])
        margin = min(margin, float(np.abs(z / 0.2 - 1.0).min()))
    return dict(a=outs[0], b=outs[1], near_margin=margin, cam=cam, leaves=leaves, moved=moved)


def _hip_render(leaves_dev, cam, view, dev):
    from dreamscene_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)
    s = GaussianRasterizationSettings(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, t([1, 1, 1]), 1.0,
                                      t(view["viewmatrix"]), t(view["projmatrix"]), 3, t(view["campos"]), False, False)
    a = activate(leaves_dev)
    with torch.no_grad():
        img, radii, da = GaussianRasterizer(raster_settings=s)(
            means3D=a["means3D"], means2D=torch.zeros_like(a["means3D"]), shs=a["shs"], colors_precomp=None,
            opacities=a["opacities"], scales=a["scales"], rotations=a["rotations"], cov3D_precomp=None)
    return img.cpu().numpy(), radii.cpu().numpy(), da.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIM_CASES))
def test_placed_object_renders_the_same_on_the_hip_rasterizer(built_lib, c_oracle, name):
    """HIP render of the object == HIP render of compose.place's output from the moved camera: equal radii, image and depth_alpha
    within 4x what the fp32 oracle itself shows for the pair (two independent fp32 evaluation orders on each side). First the
    oracle alone: no hard gate may flip between the two configurations, and nothing may sit on the near plane."""
    from dreamscene_amd import compose
    from tests.test_compose import invariance_pair
    case = SIM_CASES[name]
    dev = torch.device("cuda:0")
    o = oracle_pair_c(c_oracle, **case)
    flips = (int((o["a"]["radii"] != o["b"]["radii"]).sum()), int((o["a"]["n_contrib"] != o["b"]["n_contrib"]).sum()))
    f_img = float(np.abs(o["a"]["image"] - o["b"]["image"]).max())
    f_da = float(np.abs(o["a"]["depth_alpha"] - o["b"]["depth_alpha"]).max())
    print(f"[invariance {name}] fp32 C oracle alone: image {f_img:.2e}, depth_alpha {f_da:.2e}; radii differing {flips[0]}, "
          f"n_contrib differing {flips[1]}; nearest to the near plane {o['near_margin']:.3f}")
    if case["P"] <= 1000:
        # the small case also on the torch oracle in fp32, the figure the issue quotes (7.7e-7 / 5.0e-6 at scale 1)
        from dreamscene_amd import synth
        g = synth.g_object(case["P"], seed=case["seed"], K=16)
        a32, b32 = invariance_pair(g, o["cam"], case["rotation"], case["scale"], case["t"], torch.float32, renormalise=False)
        print(f"[invariance {name}] torch oracle fp32: image {np.abs(a32[0] - b32[0]).max():.2e}, "
              f"depth_alpha {np.abs(a32[2] - b32[2]).max():.2e}")
    # measure first, assert afterwards: the log holds every figure whichever assertion fails
    model = tuple(torch.as_tensor(x, device=dev) for x in o["leaves"])
    po = compose.place(model, case["rotation"], [case["scale"]], case["t"], ground=False)
    view = dict(viewmatrix=o["cam"].world_view_transform, projmatrix=o["cam"].full_proj_transform, campos=o["cam"].camera_center)
    img_a, radii_a, da_a = _hip_render(model, o["cam"], view, dev)
    img_b, radii_b, da_b = _hip_render(tuple(po), o["cam"], o["moved"], dev)
    e_img, e_da = float(np.abs(img_a - img_b).max()), float(np.abs(da_a - da_b).max())
    print(f"[invariance {name}] HIP: image {e_img:.2e}, depth_alpha {e_da:.2e}; radii differing {int((radii_a != radii_b).sum())}")
    assert o["near_margin"] > 0.01, f"{name}: a Gaussian within 1 % of the near plane ({o['near_margin']:.4f})"
    assert flips == (0, 0), f"{name}: the oracle alone takes a hard gate differently (radii, n_contrib) = {flips}"
    assert int((o["a"]["radii"] > 0).sum()) >= case["P"] // 2
    assert np.array_equal(radii_a, radii_b)
    assert e_img <= 4 * f_img and e_da <= 4 * f_da


# ---- the pipeline and capture ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_placed_object_in_the_scene_pipeline(built_lib, c_oracle):
    """compose.place's output and a second model through scene's fused multi-model path == the oracle on the concatenated
    activated tensors, at the bar of tests/test_scene.py::test_fused_scene_vs_oracle."""
    from dreamscene_amd import compose, rasterizer as R, scene, synth
    from tests.test_scene import _random_models
    from tests.util import oracle_view, settings_for, tol_ok
    CO = c_oracle
    dev = torch.device("cuda:0")
    K, D, H, W = 16, 3, 112, 96
    a, b = _random_models([700, 257], K, 21, dev)
    po = compose.place(tuple(t.detach() for t in a), (15.0, -30.0, 70.0), [0.8], (0.3, -0.2, -0.4))
    models = [po, tuple(t.detach() for t in b)]
    P = 957
    cam = synth.object_cameras(2, H, W, radius=3.0)[1]
    bg = [0.3, 0.6, 0.9]
    s = settings_for(cam, bg, D, dev)
    out, _ = R.rasterize_forward_raw(s, None, None, None, None, None, None, None,
                                     scene=dict(models=models, scale_noise=None, sh_noise=None, want_act=True))
    cat = [torch.cat([m[k] for m in models]) for k in range(6)]
    ov = oracle_view(CO, cam, P, K, D, bg)
    ref = CO.forward(ov, cat[0].cpu().numpy(), out["act_opacities"].cpu().numpy(), shs=torch.cat((cat[4], cat[5]), 1).cpu().numpy(),
                     scales=out["act_scales"].cpu().numpy(), rotations=out["act_rotations"].cpu().numpy())
    assert int((ref["radii"] > 0).sum()) > 600
    assert np.array_equal(out["radii"].cpu().numpy(), ref["radii"])
    assert tol_ok(out["color"].cpu().numpy(), ref["image"])
    assert tol_ok(out["depth_alpha"].cpu().numpy(), ref["depth_alpha"])
    np.testing.assert_allclose(out["act_scales"].cpu().numpy(), torch.exp(cat[1]).cpu().numpy(), rtol=4e-7)
    img, radii, da, scales = scene.rasterize_models(s, models, torch.zeros((P, 3), device=dev))
    assert np.array_equal(radii.cpu().numpy(), ref["radii"])
    assert tol_ok(img.cpu().numpy(), ref["image"]) and tol_ok(da.cpu().numpy(), ref["depth_alpha"])


@pytest.mark.gpu
def test_gsr_place_replays_from_a_captured_graph(built_lib):
    from dreamscene_amd import _lib, compose
    lib = built_lib
    dev = torch.device("cuda:0")
    P, K = 30_001, 16
    model = random_leaves(P, K, 12, dev)
    eager = compose.place(model, GENERIC_Q, [0.5, 1.0, 2.0], CENTER)
    c = compose.placement_constants(GENERIC_Q, [0.5, 1.0, 2.0], CENTER)
    outs = [torch.zeros_like(model[k]) for k in (0, 1, 2, 5)]
    box = torch.zeros(12, device=dev)
    nbytes = lib.gsr_place_scratch_bytes(P)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    p = _lib.GsrPlacement()
    p.P, p.K, p.ground = P, K, 1
    p.xyz, p.scaling, p.rotation, p.opacity, p.features_dc, p.features_rest = (t.data_ptr() for t in model)
    p.xyz_out, p.scaling_out, p.rotation_out, p.features_rest_out = (t.data_ptr() for t in outs)
    for name in c._fields:
        getattr(p, name)[:] = getattr(c, name).tolist()
    p.bounds, p.t_effective = box.data_ptr(), box.data_ptr() + 32
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.gsr_place(ctypes.byref(p), scratch.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    for _ in range(2):
        for t in outs + [box]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, k in zip(outs, (0, 1, 2, 5)):
            assert torch.equal(a, eager[k])
        assert torch.equal(box[:6], eager.bbox) and torch.equal(box[8:11], eager.t_effective)
