"""GPU: the glue ops' kernels (csrc/glue.hip through dreamscene_amd/glue.py) against torch's glue on the same device, the float64
helper, themselves (determinism, hipGraph capture), and inside object_render / scene_render (fused_disp=True)."""
import numpy as np
import pytest
import torch

from tests.glue_ref import (bits_equal, disp_f64, random_planes, tie_planes, torch_disp, torch_tv, tv_f64, tv_grad_f64)
from tests.util import settings_for, small_scene

DEV = torch.device("cuda:0")


def _render_depth_alpha(cams, P=600, seed=3):
    """depth_alpha [2,H,W] of util.small_scene rendered by the rasterizer, one per camera."""
    from dreamscene_amd.rasterizer import GaussianRasterizer
    g, _ = small_scene(P=P, seed=seed, scale_mul=1.0)
    t = {k: torch.tensor(v, device=DEV) for k, v in g.items()}
    out = []
    for cam in cams:
        _, _, da = GaussianRasterizer(raster_settings=settings_for(cam, [1.0, 1.0, 1.0], 3, DEV))(
            means3D=t["means3D"], means2D=None, shs=t["shs"], opacities=t["opacities"], scales=t["scales"],
            rotations=t["rotations"])
        out.append(da.detach().contiguous())
    return out


def _cams(n, H, W):
    from dreamscene_amd import synth
    return [synth.orbit_camera(5.35, 75.0, 45.0 * i + 10.0, 0.4 + 0.07 * i, H, W) for i in range(n)]


# ------------------------------------------------------------------------------------------------------ 1. forward bits
@pytest.mark.gpu
@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("HW", [(96, 80), (801, 799), (1024, 1024)])
def test_disp_forward_bits_random_planes(built_lib, V, HW):
    from dreamscene_amd import glue
    H, W = HW
    planes = random_planes(V, H, W, seed=11 + V, device=DEV)
    fovs = [0.35 + 0.1 * k for k in range(V)]
    if V == 4:
        planes[2][1] += 0.11                  # one view without a masked pixel (the fallback)
    d, a = glue.disp_from_depth_alpha(planes if V > 1 else planes[0], fovs if V > 1 else fovs[0])
    for k in range(V):
        rd, ra = torch_disp(planes[k], fovs[k])
        gd, ga = (d[k], a[k]) if V > 1 else (d, a)
        assert bits_equal(gd, rd), (k, float((gd - rd).abs().max()))
        assert bits_equal(ga, ra)


@pytest.mark.gpu
@pytest.mark.parametrize("HW", [(96, 80), (801, 799)])
def test_disp_forward_bits_rendered(built_lib, HW):
    from dreamscene_amd import glue
    H, W = HW
    cams = _cams(4, H, W)
    das = _render_depth_alpha(cams)
    print(f"[{H}x{W}] masked fraction per view: " + ", ".join(f"{float((da[1] <= 0.1).float().mean()):.3f}" for da in das))
    d, a = glue.disp_from_depth_alpha(das, [c.FoVx for c in cams])
    for k, (da, c) in enumerate(zip(das, cams)):
        rd, ra = torch_disp(da, c.FoVx)
        assert bits_equal(d[k], rd) and bits_equal(a[k], ra), k
        d1, a1 = glue.disp_from_depth_alpha(da, c.FoVx)
        assert d1.shape == (1, H, W) and bits_equal(d1, rd) and bits_equal(a1, ra)


# ------------------------------------------------------------------------------------------------------- 2. edge cases
def _edge_plane(case, H=64, W=48):
    da = random_planes(1, H, W, seed=21)[0]
    if case == "no_masked_pixel":
        da[1] = da[1] * 0.5 + 0.5
    elif case == "alpha_at_0.1":                        # exactly one masked pixel, alpha = float32(0.1)
        da[1] = da[1] * 0.5 + 0.5
        da[1, 7, 9] = float(np.float32(0.1))
        da[0, 7, 9] = 9.0                               # u = 10 + 1e-5, inside the unmasked pixels' range [5.5, 15.5)
    elif case == "ties":                                # 9 masked pixels tied at the min + one equal pixel outside; 4 at the max
        tie_planes(da)
    elif case == "flat":
        da.zero_()
    return da.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["no_masked_pixel", "alpha_at_0.1", "ties", "flat"])
def test_disp_edge_cases_against_torch_autograd(built_lib, case):
    from dreamscene_amd import glue
    da = _edge_plane(case)
    fovx = 0.5
    gen = torch.Generator(device=DEV).manual_seed(3)
    g = torch.rand((1,) + tuple(da.shape[1:]), device=DEV, generator=gen)
    ga = torch.rand((1,) + tuple(da.shape[1:]), device=DEV, generator=gen)
    x1, x2 = da.clone().requires_grad_(True), da.clone().requires_grad_(True)
    d1, a1 = glue.disp_from_depth_alpha(x1, fovx)
    d2, a2 = torch_disp(x2, fovx)
    assert bits_equal(d1, d2) and bits_equal(a1, a2)
    torch.autograd.backward([d1, a1], [g, ga])
    torch.autograd.backward([d2, a2], [g, ga])
    h = disp_f64(da, fovx, g.cpu().numpy(), ga.cpu().numpy())
    if case == "flat":
        assert torch.isnan(d1).all() and torch.isnan(x1.grad[0]).all() and torch.isnan(x2.grad[0]).all()
        return
    if case == "alpha_at_0.1":
        assert h["masked"] and h["tie_m"].sum() == 1 and h["tie_m"][7, 9] and h["M"] > h["m"]
    if case == "ties":
        assert h["tie_m"].sum() == 9 and h["tie_M"].sum() == 4 and not h["tie_m"][5, 5]
    ref = h["grad"]
    scale = float(np.abs(ref).max())
    e_hip = float(np.abs(x1.grad.cpu().numpy() - ref).max())
    e_torch = float(np.abs(x2.grad.cpu().numpy() - ref).max())
    e_vs_torch = float((x1.grad - x2.grad).abs().max())
    print(f"[{case}] |hip - f64| {e_hip / scale:.1e}, |torch - f64| {e_torch / scale:.1e}, |hip - torch| {e_vs_torch / scale:.1e}"
          " of max|ref|")
    assert e_hip <= 1e-6 * scale
    assert e_vs_torch <= 1e-5 * scale            # the tie shares are torch's (an unshared share would be off by ~scale)


# -------------------------------------------------------------------------------------------------------- 3. backward
@pytest.mark.gpu
@pytest.mark.parametrize("HW", [(801, 799), (1024, 1024)])
def test_disp_backward_against_f64(built_lib, HW):
    from dreamscene_amd import glue
    H, W = HW
    V = 4
    planes = random_planes(V, H, W, seed=31, device=DEV)
    planes[3][1] += 0.11
    fovs = [0.4, 0.45, 0.5, 0.55]
    gen = torch.Generator(device=DEV).manual_seed(5)
    g = torch.randn((V, 1, H, W), device=DEV, generator=gen)
    ga = torch.randn((V, 1, H, W), device=DEV, generator=gen)
    xs = [p.clone().requires_grad_(True) for p in planes]
    d, a = glue.disp_from_depth_alpha(xs, fovs)
    torch.autograd.backward([d, a], [g, ga])
    for k in range(V):
        h = disp_f64(planes[k], fovs[k], g[k].cpu().numpy(), ga[k].cpu().numpy())
        ref = h["grad"]
        y = planes[k].clone().requires_grad_(True)
        d2, a2 = torch_disp(y, fovs[k])
        torch.autograd.backward([d2, a2], [g[k], ga[k]])
        scale = float(np.abs(ref).max())
        e_hip = float(np.abs(xs[k].grad.cpu().numpy() - ref).max())
        e_torch = float(np.abs(y.grad.cpu().numpy() - ref).max())
        print(f"[{H}x{W} view {k}] |hip - f64| {e_hip / scale:.2e}, |torch fp32 - f64| {e_torch / scale:.2e} of max|ref|")
        assert e_hip <= 1e-6 * scale, (k, e_hip / scale)
        assert e_hip <= e_torch, (k, e_hip, e_torch)


# -------------------------------------------------------------------------------------------------------------- 4. TV
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 3, 1024, 1024), (4, 1, 1024, 1024), (1, 1, 2, 2), (2, 3, 37, 51), (3, 2, 5, 3),
                                   (1, 2, 9, 8)])
def test_tv_against_f64(built_lib, shape):
    from dreamscene_amd import glue
    x = torch.rand(shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    for unaligned in (False, True):
        if unaligned:                              # a 4-byte offset: the scalar path of the kernels
            buf = torch.empty(x.numel() + 1, device=DEV)
            buf[1:] = x.reshape(-1)
            xi = buf[1:].view(shape)
        else:
            xi = x.clone()
        xi.requires_grad_(True)
        loss = glue.tv_loss(xi)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        loss.backward(torch.tensor(0.7, device=DEV))
        ref = tv_f64(x)
        assert abs(float(loss) - ref) <= 1e-6 * abs(ref), (float(loss), ref)
        gref = tv_grad_f64(x, 0.7)
        e = float(np.abs(xi.grad.cpu().numpy() - gref).max())
        assert e <= 1e-6 * float(np.abs(gref).max()), e
        lt = torch_tv(x)                                                      # torch's own fp32 value, for the record
        assert abs(float(lt) - ref) <= 1e-4 * abs(ref)


# ------------------------------------------------------------------------------------------------------ 5. determinism
@pytest.mark.gpu
def test_glue_is_deterministic(built_lib):
    from dreamscene_amd import glue
    H = W = 1024
    planes = random_planes(4, H, W, seed=41, device=DEV)
    imgs = torch.rand((4, 3, H, W), device=DEV)
    fovs = [0.4, 0.5, 0.6, 0.7]
    gen = torch.Generator(device=DEV).manual_seed(6)
    g = torch.randn((4, 1, H, W), device=DEV, generator=gen)

    def run():
        xs = [p.clone().requires_grad_(True) for p in planes]
        im = imgs.clone().requires_grad_(True)
        d, a = glue.disp_from_depth_alpha(xs, fovs)
        loss = glue.tv_loss(im) + glue.tv_loss(d) + (d * g).sum()
        loss.backward()
        return [d, a, loss] + [x.grad for x in xs] + [im.grad]
    r1, r2 = run(), run()
    for u, v in zip(r1, r2):
        assert bits_equal(u, v)


# ------------------------------------------------------------------------------------------------------------ 6. capture
@pytest.mark.gpu
def test_glue_captured_in_a_graph_matches_eager(built_lib):
    from dreamscene_amd import glue
    V, H, W = 4, 256, 192
    fovs = [0.4, 0.5, 0.6, 0.7]
    static = [torch.zeros((2, H, W), device=DEV, requires_grad=True) for _ in range(V)]
    static_img = torch.zeros((V, 3, H, W), device=DEV, requires_grad=True)

    def step(planes, img):
        d, a = glue.disp_from_depth_alpha(planes, fovs)
        loss = glue.tv_loss(img) + glue.tv_loss(d) + glue.tv_loss(a)
        grads = torch.autograd.grad(loss, list(planes) + [img])
        return [d, a, loss] + list(grads)

    def fill(seed):
        ps = random_planes(V, H, W, seed=seed, device=DEV)
        im = torch.rand((V, 3, H, W), generator=torch.Generator().manual_seed(seed)).to(DEV)
        return ps, im

    ps, im = fill(1)
    with torch.no_grad():
        for s, p in zip(static, ps):
            s.copy_(p)
        static_img.copy_(im)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(static, static_img)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(static, static_img)
    for seed in (2, 3):
        ps, im = fill(seed)
        ps[seed % V][1] += 0.11                           # a view whose mask is empty in this replay only
        with torch.no_grad():
            for s, p in zip(static, ps):
                s.copy_(p)
            static_img.copy_(im)
        graph.replay()
        torch.cuda.synchronize()
        eager = step([p.clone().requires_grad_(True) for p in ps], im.clone().requires_grad_(True))
        for u, v in zip(outs, eager):
            assert bits_equal(u, v)
        for k in range(V):
            assert bits_equal(outs[0][k], torch_disp(ps[k], fovs[k])[0])


# -------------------------------------------------------------------------------------------------------------- 7. views
@pytest.mark.gpu
def test_rasterizer_views_outputs_go_in_without_a_stack(built_lib):
    from dreamscene_amd import glue
    from dreamscene_amd.views import GaussianRasterizerViews
    V, H, W = 4, 96, 80
    g, _ = small_scene()
    t = {k: torch.tensor(v, device=DEV, requires_grad=True) for k, v in g.items()}
    cams = _cams(V, H, W)
    sets = [settings_for(c, [1.0, 1.0, 1.0], 3, DEV) for c in cams]
    fovs = [c.FoVx for c in cams]
    gen = torch.Generator(device=DEV).manual_seed(8)
    gd = torch.randn((V, 1, H, W), device=DEV, generator=gen)

    def render():
        return GaussianRasterizerViews(sets)(means3D=t["means3D"], means2D=None, shs=t["shs"], opacities=t["opacities"],
                                             scales=t["scales"], rotations=t["rotations"])
    outs = render()
    das = [o[2] for o in outs]
    d, a = glue.disp_from_depth_alpha(das, fovs)
    gr1 = torch.autograd.grad((d * gd).sum() + (a * gd).sum(), das, retain_graph=True)
    singles = [glue.disp_from_depth_alpha(da, f) for da, f in zip(das, fovs)]
    d2, a2 = torch.stack([s[0] for s in singles]), torch.stack([s[1] for s in singles])
    gr2 = torch.autograd.grad((d2 * gd).sum() + (a2 * gd).sum(), das, retain_graph=True)
    assert bits_equal(d, d2) and bits_equal(a, a2)
    for u, v in zip(gr1, gr2):
        assert bits_equal(u, v)
    leaf = torch.autograd.grad((d * gd).sum(), [t["means3D"], t["opacities"]])      # and on through the rasterizer's backward
    assert all(bool(torch.isfinite(x).all()) for x in leaf)


# -------------------------------------------------------------------------------------------------------- 8. integration
E2E_GRAD_TOL = 4e-4      # SEMANTICS.md "end to end through the reference's glue" (tests/test_golden.py)


def _params(g, D=3):
    from dreamscene_amd.render_api import GaussianParams
    op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV, requires_grad=True)
    return GaussianParams(t(g["means3D"]), t(np.log(g["scales"])), t(g["rotations"]), t(np.log(op / (1 - op))),
                          t(g["shs"][:, :1]), t(g["shs"][:, 1:]), D)


@pytest.mark.gpu
def test_object_render_fused_disp(built_lib):
    from dreamscene_amd import render_api
    g, cam = small_scene()
    bg = torch.tensor([1.0, 1.0, 1.0], device=DEV)
    res = []
    for fused in (False, True):
        p = _params(g)
        out = render_api.object_render(p, cam, bg, fused_disp=fused)
        gi = torch.randn(out["image"].shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        gd = torch.randn(out["depth"].shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
        ga = torch.randn(out["alpha"].shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
        ((out["image"] * gi).sum() + (out["depth"] * gd).sum() + (out["alpha"] * ga).sum()).backward()
        res.append((out, p))
    (o0, p0), (o1, p1) = res
    assert o1["depth"].shape == o0["depth"].shape == (1, cam.image_height, cam.image_width)
    assert bits_equal(o1["depth"], o0["depth"]) and bits_equal(o1["alpha"], o0["alpha"])
    assert bits_equal(o1["image"], o0["image"])
    worst = {}
    for name, a, b in [("viewspace_points", o0["viewspace_points"].grad, o1["viewspace_points"].grad)] + \
            [(n, getattr(p0, n).grad, getattr(p1, n).grad) for n in ("_xyz", "_scaling", "_rotation", "_opacity",
                                                                     "_features_dc", "_features_rest")]:
        scale = max(1e-12, float(a.abs().max()))
        worst[name] = float((a - b).abs().max()) / scale
    print("object_render fused_disp=True vs False, leaf gradient difference / max|ref|: "
          + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, e in worst.items():
        assert e <= E2E_GRAD_TOL, (k, e)


@pytest.mark.gpu
def test_scene_render_fused_disp(built_lib):
    from dreamscene_amd import scene
    g, cam = small_scene()
    bg = torch.tensor([1.0, 1.0, 1.0], device=DEV)
    outs = []
    for fused in (False, True):
        p = _params(g)
        model = (p._xyz, p._scaling, p._rotation, p._opacity, p._features_dc, p._features_rest)
        out = scene.scene_render([model], cam, bg, 3, test=True, fused_disp=fused)
        gd = torch.randn(out["depth"].shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
        ((out["image"]).sum() + (out["depth"] * gd).sum()).backward()
        outs.append((out, p))
    (o0, p0), (o1, p1) = outs
    assert bits_equal(o1["depth"], o0["depth"]) and bits_equal(o1["alpha"], o0["alpha"])
    for n in ("_xyz", "_opacity", "_features_dc"):
        a, b = getattr(p0, n).grad, getattr(p1, n).grad
        assert float((a - b).abs().max()) <= E2E_GRAD_TOL * max(1e-12, float(a.abs().max())), n
