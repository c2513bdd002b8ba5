"""GPU: the fused photometric loss (dreamscene_amd/photometric.py, csrc/photometric.hip) against torch's fp32 expression and the
float64 helper of tests/photometric_ref.py on the same device and inputs, at the sizes where the kernels can go wrong; then the
borders, the exact cases, half_images, determinism, hipGraph capture, no_grad, and end to end behind GaussianRasterizerViews.

The parity bar (photometric_ref.parity): with e_ref the distance of torch's fp32 expression from float64, the fused result lies
within 4 e_ref + 4 ulp(fp32) of float64, per tensor and relative to its own largest entry, every entry compared."""
import pytest
import torch

from tests import photometric_ref as R
from tests.util import settings_for, small_scene

DEV = torch.device("cuda:0")
TILE = 32                                                   # csrc/photometric.hip kTS
L2 = dict(l2=1.0)
DSSIM = dict(dssim=1.0)
ALL = dict(l2=0.3, l1=0.5, dssim=0.2)
WEIGHTS = {"l2": L2, "dssim": DSSIM, "all": ALL}
# at or under the window; a tile, one under and one past it in either direction; several tiles; many tiles with ragged edges
SIZES = [(1, 1), (5, 7), (11, 11), (TILE, TILE), (TILE - 1, TILE + 1), (TILE + 1, 2 * TILE - 1), (96, 80), (801, 799)]


def fused(xs, ys, g=None, **kw):
    """-> dict(loss [V], terms [V,3], grad: list) of the fused op on a list of views."""
    from dreamscene_amd import photometric as P
    leaves = [x.detach().clone().requires_grad_(True) for x in xs]
    loss, terms = P.photometric_loss(leaves, ys, return_terms=True, **kw)
    g = torch.ones_like(loss) if g is None else g
    grads = torch.autograd.grad(loss, leaves, grad_outputs=g)
    return dict(loss=loss.detach(), terms=terms, grad=list(grads))


def check_parity(xs, ys, g=None, what="", **kw):
    a, r32, r64 = fused(xs, ys, g, **kw), R.torch_loss(xs, ys, g, **kw), R.f64_loss(xs, ys, g, **kw)
    results = [R.parity("loss", a["loss"], r32["loss"], r64["loss"])]
    for k, name in enumerate(("L2", "L1", "D-SSIM")):
        if name == "D-SSIM" and kw.get("dssim", 0.0) == 0.0:                 # not evaluated by either fp32 form
            assert bool(torch.isnan(a["terms"][:, k]).all()) and bool(torch.isnan(r32["terms"][:, k]).all())
            continue
        results.append(R.parity(f"term {name}", a["terms"][:, k], r32["terms"][:, k], r64["terms"][:, k]))
    for v in range(len(xs)):
        results.append(R.parity(f"dL/dx view {v}", a["grad"][v], r32["grad"][v], r64["grad"][v]))
    worst = max(results, key=lambda r: (not r[0], r[1]))
    print("\n".join(f"[{what}] {line}" for _, line in results))
    assert all(ok for ok, _ in results), worst[1]
    return a, r32, r64


def _grad_scale(V, seed):
    return 0.5 + torch.rand(V, generator=torch.Generator().manual_seed(seed)).to(DEV)     # dL/dloss per view


def _size_cases():
    """Every size x channel count x weight set; the view count (1, 4, 17: the chunk boundary), the target dtype and the input
    kind rotate so that each appears with each weight set."""
    cases, i = [], 0
    for (H, W) in SIZES:
        for C in (1, 3):
            for wname in WEIGHTS:
                V = (1, 4, 17)[i % 3] if H * W <= 96 * 80 else (1, 4)[i % 2]
                dtype = (torch.float32, torch.float16)[(i // 3) % 2]
                kind = R.KINDS[(i + i // 5) % len(R.KINDS)]
                cases.append(pytest.param(H, W, C, V, wname, dtype, kind,
                                          id=f"{H}x{W}-C{C}-V{V}-{wname}-{str(dtype)[-7:]}-{kind}"))
                i += 1
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,V,wname,dtype,kind", _size_cases())
def test_parity_over_sizes(built_lib, H, W, C, V, wname, dtype, kind):
    xs, ys = R.make_inputs(kind, V, C, H, W, seed=1, device=DEV, target_dtype=dtype)
    check_parity(xs, ys, _grad_scale(V, H + W), what=f"{H}x{W} C{C} V{V} {wname} {kind}", **WEIGHTS[wname])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["y32", "y16"])
@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("kind", R.KINDS)
def test_parity_over_input_kinds(built_lib, kind, wname, dtype):
    """Every input kind with every weight set and target dtype, one past a tile in either direction, three channels."""
    H, W, V = TILE + 1, 2 * TILE + 1, 4
    xs, ys = R.make_inputs(kind, V, 3, H, W, seed=2, device=DEV, target_dtype=dtype)
    check_parity(xs, ys, _grad_scale(V, 5), what=f"{kind} {wname}", half_images=(dtype == torch.float16), **WEIGHTS[wname])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(17, 33), (TILE + 1, 2 * TILE + 1)])
def test_borders_on_their_own(built_lib, H, W):
    """The 5-pixel frame of dL/dx and its four corners, each as a tensor of its own against float64 (zero padding, the halo)."""
    xs, ys = R.make_inputs("smooth", 2, 3, H, W, seed=3, device=DEV)
    a, r32, r64 = check_parity(xs, ys, what=f"borders {H}x{W}", **DSSIM)
    frame = torch.ones((H, W), dtype=torch.bool, device=DEV)
    frame[5:H - 5, 5:W - 5] = False
    for v in range(2):
        ga, g32, g64 = a["grad"][v], r32["grad"][v], r64["grad"][v]
        ok, line = R.parity("frame", ga[:, frame], g32[:, frame], g64[:, frame])
        print(line)
        assert ok, line
        corners = lambda t: torch.stack([t[:, 0, 0], t[:, 0, -1], t[:, -1, 0], t[:, -1, -1]])   # noqa: E731
        ok, line = R.parity("corners", corners(ga), corners(g32), corners(g64))
        print(line)
        assert ok, line


@pytest.mark.gpu
def test_identical_images_are_exact(built_lib):
    """y = x: ssim_map is 1 (D-SSIM term 0) and every gradient is exactly 0 -- |x-y| has derivative 0 at 0 as torch's abs, and
    the SSIM planes are formed so that their contributions cancel exactly."""
    xs, ys = R.make_inputs("identical", 3, 3, 45, 70, seed=4, device=DEV)
    a, _, _ = check_parity(xs, ys, what="identical dssim", **DSSIM)
    assert bool((a["terms"][:, 2] == 0).all()) and bool((a["loss"] == 0).all())
    for kw in (dict(l1=1.0), DSSIM, ALL):
        r = fused(xs, ys, **kw)
        assert all(bool((q == 0).all()) for q in r["grad"]), kw
        assert bool((r["loss"] == 0).all())


@pytest.mark.gpu
def test_flat_black_is_exact_and_finite(built_lib):
    """x = y = 0: ssim_map == 1 everywhere (C1 C2 / (C1 C2)), so the D-SSIM term is exactly 0; the gradients are finite."""
    xs, ys = R.make_inputs("flat_black", 2, 3, 40, 33, seed=5, device=DEV)
    for kw in (DSSIM, ALL):
        r = fused(xs, ys, **kw)
        assert bool((r["terms"][:, 2] == 0).all()) and bool((r["loss"] == 0).all())
        assert all(bool(torch.isfinite(q).all()) for q in r["grad"])


@pytest.mark.gpu
@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["y32", "y16"])
def test_half_images_is_the_rounded_input(built_lib, wname, dtype):
    """half_images=True equals the fused op fed x.half().float(), bit for bit, forward and gradient (straight through)."""
    xs, ys = R.make_inputs("random", 3, 3, 37, 66, seed=6, device=DEV, target_dtype=dtype)
    g = _grad_scale(3, 9)
    a = fused(xs, ys, g, half_images=True, **WEIGHTS[wname])
    b = fused([x.to(torch.float16).to(torch.float32) for x in xs], ys, g, **WEIGHTS[wname])
    c = fused(xs, ys, g, **WEIGHTS[wname])
    assert R.bits_equal(a["loss"], b["loss"]) and R.bits_equal(torch.nan_to_num(a["terms"]), torch.nan_to_num(b["terms"]))
    assert all(R.bits_equal(u, v) for u, v in zip(a["grad"], b["grad"]))
    assert not R.bits_equal(a["loss"], c["loss"])                        # the rounding is not a no-op on these inputs


@pytest.mark.gpu
def test_eight_runs_give_identical_bits(built_lib):
    xs, ys = R.make_inputs("smooth", 4, 3, 96, 80, seed=7, device=DEV)
    g = _grad_scale(4, 11)
    first = fused(xs, ys, g, **ALL)
    for _ in range(7):
        r = fused(xs, ys, g, **ALL)
        assert R.bits_equal(r["loss"], first["loss"]) and R.bits_equal(r["terms"], first["terms"])
        assert all(R.bits_equal(u, v) for u, v in zip(r["grad"], first["grad"]))


@pytest.mark.gpu
def test_captured_in_a_graph_matches_eager(built_lib):
    """Forward and backward of both forms in one torch.cuda.graph; replays with rewritten images, targets and dL/dloss."""
    from dreamscene_amd import photometric as P
    V, C, H, W = 4, 3, 96, 80
    s_x = [torch.zeros((C, H, W), device=DEV, requires_grad=True) for _ in range(V)]
    s_y = [torch.zeros((C, H, W), device=DEV) for _ in range(V)]
    s_yh = [torch.zeros((C, H, W), device=DEV, dtype=torch.float16) for _ in range(V)]
    s_g = torch.ones((V,), device=DEV)

    def step(x, y, yh, g):
        la = P.photometric_loss(x, y, l1=0.8, dssim=0.2)
        lb = P.photometric_loss(x, yh, l2=1.0, half_images=True)
        ga = torch.autograd.grad(la, x, grad_outputs=g)
        gb = torch.autograd.grad(lb, x, grad_outputs=g)
        return [la, lb] + list(ga) + list(gb)

    def fill(seed):
        xs, ys = R.make_inputs("smooth", V, C, H, W, seed=seed, device=DEV)
        with torch.no_grad():
            for k in range(V):
                s_x[k].copy_(xs[k])
                s_y[k].copy_(ys[k])
                s_yh[k].copy_(ys[k].flip(-1).to(torch.float16))
            s_g.copy_(_grad_scale(V, seed))
        return xs, ys

    fill(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(s_x, s_y, s_yh, s_g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(s_x, s_y, s_yh, s_g)
    for seed in (2, 3):
        xs, ys = fill(seed)
        graph.replay()
        torch.cuda.synchronize()
        eager = step([x.clone().requires_grad_(True) for x in xs], ys, [y.flip(-1).to(torch.float16) for y in ys],
                     _grad_scale(V, seed))
        for u, v in zip(outs, eager):
            assert R.bits_equal(u, v)
        assert float(outs[0].detach().abs().sum()) > 0


@pytest.mark.gpu
def test_no_grad_forward_allocates_no_saved_planes(built_lib):
    from dreamscene_amd import photometric as P
    V, C, H, W = 4, 3, 256, 256
    xs, ys = R.make_inputs("random", V, C, H, W, seed=8, device=DEV)
    planes = 3 * V * C * H * W * 4
    leaves = [x.clone().requires_grad_(True) for x in xs]

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated(DEV) - base

    with_grad, p1 = peak(lambda: P.photometric_loss(leaves, ys, l1=0.8, dssim=0.2))
    with torch.no_grad():
        without, p0 = peak(lambda: P.photometric_loss(leaves, ys, l1=0.8, dssim=0.2))
    detached, p2 = peak(lambda: P.photometric_loss(xs, ys, l1=0.8, dssim=0.2))          # nothing requires a gradient
    assert p1 >= planes and p0 < planes // 8 and p2 < planes // 8, (p1, p0, p2, planes)
    assert not without.requires_grad and R.bits_equal(without, with_grad) and R.bits_equal(detached, with_grad)


# ------------------------------------------------------------------------------------------------------------ end to end
E2E_TOL = 1e-5            # of the tensor's own largest entry: tests/test_views.py's bar


@pytest.mark.gpu
def test_end_to_end_behind_the_rasterizer(built_lib):
    """Two 64x64 views of util.small_scene through GaussianRasterizerViews, 0.8 L1 + 0.2 D-SSIM against seeded targets, backward:
    every leaf gradient against the same pipeline with torch's fp32 expression. Where that pipeline is itself further than the
    bar from a float64 loss feeding the same rasterizer, the 4 e_ref rule takes over for that tensor."""
    from dreamscene_amd import photometric as P, synth
    from dreamscene_amd.views import GaussianRasterizerViews
    V, H, W = 2, 64, 64
    g, _ = small_scene()
    cams = [synth.orbit_camera(5.35, 75.0, 45.0 * i + 10.0, 0.4 + 0.07 * i, H, W) for i in range(V)]
    sets = [settings_for(c, [1.0, 1.0, 1.0], 3, DEV) for c in cams]
    targets = [t for t in torch.rand((V, 3, H, W), generator=torch.Generator().manual_seed(21)).to(DEV)]
    kw = dict(l1=0.8, dssim=0.2)
    names = ("means3D", "shs", "opacities", "scales", "rotations")

    def pipeline(loss_fn):
        t = {k: torch.tensor(v, device=DEV, requires_grad=True) for k, v in g.items()}
        outs = GaussianRasterizerViews(sets)(means3D=t["means3D"], means2D=None, shs=t["shs"], opacities=t["opacities"],
                                             scales=t["scales"], rotations=t["rotations"])
        loss = loss_fn([o[0] for o in outs])
        return float(loss), torch.autograd.grad(loss, [t[n] for n in names])

    def f64(images):
        total = 0
        for x, y in zip(images, targets):
            x, y = x.double(), y.double()
            total = total + 0.8 * torch.abs(x - y).mean() + 0.2 * (1 - R.ssim_map(x, y).mean())
        return total

    la, ga = pipeline(lambda ims: P.photometric_loss(ims, targets, **kw).sum())
    lb, gb = pipeline(lambda ims: torch.stack([R.torch_view(x, y, **kw)[0] for x, y in zip(ims, targets)]).sum())
    lc, gc = pipeline(f64)
    assert abs(la - lb) <= 1e-6 * abs(lb)
    for n, a, b, c in zip(names, ga, gb, gc):
        scale = float(b.abs().max())
        assert scale > 0 and bool(torch.isfinite(a).all())
        d_ab = float((a - b).abs().max()) / scale
        e_ref = float((b - c).abs().max()) / scale
        e_fused = float((a - c).abs().max()) / scale
        print(f"{n}: fused vs torch {d_ab:.3e}, torch vs float64 loss {e_ref:.3e}, fused vs float64 loss {e_fused:.3e}")
        if e_ref <= E2E_TOL:
            assert d_ab <= E2E_TOL, (n, d_ab)
        else:
            assert e_fused <= 4 * e_ref + 4 * R.FP32_ULP, (n, e_fused, e_ref)
