"""CPU: the glue ops' interface (dreamscene_amd/glue.py) -- argument errors, the CPU path against the reference's expressions bit
for bit, the float64 helper's selections, and the C ABI's host-side checks (no GPU needed)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.glue_ref import bits_equal, disp_f64, random_planes, tie_planes, torch_disp, torch_tv, tv_f64, tv_grad_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_errors():
    from dreamscene_amd import glue
    da = torch.rand(2, 8, 6)
    with pytest.raises(ValueError):
        glue.disp_from_depth_alpha(torch.rand(3, 8, 6), 0.5)            # not [2,H,W]
    with pytest.raises(ValueError):
        glue.disp_from_depth_alpha(torch.rand(8, 6), 0.5)
    with pytest.raises(TypeError):
        glue.disp_from_depth_alpha(da.double(), 0.5)                    # not fp32
    with pytest.raises(ValueError, match="same image size"):
        glue.disp_from_depth_alpha([da, torch.rand(2, 6, 8)], 0.5)       # mixed sizes
    with pytest.raises(ValueError):
        glue.disp_from_depth_alpha([da, da], [0.5])                     # one fovx for two views
    with pytest.raises(ValueError):
        glue.disp_from_depth_alpha(da, [0.5, 0.6])
    with pytest.raises(ValueError):
        glue.disp_from_depth_alpha([], 0.5)
    with pytest.raises(ValueError):
        glue.tv_loss(torch.rand(1, 1, 1, 5))                            # H < 2
    with pytest.raises(ValueError):
        glue.tv_loss(torch.rand(1, 1, 5, 1))                            # W < 2
    with pytest.raises(ValueError):
        glue.tv_loss(torch.rand(3, 5, 5))                               # not [B,C,H,W]
    with pytest.raises(TypeError):
        glue.tv_loss(torch.rand(1, 1, 5, 5, dtype=torch.float64))


@pytest.mark.parametrize("case", ["random", "no_masked_pixel", "flat"])
def test_cpu_disp_is_the_reference_expression(case):
    """The CPU path is the reference's expression: the same bits, the try / except fallback included (an empty mask raises in
    .min() and the global minimum is used), the same gradients."""
    from dreamscene_amd import glue
    da = random_planes(1, 33, 29, seed=4)[0]
    if case == "no_masked_pixel":
        da[1] = da[1] * 0.5 + 0.5
    elif case == "flat":
        da.zero_()
    a = da.clone().requires_grad_(True)
    b = da.clone().requires_grad_(True)
    d1, al1 = glue.disp_from_depth_alpha(a, 0.61)
    d2, al2 = torch_disp(b, 0.61)
    assert d1.shape == (1, 33, 29) and al1.shape == (1, 33, 29)
    assert bits_equal(d1, d2) and bits_equal(al1, al2)
    if case == "flat":
        assert torch.isnan(d1).all()
    g = torch.rand_like(d1)
    ga = torch.rand_like(al1)
    (d1 * g).sum().add((al1 * ga).sum()).backward()
    (d2 * g).sum().add((al2 * ga).sum()).backward()
    assert bits_equal(a.grad, b.grad)


def test_cpu_disp_list_of_views():
    from dreamscene_amd import glue
    planes = random_planes(3, 17, 21, seed=5)
    planes[1][1] += 0.2                        # view 1: no masked pixel
    fovs = [0.4, 0.5, 0.6]
    d, al = glue.disp_from_depth_alpha(planes, fovs)
    assert d.shape == (3, 1, 17, 21) and al.shape == (3, 1, 17, 21)
    for k in range(3):
        rd, ra = torch_disp(planes[k], fovs[k])
        assert bits_equal(d[k], rd) and bits_equal(al[k], ra)
    d1, _ = glue.disp_from_depth_alpha(planes, 0.5)                     # one fovx for every view
    assert bits_equal(d1[1], torch_disp(planes[1], 0.5)[0])


@pytest.mark.parametrize("shape", [(4, 3, 16, 20), (1, 1, 2, 2), (2, 3, 7, 5)])
def test_cpu_tv_is_the_reference_expression(shape):
    from dreamscene_amd import glue
    x = torch.rand(shape, generator=torch.Generator().manual_seed(2))
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    la, lb = glue.tv_loss(a), torch_tv(b)
    assert la.dim() == 0 and bits_equal(la, lb)
    la.backward()
    lb.backward()
    assert bits_equal(a.grad, b.grad)
    assert abs(float(la.detach()) - tv_f64(x)) <= 1e-5 * tv_f64(x)
    assert np.abs(a.grad.numpy() - tv_grad_f64(x)).max() <= 1e-5 * np.abs(tv_grad_f64(x)).max()


@pytest.mark.parametrize("case", ["random", "no_masked_pixel", "ties"])
def test_f64_helper_reproduces_the_glue_selections(case):
    """The float64 helper forms d in fp32 exactly as torch does: its m, M, mask flag and tie sets are the torch glue's, and its
    disp rounds to within an ulp of torch's; its gradient is torch's (CPU autograd) up to fp32 rounding."""
    da = random_planes(1, 40, 31, seed=7)[0]
    if case == "no_masked_pixel":
        da[1] = da[1] * 0.5 + 0.5
    elif case == "ties":
        tie_planes(da)
    fovx = 0.55
    depth, alpha = da[0], da[1]
    disp = (1 / (2 * math.tan(fovx / 2))) / (depth + alpha * 10 + 1e-5)
    mask = alpha <= 0.1
    m_t = float(disp[mask].min()) if bool(mask.any()) else float(disp.min())
    h = disp_f64(da, fovx)
    assert np.float32(h["m"]) == np.float32(m_t) and np.float32(h["M"]) == np.float32(float(disp.max()))
    assert np.array_equal(h["d32"], disp.numpy())
    assert h["masked"] == bool(mask.any())
    if case == "ties":
        assert h["tie_m"].sum() == 9 and h["tie_M"].sum() == 4 and not h["tie_m"][5, 5] and h["d32"][5, 5] == np.float32(h["m"])
    ref, _ = torch_disp(da, fovx)
    assert np.abs(np.float32(h["disp"]) - ref[0].numpy()).max() <= 4e-7
    g = torch.rand((1,) + tuple(da.shape[1:]), generator=torch.Generator().manual_seed(1))
    ga = torch.rand_like(g)
    x = da.clone().requires_grad_(True)
    d2, a2 = torch_disp(x, fovx)
    torch.autograd.backward([d2, a2], [g, ga])
    hg = disp_f64(da, fovx, g.numpy(), ga.numpy())["grad"]
    assert np.abs(x.grad.numpy() - hg).max() <= 1e-4 * np.abs(hg).max()


def test_abi_host_checks(built_lib):
    """The glue entry points refuse bad shapes before touching the device, and GsrDispViews has the C layout."""
    from dreamscene_amd import _lib
    lib = built_lib
    assert lib.gsr_disp_scratch_bytes(0, 8, 8) == 0 and lib.gsr_disp_scratch_bytes(_lib.GSR_MAX_DISP_VIEWS + 1, 8, 8) == 0
    assert lib.gsr_disp_scratch_bytes(4, 1024, 1024) >= 4 * 256 * 32
    assert lib.gsr_disp_scratch_bytes(1, 1, 1) % 256 == 0
    assert lib.gsr_tv_scratch_bytes(1, 1, 1, 8) == 0 and lib.gsr_tv_scratch_bytes(1, 1, 8, 1) == 0
    assert lib.gsr_tv_scratch_bytes(4, 3, 1024, 1024) >= 2048 * 16
    assert lib.gsr_disp_forward(None, None, None, None, None, 0, None) == -1
    assert lib.gsr_disp_backward(None, None, None, None, None, 0, None) == -1
    t = _lib.GsrDispViews()
    t.n_views, t.height, t.width = 0, 8, 8
    assert lib.gsr_disp_forward(ctypes.byref(t), 16, 16, 16, 256, 4096, None) == -1    # no views
    t.n_views = 1                                                                     # a view without a plane
    assert lib.gsr_disp_forward(ctypes.byref(t), 16, 16, 16, 256, 4096, None) == -1
    assert lib.gsr_tv_forward(16, 1, 1, 1, 4, 16, 256, 4096, None) == -1               # H < 2
    assert lib.gsr_tv_backward(16, 1, 1, 4, 1, 16, 16, None) == -1                     # W < 2
    assert lib.gsr_tv_forward(16, 1, 1, 4, 4, 16, 256, 0, None) == -4                  # scratch too small
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "gsrast.h"
    int main(){ printf("%zu %zu %zu %zu %d %d\n", sizeof(GsrDispViews), offsetof(GsrDispViews, depth_alpha),
                       offsetof(GsrDispViews, dL_ddepth_alpha), offsetof(GsrDispViews, focal), GSR_MAX_DISP_VIEWS,
                       GSR_DISP_STATS_FLOATS); return 0; }
    '''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    V = _lib.GsrDispViews
    assert got == [ctypes.sizeof(V), V.depth_alpha.offset, V.dL_ddepth_alpha.offset, V.focal.offset, _lib.GSR_MAX_DISP_VIEWS,
                   _lib.GSR_DISP_STATS_FLOATS]


def test_glue_kernels_in_the_fat_binary(built_lib):
    from dreamscene_amd import _lib
    out = subprocess.run(["strings", "-n", "6", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_disp_reduce", "k_disp_apply", "k_disp_bsum", "k_disp_bapply", "k_tv_partial", "k_tv_final", "k_tv_bwd"):
        assert k in out, k


def test_render_glue_defaults_unchanged():
    """fused_disp is opt-in: the defaults of object_render and scene_render leave the reference's glue in place."""
    import inspect
    from dreamscene_amd import render_api, scene
    assert inspect.signature(render_api.object_render).parameters["fused_disp"].default is False
    assert inspect.signature(scene.scene_render).parameters["fused_disp"].default is False
