"""CPU: the frame export's interface (dreamscene_amd/frames.py) -- the C layout of GsrFrameViews and the host-side checks of the
entry points, the argument errors (raised before any launch), and a self-check of the crafted inputs of tests/test_frames_gpu.py,
so that the GPU tests cannot pass vacuously."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import frames_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_and_host_checks(built_lib):
    from dreamscene_amd import _lib
    lib = built_lib
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "gsrast.h"
    int main(){ printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(GsrFrameViews), offsetof(GsrFrameViews, n_views),
                       offsetof(GsrFrameViews, height), offsetof(GsrFrameViews, width), offsetof(GsrFrameViews, image),
                       offsetof(GsrFrameViews, depth_alpha), GSR_MAX_FRAME_VIEWS); return 0; }
    '''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    T = _lib.GsrFrameViews
    assert got == [ctypes.sizeof(T), T.n_views.offset, T.height.offset, T.width.offset, T.image.offset, T.depth_alpha.offset,
                   _lib.GSR_MAX_FRAME_VIEWS]
    # shapes
    assert lib.gsr_frames_scratch_bytes(0, 8, 8) == 0 and lib.gsr_frames_scratch_bytes(_lib.GSR_MAX_FRAME_VIEWS + 1, 8, 8) == 0
    assert lib.gsr_frames_scratch_bytes(1, 0, 8) == 0 and lib.gsr_frames_scratch_bytes(1, 1 << 16, 1 << 16) == 0
    assert lib.gsr_frames_scratch_bytes(1, 1, 1) == 256
    assert lib.gsr_frames_scratch_bytes(16, 1024, 1024) >= 16 * 256 * 4
    # refusals before any HIP call (the pointers are never dereferenced)
    assert lib.gsr_frames_quantize(None, 16, 16, 256, 4096, None) == -1
    t = T()
    t.n_views, t.height, t.width = 0, 8, 8
    assert lib.gsr_frames_quantize(ctypes.byref(t), 16, None, None, 0, None) == -1        # no views
    t.n_views = 2
    t.image[0] = 256
    assert lib.gsr_frames_quantize(ctypes.byref(t), 16, None, None, 0, None) == -1        # view 1 has no image
    t.image[1] = 512
    assert lib.gsr_frames_quantize(ctypes.byref(t), None, None, None, 0, None) == -1      # no output
    assert lib.gsr_frames_quantize(ctypes.byref(t), 16, 16, 256, 4096, None) == -1        # depth wanted, no depth_alpha
    t.depth_alpha[0], t.depth_alpha[1] = 1024, 2048
    assert lib.gsr_frames_quantize(ctypes.byref(t), 16, 16, None, 0, None) == -1          # depth wanted, no scratch
    assert lib.gsr_frames_quantize(ctypes.byref(t), 16, 16, 256, 0, None) == -4           # scratch too small
    t.image[1] = 514
    assert lib.gsr_frames_quantize(ctypes.byref(t), 16, None, None, 0, None) == -1        # a plane that is no float pointer


def test_kernels_in_the_fat_binary(built_lib):
    from dreamscene_amd import _lib
    out = subprocess.run(["strings", "-n", "6", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_frames_max", "k_frames_quant"):
        assert k in out, k


def _settings(H=8, W=8, score_flag=False):
    from dreamscene_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                         scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                         campos=torch.zeros(3), prefiltered=False, score_flag=score_flag)


def test_render_frames_argument_errors():
    from dreamscene_amd import frames
    from dreamscene_amd._lib import GsrError
    g = dict(means3D=torch.zeros(4, 3), opacities=torch.zeros(4, 1), shs=torch.zeros(4, 1, 3), scales=torch.zeros(4, 3),
             rotations=torch.zeros(4, 4))
    two = [_settings(), _settings()]
    with pytest.raises(ValueError, match="chunk"):
        frames.render_frames(two, chunk=0, **g)
    with pytest.raises(ValueError, match="chunk"):
        frames.render_frames(two, chunk=-3, **g)
    with pytest.raises(ValueError, match="same image size"):
        frames.render_frames([_settings(8, 8), _settings(8, 16)], **g)
    with pytest.raises(ValueError, match="score_flag"):
        frames.render_frames([_settings(), _settings(score_flag=True)], **g)
    with pytest.raises(ValueError, match="no views"):
        frames.render_frames([], **g)
    ok_d = torch.empty((2, 8, 8, 1), dtype=torch.uint8)
    with pytest.raises(ValueError, match="shape"):                                        # wrong shape
        frames.render_frames(two, out=(torch.empty((2, 8, 8, 4), dtype=torch.uint8), ok_d), **g)
    with pytest.raises(ValueError, match="shape"):                                        # wrong number of frames
        frames.render_frames(two, out=(torch.empty((3, 8, 8, 3), dtype=torch.uint8), ok_d), **g)
    with pytest.raises(ValueError, match="uint8"):                                        # wrong dtype
        frames.render_frames(two, out=(torch.empty((2, 8, 8, 3), dtype=torch.float32), ok_d), **g)
    with pytest.raises(ValueError, match="page-locked"):                                  # pageable host memory
        frames.render_frames(two, out=(torch.empty((2, 8, 8, 3), dtype=torch.uint8), ok_d), **g)
    with pytest.raises(ValueError, match="pair"):
        frames.render_frames(two, out=torch.empty((2, 8, 8, 3), dtype=torch.uint8), **g)
    with pytest.raises(ValueError, match="exactly one"):
        frames.render_frames(two, means3D=g["means3D"], opacities=g["opacities"], scales=g["scales"], rotations=g["rotations"])
    with pytest.raises(GsrError):                                                         # host tensors: there is no CPU path
        frames.render_frames(two, **g)
    with pytest.raises(GsrError):
        frames.render_frames(two, to_host=False, **g)


def test_quantize_frames_argument_errors():
    from dreamscene_amd import frames
    from dreamscene_amd._lib import GsrError
    img, da = torch.rand(3, 8, 6), torch.rand(2, 8, 6)
    with pytest.raises(ValueError):
        frames.quantize_frames([])
    with pytest.raises(ValueError):
        frames.quantize_frames([torch.rand(4, 8, 6)])                                     # not [3,H,W]
    with pytest.raises(ValueError):
        frames.quantize_frames(torch.rand(3, 8, 6))                                       # a stacked tensor is [F,3,H,W]
    with pytest.raises(ValueError):
        frames.quantize_frames([img.double()])
    with pytest.raises(ValueError, match="same image size"):
        frames.quantize_frames([img, torch.rand(3, 6, 8)])
    with pytest.raises(ValueError, match="same image size"):
        frames.quantize_frames([img], [torch.rand(2, 6, 8)])
    with pytest.raises(ValueError):
        frames.quantize_frames([img, img], [da])                                          # one depth_alpha for two images
    with pytest.raises(ValueError):
        frames.quantize_frames([img], None, None, torch.empty((1, 8, 6, 1), dtype=torch.uint8))
    with pytest.raises(GsrError):
        frames.quantize_frames([img], [da])
    with pytest.raises(GsrError):
        frames.quantize_frames(torch.rand(2, 3, 8, 6))


def test_reference_tail_is_the_reference_expression():
    """frames_ref restates the reference's lines; spot values of the chain, ties to even included."""
    x = torch.tensor([-1.0, -0.0, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.5, 1.0, 7.0]).reshape(1, 1, 9).repeat(3, 1, 1)
    y = FR.ref_rgb(x)
    assert y.shape == (1, 9, 3) and y.dtype == np.uint8
    # fl32(0.5 / 255) * 255 = 0.5 exactly -> 0 (even); 1.5 / 255 -> 1.5 -> 2; 2.5 / 255 -> 2.5 -> 2
    t = (torch.tensor([0.5 / 255, 1.5 / 255, 2.5 / 255]).numpy() * np.float32(255)).tolist()
    expect_mid = [int(np.rint(np.float32(v))) for v in t]
    assert y[0, :, 0].tolist() == [0, 0, 0] + expect_mid + [128, 255, 255]
    da = torch.zeros(2, 2, 3)
    assert FR.ref_depth(da).shape == (2, 3, 1) and not FR.ref_depth(da).any()            # the all-zero frame: defined as 0
    da[0] = torch.tensor([[0.0, 1.0, 2.0], [4.0, 3.0, 0.5]])
    assert FR.ref_depth(da)[..., 0].tolist() == [[0, 64, 128], [255, 191, 32]]           # 63.75 -> 64, 127.5 -> 128, 31.875


def test_crafted_inputs_are_not_vacuous():
    ties = FR.tie_candidates()
    assert ties.size == 765 and ties.dtype == np.float32
    on_tie, rint_vs_floor = FR.tie_counts(ties)
    print(f"tie candidates: {on_tie} exactly on a tie, rint and floor(x + 0.5) differ on {rint_vs_floor}")
    assert on_tie > 0 and rint_vs_floor > 0
    full = FR.division_sensitive(FR.division_plane())
    print(f"division plane: {full} bytes differ between division and reciprocal-multiply")
    assert full > 0
    images, das = FR.crafted_planes()
    n = FR.H0 * FR.W0
    assert images.shape == (3, 3, FR.H0, FR.W0) and das.shape == (3, 2, FR.H0, FR.W0) and n % 2 == 1 and (3 * n) % 4 != 0
    assert bool(torch.isfinite(images).all()) and bool(torch.isfinite(das).all())
    for f in range(3):
        for c in range(3):
            p = images[f, c].numpy().reshape(-1)
            assert np.isin(ties, p).all()                                                 # every candidate is in every plane
            assert FR.tie_counts(p)[1] >= rint_vs_floor
            assert (p < 0).any() and (p > 1).any() and (p == 1.0).any()
            assert (np.signbit(p) & (p == 0)).any()                                       # -0.0
    d = das[:, 0].numpy().reshape(3, -1)
    crop_count = FR.division_sensitive(d[0])
    print(f"depth frame 0 (the crop): {crop_count} division-sensitive bytes")
    assert crop_count > 0
    assert d[0].argmax() == n - 1 and (d[0][:-1] < d[0][-1]).all()                        # the maximum in the last pixel
    assert not d[1].any()                                                                 # the all-zero frame
    assert d[2].argmax() == 0 and (d[2][1:] < d[2][0]).all()                              # the maximum in the first pixel
    rgb, dep = FR.ref_frames(images, das)
    assert rgb.shape == (3, FR.H0, FR.W0, 3) and dep.shape == (3, FR.H0, FR.W0, 1) and not dep[1].any()
    assert dep[0].reshape(-1)[-1] == 255 and dep[2].reshape(-1)[0] == 255
