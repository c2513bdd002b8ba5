"""-m gpu: csrc/frames.hip through dreamscene_amd.frames against the reference's tail (tests/frames_ref.py) computed from the same
fp32 tensors. Every comparison is byte-exact: no tolerance, no outliers."""
import faulthandler
import functools

import numpy as np
import pytest
import torch

from tests import frames_ref as FR
from tests import util

TEST_SECONDS = 120


@pytest.fixture(autouse=True)
def _time_limit():
    """A hung kernel does not return to Python: the watchdog thread ends the process with a traceback instead."""
    faulthandler.dump_traceback_later(TEST_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dev():
    return torch.device("cuda:0")


def same_bytes(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    ne = got != ref
    n = int(ne.sum())
    print(f"[frames] {what}: {n} of {ref.size} bytes differ")
    assert n == 0, f"{what}: {n} bytes differ, first at {np.argwhere(ne)[:4].tolist()}: {got[ne][:4]} vs {ref[ne][:4]}"


@functools.lru_cache(maxsize=None)
def crafted():
    images, das = FR.crafted_planes()
    return images, das, FR.ref_frames(images, das)


@functools.lru_cache(maxsize=None)
def randoms(F, H, W):
    images, das = FR.random_planes(F, H, W, seed=100 * F + H)
    return images, das, FR.ref_frames(images, das)


@pytest.mark.gpu
def test_crafted_planes(built_lib):
    """F = 3 of 37x53 (H*W odd): ties, values outside [0, 1], -0.0, 1.0; the depth maximum in the first and in the last pixel,
    an all-zero depth frame, the division-sensitive crop."""
    from dreamscene_amd import frames
    images, das, (ref_rgb, ref_dep) = crafted()
    assert FR.tie_counts(images.numpy())[1] > 0 and FR.division_sensitive(das[0, 0].numpy()) > 0
    imgs = [images[f].to(dev()) for f in range(3)]
    dal = [das[f].to(dev()) for f in range(3)]
    rgb, dep = frames.quantize_frames(imgs, dal)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (3, FR.H0, FR.W0, 3) and tuple(dep.shape) == (3, FR.H0, FR.W0, 1)
    same_bytes(rgb, ref_rgb, "crafted rgb")
    same_bytes(dep, ref_dep, "crafted depth")
    assert not dep[1].any()                                          # the all-zero frame
    # the same planes stacked, and at plane bases that are only 4-byte aligned (the dword-load path)
    flat_i = torch.empty(images.numel() + 1, device=dev())
    flat_d = torch.empty(das.numel() + 1, device=dev())
    si = flat_i[1:].view(images.shape).copy_(images)
    sd = flat_d[1:].view(das.shape).copy_(das)
    rgb2, dep2 = frames.quantize_frames(si, sd)
    same_bytes(rgb2, ref_rgb, "crafted rgb, stacked")
    same_bytes(dep2, ref_dep, "crafted depth, stacked")


@pytest.mark.gpu
@pytest.mark.parametrize("F,H,W", [(1, 96, 80), (5, 96, 80), (1, 1024, 1024), (5, 1024, 1024), (1, 1400, 1536)])
def test_random_planes(built_lib, F, H, W):
    """96x80: several blocks; 1024x1024: the full size, the maximum's grid-stride loop; 1400x1536: more units than the quantise
    grid holds (its grid-stride loop). With depth, without, into the caller's outputs, and from planes off the 16-byte grid."""
    from dreamscene_amd import frames
    images, das, (ref_rgb, ref_dep) = randoms(F, H, W)
    stacked_i, stacked_d = images.to(dev()), das.to(dev())
    imgs, dal = list(stacked_i.unbind(0)), list(stacked_d.unbind(0))
    rgb, dep = frames.quantize_frames(imgs, dal)
    same_bytes(rgb, ref_rgb, "rgb")
    same_bytes(dep, ref_dep, "depth")
    rgb_only, none = frames.quantize_frames(imgs)
    assert none is None
    same_bytes(rgb_only, ref_rgb, "rgb, depth_alphas=None")
    out_rgb = torch.full((F, H, W, 3), 7, dtype=torch.uint8, device=dev())
    out_dep = torch.full((F, H, W, 1), 7, dtype=torch.uint8, device=dev())
    r, d = frames.quantize_frames(stacked_i, stacked_d, out_rgb, out_dep)
    assert r is out_rgb and d is out_dep
    same_bytes(out_rgb, ref_rgb, "rgb, given output, stacked input")
    same_bytes(out_dep, ref_dep, "depth, given output, stacked input")
    if H * W <= 96 * 80:
        flat_i = torch.empty(images.numel() + 3, device=dev())
        flat_d = torch.empty(das.numel() + 3, device=dev())
        r, d = frames.quantize_frames(flat_i[3:].view(images.shape).copy_(images), flat_d[3:].view(das.shape).copy_(das))
        same_bytes(r, ref_rgb, "rgb, planes 4-byte aligned")
        same_bytes(d, ref_dep, "depth, planes 4-byte aligned")
        # outputs that start at an odd address: the byte stores
        ob = torch.zeros(F * H * W * 3 + 1, dtype=torch.uint8, device=dev())
        od = torch.zeros(F * H * W + 1, dtype=torch.uint8, device=dev())
        frames.quantize_frames(imgs, dal, ob[1:].view(F, H, W, 3), od[1:].view(F, H, W, 1))
        same_bytes(ob[1:].view(F, H, W, 3), ref_rgb, "rgb, odd output address")
        same_bytes(od[1:].view(F, H, W, 1), ref_dep, "depth, odd output address")
        assert int(ob[0]) == 0 and int(od[0]) == 0


def orbit_settings(n, H=96, W=80):
    from dreamscene_amd import synth
    cams = [synth.orbit_camera(3.0, 75.0, 360.0 * i / n, 0.46, H, W) for i in range(n)]
    return [util.settings_for(c, [1, 1, 1], 3, dev()) for c in cams]


def scene_tensors():
    g, _ = util.small_scene(P=600)
    p = {k: torch.tensor(v, device=dev()) for k, v in g.items()}
    return dict(means3D=p["means3D"], opacities=p["opacities"], shs=p["shs"], scales=p["scales"], rotations=p["rotations"])


def reference_frames(sl, args, chunk):
    """The reference's tail on the fp32 outputs of the forward, called with render_frames' chunking."""
    from dreamscene_amd import rasterizer as R, views
    rc = R.DEFAULT_CONTEXT.snapshot()
    rc._forward_only = True
    imgs, das = [], []
    with torch.no_grad():
        for i in range(0, len(sl), chunk):
            res = views.rasterize_views_forward_raw(sl[i:i + chunk], args["means3D"], args["opacities"], args["shs"], None,
                                                    args["scales"], args["rotations"], None, rc=rc)
            imgs += [o["color"].cpu() for o, _ in res]
            das += [o["depth_alpha"].cpu() for o, _ in res]
    return FR.ref_frames(imgs, das)


@pytest.mark.gpu
def test_render_frames_end_to_end(built_lib):
    """7 orbit cameras, chunk = 3: chunks of 3, 3 and 1 (the last one takes the unbatched forward)."""
    from dreamscene_amd import frames
    sl, args = orbit_settings(7), scene_tensors()
    fr = frames.render_frames(sl, chunk=3, **args)
    ref_rgb, ref_dep = reference_frames(sl, args, 3)
    assert int(ref_dep.max()) == 255 and int(ref_rgb.min()) < 250             # a picture, not a blank
    assert fr.rgb.device.type == "cpu" and fr.rgb.is_pinned() and fr.depth.is_pinned()
    same_bytes(fr.rgb, ref_rgb, "render_frames rgb")
    same_bytes(fr.depth, ref_dep, "render_frames depth")
    assert len(list(fr.rgb.numpy())) == 7                                      # img_frames of the reference's callers
    nd = frames.render_frames(sl, chunk=3, depth=False, **args)
    assert nd.depth is None
    same_bytes(nd.rgb, ref_rgb, "render_frames rgb, depth=False")
    on_dev = frames.render_frames(sl, chunk=3, to_host=False, **args)
    assert on_dev.rgb.device == dev() and on_dev.depth.device == dev()
    same_bytes(on_dev.rgb, fr.rgb.numpy(), "to_host=False rgb against the host bytes")
    same_bytes(on_dev.depth, fr.depth.numpy(), "to_host=False depth against the host bytes")


@pytest.mark.gpu
def test_slot_reuse_and_ordering(built_lib):
    """F = 9, chunk = 2: five chunks through the two staging slots; twice into the same pinned buffers; one chunk of 9; and
    on a stream that is not the default one."""
    from dreamscene_amd import frames
    sl, args = orbit_settings(9), scene_tensors()
    ref_rgb, ref_dep = reference_frames(sl, args, 2)
    out = frames.Frames(torch.zeros((9, 96, 80, 3), dtype=torch.uint8).pin_memory(),
                        torch.zeros((9, 96, 80, 1), dtype=torch.uint8).pin_memory())
    a = frames.render_frames(sl, chunk=2, out=out, **args)
    assert a.rgb is out.rgb and a.depth is out.depth
    first = (a.rgb.numpy().copy(), a.depth.numpy().copy())
    same_bytes(first[0], ref_rgb, "chunk=2 rgb")
    same_bytes(first[1], ref_dep, "chunk=2 depth")
    out.rgb.zero_()
    out.depth.zero_()
    frames.render_frames(sl, chunk=2, out=out, **args)
    same_bytes(out.rgb, first[0], "chunk=2 again, same buffers, rgb")
    same_bytes(out.depth, first[1], "chunk=2 again, same buffers, depth")
    one = frames.render_frames(sl, chunk=9, **args)
    same_bytes(one.rgb, first[0], "chunk=9 rgb")
    same_bytes(one.depth, first[1], "chunk=9 depth")
    side = torch.cuda.Stream(dev())
    with torch.cuda.stream(side):
        s = frames.render_frames(sl, chunk=2, **args)
    same_bytes(s.rgb, first[0], "side stream rgb")
    same_bytes(s.depth, first[1], "side stream depth")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_quantize_frames_is_capturable(built_lib):
    from dreamscene_amd import frames
    F, H, W = 3, 96, 80
    sets = [FR.random_planes(F, H, W, seed=s) for s in (1, 2, 3)]
    imgs = [sets[0][0][f].to(dev()) for f in range(F)]
    dal = [sets[0][1][f].to(dev()) for f in range(F)]
    out_rgb = torch.zeros((F, H, W, 3), dtype=torch.uint8, device=dev())
    out_dep = torch.zeros((F, H, W, 1), dtype=torch.uint8, device=dev())
    frames.quantize_frames(imgs, dal, out_rgb, out_dep)                         # eager, first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        frames.quantize_frames(imgs, dal, out_rgb, out_dep)
    for images, das in sets[1:]:
        for f in range(F):
            imgs[f].copy_(images[f])
            dal[f].copy_(das[f])
        out_rgb.zero_()
        out_dep.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager_rgb, eager_dep = frames.quantize_frames([i.clone() for i in imgs], [d.clone() for d in dal])
        ref_rgb, ref_dep = FR.ref_frames(images, das)
        same_bytes(out_rgb, eager_rgb.cpu().numpy(), "replayed rgb against eager")
        same_bytes(out_dep, eager_dep.cpu().numpy(), "replayed depth against eager")
        same_bytes(out_rgb, ref_rgb, "replayed rgb against the reference tail")
        same_bytes(out_dep, ref_dep, "replayed depth against the reference tail")
