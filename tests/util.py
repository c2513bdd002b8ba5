"""Shared scene builders / comparison helpers for the parity tests."""
from __future__ import annotations

import numpy as np
import torch

from dreamscene_amd import synth
from dreamscene_amd.camera import Camera, focal2fov, fov2focal


def small_scene(P=600, H=96, W=80, K=16, seed=3, scale_mul=6.0, radius=3.0, cam_idx=1, init_opacity=False):
    g = synth.g_object(P, seed=seed, K=K, init_opacity=init_opacity)
    g["scales"] = (g["scales"] * scale_mul).astype(np.float32)
    cam = synth.object_cameras(cam_idx + 1, H, W, radius=radius)[cam_idx]
    return g, cam


FUZZ_FOVS = (0.2, 0.46, 1.2, 2.2)          # tan(fov / 2) from 0.10 to 1.96: both sides of 1
FUZZ_RADII = (0.6, 1.5, 3.0, 6.0)         # 0.6: the eye at the rim of the cloud (near-plane culls, huge footprints)
FUZZ_SCALE_MODIFIERS = (0.25, 0.5, 1.0, 1.7, 3.0)


# The 24 seeds of random_settings_config that tests/test_fuzz_cameras.py (GPU) and test_oracle_consistency.py (CPU: the C
# oracle against float64 autograd on the same seeds) run. 0 ... 23 with two replaced by the next seeds that qualify:
#   12 -> 25   the C oracle itself is 1.07e-5 of max|dL/dproj| away from float64 (65 Gaussians, tanfov 1.97 x 0.10, 38 of them
#              visible: a sum of cancelling terms in fp32), so it cannot arbitrate 1e-5 there
#   22 -> 26   P = 1 and the one Gaussian is outside the frustum: nothing is rendered, no gradient is defined
#   (24 is skipped as a replacement for the same reason as 22)
CAMERA_FUZZ_SEEDS = tuple(s for s in range(24) if s not in (12, 22)) + (25, 26)


def random_camera(rng, H, W) -> Camera:
    """A look-at camera from anywhere on a sphere (poles included) towards a target off the origin, with arbitrary roll (the
    "up" vector is random) and fovx from FUZZ_FOVS; fovy is drawn independently half the time and follows the reference's
    focal2fov(fov2focal(fovx, H), W) rule otherwise. R and T are built the way camera.look_at_camera builds them."""
    d = rng.normal(size=3)
    eye = d / np.linalg.norm(d) * float(rng.choice(FUZZ_RADII))
    target = rng.normal(scale=0.3, size=3)
    f = target - eye
    f /= np.linalg.norm(f)
    while True:
        up = rng.normal(size=3)
        r = np.cross(f, up)
        if np.linalg.norm(r) > 1e-3 * np.linalg.norm(up):      # (an "up" along the viewing direction defines no roll)
            break
    r /= np.linalg.norm(r)
    dn = np.cross(f, r)                         # camera +y points down in image space
    R = np.stack((r, dn, f), axis=-1)           # C2W rotation, columns = camera axes
    T = -R.T @ eye
    fovx = float(rng.choice(FUZZ_FOVS))
    if rng.random() < 0.5:
        fovy = float(rng.choice(FUZZ_FOVS))
    else:
        fovy = focal2fov(fov2focal(fovx, H), W)
    return Camera.from_RT(R.astype(np.float32), T.astype(np.float32), fovx, fovy, H, W)


def random_settings_config(seed):
    """Camera and settings space (tests/test_fuzz.py covers Gaussian space): -> (g, cam, bg, P, K, D, scale_modifier).
    Everything derives from default_rng(5000 + seed)."""
    from dreamscene_amd import synth
    rng = np.random.default_rng(5000 + seed)
    P = int(rng.choice([1, 65, 257, 600]))
    K = int(rng.choice([1, 4, 9, 16]))
    D = int(rng.integers(0, min(3, int(np.sqrt(K)) - 1) + 1))
    H = int(rng.integers(8, 120))
    W = int(rng.integers(8, 140))
    g = synth.g_object(max(P, 64), seed=seed, K=K)
    g = {k: np.ascontiguousarray(v[:P]) for k, v in g.items()}
    g["scales"] = (g["scales"] * float(rng.choice([0.3, 2.0, 6.0]))).astype(np.float32)
    scale_modifier = float(rng.choice(FUZZ_SCALE_MODIFIERS))
    cam = random_camera(rng, H, W)
    bg = rng.random(3).astype(np.float32)
    return g, cam, bg, P, K, D, scale_modifier


def settings_for(cam: Camera, bg, sh_degree, device, score_flag=False, scale_modifier=1.0, cls=None):
    from dreamscene_amd.rasterizer import GaussianRasterizationSettings
    cls = cls or GaussianRasterizationSettings
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=device)
    return cls(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
               bg=t(bg), scale_modifier=scale_modifier, viewmatrix=t(cam.world_view_transform),
               projmatrix=t(cam.full_proj_transform), sh_degree=sh_degree, campos=t(cam.camera_center),
               prefiltered=False, score_flag=score_flag)


def oracle_view(CO, cam: Camera, P, K, D, bg, scale_modifier=1.0, score_mode=0):
    return CO.make_view(P, K, D, cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, bg,
                        cam.world_view_transform, cam.full_proj_transform, cam.camera_center,
                        scale_modifier=scale_modifier, score_mode=score_mode)


def err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) if a.size else 0.0


# The 1e-5 fp32 bar of BASELINE.json, PER TENSOR and relative to that tensor's own largest reference entry: an entry may be
# off by 1e-5 * max|ref| of ITS tensor. (Rounds 1-5 used max(1, max|ref|): for the small tensors -- dL/dshs ~ 1e-2, dL/dopacity
# ~ 3e-2 at C2 -- that was a bar of 1e-3 of their own scale.) The only absolute floor: a tensor whose reference is identically
# (or numerically) zero -- max|ref| < REL_FLOOR -- is held to 1e-5 * REL_FLOOR.
REL_FLOOR = 1e-6


def rel_scale(ref, floor=REL_FLOOR):
    if isinstance(ref, torch.Tensor):
        ref = ref.detach().cpu().numpy()
    ref = np.asarray(ref, dtype=np.float64)
    return max(floor, float(np.abs(ref).max()) if ref.size else floor)


def tol_ok(a, ref, atol=1e-5, rtol=1e-5):
    """|a-ref| <= atol * max|ref| for every entry (rel_scale above)"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    if isinstance(ref, torch.Tensor):
        ref = ref.detach().cpu().numpy()
    return err(a, ref) <= atol * rel_scale(ref)


def same_bits(a, b, what="", max_ties=4):
    """Two runs of the HIP backward on the same inputs: the same BITS. K7 adds its wave results across waves in double --
    the sum of fp32 addends is exact in double whatever the arrival order as long as the addends lie within 2^29 of each
    other; an addend smaller than that (a pixel at the splat's centre, where q u^2 -> 0) can lose its last bits, the double
    then differs by 2^-53 between two orders, and once in ~10^9 values that difference sits on an fp32 rounding boundary of
    the final fp32 value. So: bit-identical, except that at most `max_ties` entries of a tensor may differ by ONE fp32 ulp
    (a whole-suite run compares ~10^8 values; without this allowance it would fail spuriously every few dozen runs)."""
    import torch
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: shape / dtype"
    if np.array_equal(a, b):
        return
    ne = a != b
    n = int(ne.sum())
    assert n <= max_ties, f"{what}: {n} entries differ between two runs (bit-reproducibility lost)"
    x, y = a[ne].astype(np.float64), b[ne].astype(np.float64)
    ulp = np.maximum(np.abs(x), np.abs(y)) * 2.0 ** -23
    assert bool((np.abs(x - y) <= ulp).all()), f"{what}: entries differ by more than one fp32 ulp: {x} vs {y}"
