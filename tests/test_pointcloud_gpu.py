"""dreamscene_amd.pointcloud on the GPU: the kernels of csrc/sample.hip against the numpy restatement tests/sample_ref.py (which
tests/test_pointcloud.py holds to the reference's distributions), and SeededGaussianModel against GaussianModel.create_from_pcd
fed the same cloud from the host. Indoor env and floor and every colour are +, -, *, / only: compared bit for bit. Coordinates that
pass through cbrtf / sinf / cosf (and the mesh's, whose mean is summed in another order): within 1e-5 R, R the cloud's radius."""
import gc
import math

import numpy as np
import pytest
import torch

from dreamscene_amd import model as M
from dreamscene_amd import pointcloud as PC
from dreamscene_amd import render_api, synth
from tests import sample_ref as SR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0xC0FFEE_0000_0001
SIZES = (1, 63, 64, 65, 255, 257, 4097)
BOX = np.array([-3.5, -2.5, 0.0, 3.5, 2.5, 5.0])
OBOX = np.array([-1.5, -1.0, -0.25, 1.25, 2.0, 1.0])
ENV_COLOR, FLOOR_COLOR = (135.0, 206.0, 300.0), (120.0, 90.0, 60.0)
NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
# four triangles around vertex 0 with areas 1, 2, 0 (collinear) and 5, each in a coordinate plane
MESH_V = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 2], [0, 2, 0], [5, 0, 0], [0, 0, 1], [1, 0, 0]], np.float64)
MESH_F = np.array([[0, 1, 2], [0, 3, 4], [0, 7, 1], [0, 5, 3]])


@pytest.fixture(scope="module", autouse=True)
def release_cached_blocks():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def eps(m):
    return math.sqrt(math.log(2.0 / 1e-9) / (2.0 * m))


def _np(t):
    return t.detach().cpu().numpy()


def bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} entries differ in their bits"


def seed_points(n):
    """The first n of one fixed set of seed points and colours."""
    rng = np.random.default_rng(5)
    pts, cols = rng.normal(size=(max(SIZES), 3)).astype(np.float32) * np.float32(0.3), rng.random((max(SIZES), 3))
    return pts[:n], cols[:n].astype(np.float32)


# kind -> (device draw(n), restatement(n), R or None for "bit for bit")
def _jitter_pair(use_colors):
    def dev(n):
        p, c = seed_points(n)
        return PC.jitter_cloud(torch.tensor(p, device=DEV), torch.tensor(c, device=DEV), seed=SEED, use_colors=use_colors)

    def ref(n):
        return SR.jitter(SEED, *seed_points(n), use_colors=use_colors)
    return dev, ref, 0.05


KINDS = {
    "env_indoor": (lambda n: PC.sample_env("indoor", BOX, seed=SEED, num_pts=n, device=DEV),
                   lambda n: SR.env_indoor(SEED, BOX, n), None),
    "floor_indoor": (lambda n: PC.sample_floor("indoor", BOX, seed=SEED, floor_init_color=FLOOR_COLOR, num_pts=n, device=DEV),
                     lambda n: SR.floor_indoor(SEED, BOX, FLOOR_COLOR, n), None),
    "env_outdoor": (lambda n: PC.sample_env("outdoor", OBOX, seed=SEED, env_init_color=ENV_COLOR, num_pts=n, device=DEV),
                    lambda n: SR.env_outdoor(SEED, OBOX, ENV_COLOR, n, False), SR.radius_base(OBOX)),
    "env_outdoor_zero_ground": (lambda n: PC.sample_env("outdoor", OBOX, seed=SEED, zero_ground=True, env_init_color=ENV_COLOR,
                                                        num_pts=n, device=DEV),
                                lambda n: SR.env_outdoor(SEED, OBOX, ENV_COLOR, n, True), SR.radius_base(OBOX)),
    "floor_outdoor": (lambda n: PC.sample_floor("outdoor", OBOX, seed=SEED, zero_ground=True, floor_init_color=FLOOR_COLOR,
                                                num_pts=n, device=DEV),
                      lambda n: SR.floor_outdoor(SEED, OBOX, FLOOR_COLOR, n), SR.radius_base(OBOX)),
    "ball": (lambda n: PC.sample_ball(n, 0.5, seed=SEED, device=DEV), lambda n: SR.ball(SEED, n, 0.5), 0.5),
    "jitter_rgb": _jitter_pair(True),
    "jitter_sh": _jitter_pair(False),
    "mesh": (lambda n: PC.sample_mesh(MESH_V, MESH_F, n, seed=SEED, device=DEV), lambda n: SR.mesh(SEED, MESH_V, MESH_F, n)[:2],
             5.0 / 80.0),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_device_against_the_restatement(kind):
    dev, ref, R = KINDS[kind]
    worst = 0.0
    for n in SIZES:
        cloud = dev(n)
        rp, rc = ref(n)
        assert cloud.points.dtype == torch.float32 and cloud.points.device == DEV and cloud.points.is_contiguous()
        assert tuple(cloud.points.shape) == rp.shape and tuple(cloud.colors.shape) == rc.shape, (kind, n)
        bits(_np(cloud.colors), rc, f"{kind} colours at {n}")
        if R is None:
            bits(_np(cloud.points), rp, f"{kind} points at {n}")
        else:
            if kind.startswith("jitter"):                      # the offsets are what the bar is about: take the seed points off
                base = np.repeat(seed_points(n)[0] * np.float32([1, -1, 1]) + np.float32([0, 0, 0.15]), 20, axis=0)
                assert np.abs(_np(cloud.points) - base).max() <= 0.05 + 1e-6
            d = float(np.abs(_np(cloud.points).astype(np.float64) - rp.astype(np.float64)).max())
            worst = max(worst, d / R)
            assert np.isfinite(_np(cloud.points)).all() and d <= 1e-5 * R, f"{kind} at {n}: {d:.3e} > 1e-5 * {R}"
    print(f"{kind}: worst distance {worst:.3e} of R (bar 1e-5)")


@pytest.mark.parametrize("kind", list(KINDS))
def test_prefix_property_on_the_device_s_bits(kind):
    dev = KINDS[kind][0]
    small, big = dev(65), dev(4097)
    sheets = 5 if kind == "env_indoor" else 1
    for field in ("points", "colors"):
        if kind == "mesh" and field == "points":
            continue                                           # the mean that is taken off is the whole draw's
        a, b = _np(getattr(small, field)), _np(getattr(big, field))
        for sa, sb in zip(np.split(a, sheets), np.split(b, sheets)):
            bits(sa, sb[:len(sa)], f"{kind}: the first {len(sa)} rows")
    if kind == "mesh":                                         # up to the shift of the two means, the rows are the same
        d = _np(big.points)[:65].astype(np.float64) - _np(small.points).astype(np.float64)
        assert np.abs(d - d.mean(axis=0)).max() <= 1e-5 * 5.0 / 80.0


def test_box_on_the_device_and_on_the_host_give_equal_bits():
    dbox = torch.tensor(BOX, dtype=torch.float32, device=DEV)
    for n in (65, 257):
        a = PC.sample_env("indoor", dbox, seed=SEED, num_pts=n)
        b = PC.sample_env("indoor", BOX, seed=SEED, num_pts=n, device=DEV)
        c = PC.sample_env("indoor", list(BOX), seed=SEED, num_pts=n, device=DEV)
        fa = PC.sample_floor("indoor", dbox, seed=SEED, floor_init_color=FLOOR_COLOR, num_pts=n)
        fb = PC.sample_floor("indoor", BOX, seed=SEED, floor_init_color=FLOOR_COLOR, num_pts=n, device=DEV)
        for x, y in ((a, b), (a, c), (fa, fb)):
            bits(_np(x.points), _np(y.points), "points")
            bits(_np(x.colors), _np(y.colors), "colours")
    obox = torch.tensor(OBOX, dtype=torch.float64, device=DEV)     # outdoor: the host reads the box once
    a = PC.sample_env("outdoor", obox, seed=SEED, env_init_color=ENV_COLOR, num_pts=257)
    b = PC.sample_env("outdoor", OBOX, seed=SEED, env_init_color=ENV_COLOR, num_pts=257, device=DEV)
    bits(_np(a.points), _np(b.points), "outdoor points")
    assert a.points.device == DEV
    n_default = PC.sample_floor("outdoor", OBOX, seed=SEED, zero_ground=True, floor_init_color=FLOOR_COLOR, device=DEV)
    assert n_default.points.shape[0] == SR.outdoor_rows(OBOX, 20_000)
    assert not torch.equal(PC.sample_ball(65, 0.5, seed=1, device=DEV).points, PC.sample_ball(65, 0.5, seed=2, device=DEV).points)


def test_mesh_triangles_and_barycentric_coordinates():
    n = 65_536
    cloud, tri = PC.sample_mesh(MESH_V, MESH_F, n, seed=SEED, device=DEV, return_triangles=True)
    tri, p = _np(tri), _np(cloud.points).astype(np.float64) * 80.0
    assert tri.dtype == np.int32 and tri.min() >= 0 and tri.max() <= 3 and not (tri == 2).any()
    share = np.bincount(tri, minlength=4) / n
    d = float(np.abs(np.cumsum(share) - np.array([1, 3, 3, 8]) / 8.0).max())
    print(f"chosen-triangle CDF: {d:.5f} (bar {eps(n):.5f})")
    assert d <= eps(n)
    assert np.array_equal(tri, SR.mesh(SEED, MESH_V, MESH_F, n)[2])
    # the mean that was taken off, from the device's own output: triangle 0 lies in the mesh's z = 0 plane (the second output
    # column after the (x, z, y) swap), triangle 1 in x = 0, triangle 3 in y = 0 (the third output column)
    mean = -np.array([np.median(p[tri == 1, 0]), np.median(p[tri == 0, 1]), np.median(p[tri == 3, 2])])
    raw = (p + mean)[:, [0, 2, 1]]                                  # back to the mesh's axes
    lo, hi = 0.0, 1.0
    for t in (0, 1, 3):
        v0, v1, v2 = MESH_V[MESH_F[t]]
        q = raw[tri == t] - v0
        bc, res, _, _ = np.linalg.lstsq(np.stack([v1 - v0, v2 - v0], 1), q.T, rcond=None)
        w = np.stack([1.0 - bc[0] - bc[1], bc[0], bc[1]])
        assert np.abs(np.stack([v1 - v0, v2 - v0], 1) @ bc - q.T).max() <= 1e-6 * 5.0      # in the triangle's plane
        lo, hi = min(lo, float(w.min())), max(hi, float(w.max()))
    print(f"barycentric coordinates in [{lo:.3e}, 1 + {hi - 1:.3e}]")
    assert lo >= -1e-6 and hi <= 1 + 1e-6
    mine = _np(cloud.points).astype(np.float64).mean(axis=0)
    assert np.abs(mine).max() <= 1e-6                                # centred


def host_twin(cloud, sh_degree, require_grad, scale):
    pcd = M.BasicPointCloud(points=_np(cloud.points), colors=_np(cloud.colors), normals=None)
    gm = M.GaussianModel({"sh_degree": sh_degree}, "scene")
    gm.create_from_pcd(pcd, require_grad, scale)
    return gm


class Recording(PC.SeededGaussianModel):
    """Notes what the samplers hand to create_from_cloud."""

    def create_from_cloud(self, cloud, require_grad=True, spatial_lr_scale=1):
        self.handed = (require_grad, spatial_lr_scale)
        super().create_from_cloud(cloud, require_grad, spatial_lr_scale)


def same_model(gm, twin, rows, require_grad, scale):
    """require_grad is what the sampler passes, as the reference's does (False for the floor); what the leaves then say is
    create_from_pcd's, which wraps them in nn.Parameter like the reference (SEMANTICS.md section 15.6)."""
    assert gm.spatial_lr_scale == scale == twin.spatial_lr_scale
    if isinstance(gm, Recording):
        assert gm.handed == (require_grad, scale)
    for name in NAMES:
        a, b = getattr(gm, name), getattr(twin, name)
        assert isinstance(a, torch.nn.Parameter) and a.requires_grad == b.requires_grad, name
        assert a.shape[0] == rows and a.device == DEV and a.is_contiguous()
        bits(_np(a), _np(b), name)
    assert gm._background.shape == (3, 1, 1) and gm._background.requires_grad == twin._background.requires_grad
    for a, b in zip(gm.stats.tensors(), twin.stats.tensors()):
        assert a.shape == b.shape and a.shape[0] == rows and not a.any()
    assert gm.max_radii2D.shape == (rows,) and gm.xyz_gradient_accum.shape == (rows, 1) and gm.denom.shape == (rows, 1)


def test_seeded_model_env_floor_and_ball_match_create_from_pcd_and_render():
    scene = dict(sh_degree=1, cam_pose_method="indoor", scene_box=BOX, zero_ground=False, env_init_color=ENV_COLOR,
                 floor_init_color=FLOOR_COLOR, num_pts=1000, seed=SEED)
    env = Recording(scene, "env")
    same_model(env, host_twin(PC.sample_env("indoor", BOX, seed=SEED, num_pts=1000, device=DEV), 1, True, 1), 5000, True, 1)
    floor = Recording(scene, "floor")
    same_model(floor, host_twin(PC.sample_floor("indoor", BOX, seed=SEED, floor_init_color=FLOOR_COLOR, num_pts=1000, device=DEV),
                                1, False, 1), 1000, False, 1)
    ball = Recording(dict(sh_degree=3, init_guided="default", init_prompt="a ball", num_pts=4097, radius=0.5,
                                       seed=SEED), "object", "unused")
    same_model(ball, host_twin(PC.sample_ball(4097, 0.5, seed=SEED, device=DEV), 3, True, 10), 4097, True, 10)
    # the class attribute is the seed of a dict without one
    a = PC.SeededGaussianModel({k: v for k, v in scene.items() if k != "seed"}, "env")
    bits(_np(a._xyz), _np(PC.sample_env("indoor", BOX, seed=0, num_pts=1000, device=DEV).points), "seed 0")
    assert not torch.equal(a._xyz, env._xyz)
    cam = synth.indoor_cameras(1, 64, 64)[0]                          # the eye inside the box, looking at a wall
    with torch.no_grad():
        out = render_api.object_render(env, cam, torch.ones(3, device=DEV))
    image = _np(out["image"])
    assert image.shape == (3, 64, 64) and np.isfinite(image).all() and np.isfinite(_np(out["alpha"])).all()
    assert int((_np(out["radii"]) > 0).sum()) > 0 and float(_np(out["alpha"]).max()) > 0


def test_seeded_model_outdoor_pointe_and_shapes(tmp_path):
    scene = dict(sh_degree=0, cam_pose_method="outdoor", scene_box=torch.tensor(OBOX, device=DEV), zero_ground=True,
                 env_init_color=ENV_COLOR, floor_init_color=FLOOR_COLOR, num_pts=4097, seed=3)
    env = Recording(scene, "env")
    same_model(env, host_twin(PC.sample_env("outdoor", OBOX, seed=3, zero_ground=True, env_init_color=ENV_COLOR, num_pts=4097,
                                            device=DEV), 0, True, 1), 4097, True, 1)
    assert float(env._xyz[:, 2].min()) > 0                           # zero_ground: the upper half
    floor = Recording(scene, "floor")
    assert floor._xyz.shape[0] == 4097 and floor.handed == (False, 1)
    assert float(floor._xyz[:, 2].max()) <= OBOX[2] + 1e-6 and float(floor._xyz[:, 2].min()) >= OBOX[2] - 0.1 - 1e-6
    pts, cols = seed_points(64)
    for use_rgb in (True, False):
        p = dict(sh_degree=0, init_guided="pointe", init_prompt="a chair", use_pointe_rgb=use_rgb, seed=9,
                 init_points=M.BasicPointCloud(points=pts.astype(np.float64), colors=cols.astype(np.float64), normals=None))
        gm = Recording(p, "object", str(tmp_path))
        cloud = PC.jitter_cloud(torch.tensor(pts, device=DEV), torch.tensor(cols, device=DEV), seed=9, use_colors=use_rgb)
        same_model(gm, host_twin(cloud, 0, True, 1), 1280, True, 1)
    obj = tmp_path / "mesh.OBJ"
    obj.write_text("".join(f"v {a} {b} {c}\n" for a, b, c in MESH_V) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in MESH_F))
    gm = Recording(dict(sh_degree=0, init_guided="shapes", init_prompt=str(obj), seed=9), "object", str(tmp_path))
    same_model(gm, host_twin(PC.sample_mesh(MESH_V, MESH_F, PC.SHAPES_PTS, seed=9, device=DEV), 0, True, 1), PC.SHAPES_PTS, True, 1)
    direct = M.BasicPointCloud(points=pts, colors=cols, normals=None)          # the branches the base class has too
    gm = PC.SeededGaussianModel(dict(sh_degree=0, init_guided=direct), "object", str(tmp_path))
    assert gm._xyz.shape[0] == 64 and gm.spatial_lr_scale == 1
