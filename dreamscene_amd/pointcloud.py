"""The point clouds a new model starts from, drawn on the device from a seed (csrc/sample.hip; SEMANTICS.md section 17).

The reference draws its env shell, floor and object clouds on the host with numpy's float64 stream (gs_renderer.py:218-408) and
`create_from_pcd` converts and copies them. Here a row is a pure function of (seed, cloud id, row index): the cloud is written as
fp32 straight into device memory, is the same on every rank that holds the seed, and goes on to `knn.distCUDA2` and
`gsr_model_init` without touching the host.

  sample_env / sample_floor     the env shell and the floor of an indoor box or an outdoor sphere
  sample_ball                   the `default` object cloud
  jitter_cloud                  the `pointe*` object cloud around given seed points (Point-E itself is not part of this package)
  sample_mesh, read_obj         the `shapes` object cloud on a triangle mesh read from an OBJ file
  SeededGaussianModel           GaussianModel with init_env_pcd, init_floor_pcd and init_pcd on these: env, floor and object models
                                with no DreamScene checkout. The seed is initialize_param["seed"], else the class attribute `seed`.

The reference's `_init_points3d.ply` cache is neither written nor read: the seed is what makes a cloud repeatable. No CPU fallback:
torch tensors that are not on a ROCm device raise `GsrError`. Arguments that cannot be drawn from raise `ValueError` before any
launch.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L
from . import knn
from .model import BasicPointCloud, GaussianModel

ENV_INDOOR_PTS = 400_000          # per sheet, five sheets (gs_renderer.py:221)
FLOOR_INDOOR_PTS = 300_000        # :282
ENV_OUTDOOR_DENSITY = 50_000      # rows per unit of radius_base (:254)
FLOOR_OUTDOOR_DENSITY = 20_000    # :303
SHAPES_PTS = 50_000               # :330
JITTER_COPIES, JITTER_RADIUS = 20, 0.05      # :380-387
POINTE_MODES = ("pointe", "pointe_330k", "pointe_825k")


class DeviceCloud(NamedTuple):
    points: torch.Tensor          # [n,3] fp32 on the ROCm device
    colors: torch.Tensor          # [n,3] fp32, 0..1


def _seed64(seed) -> int:
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _count(num_pts, what: str) -> int:
    n = int(num_pts)
    if n <= 0 or n != num_pts:
        raise ValueError(f"{what}: num_pts must be a positive integer, got {num_pts!r}")
    if n > 2 ** 31 - 1:
        raise ValueError(f"{what}: {n} rows are more than the generator's 32-bit row counter holds")
    return n


def _colour(rgb, what: str) -> tuple:
    """min(c / 255, 1) of an 0..255 colour, in fp32."""
    if rgb is None or len(rgb) != 3:
        raise ValueError(f"{what}: the initial colour must be three numbers (0..255), got {rgb!r}")
    c = np.minimum(np.asarray(rgb, np.float32) / np.float32(255.0), np.float32(1.0))
    if not np.isfinite(c).all():
        raise ValueError(f"{what}: the initial colour {rgb!r} is not finite")
    return tuple(float(v) for v in c)


def _device(device) -> torch.device:
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise L.GsrError(f"point clouds are drawn on a cuda (ROCm) device, not on {dev}; there is no CPU fallback")
    return dev


def _host_box(scene_box, what: str) -> np.ndarray:
    box = np.asarray(scene_box.detach().cpu() if isinstance(scene_box, torch.Tensor) else scene_box, dtype=np.float64).reshape(-1)
    if box.shape[0] != 6:
        raise ValueError(f"{what}: scene_box must hold 6 numbers (x0 y0 z0 x1 y1 z1), got {box.shape[0]}")
    if not np.isfinite(box).all():
        raise ValueError(f"{what}: scene_box {box.tolist()} is not finite")
    return box


def _device_box(scene_box, device, what: str) -> torch.Tensor:
    """scene_box as 6 fp32 in device memory. A tensor that already is on the device is not read by the host (so it is not
    checked for finiteness either); anything else is checked and uploaded."""
    if isinstance(scene_box, torch.Tensor) and scene_box.device.type == "cuda":
        if scene_box.numel() != 6:
            raise ValueError(f"{what}: scene_box must hold 6 numbers (x0 y0 z0 x1 y1 z1), got {scene_box.numel()}")
        return scene_box.detach().reshape(6).to(torch.float32).contiguous()
    box = _host_box(scene_box, what)
    return torch.tensor(box.astype(np.float32), device=_device(device))


def radius_base(scene_box: np.ndarray) -> float:
    """sqrt(sum(max(|box[:3]|, |box[3:]|)^2)) in double (gs_renderer.py:250-253)."""
    b = np.abs(np.asarray(scene_box, np.float64))
    return float(np.sqrt(np.sum(np.maximum(b[:3], b[3:]) ** 2)))


def _new_cloud(rows: int, dev: torch.device) -> DeviceCloud:
    return DeviceCloud(torch.empty((rows, 3), dtype=torch.float32, device=dev),
                       torch.empty((rows, 3), dtype=torch.float32, device=dev))


def _launch(cloud: DeviceCloud, name: str, args):
    """lib.<name>(*args(points, colors), stream) on the cloud's device and torch's current stream."""
    dev = cloud.points.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(getattr(L.load(), name)(*args(cloud.points.data_ptr(), cloud.colors.data_ptr()), stream), name)
    return cloud


def _box_mode(cam_pose_method, scene_box, device, num_pts, default_pts, density, what):
    """(device box or None, host box or None, rows per sheet, device) of an indoor / outdoor draw."""
    if cam_pose_method == "indoor":
        n = _count(default_pts if num_pts is None else num_pts, what)
        box = _device_box(scene_box, device, what)
        return box, None, n, box.device
    host = _host_box(scene_box, what)                  # the one host read of an outdoor draw: radius_base sets the row count
    rb = radius_base(host)
    n = _count(math.ceil(rb * density) if num_pts is None else num_pts, what)
    dev = scene_box.device if isinstance(scene_box, torch.Tensor) and scene_box.device.type == "cuda" else _device(device)
    return None, host, n, dev


def sample_env(cam_pose_method, scene_box, *, seed, zero_ground=False, env_init_color=None, num_pts=None,
               device=None) -> Optional[DeviceCloud]:
    """The env cloud of init_env_pcd. indoor: five sheets of num_pts (400 000) rows each around scene_box, which the kernel reads
    from device memory when it is a device tensor (no host read). outdoor: num_pts (ceil(radius_base * 50 000)) rows of a shell
    around the origin in env_init_color; scene_box is read by the host once. Any other cam_pose_method: None."""
    if cam_pose_method not in ("indoor", "outdoor"):
        return None
    what = "sample_env"
    if cam_pose_method == "outdoor":
        rgb = _colour(env_init_color, what)
    box, host, n, dev = _box_mode(cam_pose_method, scene_box, device, num_pts, ENV_INDOOR_PTS, ENV_OUTDOOR_DENSITY, what)
    s = _seed64(seed)
    if box is not None:
        _count(5 * n, what)
        return _launch(_new_cloud(5 * n, dev), "gsr_sample_env_indoor", lambda p, c: (s, box.data_ptr(), n, p, c))
    rb = radius_base(host)
    return _launch(_new_cloud(n, dev), "gsr_sample_shell", lambda p, c: (s, rb, 1 if zero_ground else 0, *rgb, n, p, c))


def sample_floor(cam_pose_method, scene_box, *, seed, zero_ground=False, floor_init_color=None, num_pts=None,
                 device=None) -> Optional[DeviceCloud]:
    """The floor cloud of init_floor_pcd in floor_init_color. indoor: num_pts (300 000) rows under the box. outdoor: num_pts
    (ceil(radius_base * 20 000)) rows of a disc, with zero_ground only (the reference has no cloud without it and dies on an
    unbound name: ValueError here). Any other cam_pose_method: None."""
    if cam_pose_method not in ("indoor", "outdoor"):
        return None
    what = "sample_floor"
    if cam_pose_method == "outdoor" and not zero_ground:
        raise ValueError("sample_floor: an outdoor scene has a floor cloud only with zero_ground")
    rgb = _colour(floor_init_color, what)
    box, host, n, dev = _box_mode(cam_pose_method, scene_box, device, num_pts, FLOOR_INDOOR_PTS, FLOOR_OUTDOOR_DENSITY, what)
    s = _seed64(seed)
    if box is not None:
        return _launch(_new_cloud(n, dev), "gsr_sample_floor_indoor", lambda p, c: (s, box.data_ptr(), *rgb, n, p, c))
    rb, z0 = radius_base(host), float(np.float32(host[2]))      # the signed box value
    return _launch(_new_cloud(n, dev), "gsr_sample_disc", lambda p, c: (s, rb, z0, *rgb, n, p, c))


def _radius(radius, what: str) -> float:
    r = float(radius)
    if not math.isfinite(r) or r < 0:
        raise ValueError(f"{what}: radius must be finite and >= 0, got {radius!r}")
    return r


def sample_ball(num_pts, radius, *, seed, device=None) -> DeviceCloud:
    """num_pts rows uniform in the ball of `radius` (init_pcd, `default`), colours in the narrow SH range around 0.5."""
    n, r, s = _count(num_pts, "sample_ball"), _radius(radius, "sample_ball"), _seed64(seed)
    return _launch(_new_cloud(n, _device(device)), "gsr_sample_ball", lambda p, c: (s, r, n, p, c))


def _rows3(a, dtype, device, what: str) -> torch.Tensor:
    """a as a contiguous [n,3] tensor of dtype on the device: numpy arrays are uploaded, torch tensors must be there already."""
    if isinstance(a, torch.Tensor):
        if a.device.type != "cuda":
            raise L.GsrError(f"{what} needs its tensors on a cuda (ROCm) device; there is no CPU fallback")
        t = a.detach()
    else:
        host = np.ascontiguousarray(np.asarray(a), dtype=np.float32 if dtype == torch.float32 else np.int64)
        if host.ndim != 2 or host.shape[1] != 3:
            raise ValueError(f"{what}: expected [n,3], got {host.shape}")
        t = torch.as_tensor(host).to(_device(device))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: expected [n,3], got {tuple(t.shape)}")
    return t.to(dtype).contiguous()


def jitter_cloud(points, colors, *, seed, copies=JITTER_COPIES, radius=JITTER_RADIUS, use_colors=False, device=None) -> DeviceCloud:
    """`copies` rows around every seed point (init_pcd, `pointe*`): row i * copies + k is (x, -y, z + 0.15) of seed point i plus
    offset k, the offsets being shared by all seed points. Colours: colors[i] + 1e-4 u with use_colors, else the ball's."""
    what = "jitter_cloud"
    copies, r, s = _count(copies, what), _radius(radius, what), _seed64(seed)
    pts = _rows3(points, torch.float32, device, what)
    n = _count(pts.shape[0], what)
    _count(n * copies, what)
    col = None
    if use_colors:
        col = _rows3(colors, torch.float32, pts.device, what)
        if col.shape[0] != n or col.device != pts.device:
            raise ValueError(f"{what}: {n} points with {col.shape[0]} colours")
    return _launch(_new_cloud(n * copies, pts.device), "gsr_sample_jitter",
                   lambda p, c: (s, pts.data_ptr(), None if col is None else col.data_ptr(), n, copies, r, p, c))


def sample_mesh(vertices, faces, num_pts, *, seed, device=None, return_triangles=False):
    """num_pts rows uniform over the surface of the triangle mesh (vertices [V,3], faces [F,3] of 0-based indices), then the
    reference's (x, z, y) axis swap, centring on the mean and division by 80 (init_pcd, `shapes`). Triangles are chosen by binary
    search in the normalised float64 running sum of their areas, so one of zero area is never chosen. return_triangles: also the
    [num_pts] int32 tensor of each row's triangle."""
    what = "sample_mesh"
    n, s = _count(num_pts, what), _seed64(seed)
    v = _rows3(vertices, torch.float32, device, what)
    f = _rows3(faces, torch.int32, v.device, what)
    V, F = v.shape[0], f.shape[0]
    if V == 0 or F == 0 or f.device != v.device:
        raise ValueError(f"{what}: a mesh of {V} vertices and {F} faces has no surface")
    _count(F, what)
    dev = v.device
    lib = L.load()
    area = torch.empty(F, dtype=torch.float64, device=dev)
    cloud = _new_cloud(n, dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(lib.gsr_mesh_areas(v.data_ptr(), V, f.data_ptr(), F, area.data_ptr(), stream), "gsr_mesh_areas")
        cdf = torch.cumsum(area, 0)
        cdf = (cdf / cdf[-1]).contiguous()               # a mesh without area: NaN, every row lands in the last triangle
        L.check(lib.gsr_sample_mesh(s, v.data_ptr(), V, f.data_ptr(), F, cdf.data_ptr(), n, cloud.points.data_ptr(),
                                    cloud.colors.data_ptr(), tri.data_ptr(), stream), "gsr_sample_mesh")
        mean = cloud.points.to(torch.float64).mean(dim=0).contiguous()
        L.check(lib.gsr_mesh_center(mean.data_ptr(), n, cloud.points.data_ptr(), stream), "gsr_mesh_center")
    return (cloud, tri) if return_triangles else cloud


def read_obj(path) -> tuple:
    """(vertices [V,3] float64, faces [F,3] int64, 0-based) of a Wavefront OBJ: `v x y z` and `f a b c ...` lines; `a/t/n` forms keep
    the vertex index, negative indices count from the last vertex read so far, polygons become fans around their first corner."""
    vertices, faces = [], []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            tok = line.split()
            if not tok or tok[0] not in ("v", "f"):
                continue
            try:
                if tok[0] == "v":
                    vertices.append([float(tok[1]), float(tok[2]), float(tok[3])])
                    continue
                idx = []
                for t in tok[1:]:
                    k = int(t.split("/")[0])
                    k = k - 1 if k > 0 else len(vertices) + k
                    if k < 0 or k >= len(vertices) or t.split("/")[0] == "0":
                        raise ValueError(f"index {t} with {len(vertices)} vertices")
                    idx.append(k)
                if len(idx) < 3:
                    raise ValueError("a face needs three corners")
            except (ValueError, IndexError) as e:
                raise ValueError(f"read_obj: {path}:{no}: {e}") from e
            faces.extend([idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1))
    return np.array(vertices, np.float64).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3)


class SeededGaussianModel(GaussianModel):
    """GaussianModel with the three samplers the reference's class has, drawn on the device. A checkout derives its
    gs_renderer.GaussianModel from this class and deletes its own init_pcd / init_env_pcd / init_floor_pcd."""
    seed = 0

    def _seed(self, initialize_param: dict) -> int:
        return initialize_param.get("seed", type(self).seed)

    def create_from_cloud(self, cloud: DeviceCloud, require_grad=True, spatial_lr_scale: float = 1):
        """create_from_pcd for a cloud that is on the device already: distCUDA2 and the leaf kernel, no host round trip."""
        pts, col = cloud.points, cloud.colors
        for t in (pts, col):
            if t.device.type != "cuda":
                raise L.GsrError("SeededGaussianModel.create_from_cloud needs its tensors on a cuda (ROCm) device; there is no "
                                 "CPU fallback")
        if pts.dim() != 2 or pts.shape[1] != 3 or col.shape != pts.shape:
            raise ValueError(f"create_from_cloud: points {tuple(pts.shape)} and colours {tuple(col.shape)} must both be [n,3]")
        if (self.max_sh_degree + 1) ** 2 not in (1, 4, 9, 16):
            raise ValueError(f"create_from_cloud: sh_degree {self.max_sh_degree} is not 0..3")
        self.spatial_lr_scale = spatial_lr_scale
        pts = pts.detach().to(torch.float32).contiguous()
        col = col.detach().to(device=pts.device, dtype=torch.float32).contiguous()
        self._create_from_device(pts, col, require_grad, None, pts.device)

    def init_env_pcd(self, initialize_param: dict):
        p = initialize_param
        cloud = sample_env(p["cam_pose_method"], p["scene_box"], seed=self._seed(p), zero_ground=p.get("zero_ground", False),
                           env_init_color=p.get("env_init_color"), num_pts=p.get("num_pts"), device=self.device)
        if cloud is not None:
            self.create_from_cloud(cloud, True, 1)

    def init_floor_pcd(self, initialize_param: dict):
        p = initialize_param
        cloud = sample_floor(p["cam_pose_method"], p["scene_box"], seed=self._seed(p), zero_ground=p.get("zero_ground", False),
                             floor_init_color=p.get("floor_init_color"), num_pts=p.get("num_pts"), device=self.device)
        if cloud is not None:
            self.create_from_cloud(cloud, False, 1)

    def init_pcd(self, initialize_param: dict, exp_path: str = None):
        p = initialize_param
        guided, seed = p["init_guided"], self._seed(p)
        if isinstance(guided, BasicPointCloud):
            self.create_from_pcd(guided, True, 1)
        elif guided == "shapes":
            path = p["init_prompt"]
            if not str(path).lower().endswith(".obj"):
                raise ValueError(f"SeededGaussianModel: init_guided 'shapes' reads OBJ meshes only, not {path!r}")
            vertices, faces = read_obj(path)
            if not len(faces):
                raise ValueError(f"SeededGaussianModel: {path!r} has no faces")
            self.create_from_cloud(sample_mesh(vertices, faces, SHAPES_PTS, seed=seed, device=self.device), True, 1)
        elif guided == "default":
            self.create_from_cloud(sample_ball(p["num_pts"], p["radius"], seed=seed, device=self.device), True, 10)
        elif guided in POINTE_MODES:
            seeds = p.get("init_points")
            if not isinstance(seeds, BasicPointCloud):
                raise ValueError(f"SeededGaussianModel: init_guided {guided!r} needs initialize_param['init_points'], a "
                                 "BasicPointCloud of the Point-E output (Point-E itself is not part of this package)")
            cloud = jitter_cloud(seeds.points, seeds.colors, seed=seed, use_colors=bool(p.get("use_pointe_rgb", False)),
                                 device=self.device)
            self.create_from_cloud(cloud, True, 1)
        elif guided == "obj":
            raise ValueError("SeededGaussianModel: init_guided 'obj' has no point cloud in the reference either (it fails on an "
                             "unbound name); use 'shapes' with an OBJ file")
        elif isinstance(guided, (str, os.PathLike)):
            self.load_ply(guided)
        else:
            raise ValueError(f"SeededGaussianModel: init_guided {guided!r} is neither a mode, a BasicPointCloud nor a path")
