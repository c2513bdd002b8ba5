"""Scene composition: trained objects placed into the scene frame (SceneGaussian.add_objects_to_scene, scene_gaussian.py:318-427,
and final_combine_all, :519-544) -- the step between training the objects and `scene.rasterize_models`.

The reference needs pytorch3d.transforms (Euler angles / quaternions) and e3nn.o3 (Wigner D matrices) for it; here the rotation
helpers and the SH band matrices are ~100 lines of float64 host code that runs once per placement, and the pass over the object
(up to 1.2 M rows x 220 B) is two launches of csrc/compose.hip. What is computed is what the reference INTENDS (SEMANTICS.md
"Object placement"): the view-dependent colour is rotated so that the placed object seen from the correspondingly moved camera
gives the same picture -- the reference's band 1 mixes the colour axis instead, and its repeated placements compound.

    placed = place(model, rotation=(0, 0, 90), scale=[1.2], center=(1.0, 2.0, 0.0))      # -> PlacedObject, a 6-tuple of leaves
    placed, box = add_objects_to_scene([(model, [dict(rotation=..., scale=..., center=...), ...]), ...])
    image, radii, depth_alpha, scales = scene.rasterize_models(settings, placed, means2D)

No CPU fallback: the leaves live on a ROCm device."""
from __future__ import annotations

import ctypes as C
import math
from typing import Iterable, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .scene import LEAVES, _leaves

# ---- rotations (float64, host) ---------------------------------------------------------------------------------------------------


def rotation_matrix(rotation: Sequence[float]) -> np.ndarray:
    """3 numbers: Euler angles in DEGREES, R = Rx(a) Ry(b) Rz(c) (pytorch3d's "XYZ" convention after the reference's np.deg2rad,
    scene_gaussian.py:335, :484). 4 numbers: a quaternion (w, x, y, z) of any non-zero length."""
    r = [float(v) for v in rotation]
    if len(r) == 3:
        a, b, c = (math.radians(v) for v in r)
        ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
        Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]], dtype=np.float64)
        Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]], dtype=np.float64)
        Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]], dtype=np.float64)
        return Rx @ Ry @ Rz
    if len(r) == 4:
        n2 = sum(v * v for v in r)
        if not n2 > 0.0 or not math.isfinite(n2):
            raise ValueError("rotation_matrix: a quaternion of non-zero finite length expected")
        w, x, y, z = r
        s = 2.0 / n2
        return np.array([[1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                         [s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)],
                         [s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]], dtype=np.float64)
    raise ValueError("rotation_matrix: 3 Euler angles (degrees) or a quaternion (w, x, y, z)")


def quaternion_of(R: np.ndarray) -> np.ndarray:
    """The unit quaternion (w, x, y, z) of a rotation matrix, real part >= 0 (the sign does not change what is rendered; it is
    fixed so that every rank computes the same numbers). The largest of the four squared components is the pivot."""
    R = np.asarray(R, dtype=np.float64)
    m00, m11, m22 = R[0, 0], R[1, 1], R[2, 2]
    four = np.array([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22])
    k = int(np.argmax(four))
    if k == 0:
        q = np.array([four[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], four[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], four[2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], four[3]])
    q = q / np.linalg.norm(q)
    if q[0] < 0 or (q[0] == 0 and q[np.nonzero(q)[0][0]] < 0):
        q = -q
    return q + 0.0       # no negative zeros


# ---- SH band matrices --------------------------------------------------------------------------------------------------------------

_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435)


def _sh_bands(d: np.ndarray) -> tuple:
    """The basis functions of bands 1, 2, 3 at unit directions d [n,3], signs and constants included: the colour is
    sum_i k_i Y_i(d) (utils/sh_utils.py:56-102). -> ([n,3], [n,5], [n,7])"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    b1 = np.stack([-_C1 * y, _C1 * z, -_C1 * x], axis=1)
    b2 = np.stack([_C2[0] * xy, _C2[1] * yz, _C2[2] * (2.0 * zz - xx - yy), _C2[3] * xz, _C2[4] * (xx - yy)], axis=1)
    b3 = np.stack([_C3[0] * y * (3.0 * xx - yy), _C3[1] * xy * z, _C3[2] * y * (4.0 * zz - xx - yy),
                   _C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), _C3[4] * x * (4.0 * zz - xx - yy),
                   _C3[5] * z * (xx - yy), _C3[6] * x * (xx - 3.0 * yy)], axis=1)
    return b1, b2, b3


def _directions(n: int = 48) -> np.ndarray:
    """A fixed spread of unit directions (Fibonacci lattice): every band's basis has full, well-conditioned rank on it."""
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - 2.0 * (i + 0.5) / n
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def sh_band_matrices(R: np.ndarray) -> tuple:
    """(M1 [3,3], M2 [5,5], M3 [7,7]) with Y_i(R^T d) = sum_j M_l[i,j] Y_j(d) in the basis above: the coefficients of a
    function rotated by R are k'[j] = sum_i k[i] M_l[i,j]. Each band is solved on its own from the basis evaluated at a fixed
    set of directions (block-diagonal by construction, no random state) and replaced by its nearest orthogonal matrix (the
    bands are orthonormal bases of rotation-invariant spaces, so the exact matrix is orthogonal; the solve is within 1e-15)."""
    R = np.asarray(R, dtype=np.float64)
    if R.shape != (3, 3):
        raise ValueError("sh_band_matrices: a 3x3 rotation matrix expected")
    d = _directions()
    at_d, at_rtd = _sh_bands(d), _sh_bands(d @ R)          # rows of d @ R are R^T d
    out = []
    for A, B in zip(at_d, at_rtd):
        Mt = np.linalg.lstsq(A, B, rcond=None)[0]           # A Mt = B,  Mt[j,i] = M[i,j]
        u, _, vt = np.linalg.svd(Mt.T)
        out.append(u @ vt)
    return tuple(out)


# ---- placement ---------------------------------------------------------------------------------------------------------------------

class PlacementConstants(NamedTuple):
    """What one placement hands to gsr_place, every entry already rounded once to fp32."""
    rs: np.ndarray          # [9]  R S, row-major
    t: np.ndarray           # [3]  the centre
    log_scale: np.ndarray   # [3]
    q: np.ndarray           # [4]  quaternion of R
    m1: np.ndarray          # [9]
    m2: np.ndarray          # [25]
    m3: np.ndarray          # [49]


def _scale3(scale) -> np.ndarray:
    s = np.atleast_1d(np.asarray(scale, dtype=np.float64)).reshape(-1)
    if s.size == 1:
        s = np.repeat(s, 3)
    if s.size != 3 or not np.all(np.isfinite(s)) or not np.all(s > 0):
        raise ValueError("place: scale is 1 or 3 positive numbers")
    return s


def placement_constants(rotation, scale, center) -> PlacementConstants:
    R = rotation_matrix(rotation)
    s = _scale3(scale)
    c = np.asarray(center, dtype=np.float64).reshape(-1)
    if c.size != 3:
        raise ValueError("place: center is 3 numbers")
    m1, m2, m3 = sh_band_matrices(R)
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1), dtype=np.float32)
    return PlacementConstants(f(R * s[None, :]), f(c), f(np.log(s)), f(quaternion_of(R)), f(m1), f(m2), f(m3))


class PlacedObject(tuple):
    """The six leaves of the placed object in scene.LEAVES order (a 6-tuple: `scene.rasterize_models` takes it as a model), plus
    bbox [6] (xyz_min, xyz_max) and t_effective [3] on the device, the three statistics tensors when the model had them, and
    affine = {"T", "R", "S"} as the reference's ObjectArgs keeps them (T on the device: with `ground` its z depends on the data)."""
    bbox: torch.Tensor
    t_effective: torch.Tensor
    affine: dict
    stats: Optional[tuple] = None

    def __getattr__(self, name):
        if name in LEAVES:
            return self[LEAVES.index(name)]
        raise AttributeError(name)


STATS = ("max_radii2D", "xyz_gradient_accum", "denom")


def _checked(t: torch.Tensor, what: str, dev=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise L.GsrError(f"place needs {what} on a cuda (ROCm) device; there is no CPU fallback")
    if t.dtype != torch.float32:
        raise ValueError(f"place: {what} must be fp32")
    if dev is not None and t.device != dev:
        raise ValueError(f"place: {what} is on {t.device}, the model on {dev}")
    return t.detach().contiguous()


@torch.no_grad()
def place(model, rotation, scale, center, ground: bool = True, copy: bool = True) -> PlacedObject:
    """One placement of `model` (an object with GaussianModel's `_xyz ... _features_rest`, or the 6-tuple in scene.LEAVES order):
    rotation = 3 Euler angles in degrees or a quaternion, scale = 1 or 3 numbers, center = the translation; ground: the object
    is set down on z = center[2] (scene_gaussian.py:344-350). The model's tensors are never written; xyz, scaling, rotation and
    f_rest of the result are new tensors, f_dc / opacity / statistics are clones, or with copy=False the model's own storage."""
    consts = placement_constants(rotation, scale, center)
    lv = _leaves(model)
    xyz = _checked(lv[0], "_xyz")
    dev, P = xyz.device, xyz.shape[0]
    scaling, rot, opacity, f_dc, f_rest = (_checked(t, n, dev) for t, n in zip(lv[1:], LEAVES[1:]))
    K = f_rest.shape[1] + 1 if f_rest.dim() == 3 else -1
    if tuple(xyz.shape) != (P, 3) or tuple(scaling.shape) != (P, 3) or tuple(rot.shape) != (P, 4) or \
            tuple(opacity.shape) != (P, 1) or tuple(f_dc.shape) != (P, 1, 3) or tuple(f_rest.shape) != (P, K - 1, 3) or \
            K not in (1, 4, 9, 16):
        raise ValueError("place: xyz [P,3], scaling [P,3], rotation [P,4], opacity [P,1], f_dc [P,1,3], f_rest [P,K-1,3] "
                         "(K in 1, 4, 9, 16) expected")
    if P == 0:
        raise ValueError("place: the model has no Gaussians")
    lib = L.load()
    nbytes = lib.gsr_place_scratch_bytes(P)
    if nbytes == 0:
        raise ValueError(f"place: P = {P} does not fit 32-bit offsets")
    with torch.cuda.device(dev):
        out = [torch.empty_like(t) for t in (xyz, scaling, rot, f_rest)]
        box = torch.empty(9, dtype=torch.float32, device=dev)            # bbox [6] and t_effective [3] in one allocation
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p = L.GsrPlacement()
        p.P, p.K, p.ground = P, K, 1 if ground else 0
        p.xyz, p.scaling, p.rotation = xyz.data_ptr(), scaling.data_ptr(), rot.data_ptr()
        p.opacity, p.features_dc = opacity.data_ptr(), f_dc.data_ptr()
        p.features_rest = f_rest.data_ptr() if K > 1 else None
        p.xyz_out, p.scaling_out, p.rotation_out = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()
        p.features_rest_out = out[3].data_ptr() if K > 1 else None
        for name in PlacementConstants._fields:
            getattr(p, name)[:] = getattr(consts, name).tolist()
        p.bounds, p.t_effective = box.data_ptr(), box.data_ptr() + 6 * 4
        L.check(lib.gsr_place(C.byref(p), scratch.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream), "gsr_place")
    keep = (lambda t: t.clone()) if copy else (lambda t: t)
    res = PlacedObject((out[0], out[1], out[2], keep(opacity), keep(f_dc), out[3]))
    res.bbox, res.t_effective = box[:6], box[6:]
    res.affine = {"T": res.t_effective, "R": torch.tensor([float(v) for v in rotation], dtype=torch.float32),
                  "S": torch.tensor(np.atleast_1d(np.asarray(scale, dtype=np.float32)).reshape(-1))}
    if isinstance(model, PlacedObject):
        res.stats = None if model.stats is None else tuple(keep(t) for t in model.stats)
    elif not isinstance(model, (tuple, list)) and all(hasattr(model, n) for n in STATS):
        res.stats = tuple(keep(getattr(model, n).detach()) for n in STATS)
    return res


def add_objects_to_scene(objects: Iterable, scene_box: Optional[torch.Tensor] = None, ground: bool = True,
                         copy: bool = True) -> tuple:
    """objects: (model, [placement, ...]) pairs, a placement being a dict with rotation / scale / center (the reference's
    `obj.params`). -> (one PlacedObject per placement in the reference's order, scene_box [6] on the device: the running
    min / max over the placed boxes, scene_gaussian.py:382-385, started from `scene_box` if given). Every placement starts from
    the model as given: placing an object twice does not rotate its SH twice. Nothing is read back to the host."""
    placed = []
    for model, params in objects:
        for prm in params:
            get = prm.get if isinstance(prm, dict) else (lambda k, prm=prm: getattr(prm, k))
            placed.append(place(model, get("rotation"), get("scale"), get("center"), ground=ground, copy=copy))
    if not placed:
        raise ValueError("add_objects_to_scene: no placement given")
    dev = placed[0].bbox.device
    box = None if scene_box is None else scene_box.detach().to(device=dev, dtype=torch.float32).clone()
    for po in placed:
        b = po.bbox.to(dev)
        box = b.clone() if box is None else torch.cat((torch.minimum(box[:3], b[:3]), torch.maximum(box[3:], b[3:])))
    return placed, box


def combine(models: Sequence) -> tuple:
    """final_combine_all (scene_gaussian.py:519-544): the concatenated leaves in scene.LEAVES order and, when every model carries
    them, the concatenated statistics (max_radii2D, xyz_gradient_accum, denom), else None."""
    rows = [_leaves(m) if not isinstance(m, PlacedObject) else tuple(m) for m in models]
    leaves = tuple(torch.cat([r[k].detach() for r in rows]) for k in range(6))
    stats = []
    for m in models:
        s = m.stats if isinstance(m, PlacedObject) else \
            (tuple(getattr(m, n).detach() for n in STATS) if all(hasattr(m, n) for n in STATS) else None)
        stats.append(s)
    if any(s is None for s in stats):
        return leaves, None
    return leaves, tuple(torch.cat([s[k] for s in stats]) for k in range(3))
