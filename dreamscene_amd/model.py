"""`GaussianModel`: the container the reference's trainers talk to (gs_renderer.py:166-1105), on the fused ops.

A DreamScene checkout binds it by making `gs_renderer.GaussianModel` a subclass that keeps only its own point-cloud samplers
("The model container"); `scene_gaussian.py` and the trainers then call it unchanged. What each call runs:

  create_from_pcd                     knn.distCUDA2, then ONE launch that writes the six leaves (csrc/model.hip, K_init)
  training_setup                      optim.FusedAdam over the reference's seven groups, and the four learning-rate schedules
  add_densification_stats(_div)       one launch on `viewspace_point_tensor.grad` (K_stats): no boolean-mask indexing, no `nonzero`
  reset_opacity                       one launch (K_reset) and the reference's replacement of the optimizer's parameter
  densify_and_prune / prune /
  prune_points / prune_gaussians      densify.* and densify.importance_prune_mask
  save_ply / load_ply                 ply
  extract_fields                      fields.extract_fields: five launches and one host read (csrc/fields.hip)
  max_radii2D / xyz_gradient_accum /
  denom                               views of the `densify.DensifyStats` at `self.stats`, which `stats.collect(...)` can also fill
                                      from inside the rasterizer backward

The remaining methods are torch one-liners, or torch restatements that exist so that code calling them keeps working
(densify_and_clone, densify_and_split, densification_postfix, cat_tensors_to_optimizer, _prune_optimizer,
replace_tensor_to_optimizer): they are not on any hot path here. Not provided: the host-side samplers `init_pcd`, `init_env_pcd`,
`init_floor_pcd`, which a checkout keeps (the constructor calls them when a subclass has them; `pointcloud.SeededGaussianModel` is
a subclass that draws them on the device from a seed).
Decisions the reference leaves open: SEMANTICS.md section 15. No CPU fallback: the kernels refuse tensors that are not on a ROCm
device with `GsrError`.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import densify as D
from . import knn
from . import ply
from .optim import FusedAdam

OPACITY_RESET_CAP = 0.01          # reset_opacity: min(sigmoid(x), 0.01)
INITIAL_OPACITY = 0.1             # create_from_pcd: every row starts at inverse_sigmoid(0.1)
_LEAVES = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
           ("scaling", "_scaling"), ("rotation", "_rotation"))
_SAMPLER_MODES = ("shapes", "default", "pointe", "pointe_330k", "pointe_825k", "obj")


class BasicPointCloud(NamedTuple):
    points: np.ndarray
    colors: np.ndarray
    normals: np.ndarray


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """step -> learning rate: log-linear from lr_init to lr_final over max_steps, times an optional sine warm-up from
    lr_delay_mult over lr_delay_steps. numpy double arithmetic."""
    def lr_at(step):
        if lr_init == lr_final:
            return lr_init
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        warm = 1.0
        if lr_delay_steps > 0:
            warm = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
        t = np.clip(step / max_steps, 0, 1)
        return warm * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)
    return lr_at


def _rotation_matrices(q: torch.Tensor) -> torch.Tensor:
    """[N,4] quaternions (real part first, any length) -> [N,3,3] rotation matrices."""
    w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(1)
    rows = (1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y))
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def _covariance6(scaling: torch.Tensor, scaling_modifier, rotation: torch.Tensor) -> torch.Tensor:
    """The upper triangle (xx, xy, xz, yy, yz, zz) of R S S^T R^T, [N,6]."""
    m = _rotation_matrices(rotation) * (scaling_modifier * scaling)[:, None, :]
    cov = m @ m.transpose(1, 2)
    return torch.stack((cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]), dim=1)


def _on_rocm(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.device.type != "cuda":
        raise L.GsrError(f"GaussianModel.{what} needs its tensors on a cuda (ROCm) device; there is no CPU fallback")
    return t


def _resolve_cut(total: int, cut_start, cut_end) -> tuple:
    """(first row, rows) of `[cut_start:cut_end]` over `total` rows, `cut_end` of None or 0 meaning "to the end" (the reference
    tests `if cut_end:`)."""
    start, stop, _ = slice(cut_start, cut_end if cut_end else None).indices(total)
    return start, max(0, stop - start)


class GaussianModel:
    device = "cuda"               # where create_from_pcd / load_ply put the leaves

    def setup_functions(self):
        self.scaling_activation = torch.exp
        self.scaling_inverse_activation = torch.log
        self.covariance_activation = _covariance6
        self.opacity_activation = torch.sigmoid
        self.inverse_opacity_activation = inverse_sigmoid
        self.rotation_activation = torch.nn.functional.normalize

    def __init__(self, initialize_param: dict, gaussian_class: str, exp_path: str = None):
        self.active_sh_degree = 0
        self.max_sh_degree = initialize_param["sh_degree"]
        self._clear()
        self.setup_functions()
        if gaussian_class == "object":
            if exp_path is None:
                raise ValueError("GaussianModel: gaussian_class 'object' needs an exp_path")
            self._init_object(initialize_param, exp_path)
        elif gaussian_class == "scene":
            pass
        elif gaussian_class in ("tmp", "restore"):
            self.load_ply(initialize_param["path"], gaussian_class == "restore")
        elif gaussian_class in ("env", "floor"):
            name = f"init_{gaussian_class}_pcd"
            sampler = getattr(self, name, None)
            if sampler is None:
                raise ValueError(f"GaussianModel: gaussian_class {gaussian_class!r} draws its point cloud on the host; a "
                                 f"subclass has to provide {name}(initialize_param)")
            sampler(initialize_param)
        else:
            raise ValueError(f"GaussianModel: unknown gaussian_class {gaussian_class!r} (object, scene, tmp, restore; env and "
                             "floor with a subclass that provides init_env_pcd / init_floor_pcd)")

    def _clear(self):
        self._xyz = torch.empty(0)
        self._features_dc = torch.empty(0)
        self._features_rest = torch.empty(0)
        self._scaling = torch.empty(0)
        self._rotation = torch.empty(0)
        self._opacity = torch.empty(0)
        self._background = torch.empty(0)
        self.stats = D.DensifyStats(0, "cpu")
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0

    def _init_object(self, initialize_param: dict, exp_path: str):
        sampler = getattr(self, "init_pcd", None)
        if sampler is not None:                      # a checkout's subclass keeps the reference's sampler, all modes
            sampler(initialize_param, exp_path)
            return
        guided = initialize_param["init_guided"]
        if isinstance(guided, BasicPointCloud):
            self.create_from_pcd(guided, True, 1)
        elif isinstance(guided, str) and guided not in _SAMPLER_MODES:
            self.load_ply(guided)
        else:
            raise ValueError(f"GaussianModel: init_guided {guided!r} draws its point cloud on the host; a subclass has to "
                             "provide init_pcd(initialize_param, exp_path). Without one, init_guided is a BasicPointCloud or "
                             "the path of a PLY")

    # ---- the densification statistics: views of self.stats ------------------------------------------------------------------

    @property
    def max_radii2D(self) -> torch.Tensor:
        return self.stats.max_radii2D

    @max_radii2D.setter
    def max_radii2D(self, value: torch.Tensor):
        self.stats.max_radii2D = value.detach().reshape(-1).to(torch.float32)

    @property
    def xyz_gradient_accum(self) -> torch.Tensor:
        return self.stats.xyz_gradient_accum[:, None]

    @xyz_gradient_accum.setter
    def xyz_gradient_accum(self, value: torch.Tensor):
        self.stats.xyz_gradient_accum = value.detach().reshape(-1).to(torch.float32)

    @property
    def denom(self) -> torch.Tensor:
        return self.stats.denom[:, None]

    @denom.setter
    def denom(self, value: torch.Tensor):
        self.stats.denom = value.detach().reshape(-1).to(torch.float32)

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------

    def capture(self):
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
                self._opacity, self.max_radii2D, self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(),
                self.spatial_lr_scale)

    def restore(self, model_args, training_args):
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity,
         max_radii2D, xyz_gradient_accum, denom, opt_dict, self.spatial_lr_scale) = model_args
        if self._background.numel() == 0:
            self._background = nn.Parameter(torch.zeros((3, 1, 1), device=self._xyz.device))
        self.training_setup(training_args)
        self.max_radii2D = max_radii2D
        self.xyz_gradient_accum = xyz_gradient_accum
        self.denom = denom
        self.optimizer.load_state_dict(opt_dict)

    # ---- torch one-liners ----------------------------------------------------------------------------------------------------

    @property
    def get_scaling(self):
        return self.scaling_activation(self._scaling)

    @property
    def get_rotation(self):
        return self.rotation_activation(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_background(self):
        return torch.sigmoid(self._background)

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return self.opacity_activation(self._opacity)

    def get_covariance(self, scaling_modifier=1):
        return self.covariance_activation(self.get_scaling, scaling_modifier, self._rotation)

    @torch.no_grad()
    def extract_fields(self, resolution=128, num_blocks=16, relax_ratio=1.5):
        """The opacity-weighted density on a resolution^3 grid, fp32 on the device; sets `center` (fp32 [3], device) and `scale`
        (float), the normalisation of the kept rows, as the reference does."""
        from . import fields
        result = fields.extract_fields(self._xyz, self._opacity, self._scaling, self._rotation, resolution, num_blocks, relax_ratio)
        self.center, self.scale = result.center, result.scale
        return result.occ

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def _leaves(self):
        return (self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation)

    def active_grad(self):
        for t in self._leaves() + (self._background,):
            t.requires_grad = True

    def deactive_grad(self):
        for t in self._leaves() + (self._background,):
            t.requires_grad = False

    def free_memory(self):
        self._clear()

    # ---- initialisation ------------------------------------------------------------------------------------------------------

    def create_from_pcd(self, pcd: BasicPointCloud, require_grad=True, spatial_lr_scale: float = 1, *,
                        dist2: Optional[torch.Tensor] = None):
        """dist2 [P]: the mean squared distances to use instead of running knn.distCUDA2 on the points."""
        self.spatial_lr_scale = spatial_lr_scale
        dev = torch.device(self.device)
        # float64 numpy is rounded to fp32 once on the host
        host = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a), dtype=np.float32)).reshape(-1, 3)
        points, colors = host(pcd.points), host(pcd.colors)
        P, K = points.shape[0], (self.max_sh_degree + 1) ** 2
        if colors.shape[0] != P:
            raise ValueError(f"create_from_pcd: {P} points with {colors.shape[0]} colours")
        if K not in (1, 4, 9, 16):
            raise ValueError(f"create_from_pcd: sh_degree {self.max_sh_degree} is not 0..3")
        self._create_from_device(points.to(dev), colors.to(dev), require_grad, dist2, dev)

    def _create_from_device(self, points: torch.Tensor, colors: torch.Tensor, require_grad, dist2: Optional[torch.Tensor], dev):
        """The six leaves from contiguous fp32 [P,3] points and colours on the device `dev` (create_from_pcd's second half; what
        pointcloud.SeededGaussianModel.create_from_cloud runs on a cloud that never was on the host)."""
        P, K = points.shape[0], (self.max_sh_degree + 1) ** 2
        if dist2 is None:
            dist2 = knn.distCUDA2(points)
        else:
            dist2 = _on_rocm(torch.as_tensor(dist2), "create_from_pcd").to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if dist2.shape[0] != P:
                raise ValueError(f"create_from_pcd: dist2 has {dist2.shape[0]} entries for {P} points")
        _on_rocm(points, "create_from_pcd")
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out = dict(xyz=new(P, 3), f_dc=new(P, 1, 3), f_rest=new(P, K - 1, 3), opacity=new(P, 1), scaling=new(P, 3),
                   rotation=new(P, 4))
        if P:
            # one value for every row, formed once on the host in fp32
            tenth = np.float32(INITIAL_OPACITY)
            logit = float(np.log(tenth / (np.float32(1) - tenth), dtype=np.float32))
            lib = L.load()
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                L.check(lib.gsr_model_init(points.data_ptr(), colors.data_ptr(), dist2.data_ptr(), P, K, logit,
                                           out["xyz"].data_ptr(), out["f_dc"].data_ptr(),
                                           out["f_rest"].data_ptr() if K > 1 else None, out["scaling"].data_ptr(),
                                           out["rotation"].data_ptr(), out["opacity"].data_ptr(), stream), "gsr_model_init")
            for t in out.values():
                torch.autograd.graph.increment_version(t)
        for name, attr in _LEAVES:
            setattr(self, attr, nn.Parameter(out[name].requires_grad_(require_grad)))
        self._background = nn.Parameter(torch.zeros((3, 1, 1), device=dev).requires_grad_(require_grad))
        self.stats = D.DensifyStats(P, dev)

    def load_ply(self, path, require_grad=True):
        dev = torch.device(self.device)
        d = ply.load_ply(path, self.max_sh_degree)
        leaf = lambda a: nn.Parameter(torch.tensor(a, dtype=torch.float32, device=dev).requires_grad_(require_grad))
        self._xyz, self._features_dc, self._features_rest = leaf(d["xyz"]), leaf(d["features_dc"]), leaf(d["features_rest"])
        self._opacity, self._scaling, self._rotation = leaf(d["opacity"]), leaf(d["scaling"]), leaf(d["rotation"])
        self._background = nn.Parameter(torch.zeros((3, 1, 1), device=dev).requires_grad_(require_grad))
        self.stats = D.DensifyStats(self._xyz.shape[0], dev)
        self.active_sh_degree = self.max_sh_degree

    def construct_list_of_attributes(self):
        return ply.attribute_names(self._features_rest.shape[1] * self._features_rest.shape[2] // 3)

    def save_ply(self, path):
        host = [t.detach().cpu().numpy() for t in (self._xyz, self._features_dc, self._features_rest, self._opacity,
                                                   self._scaling, self._rotation)]          # each leaf moves once
        ply.save_ply(path, *host)

    # ---- optimizer and schedules ---------------------------------------------------------------------------------------------

    def training_setup(self, training_args):
        a = training_args
        self.percent_dense = a.percent_dense
        P, dev = self._xyz.shape[0], self._xyz.device
        if self.stats.max_radii2D.shape[0] != P or self.stats.max_radii2D.device != dev:
            self.stats = D.DensifyStats(P, dev)
        else:
            self.stats.xyz_gradient_accum = torch.zeros(P, dtype=torch.float32, device=dev)
            self.stats.denom = torch.zeros(P, dtype=torch.float32, device=dev)
        position_lr = a.position_lr_init * self.spatial_lr_scale
        groups = [
            {"params": [self._xyz], "lr": position_lr, "name": "xyz"},
            {"params": [self._features_dc], "lr": a.feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": a.feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": a.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": a.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": a.rotation_lr, "name": "rotation"},
            {"params": [self._background], "lr": a.feature_lr, "name": "background"},
        ]
        self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
        schedule = lambda first, last: get_expon_lr_func(lr_init=first, lr_final=last, lr_delay_mult=a.position_lr_delay_mult,
                                                         max_steps=a.iterations)
        self.xyz_scheduler_args = schedule(position_lr, a.position_lr_final * self.spatial_lr_scale)
        self.rotation_scheduler_args = schedule(a.rotation_lr, a.rotation_lr_final)
        self.scaling_scheduler_args = schedule(a.scaling_lr, a.scaling_lr_final)
        self.feature_scheduler_args = schedule(a.feature_lr, a.feature_lr_final)

    def _group(self, name: str) -> Optional[dict]:
        for group in self.optimizer.param_groups:
            if group["name"] == name:
                return group
        return None

    def _set_lr(self, name: str, schedule, iteration):
        group = self._group(name)
        if group is None:
            return None
        group["lr"] = lr = schedule(iteration)
        return lr

    def update_learning_rate(self, iteration):
        return self._set_lr("xyz", self.xyz_scheduler_args, iteration)

    def update_feature_learning_rate(self, iteration):
        return self._set_lr("f_dc", self.feature_scheduler_args, iteration)

    def update_rotation_learning_rate(self, iteration):
        return self._set_lr("rotation", self.rotation_scheduler_args, iteration)

    def update_scaling_learning_rate(self, iteration):
        return self._set_lr("scaling", self.scaling_scheduler_args, iteration)

    # ---- per-step statistics -------------------------------------------------------------------------------------------------

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        self.add_densification_stats_div(viewspace_point_tensor, update_filter, 0, None)

    def add_densification_stats_div(self, viewspace_point_tensor, update_filter, cut_start, cut_end=None):
        grad = viewspace_point_tensor.grad
        if grad is None:
            raise ValueError("add_densification_stats: viewspace_point_tensor has no .grad (call it after backward, on the "
                             "tensor that was handed to the rasterizer as means2D)")
        if grad.dim() != 2 or grad.shape[1] != 3 or grad.dtype != torch.float32:
            raise ValueError(f"add_densification_stats: the gradient must be fp32 [P,3], got {tuple(grad.shape)} {grad.dtype}")
        if update_filter.dtype not in (torch.bool, torch.uint8):
            raise ValueError("add_densification_stats: update_filter must be a bool or uint8 mask")
        update_filter = update_filter.reshape(-1)
        start, n = _resolve_cut(grad.shape[0], cut_start, cut_end)
        accum, denom = self.stats.xyz_gradient_accum, self.stats.denom
        if update_filter.shape[0] != n or accum.shape[0] != n:
            raise ValueError(f"add_densification_stats: the cut [{cut_start}:{cut_end}] of {grad.shape[0]} rows has {n} rows, "
                             f"update_filter {update_filter.shape[0]} and the model {accum.shape[0]}")
        for t in (grad, update_filter, accum, denom):
            _on_rocm(t, "add_densification_stats")
        if n == 0:
            return
        grad, update_filter = grad.contiguous(), update_filter.contiguous()
        dev = accum.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            L.check(L.load().gsr_densify_stats(grad.data_ptr(), grad.shape[0], update_filter.data_ptr(), start, n,
                                               accum.data_ptr(), denom.data_ptr(), stream), "gsr_densify_stats")
        torch.autograd.graph.increment_version(accum)
        torch.autograd.graph.increment_version(denom)

    # ---- surgery -------------------------------------------------------------------------------------------------------------

    @torch.no_grad()
    def reset_opacity(self):
        if self.optimizer is None:
            raise ValueError("reset_opacity: the model has no optimizer (call training_setup first)")
        group = self._group("opacity")
        old = _on_rocm(group["params"][0], "reset_opacity")
        if old.dtype != torch.float32 or not old.is_contiguous():
            raise ValueError("reset_opacity: the opacity parameter must be contiguous fp32")
        state = self.optimizer.state.get(old, None)
        moments = [None, None]
        if state is not None and "exp_avg" in state:
            for k, name in enumerate(("exp_avg", "exp_avg_sq")):
                m = state[name]
                if m.shape != old.shape or m.dtype != torch.float32 or m.device != old.device:
                    raise ValueError(f"reset_opacity: {name} of 'opacity' does not match its parameter")
                if not m.is_contiguous():
                    m = state[name] = m.contiguous()
                moments[k] = m
        new = torch.empty_like(old, requires_grad=False)
        P, dev = old.numel(), old.device
        if P:
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                L.check(L.load().gsr_opacity_reset(old.data_ptr(), P, OPACITY_RESET_CAP, new.data_ptr(),
                                                   None if moments[0] is None else moments[0].data_ptr(),
                                                   None if moments[1] is None else moments[1].data_ptr(), stream),
                        "gsr_opacity_reset")
            for t in [new] + [m for m in moments if m is not None]:
                torch.autograd.graph.increment_version(t)
        fresh = nn.Parameter(new.requires_grad_(True))
        if state is not None:                      # the same state object, `step` kept, under the new key
            del self.optimizer.state[old]
            self.optimizer.state[fresh] = state
        group["params"][0] = fresh
        self._opacity = fresh

    def _adopt(self, tensors: dict):
        for name, attr in _LEAVES:
            setattr(self, attr, tensors[name])

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, *, seed: Optional[int] = None,
                          noise: Optional[torch.Tensor] = None, N: int = 2):
        """seed / noise / N: densify.densify_and_prune's (the split's random numbers; seed=None draws one)."""
        self._adopt(D.densify_and_prune(self.optimizer, self.stats, max_grad, min_opacity, extent, max_screen_size,
                                        percent_dense=self.percent_dense, N=N, seed=seed, noise=noise))

    def prune(self, min_opacity, extent, max_screen_size):
        self._adopt(D.prune(self.optimizer, self.stats, min_opacity, extent, max_screen_size))

    def prune_points(self, mask):
        self._adopt(D.prune_points(self.optimizer, self.stats, mask))

    def prune_gaussians(self, percent: float, important_score) -> None:
        self.prune_points(D.importance_prune_mask(important_score, percent))

    # ---- torch restatements of the surgery's building blocks (not hot: densify_and_prune does not go through them) -------------

    def _model_groups(self):
        return [g for g in self.optimizer.param_groups if g["name"] != "background"]

    def _swap_parameter(self, group: dict, tensor: torch.Tensor, moments=None) -> nn.Parameter:
        """Put `tensor` in place of the group's parameter; its Adam state (if any) moves to the new key, with `moments` (m1, m2)."""
        old = group["params"][0]
        fresh = nn.Parameter(tensor.requires_grad_(True))
        state = self.optimizer.state.get(old, None)
        if state is not None:
            if moments is not None:
                state["exp_avg"], state["exp_avg_sq"] = moments
            del self.optimizer.state[old]
            self.optimizer.state[fresh] = state
        group["params"][0] = fresh
        return fresh

    def _state_moments(self, group: dict):
        state = self.optimizer.state.get(group["params"][0], None)
        return None if state is None else (state["exp_avg"], state["exp_avg_sq"])

    def replace_tensor_to_optimizer(self, tensor, name):
        out = {}
        for group in self._model_groups():
            if group["name"] == name:
                zeros = (torch.zeros_like(tensor), torch.zeros_like(tensor))
                out[name] = self._swap_parameter(group, tensor, zeros if self._state_moments(group) is not None else None)
        return out

    def _prune_optimizer(self, mask):
        out = {}
        for group in self._model_groups():
            m = self._state_moments(group)
            kept = None if m is None else (m[0][mask], m[1][mask])
            out[group["name"]] = self._swap_parameter(group, group["params"][0].detach()[mask], kept)
        return out

    def cat_tensors_to_optimizer(self, tensors_dict):
        out = {}
        for group in self._model_groups():
            if len(group["params"]) != 1:
                raise ValueError(f"cat_tensors_to_optimizer: group {group['name']!r} must hold one parameter")
            extra = tensors_dict[group["name"]].detach()
            m = self._state_moments(group)
            grown = None if m is None else tuple(torch.cat((t, torch.zeros_like(extra)), dim=0) for t in m)
            out[group["name"]] = self._swap_parameter(group, torch.cat((group["params"][0].detach(), extra), dim=0), grown)
        return out

    def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling, new_rotation):
        self._adopt(self.cat_tensors_to_optimizer({"xyz": new_xyz, "f_dc": new_features_dc, "f_rest": new_features_rest,
                                                   "opacity": new_opacities, "scaling": new_scaling, "rotation": new_rotation}))
        self.stats = D.DensifyStats(self._xyz.shape[0], self._xyz.device)

    def _prune_points_torch(self, mask):
        keep = ~mask
        kept_stats = [t[keep] for t in self.stats.tensors()]
        self._adopt(self._prune_optimizer(keep))
        self.stats.replace(*kept_stats)

    @torch.no_grad()
    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2):
        P = self._xyz.shape[0]
        padded = torch.zeros(P, device=self._xyz.device)
        padded[:grads.shape[0]] = grads.reshape(-1)
        scale = self.get_scaling
        chosen = (padded >= grad_threshold) & (scale.max(dim=1).values > self.percent_dense * scene_extent)
        std = scale[chosen].repeat(N, 1)
        offset = torch.normal(mean=torch.zeros_like(std), std=std)
        rot = _rotation_matrices(self._rotation[chosen]).repeat(N, 1, 1)
        self.densification_postfix(
            torch.bmm(rot, offset[:, :, None])[:, :, 0] + self._xyz[chosen].repeat(N, 1),
            self._features_dc[chosen].repeat(N, 1, 1), self._features_rest[chosen].repeat(N, 1, 1),
            self._opacity[chosen].repeat(N, 1), self.scaling_inverse_activation(std / (0.8 * N)),
            self._rotation[chosen].repeat(N, 1))
        children = torch.zeros(N * int(chosen.sum()), dtype=torch.bool, device=chosen.device)
        self._prune_points_torch(torch.cat((chosen, children)))

    @torch.no_grad()
    def densify_and_clone(self, grads, grad_threshold, scene_extent):
        chosen = (torch.norm(grads, dim=-1) >= grad_threshold) & \
            (self.get_scaling.max(dim=1).values <= self.percent_dense * scene_extent)
        self.densification_postfix(self._xyz[chosen], self._features_dc[chosen], self._features_rest[chosen],
                                   self._opacity[chosen], self._scaling[chosen], self._rotation[chosen])
