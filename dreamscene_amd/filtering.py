"""3D Gaussian filtering: `gaussian_filtering` -> `prune_list` -> `calculate_v_imp_score` -> `GaussianModel.prune_gaussians` of the
reference (scene_gaussian.py:1046-1103, gs_renderer.py:1082-1087; called at object_trainer.py:431, :450 and by compress_objects),
on an exact k-th value select that stays in device memory (csrc/select.hip; SEMANTICS.md section 16).

  kth_value               the value torch.sort(x)[0][k] has, as a 0-dim device tensor: six launches, no host read
  calculate_v_imp_score   (volume / volume at 90 % of the descending order) ** v_pow * importance: six launches
  importance_prune_mask   everything at or below the value at int(percent * (n - 1)) of the ascending order: six launches
  importance_filter       both in one call, ten launches; the two thresholds never leave device memory (capturable)
  prune_list              the score sum over the cameras, through views.importance_scores
  gaussian_filtering      the reference's function; ends in object_gs.prune_points(mask)

A DreamScene checkout binds the last three by name. `densify.v_importance`, `densify.
importance_prune_mask` and `GaussianModel.prune_gaussians` keep their torch.kthvalue form. No CPU fallback: tensors that are not on
a ROCm device are refused with `GsrError`.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L

# csrc/select.hip's launch shape (tests/test_filtering.py holds the two files together): the sizes at which the kernels take
# another path are multiples of these
WAVE = 64                          # lanes a wave
BLOCK = 256                        # threads a block
BLOCK_ITEMS = 2048                 # elements a block takes per trip of its stride loop
MAX_BLOCKS = 1024                  # the grid's cap: more than MAX_BLOCKS * BLOCK_ITEMS elements and the loop runs twice
KTH_VALUE_LAUNCHES = 6             # clear, four passes, finish
IMPORTANCE_FILTER_LAUNCHES = 10    # clear, volume + pass, 3 passes, v + pass, 3 passes, mask
VOLUME_RANK_FRACTION = 0.9         # calculate_v_imp_score: sorted_descending[int(n * 0.9)]


def volume_rank(n: int) -> int:
    """The ascending 0-based rank of the reference's `sorted_volume_descending[int(n * 0.9)]`."""
    return n - 1 - int(n * VOLUME_RANK_FRACTION)


def threshold_rank(n: int, percent: float) -> int:
    """prune_gaussians' `int(percent * (n - 1))` of the ascending order."""
    return int(percent * (n - 1))


def _rows(n: int, what: str) -> int:
    if n <= 0:
        raise ValueError(f"{what}: no rows (n == 0)")
    if n > 2 ** 31 - 1:
        raise ValueError(f"{what}: {n} rows do not fit an int32")
    return n


def _percent(percent: float, what: str) -> float:
    percent = float(percent)
    if not 0.0 <= percent <= 1.0:                  # a NaN fails both comparisons
        raise ValueError(f"{what}: percent {percent} is outside [0, 1]")
    return percent


def _on_rocm(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.device.type != "cuda":
        raise L.GsrError(f"filtering.{what} needs its tensors on a cuda (ROCm) device, got one on {t.device}; there is no CPU "
                         "fallback")
    return t


def _fp32(t: torch.Tensor, shape: Tuple[int, ...], what: str, dev=None) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32:
        raise ValueError(f"filtering.{what} must be fp32, got {t.dtype}")
    if dev is not None and t.device != dev:
        raise ValueError(f"filtering.{what} is on {t.device}, the other tensors on {dev}")
    return t.reshape(shape).contiguous()


def _scratch(lib, n: int, dev, scratch: Optional[torch.Tensor]) -> Tuple[torch.Tensor, int]:
    need = int(lib.gsr_select_scratch_bytes(n))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif scratch.device != dev or scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < need:
        raise ValueError(f"filtering: scratch must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
    return scratch, scratch.numel()


def scratch_bytes(n: int) -> int:
    """Bytes of scratch a call on n elements needs (the `scratch=` of kth_value and importance_filter)."""
    return int(L.load().gsr_select_scratch_bytes(_rows(int(n), "scratch_bytes")))


@torch.no_grad()
def kth_value(x: torch.Tensor, k: int, *, descending: bool = False, out: Optional[torch.Tensor] = None,
              scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.sort(x.reshape(-1), descending=descending)[0][k] as a 0-dim device tensor (`out` if given), exactly; the host reads
    nothing. -0 and +0 are equal, a NaN sorts after +inf (first when descending) and comes back as the quiet NaN.
    scratch: a uint8 tensor of scratch_bytes(n) to use instead of allocating one; its contents do not matter."""
    n = _rows(x.numel(), "kth_value")
    k = int(k)
    if not 0 <= k < n:
        raise ValueError(f"kth_value: k = {k} is outside [0, {n})")
    _on_rocm(x, "kth_value")
    x = _fp32(x, (-1,), "kth_value: x")
    dev = x.device
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=dev)
    elif out.device != dev or out.dtype != torch.float32 or out.numel() != 1:
        raise ValueError(f"kth_value: out must be one fp32 element on {dev}")
    lib = L.load()
    scratch, nbytes = _scratch(lib, n, dev, scratch)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(lib.gsr_kth_value(x.data_ptr(), n, n - 1 - k if descending else k, out.data_ptr(), scratch.data_ptr(), nbytes,
                                  stream), "gsr_kth_value")
    torch.autograd.graph.increment_version(out)
    return out


def _filter(what, scaling, activated, imp, v_pow, v_in, percent, want_v, want_count, scratch):
    """The three forms of gsr_importance_filter. -> (mask or None, v_list or None, n_pruned or None)."""
    score, cut = scaling is not None, percent is not None
    first = scaling if score else v_in
    n = _rows(first.shape[0] if score and first.dim() == 2 else first.numel(), what)
    if cut:
        percent = _percent(percent, what)
    _on_rocm(first, what)
    dev = first.device
    if score:
        if scaling.dim() != 2 or scaling.shape[1] != 3:
            raise ValueError(f"filtering.{what}: scaling must be [P,3], got {tuple(scaling.shape)}")
        if imp.numel() != n:
            raise ValueError(f"filtering.{what}: {imp.numel()} importance scores for {n} rows")
        _on_rocm(imp, what)
        scaling, imp = _fp32(scaling, (n, 3), f"{what}: scaling"), _fp32(imp, (n,), f"{what}: imp_list", dev)
        v = torch.empty(n, dtype=torch.float32, device=dev) if want_v else None
    else:
        v = _fp32(v_in, (n,), f"{what}: v_list")
    mask = torch.empty(n, dtype=torch.bool, device=dev) if cut else None
    count = torch.empty((), dtype=torch.int32, device=dev) if cut and want_count else None
    lib = L.load()
    scratch, nbytes = _scratch(lib, n, dev, scratch)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(lib.gsr_importance_filter(ptr(scaling), 1 if activated else 0, ptr(imp), n, float(v_pow) if score else 0.0,
                                          volume_rank(n) if score else 0, threshold_rank(n, percent) if cut else 0, ptr(mask),
                                          ptr(v), ptr(count), scratch.data_ptr(), nbytes, stream), "gsr_importance_filter")
    for t in (mask, count) + ((v,) if score else ()):
        if t is not None:
            torch.autograd.graph.increment_version(t)
    return mask, v, count


@torch.no_grad()
def calculate_v_imp_score(gaussians_or_scaling, imp_list: torch.Tensor, v_pow: float) -> torch.Tensor:
    """scene_gaussian.py:1046-1061. gaussians_or_scaling: a model with `get_scaling`, or the activated scaling [P,3] itself."""
    scaling = gaussians_or_scaling if isinstance(gaussians_or_scaling, torch.Tensor) else gaussians_or_scaling.get_scaling
    return _filter("calculate_v_imp_score", scaling, True, imp_list, v_pow, None, None, True, False, None)[1]


@torch.no_grad()
def importance_prune_mask(v_list: torch.Tensor, percent: float) -> torch.Tensor:
    """The mask GaussianModel.prune_gaussians hands to prune_points (gs_renderer.py:1082-1087): bool [n], True = remove."""
    return _filter("importance_prune_mask", None, True, None, 0.0, v_list, percent, False, False, None)[0]


class FilterResult(tuple):
    """(mask, v_list, n_pruned): bool [P], fp32 [P], and the number of True entries as a 0-dim int32 DEVICE tensor."""
    mask = property(lambda self: self[0])
    v_list = property(lambda self: self[1])
    n_pruned = property(lambda self: self[2])


@torch.no_grad()
def importance_filter(scaling: torch.Tensor, imp_list: torch.Tensor, v_pow: float, percent: float, *, activated: bool = True,
                      scratch: Optional[torch.Tensor] = None) -> FilterResult:
    """calculate_v_imp_score and importance_prune_mask in one call: ten launches, nothing read by the host (the call can be
    captured in a graph). scaling [P,3]: the activated scaling, or with activated=False the raw log-scale (`_scaling`; expf is
    applied in the kernel)."""
    return FilterResult(_filter("importance_filter", scaling, activated, imp_list, v_pow, None, percent, True, True, scratch))


def _score_settings(object_gs, cameras: Sequence, bg_color: torch.Tensor) -> list:
    """score_render's settings (scene_gaussian.py:581-599: scaling_modifier 1, the model's active SH degree, score_flag) for
    cameras with RCamera's attributes; settings that already have score_flag=True pass through."""
    from .rasterizer import GaussianRasterizationSettings
    dev = object_gs.get_xyz.device
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=dev)
    out = []
    for cam in cameras:
        if hasattr(cam, "score_flag"):
            if not cam.score_flag:
                raise ValueError("prune_list: settings must have score_flag=True")
            out.append(cam)
            continue
        out.append(GaussianRasterizationSettings(
            image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
            tanfovy=math.tan(cam.FoVy * 0.5), bg=t(bg_color), scale_modifier=1.0, viewmatrix=t(cam.world_view_transform),
            projmatrix=t(cam.full_proj_transform), sh_degree=int(object_gs.active_sh_degree), campos=t(cam.camera_center),
            prefiltered=False, score_flag=True))
    return out


@torch.no_grad()
def prune_list(object_gs, cameras: Sequence, bg_color: torch.Tensor, *, context=None) -> torch.Tensor:
    """scene_gaussian.py:1063-1079: the sum over the cameras of every Gaussian's importance score, [P] fp32. cameras: objects
    with RCamera's attributes (the reference's `loadSphereCam(pose_args)`), or rasterizer settings with score_flag=True."""
    from . import views
    cameras = list(cameras)
    if not cameras:
        raise ValueError("prune_list: no cameras")
    _rows(object_gs.get_xyz.shape[0], "prune_list")
    _on_rocm(object_gs.get_xyz, "prune_list")
    return views.importance_scores(_score_settings(object_gs, cameras, bg_color), object_gs.get_xyz.detach(),
                                   object_gs.get_opacity.detach(), shs=object_gs.get_features.detach(),
                                   scales=object_gs.get_scaling.detach(), rotations=object_gs.get_rotation.detach(),
                                   context=context)


@torch.no_grad()
def gaussian_filtering(object_gs, cameras: Sequence, bg_color: torch.Tensor, v_pow: float, prune_decay: float,
                       prune_percent: float, *, context=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """scene_gaussian.py:1081-1103, with the cameras in place of `renderer, pose_args`. Removes the rows from `object_gs` (through
    its prune_points) and returns (mask [P] bool over the rows as they were, the score sum [P])."""
    prune_decay_i = 1
    percent = _percent((prune_decay ** prune_decay_i) * prune_percent, "gaussian_filtering")
    _rows(object_gs.get_xyz.shape[0], "gaussian_filtering")
    imp_list = prune_list(object_gs, cameras, bg_color, context=context)
    mask = _filter("gaussian_filtering", object_gs.get_scaling, True, imp_list, v_pow, None, percent, False, False, None)[0]
    object_gs.prune_points(mask)
    return mask, imp_list
