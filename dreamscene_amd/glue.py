"""The per-pixel glue between the rasterizer and the loss as HIP ops with exact autograd (csrc/glue.hip).

  disp, alpha = disp_from_depth_alpha(depth_alpha, fovx)     scene_gaussian.py:651-658, :874-881, :1023-1032
  loss = tv_loss(images) + tv_loss(depths)                   utils/system_utils.py:39-47 (object_trainer.py:380,
                                                             scene_trainer.py:869-870)

disp_from_depth_alpha takes one [2,H,W] depth_alpha (-> disp, alpha of [1,H,W] each: what the reference's torch.chunk gives)
or a list of V of them of one size (-> [V,1,H,W] each; a list of GaussianRasterizerViews outputs goes in without a stack), and
fovx as a float or one per view. Device tensors run the kernels: the forward bits are those of torch's op chain, the masked
minimum is chosen on the device (no host read: the call is capturable), the backward is torch's gradient with the ties of
min / max shared evenly (SEMANTICS.md "disp post-processing and tv_loss"). CPU tensors run the reference's torch expression.
Opt-in: render_api.object_render(fused_disp=True) and scene.scene_render(fused_disp=True).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence, Union

import torch

from . import _lib as L


def _focal(fovx: float) -> float:
    return 1 / (2 * math.tan(fovx / 2))      # the reference's Python expression (double; rounded to fp32 where torch does)


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _scratch(nbytes: int, dev: torch.device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _table(planes, focals, H: int, W: int, grads=None) -> L.GsrDispViews:
    t = L.GsrDispViews()
    t.n_views, t.height, t.width = len(planes), H, W
    for k, p in enumerate(planes):
        t.depth_alpha[k] = p.data_ptr()
        t.focal[k] = focals[k]
        if grads is not None:
            t.dL_ddepth_alpha[k] = grads[k].data_ptr()
    return t


class _DispViews(torch.autograd.Function):
    @staticmethod
    def forward(ctx, focals, *planes):
        lib = L.load()
        V, (H, W), dev = len(planes), planes[0].shape[1:], planes[0].device
        disp = torch.empty((V, 1, H, W), dtype=torch.float32, device=dev)
        alpha = torch.empty((V, 1, H, W), dtype=torch.float32, device=dev)
        stats = torch.empty((V, L.GSR_DISP_STATS_FLOATS), dtype=torch.float32, device=dev)
        nbytes = lib.gsr_disp_scratch_bytes(V, H, W)
        scratch = _scratch(nbytes, dev)
        tab = _table(planes, focals, H, W)
        L.check(lib.gsr_disp_forward(C.byref(tab), disp.data_ptr(), alpha.data_ptr(), stats.data_ptr(), scratch.data_ptr(),
                                     nbytes, _stream(dev)), "gsr_disp_forward")
        ctx.save_for_backward(*planes)
        ctx.stats, ctx.focals = stats, focals
        ctx.set_materialize_grads(False)
        return disp, alpha

    @staticmethod
    def backward(ctx, g_disp, g_alpha):
        planes = ctx.saved_tensors
        V = len(planes)
        if g_disp is None and g_alpha is None:
            return (None,) * (1 + V)
        lib = L.load()
        (H, W), dev = planes[0].shape[1:], planes[0].device
        if g_disp is None:
            g_disp = torch.zeros((V, 1, H, W), dtype=torch.float32, device=dev)
        g_disp = g_disp.to(torch.float32).contiguous()
        g_alpha = None if g_alpha is None else g_alpha.to(torch.float32).contiguous()
        grads = [torch.empty((2, H, W), dtype=torch.float32, device=dev) for _ in range(V)]
        nbytes = lib.gsr_disp_scratch_bytes(V, H, W)
        scratch = _scratch(nbytes, dev)
        tab = _table(planes, ctx.focals, H, W, grads)
        L.check(lib.gsr_disp_backward(C.byref(tab), ctx.stats.data_ptr(), g_disp.data_ptr(),
                                      None if g_alpha is None else g_alpha.data_ptr(), scratch.data_ptr(), nbytes,
                                      _stream(dev)), "gsr_disp_backward")
        return (None, *grads)


def _disp_reference(depth_alpha: torch.Tensor, fovx: float):
    """scene_gaussian.py:1023-1032 as the reference writes it (the boolean-mask minimum with its try / except)."""
    depth, alpha = torch.chunk(depth_alpha, 2)
    focal = _focal(fovx)
    disp = focal / (depth + (alpha * 10) + 1e-5)
    try:
        min_d = disp[alpha <= 0.1].min()
    except Exception:
        min_d = disp.min()
    disp = torch.clamp((disp - min_d) / (disp.max() - min_d), 0.0, 1.0)
    return disp, alpha


def disp_from_depth_alpha(depth_alpha: Union[torch.Tensor, Sequence[torch.Tensor]],
                          fovx: Union[float, Sequence[float]]):
    """-> (disp, alpha): [1,H,W] each for one [2,H,W] depth_alpha, [V,1,H,W] each for a list of V of them."""
    single = isinstance(depth_alpha, torch.Tensor)
    planes = [depth_alpha] if single else list(depth_alpha)
    if not planes:
        raise ValueError("disp_from_depth_alpha: no views")
    if isinstance(fovx, (list, tuple)):
        if single or len(fovx) != len(planes):
            raise ValueError(f"disp_from_depth_alpha: {len(fovx)} fovx values for {len(planes)} views")
        fovs = [float(f) for f in fovx]
    else:
        fovs = [float(fovx)] * len(planes)
    H = W = None
    for p in planes:
        if not isinstance(p, torch.Tensor) or p.dim() != 3 or p.shape[0] != 2:
            raise ValueError("disp_from_depth_alpha: every depth_alpha must be a [2,H,W] tensor")
        if p.dtype != torch.float32:
            raise TypeError(f"disp_from_depth_alpha: depth_alpha must be float32, got {p.dtype}")
        if H is None:
            H, W = int(p.shape[1]), int(p.shape[2])
        elif (int(p.shape[1]), int(p.shape[2])) != (H, W):
            raise ValueError("disp_from_depth_alpha: all views of a call must have the same image size")
        if p.device != planes[0].device:
            raise ValueError("disp_from_depth_alpha: all views must be on one device")
    if planes[0].device.type == "cpu":
        outs = [_disp_reference(p, f) for p, f in zip(planes, fovs)]
        if single:
            return outs[0]
        return torch.stack([d for d, _ in outs]), torch.stack([a for _, a in outs])
    if planes[0].device.type != "cuda":
        raise L.GsrError(f"disp_from_depth_alpha: unsupported device {planes[0].device}")
    focals = [_focal(f) for f in fovs]
    planes = [p.contiguous() for p in planes]
    M = L.GSR_MAX_DISP_VIEWS
    chunks = [_DispViews.apply(tuple(focals[i:i + M]), *planes[i:i + M]) for i in range(0, len(planes), M)]
    disp = chunks[0][0] if len(chunks) == 1 else torch.cat([c[0] for c in chunks])
    alpha = chunks[0][1] if len(chunks) == 1 else torch.cat([c[1] for c in chunks])
    if single:
        return disp[0], alpha[0]
    return disp, alpha


class _TV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = L.load()
        B, Cn, H, W = (int(s) for s in x.shape)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        nbytes = lib.gsr_tv_scratch_bytes(B, Cn, H, W)
        scratch = _scratch(nbytes, x.device)
        L.check(lib.gsr_tv_forward(x.data_ptr(), B, Cn, H, W, out.data_ptr(), scratch.data_ptr(), nbytes, _stream(x.device)),
                "gsr_tv_forward")
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        lib = L.load()
        B, Cn, H, W = (int(s) for s in x.shape)
        g = g.to(torch.float32).contiguous()
        gx = torch.empty_like(x)
        L.check(lib.gsr_tv_backward(x.data_ptr(), B, Cn, H, W, g.data_ptr(), gx.data_ptr(), _stream(x.device)),
                "gsr_tv_backward")
        return gx


def _tv_reference(x: torch.Tensor) -> torch.Tensor:
    """utils/system_utils.py:39-47 restated."""
    b, h, w = x.size(0), x.size(2), x.size(3)
    count_h = x[:, :, 1:, :].numel() // b
    count_w = x[:, :, :, 1:].numel() // b
    h_tv = torch.pow(x[:, :, 1:, :] - x[:, :, : h - 1, :], 2).sum()
    w_tv = torch.pow(x[:, :, :, 1:] - x[:, :, :, : w - 1], 2).sum()
    return 2 * (h_tv / count_h + w_tv / count_w) / b


def tv_loss(x: torch.Tensor) -> torch.Tensor:
    """The reference's tv_loss of x [B,C,H,W] (H, W >= 2) as a 0-dim tensor, differentiable."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("tv_loss: x must be a [B,C,H,W] tensor")
    if x.dtype != torch.float32:
        raise TypeError(f"tv_loss: x must be float32, got {x.dtype}")
    if x.shape[2] < 2 or x.shape[3] < 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"tv_loss: needs B, C >= 1 and H, W >= 2, got {tuple(x.shape)}")
    if x.device.type == "cpu":
        return _tv_reference(x)
    if x.device.type != "cuda":
        raise L.GsrError(f"tv_loss: unsupported device {x.device}")
    return _TV.apply(x.contiguous())
