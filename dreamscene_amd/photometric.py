"""The photometric loss of the reconstructive refine steps as one HIP op with exact autograd (csrc/photometric.hip).

  loss = photometric_loss(images, targets, l2=1.0, half_images=True)        training/object_trainer.py:626-653,
  loss = photometric_loss(images, targets, l1=0.8, dssim=0.2)               training/scene_trainer.py:1269-1293, :1737-1770
  l2_loss(a, b), l1_loss(a, b), ssim(img1, img2)                            utils/system_utils.py:59-126, the same signatures

Per view  l2 mean((x-y)^2) + l1 mean|x-y| + dssim (1 - mean(ssim_map(x, y)))  (SEMANTICS.md "Photometric loss"). images and
targets are one [C,H,W] tensor (-> a 0-dim loss), one [V,C,H,W] tensor or a list of V [C,H,W] tensors (-> [V] per-view losses; a
list of GaussianRasterizerViews outputs goes in without a stack). images are float32; targets float32 or float16 (widened
exactly); half_images rounds the image to fp16 on load, the refine steps' `.to(torch.float16)`, with a straight-through gradient.
No gradient goes to the targets. Device tensors run the kernels: fp32 arithmetic, sums in double in a fixed order, no host read
(the call is capturable). CPU tensors run the torch expression.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence, Union

import torch
import torch.nn.functional as F

from . import _lib as L

WINDOW_SIZE = 11
SIGMA = 1.5
C1 = 0.01 ** 2
C2 = 0.03 ** 2

Views = Union[torch.Tensor, Sequence[torch.Tensor]]


def ssim_window() -> torch.Tensor:
    """The 11 taps [11] fp32: exp(-(i-5)^2 / 4.5) as Python doubles, rounded to fp32, divided in fp32 by their fp32 sum (the
    correctly rounded sum of the fp32 taps, which is what the reference's torch sum gives)."""
    g = torch.tensor([math.exp(-((i - WINDOW_SIZE // 2) ** 2) / float(2 * SIGMA ** 2)) for i in range(WINDOW_SIZE)],
                     dtype=torch.float32)
    return g / g.double().sum().float()


def _ssim_map(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """utils/system_utils.py:97-121 restated for one [C,H,W] (or [B,C,H,W]) pair."""
    ch = x.size(-3)
    w1 = ssim_window().to(x.device).unsqueeze(1)
    window = w1.mm(w1.t()).unsqueeze(0).unsqueeze(0).expand(ch, 1, WINDOW_SIZE, WINDOW_SIZE).contiguous().type_as(x)
    pad = WINDOW_SIZE // 2
    mu1 = F.conv2d(x, window, padding=pad, groups=ch)
    mu2 = F.conv2d(y, window, padding=pad, groups=ch)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(x * x, window, padding=pad, groups=ch) - mu1_sq
    sigma2_sq = F.conv2d(y * y, window, padding=pad, groups=ch) - mu2_sq
    sigma12 = F.conv2d(x * y, window, padding=pad, groups=ch) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


class _RoundToHalf(torch.autograd.Function):
    """x rounded to fp16 and widened again; the gradient passes straight through (torch's own cast would round it to fp16)."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.float16).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        return g


def _reference_view(x: torch.Tensor, y: torch.Tensor, l2: float, l1: float, dssim: float, half_images: bool):
    """One view's (loss, terms [3]) as the torch expression: the terms with a non-zero weight, added in the order L2, L1,
    D-SSIM. The D-SSIM term is NaN where it is not evaluated (dssim == 0)."""
    if half_images:
        x = _RoundToHalf.apply(x)
    y = y.to(torch.float32)
    t_l2 = ((x - y) ** 2).mean()
    t_l1 = torch.abs(x - y).mean()
    t_ds = 1 - _ssim_map(x, y).mean() if dssim != 0 else torch.full((), float("nan"), dtype=torch.float32, device=x.device)
    loss = None
    for w, t in ((l2, t_l2), (l1, t_l1), (dssim, t_ds)):
        if w != 0:
            loss = w * t if loss is None else loss + w * t
    return loss, torch.stack([t_l2, t_l1, t_ds]).detach()


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _table(images, targets, half_images: bool, grads=None) -> L.GsrPhotoViews:
    t = L.GsrPhotoViews()
    t.n_views = len(images)
    t.channels, t.height, t.width = (int(s) for s in images[0].shape)
    t.target_is_half = 1 if targets[0].dtype == torch.float16 else 0
    t.round_image_to_half = 1 if half_images else 0
    for k, (im, tg) in enumerate(zip(images, targets)):
        t.image[k] = im.data_ptr()
        t.target[k] = tg.data_ptr()
        if grads is not None:
            t.dL_dimage[k] = grads[k].data_ptr()
    return t


class _Photo(torch.autograd.Function):
    """cfg = (l2, l1, dssim, half_images, need_grad); targets: a tuple of tensors (no gradient); images: V tensors."""

    @staticmethod
    def forward(ctx, cfg, targets, *images):
        lib = L.load()
        l2, l1, dssim, half_images, need_grad = cfg
        V, dev = len(images), images[0].device
        Cn, H, W = (int(s) for s in images[0].shape)
        loss = torch.empty((V,), dtype=torch.float32, device=dev)
        terms = torch.empty((V, 3), dtype=torch.float32, device=dev)
        saved = torch.empty((3, V, Cn, H, W), dtype=torch.float32, device=dev) if (need_grad and dssim != 0) else None
        nbytes = lib.gsr_photo_scratch_bytes(V, Cn, H, W)
        scratch = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
        tab = _table(images, targets, half_images)
        wts = L.GsrPhotoWeights(l2, l1, dssim)
        L.check(lib.gsr_photo_forward(C.byref(tab), C.byref(wts), loss.data_ptr(), terms.data_ptr(),
                                      None if saved is None else saved.data_ptr(), scratch.data_ptr(), nbytes, _stream(dev)),
                "gsr_photo_forward")
        ctx.save_for_backward(*images)
        ctx.targets, ctx.planes, ctx.cfg = targets, saved, cfg
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, g, _g_terms):
        images = ctx.saved_tensors
        l2, l1, dssim, half_images, _ = ctx.cfg
        if dssim != 0 and ctx.planes is None:
            raise L.GsrError("photometric_loss: backward through a forward that ran without gradients")
        lib = L.load()
        g = g.to(torch.float32).contiguous()
        grads = [torch.empty_like(im) for im in images]
        tab = _table(images, ctx.targets, half_images, grads)
        wts = L.GsrPhotoWeights(l2, l1, dssim)
        L.check(lib.gsr_photo_backward(C.byref(tab), C.byref(wts), None if ctx.planes is None else ctx.planes.data_ptr(),
                                       g.data_ptr(), _stream(images[0].device)), "gsr_photo_backward")
        return (None, None, *grads)


def _views(name: str, a: Views):
    """-> (list of [C,H,W] tensors, single)"""
    if isinstance(a, torch.Tensor):
        if a.dim() == 3:
            return [a], True
        if a.dim() == 4:
            return list(a.unbind(0)), False
        raise ValueError(f"photometric_loss: {name} must be [C,H,W], [V,C,H,W] or a list of [C,H,W] tensors")
    views = list(a)
    for p in views:
        if not isinstance(p, torch.Tensor) or p.dim() != 3:
            raise ValueError(f"photometric_loss: every entry of {name} must be a [C,H,W] tensor")
    return views, False


def photometric_loss(images: Views, targets: Views, *, l2: float = 0.0, l1: float = 0.0, dssim: float = 0.0,
                     half_images: bool = False, return_terms: bool = False):
    """-> the loss: 0-dim for one [C,H,W] pair, else [V] per-view losses (the caller sums the views and applies its `* 100`).
    return_terms: also the unweighted (L2, L1, D-SSIM) terms, [3] or [V,3], detached, for logging (D-SSIM is NaN when
    dssim == 0: the point-wise form does not evaluate it)."""
    ims, single = _views("images", images)
    tgs, tsingle = _views("targets", targets)
    if not ims:
        raise ValueError("photometric_loss: no views")
    if len(ims) != len(tgs) or single != tsingle:
        raise ValueError(f"photometric_loss: {len(ims)} images for {len(tgs)} targets")
    l2, l1, dssim = float(l2), float(l1), float(dssim)
    if l2 == 0.0 and l1 == 0.0 and dssim == 0.0:
        raise ValueError("photometric_loss: all weights are zero")
    shape, dev, tdtype = tuple(ims[0].shape), ims[0].device, tgs[0].dtype
    for im, tg in zip(ims, tgs):
        if im.dtype != torch.float32:
            raise TypeError(f"photometric_loss: images must be float32, got {im.dtype}")
        if tg.dtype not in (torch.float32, torch.float16) or tg.dtype != tdtype:
            raise TypeError(f"photometric_loss: targets must be all float32 or all float16, got {tg.dtype}")
        if tuple(im.shape) != shape or tuple(tg.shape) != shape:
            raise ValueError("photometric_loss: all images and targets of a call must have the same [C,H,W] size")
        if im.device != dev or tg.device != dev:
            raise ValueError("photometric_loss: all images and targets must be on one device")
    if min(shape) < 1 or shape[0] > L.GSR_MAX_PHOTO_CHANNELS:
        raise ValueError(f"photometric_loss: needs C in 1..{L.GSR_MAX_PHOTO_CHANNELS} and H, W >= 1, got {shape}")
    if dev.type == "cpu":
        outs = [_reference_view(im, tg, l2, l1, dssim, half_images) for im, tg in zip(ims, tgs)]
        loss = outs[0][0] if single else torch.stack([o[0] for o in outs])
        terms = outs[0][1] if single else torch.stack([o[1] for o in outs])
    elif dev.type == "cuda":
        need_grad = torch.is_grad_enabled() and any(im.requires_grad for im in ims)
        cfg = (l2, l1, dssim, bool(half_images), need_grad)
        ims = [im.contiguous() for im in ims]
        tgs = [tg.detach().contiguous() for tg in tgs]
        M = L.GSR_MAX_PHOTO_VIEWS
        chunks = [_Photo.apply(cfg, tuple(tgs[i:i + M]), *ims[i:i + M]) for i in range(0, len(ims), M)]
        loss = chunks[0][0] if len(chunks) == 1 else torch.cat([c[0] for c in chunks])
        terms = chunks[0][1] if len(chunks) == 1 else torch.cat([c[1] for c in chunks])
        if single:
            loss, terms = loss[0], terms[0]
    else:
        raise L.GsrError(f"photometric_loss: unsupported device {dev}")
    return (loss, terms) if return_terms else loss


# ---- the reference's signatures (utils/system_utils.py:59-64, :86-94): a checkout swaps one import -------------------------
def _as_images(a: torch.Tensor) -> torch.Tensor:
    if not isinstance(a, torch.Tensor) or a.dim() not in (3, 4):
        raise ValueError("expected a [C,H,W] or [B,C,H,W] tensor")
    return a.to(torch.float32) if a.dtype == torch.float16 else a      # exact widening


def l2_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """((network_output - gt) ** 2).mean() in fp32 arithmetic, 0-dim."""
    return photometric_loss(_as_images(network_output), gt, l2=1.0).mean()


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """torch.abs(network_output - gt).mean(), 0-dim."""
    return photometric_loss(_as_images(network_output), gt, l1=1.0).mean()


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """The mean of ssim_map: 0-dim, or with size_average=False the per-image means [B] of a [B,C,H,W] batch."""
    if window_size != WINDOW_SIZE:
        raise ValueError(f"ssim: only window_size={WINDOW_SIZE} is supported, got {window_size}")
    img1 = _as_images(img1)
    if not size_average and img1.dim() != 4:
        raise ValueError("ssim: size_average=False needs a [B,C,H,W] batch")
    per_image = 1 - photometric_loss(img1, img2, dssim=1.0)
    return per_image.mean() if size_average else per_image
