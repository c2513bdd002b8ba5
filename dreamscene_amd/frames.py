"""Frame export: the uint8 tail of the reference's inference paths as HIP (csrc/frames.hip; SEMANTICS.md "Frame export").

video_inference (training/object_trainer.py:81-118), scene_video_inference and scene_cams_record (training/scene_trainer.py:
261-340) end every frame with a blocking fp32 device-to-host copy, a host read of depth.max() and a numpy pass:

    image  = clamp(rgb, 0, 1).cpu().permute(1, 2, 0).numpy();                 (image  * 255).round().astype(np.uint8)
    depths = clamp(depth / depth.max(), 0, 1).cpu().permute(1, 2, 0).numpy(); (depths * 255).round().astype(np.uint8)

  rgb, depth = quantize_frames(images, depth_alphas)      the same bytes from the per-view device tensors, on the device:
                                                          uint8 [F,H,W,3] and [F,H,W,1]; no host read, capturable
  frames = render_frames(settings_list, means3D, ...)     renders the cameras `chunk` at a time through the batched forward,
                                                          quantises every chunk and copies its bytes (4 per pixel, not 16) into
                                                          page-locked host memory on a copy stream while the next chunk renders;
                                                          the host waits once, at the end. frames.rgb.numpy() is the video.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Union

import torch

from . import _lib as L
from . import rasterizer as R
from . import views as V

MAX_VIEWS = L.GSR_MAX_FRAME_VIEWS


class Frames(NamedTuple):
    rgb: torch.Tensor                      # uint8 [F,H,W,3]
    depth: Optional[torch.Tensor]          # uint8 [F,H,W,1], or None (depth=False)


_SCRATCH = {}        # (device index, stream handle) -> the maxima of one call (16 KB): work on one stream is ordered
_COPY_STREAM = {}    # device index -> render_frames' one copy stream


def _scratch(lib, dev: torch.device, stream: int) -> torch.Tensor:
    key = (dev.index, stream)
    buf = _SCRATCH.get(key)
    if buf is None:
        nbytes = int(lib.gsr_frames_scratch_bytes(MAX_VIEWS, 1 << 15, 1 << 15))      # the largest any shape needs
        buf = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return buf


def _planes(x, channels: int, what: str):
    """A stacked [F,C,H,W] tensor or a sequence of [C,H,W] tensors -> the list of per-view tensors."""
    if isinstance(x, torch.Tensor):
        if x.dim() != 4:
            raise ValueError(f"quantize_frames: a stacked {what} must be [F,{channels},H,W], got {tuple(x.shape)}")
        x = list(x.unbind(0))
    else:
        x = list(x)
    for p in x:
        if not isinstance(p, torch.Tensor) or p.dim() != 3 or p.shape[0] != channels:
            raise ValueError(f"quantize_frames: every {what} must be a [{channels},H,W] tensor")
        if p.dtype != torch.float32:
            raise ValueError(f"quantize_frames: {what} must be float32, got {p.dtype}")
    return x


def _check_device_out(t, shape, dev, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous uint8 tensor of shape {shape}")
    if t.device != dev:
        raise ValueError(f"{what} must be on {dev}")


def quantize_frames(images: Union[torch.Tensor, Sequence[torch.Tensor]],
                    depth_alphas: Union[None, torch.Tensor, Sequence[torch.Tensor]] = None,
                    out_rgb: Optional[torch.Tensor] = None, out_depth: Optional[torch.Tensor] = None):
    """images: F tensors [3,H,W] (or one [F,3,H,W]); depth_alphas: None, or F tensors [2,H,W] (or one [F,2,H,W]) as the
    rasterizer returns them. -> (rgb uint8 [F,H,W,3], depth uint8 [F,H,W,1] or None) on the inputs' device, written on the
    current stream: byte = rint(clamp(x, 0, 1) * 255), x = colour or depth / (the frame's maximum depth) (csrc/frames.hip; an
    all-zero depth frame gives zeros). Inputs are finite. No host read; with out_rgb / out_depth given, and after the first call
    on a stream, no allocation either (capturable). One launch per 16 frames, two with depth."""
    imgs = _planes(images, 3, "image")
    if not imgs:
        raise ValueError("quantize_frames: no frames")
    das = None if depth_alphas is None else _planes(depth_alphas, 2, "depth_alpha")
    F, (H, W), dev = len(imgs), (int(imgs[0].shape[1]), int(imgs[0].shape[2])), imgs[0].device
    if das is not None and len(das) != F:
        raise ValueError(f"quantize_frames: {len(das)} depth_alphas for {F} images")
    if out_depth is not None and das is None:
        raise ValueError("quantize_frames: out_depth without depth_alphas")
    if H < 1 or W < 1:
        raise ValueError("quantize_frames: empty frames")
    for p in imgs + (das or []):
        if (int(p.shape[1]), int(p.shape[2])) != (H, W):
            raise ValueError("quantize_frames: all frames of a call must have the same image size")
    for p in imgs + (das or []):
        if p.device.type != "cuda":
            raise L.GsrError(f"quantize_frames: tensors must be on a ROCm device, got {p.device} (there is no CPU path)")
        if p.device != dev:
            raise ValueError("quantize_frames: all frames must be on one device")
    if out_rgb is not None:
        _check_device_out(out_rgb, (F, H, W, 3), dev, "out_rgb")
    if out_depth is not None:
        _check_device_out(out_depth, (F, H, W, 1), dev, "out_depth")
    lib = L.load()
    rgb = out_rgb if out_rgb is not None else torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    depth = None
    if das is not None:
        depth = out_depth if out_depth is not None else torch.empty((F, H, W, 1), dtype=torch.uint8, device=dev)
    imgs = [p.contiguous() for p in imgs]
    das = None if das is None else [p.contiguous() for p in das]
    stream = torch.cuda.current_stream(dev).cuda_stream
    scratch = _scratch(lib, dev, stream) if das is not None else None
    for i in range(0, F, MAX_VIEWS):
        n = min(MAX_VIEWS, F - i)
        tab = L.GsrFrameViews()
        tab.n_views, tab.height, tab.width = n, H, W
        for k in range(n):
            tab.image[k] = imgs[i + k].data_ptr()
            if das is not None:
                tab.depth_alpha[k] = das[i + k].data_ptr()
        L.check(lib.gsr_frames_quantize(C.byref(tab), rgb[i:i + n].data_ptr(), None if depth is None else depth[i:i + n].data_ptr(),
                                        None if scratch is None else scratch.data_ptr(), 0 if scratch is None else scratch.numel(),
                                        stream), "gsr_frames_quantize")
    return rgb, depth


def _check_out(out, F, H, W, depth, to_host, dev):
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError("render_frames: out must be a Frames (rgb, depth) pair")
    rgb, dep = out
    for t, shape, what in ((rgb, (F, H, W, 3), "out.rgb"), (dep, (F, H, W, 1), "out.depth")):
        if t is None and what == "out.depth" and not depth:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"render_frames: {what} must be a contiguous uint8 tensor of shape {shape}")
        if to_host and (t.device.type != "cpu" or not t.is_pinned()):
            raise ValueError(f"render_frames: {what} must be page-locked host memory (torch.empty(..., pin_memory=True))")
        if not to_host and t.device != dev:
            raise ValueError(f"render_frames: with to_host=False {what} must be on {dev}")
    return rgb, (dep if depth else None)


def render_frames(settings_list: Sequence, means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                  cov3D_precomp=None, *, depth: bool = True, chunk: int = 8, out=None, context=None,
                  to_host: bool = True) -> Frames:
    """The frames of a video: every camera of settings_list (GaussianRasterizationSettings of one image size) rendered forward
    only, `chunk` (<= 16) at a time through views.rasterize_views_forward_raw, and quantised on the device (quantize_frames).
    to_host=True  -> Frames of page-locked host tensors (`out` = a Frames from an earlier call reuses them): every chunk's bytes
                     go into one of two device staging slots and from there to the host on one copy stream; events order
                     "quantised -> copied" and "copied -> slot written again"; the host waits once, when the last copy is done.
    to_host=False -> Frames of device tensors, no copy (`out`: device tensors).
    depth=False   -> Frames.depth is None and depth_alpha is not read.
    Nothing here reads a frame back to the host; the forward's own pair-count read stays as it is."""
    settings_list = list(settings_list)
    if not settings_list:
        raise ValueError("render_frames: no views")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"render_frames: chunk must be >= 1, got {chunk}")
    chunk = min(chunk, V.MAX_VIEWS, MAX_VIEWS)
    if any(s.score_flag for s in settings_list):
        raise ValueError("render_frames: score_flag views render no frames (use views.importance_scores)")
    H, W = int(settings_list[0].image_height), int(settings_list[0].image_width)
    if any((int(s.image_height), int(s.image_width)) != (H, W) for s in settings_list):
        raise ValueError("render_frames: all views must have the same image size")
    if (shs is None) == (colors_precomp is None):
        raise ValueError("render_frames: provide exactly one of shs and colors_precomp")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise ValueError("render_frames: provide exactly one of the scales / rotations pair and cov3D_precomp")
    dev, F = means3D.device, len(settings_list)
    if out is not None:
        out = _check_out(out, F, H, W, depth, to_host, dev)
    for t in (means3D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp):
        if t is not None and (not isinstance(t, torch.Tensor) or t.device.type != "cuda"):
            raise L.GsrError("render_frames: the Gaussians must be tensors on a ROCm device (there is no CPU path)")
    rc = (context or R.DEFAULT_CONTEXT).snapshot()
    rc._forward_only = True

    def render(i):
        res = V.rasterize_views_forward_raw(settings_list[i:i + chunk], means3D, opacities, shs, colors_precomp, scales,
                                            rotations, cov3D_precomp, rc=rc)
        return [o["color"] for o, _ in res], ([o["depth_alpha"] for o, _ in res] if depth else None)

    with torch.no_grad(), torch.cuda.device(dev):
        if not to_host:
            rgb, dep = out if out is not None else (
                torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev),
                torch.empty((F, H, W, 1), dtype=torch.uint8, device=dev) if depth else None)
            for i in range(0, F, chunk):
                imgs, das = render(i)
                quantize_frames(imgs, das, rgb[i:i + len(imgs)], None if dep is None else dep[i:i + len(imgs)])
            return Frames(rgb, dep)
        rgb, dep = out if out is not None else (
            torch.empty((F, H, W, 3), dtype=torch.uint8, pin_memory=True),
            torch.empty((F, H, W, 1), dtype=torch.uint8, pin_memory=True) if depth else None)
        cur = torch.cuda.current_stream(dev)
        copy = _COPY_STREAM.get(dev.index)
        if copy is None:
            copy = _COPY_STREAM[dev.index] = torch.cuda.Stream(dev)
        n_slots = min(2, (F + chunk - 1) // chunk)
        slots = [(torch.empty((chunk, H, W, 3), dtype=torch.uint8, device=dev),
                  torch.empty((chunk, H, W, 1), dtype=torch.uint8, device=dev) if depth else None) for _ in range(n_slots)]
        quantised = [torch.cuda.Event() for _ in range(n_slots)]
        copied = [torch.cuda.Event() for _ in range(n_slots)]
        for c, i in enumerate(range(0, F, chunk)):
            s = c % 2
            imgs, das = render(i)
            n = len(imgs)
            if c >= 2:
                cur.wait_event(copied[s])                  # the slot's previous bytes have left it
            s_rgb, s_dep = slots[s]
            quantize_frames(imgs, das, s_rgb[:n], None if s_dep is None else s_dep[:n])
            quantised[s].record(cur)
            copy.wait_event(quantised[s])
            with torch.cuda.stream(copy):
                rgb[i:i + n].copy_(s_rgb[:n], non_blocking=True)
                if depth:
                    dep[i:i + n].copy_(s_dep[:n], non_blocking=True)
                copied[s].record(copy)
        copy.synchronize()                                 # the one host wait; the slots are free to die after it
        return Frames(rgb, dep)
