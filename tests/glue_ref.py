"""References for the glue ops (dreamscene_amd/glue.py): the reference's torch expressions, written out here independently of the
package, and a float64 helper for the disp post-processing."""
from __future__ import annotations

import math

import numpy as np
import torch


def torch_disp(depth_alpha: torch.Tensor, fovx: float):
    """scene_gaussian.py:1023-1032 verbatim (the boolean-mask minimum and its try / except), on depth_alpha's device."""
    depth, alpha = torch.chunk(depth_alpha, 2)
    focal = 1 / (2 * math.tan(fovx / 2))
    disp = focal / (depth + (alpha * 10) + 1e-5)
    try:
        min_d = disp[alpha <= 0.1].min()
    except Exception:
        min_d = disp.min()
    disp = torch.clamp((disp - min_d) / (disp.max() - min_d), 0.0, 1.0)
    return disp, alpha


def torch_tv(x: torch.Tensor) -> torch.Tensor:
    """utils/system_utils.py:39-47 verbatim."""
    batch_size = x.size()[0]
    h_x = x.size()[2]
    w_x = x.size()[3]
    count_h = x[:, :, 1:, :].size()[1] * x[:, :, 1:, :].size()[2] * x[:, :, 1:, :].size()[3]
    count_w = x[:, :, :, 1:].size()[1] * x[:, :, :, 1:].size()[2] * x[:, :, :, 1:].size()[3]
    h_tv = torch.pow((x[:, :, 1:, :] - x[:, :, : h_x - 1, :]), 2).sum()
    w_tv = torch.pow((x[:, :, :, 1:] - x[:, :, :, : w_x - 1]), 2).sum()
    return 2 * (h_tv / count_h + w_tv / count_w) / batch_size


def disp_f64(depth_alpha, fovx: float, g_disp=None, g_alpha=None) -> dict:
    """d in fp32 in torch's order of operations (t = alpha * 10, u = (depth + t) + 1e-5, d = (1 / u) * focal), everything after
    it in float64 on those values: the same selections (mask, m, M, ties) as the glue. With g_disp (and g_alpha), also
    dL/d depth_alpha [2,H,W] in float64 (torch's rules: inclusive clamp mask, ties of min / max shared evenly)."""
    da = np.asarray(depth_alpha.detach().cpu().numpy() if isinstance(depth_alpha, torch.Tensor) else depth_alpha, np.float32)
    depth, alpha = da[0], da[1]
    focal32 = np.float32(1 / (2 * math.tan(fovx / 2)))
    u32 = (depth + alpha * np.float32(10)) + np.float32(1e-5)
    d32 = (np.float32(1) / u32) * focal32
    d = d32.astype(np.float64)
    mask = alpha <= np.float32(0.1)
    masked = bool(mask.any())
    sel = mask if masked else np.ones_like(mask)
    m, M = np.float64(d[sel].min()), np.float64(d.max())
    r = M - m
    with np.errstate(invalid="ignore", divide="ignore"):
        q = (d - m) / r
        out = dict(d32=d32, m=m, M=M, masked=masked, disp=np.clip(q, 0.0, 1.0),
                   tie_m=sel & (d == m), tie_M=(d == M))
        if g_disp is not None:
            g = np.asarray(g_disp, np.float64).reshape(d.shape)
            h = np.where((q >= 0) & (q <= 1), g, 0.0)
            dd = h / r
            dm = float(np.sum(h * (-1.0 / r + (d - m) / (r * r))))
            dM = float(-np.sum(h * (d - m) / (r * r)))
            dd = dd + np.where(out["tie_m"], dm / max(1, out["tie_m"].sum()), 0.0)
            dd = dd + np.where(out["tie_M"], dM / max(1, out["tie_M"].sum()), 0.0)
            du = -dd * float(focal32) / (u32.astype(np.float64) ** 2)
            ga = 0.0 if g_alpha is None else np.asarray(g_alpha, np.float64).reshape(d.shape)
            out["grad"] = np.stack([du, 10.0 * du + ga])
    return out


def tv_f64(x) -> float:
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float64)
    B, C, H, W = x.shape
    h = np.sum((x[:, :, 1:, :] - x[:, :, :-1, :]) ** 2)
    w = np.sum((x[:, :, :, 1:] - x[:, :, :, :-1]) ** 2)
    return 2.0 * (h / (C * (H - 1) * W) + w / (C * H * (W - 1))) / B


def tv_grad_f64(x, g: float = 1.0) -> np.ndarray:
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float64)
    B, C, H, W = x.shape
    ch, cw = 4.0 / (B * C * (H - 1) * W), 4.0 / (B * C * H * (W - 1))
    gx = np.zeros_like(x)
    dh = x[:, :, 1:, :] - x[:, :, :-1, :]
    dw = x[:, :, :, 1:] - x[:, :, :, :-1]
    gx[:, :, 1:, :] += ch * dh
    gx[:, :, :-1, :] -= ch * dh
    gx[:, :, :, 1:] += cw * dw
    gx[:, :, :, :-1] -= cw * dw
    return g * gx


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape, same NaN positions, the same bits everywhere else."""
    if tuple(a.shape) != tuple(b.shape):
        return False
    a, b = a.detach().contiguous(), b.detach().contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb])


def random_planes(V: int, H: int, W: int, seed: int, device="cpu"):
    """depth in [0.5, 5.5), alpha in [0, 1): about a tenth of the pixels inside the mask."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(V):
        da = torch.empty((2, H, W), dtype=torch.float32)
        da[0] = torch.rand((H, W), generator=g) * 5 + 0.5
        da[1] = torch.rand((H, W), generator=g)
        out.append(da.to(device))
    return out


def tie_planes(da: torch.Tensor) -> torch.Tensor:
    """In place on a [2,H,W] plane (H >= 11, W >= 6) from random_planes: the masked pixels get u <= 4.5, then u = 5.5 + 1e-5
    exactly (the masked minimum of d) on the 9 masked pixels [:3, :3] and on the unmasked pixel (5, 5), and u = 1e-5 (the
    maximum) on the 4 masked pixels (10, :4)."""
    mask = da[1] <= 0.1
    da[1][mask] = torch.clamp(da[1][mask], max=0.05)
    da[0][mask] = torch.clamp(da[0][mask], max=4.0)
    da[0, :3, :3], da[1, :3, :3] = 4.875, 0.0625
    da[0, 5, 5], da[1, 5, 5] = 4.25, 0.125
    da[0, 10, :4], da[1, 10, :4] = 0.0, 0.0
    return da
