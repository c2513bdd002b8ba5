"""The photometric loss between rendered images and their targets, torch's kernel chain against the HIP op of
dreamscene_amd/photometric.py. Every leg is a forward plus backward to the images:
  l2_torch / l2_fused       the refine steps' setting: L2 only, fp16 targets, the image rounded to fp16 (in fp32 arithmetic);
  dssim_torch / dssim_fused 0.8 L1 + 0.2 D-SSIM (the 3DGS default): torch's five depth-wise 11x11 conv2d against the tiled kernel;
  step_*                    a refine-shaped step with both losses: GaussianRasterizerViews over --views views of a synthetic
                            object of --gaussians Gaussians (tests/util.small_scene's make), the loss, backward().
Shapes: --views x 3 x res^2 for res in --res (default 1024 and 512).
Method: the legs of a pair alternate in one process (A B A B ...), each window >= --seconds of whole iterations after a warm-up,
one device synchronisation at both ends of a window; the median window per leg is reported. The fused forward and backward are
also timed apart (events around --iters back-to-back calls) and set against the algorithmic bytes per element -- forward 8 read
(6 with fp16 targets) + 12 written with the SSIM planes, point-wise 8 (6) read; backward 20 read + 4 written, point-wise 8 (6) + 4
-- as a share of the 8 TB/s peak. Launches per iteration are counted with torch.profiler (null where it is not available).
usage: python tools/bench_photometric.py [--seconds 1.0] [--rounds 3] [--res 1024 512] [--views 4] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8.0e12
SETTINGS = {"l2": dict(l2=1.0, half_images=True), "dssim": dict(l1=0.8, dssim=0.2)}


def torch_view_loss(x, y, l2=0.0, l1=0.0, dssim=0.0, half_images=False):
    """The torch chain a user of the rasterizer writes today (the package's own CPU expression, on the device)."""
    from dreamscene_amd import photometric as P
    return P._reference_view(x, y, l2, l1, dssim, half_images)[0]


def loss_legs(images, targets, name):
    from dreamscene_amd import photometric as P
    kw = SETTINGS[name]

    def torch_leg():
        loss = torch.stack([torch_view_loss(x, y, **kw) for x, y in zip(images, targets)]).sum()
        return torch.autograd.grad(loss, images)

    def fused_leg():
        return torch.autograd.grad(P.photometric_loss(images, targets, **kw).sum(), images)
    return {f"{name}_torch": torch_leg, f"{name}_fused": fused_leg}


def step_legs(P_, H, W, V, dev, targets32, targets16):
    from dreamscene_amd import photometric as P, synth
    from dreamscene_amd.rasterizer import GaussianRasterizationSettings
    from dreamscene_amd.views import GaussianRasterizerViews
    g = synth.g_object(P_, seed=3, K=16)
    g["scales"] = (g["scales"] * 6.0).astype(np.float32)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)      # noqa: E731
    cams = [synth.orbit_camera(5.35, 75.0, 45.0 * i + 10.0, 0.4 + 0.07 * i, H, W) for i in range(V)]
    sets = [GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t([1, 1, 1]),
                                          scale_modifier=1.0, viewmatrix=t(c.world_view_transform),
                                          projmatrix=t(c.full_proj_transform), sh_degree=3, campos=t(c.camera_center),
                                          prefiltered=False, score_flag=False) for c in cams]
    lv = {k: t(v).requires_grad_(True) for k, v in g.items()}

    def make(name, fused):
        kw = SETTINGS[name]
        tg = targets16 if name == "l2" else targets32

        def step():
            for p in lv.values():
                p.grad = None
            outs = GaussianRasterizerViews(sets)(means3D=lv["means3D"], means2D=None, shs=lv["shs"], opacities=lv["opacities"],
                                                 scales=lv["scales"], rotations=lv["rotations"])
            ims = [o[0] for o in outs]
            if fused:
                loss = P.photometric_loss(ims, tg, **kw).sum() * 100
            else:
                loss = torch.stack([torch_view_loss(x, y, **kw) for x, y in zip(ims, tg)]).sum() * 100
            loss.backward()
        return step
    return {f"step_{n}_{'fused' if f else 'torch'}": make(n, f) for n in SETTINGS for f in (False, True)}


def window(fn, seconds, dev):
    torch.cuda.synchronize(dev)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        n += 1
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n * 1e3


def pair(legs, A, B, a, dev, res):
    ms = {A: [], B: []}
    for name in (A, B):
        for _ in range(a.warmup):
            legs[name]()
    for _ in range(a.rounds):
        for name in (A, B):
            ms[name].append(window(legs[name], a.seconds, dev))
    for name in (A, B):
        res[name] = {"ms": round(statistics.median(ms[name]), 4), "windows_ms": [round(x, 4) for x in ms[name]]}
    res[f"{A}_over_{B}"] = round(res[A]["ms"] / res[B]["ms"], 3)


def launches(fn):
    """Device kernels of one call of fn, or None where the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def fused_halves(images, targets, name, iters, dev):
    """ms of the fused forward and of the fused backward alone, and their share of the peak on the algorithmic bytes."""
    from dreamscene_amd import photometric as P
    kw = SETTINGS[name]
    n = sum(x.numel() for x in images)
    tb = 2 if targets[0].dtype == torch.float16 else 4
    ssim = kw.get("dssim", 0.0) != 0.0
    fwd_bytes = n * (4 + tb + (12 if ssim else 0))
    bwd_bytes = n * (4 + tb + (12 if ssim else 0) + 4)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    losses = []
    for _ in range(3):
        torch.autograd.grad(P.photometric_loss(images, targets, **kw).sum(), images)
    torch.cuda.synchronize(dev)
    e[0].record()
    for _ in range(iters):
        losses.append(P.photometric_loss(images, targets, **kw))
    e[1].record()
    g = torch.ones_like(losses[0])
    e[2].record()
    for loss in losses:
        torch.autograd.grad(loss, images, grad_outputs=g)
    e[3].record()
    torch.cuda.synchronize(dev)
    f_ms, b_ms = e[0].elapsed_time(e[1]) / iters, e[2].elapsed_time(e[3]) / iters
    return {"forward_ms": round(f_ms, 4), "backward_ms": round(b_ms, 4),
            "forward_share_of_peak": round(fwd_bytes / (f_ms * 1e-3) / PEAK_BYTES_PER_S, 3),
            "backward_share_of_peak": round(bwd_bytes / (b_ms * 1e-3) / PEAK_BYTES_PER_S, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[1024, 512])
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--gaussians", type=int, default=600)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    V = a.views
    out = {"workload": f"{V} views x 3 channels, forward + backward to the images", "shapes": {}}
    for r in a.res:
        gen = torch.Generator().manual_seed(r)
        images = [torch.rand((3, r, r), generator=gen).to(dev).requires_grad_(True) for _ in range(V)]
        t32 = [torch.rand((3, r, r), generator=gen).to(dev) for _ in range(V)]
        t16 = [y.to(torch.float16) for y in t32]
        res = {}
        for name in SETTINGS:
            tg = t16 if name == "l2" else t32
            legs = loss_legs(images, tg, name)
            A, B = f"{name}_torch", f"{name}_fused"
            ga, gb = legs[A](), legs[B]()                      # the legs compute the same thing: checked before they are timed
            scale = max(float(q.abs().max()) for q in ga)
            res[f"{name}_max_grad_difference"] = float(f"{max(float((u - v).abs().max()) for u, v in zip(ga, gb)) / scale:.3e}")
            pair(legs, A, B, a, dev, res)
            res[A]["launches"], res[B]["launches"] = launches(legs[A]), launches(legs[B])
            res[B].update(fused_halves(images, tg, name, a.iters, dev))
        if not a.no_step:
            legs = step_legs(a.gaussians, r, r, V, dev, t32, t16)
            for name in SETTINGS:
                pair(legs, f"step_{name}_torch", f"step_{name}_fused", a, dev, res)
        out["shapes"][f"{V}x3x{r}x{r}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
