"""The per-pixel glue between the rasterizer and the loss, torch's kernel chain against the HIP ops of dreamscene_amd/glue.py, at C3
(4 views at 1024^2 of the 500 k-Gaussian G-object, depth_alpha rendered by the rasterizer). Every leg is a forward plus backward:
  glue_torch   four `disp_on_device` (tools/train_step.py: the reference's arithmetic, masked minimum without the host read), the
               stacks, tv_loss(images) + tv_loss(depths) (utils/system_utils.py:39-47 restated), torch.autograd.grad to the inputs;
  glue_fused   glue.disp_from_depth_alpha over the four planes (one call), glue.tv_loss(stacked images) + glue.tv_loss(disp);
  step_torch / step_fused   the `views_fused` training step of tools/train_step.py (GaussianRasterizerViews, statistics in K8,
               FusedAdam, the same stand-in guidance loss and scale loss) with either glue.
Method: the legs alternate in one process (A B A B ...), each window >= --seconds of whole iterations after a warm-up, one device
synchronisation at both ends of a window; the median window per leg is reported.
--profile-leg glue_torch|glue_fused: run only that leg --iters times on planes made on the host (no kernel outside the leg), for
one `rocprofv3 --kernel-trace --stats` pass per leg: kernels per iteration = kernels in the trace / --iters.
usage: python tools/bench_glue.py [--seconds 1.0] [--rounds 3] [--gaussians 500000] [--res 1024] [--no-step]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def glue_legs(planes, images, fovs):
    """-> {name: fn()} over leaf tensors planes [V x [2,H,W]] and images [V x [3,H,W]]; fn returns the input gradients."""
    from dreamscene_amd import glue
    from tools import train_step as TS
    leaves = list(planes) + list(images)

    def torch_glue():
        depths = [TS.disp_on_device(da, f)[0] for da, f in zip(planes, fovs)]
        loss = TS.tv_loss(torch.stack(images, dim=0)) + TS.tv_loss(torch.stack(depths, dim=0))
        return torch.autograd.grad(loss, leaves)

    def fused_glue():
        disp, _ = glue.disp_from_depth_alpha(planes, fovs)
        loss = glue.tv_loss(torch.stack(images, dim=0)) + glue.tv_loss(disp)
        return torch.autograd.grad(loss, leaves)
    return {"glue_torch": torch_glue, "glue_fused": fused_glue}


def step_legs(P, H, W, V, dev):
    """The `views_fused` step of tools/train_step.py with each glue (same parameters, cameras and random decisions)."""
    from dreamscene_amd import densify, glue, synth
    from dreamscene_amd.optim import FusedAdam
    from dreamscene_amd.rasterizer import RasterContext
    from dreamscene_amd.views import GaussianRasterizerViews
    from tools import train_step as TS
    K, D = 16, 3
    g = synth.g_object(P, seed=0, K=K)
    rng = np.random.default_rng(11)
    cams = [synth.orbit_camera(float(rng.uniform(5.2, 5.5)), float(rng.uniform(60.0, 90.0)), 360.0 * i / 64.0,
                               float(rng.uniform(0.32, 0.60)), H, W) for i in range(64)]
    op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
    raw0 = dict(_xyz=g["means3D"], _features_dc=g["shs"][:, :1], _features_rest=g["shs"][:, 1:],
                _opacity=np.log(op / (1 - op)).reshape(P, 1), _scaling=np.log(g["scales"]), _rotation=g["rotations"])
    targets = torch.rand((V, 3, H, W), device=dev)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)
    cam_t = [(c, t(c.world_view_transform), t(c.full_proj_transform), t(c.camera_center)) for c in cams]
    white, black = t([1.0, 1.0, 1.0]), t([0.0, 0.0, 0.0])
    from dreamscene_amd.rasterizer import GaussianRasterizationSettings

    def make(fused):
        lv = {k: torch.tensor(np.ascontiguousarray(v, dtype=np.float32), device=dev, requires_grad=True) for k, v in raw0.items()}
        opt = FusedAdam([{"params": [lv[k]], "lr": TS.LRS[k], "name": k} for k in TS.LRS], lr=0.0, eps=1e-15)
        stats, rc, pyrng = densify.DensifyStats(P, dev), RasterContext(), random.Random(5)

        def step(i):
            vs = []
            for j in range(V):
                c, vm, pm, cp = cam_t[(V * i + j) % 64]
                sh = 0 if pyrng.random() < TS.SH_DEG_AUG else D
                bg = white
                if pyrng.random() < TS.BG_AUG:
                    bg = torch.rand(3, device=dev) if pyrng.random() < 0.5 else black
                vs.append((c, GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy,
                                                            bg=bg, scale_modifier=1.0, viewmatrix=vm, projmatrix=pm, sh_degree=sh,
                                                            campos=cp, prefiltered=False, score_flag=False)))
            scales = torch.exp(lv["_scaling"])
            rots = torch.nn.functional.normalize(lv["_rotation"])
            opac = torch.sigmoid(lv["_opacity"])
            shs = torch.cat((lv["_features_dc"], lv["_features_rest"]), dim=1)
            vsp = torch.zeros((V, P, 3), device=dev, requires_grad=True)
            sc = torch.clamp(scales[None] + torch.randn((V, P, 3), device=dev) * ((0.2 ** 0.5) * scales[None] / 4), 0.0)
            with stats.collect(rc):
                outs = GaussianRasterizerViews([s for _, s in vs], context=rc)(
                    means3D=lv["_xyz"], means2D=vsp, shs=shs, opacities=opac, scales=sc, rotations=rots)
            images = torch.stack([o[0] for o in outs], dim=0)
            if fused:
                depths, _ = glue.disp_from_depth_alpha([o[2] for o in outs], [c.FoVx for c, _ in vs])
                tv = glue.tv_loss(images) + glue.tv_loss(depths)
            else:
                depths = torch.stack([TS.disp_on_device(o[2], c.FoVx)[0] for (c, _), o in zip(vs, outs)], dim=0)
                tv = TS.tv_loss(images) + TS.tv_loss(depths)
            guidance = TS.LAMBDA_GUIDANCE * ((images - targets) ** 2).mean()
            loss_scale = torch.mean(torch.stack(list(sc), dim=0), dim=-1).mean()
            (guidance + TS.LAMBDA_TV * tv + TS.LAMBDA_SCALE * loss_scale).backward()
            opt.step(set_to_none=True)
        return step
    return {"step_torch": make(False), "step_fused": make(True)}


def rendered_inputs(P, H, W, V, dev):
    """depth_alpha and images of V C3 views, rendered by the rasterizer (tools/train_step.py's cameras)."""
    from dreamscene_amd import synth
    from dreamscene_amd.rasterizer import GaussianRasterizationSettings
    from dreamscene_amd.views import GaussianRasterizerViews
    g = synth.g_object(P, seed=0, K=16)
    rng = np.random.default_rng(11)
    cams = [synth.orbit_camera(float(rng.uniform(5.2, 5.5)), float(rng.uniform(60.0, 90.0)), 360.0 * i / 64.0,
                               float(rng.uniform(0.32, 0.60)), H, W) for i in range(V)]
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)
    sets = [GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t([1, 1, 1]),
                                          scale_modifier=1.0, viewmatrix=t(c.world_view_transform),
                                          projmatrix=t(c.full_proj_transform), sh_degree=3, campos=t(c.camera_center),
                                          prefiltered=False, score_flag=False) for c in cams]
    p = {k: t(v) for k, v in g.items()}
    with torch.no_grad():
        outs = GaussianRasterizerViews(sets)(means3D=p["means3D"], means2D=None, shs=p["shs"], opacities=p["opacities"],
                                             scales=p["scales"], rotations=p["rotations"])
    planes = [o[2].detach().clone().requires_grad_(True) for o in outs]
    images = [o[0].detach().clone().requires_grad_(True) for o in outs]
    masked = [float((o[2][1] <= 0.1).float().mean()) for o in outs]
    return planes, images, [c.FoVx for c in cams], masked


def window(fn, seconds, dev, i0=0):
    torch.cuda.synchronize(dev)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn(i0 + n) if fn.__code__.co_argcount else fn()
        n += 1
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=500000)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--profile-leg", choices=["glue_torch", "glue_fused"])
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, H, W, V = a.gaussians, a.res, a.res, a.views
    if a.profile_leg:
        gen = torch.Generator().manual_seed(0)
        planes = []
        for _ in range(V):
            da = torch.empty((2, H, W))
            da[0] = torch.rand((H, W), generator=gen) * 5 + 0.5
            da[1] = torch.rand((H, W), generator=gen)
            planes.append(da.to(dev).requires_grad_(True))
        images = [torch.rand((3, H, W), generator=gen).to(dev).requires_grad_(True) for _ in range(V)]
        fn = glue_legs(planes, images, [0.4, 0.45, 0.5, 0.55][:V] + [0.5] * max(0, V - 4))[a.profile_leg]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize(dev)
        print(json.dumps({"profile_leg": a.profile_leg, "iters": a.iters}))
        return
    planes, images, fovs, masked = rendered_inputs(P, H, W, V, dev)
    legs = glue_legs(planes, images, fovs)
    res = {"workload": f"C3: {P} Gaussians, {V} views @{W}x{H}, depth_alpha rendered by the rasterizer; forward + backward",
           "masked_fraction": [round(m, 4) for m in masked]}
    # the two glues compute the same disp (bits) -- checked here so that the timing compares like with like
    from dreamscene_amd import glue
    from tools import train_step as TS
    with torch.no_grad():
        d_f, _ = glue.disp_from_depth_alpha(planes, fovs)
        d_t = torch.stack([TS.disp_on_device(da, f)[0] for da, f in zip(planes, fovs)])
        res["disp_bits_equal"] = bool(torch.equal(d_f.view(torch.int32), d_t.view(torch.int32)))
    groups = [("glue_torch", "glue_fused")] + ([] if a.no_step else [("step_torch", "step_fused")])
    if not a.no_step:
        legs.update(step_legs(P, H, W, V, dev))
    for A, B in groups:
        ms = {A: [], B: []}
        for name in (A, B):
            for i in range(a.warmup):
                legs[name](i) if legs[name].__code__.co_argcount else legs[name]()
        i0 = a.warmup
        for _ in range(a.rounds):
            for name in (A, B):
                t, n = window(legs[name], a.seconds, dev, i0)
                i0 += n
                ms[name].append(t)
        for name in (A, B):
            res[name] = {"ms": round(statistics.median(ms[name]), 4), "windows_ms": [round(x, 4) for x in ms[name]]}
        res[f"{A}_over_{B}"] = round(res[A]["ms"] / res[B]["ms"], 3)
        res[f"{A}_minus_{B}_ms"] = round(res[A]["ms"] - res[B]["ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
