"""The three pieces of GaussianModel's lifecycle that csrc/model.hip fuses, each against the torch chain of the reference's op
sequence on the GPU (tests/model_ref.py: gs_renderer.py:582-608, :746-749 with :854-868, :1061-1065), K = 16:
  create   create_from_pcd(pcd, dist2=...) -- the kNN is shared (run once, handed to both legs); both legs include the host's
           float64 -> fp32 conversion and the copy to the device, which is what a trainer pays;
  reset    reset_opacity with Adam moments present;
  stats    add_densification_stats with 35 % of the rows visible.
Method (guide: measuring on the MI355X): the legs alternate in one process (ref fused ref fused ...); a leg's figure is the median
of three windows of >= 0.5 s of back-to-back calls, each window closed by one device synchronisation; reset replaces its parameter
on every call, so it runs on the same optimizer call after call.
--train-step adds the fourth leg to tools/train_step.py's shape: the as-imported trainer loop (render_api.object_render per view,
the trainer's max_radii2D update) with dreamscene_amd.model.GaussianModel as its model -- FusedAdam and add_densification_stats
behind the reference's calls -- next to train_step's own `as_imported` (torch.optim.Adam and boolean-mask statistics).
usage: python tools/bench_model.py [--rows 500000,1200000] [--window 0.5] [--train-step]"""
import argparse
import json
import os
import random
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K_DEGREE = 3
ARGS = types.SimpleNamespace(iterations=2000, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                             feature_lr=5e-3, feature_lr_final=3e-3, opacity_lr=5e-2, scaling_lr=5e-3, scaling_lr_final=1e-3,
                             rotation_lr=1e-3, rotation_lr_final=2e-4, percent_dense=0.003)


def window(fn, seconds, dev):
    torch.cuda.synchronize(dev)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        n += 1
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n


def alternate(legs, seconds, dev, windows=3):
    for fn in legs.values():
        fn()
    times = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            times[k].append(window(fn, seconds, dev))
    out = {k: {"median_ms": 1e3 * statistics.median(v), "windows_ms": [round(1e3 * x, 4) for x in v]} for k, v in times.items()}
    out["ref_over_fused"] = out["ref"]["median_ms"] / out["fused"]["median_ms"]
    return out


def ops(P, dev, seconds):
    from dreamscene_amd import knn
    from dreamscene_amd import model as M
    from tests.model_ref import TorchModel
    rng = np.random.default_rng(0)
    pcd = M.BasicPointCloud(points=rng.normal(size=(P, 3)), colors=rng.random((P, 3)), normals=np.zeros((P, 3)))
    dist2 = knn.distCUDA2(torch.tensor(pcd.points, dtype=torch.float32, device=dev))
    models = {"ref": TorchModel({"sh_degree": K_DEGREE}, "scene"), "fused": M.GaussianModel({"sh_degree": K_DEGREE}, "scene")}
    res = {"create": alternate({k: (lambda m=m: m.create_from_pcd(pcd, True, 1, dist2=dist2)) for k, m in models.items()},
                               seconds, dev)}
    grad = torch.randn(P, 3, device=dev) * 1e-3
    seen = torch.rand(P, device=dev) < 0.35
    vsp = types.SimpleNamespace(grad=grad)
    for m in models.values():
        m.training_setup(ARGS)
        m._opacity.grad = torch.randn_like(m._opacity)
        m.optimizer.step()                                   # moments present
    res["stats"] = alternate({k: (lambda m=m: m.add_densification_stats(vsp, seen)) for k, m in models.items()}, seconds, dev)
    res["reset"] = alternate({k: m.reset_opacity for k, m in models.items()}, seconds, dev)
    return res


def train_step_leg(P, H, W, V, dev, seconds):
    """tools/train_step.py's `as_imported` loop with the model container in place of loose leaves, Adam and indexing."""
    from dreamscene_amd import model as M
    from dreamscene_amd import render_api, synth
    from tools import train_step as TS
    g = synth.g_object(P, seed=0, K=16)
    op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
    gm = M.GaussianModel({"sh_degree": K_DEGREE}, "scene")
    leaf = lambda a: torch.nn.Parameter(torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev))
    gm._xyz, gm._features_dc, gm._features_rest = leaf(g["means3D"]), leaf(g["shs"][:, :1]), leaf(g["shs"][:, 1:])
    gm._opacity, gm._scaling, gm._rotation = leaf(np.log(op / (1 - op)).reshape(P, 1)), leaf(np.log(g["scales"])), leaf(g["rotations"])
    gm._background = torch.nn.Parameter(torch.zeros(3, 1, 1, device=dev))
    gm.spatial_lr_scale, gm.active_sh_degree = 1, K_DEGREE
    gm.training_setup(ARGS)
    rng = np.random.default_rng(11)
    cams = [synth.orbit_camera(float(rng.uniform(5.2, 5.5)), float(rng.uniform(60.0, 90.0)), 360.0 * i / 64.0,
                               float(rng.uniform(0.32, 0.60)), H, W) for i in range(64)]
    targets = torch.rand((V, 3, H, W), device=dev)
    white = torch.ones(3, device=dev)
    pyrng = random.Random(5)

    def step(i):
        images, depths, scales = [], [], []
        for j in range(V):
            out = render_api.object_render(gm, cams[(V * i + j) % 64], white, test=False, sh_deg_aug_ratio=TS.SH_DEG_AUG,
                                           bg_aug_ratio=TS.BG_AUG, shs_aug_ratio=TS.SHS_AUG, scale_aug_ratio=TS.SCALE_AUG, rng=pyrng)
            images.append(out["image"]); depths.append(out["depth"]); scales.append(out["scales"])
        images, depths = torch.stack(images, dim=0), torch.stack(depths, dim=0)
        loss = TS.LAMBDA_GUIDANCE * ((images - targets) ** 2).mean() + TS.LAMBDA_TV * (TS.tv_loss(images) + TS.tv_loss(depths)) + \
            TS.LAMBDA_SCALE * torch.mean(torch.stack(scales, dim=0), dim=-1).mean()
        loss.backward()
        vis, radii = out["visibility_filter"], out["radii"]
        gm.max_radii2D[vis] = torch.max(gm.max_radii2D[vis], radii[vis].float())
        gm.add_densification_stats(out["viewspace_points"], vis)
        gm.optimizer.step()
        gm.optimizer.zero_grad(set_to_none=True)

    for i in range(5):
        step(i)
    torch.cuda.synchronize(dev)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(4):
            step(5 + n)
            n += 1
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / n
    ref = TS.measure(P, H, W, V, dev=dev, seconds=seconds, legs=("as_imported",))
    return {"as_imported_with_model": {"ms_per_step": round(dt * 1e3, 3), "steps": n}, **ref}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="500000,1200000")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--train-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for P in (int(x) for x in a.rows.split(",")):
        print(json.dumps({"tool": "bench_model", "rows": P, "K": (K_DEGREE + 1) ** 2, "window_s": a.window, **ops(P, dev, a.window)}),
              flush=True)
    if a.train_step:
        # bench.py's `trainer_step` shape (C3): 500 k Gaussians, 1024 x 1024, four views per step
        print(json.dumps({"tool": "bench_model", "leg": "train_step", "rows": 500000, "image": [1024, 1024], "views": 4,
                          **train_step_leg(500000, 1024, 1024, 4, dev, 1.5)}), flush=True)


if __name__ == "__main__":
    main()
