"""The scene path's augmentation noise: tensors drawn with torch.randn against the generator inside K1 / K8 (scene.NoiseSpec).
Every leg is one training step of the fused raw-leaf path: scene.rasterize_models_views over 4 views, forward plus backward
to the leaves, scale noise and SH noise on every view.
  randn    (a) torch.randn of both tensors ([V,P,3] and [V,P,K,3]) inside the step, then the tensor form
  tensors  (b) the tensor form with the tensors drawn once, outside: the kernels alone
  tensors2     leg (b) again: the spread of a repeated leg, the yardstick for "(b) did not move" against another build
  seeded   (c) noise=NoiseSpec(seed, step * V): no noise tensor exists
Shapes (--shapes): c3 = one model of 500 k Gaussians, K = 16, 1024^2; indoor = 5 x 400 k + 300 k Gaussians (synth.g_indoor), K = 16,
1024^2; small = 100 k Gaussians, 512^2.
Method: the legs alternate in one process (a b b c a b b c ...), each window >= --seconds of whole steps after a warm-up, one device
synchronisation at both ends of a window; the median window per leg is reported, with all windows. noise_bytes_avoided: the
bytes of the two tensors of one step, computed from the shapes (they are written once by randn and read by K1 and K8).
Kernel times (K1, K8, torch's randn kernels) come from a separate run under a kernel tracer:
  rocprofv3 --kernel-trace --stats -- python tools/bench_noise.py --shapes c3 --legs randn seeded --rounds 1
--legs without `seeded` runs on a build that has no NoiseSpec.
usage: python tools/bench_noise.py [--shapes c3 indoor small] [--legs randn tensors tensors2 seeded] [--seconds 0.5] [--rounds 3]"""
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

V = 4
SHAPES = {"c3": dict(kind="object", sizes=[500_000], K=16, res=1024),
          "indoor": dict(kind="indoor", sizes=[400_000] * 5 + [300_000], K=16, res=1024),
          "small": dict(kind="object", sizes=[100_000], K=16, res=512)}
LEGS = ("randn", "tensors", "tensors2", "seeded")


def build(shape, dev):
    from dreamscene_amd import synth
    from dreamscene_amd.rasterizer import GaussianRasterizationSettings
    K, H, W = shape["K"], shape["res"], shape["res"]
    P = sum(shape["sizes"])
    if shape["kind"] == "indoor":
        g = synth.g_indoor(seed=0, per_wall=-(-P // 5), K=K)
        cams = synth.indoor_cameras(V, H, W)
    else:
        g = synth.g_object(P, seed=0, K=K)
        cams = synth.object_cameras(V, H, W)
    g = {k: v[:P] for k, v in g.items()}
    cuts = np.concatenate([[0], np.cumsum(shape["sizes"])])
    op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
    raw = (g["means3D"], np.log(np.maximum(g["scales"], 1e-12)), g["rotations"] * 1.7, np.log(op / (1 - op)),
           g["shs"][:, :1, :], g["shs"][:, 1:, :])
    models = [tuple(torch.tensor(np.ascontiguousarray(x[cuts[m]:cuts[m + 1]], dtype=np.float32), device=dev, requires_grad=True)
                    for x in raw) for m in range(len(shape["sizes"]))]
    t = lambda v: torch.tensor(np.asarray(v, dtype=np.float32), device=dev)      # noqa: E731
    sets = [GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t([1, 1, 1]),
                                          scale_modifier=1.0, viewmatrix=t(c.world_view_transform),
                                          projmatrix=t(c.full_proj_transform), sh_degree=3, campos=t(c.camera_center),
                                          prefiltered=False, score_flag=False) for c in cams]
    gi_np, gda_np = synth.upstream_grads(H, W, seed=0)
    return models, sets, torch.tensor(gi_np, device=dev), torch.tensor(gda_np, device=dev), P


def legs_of(shape, dev):
    from dreamscene_amd import scene
    models, sets, gi, gda, P = build(shape, dev)
    K = shape["K"]
    leaves = [x for m in models for x in m]
    fixed = (torch.randn((V, P, 3), device=dev), torch.randn((V, P, K, 3), device=dev))
    step_no = [0]

    def step(**noise):
        for x in leaves:
            x.grad = None
        m2d = torch.zeros((V, P, 3), device=dev, requires_grad=True)
        outs = scene.rasterize_models_views(sets, models, m2d, **noise)
        sum((img * gi).sum() + (da * gda).sum() + 0.01 * sc.mean() for img, _, da, sc in outs).backward()

    def randn():
        step(scale_noise=torch.randn((V, P, 3), device=dev), sh_noise=torch.randn((V, P, K, 3), device=dev))

    def tensors():
        step(scale_noise=fixed[0], sh_noise=fixed[1])

    def seeded():
        step_no[0] += 1
        step(noise=scene.NoiseSpec(20240607, (step_no[0] * V) & 0xFFFFFFFF))

    return {"randn": randn, "tensors": tensors, "tensors2": tensors, "seeded": seeded}, P


def window(fn, seconds, dev):
    torch.cuda.synchronize(dev)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        n += 1
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"workload": f"rasterize_models_views, {V} views, forward + backward, scale and SH noise on every view", "shapes": {}}
    for name in a.shapes:
        shape = SHAPES[name]
        legs, P = legs_of(shape, dev)
        for leg in a.legs:
            for _ in range(a.warmup):
                legs[leg]()
        ms = {leg: [] for leg in a.legs}
        for _ in range(a.rounds):
            for leg in a.legs:
                ms[leg].append(window(legs[leg], a.seconds, dev))
        res = {leg: {"ms_per_step": round(statistics.median(ms[leg]), 4), "windows_ms": [round(x, 4) for x in ms[leg]]}
               for leg in a.legs}
        res["gaussians"], res["K"], res["res"] = P, shape["K"], shape["res"]
        res["noise_bytes_avoided_per_step"] = V * P * (3 + 3 * shape["K"]) * 4
        if "tensors" in res and "tensors2" in res:
            res["repeat_spread"] = round(abs(res["tensors"]["ms_per_step"] - res["tensors2"]["ms_per_step"]) /
                                         res["tensors"]["ms_per_step"], 4)
        if "seeded" in res:
            for other in ("randn", "tensors"):
                if other in res:
                    res[f"{other}_over_seeded"] = round(res[other]["ms_per_step"] / res["seeded"]["ms_per_step"], 3)
        out["shapes"][name] = res
        del legs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
