"""The raw-leaf views step enqueued from Python against the same step replayed from captured graphs.
Every leg is one training step of the fused raw-leaf path over 4 views, forward plus backward, seeded scale noise on every view
(NoiseSpec(seed, step * V, shs=False): the reference's ratios), the gradients ADDED into model_grad_buffers:
  eager      scene.rasterize_models_views
  eager2     the same leg again: the spread of a repeated leg, the yardstick for "eager did not move" against another build
  captured   scene_graph.CapturedModelsViews (its warm-up and capture happen in the warm-up steps)
  captured2  the same leg again (its own module and capture)
--loss direct (default): the step's backward starts from fixed upstream gradient tensors (image, depth_alpha, returned scales), as
bench.py's does -- the rasterizer's own host and GPU work; --loss torch: tools/bench_noise.py's loss written in torch ops (about a
hundred small launches per step that neither leg can save).
Shapes (--shapes): small = 100 k Gaussians, K = 16, 512^2 (the regime of the reference's object training); c3 = 500 k, K = 16,
1024^2; indoor = 5 x 400 k + 300 k Gaussians (synth.g_indoor), K = 4, 1024^2.
Method (tools/bench_noise.py's): the legs alternate in one process, each window >= --seconds of whole steps after a warm-up,
one device synchronisation at both ends of a window; the median window per leg is reported, with all windows.
--legs eager eager2 runs on a build that has no scene_graph module.
usage: python tools/bench_scene_graph.py [--shapes small c3 indoor] [--legs eager eager2 captured captured2] [--seconds 0.5]
       [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_noise import V, build, window      # noqa: E402

SHAPES = {"small": dict(kind="object", sizes=[100_000], K=16, res=512),
          "c3": dict(kind="object", sizes=[500_000], K=16, res=1024),
          "indoor": dict(kind="indoor", sizes=[400_000] * 5 + [300_000], K=4, res=1024)}
LEGS = ("eager", "eager2", "captured", "captured2")
SEED = 20240607


def legs_of(shape, dev, wanted, loss):
    from dreamscene_amd import scene
    models, sets, gi, gda, P = build(shape, dev)
    sets = [s._replace(sh_degree=min(3, int(shape["K"] ** 0.5) - 1)) for s in sets]     # (the degree K coefficients hold)
    step_no = [0]
    g_sc = torch.full((P, 3), 0.01 / (3 * P), device=dev)
    ups = [x for _ in range(V) for x in (gi, gda, g_sc)]

    def context():
        return scene.SceneContext(model_grad_buffers=[tuple(torch.zeros_like(x) for x in m) for m in models])

    def leg(call):
        def step():
            step_no[0] += 1
            m2d = torch.zeros((V, P, 3), device=dev, requires_grad=True)
            outs = call(m2d, scene.NoiseSpec(SEED, (step_no[0] * V) & 0xFFFFFFFF, shs=False))
            if loss == "torch":
                sum((img * gi).sum() + (da * gda).sum() + 0.01 * sc.mean() for img, _, da, sc in outs).backward()
            else:
                torch.autograd.backward([x for img, _, da, sc in outs for x in (img, da, sc)], ups)
        return step

    def eager():
        ctx = context()
        return leg(lambda m2d, spec: scene.rasterize_models_views(sets, models, m2d, context=ctx, noise=spec))

    def captured():
        from dreamscene_amd.scene_graph import CapturedModelsViews
        rast = CapturedModelsViews(context=context())
        step = leg(lambda m2d, spec: rast(sets, models, m2d, noise=spec))
        step.stats = rast.stats
        return step
    make = {"eager": eager, "eager2": eager, "captured": captured, "captured2": captured}
    return {name: make[name]() for name in wanted}, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--loss", default="direct", choices=["direct", "torch"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"workload": f"raw-leaf step, {V} views, forward + backward, seeded scale noise, gradients into buffers", "loss": a.loss,
           "shapes": {}}
    for name in a.shapes:
        shape = SHAPES[name]
        legs, P = legs_of(shape, dev, a.legs, a.loss)
        for leg in a.legs:
            for _ in range(a.warmup):
                legs[leg]()
        ms = {leg: [] for leg in a.legs}
        for _ in range(a.rounds):
            for leg in a.legs:
                ms[leg].append(window(legs[leg], a.seconds, dev))
        res = {leg: {"ms_per_step": round(statistics.median(ms[leg]), 4), "windows_ms": [round(x, 4) for x in ms[leg]]}
               for leg in a.legs}
        for leg in a.legs:
            if hasattr(legs[leg], "stats"):
                res[leg]["stats"] = dict(legs[leg].stats)
        res["gaussians"], res["K"], res["res"] = P, shape["K"], shape["res"]
        for x, y in (("eager", "eager2"), ("captured", "captured2")):
            if x in res and y in res:
                res[f"{x}_repeat_spread"] = round(abs(res[x]["ms_per_step"] - res[y]["ms_per_step"]) / res[x]["ms_per_step"], 4)
        if "eager" in res and "captured" in res:
            res["captured_over_eager"] = round(res["captured"]["ms_per_step"] / res["eager"]["ms_per_step"], 3)
        out["shapes"][name] = res
        del legs
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
