"""3D Gaussian filtering's middle -- calculate_v_imp_score and the mask of prune_gaussians (scene_gaussian.py:1046-1061,
gs_renderer.py:1082-1087) -- three ways on the GPU, at P = 500 k and 1.2 M:
  ref     the reference's chain of torch operations, two full torch.sort;
  kth     today's densify.v_importance + densify.importance_prune_mask, two torch.kthvalue;
  fused   filtering.importance_filter (csrc/select.hip), one C call, ten launches.
No leg reads anything on the host. Method (guide: measuring on the MI355X): the legs alternate in one process (ref kth fused ref
...); a leg's figure is the median of three windows of >= 0.5 s of back-to-back calls, each window closed by one device
synchronisation. Launch counts: device kernels per call as torch's profiler sees them.
Then the whole gaussian_filtering at 500 k Gaussians, K = 16, with 48 synth.sphere_cameras at 512 x 512 and the prune with Adam
moments included: filtering.gaussian_filtering against the same call assembled from today's pieces (views.importance_scores,
densify.v_importance, GaussianModel.prune_gaussians). Every call shrinks its model, so each is timed on a model of its own (built
outside the timed region), one synchronisation on either side; the legs alternate and the figure is the median of the calls.
usage: python tools/bench_filtering.py [--rows 500000,1200000] [--window 0.5] [--no-end-to-end] [--calls 5]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

V_POW, PERCENT = 0.1, 0.4                                    # configs: v_pow 0.1, prune_decay 0.8 * prune_percent 0.5
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


def launches(fn, dev):
    """Device kernels one call enqueues (None where the profiler reports none)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize(dev)
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize(dev)
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception:
        return None
    return n or None


def middle(P, dev, seconds, windows=3):
    from dreamscene_amd import densify, filtering
    rng = np.random.default_rng(P)
    scaling = torch.tensor(np.exp(np.log(0.02) + rng.normal(scale=0.5, size=(P, 3))).astype(np.float32), device=dev)
    imp = torch.tensor(rng.gamma(2.0, 30.0, size=P).astype(np.float32), device=dev)

    def ref():
        volume = torch.prod(scaling, dim=1)
        sorted_volume, _ = torch.sort(volume, descending=True)
        v_list = torch.pow(volume / sorted_volume[int(len(volume) * 0.9)], V_POW) * imp
        sortedvalues, _ = torch.sort(v_list)
        return (v_list <= sortedvalues[int(PERCENT * (len(sortedvalues) - 1))]).squeeze()

    def kth():
        return densify.importance_prune_mask(densify.v_importance(scaling, imp, V_POW), PERCENT)

    def fused():
        return filtering.importance_filter(scaling, imp, V_POW, PERCENT).mask

    legs = {"ref": ref, "kth": kth, "fused": fused}
    masks = {k: fn() for k, fn in legs.items()}
    agree = {k: int((masks[k] != masks["ref"]).sum()) for k in ("kth", "fused")}
    times = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            times[k].append(window(fn, seconds, dev))
    out = {k: {"median_ms": round(1e3 * statistics.median(v), 4), "windows_ms": [round(1e3 * x, 4) for x in v],
               "launches": launches(legs[k], dev)} for k, v in times.items()}
    out["mask_entries_differing_from_ref"] = agree
    out["ref_over_fused"] = round(out["ref"]["median_ms"] / out["fused"]["median_ms"], 3)
    out["kth_over_fused"] = round(out["kth"]["median_ms"] / out["fused"]["median_ms"], 3)
    return out


def end_to_end(P, H, W, n_cams, dev, calls):
    from dreamscene_amd import densify, filtering, synth, views
    from dreamscene_amd import model as M
    g = synth.g_object(P, seed=0, K=16)
    op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
    host = dict(_xyz=g["means3D"], _features_dc=g["shs"][:, :1], _features_rest=g["shs"][:, 1:],
                _opacity=np.log(op / (1 - op)).reshape(P, 1), _scaling=np.log(g["scales"]), _rotation=g["rotations"])
    master = {k: torch.tensor(np.ascontiguousarray(v, dtype=np.float32), device=dev) for k, v in host.items()}
    cams = synth.sphere_cameras(n_cams, H, W)
    white = torch.ones(3, device=dev)

    def fresh():
        gm = M.GaussianModel({"sh_degree": 3}, "scene")
        for k, v in master.items():
            setattr(gm, k, torch.nn.Parameter(v.clone()))
        gm._background = torch.nn.Parameter(torch.zeros(3, 1, 1, device=dev))
        gm.spatial_lr_scale, gm.active_sh_degree = 1, 3
        gm.training_setup(ARGS)
        for k in master:
            getattr(gm, k).grad = torch.full_like(master[k], 1e-3)
        gm.optimizer.step()                                  # Adam moments present
        gm.optimizer.zero_grad(set_to_none=True)
        return gm

    settings = filtering._score_settings(fresh(), cams, white)

    def pieces(gm):
        with torch.no_grad():
            scores = views.importance_scores(settings, gm.get_xyz, gm.get_opacity, shs=gm.get_features, scales=gm.get_scaling,
                                             rotations=gm.get_rotation)
            gm.prune_gaussians(PERCENT, densify.v_importance(gm.get_scaling, scores, V_POW))

    def fused(gm):
        filtering.gaussian_filtering(gm, cams, white, V_POW, 0.8, 0.5)

    legs = {"pieces": pieces, "fused": fused}
    for fn in legs.values():                                 # twice: the first call learns the views' pair counts
        fn(fresh())
        fn(fresh())
    times, rows = {k: [] for k in legs}, {}
    for _ in range(calls):
        for k, fn in legs.items():
            gm = fresh()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn(gm)
            torch.cuda.synchronize(dev)
            times[k].append(time.perf_counter() - t0)
            rows[k] = gm._xyz.shape[0]
    out = {k: {"median_ms": round(1e3 * statistics.median(v), 3), "calls_ms": [round(1e3 * x, 3) for x in v], "rows_left": rows[k]}
           for k, v in times.items()}
    out["pieces_over_fused"] = round(out["pieces"]["median_ms"] / out["fused"]["median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="500000,1200000")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for P in (int(x) for x in a.rows.split(",")):
        print(json.dumps({"tool": "bench_filtering", "leg": "middle", "rows": P, "v_pow": V_POW, "percent": PERCENT,
                          "window_s": a.window, **middle(P, dev, a.window)}), flush=True)
    if not a.no_end_to_end:
        print(json.dumps({"tool": "bench_filtering", "leg": "gaussian_filtering", "rows": 500000, "K": 16, "image": [512, 512],
                          "cameras": 48, **end_to_end(500000, 512, 512, 48, dev, a.calls)}), flush=True)


if __name__ == "__main__":
    main()
