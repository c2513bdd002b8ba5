"""densify_and_prune on the device: the torch chain of tests/densify_ref.py (GaussianModel's own op sequence, gs_renderer.py:
854-1059, the only way to do this step before dreamscene_amd.densify had it) against the fused call, K = 16, Adam moments present.
  ref     densify_ref.RefGaussians.densify_and_prune on the GPU: boolean-mask gathers + torch.cat per parameter and moment;
  fused   dreamscene_amd.densify.densify_and_prune: plan, one host read, one gather pass (csrc/densify.hip).
Workload (an ASSUMPTION about training, not a measurement of it): about 5 % of the rows cloned, 5 % split, 2 % pruned; the shares
the state really has are on the output line.
Method: the legs alternate in one process (a b a b ...) from fresh copies of the same state, --reps timed calls each after
--warmup, the host clock around work that ends in a device synchronise (both legs include their host reads: that is what a trainer
pays); median, minimum, maximum and inter-quartile range per leg; peak memory of each from torch.cuda.max_memory_allocated.
gather_bytes: the algorithmic bytes of the gather kernel (read + write of every output row of the 18 tensors + the statistics).
--profile-leg ref|fused: only that leg --reps times, for a `rocprofv3 --kernel-trace --stats -- python tools/bench_densify.py ...`
pass (kernels per call = kernels in the trace / --reps, minus the state copies).
usage: python tools/bench_densify.py [--rows 500000,1200000] [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
TH = dict(max_grad=0.0002, min_opacity=0.005, extent=2.0, percent_dense=0.01)
K, N = 16, 2


def base_state(P, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)
    u = lambda *s: torch.rand(*s, generator=g, device=dev)
    st = {"xyz": r(P, 3), "f_dc": r(P, 1, 3), "f_rest": r(P, K - 1, 3), "rotation": r(P, 4)}
    big = u(P) < 0.5                                     # half the rows above the clone / split threshold 0.02
    top = torch.where(big, 0.03 + 0.1 * u(P), 0.004 + 0.012 * u(P))
    st["scaling"] = torch.log(top[:, None] * (0.3 + 0.7 * u(P, 3)))
    o = torch.where(u(P) < 0.02, 0.001 + 0.003 * u(P), 0.05 + 0.9 * u(P))          # 2 % below min_opacity
    st["opacity"] = torch.log(o / (1 - o))[:, None]
    st["denom"] = torch.randint(1, 6, (P,), generator=g, device=dev).float()
    grad = torch.where(u(P) < 0.10, 0.0003 + 0.001 * u(P), 0.00015 * u(P))         # 10 % selected: ~5 % clone, ~5 % split
    st["xyz_gradient_accum"] = grad * st["denom"]
    st["max_radii2D"] = torch.floor(30 * u(P))
    for n in NAMES:
        st[n + "/m1"] = 0.01 * r(*st[n].shape)
        st[n + "/m2"] = 1e-4 * r(*st[n].shape) ** 2
    return st


def fresh(st, dev):
    params = {n: nn.Parameter(st[n].clone()) for n in NAMES}
    opt = torch.optim.Adam([{"params": [params[n]], "lr": 1e-3, "name": n} for n in NAMES], lr=0.0, eps=1e-15)
    for n in NAMES:
        opt.state[params[n]] = {"step": torch.tensor(3.0), "exp_avg": st[n + "/m1"].clone(), "exp_avg_sq": st[n + "/m2"].clone()}
    return opt, tuple(st[k].clone() for k in ("xyz_gradient_accum", "denom", "max_radii2D"))


def legs(st, dev, noise):
    from dreamscene_amd import densify
    from tests import densify_ref as DR

    def ref():
        opt, (accum, denom, radii) = fresh(st, dev)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        m = DR.RefGaussians(opt, accum, denom, radii, percent_dense=TH["percent_dense"])
        m.densify_and_prune(TH["max_grad"], TH["min_opacity"], TH["extent"], None, N=N, noise=noise)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, torch.cuda.max_memory_allocated(dev), m.segments(N)

    def fused():
        opt, (accum, denom, radii) = fresh(st, dev)
        stats = densify.DensifyStats(accum.shape[0], dev)
        stats.replace(radii, accum, denom)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        res = densify.densify_and_prune(opt, stats, TH["max_grad"], TH["min_opacity"], TH["extent"], None,
                                        percent_dense=TH["percent_dense"], N=N, noise=noise)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, torch.cuda.max_memory_allocated(dev), res.segments
    return {"ref": ref, "fused": fused}


def summary(ts):
    q = statistics.quantiles(ts, n=4)
    return dict(median_ms=1e3 * statistics.median(ts), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), iqr_ms=1e3 * (q[2] - q[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="500000,1200000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-leg", choices=["ref", "fused"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for P in (int(x) for x in a.rows.split(",")):
        st = base_state(P, dev)
        noise = torch.randn(N, P, 3, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        fn = legs(st, dev, noise)
        if a.profile_leg:
            for _ in range(a.reps):
                fn[a.profile_leg]()
            print(json.dumps({"tool": "bench_densify", "rows": P, "profiled_leg": a.profile_leg, "calls": a.reps}))
            continue
        times, peak, seg = {"ref": [], "fused": []}, {}, {}
        for i in range(a.warmup + a.reps):
            for leg in ("ref", "fused"):
                t, mem, seg[leg] = fn[leg]()
                if i >= a.warmup:
                    times[leg].append(t)
                    peak[leg] = max(peak.get(leg, 0), mem)
        assert tuple(seg["ref"]) == tuple(seg["fused"]), seg
        S, C, Kc = seg["fused"][:3]
        P_out = S + C + N * Kc
        floats_per_row = 14 + 3 * K                      # 3 + 3 + 3 (K - 1) + 1 + 3 + 4
        out = {"tool": "bench_densify", "rows": P, "K": K, "N": N, "P_out": P_out,
               "shares_assumed_workload": {"clone": C / P, "split": Kc / P, "pruned": (P - S - Kc) / P},
               "ref": summary(times["ref"]), "fused": summary(times["fused"]),
               "speedup_of_medians": statistics.median(times["ref"]) / statistics.median(times["fused"]),
               "fused_wins_by_more_than_ref_spread": statistics.median(times["ref"]) - statistics.median(times["fused"]) >
               max(times["ref"]) - min(times["ref"]),
               "peak_bytes": peak, "gather_bytes": P_out * (2 * 3 * floats_per_row * 4 + 3 * 4), "reps": a.reps}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
