"""Object placement on the device: the reference's op sequence (scene_gaussian.py:329-385) restated in torch against the fused
call (dreamscene_amd.compose.place, csrc/compose.hip).
  ref     R @ S @ xyz^T, min (with the reference's .item() host read), + T, permute; scaling + log(scale); the three band
          products on a clone of f_rest; quaternion_raw_multiply; min / max of the result. The band matrices are
          compose.sh_band_matrices on the COEFFICIENT axis, so that both legs do the same mathematics (the reference's own
          band 1 mixes the colour axis and its bands 2, 3 need e3nn).
  fused   compose.place(copy=False): two launches plus its allocations;
  raw     gsr_place alone into preallocated outputs (what a captured graph replays).
Method: the legs alternate in one process after --warmup calls each; every timed call sits between two device events on the
current stream (the ref leg's host read is inside its window, as a trainer pays it); median, minimum, maximum and inter-quartile
range over --reps. Launches: counted with torch.profiler in a separate, untimed call (null where the profiler gives nothing).
apply_fraction_of_8TBs: the apply kernel's algorithmic bytes (read + write of xyz, scaling, rotation, f_rest: 440 B per row at
K = 16) over the time of BOTH launches of the raw leg, over 8 TB/s -- a lower bound of the apply kernel's own share, since the
window also holds the pass over xyz (12 B per row).
usage: python tools/bench_compose.py [--cases 500000:16,1200000:16,1200000:4] [--reps 50] [--warmup 5]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROTATION, SCALE, CENTER = (0.3, -0.5, 0.7, 0.4), [0.5, 1.0, 2.0], (1.5, -2.0, 0.7)


def model(P, K, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)
    return (r(P, 3), -3.0 + 0.5 * r(P, 3), r(P, 4), r(P, 1), r(P, 1, 3), 0.3 * r(P, K - 1, 3))


def ref_leg(m, dev):
    from dreamscene_amd import compose
    import numpy as np
    R64 = compose.rotation_matrix(ROTATION)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=dev)
    R, S, q = t(R64), torch.diag(t(SCALE)), t(compose.quaternion_of(R64))
    Ms = [t(M) for M in compose.sh_band_matrices(R64)]
    xyz, scaling, rot, _, _, f_rest = m

    def run():
        P = xyz.shape[0]
        y = R @ S @ xyz.permute(1, 0)
        z_min = y.min(dim=1)[0][2]
        T = t([CENTER[0], CENTER[1], CENTER[2] - z_min.item()])
        out_xyz = (y + T.unsqueeze(1).repeat(1, P)).permute(1, 0)
        out_scaling = scaling + torch.log(t(SCALE))
        fr = f_rest.clone()                      # the reference rotates the loaded object's own tensor
        for (a, b), M in zip(((0, 3), (3, 8), (8, 15)), Ms):
            if fr.shape[1] >= b:
                fr[:, a:b, :] = M.T @ fr[:, a:b, :]
        aw, ax, ay, az = q.unsqueeze(0).expand(rot.shape).unbind(-1)
        bw, bx, by, bz = rot.unbind(-1)
        out_rot = torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                               aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)
        box = torch.cat((out_xyz.min(dim=0)[0], out_xyz.max(dim=0)[0]))
        return out_xyz, out_scaling, out_rot, fr, box
    return run


def fused_leg(m):
    from dreamscene_amd import compose
    return lambda: compose.place(m, ROTATION, SCALE, CENTER, copy=False)


def raw_leg(m, K, dev):
    from dreamscene_amd import _lib, compose
    lib = _lib.load()
    P = m[0].shape[0]
    c = compose.placement_constants(ROTATION, SCALE, CENTER)
    outs = [torch.empty_like(m[k]) for k in (0, 1, 2, 5)]
    box = torch.empty(12, device=dev)
    nbytes = lib.gsr_place_scratch_bytes(P)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = _lib.GsrPlacement()
    p.P, p.K, p.ground = P, K, 1
    p.xyz, p.scaling, p.rotation, p.opacity, p.features_dc, p.features_rest = (x.data_ptr() for x in m)
    p.xyz_out, p.scaling_out, p.rotation_out, p.features_rest_out = (x.data_ptr() for x in outs)
    for name in c._fields:
        getattr(p, name)[:] = getattr(c, name).tolist()
    p.bounds, p.t_effective = box.data_ptr(), box.data_ptr() + 32

    def run():
        _lib.check(lib.gsr_place(ctypes.byref(p), scratch.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream),
                   "gsr_place")
        return outs, box
    return run


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(fn, dev):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize(dev)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize(dev)
        n = sum(1 for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower())
        return n or None
    except Exception:
        return None


def summary(ts):
    q = statistics.quantiles(ts, n=4)
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), iqr_ms=q[2] - q[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="500000:16,1200000:16,1200000:4")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_compose needs a ROCm device: nothing here is measured without one")
    dev = torch.device("cuda:0")
    for case in a.cases.split(","):
        P, K = (int(v) for v in case.split(":"))
        m = model(P, K, dev)
        legs = {"ref": ref_leg(m, dev), "fused": fused_leg(m), "raw": raw_leg(m, K, dev)}
        # the legs agree before anything is timed (different fp32 evaluation orders: a tolerance, not bits)
        r, f = legs["ref"](), legs["fused"]()
        for x, y in zip(r[:4], (f[0], f[1], f[2], f[5])):
            assert torch.allclose(x, y, rtol=1e-4, atol=1e-5), "the two legs disagree"
        times = {k: [] for k in legs}
        for i in range(a.warmup + a.reps):
            for k, fn in legs.items():
                t = timed(fn, dev)
                if i >= a.warmup:
                    times[k].append(t)
        apply_bytes = P * 8 * (10 + 3 * (K - 1))
        raw_med = statistics.median(times["raw"])
        out = {"tool": "bench_compose", "rows": P, "K": K, "reps": a.reps,
               "ref": summary(times["ref"]), "fused": summary(times["fused"]), "raw": summary(times["raw"]),
               "launches": {k: launches(fn, dev) for k, fn in legs.items()},
               "speedup_of_medians_fused_vs_ref": statistics.median(times["ref"]) / statistics.median(times["fused"]),
               "apply_bytes": apply_bytes, "bounds_bytes": 12 * P,
               "apply_fraction_of_8TBs": apply_bytes / (raw_med * 1e-3) / 8e12,
               "both_launches_TBs": (apply_bytes + 12 * P) / (raw_med * 1e-3) / 1e12}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
