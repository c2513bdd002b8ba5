"""Starting a model from a fresh point cloud, two ways, at the reference's sizes (indoor env 5 x 400 k rows, indoor floor 300 k,
`default` ball 100 k), sh_degree 3:
  ref     the reference-shaped host leg: the cloud drawn with numpy's float64 stream in the reference's op sequence
          (gs_renderer.py:221-248, :282-296, :353-369), then GaussianModel.create_from_pcd (fp32 conversion, copy, kNN, leaves);
  fused   SeededGaussianModel: the cloud drawn on the device (csrc/sample.hip), kNN and leaves with no host round trip;
  kernel  the sampling launch alone (pointcloud.sample_*, output tensors included).
Both model legs run the same kNN, which dominates them at these sizes; `kernel` shows what the draw itself costs.
Method (guide: measuring on the MI355X; tools/bench_model.py): the legs alternate in one process (ref fused kernel ref ...); a leg's
figure is the median of three windows of >= --window seconds of back-to-back calls, each closed by one device synchronisation.
usage: python tools/bench_sample.py [--window 0.5] [--clouds env,floor,ball]"""
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

BOX = np.array([-3.5, -2.5, 0.0, 3.5, 2.5, 5.0])
FLOOR_COLOR = (120.0, 90.0, 60.0)
SH_DEGREE = 3
SH_C0 = 0.28209479177387814


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
    out = {k: {"median_ms": round(1e3 * statistics.median(v), 4), "windows_ms": [round(1e3 * x, 4) for x in v]}
           for k, v in times.items()}
    out["ref_over_fused"] = round(out["ref"]["median_ms"] / out["fused"]["median_ms"], 3)
    return out


def host_env(n):
    r = np.random.random
    walls = np.ones((n, 6)) * BOX
    walls[:, :3] -= r((n, 3)) / 50.0
    walls[:, 3:] += r((n, 3)) / 50.0
    xs, ys, zs = (r((n,)) * (BOX[3 + k] - BOX[k]) + BOX[k] for k in range(3))
    xyz = np.concatenate([np.stack(s, axis=1) for s in ((walls[:, 0], ys, zs), (walls[:, 3], ys, zs), (xs, walls[:, 1], zs),
                                                          (xs, walls[:, 4], zs), (xs, ys, walls[:, 5]))])
    colors = np.concatenate([v * np.ones((n, 3)) for v in (0.5, 0.5, 0.7, 0.7, 0.9)])
    return xyz, colors


def host_floor(n):
    r = np.random.random
    walls = np.ones((n, 6)) * BOX + r((n, 6)) / 50.0 - 0.01
    xs, ys = (r((n,)) * (BOX[3 + k] - BOX[k]) + BOX[k] for k in range(2))
    colors = np.ones((n, 3)) * np.minimum(np.array(FLOOR_COLOR) / 255.0, 1.0)
    return np.stack((xs, ys, walls[:, 2]), axis=1), colors


def host_ball(n, radius=0.5):
    r = np.random.random
    phi, theta = r((n,)) * 2 * np.pi, np.arccos(r((n,)) * 2 - 1)
    rad = radius * np.cbrt(r((n,)))
    xyz = np.stack((rad * np.sin(theta) * np.cos(phi), rad * np.sin(theta) * np.sin(phi), rad * np.cos(theta)), axis=1)
    return xyz, r((n, 3)) / 255.0 * SH_C0 + 0.5


def legs_for(cloud, dev):
    from dreamscene_amd import model as M
    from dreamscene_amd import pointcloud as PC
    host = M.GaussianModel({"sh_degree": SH_DEGREE}, "scene")
    scene = dict(sh_degree=SH_DEGREE, cam_pose_method="indoor", scene_box=torch.tensor(BOX, dtype=torch.float32, device=dev),
                 floor_init_color=FLOOR_COLOR, seed=1)
    if cloud == "env":
        n = PC.ENV_INDOOR_PTS

        def ref():
            xyz, col = host_env(n)
            host.create_from_pcd(M.BasicPointCloud(xyz, col, None), True, 1)
        return 5 * n, {"ref": ref, "fused": lambda: PC.SeededGaussianModel(scene, "env"),
                       "kernel": lambda: PC.sample_env("indoor", scene["scene_box"], seed=1)}
    if cloud == "floor":
        n = PC.FLOOR_INDOOR_PTS

        def ref():
            xyz, col = host_floor(n)
            host.create_from_pcd(M.BasicPointCloud(xyz, col, None), False, 1)
        return n, {"ref": ref, "fused": lambda: PC.SeededGaussianModel(scene, "floor"),
                   "kernel": lambda: PC.sample_floor("indoor", scene["scene_box"], seed=1, floor_init_color=FLOOR_COLOR)}
    n = 100_000
    obj = dict(sh_degree=SH_DEGREE, init_guided="default", init_prompt="", num_pts=n, radius=0.5, seed=1)

    def ref():
        xyz, col = host_ball(n)
        host.create_from_pcd(M.BasicPointCloud(xyz, col, None), True, 10)
    return n, {"ref": ref, "fused": lambda: PC.SeededGaussianModel(obj, "object", "unused"),
               "kernel": lambda: PC.sample_ball(n, 0.5, seed=1, device=dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--clouds", default="env,floor,ball")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    np.random.seed(0)
    for cloud in a.clouds.split(","):
        rows, legs = legs_for(cloud, dev)
        print(json.dumps({"tool": "bench_sample", "cloud": cloud, "rows": rows, "K": (SH_DEGREE + 1) ** 2, "window_s": a.window,
                          **alternate(legs, a.window, dev)}), flush=True)


if __name__ == "__main__":
    main()
