"""Generates tests/golden/samplers.npz from the reference's OWN point-cloud samplers (gs_renderer.py:218-408: init_env_pcd,
init_floor_pcd, init_pcd), run unchanged on the CPU with a fixed np.random.seed. Like make_model_golden.py it runs only where the
reference checkout is, with make_golden.py's stubs; `create_from_pcd` and `storePly` of the reference's class are patched to
capture the cloud. Nothing of the reference travels: the fixture holds arrays only.

Per cloud `<name>` (env|floor _ indoor|outdoor _ zg0|zg1, ball, pointe):
  <name>/rows        the row count                      <name>/raises   True where the reference itself dies (floor_outdoor_zg0)
  <name>/box, /R     the scene box and radius_base (the ball: its radius)
  <name>/q           [sheets, columns, 1025] fp32: quantiles k / 1024 of each column of each sheet. Columns are x, y, z and, for
                     the clouds around the origin, |p|^3 / R^3 (the disc: (x^2 + y^2) / R^2), z / |p| and atan2(y, x)
  <name>/colors      the distinct colour rows (ball and pointe: the quantiles of the three channels instead, /qcolors)
  env_indoor_*/shared   sheets 0,1 share ys and zs, sheets 2,3 share xs and zs, sheet 4 has sheets 2's xs and sheet 0's ys
  pointe/seeds, /seed_colors, /points, /point_colors   the first 64 of the 4096 seed points given in place of Point-E's, and the
                     64 x 20 rows made of them (use_pointe_rgb); /offsets_shared: every seed point has the same 20 offsets;
                     /offset_norm_max; /qdelta: quantiles of (colour - seed colour) / 1e-4
Usage: python tests/golden/make_samplers_golden.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repository and the reference on sys.path)

NP_SEED = 20261020
Q = np.linspace(0.0, 1.0, 1025)
BOX_INDOOR = np.array([-3.5, -2.5, 0.0, 3.5, 2.5, 5.0])             # the sample indoor scene's room
BOX_OUTDOOR = np.array([-1.5, -1.0, -0.25, 1.25, 2.0, 1.0])
ENV_COLOR, FLOOR_COLOR = (135.0, 206.0, 300.0), (120.0, 90.0, 60.0)   # 300: clamped to 1


def quantiles(cols):
    return np.stack([np.quantile(np.asarray(c, np.float64), Q) for c in cols]).astype(np.float32)


def around_origin(p, R, disc=False):
    r = np.linalg.norm(p, axis=1)
    first = (p[:, 0] ** 2 + p[:, 1] ** 2) / R ** 2 if disc else r ** 3 / R ** 3
    return [p[:, 0], p[:, 1], p[:, 2], first, p[:, 2] / r, np.arctan2(p[:, 1], p[:, 0])]


def main():
    MG.install_stubs()
    MG.cuda_to_cpu()
    import gs_renderer as G
    captured = {}

    def capture(self, pcd, require_grad, spatial_lr_scale):
        captured.update(pcd=pcd, require_grad=require_grad, spatial_lr_scale=spatial_lr_scale)
    G.GaussianModel.create_from_pcd = capture
    G.storePly = lambda *a, **kw: None
    np.random.seed(NP_SEED)
    out = {"np_seed": np.int64(NP_SEED)}

    def run(kind, params, exp_path=None):
        captured.clear()
        G.GaussianModel(dict(params, sh_degree=0), kind, exp_path)
        pcd = captured["pcd"]
        return np.asarray(pcd.points, np.float64), np.asarray(pcd.colors, np.float64)

    for method, box in (("indoor", BOX_INDOOR), ("outdoor", BOX_OUTDOOR)):
        for zg in (False, True):
            params = dict(cam_pose_method=method, scene_box=box.copy(), zero_ground=zg, env_init_color=ENV_COLOR,
                          floor_init_color=FLOOR_COLOR)
            R = float(np.sqrt(np.sum(np.maximum(np.abs(box[:3]), np.abs(box[3:])) ** 2)))
            for kind in ("env", "floor"):
                name = f"{kind}_{method}_zg{int(zg)}"
                out[f"{name}/box"], out[f"{name}/R"] = box, np.float64(R)
                try:
                    p, c = run(kind, params)
                except UnboundLocalError:
                    out[f"{name}/raises"] = np.bool_(True)
                    continue
                out[f"{name}/raises"] = np.bool_(False)
                out[f"{name}/rows"] = np.int64(p.shape[0])
                out[f"{name}/require_grad"] = np.bool_(captured["require_grad"])
                out[f"{name}/spatial_lr_scale"] = np.float64(captured["spatial_lr_scale"])
                out[f"{name}/colors"] = np.unique(c, axis=0) if method == "outdoor" or kind == "floor" else \
                    np.stack([np.unique(s, axis=0)[0] for s in np.split(c, 5)])
                if kind == "env" and method == "indoor":
                    s = np.split(p, 5)
                    out[f"{name}/q"] = np.stack([quantiles(x.T) for x in s])
                    out[f"{name}/shared"] = np.bool_(
                        np.array_equal(s[0][:, 1:], s[1][:, 1:]) and np.array_equal(s[2][:, [0, 2]], s[3][:, [0, 2]])
                        and np.array_equal(s[4][:, 0], s[2][:, 0]) and np.array_equal(s[4][:, 1], s[0][:, 1])
                        and np.array_equal(s[0][:, 2], s[2][:, 2]))
                elif method == "indoor":
                    out[f"{name}/q"] = quantiles(p.T)[None]
                else:
                    out[f"{name}/q"] = quantiles(around_origin(p, R, disc=(kind == "floor")))[None]

    with tempfile.TemporaryDirectory() as exp:
        radius, n = 0.5, 100_000
        p, c = run("object", dict(init_guided="default", init_prompt="a ball", num_pts=n, radius=radius), exp)
        out["ball/rows"], out["ball/R"] = np.int64(p.shape[0]), np.float64(radius)
        out["ball/spatial_lr_scale"] = np.float64(captured["spatial_lr_scale"])
        out["ball/require_grad"] = np.bool_(captured["require_grad"])
        out["ball/q"] = quantiles(around_origin(p, radius))[None]
        out["ball/qcolors"] = quantiles(c.T)

        rng = np.random.default_rng(NP_SEED)
        v = rng.normal(size=(4096, 3))
        seeds = v / np.linalg.norm(v, axis=1, keepdims=True) * (0.5 * np.cbrt(rng.random((4096, 1))))
        seed_colors = rng.random((4096, 3))
        G.init_from_pointe = lambda prompt, guided: (seeds.copy(), seed_colors.copy())
        p, c = run("object", dict(init_guided="pointe", init_prompt="a chair", use_pointe_rgb=True), exp)
        assert p.shape == (4096 * 20, 3)
        base = seeds * np.array([1.0, -1.0, 1.0]) + np.array([0.0, 0.0, 0.15])
        off = p.reshape(4096, 20, 3) - base[:, None, :]
        out["pointe/rows"] = np.int64(p.shape[0])
        out["pointe/spatial_lr_scale"] = np.float64(captured["spatial_lr_scale"])
        out["pointe/seeds"], out["pointe/seed_colors"] = seeds[:64], seed_colors[:64]
        out["pointe/points"], out["pointe/point_colors"] = p[:64 * 20], c[:64 * 20]
        out["pointe/offsets_shared"] = np.bool_(np.abs(off - off[:1]).max() < 1e-12)
        out["pointe/offset_norm_max"] = np.float64(np.linalg.norm(off[0], axis=1).max())
        out["pointe/qdelta"] = quantiles(((c.reshape(4096, 20, 3) - seed_colors[:, None, :]) / 1e-4).reshape(-1, 3).T)
        p2, c2 = run("object", dict(init_guided="pointe", init_prompt="a chair", use_pointe_rgb=False), exp)
        out["pointe/qcolors"] = quantiles(c2.T)

    path = os.path.join(HERE, "samplers.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    for k in sorted(out):
        print(k, np.asarray(out[k]).shape)
    assert size <= 1_000_000, size


if __name__ == "__main__":
    main()
