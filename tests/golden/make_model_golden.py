"""Generates tests/golden/model.npz from the reference's OWN GaussianModel (gs_renderer.py:166-1105), run unchanged on the CPU.
Like make_golden.py it runs only where the reference checkout is; nothing of the reference travels: the fixture holds arrays and
lists of names.

  surface/   the public names of the reference's class and every method's parameter names
  create/    create_from_pcd for sh_degree 0, 1, 3: 257 float64 points and colours (0, 0.5 and 1 among them) and a recorded dist2
             -- what the patched gs_renderer.distCUDA2 returns, with entries 0, 5e-8, exactly 1e-7 and large -- and the six leaves
  reset/     reset_opacity on 300 logits (0, +-50, -80, -100, -200, logit(0.01) and its two fp32 neighbours, NaN; no other finite
             value inside -103.3 < x < -87.3, where fp32 sigmoid is subnormal) after three Adam steps with every learning rate 0 (the
             logits stay as drawn, the moments are non-zero): moments before, new logits, moments after, step
  stats/     add_densification_stats_div(filter, -300), (filter, -500, -300), (filter, 0, 400) and add_densification_stats on
             gradients [700,3], two calls in a row each (two gradients, two filters): accum and denom after each call
  lr/        the four schedules of training_setup(OptimizationParams()) -- config.py's defaults, read here -- for
             spatial_lr_scale 1 and 10 at steps 0, 1, 10, 500, 1500, iterations, iterations + 1
  setup/     the optimizer's group names in order and their initial learning rates; the config fields training_setup reads
Usage: python tests/golden/make_model_golden.py
"""
import inspect
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repository and the reference on sys.path)

LEAF = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation"}
CONFIG_FIELDS = ("iterations", "position_lr_init", "position_lr_final", "position_lr_delay_mult", "feature_lr", "feature_lr_final",
                 "opacity_lr", "scaling_lr", "scaling_lr_final", "rotation_lr", "rotation_lr_final", "percent_dense")


def surface(cls):
    names, params = [], []
    for name, member in vars(cls).items():
        if name.startswith("_") and name != "__init__":
            continue
        if isinstance(member, property):
            names.append(name)
            params.append(name + ":<property>")
        elif inspect.isfunction(member):
            names.append(name)
            params.append(name + ":" + ",".join(list(inspect.signature(member).parameters)[1:]))
    return np.array(names), np.array(params)


def scene_model(G, sh_degree, leaves):
    gm = G.GaussianModel({"sh_degree": sh_degree}, "scene")
    for n, a in leaves.items():
        setattr(gm, LEAF[n], torch.nn.Parameter(torch.tensor(a)))
    gm._background = torch.nn.Parameter(torch.zeros(3, 1, 1))
    gm.spatial_lr_scale = 1
    return gm


def main():
    MG.install_stubs()
    MG.cuda_to_cpu()
    import gs_renderer as G
    from config import OptimizationParams
    rng = np.random.default_rng(20261019)
    out = {}

    out["surface/names"], out["surface/params"] = surface(G.GaussianModel)

    # ---- create ----
    P = 257
    points = rng.normal(size=(P, 3))                                   # float64 on purpose
    colors = rng.random(size=(P, 3))
    colors[0], colors[1], colors[2] = (0.0, 0.5, 1.0), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5)
    dist2 = np.exp(rng.uniform(np.log(1e-9), np.log(1e3), size=P)).astype(np.float32)
    dist2[:6] = np.array([0.0, 5e-8, 1e-7, 1e6, 3.0e38, np.nextafter(np.float32(1e-7), np.float32(1))], np.float32)
    assert dist2[2] == np.float32(1e-7)
    out["create/points"], out["create/colors"], out["create/dist2"] = points, colors, dist2
    G.distCUDA2 = lambda pts: torch.tensor(dist2)
    for deg in (0, 1, 3):
        gm = G.GaussianModel({"sh_degree": deg}, "scene")
        gm.create_from_pcd(G.BasicPointCloud(points=points, colors=colors, normals=np.zeros((P, 3))), True, 1)
        for n, attr in LEAF.items():
            out[f"create/{deg}/{n}"] = getattr(gm, attr).detach().numpy().copy()
        assert out[f"create/{deg}/f_rest"].shape == (P, (deg + 1) ** 2 - 1, 3)

    # ---- reset ----
    P = 300
    cap_logit = np.log(np.float32(0.01) / (np.float32(1) - np.float32(0.01)), dtype=np.float32)
    special = np.array([0.0, 50.0, -50.0, -80.0, -100.0, -200.0, cap_logit, np.nextafter(cap_logit, np.float32(0)),
                        np.nextafter(cap_logit, np.float32(-10)), np.nan, 88.0, -20.0, 20.0], np.float32)
    logits = np.concatenate((special, rng.uniform(-12, 12, size=P - special.size).astype(np.float32))).astype(np.float32)
    fin = np.delete(logits, 4)                                         # -100 itself is on the list: both sides give -inf there
    fin = fin[np.isfinite(fin)]
    assert not ((fin > np.float32(-103.3)) & (fin < np.float32(-87.3))).any()
    leaves = dict(xyz=rng.normal(size=(P, 3)).astype(np.float32), f_dc=rng.normal(size=(P, 1, 3)).astype(np.float32),
                  f_rest=np.zeros((P, 3, 3), np.float32), opacity=logits[:, None].copy(),
                  scaling=rng.normal(size=(P, 3)).astype(np.float32), rotation=rng.normal(size=(P, 4)).astype(np.float32))
    gm = scene_model(G, 1, leaves)
    opt = OptimizationParams()
    gm.training_setup(opt)
    for g in gm.optimizer.param_groups:
        g["lr"] = 0.0
    grads = [{n: rng.normal(size=a.shape).astype(np.float32) for n, a in leaves.items()} for _ in range(3)]
    for step in grads:
        for n, attr in LEAF.items():
            getattr(gm, attr).grad = torch.tensor(step[n])
        gm._background.grad = torch.ones(3, 1, 1)
        gm.optimizer.step()
    assert gm._opacity.detach().numpy().tobytes() == logits[:, None].tobytes()          # lr 0: the logits are as drawn
    others = {n: (getattr(gm, attr), gm.optimizer.state[getattr(gm, attr)]) for n, attr in LEAF.items() if n != "opacity"}
    st = gm.optimizer.state[gm._opacity]
    out["reset/logits"] = logits
    out["reset/grads"] = np.stack([s["opacity"] for s in grads])
    out["reset/exp_avg_in"], out["reset/exp_avg_sq_in"] = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
    assert np.abs(out["reset/exp_avg_in"]).min() > 0
    gm.reset_opacity()
    st = gm.optimizer.state[gm._opacity]
    out["reset/new_logits"] = gm._opacity.detach().numpy().reshape(-1).copy()
    out["reset/exp_avg_out"], out["reset/exp_avg_sq_out"] = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
    out["reset/step"] = np.float64(st["step"])
    out["reset/cap"] = np.float32(0.01)
    assert not out["reset/exp_avg_out"].any() and out["reset/step"] == 3
    assert all(getattr(gm, LEAF[n]) is p and gm.optimizer.state[p] is s for n, (p, s) in others.items())
    new = out["reset/new_logits"]
    assert np.isneginf(new[[4, 5]]).all() and np.isnan(new[9]) and np.isfinite(np.delete(new, [4, 5, 9])).all()

    # ---- stats ----
    T = 700
    g2 = [rng.normal(size=(T, 3)).astype(np.float32) * np.float32(1e-3) for _ in range(2)]
    g2[0][:4] = np.array([[0, 0, 5], [3e-10, 4e-10, 1], [0.25, -0.5, 0], [-2.5, 0, 0]], np.float32)
    out["stats/grad0"], out["stats/grad1"] = g2
    for tag, cut in (("tail", (-300,)), ("mid", (-500, -300)), ("head", (0, 400)), ("whole", None)):
        n = len(range(T)[slice(*cut)]) if cut and len(cut) == 2 else (len(range(T)[cut[0]:]) if cut else T)
        gm = scene_model(G, 0, dict(xyz=np.zeros((n, 3), np.float32)))
        gm.xyz_gradient_accum, gm.denom = torch.zeros(n, 1), torch.zeros(n, 1)
        for r in range(2):
            f = rng.random(n) < 0.35
            vsp = types.SimpleNamespace(grad=torch.tensor(g2[r]))
            if cut is None:
                gm.add_densification_stats(vsp, torch.tensor(f))
            else:
                gm.add_densification_stats_div(vsp, torch.tensor(f), *cut)
            out[f"stats/{tag}/filter{r}"] = f
            out[f"stats/{tag}/accum{r}"] = gm.xyz_gradient_accum.numpy().reshape(-1).copy()
            out[f"stats/{tag}/denom{r}"] = gm.denom.numpy().reshape(-1).copy()
        out[f"stats/{tag}/cut"] = np.array(cut if cut else (), np.int64)
        assert out[f"stats/{tag}/denom1"].max() == 2

    # ---- lr, setup ----
    out["setup/config_names"] = np.array(CONFIG_FIELDS)
    out["setup/config_values"] = np.array([float(getattr(opt, k)) for k in CONFIG_FIELDS], np.float64)
    steps = [0, 1, 10, 500, 1500, opt.iterations, opt.iterations + 1]
    out["lr/steps"] = np.array(steps, np.int64)
    for scale in (1, 10):
        gm = scene_model(G, 1, leaves)
        gm.spatial_lr_scale = scale
        gm.training_setup(opt)
        out[f"setup/{scale}/names"] = np.array([g["name"] for g in gm.optimizer.param_groups])
        out[f"setup/{scale}/lrs"] = np.array([g["lr"] for g in gm.optimizer.param_groups], np.float64)
        for name, group in (("update_learning_rate", "xyz"), ("update_feature_learning_rate", "f_dc"),
                            ("update_rotation_learning_rate", "rotation"), ("update_scaling_learning_rate", "scaling")):
            vals = []
            for s in steps:
                v = getattr(gm, name)(s)
                assert v == [g for g in gm.optimizer.param_groups if g["name"] == group][0]["lr"]
                vals.append(float(v))
            out[f"lr/{scale}/{name}"] = np.array(vals, np.float64)

    path = os.path.join(HERE, "model.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= 500_000, size


if __name__ == "__main__":
    main()
