"""Generates tests/golden/densify.npz from the reference's OWN GaussianModel.densify_and_prune / prune / prune_gaussians
(gs_renderer.py:854-1087), run unchanged on the CPU. Like make_golden.py it runs only where the reference checkout is;
nothing of the reference travels: the fixture is plain input / output arrays.

One model (P0 = 600, K = 16) with a torch.optim.Adam that has taken three steps, four runs from fresh copies of it:
  dp_none/   densify_and_prune(max_grad, min_opacity, extent, None)
  dp_20/     densify_and_prune(max_grad, min_opacity, extent, 20)
  prune/     prune(min_opacity, extent, 20)                       (the live max_radii2D decides)
  imp/       prune_gaussians(percent, important_score)            (the mask it hands to prune_points is stored too)
`torch.normal` is patched to draw its standard normals itself and record them: noise [N, P0, 3], indexed [copy, original row].
Stored per run: the six parameters, their twelve moments, the three statistics, the segment sizes (from the masks the run hands
to prune_points) and the origin of every output row (found through the f_rest rows, which are unique).

So that the file stays below 1 MB: the SH coefficients and the gradients of the three Adam steps are drawn on a coarse dyadic
grid and Adam runs with betas (0.5, 0.75) and lr 0, which keeps the big arrays' mantissas short (they compress); xyz, scaling,
rotation and opacity -- everything arithmetic is done on -- are full-precision draws.
Condition on the inputs, asserted here and again by the test: no row has max exp(scaling), that over 0.8 N, or sigmoid(opacity)
within a relative 1e-4 of a threshold it is compared with (such rows are redrawn).
Usage: python tests/golden/make_densify_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repository and the reference on sys.path)

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LEAF = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation"}
P0, K, N = 600, 16, 2
MAX_GRAD, MIN_OPACITY, EXTENT, PERCENT_DENSE, SCREEN = 0.0002, 0.05, 2.0, 0.01, 20
MARGIN = 1e-4


def near(v, thr):
    return np.abs(v - thr) <= MARGIN * abs(thr)


def margin_violations(scaling, opacity):
    """Rows whose decisions could depend on the last bits of exp / log / sigmoid."""
    smax = np.exp(scaling.astype(np.float64)).max(axis=1)
    sig = 1.0 / (1.0 + np.exp(-opacity.astype(np.float64).reshape(-1)))
    bad = near(smax, PERCENT_DENSE * EXTENT) | near(smax, 0.1 * EXTENT) | near(smax / (0.8 * N), 0.1 * EXTENT) | \
        near(sig, MIN_OPACITY)
    return bad


def draw_inputs(rng):
    d = {}
    d["xyz"] = rng.normal(size=(P0, 3)).astype(np.float32)
    d["rotation"] = (rng.normal(size=(P0, 4)) * 1.3).astype(np.float32)             # un-normalised on purpose
    d["f_dc"] = (np.round(rng.normal(size=(P0, 1, 3)) * 64) / 64 + 0.0).astype(np.float32)          # + 0.0: no -0.0, which
    d["f_rest"] = (np.round(rng.normal(size=(P0, K - 1, 3)) * 64) / 64 + 0.0).astype(np.float32)    # an lr = 0 step turns to 0.0
    scaling = np.empty((P0, 3), np.float32)
    opacity = np.empty((P0, 1), np.float32)
    todo = np.ones(P0, bool)
    while todo.any():
        n = int(todo.sum())
        # max exp(scaling): half below the clone / split threshold 0.02, a tenth above the world-size threshold 0.2
        top = np.exp(rng.uniform(np.log(0.004), np.log(0.3), size=n))
        scaling[todo] = np.log(top[:, None] * rng.uniform(0.3, 1.0, size=(n, 3))).astype(np.float32)
        low = rng.random(n) < 0.3
        o = np.where(low, rng.uniform(0.002, 0.045, size=n), rng.uniform(0.06, 0.98, size=n))
        opacity[todo, 0] = np.log(o / (1 - o)).astype(np.float32)
        todo = margin_violations(scaling, opacity)
    d["scaling"], d["opacity"] = scaling, opacity
    denom = rng.integers(0, 6, size=P0).astype(np.float32)
    g = np.where(rng.random(P0) < 0.45, rng.uniform(0.00025, 0.002, size=P0), rng.uniform(0.0, 0.00015, size=P0))
    accum = (g * denom).astype(np.float32)
    zero = denom == 0
    accum[zero] = np.where(rng.random(int(zero.sum())) < 0.5, 0.0, 0.001).astype(np.float32)   # 0/0 = NaN -> 0; x/0 = inf
    d["xyz_gradient_accum"], d["denom"] = accum, denom
    d["max_radii2D"] = np.floor(rng.uniform(0, 30, size=P0)).astype(np.float32)
    return d


def build_model(G, inputs, grads):
    gm = G.GaussianModel({"sh_degree": 3}, "scene")
    for n in NAMES:
        setattr(gm, LEAF[n], torch.nn.Parameter(torch.tensor(inputs[n])))
    gm._background = torch.nn.Parameter(torch.tensor([0.25, 0.5, 0.75]))
    gm.percent_dense = PERCENT_DENSE
    groups = [{"params": [getattr(gm, LEAF[n])], "lr": 0.0, "name": n} for n in NAMES]
    groups.append({"params": [gm._background], "lr": 0.0, "name": "background"})
    gm.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15, betas=(0.5, 0.75))
    for step in grads:
        for n in NAMES:
            getattr(gm, LEAF[n]).grad = torch.tensor(step[n])
        gm._background.grad = torch.tensor([0.5, -0.25, 0.125])
        gm.optimizer.step()
    gm.xyz_gradient_accum = torch.tensor(inputs["xyz_gradient_accum"])[:, None]     # the reference's [P,1]
    gm.denom = torch.tensor(inputs["denom"])[:, None]
    gm.max_radii2D = torch.tensor(inputs["max_radii2D"])
    return gm


def state_arrays(gm, prefix):
    out = {}
    for n in NAMES:
        p = getattr(gm, LEAF[n])
        st = gm.optimizer.state[p]
        out[f"{prefix}{n}"] = p.detach().numpy().copy()
        out[f"{prefix}{n}/exp_avg"] = st["exp_avg"].numpy().copy()
        out[f"{prefix}{n}/exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
    out[f"{prefix}xyz_gradient_accum"] = gm.xyz_gradient_accum.reshape(-1).numpy().copy()
    out[f"{prefix}denom"] = gm.denom.reshape(-1).numpy().copy()
    out[f"{prefix}max_radii2D"] = gm.max_radii2D.reshape(-1).numpy().copy()
    return out


def main():
    MG.install_stubs()
    MG.cuda_to_cpu()
    import gs_renderer as G
    rng = np.random.default_rng(20261016)
    inputs = draw_inputs(rng)
    assert not margin_violations(inputs["scaling"], inputs["opacity"]).any()
    grads = [{n: (np.round(rng.normal(size=inputs[n].shape) * 8) / 8).astype(np.float32) for n in NAMES} for _ in range(3)]
    row_of = {inputs["f_rest"][i].tobytes(): i for i in range(P0)}
    assert len(row_of) == P0

    rec = {}
    real_normal = torch.normal

    def recording_normal(mean, std):
        z = torch.randn(std.shape)
        rec["z"] = z.clone()
        return z * std + mean

    out = {"P0": np.int64(P0), "K": np.int64(K), "N": np.int64(N), "max_grad": np.float64(MAX_GRAD),
           "min_opacity": np.float64(MIN_OPACITY), "extent": np.float64(EXTENT), "percent_dense": np.float64(PERCENT_DENSE),
           "max_screen_size": np.int64(SCREEN), "margin": np.float64(MARGIN)}
    first = build_model(G, inputs, grads)
    out.update(state_arrays(first, "in/"))
    out["in/step"] = np.float64(first.optimizer.state[first._xyz]["step"])

    def run(tag, call):
        gm = build_model(G, inputs, grads)
        masks = []
        orig_pp = gm.prune_points
        gm.prune_points = lambda mask: (masks.append(mask.clone()), orig_pp(mask))[1]
        torch.manual_seed(1234)
        torch.normal = recording_normal
        try:
            call(gm)
        finally:
            torch.normal = real_normal
        out.update(state_arrays(gm, tag + "/"))
        f_rest = getattr(gm, LEAF["f_rest"]).detach().numpy()
        out[tag + "/src"] = np.array([row_of[f_rest[j].tobytes()] for j in range(f_rest.shape[0])], np.int32)
        assert gm.optimizer.state[gm._background]["step"] == 3 and len(gm.optimizer.state) == 7
        return gm, masks

    for tag, screen in (("dp_none", None), ("dp_20", SCREEN)):
        gm, masks = run(tag, lambda m: m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, screen))
        parents, final = masks                       # the split's parents, then the final prune
        n_split = int(parents.sum())
        n_clone = parents.shape[0] - P0 - N * n_split
        keep = ~final.numpy()
        a, b = P0 - n_split, P0 - n_split + n_clone
        seg = [int(keep[:a].sum()), int(keep[a:b].sum())] + [int(keep[b + c * n_split:b + (c + 1) * n_split].sum()) for c in range(N)]
        assert sum(seg) == gm._xyz.shape[0]
        out[tag + "/segments"] = np.array(seg, np.int64)
        out[tag + "/n_split"], out[tag + "/n_clone"] = np.int64(n_split), np.int64(n_clone)
        noise = torch.randn(N, P0, 3)                # rows that are not split: any values, they must not be used
        noise[:, parents[:P0]] = rec["z"].reshape(N, n_split, 3)
        out[tag + "/noise"] = noise.numpy()
        shares = dict(keep=seg[0] - seg[1], clone=seg[1], split=n_split, pruned_original=a - seg[0], pruned_child=n_split - seg[2])
        print(tag, "P_out", sum(seg), "segments", seg, {k: round(v / P0, 3) for k, v in shares.items()})
        if screen is None:
            # every class of the issue's list holds >= 5 % of the rows (clone counted among its surviving sources)
            assert all(v >= 0.05 * P0 for v in shares.values()), shares
    gm, masks = run("prune", lambda m: m.prune(MIN_OPACITY, EXTENT, SCREEN))
    out["prune/segments"] = np.array([gm._xyz.shape[0]], np.int64)
    print("prune P_out", gm._xyz.shape[0])
    score = torch.tensor(rng.gamma(2.0, 30.0, size=(P0, 1)).astype(np.float32))
    gm, masks = run("imp", lambda m: m.prune_gaussians(0.4, score))
    out["imp/segments"] = np.array([gm._xyz.shape[0]], np.int64)
    out["imp/mask"] = masks[0].numpy()
    out["imp/score"], out["imp/percent"] = score.numpy(), np.float64(0.4)
    print("imp P_out", gm._xyz.shape[0])

    path = os.path.join(HERE, "densify.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= 1_000_000, size


if __name__ == "__main__":
    main()
