"""The lockstep trajectory harness's schedule and CPU references (tests/test_trajectory.py, tests/test_trajectory_gpu.py).

* `schedule(seed)`: everything random of an 18-step training trajectory with two changes of P, as CPU tensors -- cameras, the
  per-view SH degree and background, the scale noise, the loss targets, the densification seed. No leg draws a number of its own.
* the step's glue and loss in plain torch ops (`activations`, `noisy_scales`, `disp_reference`, `tv_loss`, `step_loss`): the
  reference trainer's expressions as tools/train_step.py restates them; device- and dtype-agnostic, so the GPU legs that share
  "torch glue and torch's loss expression" call these very functions.
* `shadow_step`: one step from scratch on the CPU, in float64 (oracle.torch_oracle with autograd) or in fp32 the way the reference
  would run it (oracle.c_oracle's rasterizer module inside torch's fp32 glue).
* `adam_reference`: torch.optim.Adam on the CPU in fp32 from a given state and given gradients.
* `split_normals`: the densification kernel's counter-based generator (Philox-4x32-10 + Box-Muller, csrc/densify.hip) restated
  with numpy, so that tests/densify_ref.py can follow a `seed=` call entry by entry.
* `cpu_trajectory`: the whole schedule on the CPU in fp32 (C oracle, torch Adam, densify_ref): what the conditions of
  tests/test_trajectory.py are asserted on.
Test infrastructure: nothing under dreamscene_amd/ imports it."""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from dreamscene_amd import synth
from tests import densify_ref as DR

NAMES = DR.NAMES                                   # xyz, f_dc, f_rest, opacity, scaling, rotation: the reference's six groups
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=5e-2, scaling=5e-3, rotation=1e-3)     # gs_renderer.py:615-653
ADAM_EPS = 1e-15
LAMBDA_TV, LAMBDA_SCALE, LAMBDA_GUIDANCE = 1.0, 1.0, 0.1

K, D, V = 16, 3, 3
H, W = 40, 56                                      # 3 x 4 tiles, ragged in both directions
P0 = 400                                           # two 256-Gaussian workgroups; last wave and last 64-bit reach word partial
P_MAX = 2 * P0                                     # N = 2: at most every row split
STEPS = 6                                          # per phase: 2 warm calls, the capture, replays; the ring needs 5
PHASES = ("A", "B", "C")
N_STEPS = STEPS * len(PHASES)
ANCHORS = (0, STEPS, 2 * STEPS, N_STEPS - 1)       # first step, first step after each P change, last step
EVAL_STEP = STEPS + 4                              # phase B, behind the capture and one replay
SEED = 8                                           # (7 and 9 meet the conditions of tests/test_trajectory.py too, less comfortably)
# orbit radii per view: far, middle, and -- the view whose statistics count -- the eye inside the rim of the 0.55-radius cloud, so
# that the near plane culls part of it: a step's last view must see some Gaussians and miss others, and with cameras that look at
# the cloud from outside every Gaussian reaches the screen
CAM_RADII = ((2.6, 3.4), (1.2, 2.0), (0.3, 0.6))
# synth.g_object's scales as they are: with the x4 of the parity tests the close view's footprints fill the screen and the fp32
# evaluation of the step drifts 1e-3 ... 5e-2 from float64 (e_ref), which leaves the anchor nothing to arbitrate with
SCALE_MUL = 1.0

# densify_and_prune(max_grad, min_opacity, extent, max_screen_size=None, percent_dense, N): the median mean gradient after phase A
# is ~1e-6 and the median largest scale ~0.1 = percent_dense x extent, so about half of the rows are selected, cloned and split in
# similar numbers, and P1 ~ 620. The importance prune keeps the upper 40 %: P2 ~ 250.
DENSIFY = dict(max_grad=5e-7, min_opacity=0.05, extent=10.0, percent_dense=0.01, N=2)
PRUNE = dict(n_cams=6, v_pow=0.1, percent=0.6)


class StepInputs(NamedTuple):
    cams: list                      # V dreamscene_amd.camera.Camera
    sh_degree: list                 # V ints
    bg: torch.Tensor                # [V,3]
    noise: torch.Tensor             # [V,P_MAX,3] standard normals; a phase uses the first P rows
    targets: torch.Tensor           # [V,3,H,W]
    eval_cam: Optional[object]      # a camera rendered under no_grad between forward and backward, or None


class Schedule(NamedTuple):
    leaves: Dict[str, torch.Tensor]          # the six raw leaves at P0
    steps: List[StepInputs]
    densify_seed: int
    sphere_cams: list


def schedule(seed: int = SEED) -> Schedule:
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    g = synth.g_object(P0, seed=3, K=K)
    g["scales"] = (g["scales"] * SCALE_MUL).astype(np.float32)
    op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32))
    leaves = dict(xyz=t(g["means3D"]), f_dc=t(g["shs"][:, :1]), f_rest=t(g["shs"][:, 1:]),
                  opacity=t(np.log(op / (1 - op)).reshape(P0, 1)), scaling=t(np.log(g["scales"])), rotation=t(g["rotations"]))
    steps = []
    for i in range(N_STEPS):
        cams = [synth.orbit_camera(float(rng.uniform(*CAM_RADII[j])), float(rng.uniform(60.0, 90.0)), float(rng.uniform(0.0, 360.0)),
                                   float(rng.uniform(0.32, 0.60)), H, W) for j in range(V)]
        sh = [0 if rng.random() < 0.1 else D for _ in range(V)]
        if i % STEPS == 1:
            sh[1] = 0                               # every phase has a view of degree 0
        bg = torch.ones((V, 3))
        for j in range(V):                          # white, black and random, moving through the views
            kind = (i + j) % 3
            if kind == 1:
                bg[j] = 0.0
            elif kind == 2:
                bg[j] = t(rng.random(3))
        noise = torch.randn((V, P_MAX, 3), generator=gen)
        targets = torch.rand((V, 3, H, W), generator=gen)
        eval_cam = synth.orbit_camera(3.0, 70.0, 123.0, 0.5, H, W) if i == EVAL_STEP else None
        steps.append(StepInputs(cams, sh, bg, noise, targets, eval_cam))
    return Schedule(leaves, steps, int(rng.integers(1, 2 ** 62)), synth.sphere_cameras(PRUNE["n_cams"], H, W, radius=3.0))


# ---- the step's glue and loss, as the reference trainer writes them ------------------------------------------------------------
def activations(lv):
    """-> (scales, rotations, opacities, shs) of the raw leaves (gs_renderer.py:168-182)."""
    return (torch.exp(lv["scaling"]), torch.nn.functional.normalize(lv["rotation"]), torch.sigmoid(lv["opacity"]),
            torch.cat((lv["f_dc"], lv["f_rest"]), dim=1))


def noisy_scales(scales, noise):
    """scene_gaussian.py:1005-1008 for V views at once: scales [P,3], noise [V,P,3] -> [V,P,3]."""
    return torch.clamp(scales[None] + noise * ((0.2 ** 0.5) * scales[None] / 4), 0.0)


def disp_reference(depth_alpha, fovx: float):
    """scene_gaussian.py:1023-1032, the boolean-mask minimum with its try / except."""
    depth, alpha = torch.chunk(depth_alpha, 2)
    focal = 1 / (2 * math.tan(fovx / 2))
    disp = focal / (depth + (alpha * 10) + 1e-5)
    try:
        min_d = disp[alpha <= 0.1].min()
    except Exception:
        min_d = disp.min()
    return torch.clamp((disp - min_d) / (disp.max() - min_d), 0.0, 1.0)


def tv_loss(x):
    """utils/system_utils.py:39-47 (x: [B,C,H,W])."""
    b, h, w = x.size(0), x.size(2), x.size(3)
    count_h = x[:, :, 1:, :].numel() // b
    count_w = x[:, :, :, 1:].numel() // b
    h_tv = torch.pow(x[:, :, 1:, :] - x[:, :, : h - 1, :], 2).sum()
    w_tv = torch.pow(x[:, :, :, 1:] - x[:, :, :, : w - 1], 2).sum()
    return 2 * (h_tv / count_h + w_tv / count_w) / b


def step_loss(images, disps, scales, targets):
    """object_trainer.py:372-380 with the guidance loss stood in for by 0.1 x L2 against the targets (tools/train_step.py)."""
    images, disps = torch.stack(list(images), dim=0), torch.stack(list(disps), dim=0)
    guidance = LAMBDA_GUIDANCE * ((images - targets) ** 2).mean()
    loss_scale = torch.mean(torch.stack(list(scales), dim=0), dim=-1).mean()
    return guidance + LAMBDA_TV * (tv_loss(images) + tv_loss(disps)) + LAMBDA_SCALE * loss_scale


def update_stats_reference(max_radii2D, accum, denom, radii, m2d_grad):
    """object_trainer.py:386-390 on [P] statistics: the trainer's boolean-mask updates from the LAST view."""
    vis = radii > 0
    max_radii2D[vis] = torch.max(max_radii2D[vis], radii[vis].float())
    accum[vis] += torch.norm(m2d_grad[vis, :2], dim=-1)
    denom[vis] += 1


# ---- one step from scratch on the CPU -----------------------------------------------------------------------------------------
def _settings(cls, cam, bg, sh_degree, dtype):
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dtype)
    return cls(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
               bg=bg.to(dtype), scale_modifier=1.0, viewmatrix=t(cam.world_view_transform), projmatrix=t(cam.full_proj_transform),
               sh_degree=int(sh_degree), campos=t(cam.camera_center), prefiltered=False, score_flag=False)


def shadow_forward(leaves, st: StepInputs, mode: str):
    """-> (loss, leaves with requires_grad, m2d [V,P,3], per-view (image, radii, depth_alpha)); mode "f64" or "f32"."""
    from oracle import c_oracle as CO, torch_oracle as TO
    dt = torch.float64 if mode == "f64" else torch.float32
    lv = {n: leaves[n].detach().cpu().to(dt).requires_grad_(True) for n in NAMES}
    P = lv["xyz"].shape[0]
    scales, rots, opac, shs = activations(lv)
    sc = noisy_scales(scales, st.noise[:, :P].to(dt))
    m2d = torch.zeros((V, P, 3), dtype=dt, requires_grad=True)
    module = CO.make_rasterizer_module() if mode == "f32" else None
    outs = []
    for k in range(V):
        s = _settings(TO.Settings, st.cams[k], st.bg[k], st.sh_degree[k], dt)
        if mode == "f64":
            outs.append(TO.rasterize(lv["xyz"], m2d[k], opac, shs=shs, scales=sc[k], rotations=rots, settings=s))
        else:
            outs.append(module(s)(means3D=lv["xyz"], means2D=m2d[k], opacities=opac, shs=shs, scales=sc[k], rotations=rots))
    disps = [disp_reference(o[2], c.FoVx) for o, c in zip(outs, st.cams)]
    loss = step_loss([o[0] for o in outs], disps, list(sc), st.targets.to(dt))
    return loss, lv, m2d, outs


def shadow_step(leaves, st: StepInputs, mode: str) -> dict:
    """loss, the gradients of the six raw leaves and of means2D, and every view's radii."""
    loss, lv, m2d, outs = shadow_forward(leaves, st, mode)
    grads = torch.autograd.grad(loss, [lv[n] for n in NAMES] + [m2d])
    out = dict(loss=loss.detach().reshape(1), radii=torch.stack([o[1] for o in outs]), means2D=grads[-1],
               images=torch.stack([o[0].detach() for o in outs]))
    out.update({n: g for n, g in zip(NAMES, grads)})
    return out


ANCHOR_TENSORS = ("loss",) + NAMES + ("means2D",)


def rel_err(a, ref64) -> float:
    """max|a - ref64| relative to ref64's own largest entry."""
    ref64 = ref64.detach().cpu().double()
    scale = float(ref64.abs().max())
    return float((a.detach().cpu().double().reshape(ref64.shape) - ref64).abs().max()) / (scale if scale > 0 else 1.0)


def anchor(leaves, st: StepInputs) -> dict:
    """The float64 evaluation, the fp32 one, and e_ref per tensor (the fp32 evaluation's distance from float64)."""
    r64, r32 = shadow_step(leaves, st, "f64"), shadow_step(leaves, st, "f32")
    return dict(f64=r64, f32=r32, e_ref={n: rel_err(r32[n], r64[n]) for n in ANCHOR_TENSORS},
                radii_agree=bool(torch.equal(r64["radii"], r32["radii"])))


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
def cpu_optimizer(params: dict, moments: Optional[dict] = None, step: float = 0.0):
    """torch.optim.Adam on the CPU in fp32 over the reference's six named groups, with the given state injected."""
    ps = {n: torch.nn.Parameter(params[n].detach().cpu().float().clone()) for n in NAMES}
    opt = torch.optim.Adam([{"params": [ps[n]], "lr": LRS[n], "name": n} for n in NAMES], lr=0.0, eps=ADAM_EPS)
    if moments:
        for n in NAMES:
            opt.state[ps[n]] = {"step": torch.tensor(float(step)), "exp_avg": moments[n][0].detach().cpu().float().clone(),
                                "exp_avg_sq": moments[n][1].detach().cpu().float().clone()}
    return opt, ps


def adam_reference(params: dict, moments: Optional[dict], step: float, grads: dict):
    """-> (params, moments) after one step of torch's own Adam from that state with those gradients."""
    opt, ps = cpu_optimizer(params, moments, step)
    for n in NAMES:
        ps[n].grad = grads[n].detach().cpu().float().reshape(ps[n].shape).clone()
    opt.step()
    return ({n: ps[n].detach() for n in NAMES},
            {n: (opt.state[ps[n]]["exp_avg"], opt.state[ps[n]]["exp_avg_sq"]) for n in NAMES})


# ---- the densification kernel's generator ---------------------------------------------------------------------------------------
def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return c0, c1, c2, c3


def split_normals(seed: int, P: int, N: int) -> torch.Tensor:
    """[N,P,3] fp32: the three standard normals of (seed, row, copy), Philox-4x32-10 + Box-Muller in fp32 as csrc/densify.hip
    forms them (libm's logf / cosf / sinf are within a few ulp of the device's: the children's xyz bar of 1e-5 covers that)."""
    seed &= 0xFFFFFFFFFFFFFFFF
    f = np.float32
    out = np.empty((N, P, 3), np.float32)
    rows = np.arange(P, dtype=np.uint64)
    zero = np.zeros(P, dtype=np.uint64)
    for c in range(N):
        r = _philox4x32_10(rows, zero + np.uint64(c), zero, zero, seed & 0xFFFFFFFF, seed >> 32)
        u = [((x >> np.uint64(8)).astype(np.float32) + f(0.5)) * f(1.0 / 16777216.0) for x in r]
        ra, ta = np.sqrt(f(-2.0) * np.log(u[0])), f(6.283185307179586) * u[1]
        rb, tb = np.sqrt(f(-2.0) * np.log(u[2])), f(6.283185307179586) * u[3]
        out[c, :, 0], out[c, :, 1], out[c, :, 2] = ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb)
    return torch.tensor(out)


def densify_reference(params, moments, step, stats, seed):
    """tests/densify_ref.py's densify_and_prune from the given state (stats: max_radii2D, xyz_gradient_accum, denom), with the
    noise the kernel's generator gives for `seed`. -> the RefGaussians."""
    opt, _ = cpu_optimizer(params, moments, step)
    c = lambda x: x.detach().cpu().float().clone()
    ref = DR.RefGaussians(opt, c(stats[1]), c(stats[2]), c(stats[0]), percent_dense=DENSIFY["percent_dense"])
    P = params["xyz"].shape[0]
    ref.densify_and_prune(DENSIFY["max_grad"], DENSIFY["min_opacity"], DENSIFY["extent"], None, N=DENSIFY["N"],
                          noise=split_normals(seed, P, DENSIFY["N"]))
    return ref


def prune_reference(params, moments, step, stats, mask):
    opt, _ = cpu_optimizer(params, moments, step)
    c = lambda x: x.detach().cpu().float().clone()
    ref = DR.RefGaussians(opt, c(stats[1]), c(stats[2]), c(stats[0]))
    ref.prune_points(mask.detach().cpu())
    return ref


# ---- the whole schedule on the CPU in fp32 --------------------------------------------------------------------------------------
def importance_reference(leaves, cams) -> torch.Tensor:
    """The sum over `cams` of the C oracle's importance score (weight 0: opacity per contributing pixel)."""
    from oracle import c_oracle as CO
    scales, rots, opac, shs = (x.detach().numpy() for x in activations(leaves))
    P = leaves["xyz"].shape[0]
    total = np.zeros(P, np.float64)
    for cam in cams:
        v = CO.make_view(P, K, D, H, W, cam.tanfovx, cam.tanfovy, [1, 1, 1], cam.world_view_transform, cam.full_proj_transform,
                         cam.camera_center)
        f = CO.forward(v, leaves["xyz"].detach().numpy(), opac, shs=shs, scales=scales, rotations=rots, score=True)
        total += f["important_score"]
    return torch.tensor(total.astype(np.float32))


def importance_mask(leaves, scores) -> torch.Tensor:
    from dreamscene_amd import densify
    v = densify.v_importance(torch.exp(leaves["scaling"]), scores, PRUNE["v_pow"])
    return densify.importance_prune_mask(v, PRUNE["percent"])


def cpu_trajectory(sched: Schedule) -> dict:
    """Every step in fp32 the way the reference would run it. -> pre-step leaves of every step, per-step radii of the last view,
    the densification's RefGaussians, and the sizes P0, P1, P2."""
    opt, ps = cpu_optimizer(sched.leaves)
    stats = [torch.zeros(P0) for _ in range(3)]                  # max_radii2D, xyz_gradient_accum, denom
    rec = dict(pre=[], last_radii=[], sizes=[P0])

    def state():
        moments = {n: (opt.state[ps[n]]["exp_avg"], opt.state[ps[n]]["exp_avg_sq"]) for n in NAMES} if opt.state else None
        step = float(opt.state[ps["xyz"]]["step"]) if opt.state else 0.0
        return {n: ps[n].detach() for n in NAMES}, moments, step

    for i, st in enumerate(sched.steps):
        if i == STEPS:
            params, moments, step = state()
            ref = densify_reference(params, moments, step, stats, sched.densify_seed)
            rec["densify"] = ref
        elif i == 2 * STEPS:
            params, moments, step = state()
            mask = importance_mask(params, importance_reference(params, sched.sphere_cams))
            ref = prune_reference(params, moments, step, stats, mask)
            rec["pruned"] = int(mask.sum())
        if i in (STEPS, 2 * STEPS):
            opt, ps = ref.optimizer, ref.leaves()
            for g in opt.param_groups:
                g["lr"] = LRS[g["name"]]
            stats = [ref.max_radii2D, ref.xyz_gradient_accum, ref.denom]
            rec["sizes"].append(ps["xyz"].shape[0])
        rec["pre"].append({n: ps[n].detach().clone() for n in NAMES})
        r = shadow_step({n: ps[n] for n in NAMES}, st, "f32")
        update_stats_reference(*stats, r["radii"][-1], r["means2D"][-1])
        rec["last_radii"].append(r["radii"][-1])
        for n in NAMES:
            ps[n].grad = r[n]
        opt.step()
    return rec
