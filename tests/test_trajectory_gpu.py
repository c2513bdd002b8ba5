"""-m gpu: a training trajectory in lockstep across every rasterizer form (tests/trajectory_ref.py has the schedule and the CPU
references): 18 steps on long-lived objects with P changing twice under them -- 6 steps at P0 = 400, densify_and_prune, 6 steps
at P1 > 512, an importance prune, 6 steps at P2 < P0.

`plain` (GaussianRasterizer per view, eager, torch.optim.Adam, the trainer's boolean-mask statistics) sets the pace: it runs
once per module and its record is shared. Every other leg is one object that lives for the whole schedule; before each step its
parameters, Adam state and statistics are overwritten IN PLACE with plain's pre-step state (addresses, captures, arenas and caches
survive: they are the state under test), after the step it is checked. Free-running trajectories are not compared: Adam with eps
1e-15 moves an entry by about +-lr whatever the gradient's size, so an entry whose gradient is rounding noise takes another path
in another summation order without any bug.

Checked: legs 2-6 against plain (outputs bit-equal, gradients at test_graph.py's bar, statistics); every leg's Adam step against
torch.optim.Adam on the CPU from the leg's own state and gradients (test_epilogue.py's bars); every leg's densification and prune
bit-equal to plain's, plain's against tests/densify_ref.py (test_densify.py's bars); after every step the rasterizer's scratch
cache, the arena's zero-outside promise and the replay counters; at four steps plain, fused and raw against a float64 evaluation
of the same step within 4 e_ref + 1e-5, e_ref being the distance of the reference's own fp32 evaluation from float64.
Every test runs under its own time limit."""
import faulthandler

import numpy as np
import pytest
import torch
from torch import nn

from tests import trajectory_ref as T
from tests.test_densify import assert_bit_equal, assert_matches, ours_view, ref_view
from tests.util import err, rel_scale, settings_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TEST_SECONDS = 420
NAMES, V, STEPS = T.NAMES, T.V, T.STEPS
MODEL_ORDER = ("xyz", "scaling", "rotation", "opacity", "f_dc", "f_rest")      # scene.LEAVES


@pytest.fixture(autouse=True)
def _time_limit():
    """A hung kernel does not return to Python: the watchdog thread ends the process with a traceback instead."""
    faulthandler.dump_traceback_later(TEST_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- the schedule on the device ---------------------------------------------------------------------------------------------------
class DevStep:
    def __init__(self, st: T.StepInputs):
        self.sets = [settings_for(c, st.bg[k].numpy(), st.sh_degree[k], DEV) for k, c in enumerate(st.cams)]
        self.fovx = [c.FoVx for c in st.cams]
        self.noise, self.targets = st.noise.to(DEV), st.targets.to(DEV)
        self.eval_set = None if st.eval_cam is None else settings_for(st.eval_cam, [1, 1, 1], T.D, DEV)


# ---- the legs -------------------------------------------------------------------------------------------------------------------
class Leg:
    """One trainer: parameters, optimizer, statistics, contexts, arenas and modules of its own, alive for the whole schedule.
    setup(): what lives for the whole schedule; rebuild(): what INTEGRATION.md section 4c says a caller re-creates for a new P."""
    fused_adam = True
    against_plain = True

    def __init__(self, sched: T.Schedule):
        from dreamscene_amd import densify
        from dreamscene_amd.optim import FusedAdam
        from dreamscene_amd.rasterizer import RasterContext
        self.dev = torch.device(DEV)
        self.p = {n: nn.Parameter(sched.leaves[n].to(self.dev).clone()) for n in NAMES}
        cls = FusedAdam if self.fused_adam else torch.optim.Adam
        self.opt = cls([{"params": [self.p[n]], "lr": T.LRS[n], "name": n} for n in NAMES], lr=0.0, eps=T.ADAM_EPS)
        self.stats = densify.DensifyStats(T.P0, self.dev)
        self.score_rc = RasterContext()
        self.setup()
        self.rebuild()

    @property
    def P(self) -> int:
        return self.p["xyz"].shape[0]

    def setup(self):
        pass

    def rebuild(self):
        pass

    def replays(self) -> int:
        return -1                       # (no captured code in this leg)

    # ---- state: read, and overwritten in place
    def state(self) -> dict:
        st = self.opt.state.get(self.p["xyz"], None)
        moments, step = None, 0.0
        if st is not None and "exp_avg" in st:
            moments = {n: (self.opt.state[self.p[n]]["exp_avg"].clone(), self.opt.state[self.p[n]]["exp_avg_sq"].clone())
                       for n in NAMES}
            step = float(st["step"])
            assert all(float(self.opt.state[self.p[n]]["step"]) == step for n in NAMES)
        return dict(params={n: self.p[n].detach().clone() for n in NAMES}, moments=moments, step=step,
                    stats=tuple(t.clone() for t in self.stats.tensors()))

    def overwrite(self, state: dict) -> None:
        """plain's state into this leg's own tensors, in place: every address survives, every version counter moves (whoever
        writes an input of the rasterizer owes it that: INTEGRATION.md section 5b'')."""
        with torch.no_grad():
            for n in NAMES:
                targets = [(self.p[n], state["params"][n])]
                if state["moments"] is None:
                    assert self.p[n] not in self.opt.state or not self.opt.state[self.p[n]], "a fresh optimizer has no state"
                else:
                    st = self.opt.state[self.p[n]]
                    targets += [(st["exp_avg"], state["moments"][n][0]), (st["exp_avg_sq"], state["moments"][n][1])]
                    st["step"].fill_(state["step"])
                for dst, src in targets:
                    v0, ptr = dst._version, dst.data_ptr()
                    dst.copy_(src)
                    assert dst._version > v0 and dst.data_ptr() == ptr, f"{n}: the in-place copy must bump the version counter"
            for dst, src in zip(self.stats.tensors(), state["stats"]):
                dst.copy_(src)

    # ---- one step
    def inputs(self, ds: DevStep):
        scales, rots, opac, shs = T.activations(self.p)
        return scales, rots, opac, shs, T.noisy_scales(scales, ds.noise[:, :self.P])

    def loss(self, fw: dict, ds: DevStep) -> torch.Tensor:
        """torch glue and torch's loss expression (the reference trainer's)."""
        disps = [T.disp_reference(o[2], f) for o, f in zip(fw["outs"], ds.fovx)]
        return T.step_loss([o[0] for o in fw["outs"]], disps, fw["scales"], ds.targets)

    def after_backward(self, fw: dict, m2d_grad: torch.Tensor) -> None:
        pass                            # (the statistics were updated inside K8)

    def adam(self, grads: dict) -> None:
        self.opt.step()

    def step(self, ds: DevStep) -> dict:
        for p in self.p.values():
            p.grad = None
        fw = self.forward(ds)
        ev = None
        if ds.eval_set is not None:                 # an eval view between the forward and the backward
            with torch.no_grad():
                ev = self.eval_render(ds.eval_set).clone()
        loss = self.loss(fw, ds)
        loss.backward()
        grads, m2d_grad = self.gradients(fw)
        self.after_backward(fw, m2d_grad)
        res = dict(outs=[(o[0].detach().clone(), o[1].clone(), o[2].detach().clone()) for o in fw["outs"]],
                   grads={n: grads[n].detach().clone() for n in NAMES}, m2d=m2d_grad.detach().clone(),
                   loss=loss.detach().clone(), eval=ev)
        self.adam(grads)
        return res

    # ---- P changes
    def assign(self, res) -> None:
        self.p = {n: res[n] for n in NAMES}
        self.rebuild()

    def densify(self, seed: int):
        from dreamscene_amd import densify
        d = T.DENSIFY
        res = densify.densify_and_prune(self.opt, self.stats, d["max_grad"], d["min_opacity"], d["extent"], None,
                                        percent_dense=d["percent_dense"], N=d["N"], seed=seed)
        self.assign(res)
        return res

    def prune(self, score_sets):
        from dreamscene_amd import densify, views
        with torch.no_grad():
            scales, rots, opac, shs = T.activations(self.p)
            scores = views.importance_scores(score_sets, means3D=self.p["xyz"], opacities=opac, shs=shs, scales=scales,
                                             rotations=rots, context=self.score_rc)
            mask = densify.importance_prune_mask(densify.v_importance(scales, scores, T.PRUNE["v_pow"]), T.PRUNE["percent"])
        res = densify.prune_points(self.opt, self.stats, mask)
        self.assign(res)
        return res, mask


class Plain(Leg):
    """1. GaussianRasterizer per view, eager, torch.optim.Adam, the trainer's boolean-mask statistics."""
    fused_adam = False
    accel = "off"

    def setup(self):
        from dreamscene_amd.rasterizer import RasterContext
        self.rc = RasterContext(per_view_accel=self.accel)

    def _render(self, s, m2d, shs, opac, scales, rots):
        from dreamscene_amd.rasterizer import GaussianRasterizer
        return GaussianRasterizer(raster_settings=s, context=self.rc)(
            means3D=self.p["xyz"], means2D=m2d, shs=shs, colors_precomp=None, opacities=opac, scales=scales, rotations=rots,
            cov3D_precomp=None)

    def forward(self, ds):
        scales, rots, opac, shs, sc = self.inputs(ds)
        m2ds = [torch.zeros((self.P, 3), device=self.dev, requires_grad=True) for _ in range(V)]
        outs = [self._render(ds.sets[k], m2ds[k], shs, opac, sc[k], rots) for k in range(V)]
        return dict(outs=outs, scales=list(sc), m2d=m2ds)

    def eval_render(self, s):
        scales, rots, opac, shs = T.activations(self.p)
        return self._render(s, torch.zeros((self.P, 3), device=self.dev), shs, opac, scales, rots)[0]

    def gradients(self, fw):
        return {n: self.p[n].grad for n in NAMES}, torch.stack([m.grad for m in fw["m2d"]])

    def after_backward(self, fw, m2d_grad):
        with torch.no_grad():           # the LAST view's, like the reference's trainers
            T.update_stats_reference(*self.stats.tensors(), fw["outs"][-1][1], m2d_grad[-1])


class Streams(Plain):
    """2. the same with the forwards on internal streams."""
    accel = "streams"


class Ring(Plain):
    """3. the same with the per-view call served by the captured drop-in ring."""
    accel = "graphs"

    def setup(self):
        from dreamscene_amd import dropin
        dropin.reset()
        super().setup()

    def replays(self):
        from dreamscene_amd import dropin
        return sum(r["replays"] for r in dropin.stats().values())


class Views(Leg):
    """4. GaussianRasterizerViews, DensifyStats.collect, FusedAdam."""

    def setup(self):
        from dreamscene_amd.rasterizer import RasterContext
        self.rc = RasterContext()

    def _call(self, sets, m2d, xyz, shs, opac, scales, rots):
        from dreamscene_amd.views import GaussianRasterizerViews
        return GaussianRasterizerViews(sets, context=self.rc)(means3D=xyz, means2D=m2d, shs=shs, opacities=opac, scales=scales,
                                                              rotations=rots)

    def forward(self, ds):
        scales, rots, opac, shs, sc = self.inputs(ds)
        m2d = torch.zeros((V, self.P, 3), device=self.dev, requires_grad=True)
        with self.stats.collect(self.rc):
            outs = self._call(ds.sets, m2d, self.p["xyz"], shs, opac, sc, rots)
        return dict(outs=outs, scales=list(sc), m2d=m2d)

    def eval_render(self, s):
        scales, rots, opac, shs = T.activations(self.p)
        return self._call([s], torch.zeros((1, self.P, 3), device=self.dev), self.p["xyz"], shs, opac, scales, rots)[0][0]

    def gradients(self, fw):
        return {n: self.p[n].grad for n in NAMES}, fw["m2d"].grad


class Arena(Views):
    """5. `views` with a GradArena: K8 sums the views into the arena, one torch.autograd.backward pushes the arena's gradients
    through the activations, FusedAdam takes the arena's xyz region as it is. Nothing but K8 writes the arena, so its zero-outside
    promise is kept from step to step."""

    def rebuild(self):
        from dreamscene_amd.multiview import GradArena
        self.arena = GradArena(self.P, T.K, self.dev)          # P-sized: re-created on every new P
        self.rc.grad_arena = self.arena

    def forward(self, ds):
        scales, rots, opac, shs, sc = self.inputs(ds)
        self.acts = (rots, opac, shs)
        m2d = torch.zeros((V, self.P, 3), device=self.dev, requires_grad=True)
        with self.stats.collect(self.rc):
            outs = self._call(ds.sets, m2d, self.p["xyz"], shs.detach(), opac.detach(), sc, rots.detach())
        return dict(outs=outs, scales=list(sc), m2d=m2d)

    def gradients(self, fw):
        av = self.arena.views
        torch.autograd.backward(list(self.acts), [av["rotations"], av["opacities"], av["shs"]])
        self.acts = None
        g = {n: self.p[n].grad for n in NAMES if n != "xyz"}
        g["xyz"] = av["means3D"]
        return g, fw["m2d"].grad

    def adam(self, grads):
        self.opt.step(grads=[grads[n] for n in NAMES])


class Captured(Arena):
    """6. CapturedViews with an arena, [V,P,3] per-view scales and statistics. The module and its context live through both
    changes of P; the arena, the statistics' tensors and the persistent activation buffers the graphs read are per P."""

    def setup(self):
        from dreamscene_amd.graph import CapturedViews
        super().setup()
        self.rast = CapturedViews(context=self.rc)

    def rebuild(self):
        super().rebuild()
        self.rc.densify_stats = self.stats.tensors()
        z = lambda *s: torch.zeros(s, device=self.dev)
        self.bufs = (z(self.P, 4), z(self.P, 1), z(self.P, T.K, 3))          # rotations, opacities, shs at fixed addresses

    def replays(self):
        return self.rast.stats["replays"]

    def forward(self, ds):
        scales, rots, opac, shs, sc = self.inputs(ds)
        self.acts = (rots, opac, shs)
        with torch.no_grad():
            for b, a in zip(self.bufs, self.acts):
                b.copy_(a)
        m2d = torch.zeros((V, self.P, 3), device=self.dev, requires_grad=True)
        outs = self.rast(ds.sets, means3D=self.p["xyz"], means2D=m2d, opacities=self.bufs[1], shs=self.bufs[2], scales=sc,
                         rotations=self.bufs[0])
        return dict(outs=outs, scales=list(sc), m2d=m2d)

    def eval_render(self, s):
        scales = torch.exp(self.p["scaling"])
        return self.rast([s], means3D=self.p["xyz"], means2D=torch.zeros((1, self.P, 3), device=self.dev),
                         opacities=self.bufs[1], shs=self.bufs[2], scales=scales, rotations=self.bufs[0])[0][0]


class Fused(Views):
    """7. `views` with the fused glue and the fused photometric loss: other arithmetic, checked against float64 only."""
    against_plain = False

    def loss(self, fw, ds):
        from dreamscene_amd import glue, photometric
        outs = fw["outs"]
        disp, _ = glue.disp_from_depth_alpha([o[2] for o in outs], list(ds.fovx))
        images = [o[0] for o in outs]
        guidance = T.LAMBDA_GUIDANCE * photometric.photometric_loss(images, list(ds.targets), l2=1.0).mean()
        loss_scale = torch.mean(torch.stack(fw["scales"], dim=0), dim=-1).mean()
        return guidance + T.LAMBDA_TV * (glue.tv_loss(torch.stack(images)) + glue.tv_loss(disp)) + T.LAMBDA_SCALE * loss_scale


class Raw(Leg):
    """8. scene.rasterize_models_views on the raw leaves (activations and scale noise inside the kernels), the gradients added
    into model_grad_buffers, statistics in K8, FusedAdam on the buffers."""
    against_plain = False

    def setup(self):
        from dreamscene_amd import scene
        self.rc = scene.SceneContext()

    def rebuild(self):
        self.bufs = {n: torch.zeros_like(self.p[n]) for n in NAMES}            # shaped like the leaves: per P
        self.rc.model_grad_buffers = [tuple(self.bufs[n] for n in MODEL_ORDER)]

    def _call(self, sets, m2d, noise):
        from dreamscene_amd import scene
        return scene.rasterize_models_views(sets, [tuple(self.p[n] for n in MODEL_ORDER)], m2d, scale_noise=noise,
                                            context=self.rc)

    def forward(self, ds):
        for b in self.bufs.values():
            b.zero_()
        m2d = torch.zeros((V, self.P, 3), device=self.dev, requires_grad=True)
        with self.stats.collect(self.rc):
            outs = self._call(ds.sets, m2d, ds.noise[:, :self.P].contiguous())
        return dict(outs=[o[:3] for o in outs], scales=[o[3] for o in outs], m2d=m2d)

    def eval_render(self, s):
        return self._call([s], torch.zeros((1, self.P, 3), device=self.dev), None)[0][0]

    def gradients(self, fw):
        return dict(self.bufs), fw["m2d"].grad

    def adam(self, grads):
        self.opt.step(grads=[grads[n] for n in NAMES])


LEGS = dict(plain=Plain, streams=Streams, ring=Ring, views=Views, arena=Arena, captured=Captured, fused=Fused, raw=Raw)
ANCHORED = ("plain", "fused", "raw")


# ---- the checks -------------------------------------------------------------------------------------------------------------------
class Failures(list):
    """What a leg missed, and (printed, never asserted) the largest measured fraction of each bar."""

    def __init__(self):
        super().__init__()
        self.used = {}

    def within(self, key, err, bar, msg):
        self.used[key] = max(self.used.get(key, 0.0), err / bar if bar > 0 else float(err > 0))
        self.check(err <= bar, f"{msg}: {err:.3e} against a bar of {bar:.3e}")

    def check(self, ok, msg):
        if not ok:
            self.append(msg)

    def run(self, fn, what):
        try:
            fn()
        except AssertionError as e:
            self.append(f"{what}: {str(e)[:400]}")


def check_adam(F, what, pre, grads, post):
    """Check 2: torch.optim.Adam on the CPU in fp32 from the leg's own pre-step state and its own gradients; the bars of
    tests/test_epilogue.py."""
    rp, rm = T.adam_reference(pre["params"], pre["moments"], pre["step"], grads)
    F.check(post["step"] == pre["step"] + 1.0, f"{what}: Adam's step counter {pre['step']} -> {post['step']}")
    def allclose(key, got, ref, rtol, atol, msg):        # np.testing.assert_allclose's rule, with the figure kept
        got, ref = got.cpu().numpy().astype(np.float64), ref.numpy().astype(np.float64)
        F.check(bool(np.isfinite(got).all()), f"{msg}: not finite")
        diff = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            F.within(key, float(np.where(diff == 0, 0.0, diff / (atol + rtol * np.abs(ref))).max()), 1.0, msg)
    for n in NAMES:
        allclose("Adam, parameters", post["params"][n], rp[n], 2e-6, 1e-7, f"{what}: Adam, parameter {n}")
        for k, key in enumerate(("exp_avg", "exp_avg_sq")):
            allclose("Adam, moments", post["moments"][n][k], rm[n][k], 2e-6, 2e-6 * float(rm[n][k].abs().max()),
                     f"{what}: Adam, {key} of {n}")


def check_against_plain(F, what, r, post, pr, ppost):
    """Check 1: outputs bit-equal, gradients at the bar of tests/test_graph.py, statistics."""
    for k in range(V):
        for j, name in ((1, "radii"), (0, "image"), (2, "depth_alpha")):
            F.check(torch.equal(r["outs"][k][j], pr["outs"][k][j]), f"{what}: view {k} {name} differs from plain's")
    for n, a, b in [(n, r["grads"][n], pr["grads"][n]) for n in NAMES] + [("means2D", r["m2d"], pr["m2d"])]:
        a, b = a.cpu().numpy(), b.cpu().numpy().reshape(a.shape)              # tests.util.tol_ok(atol=2e-6), with the figure kept
        F.within("gradients against plain's", err(a, b), 2e-6 * rel_scale(b), f"{what}: dL/d{n} against plain's")
    (mr, acc, den), (pmr, pacc, pden) = post["stats"], ppost["stats"]
    F.check(torch.equal(den, pden), f"{what}: denom differs from plain's")
    F.check(torch.equal(mr, pmr), f"{what}: max_radii2D differs from plain's")
    F.run(lambda: np.testing.assert_allclose(acc.cpu().numpy(), pacc.cpu().numpy(), rtol=1e-5, atol=1e-9),
          f"{what}: xyz_gradient_accum against plain's")
    if pr["eval"] is not None:
        F.check(r["eval"] is not None and torch.equal(r["eval"], pr["eval"]), f"{what}: the eval render differs from plain's")


def check_invariants(F, what, leg):
    """Check 4: the scratch cache's all-zero promise, no entry of a stale P, the arena's zero-outside promise."""
    from dreamscene_amd import rasterizer as R
    torch.cuda.synchronize()
    sizes = {}
    for key, s in list(R._SCRATCH.items()):
        sizes.setdefault(key[:3], set()).add(key[3])
        if not s.dirty:
            F.check(not bool(s.partials.any()) and not bool(s.reach.any()), f"{what}: the scratch of {key} is not all zero")
    for key, ps in sizes.items():
        F.check(len(ps) == 1, f"{what}: scratch entries of several P {sorted(ps)} on one (device, stream, views) {key}")
    arena = getattr(leg, "arena", None)
    if arena is not None and arena.zero_outside_ok():
        F.check(arena.verify_zero_outside(), f"{what}: the arena promises zeros outside its bitmap and does not hold them")


def check_surgery(F, what, leg, res, P_new):
    F.check(leg.P == P_new and all(t.shape == (P_new,) for t in leg.stats.tensors()), f"{what}: statistics of the new length")
    F.check(set(leg.opt.state.keys()) == set(res[n] for n in NAMES) and
            all(g["params"][0] is res[g["name"]] for g in leg.opt.param_groups),
            f"{what}: the optimizer's state holds exactly the new parameters")


def surgery_view(res, leg):
    v = ours_view(res, leg.opt, leg.stats)
    return dict(params={n: t.detach().clone() for n, t in v["params"].items()},
                moments={n: tuple(m.clone() for m in ms) for n, ms in v["moments"].items()},
                stats=tuple(t.clone() for t in v["stats"]), segments=res.segments, src=res.src.clone())


def check_surgery_equal(F, what, got, ref):
    """Check 3, every leg: bit-equal to plain's."""
    def go():
        assert got["segments"] == ref["segments"], (got["segments"], ref["segments"])
        assert torch.equal(got["src"], ref["src"]), "src"
        for n in NAMES:
            assert_bit_equal(got["params"][n], ref["params"][n], n)
            for k in range(2):
                assert_bit_equal(got["moments"][n][k], ref["moments"][n][k], f"moment {k} of {n}")
        for k in range(3):
            assert_bit_equal(got["stats"][k], ref["stats"][k], f"statistic {k}")
    F.run(go, f"{what}: against plain's")


def check_anchor(F, what, r, a, lines):
    """Check 5: within 4 e_ref + 1e-5 of float64, per tensor, relative to the tensor's own largest entry."""
    got = dict(r["grads"], loss=r["loss"].reshape(1), means2D=r["m2d"])
    for n in T.ANCHOR_TENSORS:
        e, e_ref = T.rel_err(got[n], a["f64"][n]), a["e_ref"][n]
        lines.append(f"[anchor] {what} {n}: err {e:.3e}  e_ref {e_ref:.3e}  err / e_ref {e / max(e_ref, 1e-300):.2f}")
        F.check(e <= 4.0 * e_ref + 1e-5, f"{what}: {n} is {e:.3e} from float64, the bar is 4 x {e_ref:.3e} + 1e-5")


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def run(name, sched, dsteps, score_sets, rec=None, anchors=None):
    """The whole schedule on one leg. rec: plain's record (None when the leg IS plain: then the record is returned)."""
    F, lines = Failures(), []
    leg = LEGS[name](sched)
    out = dict(steps=[], failures=F, lines=lines)
    compare = rec is not None and leg.against_plain
    replays = leg.replays()
    for i in range(T.N_STEPS):
        what = f"{name} step {i}"
        if i in (STEPS, 2 * STEPS):
            kind = "densify" if i == STEPS else "prune"
            F.check(replays < 0 or leg.replays() > replays, f"{name}: no replay of the captured code before the {kind}")
            replays = leg.replays()
            if rec is not None:
                leg.overwrite(rec[kind]["pre"])
            pre = leg.state()
            if kind == "densify":
                res, mask = leg.densify(sched.densify_seed), None
            else:
                res, mask = leg.prune(score_sets)
            view = surgery_view(res, leg)
            check_surgery(F, f"{name} {kind}", leg, res, res["xyz"].shape[0])
            if rec is not None:
                check_surgery_equal(F, f"{name} {kind}", view, rec[kind]["view"])
            out[kind] = dict(pre=pre, view=view, mask=mask, res=res, ours=ours_view(res, leg.opt, leg.stats))
        if rec is not None:
            leg.overwrite(rec["steps"][i]["pre"])
        pre = leg.state()
        r = leg.step(dsteps[i])
        post = leg.state()
        check_adam(F, what, pre, r["grads"], post)
        check_invariants(F, what, leg)
        if compare:
            check_against_plain(F, what, r, post, rec["steps"][i]["r"], rec["steps"][i]["post"])
        if anchors is not None and i in anchors and name in ANCHORED:
            check_anchor(F, what, r, anchors[i], lines)
        out["steps"].append(dict(pre=pre, r=r, post=post))
    F.check(replays < 0 or leg.replays() > replays, f"{name}: no replay of the captured code in the last phase")
    out["replays"] = leg.replays()
    out["leg"] = leg
    return out


def build_world() -> dict:
    """The schedule on the device, plain's record, and the four shadow steps -- computed once, shared, left unchanged."""
    faulthandler.dump_traceback_later(TEST_SECONDS, exit=True)
    try:
        sched = T.schedule()
        dsteps = [DevStep(st) for st in sched.steps]
        score_sets = [settings_for(c, [1, 1, 1], T.D, DEV, score_flag=True) for c in sched.sphere_cams]
        rec = run("plain", sched, dsteps, score_sets)
        F = rec["failures"]
        # check 3, plain: against tests/densify_ref.py at the bars of tests/test_densify.py
        for kind in ("densify", "prune"):
            d = rec[kind]
            pre = d["pre"]
            if kind == "densify":
                ref = T.densify_reference(pre["params"], pre["moments"], pre["step"], pre["stats"], sched.densify_seed)
                n_copied = sum(d["view"]["segments"][:2])
                F.check(d["view"]["segments"] == ref.segments(T.DENSIFY["N"]),
                        f"plain densify: segments {d['view']['segments']} against the checker's {ref.segments(T.DENSIFY['N'])}")
            else:
                ref = T.prune_reference(pre["params"], pre["moments"], pre["step"], pre["stats"], d["mask"])
                n_copied = int(ref.leaf("xyz").shape[0])
            got = dict(params=d["view"]["params"], moments=d["view"]["moments"], stats=d["view"]["stats"])
            F.check(d["view"]["src"].shape[0] == ref.origin.shape[0] and torch.equal(d["view"]["src"].cpu().long(), ref.origin),
                    f"plain {kind}: the origin of the rows differs from the checker's")
            F.run(lambda: assert_matches(got, ref_view(ref), f"plain {kind} vs checker", n_copied), f"plain {kind}")
        # the conditions, on the trajectory the device actually took
        S, C, K0, K1 = rec["densify"]["view"]["segments"]
        P1, P2 = S + C + K0 + K1, rec["prune"]["view"]["segments"][0]
        F.check(min(S, C, K0) > 0 and S + K0 < T.P0, f"densification without survivors, clones, children or a pruned row: {(S, C, K0, K1)}")
        F.check(P1 > 512 and P2 < T.P0, f"P1 = {P1} must exceed 512 and P2 = {P2} stay below {T.P0}")
        for i, s in enumerate(rec["steps"]):
            vis = float((s["r"]["outs"][-1][1] > 0).float().mean())
            F.check(0.05 <= vis <= 0.95, f"step {i}: {vis:.3f} of the Gaussians are visible in the last view")
        # check 5: the four shadow steps from plain's own pre-step parameters
        anchors = {i: T.anchor({n: t.cpu() for n, t in rec["steps"][i]["pre"]["params"].items()}, sched.steps[i]) for i in T.ANCHORS}
        for i, a in anchors.items():
            F.check(a["radii_agree"], f"anchor {i}: the float64 and fp32 evaluations disagree on radii")
            F.check(all(torch.equal(rec["steps"][i]["r"]["outs"][k][1].cpu(), a["f64"]["radii"][k]) for k in range(V)),
                    f"anchor {i}: plain's radii differ from the float64 evaluation's")
            check_anchor(F, f"plain step {i}", rec["steps"][i]["r"], a, rec["lines"])
        return dict(sched=sched, dsteps=dsteps, score_sets=score_sets, rec=rec, anchors=anchors)
    finally:
        faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def world(built_lib, c_oracle):
    return build_world()


@pytest.mark.parametrize("name", list(LEGS))
def test_leg_in_lockstep(world, name):
    if name == "plain":
        res = world["rec"]
    else:
        res = run(name, world["sched"], world["dsteps"], world["score_sets"], rec=world["rec"], anchors=world["anchors"])
    print("\n".join(res["lines"]))
    print(f"{name}: largest fraction of each bar used: " + ", ".join(f"{k} {v:.3f}" for k, v in res["failures"].used.items()))
    if res["replays"] >= 0:
        print(f"{name}: {res['replays']} replays", getattr(res["leg"], "rast", None) and res["leg"].rast.stats)
    assert not res["failures"], f"{len(res['failures'])} failures:\n" + "\n".join(res["failures"][:40])
