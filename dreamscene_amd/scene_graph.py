"""The raw-leaf (scene) views step -- `scene.rasterize_models_views` -- with its launches replayed from captured graphs:
same kernels, same results, a fraction of the host work. The scene path's counterpart of `graph.CapturedViews`.

    rast = CapturedModelsViews(context=SceneContext(model_grad_buffers=bufs, densify_stats=stats.tensors()))
    outs = rast(settings_list, models, means2D, noise=NoiseSpec(seed, step * V))     # [(image, radii, depth_alpha, scales)]

Protocol (graph.py has the reasons): WARM_CALLS eager steps learn the pair counts; then graph F covers the projection and the
render of all views, the host polls the pinned pair counts against the captured capacity, a view over capacity makes that
step run exactly (eagerly) and the next one capture again with more room; graph C covers the backward, captured at the first
backward after one eager run that allocates the static result tensors.

What a capture reads IN PLACE, and is therefore keyed on by address (`capture_key`): the raw leaves of every model (persistent
nn.Parameters the optimizer updates in place -- a densified model is a new tensor and a new capture, after WARM_CALLS eager
steps of its own), the `model_grad_buffers`, the `densify_stats` tensors, a NoiseSpec stream tensor of the caller's.
What is REWRITTEN per step in device memory the graphs point to: the cameras with tanfov and the active SH degree (the packed
block) and the noise stream ids of integer-stream NoiseSpecs (int32[V] words of the module's), both by one launch
(`gsr_pack_views_streams`) at the forward -- K8 reads the words again; `scale_noise` / `sh_noise` tensors, the upstream
gradients and the gradients arriving through the returned scales are copied into static buffers -- except that up to
graph.MAX_DIRECT_GRAPHS backward graphs are captured over the caller's own gradient tensors, contiguous fp32 ones, so that
nothing is copied when a loss produces them at the same addresses step after step (83 MB per 4-view step at 1024^2, and
12 B per Gaussian and view for the scales).
The outputs are static tensors: the next step's replay overwrites them (consume them within the step). Without
model_grad_buffers autograd receives the capture's static gradient tensors, which the module keeps referenced so that
AccumulateGrad COPIES them: a leaf's .grad never aliases them.
Not capturable, run eagerly and counted in stats["eager_steps"]: grids beyond 256 tiles a side, P == 0, K outside
{1, 4, 9, 16}, leaves that are not contiguous 16-byte aligned fp32 (the eager path reads a copy of those), a profile."""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Optional, Sequence

import torch

from . import _lib as L
from . import graph as G
from . import rasterizer as R
from . import scene as S
from . import views as VW
from .graph import WARM_CALLS, user_view

CAPTURABLE_K = (1, 4, 9, 16)


def capture_key(settings_list, models, scale_noise, sh_noise, specs, rc) -> tuple:
    """What a capture is valid for -- everything baked into the captured structs. Pure: reads shapes, addresses and settings,
    touches no device. models: 6-tuples of leaves; specs: scene._view_specs' result (None or one NoiseSpec / None per view).
    NOT in the key (they live in device memory rewritten per step): cameras, bg, tanfov, SH degree, integer stream ids."""
    s0 = settings_list[0]
    ptr_shape = lambda t: None if t is None else (t.data_ptr(), tuple(t.shape))
    ptrs = lambda ts: None if ts is None else tuple(None if t is None else t.data_ptr() for t in ts)

    def spec_key(sp):
        if sp is None:
            return None
        return (int(sp.seed), bool(sp.scales), bool(sp.shs),
                sp.stream.data_ptr() if isinstance(sp.stream, torch.Tensor) else None)
    bufs = getattr(rc, "model_grad_buffers", None)
    sv = rc.stats_views
    return (len(settings_list), int(s0.image_height), int(s0.image_width), float(s0.scale_modifier),
            tuple(tuple(ptr_shape(t) for t in m) for m in models),
            tuple(bool(s.prefiltered) for s in settings_list),
            (None if scale_noise is None else tuple(scale_noise.shape), None if sh_noise is None else tuple(sh_noise.shape),
             None if specs is None else tuple(spec_key(sp) for sp in specs)),
            (None if bufs is None else tuple(ptrs(row) for row in bufs), ptrs(rc.densify_stats),
             tuple(sv) if isinstance(sv, (list, tuple)) else sv, rc.fwd_variant, int(rc.score_mode), rc.seg_len))


def _scene_PK(models) -> tuple:
    """(P, K) of a model table, as the forward derives them: K from the models that have rows."""
    P, K = 0, None
    for m in models:
        n = int(m[0].shape[0])
        if n > 0 and K is None:
            K = 1 + (int(m[5].shape[1]) if m[5] is not None and m[5].numel() > 0 else 0)
        P += n
    return P, K or 1


def _in_place_readable(models, dev) -> bool:
    """Does the forward read these leaves where they are (rasterizer._prep makes no copy of them)?"""
    return all(t is None or (t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0)
               for m in models for t in m)


class _ModelsCapture(G.Captured):
    """+ the scene module's own: noise buffers, stream-id words, gradients through the returned scales, backward graphs."""
    __slots__ = ("sn", "hn", "words", "g_scales", "gC", "bwd", "bwd_m2d")


class _CapturedModelsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, settings_list, rc, scale_noise, sh_noise, specs, differentiable, means2D, *leaves):
        models = [tuple(leaves[6 * m:6 * m + 6]) for m in range(len(leaves) // 6)]
        return G.fn_forward(ctx, owner, rc, differentiable, settings_list, models, scale_noise, sh_noise, specs)

    @staticmethod
    def backward(ctx, *grads):
        G.refuse_stale_backward(ctx)
        o = ctx.owner._backward(ctx.cap_state, ctx.eager_states, grads, ctx.rc)
        if ctx.pending is not None:
            ctx.pending.done = True
        flat = []
        for row in o["model_grads"]:
            flat.extend([None] * 6 if ctx.rc.model_grad_buffers is not None else row)
        return (None, None, None, None, None, None, None, o["dL_dmeans2D"], *flat)


class CapturedModelsViews(G.CapturedModule):
    """`scene.rasterize_models_views` as a module whose steps replay from captured graphs. forward() takes the arguments of
    rasterize_models_views (the context is the module's) and applies its argument checks; image size and scale_modifier must
    stay the same from step to step, everything in `capture_key` re-captures when it changes."""
    NAME, ALTERNATIVE = "CapturedModelsViews", "rasterize_models_views"
    OUT_KEYS = ("color", "radii", "depth_alpha", "act_scales")

    def __init__(self, context=None, headroom: float = 1.5):
        super().__init__(context, headroom)
        self._key = None

    # ------------------------------------------------------------------------------------------------ public
    def forward(self, settings_list: Sequence, models: Sequence, means2D: torch.Tensor,
                scale_noise: Optional[torch.Tensor] = None, sh_noise: Optional[torch.Tensor] = None, noise=None) -> List[tuple]:
        settings_list = tuple(settings_list)
        V = len(settings_list)
        if V < 1 or V > VW.MAX_VIEWS:
            raise ValueError(f"1..{VW.MAX_VIEWS} views per call")
        flat = []
        for m in models:
            flat.extend(S._leaves(m))
        if not VW._uniform(settings_list):
            raise ValueError("CapturedModelsViews: all views of a call must have the same image size and scale_modifier")
        if any(s.score_flag for s in settings_list):
            raise ValueError("score_flag views are forward-only: GaussianRasterizerViews / views.importance_scores render them batched")
        P = sum(int(flat[6 * m].shape[0]) for m in range(len(flat) // 6))
        if means2D.dim() != 3 or tuple(means2D.shape) != (V, P, 3):
            raise ValueError(f"means2D must be [V,P,3] = [{V},{P},3], got {tuple(means2D.shape)}")
        specs = S._view_specs(noise, V, scale_noise, sh_noise)
        if not flat or flat[0].device.type != "cuda":
            raise L.GsrError("the HIP rasterizer needs tensors on a cuda (ROCm) device; there is no CPU fallback")
        rc = S._scene_rc(self.context)
        differentiable = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [means2D] + flat)
        out = _CapturedModelsFn.apply(self, settings_list, rc, scale_noise, sh_noise,
                                      None if specs is None else tuple(specs), differentiable, means2D, *flat)
        return [tuple(out[4 * k:4 * k + 4]) for k in range(V)]

    # ------------------------------------------------------------------------------------------------ internals
    def _eager_forward(self, settings_list, models, scale_noise, sh_noise, specs, rc):
        """Exactly what rasterize_models_views runs."""
        V = len(settings_list)
        scenes = [dict(models=models, scale_noise=None if scale_noise is None else scale_noise[k],
                       sh_noise=None if sh_noise is None else sh_noise[k],
                       noise=None if specs is None else specs[k]) for k in range(V)]
        res = VW.rasterize_views_forward_raw(settings_list, None, None, None, None, None, None, None, scenes=scenes, rc=rc)
        return self._eager_result(res)

    def _forward(self, settings_list, models, scale_noise, sh_noise, specs, rc):
        eager = lambda: self._eager_forward(settings_list, models, scale_noise, sh_noise, specs, rc)
        V = len(settings_list)
        s0 = settings_list[0]
        dev = models[0][0].device
        P, K = _scene_PK(models)
        if (P == 0 or K not in CAPTURABLE_K or not R.uses_columns(P, s0.image_height, s0.image_width)
                or not 1 <= len(models) <= L.GSR_MAX_MODELS or rc.profile is not None or not _in_place_readable(models, dev)):
            return eager()       # nothing to capture (module docstring), and no warm-up to count
        if scale_noise is not None and tuple(scale_noise.shape) != (V, P, 3):
            raise ValueError(f"scale_noise must be [V,P,3], got {tuple(scale_noise.shape)}")
        if sh_noise is not None and tuple(sh_noise.shape) != (V, P, K, 3):
            raise ValueError(f"sh_noise must be [V,P,K,3], got {tuple(sh_noise.shape)}")
        key = capture_key(settings_list, models, scale_noise, sh_noise, specs, rc)
        if key != self._key:
            # another step shape (a densified model is new tensors): its pair counts are learnt afresh
            self._key, self._cap, self._warm, self._peak_n = key, None, 0, 0
        cap = self._cap
        if cap is None:
            if self._warm < WARM_CALLS:
                self._warm += 1
                return eager()
            self._cap = cap = self._capture(settings_list, models, scale_noise, sh_noise, specs, rc, P, K)
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            self._write_step(cap, settings_list, scale_noise, sh_noise, specs, rc, stream.cuda_stream)
            ok = self._replay(cap, stream, rc)
        return (cap.outs, cap, None) if ok else eager()

    def _write_step(self, cap, settings_list, scale_noise, sh_noise, specs, rc, stream) -> None:
        """This step's cameras and stream ids -> the device memory the captured views point into (one launch), its noise
        tensors -> the static buffers."""
        V = cap.V
        structs = (L.GsrView * V)(*[user_view(s, cap.P, cap.K, rc) for s in settings_list])
        ids = None
        if cap.words is not None:
            ids = (C.c_uint32 * V)(*[0 if (sp is None or isinstance(sp.stream, torch.Tensor)) else int(sp.stream)
                                     for sp in specs])
        L.check(L.load().gsr_pack_views_streams(V, structs, ids, cap.packed.data_ptr(),
                                                None if cap.words is None else cap.words.data_ptr(), stream),
                "gsr_pack_views_streams")
        for bufs, src in ((cap.sn, scale_noise), (cap.hn, sh_noise)):
            if bufs is not None:
                torch._foreach_copy_(bufs, [src[k] for k in range(V)])

    def _capture(self, settings_list, models, scale_noise, sh_noise, specs, rc, P, K) -> _ModelsCapture:
        dev = models[0][0].device
        V = len(settings_list)
        # every view its own noise buffers: separate allocations, so that each is 16-byte aligned whatever P is
        new = lambda *shape: [torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(V)]

        def static_inputs(cap):
            cap.sn = new(P, 3) if scale_noise is not None else None
            cap.hn = new(P, K, 3) if sh_noise is not None else None
            # the stream ids of integer-stream specs: view k reads word k (consecutive words: one K1 / K8 pass serves the views)
            own = specs is not None and any(sp is not None and not isinstance(sp.stream, torch.Tensor) for sp in specs)
            cap.words = torch.zeros(V, dtype=torch.int32, device=dev) if own else None
            scenes = []
            for k in range(V):
                sp = None if specs is None else specs[k]
                if sp is not None and not isinstance(sp.stream, torch.Tensor):
                    sp = dataclasses.replace(sp, stream=cap.words[k:k + 1])
                scenes.append(dict(models=models, scale_noise=None if cap.sn is None else cap.sn[k],
                                   sh_noise=None if cap.hn is None else cap.hn[k], noise=sp))
            return [(None, None, None, None, None, scene) for scene in scenes]

        # (the first, un-captured write fills the words too)
        cap = G.capture_forward(
            self, _ModelsCapture, settings_list, P, K, rc, dev, static_inputs,
            lambda cap, stream: self._write_step(cap, settings_list, scale_noise, sh_noise, specs, rc, stream))
        # per view the gradient through the returned scales has its own allocation: the library wants it 16-byte aligned
        cap.g_scales = new(P, 3)
        cap.bwd = None
        cap.gC = {}              # which views have a gradient through their scales, or the caller's gradient addresses -> graph C
        return cap

    def _backward_call(self, cap: _ModelsCapture, rc, has_gs, first: bool = False, direct=None):
        """The backward over the static buffers (or, direct = (gcs, gdas, gss), over the caller's gradient tensors): once
        eagerly into fresh tensors (`first`: they become the static results and nothing of the caller's is touched -- no buffer
        added to, no statistics), then under capture."""
        bufs = rc.model_grad_buffers
        gcs, gdas, gss = direct if direct is not None else (list(cap.g_color), list(cap.g_da), cap.g_scales)
        gss = [gss[k] if has_gs[k] else None for k in range(cap.V)]
        kw = dict(dL_dscales_outs=gss if any(has_gs) else None)
        if first:
            return R.rasterize_backward_views_scene_raw(cap.states, gcs, gdas, private_scratch=True, **kw)
        return R.rasterize_backward_views_scene_raw(
            cap.states, gcs, gdas, model_grads=bufs if bufs is not None else cap.bwd["model_grads"],
            accumulate=bufs is not None, stats=rc.densify_stats, stats_views=rc.stats_views, reuse=cap.bwd, **kw)

    def _graph_c(self, cap: _ModelsCapture, rc, has_gs, direct=None):
        """Graph C of one pattern of scale gradients over the static buffers, or -- direct -- over the caller's own gradient
        tensors (graph.py, _direct_graph: a loss produces its gradients at the same addresses step after step, and then
        nothing is copied); None when the direct graphs are used up."""
        key = has_gs if direct is None else tuple(None if t is None else t.data_ptr() for ts in direct for t in ts)
        g = cap.gC.get(key)
        if g is None:
            if direct is not None and sum(not isinstance(k[0], bool) for k in cap.gC) >= G.MAX_DIRECT_GRAPHS:
                return None
            dev = cap.g_color.device
            if cap.bwd is None:
                cap.bwd = self._backward_call(cap, rc, has_gs, first=True)
                # (held here for good: autograd is handed tensors somebody else references, so AccumulateGrad copies them
                #  into .grad instead of adopting the capture's static memory)
                cap.bwd_m2d = cap.bwd["dL_dmeans2D"]
                if rc.model_grad_buffers is not None:      # K8 adds into the caller's buffers: the first run's tensors go
                    cap.bwd["model_grads"] = [(None,) * 6 for _ in cap.bwd["model_grads"]]
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=cap.gF.pool(), capture_error_mode="thread_local"):
                self._backward_call(cap, rc, has_gs, direct=direct)
            cap.gC[key] = g
            if direct is not None:
                self.stats["captures_bwd_direct"] = self.stats.get("captures_bwd_direct", 0) + 1
        return g

    def _backward(self, cap: Optional[_ModelsCapture], eager_states, grads, rc):
        V = len(grads) // 4
        gss = [grads[4 * k + 3] for k in range(V)]
        bufs = rc.model_grad_buffers
        if cap is None:            # a warm-up / overflow / uncapturable step: the eager backward on the eager states
            gcs, gdas = G.eager_upstream(eager_states, grads, 4)
            return R.rasterize_backward_views_scene_raw(eager_states, gcs, gdas, model_grads=bufs, accumulate=bufs is not None,
                                                        dL_dscales_outs=gss if any(g is not None for g in gss) else None,
                                                        stats=rc.densify_stats, stats_views=rc.stats_views, profile=rc.profile)
        dev = cap.g_color.device
        with torch.cuda.device(dev):
            # a view without a gradient through its scales gets what the eager path gives it: no pointer (one graph C per
            # pattern; a trainer's pattern does not change)
            has_gs = tuple(g is not None for g in gss)
            gcs, gdas = [grads[4 * k] for k in range(V)], [grads[4 * k + 2] for k in range(V)]
            usable = G.direct_usable(gcs, gdas, gss, cap.P)
            graph_c = self._graph_c(cap, rc, has_gs, direct=(gcs, gdas, gss)) if usable else None
            if graph_c is None:
                graph_c = self._graph_c(cap, rc, has_gs)
                G.stage_upstream(cap, gcs, gdas, cap.g_scales, gss)
            graph_c.replay()
        return dict(dL_dmeans2D=cap.bwd_m2d, model_grads=cap.bwd["model_grads"])
