"""Host-side pieces of the post-raster epilogue that are not per-step kernels.

* `DensifyStats`: the three per-Gaussian statistics tensors of GaussianModel (`max_radii2D`, `xyz_gradient_accum`,
  `denom`; gs_renderer.py:612-613, 1061-1065) updated INSIDE the rasterizer backward (K8) for the views whose FORWARD
  runs under `with stats.collect(context):` -- instead of five boolean-mask indexing kernels after `loss.backward()`
  (object_trainer.py:386-390). With several views per call the LAST view counts (that is what the reference's trainers
  do with the loop's last viewspace_points / visibility_filter / radii); `views="all"` or a list of indices opts in to
  more (then denom grows once per counted view and max_radii2D is the maximum over them).
* `importance_prune_mask`: the 3D-Gaussian-filtering threshold of `calculate_v_imp_score` + `prune_gaussians`
  (scene_gaussian.py:1046-1061, gs_renderer.py:1082-1087) with two k-th order statistics instead of two full sorts.
* `densify_and_prune`, `prune`, `prune_points`: the densification itself with its optimizer surgery (gs_renderer.py:889-1059)
  as one planning pass, one host read of the new sizes and one gather pass (csrc/densify.hip; SEMANTICS.md
  "densify_and_prune"). No CPU fallback: the parameters live on a ROCm device.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import torch
from torch import nn

from . import _lib as L
from . import rasterizer as R


class DensifyStats:
    def __init__(self, P: int, device):
        self.max_radii2D = torch.zeros(P, dtype=torch.float32, device=device)
        self.xyz_gradient_accum = torch.zeros(P, dtype=torch.float32, device=device)
        self.denom = torch.zeros(P, dtype=torch.float32, device=device)

    def tensors(self) -> tuple:
        return (self.max_radii2D, self.xyz_gradient_accum, self.denom)

    @contextlib.contextmanager
    def collect(self, context: "R.RasterContext", views=None):
        """Rasterizer calls using `context` whose FORWARD runs inside this block update the statistics in their backward
        (visible Gaussians only; the forward takes a snapshot of the context, so the backward may run later and on
        autograd's thread). views: for multi-view calls, which views count -- None = the last one, "all", or indices."""
        prev = (context.densify_stats, context.stats_views)
        context.densify_stats, context.stats_views = self.tensors(), views
        try:
            yield self
        finally:
            context.densify_stats, context.stats_views = prev

    def replace(self, max_radii2D: torch.Tensor, xyz_gradient_accum: torch.Tensor, denom: torch.Tensor) -> None:
        """Swap in the statistics of a new P (densify_and_prune / prune / prune_points do). Call it outside `collect`: a
        block that is open keeps handing the rasterizer the tensors it was entered with."""
        if not (max_radii2D.shape == xyz_gradient_accum.shape == denom.shape) or max_radii2D.dim() != 1:
            raise ValueError("DensifyStats.replace: three [P] tensors of one length")
        self.max_radii2D, self.xyz_gradient_accum, self.denom = max_radii2D, xyz_gradient_accum, denom

    def mean_grad(self) -> torch.Tensor:
        """grads = xyz_gradient_accum / denom with NaN -> 0 (gs_renderer.py:1035-1036)."""
        g = self.xyz_gradient_accum / self.denom
        g[g.isnan()] = 0.0
        return g


def v_importance(scaling_activated: torch.Tensor, imp_list: torch.Tensor, v_pow: float) -> torch.Tensor:
    """scene_gaussian.py:1046-1061: (volume / (volume at 90 % of the descending order)) ** v_pow * importance."""
    volume = torch.prod(scaling_activated, dim=1)
    n = volume.shape[0]
    index = int(n * 0.9)
    # sorted_descending[index] == the (n - index)-th smallest value
    kth_percent_largest = torch.kthvalue(volume, n - index).values
    return torch.pow(volume / kth_percent_largest, v_pow) * imp_list


def importance_prune_mask(v_list: torch.Tensor, percent: float) -> torch.Tensor:
    """gs_renderer.py:1082-1087: prune everything at or below the value at int(percent * (n - 1)) of the ascending order."""
    n = v_list.shape[0]
    index_nth_percentile = int(percent * (n - 1))
    value_nth_percentile = torch.kthvalue(v_list.reshape(-1), index_nth_percentile + 1).values
    return (v_list <= value_nth_percentile).squeeze()


# ---- the densification itself ---------------------------------------------------------------------------------------------

class DensifyResult(dict):
    """{group name: the new nn.Parameter} as the reference's `optimizable_tensors`, plus what the plan decided:
    segments = (surviving non-split originals, surviving clones, surviving children of copy 0, copy 1, ...) -- the output rows
    in that order -- and src [P_out] int32, the original row every output row comes from."""
    segments: tuple = ()
    src: Optional[torch.Tensor] = None


def _model_groups(optimizer) -> dict:
    groups = {}
    for g in optimizer.param_groups:
        name = g.get("name")
        if name in L.GSR_DENSIFY_NAMES:
            if name in groups or len(g["params"]) != 1:
                raise ValueError(f"densify: one group of one parameter named {name!r} expected")
            groups[name] = g
    missing = [n for n in L.GSR_DENSIFY_NAMES if n not in groups]
    if missing:
        raise ValueError(f"densify: the optimizer has no group named {missing}")
    return groups


def _checked(t: torch.Tensor, what: str, dev=None) -> torch.Tensor:
    if t.device.type != "cuda":
        raise L.GsrError(f"densify needs {what} on a cuda (ROCm) device; there is no CPU fallback")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"densify: {what} must be contiguous fp32")
    if dev is not None and t.device != dev:
        raise ValueError(f"densify: {what} is on {t.device}, the model on {dev}")
    return t


@torch.no_grad()
def _run(optimizer, stats, plan_fill, *, N: int = 1, zero_stats: bool = False, seed: int = 0, noise=None,
         mask: Optional[torch.Tensor] = None) -> DensifyResult:
    """plan -> host read of the sizes -> gather -> the reference's surgery on the optimizer and the statistics."""
    lib = L.load()
    groups = _model_groups(optimizer)
    params = {n: _checked(groups[n]["params"][0], f"parameter {n!r}") for n in L.GSR_DENSIFY_NAMES}
    xyz = params["xyz"]
    dev, P = xyz.device, xyz.shape[0]
    widths = {}
    for n, p in params.items():
        _checked(p, f"parameter {n!r}", dev)
        if p.shape[0] != P:
            raise ValueError(f"densify: parameter {n!r} has {p.shape[0]} rows, xyz has {P}")
        widths[n] = 1
        for d in p.shape[1:]:
            widths[n] *= d
    K = widths["f_rest"] // 3 + 1
    if (widths["xyz"], widths["f_dc"], widths["opacity"], widths["scaling"], widths["rotation"]) != (3, 3, 1, 3, 4) or \
            widths["f_rest"] != 3 * (K - 1) or K not in (1, 4, 9, 16):
        raise ValueError("densify: xyz [P,3], f_dc [P,1,3], f_rest [P,K-1,3] (K in 1, 4, 9, 16), opacity [P,1], scaling [P,3], "
                         "rotation [P,4] expected")
    moments = {}
    for n, p in params.items():
        st = optimizer.state.get(p, None)
        if st is not None and "exp_avg" in st:
            m1, m2 = st["exp_avg"], st["exp_avg_sq"]
            if m1.shape != p.shape or m2.shape != p.shape:
                raise ValueError(f"densify: the Adam state of {n!r} does not have its parameter's shape")
            moments[n] = (_checked(m1.contiguous(), f"exp_avg of {n!r}", dev), _checked(m2.contiguous(), f"exp_avg_sq of {n!r}", dev))
    stat_src = None
    if stats is not None:
        # the table's order: xyz_gradient_accum, denom, max_radii2D
        stat_src = [_checked(t.reshape(-1), "the densification statistics", dev)
                    for t in (stats.xyz_gradient_accum, stats.denom, stats.max_radii2D)]
        if any(t.shape[0] != P for t in stat_src):
            raise ValueError(f"densify: the statistics do not have {P} rows")

    nbytes = lib.gsr_densify_scratch_bytes(P, N)
    if nbytes == 0:
        raise ValueError(f"densify: P = {P} with N = {N} does not fit 32-bit offsets")
    stream = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        sizes_dev = torch.empty(L.GSR_DENSIFY_SIZE_WORDS, dtype=torch.int32, device=dev)
        sizes_host = torch.zeros(L.GSR_DENSIFY_SIZE_WORDS, dtype=torch.int32).pin_memory()
        if mask is not None:
            L.check(lib.gsr_densify_plan_mask(mask.data_ptr(), P, scratch.data_ptr(), nbytes, sizes_dev.data_ptr(),
                                              sizes_host.data_ptr(), stream.cuda_stream), "gsr_densify_plan_mask")
        else:
            plan = L.GsrDensifyPlan()
            plan.P, plan.N = P, N
            plan.scaling, plan.opacity = params["scaling"].data_ptr(), params["opacity"].data_ptr()
            plan_fill(plan, stat_src)
            L.check(lib.gsr_densify_plan(C.byref(plan), scratch.data_ptr(), nbytes, sizes_dev.data_ptr(), sizes_host.data_ptr(),
                                         stream.cuda_stream), "gsr_densify_plan")
        stream.synchronize()                       # the ONE host read: output sizes depend on the data
        sizes = sizes_host.tolist()
        S, Cn, Kc, P_out = sizes[0], sizes[1], sizes[2], sizes[L.GSR_DENSIFY_SIZE_WORDS - 1]

        tab = L.GsrDensifyTable()
        tab.P, tab.N, tab.n_survivors, tab.n_clones, tab.n_children, tab.P_out = P, N, S, Cn, Kc, P_out
        tab.zero_stats, tab.child_divisor, tab.seed = int(zero_stats), 0.8 * N, seed & 0xFFFFFFFFFFFFFFFF
        tab.noise = None if noise is None else noise.data_ptr()
        out, out_m = {}, {}
        for k, n in enumerate(L.GSR_DENSIFY_NAMES):
            p = params[n]
            out[n] = torch.empty((P_out,) + tuple(p.shape[1:]), dtype=torch.float32, device=dev)
            e = tab.t[k]
            e.src, e.dst, e.width = p.data_ptr(), out[n].data_ptr(), widths[n]
            if n in moments:
                out_m[n] = (torch.empty_like(out[n]), torch.empty_like(out[n]))
                e.m1_src, e.m1_dst = moments[n][0].data_ptr(), out_m[n][0].data_ptr()
                e.m2_src, e.m2_dst = moments[n][1].data_ptr(), out_m[n][1].data_ptr()
        stat_dst = None
        if stat_src is not None:
            stat_dst = [torch.empty(P_out, dtype=torch.float32, device=dev) for _ in range(3)]
            for k in range(3):
                tab.stat_src[k], tab.stat_dst[k] = stat_src[k].data_ptr(), stat_dst[k].data_ptr()
        src = torch.empty(P_out, dtype=torch.int32, device=dev)
        L.check(lib.gsr_densify_apply(C.byref(tab), scratch.data_ptr(), nbytes, src.data_ptr(), stream.cuda_stream),
                "gsr_densify_apply")

    res = DensifyResult()
    for n in L.GSR_DENSIFY_NAMES:
        group = groups[n]
        old = group["params"][0]
        new = nn.Parameter(out[n].requires_grad_(True))
        st = optimizer.state.get(old, None)
        if st is not None:
            if n in out_m:
                st["exp_avg"], st["exp_avg_sq"] = out_m[n]
            del optimizer.state[old]
            optimizer.state[new] = st
        group["params"][0] = new
        res[n] = new
    if stats is not None:
        stats.replace(stat_dst[2], stat_dst[0], stat_dst[1])
    res.segments = (S, Cn) + (Kc,) * N if zero_stats else (S,)      # zero_stats <=> densify_and_prune
    res.src = src
    return res


def _prune_thresholds(plan, min_opacity: float, extent: float, max_screen_size) -> None:
    # thresholds are Python floats (doubles) in the reference: formed in double, rounded to fp32 once (ctypes does that)
    plan.min_opacity = min_opacity
    plan.use_screen_size = 1 if max_screen_size else 0
    plan.world_size_threshold = 0.1 * extent
    plan.max_screen_size = float(max_screen_size) if max_screen_size else 0.0


def densify_and_prune(optimizer, stats: DensifyStats, max_grad: float, min_opacity: float, extent: float, max_screen_size,
                      *, percent_dense: float, N: int = 2, seed: Optional[int] = None,
                      noise: Optional[torch.Tensor] = None) -> DensifyResult:
    """GaussianModel.densify_and_prune (gs_renderer.py:1034-1048) on the optimizer's groups xyz, f_dc, f_rest, opacity, scaling,
    rotation and on `stats`: clone, split into N children each, final prune; the same rows in the same order with the same
    Adam state as the reference leaves, statistics reset to zeros of the new length. The split's random numbers: a counter-based
    generator inside the kernel, a pure function of (seed, original row, copy) -- seed=None draws one from torch's default CPU
    generator -- or `noise` [N,P,3], explicit standard normals indexed [copy, row]. Every replica that passes the same seed takes
    identical decisions."""
    if not max_grad > 0:
        raise ValueError("densify_and_prune: max_grad must be > 0 (clones are exempt from the split only because their "
                         "padded gradient 0 is below it)")
    if not 1 <= int(N) <= L.GSR_DENSIFY_MAX_SPLIT or int(N) != N:
        raise ValueError(f"densify_and_prune: N must be 1..{L.GSR_DENSIFY_MAX_SPLIT}")
    if stats is None:
        raise ValueError("densify_and_prune needs the DensifyStats it decides from")
    N = int(N)
    if noise is not None:
        P = _model_groups(optimizer)["xyz"]["params"][0].shape[0]
        if tuple(noise.shape) != (N, P, 3):
            raise ValueError(f"densify_and_prune: noise must be [{N}, {P}, 3]")
        _checked(noise, "noise")
        seed = 0
    elif seed is None:
        seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64).item())

    def fill(plan, stat_src):
        plan.densify = 1
        plan.xyz_gradient_accum, plan.denom = stat_src[0].data_ptr(), stat_src[1].data_ptr()
        plan.max_radii2D = None                # densification_postfix has zeroed it before the test (:969 before :1043)
        plan.max_grad, plan.dense_threshold, plan.child_divisor = max_grad, percent_dense * extent, 0.8 * N
        _prune_thresholds(plan, min_opacity, extent, max_screen_size)
    return _run(optimizer, stats, fill, N=N, zero_stats=True, seed=int(seed), noise=noise)


def prune(optimizer, stats: Optional[DensifyStats], min_opacity: float, extent: float, max_screen_size) -> DensifyResult:
    """GaussianModel.prune (gs_renderer.py:1050-1059): the final prune test alone, with the LIVE max_radii2D; the statistics of
    the surviving rows are kept."""
    if max_screen_size and stats is None:
        raise ValueError("prune with a max_screen_size needs the DensifyStats that hold max_radii2D")

    def fill(plan, stat_src):
        plan.densify, plan.child_divisor = 0, 0.8
        plan.max_radii2D = stat_src[2].data_ptr() if stat_src is not None else None
        _prune_thresholds(plan, min_opacity, extent, max_screen_size)
    return _run(optimizer, stats, fill)


def prune_points(optimizer, stats: Optional[DensifyStats], mask: torch.Tensor) -> DensifyResult:
    """GaussianModel.prune_points (gs_renderer.py:889-903): remove the rows whose mask entry is non-zero (bool / uint8 [P], e.g.
    `importance_prune_mask`)."""
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("prune_points: mask must be bool or uint8")
    P = _model_groups(optimizer)["xyz"]["params"][0].shape[0]
    mask = mask.reshape(-1)
    if mask.shape[0] != P:
        raise ValueError(f"prune_points: mask has {mask.shape[0]} entries for {P} rows")
    if mask.device.type != "cuda":
        raise L.GsrError("prune_points needs the mask on a cuda (ROCm) device; there is no CPU fallback")
    return _run(optimizer, stats, None, mask=mask.contiguous())
