"""-m gpu: grids of more than 256 tiles a side -- the GENERAL binning path of binning.hip (k_sorted_block_sums, k_scan_blocks,
k_emit_pairs with its own-lane and whole-wave branches, radix_sort_u32<kItemsLarge, kItemsLarge> driven by a device-side
count and tile_bits, k_tile_ranges, k_rebuild_keys) and everything behind it (K6, K7, K8, the work orders at tile indices
above 255 and tile ids above 65 535) against oracle/gsr_oracle.c, through every door of the package: the raw forward in its
exact and speculated-capacity forms, the autograd module, the views module, the scene form, the captured modules.

Bars: those of tests/test_gpu_parity.py, through its own helpers -- integer artefacts bit-exact, images and gradients within
1e-5 of the tensor's largest reference entry, the three camera gradients within CAM_GRAD_SLACK. No tolerance of this file's own.

Every case first proves, FROM THE ORACLE'S OUTPUTS ALONE, that its scene exercises the path (_assert_reaches): a scene that
stops doing so fails loudly instead of passing on an empty edge."""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_parity import DEV, TOL, _check_forward, _grad_check, _run_hip, _to_dev
from tests.util import (WIDE_GRID_CASES, WIDE_GRID_FOCAL, err, oracle_view, rel_scale, settings_for, strip_camera, tol_ok,
                        wide_grid_case)

pytestmark = pytest.mark.gpu

LEAF_KEYS = ("means3D", "shs", "opacities", "scales", "rotations")
ORACLE_OF_LEAF = dict(means3D="dL_dmeans3D", shs="dL_dshs", opacities="dL_dopacity", scales="dL_dscales",
                      rotations="dL_drotations")


def _oracle_forward(CO, g, cam, bg, P, K, D, **kw):
    v = oracle_view(CO, cam, P, K, D, bg)
    return v, CO.forward(v, g["means3D"], g["opacities"], shs=g.get("shs"), colors_precomp=g.get("colors_precomp"),
                         scales=g.get("scales"), rotations=g.get("rotations"), cov3D_precomp=g.get("cov3D_precomp"), **kw)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's scene and the C oracle's forward of it: computed once, shared by the tests, never written to."""
    from oracle import c_oracle as CO
    CO.build()
    g, cam, bg, P, K, D = wide_grid_case(name)
    v, f = _oracle_forward(CO, g, cam, bg, P, K, D)
    for a in list(g.values()) + [x for x in f.values() if isinstance(x, np.ndarray)]:
        a.setflags(write=False)
    return dict(g=g, cam=cam, bg=bg, P=P, K=K, D=D, v=v, f=f)


def _assert_reaches(f, cam, both_footprints=True, deep=True):
    """What a scene must reach, from the oracle's outputs: both branches of k_emit_pairs (tiles_touched on both sides of 32),
    culled Gaussians, non-empty tiles beyond index 255 on every axis that has them, a tile rectangle across the 255 | 256
    boundary of every such axis, and a tile of more than 256 entries (more than one batch, at least one checkpoint)."""
    tt, radii, rect = f["tiles_touched"], f["radii"], f["rect"]
    gx, gy = (cam.image_width + 15) // 16, (cam.image_height + 15) // 16
    assert gx > 256 or gy > 256
    cnt = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).reshape(gy, gx)
    assert int(((tt >= 1) & (tt <= 32)).sum()) >= 100, "own-lane branch of k_emit_pairs"
    if both_footprints:
        assert int((tt > 32).sum()) >= 100, "whole-wave branch of k_emit_pairs"
    assert int((radii == 0).sum()) >= 30, "culled Gaussians"
    seen = tt > 0
    if gx > 256:
        assert cnt[:, 256:].sum() > 0, "no entry in a tile column beyond 255"
        assert int((seen & (rect[:, 0] <= 255) & (rect[:, 2] > 256)).sum()) >= 1, "no rectangle across columns 255 | 256"
    if gy > 256:
        assert cnt[256:, :].sum() > 0, "no entry in a tile row beyond 255"
        assert int((seen & (rect[:, 1] <= 255) & (rect[:, 3] > 256)).sum()) >= 1, "no rectangle across rows 255 | 256"
    if deep:
        assert cnt.max() > 256, f"deepest tile holds {cnt.max()} entries"
    return cnt


def _forward(c, g=None, mode=None, rc=None, seg_len=None, score=False):
    from dreamscene_amd import rasterizer as R
    g = c["g"] if g is None else g
    s = settings_for(c["cam"], c["bg"], c["D"], DEV, score_flag=score)
    t = _to_dev(g)
    out, st = R.rasterize_forward_raw(s, t["means3D"], t["opacities"], t.get("shs"), t.get("colors_precomp"), t.get("scales"),
                                      t.get("rotations"), t.get("cov3D_precomp"), want_keys=True, mode=mode, rc=rc,
                                      seg_len=seg_len)
    torch.cuda.synchronize()
    return out, st


def _forget_hint(c):
    """The speculated capacity of (P, H, W) on this stream, learnt from whatever test ran before: forgotten."""
    from dreamscene_amd import rasterizer as R
    dev = torch.device(DEV)
    ws = R._workspace(dev, torch.cuda.current_stream(dev).cuda_stream)
    ws.hint.pop((c["P"], c["cam"].image_height, c["cam"].image_width), None)
    return ws


@pytest.mark.parametrize("case", list(WIDE_GRID_CASES))
def test_forward_and_backward_vs_c_oracle(built_lib, c_oracle, case):
    """Exact capacity, host-side count, n_dev == NULL (mode "sync"), then the second and third "auto" calls: speculated
    capacity, count_on_device, N below the capacity -- every forward kernel of the general path takes another branch in each.
    Gradients (camera gradients included) from the speculated form.

    square: 4100 x 4112 px are 17 Mpx -- ~340 MB of fp32 planes per forward -- and the test's 4.1 s are the host's. Measured on
    an MI355X machine: a HIP forward 1 ms and the backward 8 ms; scene + oracle forward 0.9 s (run twice: here and inside
    _grad_check), synth.upstream_grads' 84 M normal deviates 0.9 s, the oracle's backward 0.65 s, every _check_forward (copying
    the planes back and comparing them) 0.46 s, three of them. The size comes from the grid (257 x 257 tiles is the smallest
    with 17 tile bits and both sides beyond 256), not from work: P = 1200."""
    c = _case(case)
    f, P = c["f"], c["P"]
    _assert_reaches(f, c["cam"], both_footprints=case != "many")
    if case == "many":
        from dreamscene_amd import _lib
        assert _lib.load().gsr_num_blocks(P) > 1024          # the second trip of k_scan_blocks' loop, with its carry
    _forget_hint(c)
    out, st = _forward(c, mode="sync")
    assert int(st.binning.count_on_device) == 0
    _check_forward(out, f, P)
    del out, st
    _forward(c, mode="auto")                              # no hint yet: exact, and leaves the hint
    for rep in (2, 3):
        out, st = _forward(c, mode="auto")
        assert int(st.binning.count_on_device) == 1, f"auto call {rep} did not speculate"
        _check_forward(out, f, P)
        del out, st
    _grad_check(c["g"], c["cam"], c["bg"], c["D"], c_oracle)


def test_capacity_overflow_on_the_general_path(built_lib, c_oracle):
    """Two renders with small splats teach the capacity, the third has the full ones and outgrows it: the clamped lists
    (k_emit_pairs stops at the capacity, the sort and k_tile_ranges run on the clamped count) are discarded and the redo
    equals the oracle."""
    c = _case("wide")
    g_full = dict(c["g"], scales=(c["g"]["scales"] * np.float32(4.0)).astype(np.float32))
    g_small = dict(c["g"], scales=(g_full["scales"] / np.float32(6.0)).astype(np.float32))
    _, f_small = _oracle_forward(c_oracle, g_small, c["cam"], c["bg"], c["P"], c["K"], c["D"])
    _, f_full = _oracle_forward(c_oracle, g_full, c["cam"], c["bg"], c["P"], c["K"], c["D"])
    hint = f_small["N"]
    assert f_full["N"] > 1.5 * hint + 65536
    # ... and beyond what the forward rounds that up to (rasterizer._forward_steps: the next multiple of q)
    want = int(hint * 1.5) + 65536
    q = max(65536, 1 << max(0, want.bit_length() - 4))
    assert f_full["N"] > (want + q - 1) // q * q
    _assert_reaches(f_full, c["cam"])
    ws = _forget_hint(c)
    for _ in range(2):
        out, st = _forward(c, g=g_small, mode="auto")
        _check_forward(out, f_small, c["P"])
    assert int(st.binning.count_on_device) == 1
    assert ws.hint[(c["P"], c["cam"].image_height, c["cam"].image_width)] == hint
    out, st = _forward(c, g=g_full, mode="auto")
    assert int(st.binning.count_on_device) == 0, "the third call did not overflow its capacity"
    _check_forward(out, f_full, c["P"])
    _forget_hint(c)


@pytest.mark.parametrize("variant", ["seg64", "seg128", "seg256", "whole_tile"])
def test_checkpoint_distances_and_whole_tile_forward(built_lib, c_oracle, variant):
    """Every distance of the forward's checkpoints (= length of the backward's work items) and the whole-tile forward
    (GsrBinning.fwd_mode = 1), as test_long_lists_multi_batch and test_whole_tile_forward_variant do on the column path."""
    from dreamscene_amd import rasterizer as R
    c = _case("wide")
    _assert_reaches(c["f"], c["cam"])
    rc = R.RasterContext(fwd_variant=1) if variant == "whole_tile" else R.RasterContext(seg_len=int(variant[3:]), fwd_variant=0)
    out, st = _forward(c, rc=rc)
    assert int(st.binning.fwd_mode) == (1 if variant == "whole_tile" else 0)
    assert int(st.binning.seg_len) == (256 if variant == "whole_tile" else int(variant[3:]))
    _check_forward(out, c["f"], c["P"])
    _grad_check(c["g"], c["cam"], c["bg"], c["D"], c_oracle, rc=rc)


def test_score_on_a_wide_grid(built_lib, c_oracle):
    """score_flag through the module: mode-0 scores (opacity x integer pixel count) carry the oracle's bits, as in
    test_autograd_module_and_score."""
    from dreamscene_amd.rasterizer import GaussianRasterizer
    c = _case("wide")
    _assert_reaches(c["f"], c["cam"])
    _, f = _oracle_forward(c_oracle, c["g"], c["cam"], c["bg"], c["P"], c["K"], c["D"], score=True)
    t = _to_dev(c["g"])
    rast = GaussianRasterizer(raster_settings=settings_for(c["cam"], c["bg"], c["D"], DEV, score_flag=True))
    with torch.no_grad():
        sc, img, radii, da = rast(means3D=t["means3D"], means2D=None, shs=t["shs"], opacities=t["opacities"],
                                  scales=t["scales"], rotations=t["rotations"])
    assert np.array_equal(radii.cpu().numpy(), f["radii"])
    assert int((f["important_score"] > 0).sum()) >= 100
    assert np.array_equal(sc.cpu().numpy(), f["important_score"]), f"mode-0 scores differ: {err(sc.cpu().numpy(), f['important_score']):.3e}"
    assert err(img.cpu().numpy(), f["image"]) <= TOL
    assert err(da.cpu().numpy(), f["depth_alpha"]) <= TOL * rel_scale(f["depth_alpha"])


def test_precomputed_inputs(built_lib, c_oracle):
    """colors_precomp + cov3D_precomp on the tall grid (the kSingle form of K8)."""
    from oracle import torch_oracle as TO
    c = _case("tall")
    g, P = c["g"], c["P"]
    g2 = dict(means3D=g["means3D"], opacities=g["opacities"],
              cov3D_precomp=TO.cov3d_from_scale_rot(torch.tensor(g["scales"]), 1.0, torch.tensor(g["rotations"])).numpy(),
              colors_precomp=np.random.default_rng(5).uniform(size=(P, 3)).astype(np.float32))
    _, f = _oracle_forward(c_oracle, g2, c["cam"], c["bg"], P, 0, 0)
    _assert_reaches(f, c["cam"])
    out, _ = _run_hip(g2, c["cam"], c["bg"], 0)
    _check_forward(out, f, P)
    _grad_check(g2, c["cam"], c["bg"], 0, c_oracle)


def _view_cameras(c, phis=(24.0, 30.0, 37.0)):
    cam = c["cam"]
    return [strip_camera(cam.image_height, cam.image_width, WIDE_GRID_FOCAL, phi=phi) for phi in phis]


def _leaves(c):
    t = {k: torch.tensor(v, device=DEV, requires_grad=True) for k, v in c["g"].items()}
    return t, [t[k] for k in LEAF_KEYS]


def test_views_module_falls_back_and_sums(built_lib, c_oracle):
    """GaussianRasterizerViews with three cameras on the wide grid (second call: the capacity hint exists, and a grid of at
    most 256 tiles a side would go through shared launches): every view's outputs are the single-view module's, bit for
    bit, and the leaf gradients are the sum of the oracle's three backward passes."""
    from dreamscene_amd import synth
    from dreamscene_amd.rasterizer import GaussianRasterizer
    from dreamscene_amd.views import GaussianRasterizerViews
    c = _case("wide")
    P, K, D, bg = c["P"], c["K"], c["D"], c["bg"]
    cams = _view_cameras(c)
    V, H, W = len(cams), c["cam"].image_height, c["cam"].image_width
    t, leaves = _leaves(c)
    ups = [synth.upstream_grads(H, W, 20 + k) for k in range(V)]
    ref = {k: 0.0 for k in LEAF_KEYS}
    for k, cam in enumerate(cams):
        v, f = _oracle_forward(c_oracle, c["g"], cam, bg, P, K, D)
        _assert_reaches(f, cam)
        b = c_oracle.backward(v, f, ups[k][0], ups[k][1], c["g"]["means3D"], shs=c["g"]["shs"], scales=c["g"]["scales"],
                              rotations=c["g"]["rotations"])
        for name in LEAF_KEYS:
            ref[name] = ref[name] + np.asarray(b[ORACLE_OF_LEAF[name]], dtype=np.float64)
    sets = [settings_for(cam, bg, D, DEV) for cam in cams]
    rast = GaussianRasterizerViews(sets)
    for _ in range(2):
        m2d = torch.zeros((V, P, 3), device=DEV, requires_grad=True)
        outs = rast(means3D=t["means3D"], means2D=m2d, shs=t["shs"], opacities=t["opacities"], scales=t["scales"],
                    rotations=t["rotations"])
        grads = torch.autograd.grad([x for (img, _, da) in outs for x in (img, da)], leaves,
                                    [torch.tensor(y, device=DEV) for k in range(V) for y in ups[k]])
    with torch.no_grad():
        for k, s in enumerate(sets):
            img, radii, da = GaussianRasterizer(raster_settings=s)(means3D=t["means3D"], means2D=None, shs=t["shs"],
                                                                    opacities=t["opacities"], scales=t["scales"],
                                                                    rotations=t["rotations"])
            assert torch.equal(outs[k][0], img) and torch.equal(outs[k][2], da) and torch.equal(outs[k][1], radii), k
    for name, a in zip(LEAF_KEYS, grads):
        r = ref[name].reshape(-1)
        e = err(a.cpu().numpy().reshape(-1), r)
        assert e <= TOL * rel_scale(r), f"dL/d{name}: {e} (max|sum of the oracle's| {np.abs(r).max()})"


def test_scene_form(built_lib):
    """The fused multi-model form (raw leaves of three models, one of them empty, noise on scales and SH) on the tall grid,
    as tests/test_scene.py::test_fused_scene_vs_oracle does it and at its bars."""
    from dreamscene_amd import rasterizer as R, synth
    from oracle import c_oracle as CO, scene_oracle as SO
    from tests.test_scene import LEAVES
    c = _case("tall")
    g, cam, bg, P, K, D = c["g"], c["cam"], c["bg"], c["P"], c["K"], c["D"]
    H, W = cam.image_height, cam.image_width
    dev = torch.device(DEV)
    sizes = [700, 0, P - 700]
    op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
    raw = (g["means3D"], np.log(g["scales"]), g["rotations"] * 1.7, np.log(op / (1 - op)), g["shs"][:, :1, :], g["shs"][:, 1:, :])
    models, at = [], 0
    for n in sizes:
        models.append(tuple(torch.tensor(np.ascontiguousarray(a[at:at + n], dtype=np.float32), device=dev, requires_grad=True)
                            for a in raw))
        at += n
    s = settings_for(cam, bg, D, dev)
    gen = torch.Generator().manual_seed(5)
    sn, hn = torch.randn((P, 3), generator=gen).to(dev), torch.randn((P, K, 3), generator=gen).to(dev)
    out, st = R.rasterize_forward_raw(s, None, None, None, None, None, None, None,
                                      scene=dict(models=models, scale_noise=sn, sh_noise=hn, want_act=True))
    cpu_models = [tuple(t.detach().cpu().requires_grad_(True) for t in m) for m in models]
    a = SO.activate_and_cat(cpu_models, sn.cpu(), hn.cpu())
    np.testing.assert_allclose(out["act_scales"].cpu().numpy(), a["scales"].detach().numpy(), rtol=4e-7)
    np.testing.assert_allclose(out["act_rotations"].cpu().numpy(), a["rotations"].detach().numpy(), rtol=0, atol=2.5e-7)
    np.testing.assert_allclose(out["act_opacities"].cpu().numpy(), a["opacities"].detach().numpy().reshape(-1), rtol=4e-7)
    act = dict(means3D=a["means3D"].detach().numpy(), shs=a["shs"].detach().numpy(),
               scales=out["act_scales"].cpu().numpy(), rotations=out["act_rotations"].cpu().numpy(),
               opacities=out["act_opacities"].cpu().numpy())
    ov = oracle_view(CO, cam, P, K, D, bg)
    ref = CO.forward(ov, act["means3D"], act["opacities"], shs=act["shs"], scales=act["scales"], rotations=act["rotations"])
    _assert_reaches(ref, cam)
    assert np.array_equal(out["radii"].cpu().numpy(), ref["radii"])
    assert out["N"] == ref["N"]
    assert np.array_equal(out["point_list"].cpu().numpy().view(np.uint32), ref["point_list"])
    assert np.array_equal(out["ranges"].cpu().numpy().view(np.uint32), ref["ranges"])
    assert tol_ok(out["color"].cpu().numpy(), ref["image"])
    assert tol_ok(out["depth_alpha"].cpu().numpy(), ref["depth_alpha"])
    gi_np, gda_np = synth.upstream_grads(H, W, seed=4)
    gs = torch.randn((P, 3), generator=gen) * 1e-3
    o = R.rasterize_backward_raw(st, torch.tensor(gi_np, device=dev), torch.tensor(gda_np, device=dev), dL_dscales_out=gs.to(dev))
    rb = CO.backward(ov, ref, gi_np, gda_np, act["means3D"], shs=act["shs"], scales=act["scales"], rotations=act["rotations"])
    torch.autograd.backward(
        [a["means3D"], a["scales"], a["rotations"], a["opacities"], a["shs"]],
        [torch.tensor(rb["dL_dmeans3D"]), torch.tensor(rb["dL_dscales"]) + gs, torch.tensor(rb["dL_drotations"]),
         torch.tensor(rb["dL_dopacity"]).reshape(a["opacities"].shape), torch.tensor(rb["dL_dshs"])])
    assert tol_ok(o["dL_dmeans2D"].cpu().numpy(), rb["dL_dmeans2D"])
    for m, (hip_row, cpu_row) in enumerate(zip(o["model_grads"], cpu_models)):
        for leaf, hg, ct in zip(LEAVES, hip_row, cpu_row):
            if ct.numel() == 0:
                continue
            refg = ct.grad.numpy() if ct.grad is not None else np.zeros(ct.shape, np.float32)
            assert tol_ok(hg.cpu().numpy(), refg), f"model {m} {leaf}: {np.abs(hg.cpu().numpy() - refg).max()}"


def _six_calls(c, V, rast_c):
    """Six calls of a CapturedViews with changing cameras, each compared bit for bit with GaussianRasterizerViews."""
    from dreamscene_amd import synth
    from dreamscene_amd.views import GaussianRasterizerViews
    P, K, D, bg = c["P"], c["K"], c["D"], c["bg"]
    H, W = c["cam"].image_height, c["cam"].image_width
    t, leaves = _leaves(c)
    ups = [torch.tensor(y, device=DEV) for k in range(V) for y in synth.upstream_grads(H, W, 30 + k)]
    for call in range(6):
        cams = _view_cameras(c, phis=[16.0 + 2.0 * call + 4.0 * k for k in range(V)])
        sets = [settings_for(cam, bg, D if (call + k) % 3 else 0, DEV) for k, cam in enumerate(cams)]
        res = []
        for which in ("captured", "views"):
            m2d = torch.zeros((V, P, 3), device=DEV, requires_grad=True)
            kw = dict(means3D=t["means3D"], means2D=m2d, opacities=t["opacities"], shs=t["shs"], scales=t["scales"],
                      rotations=t["rotations"])
            outs = rast_c(sets, **kw) if which == "captured" else GaussianRasterizerViews(sets)(**kw)
            grads = torch.autograd.grad([x for (img, _, da) in outs for x in (img, da)], leaves + [m2d], ups)
            res.append(([tuple(x.clone() for x in o) for o in outs], [x.clone() for x in grads]))
        (outs_c, grads_c), (outs_v, grads_v) = res
        for k in range(V):
            for x, y, what in zip(outs_c[k], outs_v[k], ("image", "radii", "depth_alpha")):
                assert torch.equal(x, y), f"call {call} view {k}: {what}"
        for x, y, what in zip(grads_c, grads_v, LEAF_KEYS + ("means2D",)):
            assert torch.equal(x, y), f"call {call}: dL/d{what}"


@pytest.mark.parametrize("V", [1, 3])
def test_captured_views_on_a_wide_grid(built_lib, c_oracle, V):
    """graph.CapturedViews on a grid beyond 256 tiles a side takes its eager path throughout: no warm-up bookkeeping, no
    capture (V > 1: gsr_forward_project_batch rejects such views, which used to surface as an error raised from the middle
    of a stream capture on the third call), no overflow-redo-recapture cycle (V = 1)."""
    from dreamscene_amd.graph import CapturedViews
    c = _case("wide")
    _assert_reaches(c["f"], c["cam"])
    rast = CapturedViews()
    _six_calls(c, V, rast)
    assert rast.stats["captures"] == 0 and rast.stats["overflows"] == 0, rast.stats
    assert rast.stats["eager_steps"] == 6 and rast.stats["replays"] == 0, rast.stats


def test_batch_entry_point_delivers_the_count_of_one_wide_view(built_lib, c_oracle, monkeypatch):
    """gsr_forward_project_batch with n_views = 1 accepts any grid (gsrast.h). The package's own callers do not go there --
    CapturedViews declines such grids (above) -- so this test switches that guard off: the capture then runs one view of the
    wide grid through the batch entry point, the count arrives in the pinned word (it used to stay GSR_N_PENDING: every
    replay was taken for an overflow, redone eagerly and captured again, for ever) and the replays equal the eager module."""
    from dreamscene_amd import graph, rasterizer as R
    from dreamscene_amd.graph import CapturedViews

    class _NoGuard:
        uses_columns = staticmethod(lambda P, H, W: True)

        def __getattr__(self, name):
            return getattr(R, name)
    monkeypatch.setattr(graph, "R", _NoGuard())
    c = _case("wide")
    rast = CapturedViews()
    _six_calls(c, 1, rast)
    assert rast.stats["captures"] == 1 and rast.stats["overflows"] == 0, rast.stats
    assert rast.stats["eager_steps"] == graph.WARM_CALLS and rast.stats["replays"] == 6 - graph.WARM_CALLS, rast.stats


def test_dropin_ring_declines_wide_grids(built_lib, monkeypatch):
    """GSR_DROPIN_GRAPHS switched on (the way tests/test_dropin_graphs.py does it): a wide-grid call is not eligible -- outputs
    and leaf gradients are the plain module's bit for bit, and no ring, let alone a slot, was made for it."""
    from dreamscene_amd import dropin, synth
    from dreamscene_amd.rasterizer import GaussianRasterizer, RasterContext
    monkeypatch.setattr(dropin, "ENABLED", True)
    dropin.reset()
    try:
        c = _case("wide")
        cam, P = c["cam"], c["P"]
        t, leaves = _leaves(c)
        ups = [torch.tensor(y, device=DEV) for y in synth.upstream_grads(cam.image_height, cam.image_width, 40)]
        s = settings_for(cam, c["bg"], c["D"], DEV)
        res = []
        for context in (RasterContext(dropin_graphs=False), None, None, None, None):
            m2d = torch.zeros((P, 3), device=DEV, requires_grad=True)
            img, radii, da = GaussianRasterizer(raster_settings=s, context=context)(
                means3D=t["means3D"], means2D=m2d, shs=t["shs"], opacities=t["opacities"], scales=t["scales"],
                rotations=t["rotations"])
            grads = torch.autograd.grad([img, da], leaves + [m2d], ups)
            res.append([img.clone(), radii.clone(), da.clone()] + [x.clone() for x in grads])
        for call, got in enumerate(res[1:]):
            for x, y, what in zip(got, res[0], ("image", "radii", "depth_alpha") + LEAF_KEYS + ("means2D",)):
                assert torch.equal(x, y), f"call {call}: {what}"
        assert dropin.stats() == {}, dropin.stats()
    finally:
        dropin.reset()
