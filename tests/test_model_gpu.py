"""dreamscene_amd.model.GaussianModel on the GPU: the three kernels of csrc/model.hip against tests/golden/model.npz (the reference's
own class on the CPU; tests/golden/make_model_golden.py), their tails and bounds, the two routes of the densification statistics,
and the model's whole lifecycle against a second model restored from its capture and against the torch-op restatement of
tests/model_ref.py. The bar for values that pass through logf / expf / sqrtf is the project's: 1e-5 of the compared tensor's own
largest finite entry; everything else is compared bit for bit."""
import copy
import gc
import os
import types

import numpy as np
import pytest
import torch

from dreamscene_amd import _lib as L
from dreamscene_amd import knn, scene, synth, views
from dreamscene_amd import model as M
from dreamscene_amd.densify import DensifyStats
from dreamscene_amd.optim import FusedAdam
from tests import model_ref
from tests.util import same_bits, settings_for

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model.npz"))
C0 = np.float32(0.28209479177387814)
GUARD = 12345.0
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTR = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")


@pytest.fixture(scope="module", autouse=True)
def release_cached_blocks():
    """These tests allocate many small tensors of odd sizes (257, 300, 487 ... rows). When the module is done, hand the unused
    blocks of torch's caching allocator back to the driver, so that the fragments they leave in its small-block pool do not decide
    where the tensors of the tests that follow in the same process are placed."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _np(t):
    return t.detach().cpu().numpy()


def bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} entries differ in their bits"


def within_bar(a, ref, what):
    """max |a - ref| over the finite entries <= 1e-5 max |ref|; non-finite entries in the same places with the same values.
    Returns the distance as a fraction of the bar."""
    a, ref = np.asarray(a, np.float32), np.asarray(ref, np.float32)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(a), fin), f"{what}: non-finite entries in other places"
    assert np.array_equal(a[~fin], ref[~fin], equal_nan=True), f"{what}: other non-finite values"
    if not fin.any():
        return 0.0
    scale = float(np.abs(ref[fin]).max())
    d = float(np.abs(a[fin].astype(np.float64) - ref[fin].astype(np.float64)).max())
    print(f"{what}: max distance {d:.3e}, bar {1e-5 * scale:.3e}")
    assert d <= 1e-5 * scale, f"{what}: {d:.3e} > 1e-5 * {scale:.3e}"
    return d / (1e-5 * scale) if scale else 0.0


def training_args(**over):
    a = types.SimpleNamespace(**{k: float(v) for k, v in zip(GOLD["setup/config_names"], GOLD["setup/config_values"])})
    a.iterations = int(a.iterations)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def cloud(P, seed, radius=0.5):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(P, 3))
    pts = v / np.linalg.norm(v, axis=1, keepdims=True) * (radius * np.cbrt(rng.random((P, 1))))
    return M.BasicPointCloud(points=pts, colors=rng.random((P, 3)), normals=np.zeros((P, 3)))


# ---- create_from_pcd -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deg", [0, 1, 3])
def test_create_from_pcd_matches_the_reference(deg):
    pcd = M.BasicPointCloud(points=GOLD["create/points"], colors=GOLD["create/colors"], normals=None)
    assert pcd.points.dtype == np.float64                      # rounded to fp32 once on the host
    gm = M.GaussianModel({"sh_degree": deg}, "scene")
    gm.create_from_pcd(pcd, True, 10, dist2=torch.tensor(GOLD["create/dist2"], device=DEV))
    K = (deg + 1) ** 2
    P = 257
    shapes = dict(xyz=(P, 3), f_dc=(P, 1, 3), f_rest=(P, K - 1, 3), opacity=(P, 1), scaling=(P, 3), rotation=(P, 4))
    for n in NAMES:
        t = getattr(gm, ATTR[n])
        assert isinstance(t, torch.nn.Parameter) and t.requires_grad and t.is_contiguous() and tuple(t.shape) == shapes[n], n
        assert t.device == DEV and t.dtype == torch.float32
    for n in ("xyz", "f_dc", "f_rest", "rotation"):
        bits(_np(getattr(gm, ATTR[n])), GOLD[f"create/{deg}/{n}"], n)
    within_bar(_np(gm._scaling), GOLD[f"create/{deg}/scaling"], "scaling")
    within_bar(_np(gm._opacity), GOLD[f"create/{deg}/opacity"], "opacity")
    s = _np(gm._scaling)
    assert (s[:, 0] == s[:, 1]).all() and (s[:, 0] == s[:, 2]).all()
    assert s[0, 0] == s[1, 0] == s[2, 0] and (s[3:, 0] >= s[2, 0]).all()           # dist2 0, 5e-8 and 1e-7: all at the clamp 1e-7
    assert len(np.unique(_np(gm._opacity))) == 1
    assert gm.spatial_lr_scale == 10 and gm._background.shape == (3, 1, 1) and not gm._background.any()
    for t in (gm.max_radii2D, gm.xyz_gradient_accum, gm.denom):
        assert t.shape[0] == P and not t.any()


def test_create_from_pcd_with_its_own_knn_and_empty():
    pcd = cloud(1000, 1)
    pcd.points[10:14] = pcd.points[10]                         # four copies of one point: their mean squared distance is 0
    a = M.GaussianModel({"sh_degree": 1}, "scene")
    a.create_from_pcd(pcd)
    d = knn.distCUDA2(torch.tensor(pcd.points, dtype=torch.float32, device=DEV))
    assert float(d[10]) == 0.0
    b = M.GaussianModel({"sh_degree": 1}, "scene")
    b.create_from_pcd(pcd, dist2=d)
    bits(_np(a._scaling), _np(b._scaling), "scaling from the model's own kNN")
    within_bar(_np(b._scaling[:, 0]), np.log(np.sqrt(np.maximum(_np(d), np.float32(1e-7)))), "scaling against numpy")
    empty = M.GaussianModel({"sh_degree": 3}, "scene")
    empty.create_from_pcd(M.BasicPointCloud(np.zeros((0, 3)), np.zeros((0, 3)), None))
    assert empty._features_rest.shape == (0, 15, 3) and empty._opacity.shape == (0, 1) and empty.max_radii2D.shape == (0,)
    with pytest.raises(ValueError):
        b.create_from_pcd(pcd, dist2=d[:-1])


# ---- tails and bounds ----------------------------------------------------------------------------------------------------------

def carve(sizes, shift):
    """Offsets (floats) of tensors of the given sizes in one buffer, at least one guard word before and after each; shift = 0
    puts every tensor on a 16-byte boundary, 1..3 moves all of them off it."""
    offs, at = {}, 4
    for name, n in sizes.items():
        offs[name] = at + shift
        at = (at + shift + n + 1 + 3) // 4 * 4
    return offs, at + 4


def expect_reset(x, cap=np.float32(0.01)):
    with np.errstate(all="ignore"):
        s = np.float32(1) / (np.float32(1) + np.exp(-x.astype(np.float32)))
        m = np.where(np.isnan(s), s, np.minimum(s, cap)).astype(np.float32)
        return np.log(m / (np.float32(1) - m)).astype(np.float32)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_tails_and_guard_words(P):
    lib = L.load()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    rng = np.random.default_rng(P)
    for shift, K in ((0, 4), (1, 4), (2, 16), (0, 1)):
        start, total = 5, P + 7
        sizes = dict(points=3 * P, colors=3 * P, dist2=P, xyz=3 * P, f_dc=3 * P, f_rest=3 * (K - 1) * P, scaling=3 * P,
                     rotation=4 * P, opacity=P, logit=P, logit_out=P, m1=P, m2=P, grad=3 * total, accum=P, denom=P)
        offs, n_words = carve(sizes, shift)
        host = np.full(n_words, GUARD, np.float32)
        used = np.zeros(n_words, bool)
        for n, o in offs.items():
            assert not used[o - 1] and not used[o + sizes[n]]
            used[o:o + sizes[n]] = True
        put = lambda n, a: host.__setitem__(slice(offs[n], offs[n] + sizes[n]), np.asarray(a, np.float32).reshape(-1))
        inp = dict(points=rng.normal(size=(P, 3)), colors=rng.random((P, 3)), dist2=np.exp(rng.uniform(-20, 5, P)),
                   logit=rng.uniform(-15, 15, P), m1=rng.normal(size=P), m2=rng.random(P), grad=rng.normal(size=(total, 3)),
                   accum=rng.random(P), denom=np.floor(rng.uniform(0, 5, P)))
        inp = {n: np.asarray(a, np.float32) for n, a in inp.items()}
        for n, a in inp.items():
            put(n, a)
        buf = torch.tensor(host, device=DEV)
        ptr = lambda n: buf.data_ptr() + 4 * offs[n]
        # the filter is bytes: its own guarded buffer
        keep = rng.random(P) < 0.35
        fhost = np.full(P + 8, 77, np.uint8)
        fhost[3:3 + P] = keep
        fbuf = torch.tensor(fhost, device=DEV)

        L.check(lib.gsr_model_init(ptr("points"), ptr("colors"), ptr("dist2"), P, K, 0.375, ptr("xyz"), ptr("f_dc"),
                                   ptr("f_rest") if K > 1 else None, ptr("scaling"), ptr("rotation"), ptr("opacity"), stream),
                "gsr_model_init")
        with_moments = shift != 1                              # without them: the new logits alone, the moments' words untouched
        L.check(lib.gsr_opacity_reset(ptr("logit"), P, 0.01, ptr("logit_out"), ptr("m1") if with_moments else None,
                                      ptr("m2") if with_moments else None, stream), "gsr_opacity_reset")
        L.check(lib.gsr_densify_stats(ptr("grad"), total, fbuf.data_ptr() + 3, start, P, ptr("accum"), ptr("denom"), stream),
                "gsr_densify_stats")
        got = buf.cpu().numpy()
        what = f"P={P} shift={shift} K={K}"
        assert (got[~used] == GUARD).all(), f"{what}: a guard word was written"
        assert (fbuf.cpu().numpy() == fhost).all(), f"{what}: the filter was written"
        for n in ("points", "colors", "dist2", "logit", "grad"):
            bits(got[offs[n]:offs[n] + sizes[n]], inp[n].reshape(-1), f"{what}: input {n}")
        out = lambda n: got[offs[n]:offs[n] + sizes[n]]
        bits(out("xyz"), inp["points"].reshape(-1), f"{what}: xyz")
        bits(out("f_dc"), ((inp["colors"] - np.float32(0.5)) / C0).reshape(-1), f"{what}: f_dc")
        assert not out("f_rest").any(), f"{what}: f_rest"
        bits(out("rotation"), np.tile(np.array([1, 0, 0, 0], np.float32), P), f"{what}: rotation")
        bits(out("opacity"), np.full(P, 0.375, np.float32), f"{what}: opacity")
        within_bar(out("scaling"), np.repeat(np.log(np.sqrt(np.maximum(inp["dist2"], np.float32(1e-7)))), 3), f"{what}: scaling")
        within_bar(out("logit_out"), expect_reset(inp["logit"]), f"{what}: reset logits")
        if with_moments:
            assert not out("m1").any() and not out("m2").any(), f"{what}: moments"
        else:
            bits(out("m1"), inp["m1"], f"{what}: exp_avg not handed in")
            bits(out("m2"), inp["m2"], f"{what}: exp_avg_sq not handed in")
        gx, gy = inp["grad"][start:start + P, 0], inp["grad"][start:start + P, 1]
        norm = np.sqrt(gx * gx + gy * gy)                     # float32: two products, a sum, a correctly rounded root
        bits(out("accum"), np.where(keep, inp["accum"] + norm, inp["accum"]), f"{what}: accum")
        bits(out("denom"), np.where(keep, inp["denom"] + np.float32(1), inp["denom"]), f"{what}: denom")


def test_entry_points_refuse_bad_arguments_and_accept_nothing_to_do():
    lib = L.load()
    t = torch.zeros(64, device=DEV)
    p = t.data_ptr()
    assert lib.gsr_model_init(None, None, None, 0, 4, 0.0, None, None, None, None, None, None, None) == 0
    assert lib.gsr_opacity_reset(None, 0, 0.01, None, None, None, None) == 0
    assert lib.gsr_densify_stats(None, 10, None, 10, 0, None, None, None) == 0
    assert lib.gsr_model_init(p, p, p, 2, 5, 0.0, p, p, p, p, p, p, None) == -1                   # K
    assert lib.gsr_model_init(p, p, p, -1, 4, 0.0, p, p, p, p, p, p, None) == -1
    assert lib.gsr_model_init(p, p, p, 2, 4, 0.0, p, p, None, p, p, p, None) == -1                # f_rest missing at K = 4
    assert lib.gsr_opacity_reset(p, 4, 0.01, p, None, None, None) == -1                           # in place
    assert lib.gsr_opacity_reset(p, 4, 0.01, p + 8, None, None, None) == -1                       # overlapping
    assert lib.gsr_opacity_reset(p, 4, 0.01, p + 64, p + 64, None, None) == -1                    # a moment on the output
    assert lib.gsr_densify_stats(p, 10, p + 128, 8, 3, p + 64, p + 96, None) == -1                # start + n > P_total
    assert lib.gsr_densify_stats(p, 10, p + 128, -1, 3, p + 64, p + 96, None) == -1
    assert lib.gsr_densify_stats(p, 10, p + 128, 0, 3, p + 64, p + 66, None) == -1                # misaligned
    assert not t.any()


# ---- reset_opacity -------------------------------------------------------------------------------------------------------------

def reset_model(P=300, K=4):
    rng = np.random.default_rng(11)
    gm = M.GaussianModel({"sh_degree": 1}, "scene")
    p = lambda a: torch.nn.Parameter(torch.tensor(np.asarray(a, np.float32), device=DEV))
    gm._xyz, gm._features_dc, gm._features_rest = p(rng.normal(size=(P, 3))), p(rng.normal(size=(P, 1, 3))), p(np.zeros((P, K - 1, 3)))
    gm._opacity, gm._scaling, gm._rotation = p(GOLD["reset/logits"][:, None]), p(rng.normal(size=(P, 3))), p(rng.normal(size=(P, 4)))
    gm._background = torch.nn.Parameter(torch.zeros(3, 1, 1, device=DEV))
    gm.spatial_lr_scale = 1
    gm.training_setup(training_args())
    return gm


def test_reset_opacity_matches_the_reference():
    gm = reset_model()
    assert isinstance(gm.optimizer, FusedAdam)
    for g in gm.optimizer.param_groups:
        g["lr"] = 0.0                                          # the fixture's three steps: the moments move, the logits stay
    for step in GOLD["reset/grads"]:
        for n in NAMES:
            t = getattr(gm, ATTR[n])
            t.grad = torch.tensor(step, device=DEV) if n == "opacity" else torch.ones_like(t)
        gm._background.grad = torch.ones_like(gm._background)
        gm.optimizer.step()
    old = gm._opacity
    state = gm.optimizer.state[old]
    assert _np(old).tobytes() == GOLD["reset/logits"][:, None].tobytes()
    m1, m2 = state["exp_avg"], state["exp_avg_sq"]
    within_bar(_np(m1), GOLD["reset/exp_avg_in"], "exp_avg before")
    within_bar(_np(m2), GOLD["reset/exp_avg_sq_in"], "exp_avg_sq before")
    others = [(g["params"][0], gm.optimizer.state[g["params"][0]]) for g in gm.optimizer.param_groups if g["name"] != "opacity"]
    versions = (m1._version, m2._version)

    gm.reset_opacity()

    new = gm._opacity
    assert new is not old and isinstance(new, torch.nn.Parameter) and new.requires_grad and new.grad is None
    assert new.shape == (300, 1) and gm.optimizer.param_groups[3]["params"][0] is new and gm.optimizer.param_groups[3]["name"] == "opacity"
    assert old not in gm.optimizer.state and gm.optimizer.state[new] is state and len(gm.optimizer.state) == 7
    assert float(state["step"]) == float(GOLD["reset/step"]) == 3
    assert not state["exp_avg"].any() and not state["exp_avg_sq"].any()
    assert state["exp_avg"].shape == (300, 1) and m1._version > versions[0] and m2._version > versions[1]
    assert _np(old).tobytes() == GOLD["reset/logits"][:, None].tobytes()            # the old tensor is left as it was
    rest = [(g["params"][0], gm.optimizer.state[g["params"][0]]) for g in gm.optimizer.param_groups if g["name"] != "opacity"]
    assert all(a[0] is b[0] and a[1] is b[1] for a, b in zip(others, rest))
    got, want = _np(new).reshape(-1), GOLD["reset/new_logits"]
    x = GOLD["reset/logits"]
    assert np.isneginf(want[(x == -100) | (x == -200)]).all() and np.isnan(want[np.isnan(x)]).all()
    within_bar(got, want, "new logits")                        # -inf and NaN exactly where the fixture has them
    assert (got[np.isfinite(got)] <= got[1]).all()            # x = 50 sits at the cap

    # a following step works on the new parameter and the kept state
    gm.optimizer.param_groups[3]["lr"] = 0.05
    new.grad = torch.ones_like(new)
    gm.optimizer.step()
    after = _np(gm._opacity).reshape(-1)
    fin = np.isfinite(got)
    assert float(state["step"]) == 4 and (after[fin] < got[fin]).all() and np.isfinite(after[fin]).all()


def test_reset_opacity_before_any_step_replaces_the_parameter_alone():
    gm = reset_model()
    old = gm._opacity
    gm.reset_opacity()
    assert gm._opacity is not old and gm.optimizer.param_groups[3]["params"][0] is gm._opacity
    assert len(gm.optimizer.state) == 0
    within_bar(_np(gm._opacity).reshape(-1), GOLD["reset/new_logits"], "new logits")


# ---- add_densification_stats(_div) -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["tail", "mid", "head", "whole"])
def test_densification_stats_match_the_reference(tag):
    cut = tuple(int(c) for c in GOLD[f"stats/{tag}/cut"])
    n = GOLD[f"stats/{tag}/filter0"].shape[0]
    gm = M.GaussianModel({"sh_degree": 0}, "scene")
    gm._xyz = torch.nn.Parameter(torch.zeros(n, 3, device=DEV))
    gm.stats = DensifyStats(n, DEV)
    first = range(700)[slice(*cut) if len(cut) == 2 else slice(cut[0] if cut else 0, None)].start
    mine = np.zeros(n, np.float32)
    for r in range(2):
        g = GOLD[f"stats/grad{r}"]
        keep = GOLD[f"stats/{tag}/filter{r}"]
        vsp = types.SimpleNamespace(grad=torch.tensor(g, device=DEV))
        v0 = gm.stats.denom._version
        if cut:
            gm.add_densification_stats_div(vsp, torch.tensor(keep, device=DEV), *cut)
        else:
            gm.add_densification_stats(vsp, torch.tensor(keep, device=DEV))
        assert gm.stats.denom._version > v0
        gx, gy = g[first:first + n, 0], g[first:first + n, 1]
        mine = np.where(keep, mine + np.sqrt(gx * gx + gy * gy), mine).astype(np.float32)
        assert gm.xyz_gradient_accum.shape == (n, 1) and gm.denom.shape == (n, 1)
        bits(_np(gm.denom).reshape(-1), GOLD[f"stats/{tag}/denom{r}"], f"{tag}: denom after call {r}")
        bits(_np(gm.xyz_gradient_accum).reshape(-1), mine, f"{tag}: accum after call {r}")
        within_bar(_np(gm.xyz_gradient_accum).reshape(-1), GOLD[f"stats/{tag}/accum{r}"], f"{tag}: accum after call {r}")
    if tag == "mid":                                           # cut_end = 0 means "to the end": a 500-row cut, not an empty one
        with pytest.raises(ValueError, match="500 rows"):
            gm.add_densification_stats_div(vsp, torch.tensor(keep, device=DEV), -500, 0)


def two_models():
    out = []
    for P, seed, shift in ((300, 21, -0.3), (500, 22, 0.3)):
        pcd = cloud(P, seed, radius=0.4)
        pcd.points[:, 0] += shift
        gm = M.GaussianModel({"sh_degree": 1}, "scene")
        gm.create_from_pcd(pcd)
        out.append(gm)
    return out


def scene_step(models, sets, context=None):
    V, P = len(sets), sum(m._xyz.shape[0] for m in models)
    for m in models:
        for n in NAMES:
            getattr(m, ATTR[n]).grad = None
    m2d = torch.zeros((V, P, 3), device=DEV, requires_grad=True)
    outs = scene.rasterize_models_views(sets, models, m2d, context=context)
    gen = torch.Generator().manual_seed(5)
    loss = sum(((o[0] - torch.rand(o[0].shape, generator=gen).to(DEV)) ** 2).mean() + 0.1 * o[3].mean() for o in outs)
    loss.backward()
    return outs, m2d


def test_statistics_inside_the_backward_and_after_it_leave_the_same_bits():
    cams = synth.object_cameras(2, 64, 64, radius=3.0)
    sets = [settings_for(c, [1, 1, 1], 1, DEV) for c in cams]
    models = two_models()
    both = DensifyStats(800, DEV)
    rc = scene.SceneContext()
    with both.collect(rc, views="all"):
        outs, m2d = scene_step(models, sets, rc)
    grads_inside = m2d.grad.clone()
    outs, m2d = scene_step(models, sets)                       # the same step without collect ...
    same_bits(grads_inside, m2d.grad, "means2D gradients of the two steps")
    for k in range(2):                                         # ... then one call per model and view
        vsp = types.SimpleNamespace(grad=m2d.grad[k])
        seen = outs[k][1] > 0
        models[0].add_densification_stats_div(vsp, seen[:300], 0, 300)
        models[1].add_densification_stats_div(vsp, seen[300:], -500)
    assert float(both.denom.sum()) > 100 and float(both.denom.max()) == 2
    for m, rows in ((models[0], slice(0, 300)), (models[1], slice(300, 800))):
        bits(_np(m.denom).reshape(-1), _np(both.denom[rows]), "denom")
        same_bits(m.xyz_gradient_accum.reshape(-1), both.xyz_gradient_accum[rows], "xyz_gradient_accum")
        assert float(m.xyz_gradient_accum.sum()) > 0


# ---- lifecycle -----------------------------------------------------------------------------------------------------------------

V = 2


def train_steps(gm, sets, first_iteration, n):
    for it in range(first_iteration, first_iteration + n):
        outs, m2d = scene_step([gm], sets)
        radii = outs[-1][1]
        seen = radii > 0                                       # the last view's, as the reference's trainers do
        gm.max_radii2D[seen] = torch.max(gm.max_radii2D[seen], radii[seen].float())
        gm.add_densification_stats(types.SimpleNamespace(grad=m2d.grad[-1]), seen)
        gm.update_learning_rate(it)
        gm.update_feature_learning_rate(it)
        gm.update_rotation_learning_rate(it)
        gm.update_scaling_learning_rate(it)
        gm.optimizer.step()
        gm.optimizer.zero_grad(set_to_none=True)


def gap(values, lo, hi):
    """A threshold that no row sits close to: the middle of the widest gap between neighbours of the ascending order, among
    those between the fractions lo and hi of it. (The fused and the torch-op model then take the same decisions although their
    values differ in the last bits.)"""
    v = np.sort(np.asarray(values, np.float64).reshape(-1))
    j = max(range(max(1, int(lo * v.size)), int(hi * v.size)), key=lambda k: v[k] - v[k - 1])
    assert v[j] > v[j - 1]
    return float(0.5 * (v[j] + v[j - 1]))


def leaves_of(gm):
    return {n: _np(getattr(gm, ATTR[n])) for n in NAMES}


def lifecycle(cls, pcd, sets, score_sets, plan=None, **densify_kw):
    """create -> training_setup -> 3 steps -> densify_and_prune -> reset_opacity -> prune_gaussians. plan: the thresholds, the
    split's noise and the importance scores of an earlier run (None: take them from this model). Returns (model, record, plan)."""
    args = training_args()
    gm = cls({"sh_degree": 3}, "scene")
    gm.create_from_pcd(pcd, True, 1)
    # create_from_pcd leaves isotropic Gaussians, whose covariance does not depend on the rotation: its gradient is rounding
    # residue, and Adam with eps = 1e-15 turns the residue's sign into a full step -- no two correct implementations agree on it.
    # So both models start from the same anisotropic scales and tilted rotations, where every gradient is a real one.
    with torch.no_grad():
        gen = torch.Generator().manual_seed(3)
        gm._scaling.add_((0.6 * torch.rand(gm._scaling.shape, generator=gen) - 0.3).to(DEV))
        gm._rotation.copy_(torch.randn(gm._rotation.shape, generator=gen).to(DEV))
    gm.training_setup(args)
    rec = dict(groups=[g["name"] for g in gm.optimizer.param_groups], rows=[gm._xyz.shape[0]])
    train_steps(gm, sets, 1, 3)
    rec["before_densify"] = leaves_of(gm)
    rec["stats"] = [_np(t) for t in gm.stats.tensors()]
    if plan is None:
        smax = _np(gm.get_scaling.max(dim=1).values)
        plan = dict(max_grad=gap(_np(gm.stats.mean_grad()), 0.4, 0.8), extent=gap(smax, 0.3, 0.7) / args.percent_dense,
                    min_opacity=gap(_np(gm.get_opacity), 0.1, 0.4))
        assert plan["max_grad"] > 0
    gm.densify_and_prune(plan["max_grad"], plan["min_opacity"], plan["extent"], None, **densify_kw)
    rec["rows"].append(gm._xyz.shape[0])
    gm.reset_opacity()
    rec["rows"].append(gm._xyz.shape[0])
    if "scores" not in plan:
        with torch.no_grad():
            plan["scores"] = views.importance_scores(score_sets, gm.get_xyz, gm.get_opacity, shs=gm.get_features,
                                                     scales=gm.get_scaling, rotations=gm.get_rotation)
    gm.prune_gaussians(0.1, plan["scores"])
    rec["rows"].append(gm._xyz.shape[0])
    rec["groups_after"] = [g["name"] for g in gm.optimizer.param_groups]
    for n, g in zip(NAMES, gm.optimizer.param_groups):
        p = g["params"][0]
        st = gm.optimizer.state.get(p, None)
        assert p is getattr(gm, ATTR[n]) and p.shape[0] == rec["rows"][-1] and (st is None or st["exp_avg"].shape == p.shape)
    assert all(t.shape[0] == rec["rows"][-1] for t in gm.stats.tensors())
    return gm, rec, plan


@pytest.fixture(scope="module")
def lifecycle_inputs():
    cams = synth.object_cameras(V + 2, 64, 64, radius=3.0)
    sets = [settings_for(c, [1, 1, 1], 0, DEV) for c in cams[:V]]
    score_sets = [settings_for(c, [0, 0, 0], 0, DEV, score_flag=True) for c in cams[V:]]
    return cloud(400, 31), sets, score_sets


def test_lifecycle_and_a_restored_model_step_alike(lifecycle_inputs):
    pcd, sets, score_sets = lifecycle_inputs
    gm, rec, _ = lifecycle(M.GaussianModel, pcd, sets, score_sets, seed=77)
    assert rec["groups"] == rec["groups_after"] == list(GOLD["setup/1/names"])
    print("rows after create / densify_and_prune / reset_opacity / prune_gaussians:", rec["rows"])
    assert rec["rows"][1] != rec["rows"][0] and rec["rows"][2] == rec["rows"][1] and rec["rows"][3] < rec["rows"][2]
    assert float(gm.get_opacity.detach().max()) <= 0.010001
    cap = copy.deepcopy(gm.capture())                          # a checkpoint: capture() itself hands out the live tensors
    assert len(cap) == 12
    twin = M.GaussianModel({"sh_degree": 3}, "scene")
    twin.restore(cap, training_args())
    assert twin._xyz is not gm._xyz and float(twin.optimizer.state[twin._xyz]["step"]) == 3
    for m in (gm, twin):
        train_steps(m, sets, 4, 1)
    for n in NAMES:
        same_bits(getattr(gm, ATTR[n]), getattr(twin, ATTR[n]), f"{n} one step after restore")
        same_bits(gm.optimizer.state[getattr(gm, ATTR[n])]["exp_avg"], twin.optimizer.state[getattr(twin, ATTR[n])]["exp_avg"],
                  f"exp_avg of {n} one step after restore")
    for a, b in zip(gm.stats.tensors(), twin.stats.tensors()):
        same_bits(a, b, "statistics one step after restore")


def test_lifecycle_agrees_with_the_torch_restatement(lifecycle_inputs):
    pcd, sets, score_sets = lifecycle_inputs
    noise = torch.randn(2, 400, 3, generator=torch.Generator().manual_seed(9)).to(DEV)
    gm, rec, plan = lifecycle(M.GaussianModel, pcd, sets, score_sets, noise=noise)
    ref, rec_ref, _ = lifecycle(model_ref.TorchModel, pcd, sets, score_sets, plan=plan, noise=noise)
    assert isinstance(ref.optimizer, torch.optim.Adam) and not isinstance(ref.optimizer, FusedAdam)
    assert rec["groups"] == rec_ref["groups"] and rec["groups_after"] == rec_ref["groups_after"]
    print("rows:", rec["rows"], rec_ref["rows"])
    assert rec["rows"] == rec_ref["rows"]
    for n in NAMES:
        within_bar(rec["before_densify"][n], rec_ref["before_densify"][n], f"{n} before the first densification")
    for a, b, n in zip(rec["stats"], rec_ref["stats"], ("max_radii2D", "xyz_gradient_accum", "denom")):
        within_bar(a, b, n)
