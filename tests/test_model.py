"""dreamscene_amd.model.GaussianModel without a GPU: its surface against the reference's class, the learning-rate schedules and the
optimizer's group table against tests/golden/model.npz (tests/golden/make_model_golden.py: the reference's own class on the CPU),
how add_densification_stats_div resolves its cut, what is refused, and the host-side round trips (capture / restore, PLY)."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

from dreamscene_amd import model as M
from dreamscene_amd._lib import GsrError

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model.npz"))
NOT_PROVIDED = {"extract_fields", "init_pcd", "init_env_pcd", "init_floor_pcd"}          # the issue's four exclusions


class HostModel(M.GaussianModel):
    device = "cpu"               # leaves on the host: everything that launches a kernel must refuse them


def training_args(**over):
    a = types.SimpleNamespace(**{k: float(v) for k, v in zip(GOLD["setup/config_names"], GOLD["setup/config_values"])})
    a.iterations = int(a.iterations)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def host_model(P=5, K=4, seed=0, cls=HostModel):
    rng = np.random.default_rng(seed)
    gm = cls({"sh_degree": {1: 0, 4: 1, 16: 3}[K]}, "scene")
    p = lambda *s: torch.nn.Parameter(torch.tensor(rng.normal(size=s).astype(np.float32)))
    gm._xyz, gm._features_dc, gm._features_rest = p(P, 3), p(P, 1, 3), p(P, K - 1, 3)
    gm._opacity, gm._scaling, gm._rotation = p(P, 1), p(P, 3), p(P, 4)
    gm._background = torch.nn.Parameter(torch.zeros(3, 1, 1))
    gm.spatial_lr_scale = 1
    return gm


def test_surface_matches_the_reference():
    ref = dict(s.split(":", 1) for s in GOLD["surface/params"])
    assert set(ref) == set(GOLD["surface/names"]) and NOT_PROVIDED <= set(ref)
    for name, params in ref.items():
        if name in NOT_PROVIDED:
            continue
        member = inspect.getattr_static(M.GaussianModel, name, None)
        assert member is not None, f"GaussianModel.{name} is missing"
        if params == "<property>":
            assert isinstance(member, property), name
            continue
        assert inspect.isfunction(member), name
        sig = list(inspect.signature(member).parameters.values())[1:]
        positional = [p.name for p in sig if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert positional == [p for p in params.split(",") if p], (name, positional, params)
        # what this class adds (dist2=, seed=, ...) can only be passed by keyword: positional calls mean what they meant
        assert all(p.kind == p.KEYWORD_ONLY for p in sig if p.name not in positional), name
    for name in ("BasicPointCloud", "get_expon_lr_func", "inverse_sigmoid"):
        assert hasattr(M, name)
    assert M.BasicPointCloud._fields == ("points", "colors", "normals")


def test_defaults_match_the_reference():
    d = lambda f, n: inspect.signature(f).parameters[n].default
    G = M.GaussianModel
    assert d(G.__init__, "exp_path") is None and d(G.create_from_pcd, "require_grad") is True
    assert d(G.create_from_pcd, "spatial_lr_scale") == 1 and d(G.get_covariance, "scaling_modifier") == 1
    assert d(G.load_ply, "require_grad") is True and d(G.densify_and_split, "N") == 2
    assert d(G.add_densification_stats_div, "cut_end") is None


@pytest.mark.parametrize("scale", [1, 10])
def test_learning_rate_schedules_match_the_reference(scale):
    gm = host_model()
    gm.spatial_lr_scale = scale
    gm.training_setup(training_args())
    for name, group in (("update_learning_rate", "xyz"), ("update_feature_learning_rate", "f_dc"),
                        ("update_rotation_learning_rate", "rotation"), ("update_scaling_learning_rate", "scaling")):
        want = GOLD[f"lr/{scale}/{name}"]
        for step, w in zip(GOLD["lr/steps"], want):
            got = getattr(gm, name)(int(step))
            assert abs(got - w) <= 1e-12 * abs(w), (name, step, got, w)
            assert [g for g in gm.optimizer.param_groups if g["name"] == group][0]["lr"] == got


def test_expon_lr_func_edges():
    assert M.get_expon_lr_func(0.5, 0.5)(123) == 0.5                       # constant
    assert M.get_expon_lr_func(1e-2, 1e-4)(-1) == 0.0 and M.get_expon_lr_func(0.0, 0.0, max_steps=10)(3) == 0.0
    f = M.get_expon_lr_func(1e-2, 1e-4, lr_delay_steps=100, lr_delay_mult=0.01, max_steps=1000)
    assert abs(f(0) - 1e-4) <= 1e-18 and abs(f(1000) - 1e-4) <= 1e-18 and abs(f(5000) - 1e-4) <= 1e-18
    assert abs(f(500) - 1e-3) <= 1e-15                                     # the geometric middle, warm-up over


@pytest.mark.parametrize("scale", [1, 10])
def test_training_setup_builds_the_reference_s_groups(scale):
    from dreamscene_amd.optim import FusedAdam
    gm = host_model()
    gm.spatial_lr_scale = scale
    gm.training_setup(training_args())
    assert isinstance(gm.optimizer, FusedAdam)
    groups = gm.optimizer.param_groups
    assert [g["name"] for g in groups] == list(GOLD[f"setup/{scale}/names"])
    assert [g["lr"] for g in groups] == list(GOLD[f"setup/{scale}/lrs"])
    assert all(g["eps"] == 1e-15 and g["betas"] == (0.9, 0.999) and len(g["params"]) == 1 for g in groups)
    leaves = (gm._xyz, gm._features_dc, gm._features_rest, gm._opacity, gm._scaling, gm._rotation, gm._background)
    assert all(g["params"][0] is t for g, t in zip(groups, leaves))
    assert gm.percent_dense == training_args().percent_dense
    assert gm.xyz_gradient_accum.shape == (5, 1) and gm.denom.shape == (5, 1) and gm.max_radii2D.shape == (5,)


def test_cut_resolution_is_python_slicing():
    T = 700
    for start, end, n in ((-300, None, 300), (-500, -300, 200), (0, 400, 400)):             # the fixture's three forms
        assert M._resolve_cut(T, start, end) == (range(T)[start:end].start, n)
    rows = list(range(T))
    for start in (0, 1, 399, 699, 700, 701, 5000, -1, -699, -700, -701, -5000):
        for end in (None, 0, 1, 400, 700, 701, 5000, -1, -300, -700, -5000):
            want = rows[start:end] if end else rows[start:]          # `if cut_end:` -- 0 means "to the end"
            first, n = M._resolve_cut(T, start, end)
            assert n == len(want) and (n == 0 or first == want[0]), (start, end)
            assert 0 <= first and first + n <= T


def test_stats_refuse_wrong_lengths_missing_gradients_and_cpu_tensors():
    gm = host_model(P=300)
    gm.training_setup(training_args())
    vsp = types.SimpleNamespace(grad=torch.zeros(700, 3))
    keep = torch.ones(300, dtype=torch.bool)
    with pytest.raises(ValueError, match="300 rows"):
        gm.add_densification_stats_div(vsp, torch.ones(299, dtype=torch.bool), -300)
    with pytest.raises(ValueError):
        gm.add_densification_stats_div(vsp, keep, -500, -300)         # a 200-row cut for 300 rows
    with pytest.raises(ValueError):
        gm.add_densification_stats(vsp, torch.ones(700, dtype=torch.bool))          # 700 rows for a model of 300
    with pytest.raises(ValueError, match="grad"):
        gm.add_densification_stats(types.SimpleNamespace(grad=None), keep)
    with pytest.raises(ValueError):
        gm.add_densification_stats_div(vsp, torch.arange(300), -300)          # an index list is not a mask
    with pytest.raises(GsrError):
        gm.add_densification_stats_div(vsp, keep, -300)               # everything fits, but nothing is on the device
    assert not gm.xyz_gradient_accum.any() and not gm.denom.any()


def test_kernels_refuse_cpu_tensors():
    pcd = M.BasicPointCloud(points=np.zeros((4, 3)), colors=np.full((4, 3), 0.5), normals=np.zeros((4, 3)))
    gm = HostModel({"sh_degree": 1}, "scene")
    with pytest.raises(GsrError):
        gm.create_from_pcd(pcd, True, 1)
    with pytest.raises(GsrError):
        gm.create_from_pcd(pcd, True, 1, dist2=torch.ones(4))
    gm = host_model()
    gm.training_setup(training_args())
    before = gm._opacity
    with pytest.raises(GsrError):
        gm.reset_opacity()
    assert gm._opacity is before and gm.optimizer.param_groups[3]["params"][0] is before
    with pytest.raises(GsrError):
        gm.prune_points(torch.zeros(5, dtype=torch.bool))
    with pytest.raises(ValueError, match="training_setup"):
        host_model().reset_opacity()


def test_constructor_classes():
    for cls, method in (("env", "init_env_pcd"), ("floor", "init_floor_pcd")):
        with pytest.raises(ValueError, match=method):
            M.GaussianModel({"sh_degree": 0}, cls)
    for mode in ("shapes", "default", "pointe", "pointe_330k", "pointe_825k", "obj"):
        with pytest.raises(ValueError, match="init_pcd"):
            M.GaussianModel({"sh_degree": 0, "init_guided": mode, "init_prompt": "a chair"}, "object", "/tmp/exp")
    with pytest.raises(ValueError, match="gaussian_class"):
        M.GaussianModel({"sh_degree": 0}, "sky")
    with pytest.raises(ValueError, match="exp_path"):
        M.GaussianModel({"sh_degree": 0, "init_guided": "default"}, "object")
    gm = M.GaussianModel({"sh_degree": 2}, "scene")
    assert gm.max_sh_degree == 2 and gm.active_sh_degree == 0 and gm.optimizer is None and gm._xyz.numel() == 0
    assert gm.max_radii2D.numel() == 0 and gm.xyz_gradient_accum.numel() == 0 and gm.denom.numel() == 0

    # a checkout's subclass keeps its samplers: the constructor hands them what the reference hands them
    calls = []

    class Checkout(M.GaussianModel):
        def init_pcd(self, initialize_param, exp_path):
            calls.append(("init_pcd", initialize_param["init_guided"], exp_path))

        def init_env_pcd(self, initialize_param):
            calls.append(("init_env_pcd",))

        def init_floor_pcd(self, initialize_param):
            calls.append(("init_floor_pcd",))

    Checkout({"sh_degree": 0, "init_guided": "default"}, "object", "exp")
    Checkout({"sh_degree": 0}, "env")
    Checkout({"sh_degree": 0}, "floor")
    assert calls == [("init_pcd", "default", "exp"), ("init_env_pcd",), ("init_floor_pcd",)]


def test_ply_round_trip_and_constructor_classes_that_load(tmp_path):
    gm = host_model(P=37, K=16, seed=3)
    path = str(tmp_path / "sub" / "m.ply")
    gm.save_ply(path)
    assert gm.construct_list_of_attributes()[:9] == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    assert len(gm.construct_list_of_attributes()) == 14 + 3 * 16          # xyz, normals, opacity, scale, rot: 14
    names = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    for cls in ("restore", "tmp"):
        back = HostModel({"sh_degree": 3, "path": path}, cls)
        for n in names:
            a, b = getattr(gm, n), getattr(back, n)
            # nn.Parameter(t.requires_grad_(False)) requires grad: the reference's leaves do whatever require_grad says
            assert isinstance(b, torch.nn.Parameter) and b.requires_grad and b.shape == a.shape and b.is_contiguous()
            assert a.detach().numpy().tobytes() == b.detach().numpy().tobytes(), n
        assert back.active_sh_degree == 3 and back.max_radii2D.shape == (37,) and back._background.shape == (3, 1, 1)
    # an object initialised from a saved PLY (the last branch of the reference's init_pcd), and load_ply's degree rule
    obj = HostModel({"sh_degree": 3, "init_guided": path}, "object", str(tmp_path))
    assert obj._features_rest.shape == (37, 15, 3) and obj.active_sh_degree == 3
    low = HostModel({"sh_degree": 1, "path": path}, "tmp")
    assert low._features_rest.shape == (37, 3, 3) and low.active_sh_degree == 1


def test_capture_restore_tuple_layout():
    gm = host_model(P=6)
    gm.training_setup(training_args())
    gm.active_sh_degree = 1
    gm.max_radii2D[2] = 7.0                                   # the statistics are written through the properties
    gm.xyz_gradient_accum[3] = 0.5
    gm.denom[3] += 2
    assert gm.stats.max_radii2D[2] == 7 and gm.stats.xyz_gradient_accum[3] == 0.5 and gm.stats.denom[3] == 2
    st = gm.optimizer.state[gm._opacity]
    st["step"], st["exp_avg"], st["exp_avg_sq"] = torch.tensor(4.0), torch.full((6, 1), 0.25), torch.full((6, 1), 0.5)
    cap = gm.capture()
    assert len(cap) == 12 and cap[0] == 1 and cap[11] == 1
    for k, t in enumerate((gm._xyz, gm._features_dc, gm._features_rest, gm._scaling, gm._rotation, gm._opacity), start=1):
        assert cap[k] is t
    assert cap[7].shape == (6,) and cap[8].shape == (6, 1) and cap[9].shape == (6, 1)
    assert set(cap[10]) == {"state", "param_groups"} and [g["name"] for g in cap[10]["param_groups"]][3] == "opacity"

    other = HostModel({"sh_degree": 1}, "scene")
    other.restore(cap, training_args())
    assert other.active_sh_degree == 1 and other.spatial_lr_scale == 1 and other._scaling is gm._scaling
    assert torch.equal(other.max_radii2D, gm.max_radii2D) and torch.equal(other.xyz_gradient_accum, gm.xyz_gradient_accum)
    assert torch.equal(other.denom, gm.denom) and other.denom.shape == (6, 1)
    st2 = other.optimizer.state[other._opacity]
    assert float(st2["step"]) == 4 and torch.equal(st2["exp_avg"], st["exp_avg"])
    assert [g["name"] for g in other.optimizer.param_groups] == list(GOLD["setup/1/names"])
    # the statistics survive DensifyStats.replace
    other.stats.replace(torch.ones(4), torch.full((4,), 2.0), torch.full((4,), 3.0))
    assert other.max_radii2D.shape == (4,) and float(other.xyz_gradient_accum[0, 0]) == 2 and other.denom.shape == (4, 1)


def test_torch_one_liners():
    gm = host_model(P=9, K=4, seed=5)
    assert torch.equal(gm.get_xyz, gm._xyz) and gm.get_features.shape == (9, 4, 3)
    assert torch.equal(gm.get_scaling, torch.exp(gm._scaling)) and torch.equal(gm.get_opacity, torch.sigmoid(gm._opacity))
    assert torch.allclose(gm.get_rotation.norm(dim=1), torch.ones(9)) and gm.get_background.shape == (3, 1, 1)
    # covariance: R diag(s^2) R^T, upper triangle; a rotation about z by 90 degrees swaps the x and y variances
    gm._rotation.data[0] = torch.tensor([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)])
    gm._scaling.data[0] = torch.log(torch.tensor([1.0, 2.0, 3.0]))
    cov = gm.get_covariance(2.0)[0].detach()
    assert torch.allclose(cov, torch.tensor([16.0, 0.0, 0.0, 4.0, 0.0, 36.0]), atol=1e-5)
    gm.max_sh_degree = 1
    gm.oneupSHdegree(); gm.oneupSHdegree()
    assert gm.active_sh_degree == 1
    gm.deactive_grad()
    assert not gm._xyz.requires_grad and not gm._background.requires_grad
    gm.active_grad()
    assert gm._rotation.requires_grad
    x = torch.tensor([0.1, 0.5])
    assert torch.equal(M.inverse_sigmoid(x), torch.log(x / (1 - x)))
    gm.free_memory()
    assert gm._xyz.numel() == 0 and gm.optimizer is None and gm.max_radii2D.numel() == 0


def test_torch_restatements_keep_the_optimizer_consistent():
    """cat / prune / replace on host tensors: rows, Adam state and statistics stay aligned (these exist for callers, not speed)."""
    gm = host_model(P=8, K=4, seed=7)
    gm.training_setup(training_args(percent_dense=0.01))
    for g in gm.optimizer.param_groups:
        p = g["params"][0]
        gm.optimizer.state[p] = {"step": torch.tensor(2.0), "exp_avg": torch.ones_like(p), "exp_avg_sq": torch.ones_like(p)}
    xyz0 = gm._xyz.detach().clone()
    gm._scaling.data[:] = np.log(0.001)
    gm._scaling.data[4:] = np.log(0.5)
    grads = torch.tensor([1.0, 0, 1, 0, 1, 0, 1, 0])[:, None]
    gm.densify_and_clone(grads, 0.5, 1.0)                       # rows 0 and 2 are small and moving: cloned
    assert gm._xyz.shape[0] == 10 and torch.equal(gm._xyz[8:], xyz0[[0, 2]])
    st = gm.optimizer.state[gm._xyz]
    assert float(st["step"]) == 2 and st["exp_avg"][:8].eq(1).all() and st["exp_avg"][8:].eq(0).all()
    assert gm.denom.shape == (10, 1) and gm.optimizer.param_groups[0]["params"][0] is gm._xyz
    torch.manual_seed(0)
    gm.densify_and_split(grads, 0.5, 1.0)                       # rows 4 and 6 are large and moving: two children each
    assert gm._xyz.shape[0] == 10 - 2 + 4 and gm._features_rest.shape == (12, 3, 3) and gm.max_radii2D.shape == (12,)
    assert torch.allclose(gm._scaling[8:], torch.log(torch.tensor(0.5 / 1.6)).expand(4, 3))
    out = gm.replace_tensor_to_optimizer(torch.zeros(12, 1), "opacity")
    assert out["opacity"] is gm.optimizer.param_groups[3]["params"][0] and not gm.optimizer.state[out["opacity"]]["exp_avg"].any()
    assert len(gm.optimizer.state) == 7 and gm.optimizer.state[gm._background]["exp_avg"].eq(1).all()
