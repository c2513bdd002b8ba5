"""densify_and_prune / prune / prune_points (dreamscene_amd/densify.py over csrc/densify.hip) against the reference's own
functions (tests/golden/densify.npz, written by tests/golden/make_densify_golden.py) and against tests/densify_ref.py, the
plain-torch restatement that the first test pins to that fixture.

Bars: every COPIED value -- all survivors and clones, every moment, children's rotation / f_dc / f_rest / opacity, the
statistics -- bit-equal; children's xyz and scaling within 1e-5 of their tensor's own largest entry (README "Parity bars per
tensor"), no outlier allowance; P_out, segment sizes and the origin of every row equal. Inputs keep every compared quantity a
relative 1e-4 away from its threshold (asserted), so no row is exempt from anything."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

from tests import densify_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = DR.NAMES
MARGIN = 1e-4


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "densify.npz"))


def fixture_inputs(d, prefix="in/"):
    st = {n: d[prefix + n] for n in NAMES}
    st.update({n + "/exp_avg": d[f"{prefix}{n}/exp_avg"] for n in NAMES})
    st.update({n + "/exp_avg_sq": d[f"{prefix}{n}/exp_avg_sq"] for n in NAMES})
    st.update({k: d[prefix + k] for k in ("xyz_gradient_accum", "denom", "max_radii2D")})
    return st


def margin_violations(scaling, opacity, N, dense, big_ws, min_opacity):
    near = lambda v, thr: np.abs(v - thr) <= MARGIN * abs(thr)
    smax = np.exp(scaling.astype(np.float64)).max(axis=1)
    sig = 1.0 / (1.0 + np.exp(-opacity.astype(np.float64).reshape(-1)))
    return near(smax, dense) | near(smax, big_ws) | near(smax / (0.8 * N), big_ws) | near(sig, min_opacity)


TH = dict(max_grad=0.0002, min_opacity=0.05, extent=2.0, percent_dense=0.01)


def synth_state(P, K, seed, N=2, moments=True):
    """A seeded model state whose classes (keep / clone / split / pruned) are all populated, with denom = 0 rows of both kinds
    (0 / 0 = NaN -> 0 and x / 0 = inf -> selected) and the margin condition enforced by redrawing."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    st = {"xyz": f(P, 3), "f_dc": f(P, 1, 3), "f_rest": f(P, K - 1, 3), "rotation": f(P, 4) * 1.3}
    scaling, opacity = np.empty((P, 3), np.float32), np.empty((P, 1), np.float32)
    todo = np.ones(P, bool)
    while todo.any():
        n = int(todo.sum())
        top = np.exp(rng.uniform(np.log(0.004), np.log(0.5), size=n))
        scaling[todo] = np.log(top[:, None] * rng.uniform(0.3, 1.0, size=(n, 3))).astype(np.float32)
        o = np.where(rng.random(n) < 0.3, rng.uniform(0.002, 0.045, size=n), rng.uniform(0.06, 0.98, size=n))
        opacity[todo, 0] = np.log(o / (1 - o)).astype(np.float32)
        todo = margin_violations(scaling, opacity, N, TH["percent_dense"] * TH["extent"], 0.1 * TH["extent"], TH["min_opacity"])
    st["scaling"], st["opacity"] = scaling, opacity
    denom = rng.integers(0, 6, size=P).astype(np.float32)
    g = np.where(rng.random(P) < 0.45, rng.uniform(0.00025, 0.002, size=P), rng.uniform(0.0, 0.00015, size=P))
    accum = (g * denom).astype(np.float32)
    zero = denom == 0
    accum[zero] = np.where(rng.random(int(zero.sum())) < 0.5, 0.0, 0.001).astype(np.float32)
    st["xyz_gradient_accum"], st["denom"] = accum, denom
    st["max_radii2D"] = np.floor(rng.uniform(0, 30, size=P)).astype(np.float32)
    if moments:
        for n in NAMES:
            st[n + "/exp_avg"] = f(*st[n].shape) * 0.01
            st[n + "/exp_avg_sq"] = np.square(f(*st[n].shape)) * 1e-4
    return st


def check_margins(st, N=2):
    bad = margin_violations(st["scaling"], st["opacity"], N, TH["percent_dense"] * TH["extent"], 0.1 * TH["extent"],
                            TH["min_opacity"])
    assert not bad.any(), "the inputs put a row within 1e-4 of a threshold"


def make_optimizer(st, dev, cls=torch.optim.Adam, step=3.0):
    """Groups named as GaussianModel.training_setup names them (+ background); Adam state injected when st carries moments."""
    params = {n: nn.Parameter(torch.tensor(st[n], device=dev)) for n in NAMES}
    bg = nn.Parameter(torch.tensor([0.25, 0.5, 0.75], device=dev))
    groups = [{"params": [params[n]], "lr": 1e-3, "name": n} for n in NAMES] + [{"params": [bg], "lr": 1e-3, "name": "background"}]
    opt = cls(groups, lr=0.0, eps=1e-15)
    if "xyz/exp_avg" in st:
        for n in NAMES + ("background",):
            p = bg if n == "background" else params[n]
            m1 = torch.full_like(p, 0.5) if n == "background" else torch.tensor(st[n + "/exp_avg"], device=dev)
            m2 = torch.full_like(p, 0.25) if n == "background" else torch.tensor(st[n + "/exp_avg_sq"], device=dev)
            opt.state[p] = {"step": torch.tensor(step), "exp_avg": m1, "exp_avg_sq": m2}
    return opt


def make_ref(st, dev="cpu", cls=torch.optim.Adam):
    opt = make_optimizer(st, dev, cls)
    t = lambda k: torch.tensor(st[k], device=dev)
    return DR.RefGaussians(opt, t("xyz_gradient_accum"), t("denom"), t("max_radii2D"), percent_dense=TH["percent_dense"])


def make_ours(st, dev, cls=torch.optim.Adam):
    from dreamscene_amd import densify
    opt = make_optimizer(st, dev, cls)
    stats = densify.DensifyStats(st["xyz"].shape[0], dev)
    stats.replace(*(torch.tensor(st[k], device=dev) for k in ("max_radii2D", "xyz_gradient_accum", "denom")))
    return opt, stats


def bits(a):
    a = a.detach().cpu().contiguous() if isinstance(a, torch.Tensor) else torch.tensor(np.ascontiguousarray(a))
    return a.view(torch.int32) if a.dtype == torch.float32 else a


def assert_bit_equal(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} words differ"


def assert_matches(got, ref, what, n_copied):
    """got / ref: {name: tensor}, moments {name: (m1, m2)}, stats (accum, denom, radii); rows >= n_copied are children."""
    for n in NAMES:
        a, b = got["params"][n].detach().cpu(), ref["params"][n].detach().cpu()
        assert a.shape == b.shape, (what, n, tuple(a.shape), tuple(b.shape))
        if n in ("xyz", "scaling"):
            assert_bit_equal(a[:n_copied], b[:n_copied], f"{what}: {n} of the copied rows")
            if a.shape[0] > n_copied:
                bar = 1e-5 * float(b.abs().max())
                e = float((a[n_copied:].double() - b[n_copied:].double()).abs().max())
                print(f"{what}: children {n}: max error {e:.3e}, bar {bar:.3e}")
                assert e <= bar, (what, n, e, bar)
        else:
            assert_bit_equal(a, b, f"{what}: {n}")
        assert (n in got["moments"]) == (n in ref["moments"]), (what, n)
        if n in ref["moments"]:
            for k in range(2):
                assert_bit_equal(got["moments"][n][k], ref["moments"][n][k], f"{what}: moment {k} of {n}")
    for k, name in enumerate(("xyz_gradient_accum", "denom", "max_radii2D")):
        assert_bit_equal(got["stats"][k], ref["stats"][k], f"{what}: {name}")


def ref_view(ref):
    return dict(params=ref.leaves(), moments=ref.moments(), stats=(ref.xyz_gradient_accum, ref.denom, ref.max_radii2D))


def ours_view(res, opt, stats):
    moments = {}
    for n in NAMES:
        s = opt.state.get(res[n], None)
        if s is not None and "exp_avg" in s:
            moments[n] = (s["exp_avg"], s["exp_avg_sq"])
    return dict(params=dict(res), moments=moments, stats=(stats.xyz_gradient_accum, stats.denom, stats.max_radii2D))


def fixture_view(d, tag):
    return dict(params={n: torch.tensor(d[f"{tag}/{n}"]) for n in NAMES},
                moments={n: (torch.tensor(d[f"{tag}/{n}/exp_avg"]), torch.tensor(d[f"{tag}/{n}/exp_avg_sq"])) for n in NAMES},
                stats=tuple(torch.tensor(d[f"{tag}/{k}"]) for k in ("xyz_gradient_accum", "denom", "max_radii2D")))


def fixture_thresholds(d):
    return dict(max_grad=float(d["max_grad"]), min_opacity=float(d["min_opacity"]), extent=float(d["extent"]),
                percent_dense=float(d["percent_dense"]))


FIXTURE_RUNS = ("dp_none", "dp_20", "prune", "imp")


def run_ref(ref, tag, d=None, th=TH, N=2, noise=None, screen=20):
    if tag == "dp_none":
        ref.densify_and_prune(th["max_grad"], th["min_opacity"], th["extent"], None, N=N, noise=noise)
    elif tag == "dp_20":
        ref.densify_and_prune(th["max_grad"], th["min_opacity"], th["extent"], screen, N=N, noise=noise)
    elif tag == "prune":
        ref.prune(th["min_opacity"], th["extent"], screen)
    else:
        ref.prune_points(torch.tensor(d["imp/mask"], device=ref.origin.device))


def run_ours(opt, stats, tag, d=None, th=TH, N=2, noise=None, screen=20, seed=None):
    from dreamscene_amd import densify
    dev = opt.param_groups[0]["params"][0].device
    if tag in ("dp_none", "dp_20"):
        return densify.densify_and_prune(opt, stats, th["max_grad"], th["min_opacity"], th["extent"],
                                         None if tag == "dp_none" else screen, percent_dense=th["percent_dense"], N=N,
                                         noise=None if noise is None else noise.to(dev), seed=seed)
    if tag == "prune":
        return densify.prune(opt, stats, th["min_opacity"], th["extent"], screen)
    return densify.prune_points(opt, stats, torch.tensor(d["imp/mask"], device=dev))


# ---- 1. CPU: the checker reproduces the reference's own functions ------------------------------------------------------------

@pytest.mark.parametrize("tag", FIXTURE_RUNS)
def test_checker_reproduces_the_reference_fixture(tag):
    d = golden()
    th = fixture_thresholds(d)
    assert th == TH and int(d["max_screen_size"]) == 20 and int(d["N"]) == 2
    st = fixture_inputs(d)
    check_margins(st)
    ref = make_ref(st)
    noise = torch.tensor(d[tag + "/noise"]) if tag.startswith("dp") else None
    run_ref(ref, tag, d, th, noise=noise)
    if tag.startswith("dp"):
        assert ref.segments(2) == tuple(int(x) for x in d[tag + "/segments"])
        n_copied = int(d[tag + "/segments"][:2].sum())
    else:
        assert ref.leaf("xyz").shape[0] == int(d[tag + "/segments"][0])
        n_copied = ref.leaf("xyz").shape[0]
    assert np.array_equal(ref.origin.numpy().astype(np.int32), d[tag + "/src"])
    fx, rv = fixture_view(d, tag), ref_view(ref)
    assert_matches(rv, fx, "checker vs fixture " + tag, n_copied)
    # the same torch ops on the same CPU: the children are bit-equal too, which is stronger than the 1e-6 the issue asks for
    for n in ("xyz", "scaling"):
        assert_bit_equal(rv["params"][n], fx["params"][n], f"children {n} (bit-equal)")
    st_bg = ref.optimizer.state[next(g for g in ref.optimizer.param_groups if g["name"] == "background")["params"][0]]
    assert float(st_bg["step"]) == 3.0


# ---- 2. CPU: the ABI -------------------------------------------------------------------------------------------------------------

def test_densify_abi_without_gpu(built_lib):
    from dreamscene_amd import _lib
    lib = built_lib
    header = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gsr_densify_scratch_bytes", "gsr_densify_plan", "gsr_densify_plan_mask", "gsr_densify_apply"):
        assert name + "(" in header, name
        assert hasattr(raw, name), name
        assert name in bound, name
    # NULL arguments: GSR_EINVAL before any HIP call
    assert lib.gsr_densify_plan(None, None, 0, None, None, None) == -1
    assert lib.gsr_densify_plan_mask(None, 5, None, 0, None, None, None) == -1
    assert lib.gsr_densify_apply(None, None, 0, None, None) == -1
    plan = _lib.GsrDensifyPlan()
    plan.P, plan.N = 10, 2
    assert lib.gsr_densify_plan(ctypes.byref(plan), None, 0, None, None, None) == -1
    tab = _lib.GsrDensifyTable()
    assert lib.gsr_densify_apply(ctypes.byref(tab), None, 0, None, None) == -1
    # scratch: monotone in P, refused sizes are 0
    sizes = [lib.gsr_densify_scratch_bytes(P, 2) for P in (0, 1, 63, 64, 65, 257, 100_000, 1_200_000, 3_000_000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] >= 3_000_000
    assert lib.gsr_densify_scratch_bytes(3_000_000, 8) > 0          # the env model's cap, every row split eight ways
    assert lib.gsr_densify_scratch_bytes(-1, 2) == 0 and lib.gsr_densify_scratch_bytes(10, 0) == 0
    assert lib.gsr_densify_scratch_bytes(10, 9) == 0 and lib.gsr_densify_scratch_bytes(2 ** 31 - 1, 2) == 0
    # the ctypes mirrors have the C compiler's sizes
    src = r'''
    #include <stdio.h>
    #include "gsrast.h"
    int main(){ printf("%zu %zu %zu\n", sizeof(GsrDensifyPlan), sizeof(GsrDensifyTensor), sizeof(GsrDensifyTable)); return 0; }
    '''
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(tmp, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        c_sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert c_sizes == [ctypes.sizeof(t) for t in (_lib.GsrDensifyPlan, _lib.GsrDensifyTensor, _lib.GsrDensifyTable)]


def test_densify_host_side_errors(built_lib):
    from dreamscene_amd import densify
    from dreamscene_amd._lib import GsrError
    st = synth_state(40, 4, seed=1)
    opt = make_optimizer(st, "cpu")
    stats = densify.DensifyStats(40, "cpu")
    with pytest.raises(ValueError):                      # clones are exempt from the split only because 0 < max_grad
        densify.densify_and_prune(opt, stats, 0.0, 0.05, 2.0, None, percent_dense=0.01)
    with pytest.raises(ValueError):
        densify.densify_and_prune(opt, stats, 0.0002, 0.05, 2.0, None, percent_dense=0.01, N=9)
    with pytest.raises(GsrError):                        # no CPU fallback
        densify.densify_and_prune(opt, stats, 0.0002, 0.05, 2.0, None, percent_dense=0.01)
    with pytest.raises(GsrError):
        densify.prune_points(opt, stats, torch.zeros(40, dtype=torch.bool))


def test_the_product_does_not_import_the_checker():
    for dp, _, fs in os.walk(os.path.join(ROOT, "dreamscene_amd")):
        for f in fs:
            if f.endswith(".py"):
                assert "densify_ref" not in open(os.path.join(dp, f)).read(), f


# ---- 3. GPU: against the fixture and the checker ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tag", FIXTURE_RUNS)
def test_gpu_matches_the_reference_fixture(built_lib, tag):
    dev = torch.device("cuda:0")
    d = golden()
    st = fixture_inputs(d)
    check_margins(st)
    noise = torch.tensor(d[tag + "/noise"]) if tag.startswith("dp") else None
    opt, stats = make_ours(st, dev)
    res = run_ours(opt, stats, tag, d, noise=noise)
    seg = tuple(int(x) for x in d[tag + "/segments"])
    assert res.segments == seg and res["xyz"].shape[0] == sum(seg)
    assert np.array_equal(res.src.cpu().numpy(), d[tag + "/src"])
    n_copied = sum(seg[:2]) if tag.startswith("dp") else seg[0]
    assert_matches(ours_view(res, opt, stats), fixture_view(d, tag), "gpu vs fixture " + tag, n_copied)
    for n in NAMES:
        assert float(opt.state[res[n]]["step"]) == 3.0


def _gpu_vs_checker(st, tag, N=2, th=TH, seed=77, what=""):
    dev = torch.device("cuda:0")
    P = st["xyz"].shape[0]
    noise = torch.randn(N, P, 3, generator=torch.Generator().manual_seed(seed)) if tag.startswith("dp") else None
    d = {"imp/mask": (np.random.default_rng(seed).random(P) < 0.4)}
    ref = make_ref(st)
    ref.percent_dense = th["percent_dense"]
    run_ref(ref, tag, d, th, N=N, noise=noise)
    opt, stats = make_ours(st, dev)
    res = run_ours(opt, stats, tag, d, th, N=N, noise=noise)
    if tag.startswith("dp"):
        assert res.segments == ref.segments(N), (what, res.segments, ref.segments(N))
        n_copied = sum(res.segments[:2])
    else:
        n_copied = ref.leaf("xyz").shape[0]
        assert res.segments == (n_copied,)
    assert res["xyz"].shape[0] == ref.leaf("xyz").shape[0]
    assert torch.equal(res.src.cpu().long(), ref.origin), what
    assert_matches(ours_view(res, opt, stats), ref_view(ref), f"gpu vs checker {what} {tag}", n_copied)
    for n in NAMES:
        assert res[n].is_leaf and res[n].requires_grad and isinstance(res[n], nn.Parameter)
        assert res[n].shape[1:] == ref.leaf(n).shape[1:]
    return res, ref, opt, stats


@pytest.mark.gpu
@pytest.mark.parametrize("K", [16, 4])
@pytest.mark.parametrize("tag", FIXTURE_RUNS)
def test_gpu_matches_the_checker_at_100k(built_lib, K, tag):
    st = synth_state(100_000, K, seed=100 + K)
    check_margins(st)
    res, ref, _, _ = _gpu_vs_checker(st, tag, what=f"100k K={K}")
    if tag == "dp_none":
        S, C, K0, K1 = res.segments
        for share in (S - C, C, K0, 100_000 - S - K0):     # keep, clone, split, pruned: all populated
            assert share >= 5_000, res.segments


@pytest.mark.gpu
@pytest.mark.parametrize("P", [0, 1, 63, 65, 257])
@pytest.mark.parametrize("tag", FIXTURE_RUNS)
def test_gpu_small_sizes(built_lib, P, tag):
    st = synth_state(P, 16, seed=P + 5)
    check_margins(st)
    _gpu_vs_checker(st, tag, what=f"P={P}")


@pytest.mark.gpu
def test_gpu_nothing_selected_nothing_pruned(built_lib):
    st = synth_state(1000, 16, seed=3)
    th = dict(TH, max_grad=1e30, min_opacity=0.0)
    st["xyz_gradient_accum"] = np.where(st["denom"] == 0, 0.0, st["xyz_gradient_accum"]).astype(np.float32)   # no inf rows
    res, ref, opt, stats = _gpu_vs_checker(st, "dp_none", th=th, what="nothing selected")
    assert res.segments == (1000, 0, 0, 0)
    for n in NAMES:
        assert_bit_equal(res[n], st[n], n)
        assert_bit_equal(opt.state[res[n]]["exp_avg"], st[n + "/exp_avg"], n)
        assert_bit_equal(opt.state[res[n]]["exp_avg_sq"], st[n + "/exp_avg_sq"], n)


@pytest.mark.gpu
def test_gpu_every_row_split(built_lib):
    st = synth_state(777, 16, seed=4)
    st["denom"] = np.ones(777, np.float32)
    st["xyz_gradient_accum"] = np.full(777, 0.01, np.float32)
    th = dict(TH, percent_dense=0.0, min_opacity=0.0)              # max exp(scaling) > 0 always: everything selected is split
    res, _, _, _ = _gpu_vs_checker(st, "dp_none", th=th, what="every row split")
    assert res.segments == (0, 0, 777, 777)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["dp_none", "prune"])
def test_gpu_every_row_pruned(built_lib, tag):
    st = synth_state(300, 4, seed=6)
    th = dict(TH, min_opacity=2.0)
    res, _, opt, stats = _gpu_vs_checker(st, tag, th=th, what="every row pruned")
    assert res["xyz"].shape == (0, 3) and res["f_dc"].shape == (0, 1, 3) and res["f_rest"].shape == (0, 3, 3)
    assert res["opacity"].shape == (0, 1) and res["rotation"].shape == (0, 4) and res.src.shape == (0,)
    assert opt.state[res["f_rest"]]["exp_avg"].shape == (0, 3, 3) and stats.denom.shape == (0,)


@pytest.mark.gpu
def test_gpu_zero_denominators(built_lib):
    """denom = 0: accum = 0 gives NaN -> 0 (not selected), accum > 0 gives inf (selected)."""
    st = synth_state(2000, 4, seed=8)
    st["denom"][:] = 0.0
    st["xyz_gradient_accum"][:1000] = 0.0
    st["xyz_gradient_accum"][1000:] = 0.5
    res, ref, _, _ = _gpu_vs_checker(st, "dp_none", th=dict(TH, min_opacity=0.0), what="denom 0")
    src = res.src.cpu().numpy()
    S, C = res.segments[:2]
    assert (src[S:] >= 1000).all() and C + res.segments[2] == 1000       # exactly the inf rows were cloned or split
    assert set(range(1000)) <= set(src[:S].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["dp_20", "imp"])
def test_gpu_optimizer_without_state(built_lib, tag):
    st = synth_state(500, 16, seed=9, moments=False)
    res, ref, opt, _ = _gpu_vs_checker(st, tag, what="no state")
    assert len(opt.state) == 0


@pytest.mark.gpu
def test_gpu_three_children(built_lib):
    st = synth_state(3000, 9, seed=10, N=3)
    check_margins(st, N=3)
    res, _, _, _ = _gpu_vs_checker(st, "dp_20", N=3, what="N=3")
    assert len(res.segments) == 5 and res.segments[2] == res.segments[3] == res.segments[4] > 0


# ---- 4. GPU: optimizer surgery, then a step -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
def test_gpu_optimizer_surgery_and_next_step(built_lib, fused):
    from dreamscene_amd import synth
    from dreamscene_amd.optim import FusedAdam
    from dreamscene_amd.rasterizer import GaussianRasterizer
    from tests.util import settings_for
    dev = torch.device("cuda:0")
    cls = FusedAdam if fused else torch.optim.Adam
    P, K = 3000, 16
    st = synth_state(P, K, seed=21)
    st["xyz"] = (st["xyz"] * 0.4).astype(np.float32)
    noise = torch.randn(2, P, 3, generator=torch.Generator().manual_seed(5))
    opt, stats = make_ours(st, dev, cls)
    bg_group = next(g for g in opt.param_groups if g["name"] == "background")
    bg_param, bg_state = bg_group["params"][0], opt.state[bg_group["params"][0]]
    old = [g["params"][0] for g in opt.param_groups if g["name"] != "background"]
    res = run_ours(opt, stats, "dp_20", noise=noise)
    assert set(opt.state.keys()) == set(res.values()) | {bg_param} and len(opt.state) == 7
    assert all(o not in opt.state for o in old)
    assert bg_group["params"][0] is bg_param and opt.state[bg_param] is bg_state
    for g in opt.param_groups:
        if g["name"] != "background":
            assert g["params"][0] is res[g["name"]] and float(opt.state[res[g["name"]]]["step"]) == 3.0
    # the checker on the same device, the same optimizer class; then one rasterizer forward + backward and one step of each
    ref = make_ref(st, dev, cls)
    run_ref(ref, "dp_20", noise=noise.to(dev))
    cam = synth.object_cameras(1, 96, 96, radius=3.0)[0]
    gi_np, gda_np = synth.upstream_grads(96, 96, seed=3)
    gi, gda = torch.tensor(gi_np, device=dev), torch.tensor(gda_np, device=dev)

    s = settings_for(cam, [1, 1, 1], 3, dev)
    m2d = torch.zeros((res["xyz"].shape[0], 3), device=dev, requires_grad=True)
    img, radii, da = GaussianRasterizer(s)(
        means3D=res["xyz"], means2D=m2d, shs=torch.cat((res["f_dc"], res["f_rest"]), dim=1),
        opacities=torch.sigmoid(res["opacity"]), scales=torch.exp(res["scaling"]),
        rotations=torch.nn.functional.normalize(res["rotation"]))
    ((img * gi).sum() + (da * gda).sum()).backward()
    assert int((radii > 0).sum()) > 100
    # the same step from the checker's output: the gradients of the forward + backward over the RETURNED parameters go to both
    # (the rasterizer's backward sums with atomics: two runs of it are not bit-identical, an optimizer comparison needs one)
    for n in NAMES:
        assert res[n].grad is not None and res[n].grad.shape == ref.leaf(n).shape
        ref.leaf(n).grad = res[n].grad.clone()
    opt.step()
    ref.optimizer.step()
    for n in NAMES:
        a, b = res[n].detach().cpu().numpy(), ref.leaf(n).detach().cpu().numpy()
        np.testing.assert_allclose(a, b, rtol=2e-6, atol=1e-7, err_msg=n)
        sa, sb = opt.state[res[n]], ref.optimizer.state[ref.leaf(n)]
        assert float(sa["step"]) == float(sb["step"]) == 4.0
        for key in ("exp_avg", "exp_avg_sq"):
            r = sb[key].cpu().numpy()
            np.testing.assert_allclose(sa[key].cpu().numpy(), r, rtol=2e-6, atol=2e-6 * float(np.abs(r).max()), err_msg=n + key)


# ---- 5. GPU: the in-kernel generator ----------------------------------------------------------------------------------------

def _split_everything(P, seed, K=4, st_seed=30):
    st = synth_state(P, K, seed=st_seed, moments=False)
    st["denom"] = np.ones(P, np.float32)
    st["xyz_gradient_accum"] = np.full(P, 0.01, np.float32)
    th = dict(TH, percent_dense=0.0, min_opacity=0.0)
    opt, stats = make_ours(st, torch.device("cuda:0"))
    return st, run_ours(opt, stats, "dp_none", th=th, seed=seed)


@pytest.mark.gpu
def test_generator_is_a_function_of_the_seed(built_lib):
    _, a = _split_everything(5000, seed=11)
    _, b = _split_everything(5000, seed=11)
    _, c = _split_everything(5000, seed=12)
    for n in NAMES:
        assert_bit_equal(a[n], b[n], n)
        if n != "xyz":
            assert_bit_equal(a[n], c[n], n)
    assert int((a["xyz"] != c["xyz"]).any(dim=1).sum()) == a["xyz"].shape[0]
    # seed=None draws the seed from torch's default CPU generator
    torch.manual_seed(99)
    _, d = _split_everything(5000, seed=None)
    torch.manual_seed(99)
    _, e = _split_everything(5000, seed=None)
    assert_bit_equal(d["xyz"], e["xyz"], "manual_seed")
    assert not torch.equal(d["xyz"], a["xyz"])


@pytest.mark.gpu
def test_generator_does_not_depend_on_other_rows(built_lib):
    """The same parent in two different selections gets the same children."""
    dev = torch.device("cuda:0")
    P = 4000
    st = synth_state(P, 4, seed=31, moments=False)
    st["denom"] = np.ones(P, np.float32)
    th = dict(TH, percent_dense=0.0, min_opacity=0.0)
    outs = []
    for sel in (np.arange(P) % 2 == 0, np.arange(P) % 3 == 0):
        st["xyz_gradient_accum"] = np.where(sel, 0.01, 0.0).astype(np.float32)
        opt, stats = make_ours(st, dev)
        res = run_ours(opt, stats, "dp_none", th=th, seed=2024)
        S, C, Kc, _ = res.segments
        assert C == 0 and Kc == int(sel.sum())
        children = torch.zeros(2, P, 3)
        children[:, res.src[S:S + Kc].cpu().long()] = res["xyz"][S:].cpu().reshape(2, Kc, 3)
        outs.append(children)
    both = torch.arange(0, P, 6)
    assert_bit_equal(outs[0][:, both], outs[1][:, both], "children of the parents both selections split")
    assert bool((outs[0][:, both] != 0).all())


@pytest.mark.gpu
def test_generator_statistics(built_lib):
    """Whitened residuals R^T (xyz' - xyz) / exp(scaling) of >= 1e5 children per copy: mean, variance and correlations within
    five standard errors of a standard normal's (sample mean: 1 / sqrt(n); sample variance: sqrt(2 / n); sample correlation:
    1 / sqrt(n))."""
    P = 120_000
    st, res = _split_everything(P, seed=424242, st_seed=33)
    assert res.segments == (0, 0, P, P)
    src = res.src.cpu().long()
    xyz0, q, s = torch.tensor(st["xyz"]).double(), torch.tensor(st["rotation"]).double(), torch.tensor(st["scaling"]).double()
    R = DR.rotation_matrices(q)
    z = []
    for c in range(2):
        rows = slice(c * P, (c + 1) * P)
        assert torch.equal(src[rows], torch.arange(P))
        dx = res["xyz"].detach()[rows].cpu().double() - xyz0
        z.append(torch.einsum("pji,pj->pi", R, dx) / torch.exp(s))
    n = float(P)
    cols = torch.cat(z, dim=1)                        # [P, 6]: copy 0 axes, copy 1 axes
    mean, var = cols.mean(dim=0), cols.var(dim=0)
    corr = torch.corrcoef(cols.T)
    off = corr - torch.eye(6, dtype=corr.dtype)
    print("mean", mean.tolist(), "var", var.tolist(), "max |corr|", float(off.abs().max()))
    assert float(mean.abs().max()) < 5 / n ** 0.5
    assert float((var - 1).abs().max()) < 5 * (2 / n) ** 0.5
    assert float(off.abs().max()) < 5 / n ** 0.5


# ---- 6. GPU: DensifyStats carries on ----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_stats_collect_on_the_new_size(built_lib):
    from dreamscene_amd import synth
    from dreamscene_amd.rasterizer import GaussianRasterizer, RasterContext
    from tests.util import settings_for
    dev = torch.device("cuda:0")
    st = synth_state(2000, 16, seed=41)
    st["xyz"] = (st["xyz"] * 0.4).astype(np.float32)
    opt, stats = make_ours(st, dev)
    res = run_ours(opt, stats, "dp_none", seed=1)
    n = res["xyz"].shape[0]
    assert n != 2000 and all(t.shape == (n,) and not t.any() for t in stats.tensors())
    rc = RasterContext()
    cam = synth.object_cameras(1, 96, 96, radius=3.0)[0]
    gi_np, gda_np = synth.upstream_grads(96, 96, seed=3)
    m2d = torch.zeros((n, 3), device=dev, requires_grad=True)
    with stats.collect(rc):
        img, radii, da = GaussianRasterizer(settings_for(cam, [1, 1, 1], 3, dev), context=rc)(
            means3D=res["xyz"], means2D=m2d, shs=torch.cat((res["f_dc"], res["f_rest"]), dim=1),
            opacities=torch.sigmoid(res["opacity"]), scales=torch.exp(res["scaling"]),
            rotations=torch.nn.functional.normalize(res["rotation"]))
    ((img * torch.tensor(gi_np, device=dev)).sum() + (da * torch.tensor(gda_np, device=dev)).sum()).backward()
    vis = radii > 0
    assert int(vis.sum()) > 100
    assert torch.equal(stats.denom, vis.float()) and torch.equal(stats.max_radii2D, radii.float() * vis)
    np.testing.assert_allclose(stats.xyz_gradient_accum.cpu().numpy(),
                               (torch.norm(m2d.grad[:, :2], dim=-1) * vis).cpu().numpy(), rtol=1e-6, atol=1e-12)
    # ... and the next densification decides from them
    res2 = run_ours(opt, stats, "dp_none", seed=2)
    assert stats.denom.shape == (res2["xyz"].shape[0],)
