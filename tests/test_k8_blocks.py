"""-m gpu: K8's sparse form (csrc/preprocess_bwd.hip, k_preprocess_bwd_views<KT, PVS, REACHED, KPER>) workgroup by workgroup, in
both block sizes -- KPER = 1 at P = 2125 and the production form KPER = 4 at P = 262 221 -- on the scenes of tests/k8_scenes.py,
whose workgroups receive lists of 0, 1, 64 (each wave slot), 255, 256, 257, all and nearly all of their rows, a trailing chunk
past P and a partial last chunk (tests/test_k8_scenes.py checks that on the CPU). References: the sum over the views of the C
oracle's per-view gradients (computed once per case, shared), and the dense form (GSR_K8_SPARSE=0, read once per library load: one
child process for all cases). Bars: tests/util.tol_ok (1e-5 of each tensor's own max|ref|) and same_bits; every row a reference
leaves at exact zero must be BIT-zero (a missed clear of a small stale value would pass under 1e-5 * max), and every case starts
from buffers that hold stale non-zero values.

Form against form: the kernel's header says the sparse form writes bit-identical rows to the dense one; that is held here with
same_bits for every output, V >= 2, and the two forms must agree on which rows are non-zero. What same_bits (value equality)
lets through, and the header now says: a row some view SAW and no view reached is +0 in the sparse form (a clear) and may hold
-0 in the dense one, whose sigma_backward runs on an all-zero dSigma (0 * a negative rotation entry) -- about a third of such
rows in dL_dscales with shared scales. One view takes another kernel in the child (k_preprocess_bwd): 2e-6, test_scratch's bar."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import k8_layout as KL
from tests import k8_scenes as KS
from tests.util import err, rel_scale, same_bits, settings_for, tol_ok

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL, BIG = 2125, 262221
H, W = KS.H, KS.W
STALE = 7.0
PARAMS = [("means3D", "dL_dmeans3D"), ("scales", "dL_dscales"), ("rotations", "dL_drotations"), ("opacities", "dL_dopacity"),
          ("shs", "dL_dshs")]


def _bits(mask_words, P):
    """int64 words of a reached bitmap (tensor) -> bool [P]"""
    w = mask_words.cpu().numpy().view(np.uint64)
    return ((w[:, None] >> np.arange(64, dtype=np.uint64)[None]) & np.uint64(1)).astype(bool).reshape(-1)[:P]


def _check(what, a, ref, P, atol=1e-5):
    """tol_ok at the project's bar, and: every ROW the reference leaves at exact zero is bit-zero. Prints error / bar."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(P, -1)
    ref = np.asarray(ref).reshape(P, -1)
    ratio = err(a, ref) / (atol * rel_scale(ref))
    print(f"[k8 blocks] {what}: worst error / bar = {ratio:.3f}")
    assert tol_ok(a, ref, atol=atol), (what, ratio)
    zero = (ref == 0).all(1)
    assert not a[zero].view(np.int32).any(), f"{what}: a row the reference leaves at zero is not bit-zero"
    return ratio


def _poison(*numels):
    """What the next torch.empty of these sizes will hold: the caching allocator hands the freed blocks out again."""
    for n in numels:
        t = torch.full((int(n),), STALE, device=DEV)
        del t


def _tensors(case):
    t = {k: torch.tensor(v, device=DEV) for k, v in case["g"].items()}
    if case["pv"] is not None:
        t["scales"] = torch.tensor(case["pv"], device=DEV)
    return t


def _module_call(case, K, D, arena, stats=None, stats_views=None):
    """One step through GaussianRasterizerViews into `arena` -> (outs, dL_dmeans2D [V,P,3], per-view dL_dscales or None)."""
    from dreamscene_amd import rasterizer as R
    from dreamscene_amd.views import GaussianRasterizerViews
    dev = torch.device(DEV)
    V, P = len(case["cams"]), case["des"].size
    pvs = case["pv"] is not None
    t = {k: v.clone().requires_grad_(True) for k, v in _tensors(case).items()}
    sets = [settings_for(c, KS.BG, D, dev) for c in case["cams"]]
    rast = GaussianRasterizerViews(sets, context=R.RasterContext(grad_arena=arena, densify_stats=stats, stats_views=stats_views))
    m2d = torch.zeros((V, P, 3), device=dev, requires_grad=True)
    outs = rast(means3D=t["means3D"], means2D=m2d, shs=t["shs"], opacities=t["opacities"], scales=t["scales"],
                rotations=t["rotations"])
    up = [torch.tensor(y, device=dev) for k in range(V) for y in case["ups"][k]]
    _poison(V * P * 3, V * P * 3)
    gr = torch.autograd.grad([x for (img, _, da) in outs for x in (img, da)], [m2d] + ([t["scales"]] if pvs else []), up)
    torch.cuda.synchronize()
    return outs, gr[0], (gr[1] if pvs else None)


# -------------------------------------------------------------------------------------------------------------- oracle parity
PARITY = [(16, 3, False, 4), (9, 2, True, 3), (16, 1, True, 1), (9, 2, False, 1)]
PARITY_CASES = [(P, *c) for P in (SMALL, BIG) for c in PARITY] + [(SMALL, 16, 3, False, 16)]


@pytest.mark.parametrize("P,K,D,pvs,V", PARITY_CASES)
def test_oracle_parity(built_lib, c_oracle, P, K, D, pvs, V):
    """GaussianRasterizerViews into a stale GradArena, twice (the second call takes the batched K1): parameter gradients = the
    oracle's sum over the views, each view's dL_dmeans2D and per-view dL_dscales = its own oracle view, arena.reached = the rows
    some view reached, bit for bit."""
    from dreamscene_amd import multiview
    seed = (K + V) % 2
    case = KS.oracle_case(c_oracle, P, K, D, V, seed, pvs)
    union = case["reached"].any(0)
    print(f"\n[k8 blocks] P {P} K {K} V {V} pvs {pvs} seed {seed}: reached rows per block "
          f"{KL.reach_counts(union, P).tolist()[:48]}")
    for call in range(2):
        arena = multiview.GradArena(P, K, torch.device(DEV))
        arena.flat.fill_(STALE + call)
        outs, m2, dsc = _module_call(case, K, D, arena)
        tag = f"P {P} K {K} V {V} pvs {pvs} call {call}"
        for j, v in enumerate(case["views"]):
            assert np.array_equal(outs[j][1].cpu().numpy(), v["radii"]), (tag, j)
            _check(f"{tag} dL_dmeans2D[{j}]", m2[j], v["dL_dmeans2D"], P)
            if pvs:
                _check(f"{tag} dL_dscales[{j}]", dsc[j], v["dL_dscales"], P)
        for ak, rk in PARAMS:
            if not (pvs and ak == "scales"):
                _check(f"{tag} {ak}", arena.views[ak], case["sum"][rk], P)
        assert np.array_equal(_bits(arena.reached, P), union), tag


# ------------------------------------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("K,D", [(16, 3), (9, 2)])
def test_accumulate_view_by_view(built_lib, c_oracle, K, D):
    """The big form, one view at a time through rasterize_backward_raw(arena=, accumulate=j > 0): the first call overwrites the
    stale arena, the others add to the listed rows and leave the rest alone."""
    from dreamscene_amd import multiview, rasterizer as R
    P, V = BIG, 4
    case = KS.oracle_case(c_oracle, P, K, D, V, (K + V) % 2, False)
    dev = torch.device(DEV)
    t = _tensors(case)
    arena = multiview.GradArena(P, K, dev)
    arena.flat.fill_(STALE)
    for j, cam in enumerate(case["cams"]):
        s = settings_for(cam, KS.BG, D, DEV)
        _, st = R.rasterize_forward_raw(s, t["means3D"], t["opacities"], t["shs"], None, t["scales"], t["rotations"], None,
                                        want_aux=False)
        _poison(P * 3)
        o = R.rasterize_backward_raw(st, torch.tensor(case["ups"][j][0], device=DEV), torch.tensor(case["ups"][j][1], device=DEV),
                                     arena=arena, accumulate=j > 0)
        torch.cuda.synchronize()
        _check(f"accumulate K {K} dL_dmeans2D[{j}]", o["dL_dmeans2D"], case["views"][j]["dL_dmeans2D"], P)
        assert np.array_equal(_bits(arena.reached, P), case["reached"][:j + 1].any(0)), j
    for ak, rk in PARAMS:
        _check(f"accumulate K {K} {ak}", arena.views[ak], case["sum"][rk], P)


# ---------------------------------------------------------------------------------------------------------------- zero_outside
@pytest.mark.parametrize("K,D", [(9, 2), (16, 3)])
def test_zero_outside_step_after_step(built_lib, K, D):
    """GsrGrads.zero_outside (bits 1 and 2) in the big form: five steps into ONE arena, the scene (designated rows) and the
    cameras changing from step to step, step 2 with per-view scales, a torch write into the arena behind step 3 -- each step
    leaves the bits of the same step into a fresh, stale-filled arena."""
    from dreamscene_amd import multiview, synth
    P, V = BIG, 4
    dev = torch.device(DEV)
    arena = multiview.GradArena(P, K, dev)
    masks = []
    for step in range(5):
        pvs = step == 2
        g, cams, des, pv = KS.k8_scene(P, K, V, step, pvs)
        case = dict(g=g, cams=cams, des=des, pv=pv, ups=[synth.upstream_grads(H, W, seed=10 * step + k) for k in range(V)])
        assert arena.zero_outside_ok() == (step not in (3, 4)), step
        assert arena.zero_outside_ok(("means3D", "shs")) == (step != 4), step
        _, m2, dsc = _module_call(case, K, D, arena)
        fresh = multiview.GradArena(P, K, dev)
        for region in fresh.views.values():      # (region by region: the alignment padding between them is nobody's to write)
            region.fill_(STALE)
        assert not fresh.zero_outside_ok()
        _, m2_ref, dsc_ref = _module_call(case, K, D, fresh)
        for name in ("means3D", "rotations", "opacities", "shs") + (() if pvs else ("scales",)):
            assert torch.equal(arena.views[name], fresh.views[name]), f"step {step}: {name} differs from the fully cleared arena"
        if not pvs:                 # (a step with per-view scales leaves the arena's scales region as it found it)
            assert torch.equal(arena.flat, fresh.flat), step
        assert torch.equal(arena.reached, fresh.reached), step
        assert torch.equal(m2, m2_ref) and (dsc is None or torch.equal(dsc, dsc_ref)), step
        assert arena.verify_zero_outside(), step
        masks.append(arena.reached.clone())
        if step == 3:
            arena.views["shs"].mul_(2.0)      # a torch op on a view of the arena: the next backward must not trust the bitmap
    assert all(not torch.equal(masks[k], masks[k + 1]) for k in range(4)), "the steps were meant to reach different rows"
    assert arena.zero_outside_ok()


# ---------------------------------------------------------------------------------------------------------- form against form
def _raw_outputs(P, K, D, pvs, V, seed, bind=None):
    """One backward through rasterize_backward_views_raw into buffers of the test's own that hold stale values everywhere
    (a `reuse` dict) -> {name: numpy}; the dense child runs exactly this."""
    from dreamscene_amd import multiview, rasterizer as R, synth
    from dreamscene_amd import views as VW
    dev = torch.device(DEV)
    g, cams, des, pv = KS.k8_scene(P, K, V, seed, pvs)
    t = _tensors(dict(g=g, pv=pv))
    sets = [settings_for(c, KS.BG, D, dev) for c in cams]
    res = VW.rasterize_views_forward_raw(sets, t["means3D"], t["opacities"], t["shs"], None, t["scales"], t["rotations"], None)
    sts = [st for _, st in res]
    arena = multiview.GradArena(P, K, dev)
    arena.flat.fill_(STALE)
    av = arena.views
    dsc = torch.full((V, P, 3), STALE, device=dev) if pvs else av["scales"]
    reuse = dict(dL_dmeans3D=av["means3D"], dL_dopacities=av["opacities"], dL_dshs=av["shs"], dL_dcolors=None, dL_dscales=dsc,
                 dL_drotations=av["rotations"], dL_dcov3D=None, _m2d=torch.full((V, P, 3), STALE, device=dev),
                 _scratch=R._scratch_acquire(dev, V, P), _reached=None, _token=None)
    ups = [synth.upstream_grads(H, W, seed=k) for k in range(V)]
    keep = R._bind_scratch
    try:
        if bind is not None:
            R._bind_scratch = bind
        o = R.rasterize_backward_views_raw(sts, [torch.tensor(u[0], device=dev) for u in ups],
                                           [torch.tensor(u[1], device=dev) for u in ups], arena=arena, per_view_scales=pvs,
                                           reuse=reuse)
        torch.cuda.synchronize()
    finally:
        R._bind_scratch = keep
        if bind is not None:
            R._SCRATCH.clear()      # (without the contract the library may leave anything behind in the scratch)
    assert o["_zero_outside"] == 0
    out = {n: av[n].cpu().numpy().reshape(P, -1) for n in av if not (pvs and n == "scales")}
    out["dL_dmeans2D"] = o["dL_dmeans2D"].cpu().numpy().reshape(V * P, 3)
    if pvs:
        out["dL_dscales_views"] = dsc.cpu().numpy().reshape(V * P, 3)
    out["reached"] = arena.reached.cpu().numpy()
    return out


FORM_CASES = [(P, K, pvs, V) for P in (262143, 262144, BIG, SMALL) for K in (9, 16) for pvs in (False, True) for V in (2, 4)] + \
             [(BIG, K, pvs, 16) for K in (9, 16) for pvs in (False, True)] + \
             [(BIG, 16, False, 1), (BIG, 9, True, 1), (SMALL, 16, False, 1), (SMALL, 9, True, 1)]


def _form_key(P, K, pvs, V):
    return f"P{P}_K{K}_{'pvs' if pvs else 'shared'}_V{V}"


def _form_seed(P, K, pvs, V):
    return (K + V + int(pvs)) % 2


def _dense_child(path):
    """the child of the fixture below, started with GSR_K8_SPARSE=0: every FORM_CASES entry; per output the rows that hold a
    non-zero VALUE and their indices (the rows are mostly zero: 60 MB a case otherwise; a row of -0 only -- see the module's
    docstring -- is a zero row to every comparison below and is not kept), compressed"""
    store = {}
    for c in FORM_CASES:
        P, K, pvs, V = c
        for name, a in _raw_outputs(P, K, 3 if K == 16 else 2, pvs, V, _form_seed(*c)).items():
            if name == "reached":
                assert (a == -1).all() or (a[:-1] == -1).all()      # (the dense forms classify nothing: every bit set)
                continue
            nz = np.nonzero((a != 0).any(1))[0]
            store[f"{_form_key(*c)}/{name}/idx"] = nz.astype(np.int32)
            store[f"{_form_key(*c)}/{name}/rows"] = a[nz]
    np.savez_compressed(path, **store)


@pytest.fixture(scope="module")
def dense_results(built_lib, tmp_path_factory):
    """The child's results, read into memory; the file is gone again when the fixture returns."""
    path = tmp_path_factory.mktemp("k8_dense") / "dense.npz"
    cmd = [sys.executable, "-c", "import sys; from tests.test_k8_blocks import _dense_child; _dense_child(sys.argv[1])", str(path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ, GSR_K8_SPARSE="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        results = {k: z[k] for k in z.files}
    os.remove(path)
    return results


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """What this module holds for its own cases does not stay with the session: the cached oracle cases (about 200 MB of host
    memory each at the big size), the scratch of its shapes, and the device blocks the caching allocator keeps for them."""
    yield
    from dreamscene_amd import rasterizer as R
    KS.forget()
    if torch.cuda.is_available():
        R._SCRATCH.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("P,K,pvs,V", FORM_CASES)
def test_sparse_form_against_dense_form(dense_results, P, K, pvs, V):
    """The same call in this process (sparse form) and in the GSR_K8_SPARSE=0 child (dense views kernel; one view: the single-view
    kernel), both over stale buffers: the same bits in every output for V >= 2, 2e-6 for one view."""
    out = _raw_outputs(P, K, 3 if K == 16 else 2, pvs, V, _form_seed(P, K, pvs, V))
    key = _form_key(P, K, pvs, V)
    n_reached = int(_bits(torch.from_numpy(out["reached"]), P).sum())
    assert 0 < n_reached < P
    for name, a in out.items():
        if name == "reached":
            continue
        idx, rows = dense_results[f"{key}/{name}/idx"], dense_results[f"{key}/{name}/rows"]
        dense = np.zeros_like(a)
        dense[idx] = rows
        if V == 1:
            ratio = err(a, dense) / (2e-6 * rel_scale(dense))
            print(f"[k8 blocks] form against form {key} {name}: worst error / bar (2e-6) = {ratio:.3f}")
            assert tol_ok(a, dense, atol=2e-6), (key, name, ratio)
            assert not a[~(dense != 0).any(1)].view(np.int32).any(), (key, name)
        else:
            nz = (a != 0).any(1)
            assert np.array_equal(nz, (dense != 0).any(1)), (key, name, "the non-zero rows")
            assert not a[~nz].view(np.int32).any(), (key, name, "a zero row of the sparse form is not +0")
            same_bits(a, dense, f"{key} {name}")


# -------------------------------------------------------------------------------------------------------------------- no marks
@pytest.mark.parametrize("K,pvs", [(16, False), (9, True)])
def test_classification_without_marks(built_lib, K, pvs):
    """GsrGrads.reach = NULL (the protocol of test_scratch._legacy_bind): phase A classifies from the K7 sums themselves, four
    views per load group -- V = 3 is no multiple of it. Same bits as the marked run, the reached bitmap included."""
    from tests.test_scratch import _legacy_bind
    D = 3 if K == 16 else 2
    marked = _raw_outputs(BIG, K, D, pvs, 3, 1)
    plain = _raw_outputs(BIG, K, D, pvs, 3, 1, bind=_legacy_bind)
    assert 0 < int(_bits(torch.from_numpy(marked["reached"]), BIG).sum())
    for name in marked:
        same_bits(marked[name], plain[name], f"no marks K {K} {name}", max_ties=0 if name == "reached" else 4)


# ------------------------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("K,D,stats_views", [(16, 3, None), (9, 2, "all")])
def test_densification_statistics(built_lib, c_oracle, K, D, stats_views):
    """The big form with densify_stats: reached rows get theirs in the chain rule, rows a view saw and nothing reached in
    wave_exit. denom and max_radii2D are exactly what the oracle's radii give; xyz_gradient_accum is the norm of the oracle's
    dL_dmeans2D[:, :2] at the project's bar."""
    from dreamscene_amd import multiview
    P, V = BIG, 4
    case = KS.oracle_case(c_oracle, P, K, D, V, (K + V) % 2, False)
    dev = torch.device(DEV)
    counted = range(V) if stats_views == "all" else [V - 1]
    radii = np.stack([case["views"][j]["radii"] for j in counted])
    union = case["reached"].any(0)
    seen_only = (radii > 0).any(0) & ~union
    assert seen_only.sum() >= 32 and ((radii > 0).any(0) & union).sum() >= 32      # both paths are in play
    base = (np.arange(P) % 3).astype(np.float32)            # denom is ADDED to, max_radii2D maxed with what the tensors hold
    stats = tuple(torch.tensor(base * f, device=dev) for f in (1.0, 0.0, 2.0))      # (max_radii2D, xyz_gradient_accum, denom)
    arena = multiview.GradArena(P, K, dev)
    arena.flat.fill_(STALE)
    _module_call(case, K, D, arena, stats=stats, stats_views=None if stats_views is None else "all")
    assert np.array_equal(stats[2].cpu().numpy(), base * 2.0 + (radii > 0).sum(0).astype(np.float32))
    assert np.array_equal(stats[0].cpu().numpy(), np.maximum(base, radii.max(0).astype(np.float32)))
    norm = sum(np.linalg.norm(case["views"][j]["dL_dmeans2D"][:, :2].astype(np.float64), axis=1) * (case["views"][j]["radii"] > 0)
               for j in counted)
    got = stats[1].cpu().numpy().astype(np.float64)
    ratio = err(got, norm) / (1e-5 * rel_scale(norm))
    print(f"[k8 blocks] statistics K {K} views {stats_views}: xyz_gradient_accum worst error / bar = {ratio:.3f}")
    assert tol_ok(got, norm), ratio
    assert not got[norm == 0].any()
