"""-m gpu: dreamscene_amd.filtering on the device.
  A  kth_value against torch.sort on the CPU, value for value (NaN matches NaN, -0 == +0), at the sizes where csrc/select.hip takes
     another path and on the contents in which a wrong prefix or residual rank shows.
  B  importance_filter: its mask against its own v_list (exact), its v_list against tests/filter_ref.py in float64 (bar: 4 x the
     error of the reference's own fp32 chain), its mask against the reference's fp32 mask and tests/golden/prune.npz (exact).
  C  importance_filter replays from a captured graph: nothing in it is read by the host.
  D  gaussian_filtering on a model.GaussianModel against the torch chain of tests/model_ref.py.
The CPU references are computed once per input and shared."""
import functools

import numpy as np
import pytest
import torch

from dreamscene_amd import filtering as F
from dreamscene_amd import model as M
from dreamscene_amd import synth, views
from dreamscene_amd.densify import DensifyStats
from tests import filter_ref, model_ref
from tests.test_golden import load
from tests.util import settings_for

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
STRIDE_N = F.MAX_BLOCKS * F.BLOCK_ITEMS + 1            # one more than the capped grid covers: the stride loop runs
SIZES = (1, 2, F.WAVE - 1, F.WAVE, F.WAVE + 1, F.BLOCK - 1, F.BLOCK, F.BLOCK + 1, F.BLOCK_ITEMS - 1, F.BLOCK_ITEMS,
         F.BLOCK_ITEMS + 1, STRIDE_N)


def bits_to_float(u):
    return np.array(u, np.uint32).view(np.float32)


def ranks(n):
    return sorted({k for k in (0, 1, n // 2, n - 2, n - 1) if 0 <= k < n})


def same_values(got, want):
    """Equal as values: NaN matches NaN, -0 == +0."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


def check_kth(x: torch.Tensor, ks, what, scratch=None):
    """kth_value(x, k) in both directions for every k of ks against torch.sort on the CPU; one host read for all of them."""
    n = x.numel()
    ascending = torch.sort(x.reshape(-1))[0].numpy()
    descending = torch.sort(x.reshape(-1), descending=True)[0].numpy()
    xd = x.to(DEV)
    got_a = [F.kth_value(xd, k, scratch=scratch) for k in ks]
    got_d = [F.kth_value(xd, k, descending=True, scratch=scratch) for k in ks]
    assert all(t.dim() == 0 and t.device == DEV and t.dtype == torch.float32 for t in got_a + got_d)
    got_a, got_d = torch.stack(got_a).cpu().numpy(), torch.stack(got_d).cpu().numpy()
    assert same_values(got_a, ascending[list(ks)]), f"{what}, n = {n}, ascending k = {list(ks)}: {got_a} != {ascending[list(ks)]}"
    assert same_values(got_d, descending[list(ks)]), f"{what}, n = {n}, descending k = {list(ks)}: {got_d} != {descending[list(ks)]}"
    return got_a


SPECIALS = np.concatenate((bits_to_float([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF,
                                          0x807FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF]),
                           np.array([1.0, -1.0, 3.0e38, -3.0e38, 1e-30, -1e-30], np.float32)))


def content(name, n):
    rng = np.random.default_rng(1000 + n % 9973)
    if name == "equal":
        return np.full(n, -2.75, np.float32)
    if name == "specials":                                   # mixed signs with +-0, +-inf, denormals and NaNs of both signs
        x = rng.normal(size=n).astype(np.float32)
        pick = rng.random(n) < 0.6
        x[pick] = rng.choice(SPECIALS, int(pick.sum()))
        x[:min(n, len(SPECIALS))] = SPECIALS[:min(n, len(SPECIALS))]
        return x
    if name == "duplicates":
        return rng.choice(rng.normal(size=16).astype(np.float32), n)
    if name == "normal":
        return rng.normal(size=n).astype(np.float32)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["equal", "specials", "duplicates", "normal"])
def test_kth_value_equals_torch_sort(built_lib, name):
    for n in SIZES:
        if n == STRIDE_N and name in ("equal", "specials"):
            continue                                         # the stride loop is the same code for every content: two suffice
        check_kth(torch.from_numpy(content(name, n)), ranks(n), name)


@pytest.mark.parametrize("byte", [0, 1, 2, 3])
@pytest.mark.parametrize("negative", [False, True])
def test_kth_value_two_values_one_key_byte_apart(built_lib, byte, negative):
    """n values of which m are `lo` and n - m are `hi`, the two keys differing in exactly one byte: the pass of that byte is the
    only one with two occupied bins. k on both sides of the split and exactly at it."""
    a = 0x3F800000 | (0x80000000 if negative else 0)                       # +-1.0
    b = a ^ ((0x02 if byte == 3 else 0x01) << (8 * byte))                  # byte 3: 0x3F -> 0x3D, still a finite float
    pair = bits_to_float([a, b])
    key = lambda u: (~u & 0xFFFFFFFF) if u & 0x80000000 else u | 0x80000000
    differing = [i for i in range(4) if ((key(a) ^ key(b)) >> (8 * i)) & 0xFF]
    assert differing == [byte]
    for n, m in ((2, 1), (F.WAVE + 1, 1), (F.WAVE + 1, F.WAVE), (F.BLOCK_ITEMS + 1, F.BLOCK_ITEMS // 3), (2 * F.BLOCK_ITEMS + 5, F.BLOCK_ITEMS + 1)):
        x = np.full(n, max(pair), np.float32)
        x[np.random.default_rng(n + m).permutation(n)[:m]] = min(pair)
        ks = sorted({k for k in (0, m - 2, m - 1, m, m + 1, n - 1) if 0 <= k < n})
        got = check_kth(torch.from_numpy(x), ks, f"byte {byte}")
        assert all(got[i] == (min(pair) if k < m else max(pair)) for i, k in enumerate(ks))


def test_kth_value_with_dirty_scratch_and_out(built_lib):
    n = F.BLOCK_ITEMS + 1
    x = torch.from_numpy(content("normal", n))
    scratch = torch.full((F.scratch_bytes(n),), 0xFF, dtype=torch.uint8, device=DEV)
    first = check_kth(x, ranks(n), "dirty scratch", scratch=scratch)
    again = check_kth(x, ranks(n), "the same scratch again", scratch=scratch)
    assert first.tobytes() == again.tobytes()
    out = torch.full((3,), 7.0, device=DEV)
    r = F.kth_value(x.to(DEV).reshape(-1, 3), 5, out=out[1])
    assert r.data_ptr() == out[1].data_ptr() and out.tolist() == [7.0, float(torch.sort(x)[0][5]), 7.0]
    with pytest.raises(ValueError):
        F.kth_value(x.to(DEV), 0, scratch=scratch[:-16])
    with pytest.raises(ValueError):
        F.kth_value(x.to(DEV).double(), 0)


# ---- B: importance_filter ------------------------------------------------------------------------------------------------------

P_FIXTURE, P_BLOCK = 517, F.BLOCK_ITEMS + 1
BAND = 64                                                    # B3's precondition: nothing else within 64 x the B2 bar of the threshold


@functools.lru_cache(maxsize=None)
def filter_inputs(P, special=None):
    """-> (raw scaling [P,3], imp [P]) on the CPU. P_FIXTURE: tests/golden/prune.npz's; otherwise drawn like it."""
    if P == P_FIXTURE:
        d = load("prune.npz")
        raw, imp = torch.tensor(d["scaling"]), torch.tensor(d["imp"])
    else:
        rng = np.random.default_rng(P)
        raw = torch.tensor((np.log(0.02) + rng.normal(scale=0.5, size=(P, 3))).astype(np.float32))
        imp = torch.tensor(rng.gamma(2.0, 30.0, size=P).astype(np.float32))
    raw, imp = raw.clone(), imp.clone()
    if special == "imp_zero_half":
        imp[::2] = 0.0
    return raw, imp


@functools.lru_cache(maxsize=None)
def reference(P, activated, v_pow, percent, special=None):
    """-> (scaling as the call gets it, imp, v32, mask32, v64, e_ref, k): the reference's chain on the CPU in fp32 and float64."""
    raw, imp = filter_inputs(P, special)
    scaling = torch.exp(raw) if activated else raw
    if special == "zero_scale":                              # three rows with an exactly zero activated scale: volume 0, v 0
        assert activated
        scaling = scaling.clone()
        scaling[[3, P // 2, P - 1], [0, 1, 2]] = 0.0
    if special == "zero_kth":                                # a fifth of the volumes are 0, so the 90 % volume is: v is inf or NaN
        assert activated
        scaling = scaling.clone()
        scaling[::5, 1] = 0.0
    v32, mask32 = filter_ref.filtering(scaling, activated, imp, v_pow, percent)
    v64, _ = filter_ref.filtering(scaling, activated, imp, v_pow, percent, torch.float64)
    return scaling, imp, v32, mask32, v64, filter_ref.rel_err(v32, v64), filter_ref.threshold_rank(P, percent)


def threshold_is_clear(v64, k, bar):
    """No float64 v other than the threshold element lies within BAND x bar (relative) of the threshold. Entries EQUAL to it are
    allowed where the threshold is 0 or not finite: a zero importance or volume, an inf or a NaN comes out of every evaluation of
    the formulas as the same value, whatever its rounding."""
    v = v64.numpy()
    thr = np.sort(v)[k]                                      # numpy sorts NaN last, as torch does
    if not np.isfinite(thr) or thr == 0:
        with np.errstate(invalid="ignore"):
            near = np.isfinite(v) & (v != thr) & (np.abs(v - thr) <= BAND * bar * abs(thr))
        return not near.any()
    return int((np.abs(v - thr) <= BAND * bar * abs(thr)).sum()) == 1


def run_filter(P, activated, v_pow, percent, special=None):
    scaling, imp, v32, mask32, v64, e_ref, k = reference(P, activated, v_pow, percent, special)
    res = F.importance_filter(scaling.to(DEV), imp.to(DEV), v_pow, percent, activated=activated)
    assert res.mask.dtype == torch.bool and res.mask.shape == (P,) and res.v_list.shape == (P,) and res.n_pruned.dim() == 0
    assert res.n_pruned.dtype == torch.int32 and res.n_pruned.device == DEV
    # B1: exact against the call's own v_list
    own = F.importance_prune_mask(res.v_list, percent)
    v_host, mask_host = res.v_list.cpu(), res.mask.cpu()
    assert torch.equal(res.mask, own), "mask != importance_prune_mask(v_list)"
    assert torch.equal(mask_host, filter_ref.prune_mask(v_host, percent)), "mask != torch.sort of v_list on the CPU"
    assert int(res.n_pruned) == int(mask_host.sum())
    # B2: v_list against float64
    e_fused = filter_ref.rel_err(v_host, v64)
    print(f"P {P} activated {activated} v_pow {v_pow} percent {percent} {special or ''}: e_ref {e_ref:.3e}, fused {e_fused:.3e}, "
          f"pruned {int(res.n_pruned)}")
    assert e_fused <= 4 * e_ref, f"v_list is {e_fused:.3e} from float64, the reference's fp32 chain {e_ref:.3e}"
    # B3: the mask against the reference's
    assert threshold_is_clear(v64, k, 4 * e_ref), "precondition: another v sits within 64 x the bar of the threshold"
    assert torch.equal(mask_host, mask32), f"{int((mask_host != mask32).sum())} mask entries differ from the reference's"
    return res, mask_host


@pytest.mark.parametrize("percent", [0, 0.4, 1])
@pytest.mark.parametrize("v_pow", [0.1, 1.0])
@pytest.mark.parametrize("activated", [False, True])
@pytest.mark.parametrize("P", [P_FIXTURE, P_BLOCK])
def test_importance_filter(built_lib, P, activated, v_pow, percent):
    res, mask = run_filter(P, activated, v_pow, percent)
    assert int(mask.sum()) == filter_ref.threshold_rank(P, percent) + 1          # no ties in these inputs
    if P == P_FIXTURE and v_pow == 0.1 and percent == 0.4:
        d = load("prune.npz")
        assert float(d["v_pow"]) == v_pow and float(d["percent"]) == percent
        assert np.array_equal(mask.numpy(), d["mask"])
        np.testing.assert_allclose(res.v_list.cpu().numpy(), d["v_list"], rtol=1e-6)
        v = F.calculate_v_imp_score(torch.exp(filter_inputs(P)[0]).to(DEV), filter_inputs(P)[1].to(DEV), v_pow)
        if activated:
            assert torch.equal(v, res.v_list)


def test_importance_filter_ties_at_the_threshold_are_all_pruned(built_lib):
    res, mask = run_filter(P_BLOCK, True, 0.1, 0, "zero_scale")
    assert mask.nonzero().reshape(-1).tolist() == [3, P_BLOCK // 2, P_BLOCK - 1] and not res.v_list[mask.to(DEV)].any()
    res, mask = run_filter(P_BLOCK, False, 1.0, 0.4, "imp_zero_half")
    assert torch.equal(mask, filter_inputs(P_BLOCK, "imp_zero_half")[1] == 0) and int(res.n_pruned) == (P_BLOCK + 1) // 2


def test_importance_filter_with_a_zero_kth(built_lib):
    """A zero 90 % volume: v is inf (x / 0), or NaN (0 / 0, inf * 0) -- what the formulas give. A NaN is never pruned."""
    res, mask = run_filter(P_BLOCK, True, 0.1, 0.4, "zero_kth")
    v = res.v_list.cpu()
    assert bool(torch.isnan(v[::5]).all()) and bool(torch.isinf(v[1::5]).all()) and not mask[::5].any()


# ---- C: no host read -----------------------------------------------------------------------------------------------------------

def test_importance_filter_replays_from_a_captured_graph(built_lib):
    P = P_BLOCK
    raw, imp = filter_inputs(P)
    scaling_d, imp_d = raw.to(DEV), imp.to(DEV)
    F.importance_filter(scaling_d, imp_d, 0.1, 0.4, activated=False)                       # loads the library outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = F.importance_filter(scaling_d, imp_d, 0.1, 0.4, activated=False)
    gen = torch.Generator().manual_seed(5)
    for _ in range(2):
        scaling_d.copy_((raw + 0.3 * torch.randn(raw.shape, generator=gen)).to(DEV))
        imp_d.copy_((imp * torch.rand(imp.shape, generator=gen)).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        eager = F.importance_filter(scaling_d, imp_d, 0.1, 0.4, activated=False)
        assert torch.equal(captured.mask, eager.mask) and int(captured.n_pruned) == int(eager.n_pruned) == int(eager.mask.sum())
        assert captured.v_list.cpu().numpy().tobytes() == eager.v_list.cpu().numpy().tobytes()
        assert int(eager.n_pruned) >= filter_ref.threshold_rank(P, 0.4) + 1


# ---- D: end to end -------------------------------------------------------------------------------------------------------------

def test_gaussian_filtering_on_a_model_against_the_torch_chain(built_lib):
    from tests.test_model_gpu import ATTR, NAMES, cloud, training_args
    P, v_pow, prune_decay, prune_percent = 900, 0.1, 0.8, 0.5
    args = training_args()
    gm = M.GaussianModel({"sh_degree": 3}, "scene")
    gm.create_from_pcd(cloud(P, 5), True, 1)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        gm._scaling.add_((0.8 * torch.rand(gm._scaling.shape, generator=gen) - 0.4).to(DEV))
        gm._rotation.copy_(torch.randn(gm._rotation.shape, generator=gen).to(DEV))
        gm._opacity.copy_(torch.randn(gm._opacity.shape, generator=gen).to(DEV))
    gm.training_setup(args)
    for it in (1, 2):                                        # two Adam steps: non-zero moments
        for n in NAMES:
            p = getattr(gm, ATTR[n])
            p.grad = (1e-3 * torch.randn(p.shape, generator=gen)).to(DEV)
        gm.update_learning_rate(it)
        gm.optimizer.step()
        gm.optimizer.zero_grad(set_to_none=True)
    # the torch-op twin of tests/model_ref.py, in the same state
    ref = model_ref.TorchModel({"sh_degree": 3}, "scene")
    for n in NAMES:
        setattr(ref, ATTR[n], torch.nn.Parameter(getattr(gm, ATTR[n]).detach().clone()))
    ref._background = torch.nn.Parameter(gm._background.detach().clone())
    ref.spatial_lr_scale = gm.spatial_lr_scale
    ref.stats = DensifyStats(P, DEV)
    ref.training_setup(args)
    assert isinstance(ref.optimizer, torch.optim.Adam)
    for n in NAMES:
        st = gm.optimizer.state[getattr(gm, ATTR[n])]
        assert st["exp_avg"].any() and st["exp_avg_sq"].any()
        ref.optimizer.state[getattr(ref, ATTR[n])] = dict(step=torch.tensor(2.0), exp_avg=st["exp_avg"].clone(),
                                                          exp_avg_sq=st["exp_avg_sq"].clone())
    cams = synth.sphere_cameras(6, 96, 96)
    bg = torch.ones(3, device=DEV)
    with torch.no_grad():
        direct = views.importance_scores([settings_for(c, [1, 1, 1], gm.active_sh_degree, DEV, score_flag=True) for c in cams],
                                         gm.get_xyz, gm.get_opacity, shs=gm.get_features, scales=gm.get_scaling,
                                         rotations=gm.get_rotation)
        scaling_before = gm.get_scaling.clone()
    mask, scores = F.gaussian_filtering(gm, cams, bg, v_pow, prune_decay, prune_percent)
    assert torch.equal(scores, direct) and float(scores.max()) > 0
    percent = prune_decay * prune_percent
    # the decision is not a matter of rounding: float64 on the CPU sees no other row near the threshold
    v32 = filter_ref.v_imp_score(scaling_before, scores, v_pow)
    v64 = filter_ref.v_imp_score(scaling_before, scores, v_pow, torch.float64)
    assert threshold_is_clear(v64, filter_ref.threshold_rank(P, percent), 4 * filter_ref.rel_err(v32, v64))
    with torch.no_grad():                                    # the reference's chain in torch ops on the device, the same score sum
        volume = torch.prod(ref.get_scaling, dim=1)
        kth = torch.sort(volume, descending=True)[0][int(len(volume) * 0.9)]
        ref.prune_gaussians(percent, torch.pow(volume / kth, v_pow) * scores)
    kept = int((~mask).sum())
    print(f"rows {P} -> {kept}")
    assert 0 < kept <= P - (filter_ref.threshold_rank(P, percent) + 1) and gm._xyz.shape[0] == ref._xyz.shape[0] == kept
    for n, group, group_ref in zip(NAMES, gm.optimizer.param_groups, ref.optimizer.param_groups):
        p, q = getattr(gm, ATTR[n]), getattr(ref, ATTR[n])
        assert group["params"][0] is p and group_ref["params"][0] is q
        assert torch.equal(p, q), f"{n}: surviving rows or their order differ"
        for m in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(gm.optimizer.state[p][m], ref.optimizer.state[q][m]), f"{m} of {n}"
    for a, b in zip(gm.stats.tensors(), ref.stats.tensors()):
        assert torch.equal(a, b)
