"""-m gpu: dreamscene_amd.fields on the device against the reference's own GaussianModel.extract_fields (tests/golden/fields.npz,
written by tests/golden/make_fields_golden.py on the CPU). SEMANTICS.md section 18.
  1  basic     300 rows, 16^3, 4 blocks
  2  cluster   700 rows, 600 inside one block, 18^3 in chunks of 4, 4, 4, 4, 2: a member list longer than one compaction batch
  3  gaps      relax 0: centres between chunks belong to no block, some blocks are empty; the zero set is the reference's exactly
  4  all       relax 100, one block at 8^3: every row in it
  5  wide      24^3 in 2 blocks: 1728 voxels a block, several workgroups a block
  6  filter    rows at logit -6 far outside the kept cloud: center, scale and the kept count are torch's bits
  7  many      70 001 rows at 8^3: several workgroups in bounds and prepare, and a tail; plus a row count past the bounds grid's cap
  8  20 000 rows at 32^3 in 8 blocks against the torch chain (tests/fields_ref.py) on the same GPU
  9  the same bits over two runs, the second with scratch and out full of 0xFF
 10  the model method sets center and scale and takes leaves that require grad
Bar of 1 - 8: max|ours - reference| <= 1e-5 * max|reference|, the project's standard. Measured on the CPU at these shapes: a
sequential fp32 sum in index order lies 7e-7 of the field's maximum from float64, the reference's own fp32 1.2e-7, and a one-ulp
change of every covariance entry (torch's bmm order is unspecified) moves the field by 1.4e-7.
`stretch` (log-scale noise of sigma 0.8, anisotropy to about 50) is checked against float64 at 4 * e_ref + 1e-5 * max, e_ref being
the reference's own distance from float64: there a one-ulp covariance change already moves the field by 4e-6 (the precedent is
tests/test_trajectory_gpu.py).
Every fixture keeps its normalised centres 1e-5 from the chunk gates and its opacities 1e-6 from 0.005 (asserted here)."""
import functools

import numpy as np
import pytest
import torch

from dreamscene_amd import fields as F
from dreamscene_amd import model as M
from tests import fields_ref as FR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = 1e-5
GOLD = np.load(FR.GOLDEN)


@functools.lru_cache(maxsize=None)
def case(name):
    c = FR.load_case(name, GOLD)
    gate, opacity = FR.margins(c, c["resolution"], c["num_blocks"], c["relax_ratio"])
    assert gate >= FR.GATE_MARGIN and opacity >= FR.OPACITY_MARGIN, (name, gate, opacity)
    return c


def on_device(c):
    return [torch.tensor(c[k]).to(DEV) for k in FR.LEAVES]


def run(c, **kw):
    return F.extract_fields(*on_device(c), c["resolution"], c["num_blocks"], c["relax_ratio"], **kw)


def kept_on_host(c) -> int:
    return int((torch.sigmoid(torch.tensor(c["opacity"])) > 0.005).sum())


def check_against_golden(name):
    c = case(name)
    r = run(c)
    occ, want = r.occ.cpu(), torch.tensor(c["occ"])
    err, top = float((occ - want).abs().max()), float(want.abs().max())
    print(f"{name}: max|ours - reference| = {err:.3g} = {err / top:.3g} of the maximum {top:.4g}; kept {r.kept}")
    assert occ.shape == want.shape and occ.dtype == torch.float32 and r.occ.device == DEV
    assert r.center.device == DEV and r.center.dtype == torch.float32 and isinstance(r.scale, float)
    assert torch.equal(r.center.cpu(), torch.tensor(c["center"])), (r.center, c["center"])
    assert r.scale == float(c["scale"]), (r.scale, float(c["scale"]))
    assert r.kept == kept_on_host(c)
    assert bool(torch.isfinite(occ).all())
    assert err <= BAR * top, (err, top)
    return c, occ, want


@pytest.mark.parametrize("name", ["basic", "cluster", "all", "wide"])
def test_field_matches_the_reference(name):
    c, _, _ = check_against_golden(name)
    if name == "cluster":                          # five chunks, the last of two coordinates; one block's list exceeds a batch
        t = F.chunk_tables(c["resolution"], c["num_blocks"], c["relax_ratio"])
        assert (t.n_chunks, t.split_size) == (5, 4)
        _, _, centres, _, _, _ = FR.normalised(*[torch.tensor(c[k]) for k in ("xyz", "opacity", "scaling")])
        inside = ((centres[:, None, :] > t.lo[None, :, None]) & (centres[:, None, :] < t.hi[None, :, None]))     # [n, chunk, axis]
        members = torch.einsum("na,nb,nc->abc", *(inside[:, :, k].float() for k in range(3)))
        assert float(members.max()) > 2 * 256
    if name == "wide":
        assert (c["resolution"] // c["num_blocks"]) ** 3 > 4 * 256
    if name == "all":
        assert F.chunk_tables(c["resolution"], c["num_blocks"], c["relax_ratio"]).n_chunks == 1


def test_no_relaxation_leaves_the_reference_s_zeros():
    c, occ, want = check_against_golden("gaps")
    t = F.chunk_tables(c["resolution"], c["num_blocks"], c["relax_ratio"])
    _, _, centres, _, _, _ = FR.normalised(*[torch.tensor(c[k]) for k in ("xyz", "opacity", "scaling")])
    inside = (centres[:, None, :] > t.lo[None, :, None]) & (centres[:, None, :] < t.hi[None, :, None])
    assert not bool(inside.any(1).all())           # a centre lies between two chunks on some axis: it belongs to no block
    blocks = want.reshape(4, 4, 4, 4, 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(64, 64)
    assert bool((blocks == 0).all(1).any())        # a block nobody belongs to
    assert torch.equal(occ == 0, want == 0)
    assert int((want == 0).sum()) % 64 == 0        # and only whole blocks are zero


def test_filtered_rows_do_not_move_the_bounds():
    c, _, _ = check_against_golden("filter")
    low = torch.sigmoid(torch.tensor(c["opacity"])).reshape(-1) <= 0.005
    assert int(low.sum()) == 40
    xyz = torch.tensor(c["xyz"])
    assert float(xyz[low].abs().max()) > 2 * float(xyz[~low].abs().max())        # far outside the kept cloud


def test_many_rows():
    c, _, _ = check_against_golden("many")
    assert c["xyz"].shape[0] == 70001 and kept_on_host(c) < 70001


def test_bounds_past_the_grid_cap():
    """More rows than k_field_bounds' capped grid covers in one trip, the extreme rows among the last: center, scale and the
    kept count are torch's."""
    P = 1024 * 256 + 77
    rng = np.random.default_rng(11)
    d = FR.draw(rng, P, size=0.05)
    d["xyz"][-1], d["opacity"][-1] = (0.9, -0.8, 0.7), 3.0
    d["xyz"][-40], d["opacity"][-40] = (-0.95, 0.85, -0.75), 3.0
    d["xyz"][-2], d["opacity"][-2] = (5.0, 5.0, 5.0), -9.0                        # filtered
    _, _, _, _, center, scale = FR.normalised(*[torch.tensor(d[k]) for k in ("xyz", "opacity", "scaling")])
    r = F.extract_fields(*[torch.tensor(d[k]).to(DEV) for k in FR.LEAVES], 8, 2, 1.5)
    assert torch.equal(r.center.cpu(), center) and r.scale == scale and r.kept == kept_on_host(d)
    assert float((center - torch.tensor([-0.025, 0.025, -0.025])).abs().max()) < 1e-6        # the bounds are those late rows'
    assert bool(torch.isfinite(r.occ).all())


@functools.lru_cache(maxsize=None)
def large():
    d = FR.draw_clear_of_gates(np.random.default_rng(12), 20000, 32, 8, 1.5)
    gate, opacity = FR.margins(d, 32, 8, 1.5)
    assert gate >= FR.GATE_MARGIN and opacity >= FR.OPACITY_MARGIN, (gate, opacity)
    return d


def test_against_the_torch_chain_on_the_same_gpu():
    d = large()
    leaves = [torch.tensor(d[k]).to(DEV) for k in FR.LEAVES]
    want, center, scale, kept = FR.extract_fields(*leaves, 32, 8, 1.5)
    r = F.extract_fields(*leaves, 32, 8, 1.5)
    err, top = float((r.occ - want).abs().max()), float(want.abs().max())
    print(f"20 000 rows at 32^3: max|ours - torch chain| = {err:.3g} = {err / top:.3g} of the maximum {top:.4g}")
    assert torch.equal(r.center, center) and r.scale == scale and r.kept == kept
    assert err <= BAR * top, (err, top)


def test_stretched_gaussians_against_float64():
    c = case("stretch")
    exact = FR.extract_fields(*[torch.tensor(c[k]) for k in FR.LEAVES], c["resolution"], c["num_blocks"], c["relax_ratio"],
                              dtype=torch.float64)[0]
    occ, ref = run(c).occ.cpu().double(), torch.tensor(c["occ"]).double()
    e_ref, e_ours, top = float((ref - exact).abs().max()), float((occ - exact).abs().max()), float(exact.abs().max())
    print(f"stretch: e_ours = {e_ours:.3g}, e_ref = {e_ref:.3g}, ratio {e_ours / e_ref:.3g}; of the maximum: "
          f"{e_ours / top:.3g} and {e_ref / top:.3g}")
    assert e_ours <= 4 * e_ref + BAR * top, (e_ours, e_ref, top)


def test_same_bits_whatever_the_buffers_held():
    c = case("cluster")
    first = run(c)
    need = F.scratch_bytes(c["xyz"].shape[0])
    scratch = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((c["resolution"],) * 3, float("nan"), device=DEV)
    out.view(torch.int32).fill_(-1)
    second = run(c, out=out, scratch=scratch)
    assert second.occ is out and bool(torch.isfinite(out).all())
    assert torch.equal(first.occ.view(torch.int32), out.view(torch.int32))
    assert torch.equal(first.center, second.center) and first.scale == second.scale and first.kept == second.kept
    assert bool((scratch[need:] == 0xFF).all())    # nothing past what scratch_bytes asks for
    with pytest.raises(ValueError):
        run(c, scratch=scratch[:need - 16])


def test_refusals_on_the_device():
    c = case("basic")
    xyz, opacity, scaling, rotation = on_device(c)
    with pytest.raises(ValueError):                # no row passes the opacity threshold
        F.extract_fields(xyz, torch.full_like(opacity, -6.0), scaling, rotation, 16, 4, 1.5)
    with pytest.raises(ZeroDivisionError):         # one row: zero extent
        F.extract_fields(xyz[:1], opacity[:1] * 0 + 2, scaling[:1], rotation[:1], 16, 4, 1.5)
    with pytest.raises(ValueError):
        F.extract_fields(xyz, opacity, scaling, rotation.double(), 16, 4, 1.5)


def test_model_method():
    c = case("basic")
    gm = M.GaussianModel({"sh_degree": 0}, "scene")
    gm._xyz, gm._opacity, gm._scaling, gm._rotation = (torch.nn.Parameter(t.requires_grad_(True)) for t in on_device(c))
    occ = gm.extract_fields(c["resolution"], c["num_blocks"], c["relax_ratio"])
    want = torch.tensor(c["occ"])
    assert isinstance(occ, torch.Tensor) and not occ.requires_grad and occ.device == DEV
    assert float((occ.cpu() - want).abs().max()) <= BAR * float(want.max())
    assert gm.center.device == DEV and gm.center.dtype == torch.float32 and gm.center.shape == (3,)
    assert torch.equal(gm.center.cpu(), torch.tensor(c["center"]))
    assert isinstance(gm.scale, float) and gm.scale == float(c["scale"])
    assert all(t.requires_grad and t.grad is None for t in (gm._xyz, gm._opacity, gm._scaling, gm._rotation))
