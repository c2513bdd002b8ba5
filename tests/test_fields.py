"""Occupancy field extraction without a GPU (dreamscene_amd/fields.py, SEMANTICS.md section 18): the torch restatement
(tests/fields_ref.py) against the reference's own method (tests/golden/fields.npz), the host-side chunk tables, every refusal, the
model method's surface, and the C entry points' argument checks, which come before any HIP call."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from dreamscene_amd import fields as F
from dreamscene_amd import model as M
from dreamscene_amd._lib import GsrError
from tests import fields_ref as FR

GOLD = np.load(FR.GOLDEN)
MODEL_GOLD = np.load(os.path.join(os.path.dirname(FR.GOLDEN), "model.npz"))
CASES = ("basic", "cluster", "gaps", "all", "wide", "filter", "many", "stretch")
GSR_EINVAL, GSR_ESCRATCH = -1, -4


def leaves_of(c, dtype=torch.float32):
    return [torch.tensor(c[k]) for k in FR.LEAVES]


def test_fixture_is_complete_and_small():
    assert tuple(sorted(CASES)) == tuple(GOLD["cases"])
    assert os.path.getsize(FR.GOLDEN) < 300 * 1024
    assert FR.load_case("many", GOLD)["xyz"].shape == (70001, 3)
    assert FR.load_case("cluster", GOLD)["occ"].shape == (18, 18, 18)


@pytest.mark.parametrize("name", CASES)
def test_fixtures_keep_clear_of_the_gates_and_of_the_opacity_threshold(name):
    c = FR.load_case(name, GOLD)
    gate, opacity = FR.margins(c, c["resolution"], c["num_blocks"], c["relax_ratio"])
    print(f"{name}: nearest gate {gate:.3g}, nearest opacity {opacity:.3g}")
    assert gate >= FR.GATE_MARGIN and opacity >= FR.OPACITY_MARGIN


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    c = FR.load_case(name, GOLD)
    occ, center, scale, kept = FR.extract_fields(*leaves_of(c), c["resolution"], c["num_blocks"], c["relax_ratio"])
    assert torch.equal(center, torch.tensor(c["center"])) and scale == float(c["scale"])
    assert kept == int((torch.sigmoid(torch.tensor(c["opacity"])) > 0.005).sum())
    assert torch.equal(occ, torch.tensor(c["occ"])), float((occ - torch.tensor(c["occ"])).abs().max())


def test_float64_restatement_is_close_to_the_reference():
    c = FR.load_case("basic", GOLD)
    occ, center, scale, _ = FR.extract_fields(*leaves_of(c), c["resolution"], c["num_blocks"], c["relax_ratio"],
                                              dtype=torch.float64)
    assert occ.dtype == torch.float64 and center.dtype == torch.float64
    err = float((occ - torch.tensor(c["occ"]).double()).abs().max()) / float(occ.max())
    print(f"the reference's fp32 is {err:.3g} of the maximum from float64")
    assert err < 2e-6


@pytest.mark.parametrize("resolution,num_blocks,relax", [(16, 4, 1.5), (128, 16, 1.5), (8, 1, 100.0), (16, 4, 0.0)])
def test_chunk_tables_divisible(resolution, num_blocks, relax):
    t = F.chunk_tables(resolution, num_blocks, relax)
    chunks, reach = FR.gates(resolution, num_blocks, relax)
    assert t.split_size == resolution // num_blocks and t.n_chunks == num_blocks == len(chunks)
    assert torch.equal(t.coords, torch.linspace(-1, 1, resolution)) and t.coords.dtype == torch.float32
    for k, chunk in enumerate(chunks):
        assert len(chunk) == t.split_size
        assert torch.equal(t.lo[k], chunk.amin() - reach) and torch.equal(t.hi[k], chunk.amax() + reach)
    assert t.lo.dtype == t.hi.dtype == torch.float32 and t.lo.device.type == "cpu"
    assert bool((t.lo[1:] >= t.lo[:-1]).all()) and bool((t.hi[1:] >= t.hi[:-1]).all())


def test_chunk_tables_ragged():
    """18 coordinates in chunks of 18 // 4 = 4: five chunks, the last of two."""
    t = F.chunk_tables(18, 4, 1.5)
    coords = torch.linspace(-1, 1, 18)
    assert (t.split_size, t.n_chunks) == (4, 5)
    reach = torch.tensor(0.5 * 1.5)
    assert torch.equal(t.lo, coords[[0, 4, 8, 12, 16]] - reach)
    assert torch.equal(t.hi, coords[[3, 7, 11, 15, 17]] + reach)
    # with no relaxation a centre between two chunks is inside neither
    t0 = F.chunk_tables(18, 4, 0.0)
    between = (coords[3] + coords[4]) / 2
    assert not bool(((t0.lo < between) & (between < t0.hi)).any())
    # 6 coordinates in chunks of 6 // 4 = 1: six chunks of one coordinate, more than num_blocks
    t1 = F.chunk_tables(6, 4, 1.0)
    assert (t1.split_size, t1.n_chunks) == (1, 6) and torch.equal(t1.hi - t1.lo, torch.full((6,), 1.0))


def test_refusals_of_the_arguments():
    with pytest.raises(ValueError):
        F.chunk_tables(10, 3, 1.5)                 # 10 % (2 / 3) != 0
    assert 7 % (2 / 4) == 0
    F.chunk_tables(7, 4, 1.5)                      # ... the literal test lets 7 // 4 = 1 through, as the reference does
    with pytest.raises(ValueError):
        F.chunk_tables(2, 4, 1.5)                  # 2 % 0.5 == 0, but 2 // 4 < 1
    with pytest.raises(ValueError):
        F.chunk_tables(512, 256, 1.5)              # 256 chunks do not fit the membership word's 8 bits
    one = torch.tensor([1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        F.normalisation(one, one + 1, 0)           # no kept row
    with pytest.raises(ZeroDivisionError):
        F.normalisation(one, one.clone(), 1)       # one kept row: zero extent
    center, scale = F.normalisation(one, one + torch.tensor([1.0, 4.0, 2.0]), 5)
    assert torch.equal(center, torch.tensor([1.5, 4.0, 4.0])) and scale == 1.8 / 4.0 and isinstance(scale, float)
    with pytest.raises(ValueError):
        F.normalisation(one, one * float("inf"), 2)


def test_host_tensors_are_refused():
    c = FR.load_case("basic", GOLD)
    with pytest.raises(GsrError):
        F.extract_fields(*leaves_of(c), 16, 4, 1.5)
    with pytest.raises(ValueError):                # the argument checks come first
        F.extract_fields(*leaves_of(c), 10, 3, 1.5)
    with pytest.raises(ValueError):
        F.extract_fields(torch.zeros(0, 3), torch.zeros(0, 1), torch.zeros(0, 3), torch.zeros(0, 4), 16, 4)

    class HostModel(M.GaussianModel):
        device = "cpu"
    gm = HostModel({"sh_degree": 0}, "scene")
    gm._xyz, gm._opacity, gm._scaling, gm._rotation = (torch.nn.Parameter(t) for t in leaves_of(c))
    with pytest.raises(GsrError):
        gm.extract_fields(16, 4, 1.5)
    assert not hasattr(gm, "center")


def test_model_method_has_the_reference_s_signature():
    ref = dict(s.split(":", 1) for s in MODEL_GOLD["surface/params"])
    assert "extract_fields" in set(MODEL_GOLD["surface/names"])
    member = inspect.getattr_static(M.GaussianModel, "extract_fields", None)
    assert inspect.isfunction(member)
    sig = inspect.signature(member)
    assert [p.name for p in list(sig.parameters.values())[1:]] == ref["extract_fields"].split(",")
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    assert [sig.parameters[n].default for n in ("resolution", "num_blocks", "relax_ratio")] == [128, 16, 1.5]


def test_c_entry_points_check_their_arguments_before_any_hip_call(built_lib):
    """Host memory and a made-up stream: a call that got past its checks could not return quietly."""
    lib = built_lib
    P, R, split, n = 100, 16, 4, 4
    assert lib.gsr_fields_scratch_bytes(0) == 0 and lib.gsr_fields_scratch_bytes(-1) == 0
    need = int(lib.gsr_fields_scratch_bytes(P))
    assert need >= 32 + P * 8 + P * 40 and need % 16 == 0
    assert int(lib.gsr_fields_scratch_bytes(2 ** 31 - 1)) > 56 * (2 ** 31 - 1)
    arena = np.zeros(need + P * 44 + R * 4 + 2 * n * 4 + R ** 3 * 4 + 1024, np.uint8)
    at, ptr = (arena.ctypes.data + 255) // 256 * 256, {}
    for name, size in (("scratch", need), ("xyz", P * 12), ("opacity", P * 4), ("scaling", P * 12), ("rotation", P * 16),
                       ("coords", R * 4), ("lo", n * 4), ("hi", n * 4), ("occ", R ** 3 * 4)):
        ptr[name] = at
        at += (size + 15) // 16 * 16
    stream = ctypes.c_void_p(0x10)
    bounds = lambda **kw: lib.gsr_fields_bounds(*[{**dict(xyz=ptr["xyz"], opacity=ptr["opacity"], P=P, scratch=ptr["scratch"],
                                                          nbytes=need, stream=stream), **kw}[k]
                                                  for k in ("xyz", "opacity", "P", "scratch", "nbytes", "stream")])
    assert bounds(P=0) == GSR_EINVAL and bounds(xyz=None) == GSR_EINVAL and bounds(opacity=None) == GSR_EINVAL
    assert bounds(scratch=None) == GSR_EINVAL and bounds(scratch=ptr["scratch"] + 8) == GSR_EINVAL
    assert bounds(xyz=ptr["xyz"] + 2) == GSR_EINVAL and bounds(xyz=ptr["scratch"] + 64) == GSR_EINVAL
    assert bounds(nbytes=need - 1) == GSR_ESCRATCH
    center = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    order = ("xyz", "opacity", "scaling", "rotation", "P", "center", "scale", "coords", "lo", "hi", "resolution", "split", "n",
             "occ", "scratch", "nbytes", "stream")
    good = dict(ptr, P=P, center=center, scale=1.0, resolution=R, split=split, n=n, nbytes=need, stream=stream)
    extract = lambda **kw: lib.gsr_extract_fields(*[{**good, **kw}[k] for k in order])
    for name in ("xyz", "opacity", "scaling", "rotation", "coords", "lo", "hi", "occ", "scratch", "center"):
        assert extract(**{name: None}) == GSR_EINVAL, name
    for name in ("xyz", "rotation", "coords", "hi", "occ"):
        assert extract(**{name: ptr[name] + 1}) == GSR_EINVAL, name
        assert extract(**{name: ptr["scratch"] + 32}) == GSR_EINVAL, name          # inside the scratch
    assert extract(scratch=ptr["scratch"] + 4) == GSR_EINVAL
    assert extract(coords=ptr["occ"] + 64) == GSR_EINVAL                           # inside occ
    assert extract(P=0) == GSR_EINVAL and extract(resolution=0) == GSR_EINVAL and extract(resolution=1025) == GSR_EINVAL
    assert extract(split=0) == GSR_EINVAL and extract(split=17) == GSR_EINVAL
    assert extract(n=5) == GSR_EINVAL and extract(split=5, n=3) == GSR_EINVAL      # ceil(16 / 5) = 4
    assert extract(resolution=1024, split=4, n=256) == GSR_EINVAL                   # more than 255 chunks
    assert extract(scale=float("inf")) == GSR_EINVAL and extract(scale=float("nan")) == GSR_EINVAL
    assert extract(center=(ctypes.c_float * 3)(0.0, float("nan"), 0.0)) == GSR_EINVAL
    assert extract(nbytes=need - 1) == GSR_ESCRATCH
    assert not arena.any()                                                          # nothing was written
