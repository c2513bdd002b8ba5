"""distCUDA2 (csrc/knn.hip) at the edges tests/test_knn.py does not reach: point counts around n = 2 k^3, where the host
(double cbrt) and the device (float cbrtf) may size the grid differently; points on cell faces, where the early exit
`b2 <= reach^2` is an equality; coordinates far from the origin and of mixed sign (ordered-int bounding box,
`(v - lo) * inv_cell`); zero-extent axes; a grid collapsed by one outlier; the sort's tile edges; dirty scratch; and the
forms a caller may hand the points over in. Reference: oracle.knn_oracle (fp32 brute force up to 2048 points, float64
cKDTree above), at test_knn.py's bar rtol=2e-5, atol=1e-12 for EVERY entry: the fp32 brute oracle is within 1.9e-7
relative of float64 on these clouds, so the bar leaves a correct kernel 100x room and a missed neighbour none.

Out of scope: the R = 256 cap of the grid needs n >= 2 * 256^3 = 33.5 M points, too large for a unit test and for the CPU
oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2e-5, 1e-12
DEV = "cuda:0"


def _sort_tile() -> int:
    """kSortThreads * GSR_OS_ITEMS_SMALL: the keys one workgroup of the one-sweep sort takes."""
    src = open(os.path.join(ROOT, "dreamscene_amd", "csrc", "radix_sort.h")).read()
    threads = int(re.search(r"constexpr\s+int\s+kSortThreads\s*=\s*(\d+)\s*;", src).group(1))
    items = int(re.search(r"#define\s+GSR_OS_ITEMS_SMALL\s+(\d+)", src).group(1))
    return threads * items


def _sizes():
    s = [2, 3, 4, 5]
    for k in (3, 4, 5, 6, 10, 20, 40):
        s += [2 * k ** 3 + d for d in (-1, 0, 1)]
    s += [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16385]
    t = _sort_tile()
    s += [t - 1, t, t + 1]
    return sorted(set(s))


SIZES = _sizes()


def _normal(n: int) -> np.ndarray:
    return np.random.default_rng(1000 + n).normal(size=(n, 3)).astype(np.float32)


def _hip(pts) -> np.ndarray:
    from simple_knn._C import distCUDA2
    t = pts if isinstance(pts, torch.Tensor) else torch.tensor(pts, device=DEV)
    return distCUDA2(t).cpu().numpy()


def _check(got: np.ndarray, ref: np.ndarray, name: str):
    assert got.shape == ref.shape and got.dtype == np.float32, name
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), name
    assert np.array_equal(got[~fin], ref[~fin]), name            # inf where neighbours are missing, never nan
    np.testing.assert_allclose(got[fin], ref[fin], rtol=RTOL, atol=ATOL, err_msg=name)


# ------------------------------------------------------------------------------------------------ 1. sizes

@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_knn_sizes(built_lib, n):
    from oracle import knn_oracle as K
    pts = _normal(n)
    ref = K.mean_dist2(pts)
    if n == 2:
        assert np.all(np.isinf(ref))                     # one neighbour + two FLT_MAX stand-ins overflow
    if n == 3:
        assert np.all(np.isfinite(ref)) and np.all(ref > 1e38)
    _check(_hip(pts), ref, f"n={n}")


# ------------------------------------------------------------------------------------------------ 2. geometry

def _lattice(m: int) -> np.ndarray:
    g = np.arange(m, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def _extremes_cloud():
    """3000 points in the unit ball region and six more, each the single extreme of one axis direction."""
    rng = np.random.default_rng(77)
    p = rng.uniform(-1, 1, size=(3000, 3)).astype(np.float32)
    ext = rng.uniform(-0.5, 0.5, size=(6, 3)).astype(np.float32)
    for a in range(3):
        ext[2 * a, a] = -1.5 - 0.25 * a
        ext[2 * a + 1, a] = 1.75 + 0.25 * a
    where = np.array([0, 511, 1024, 1777, 2500, 3005])            # scattered through the array, first and last included
    p = np.insert(p, where - np.arange(6), ext, axis=0)
    return p, where, ext


def _geometry():
    rng = np.random.default_rng(11)
    f = np.float32
    lat = _lattice(16)
    yield "lattice-16", lat
    yield "lattice-16-x1.25", lat * f(1.25)
    yield "lattice-12-doubled", np.concatenate([_lattice(12), _lattice(12)])
    yield "far-from-origin", (rng.normal(size=(5000, 3)) * 1e-2 + np.array([1e3, -2e3, 5e2])).astype(f)
    tiny = rng.uniform(-1e-3, 1e-3, size=(4000, 3)).astype(f)
    tiny[::400, 0] = f(0.0)
    tiny[7::400, 1] = f(-0.0)
    tiny[13::400, 2] = f(0.0)
    tiny[13::800, 0] = f(-0.0)
    yield "tiny-signed-zeros", tiny
    plane = rng.uniform(-2, 2, size=(4000, 3)).astype(f)
    plane[:, 2] = f(0.25)
    yield "plane-z", plane
    line = np.zeros((3000, 3), f)
    line[:, 1] = rng.uniform(-50, 50, size=3000).astype(f)
    line[:, 0] = f(-3.0)
    yield "line-y", line
    yield "anisotropic", (rng.normal(size=(6000, 3)) * np.array([100.0, 1.0, 0.01])).astype(f)
    cl = (rng.normal(size=(20000, 3)) * 1e-3).astype(f)
    yield "cluster-plus-outlier", np.concatenate([cl, np.array([[1e3, 1e3, 1e3]], f)])
    dense = (rng.normal(size=(8000, 3)) * 1e-2).astype(f)
    sparse = (rng.normal(size=(300, 3)) * 5.0 + np.array([200.0, -100.0, 50.0])).astype(f)
    yield "two-densities", np.concatenate([dense, sparse])
    yield "distinct-extremes", _extremes_cloud()[0]


GEOMETRY = dict(_geometry())


def test_geometry_fixtures_are_what_they_claim():
    """The clouds have the properties the GPU cases rely on (no GPU needed to know that)."""
    lat = GEOMETRY["lattice-16"]
    n = lat.shape[0]
    R = int(np.cbrt(0.5 * n))
    assert n == 4096 and R == 12 and 15.0 / R == 1.25             # cell 1.25: the lattice planes 0, 5, 10, 15 are cell faces
    assert GEOMETRY["lattice-12-doubled"].shape[0] == 2 * 12 ** 3
    tiny = GEOMETRY["tiny-signed-zeros"]
    assert np.signbit(tiny[tiny == 0]).any() and (~np.signbit(tiny[tiny == 0])).any()
    assert np.ptp(GEOMETRY["plane-z"][:, 2]) == 0 and not np.ptp(GEOMETRY["line-y"][:, [0, 2]], axis=0).any()
    out = GEOMETRY["cluster-plus-outlier"]
    assert out.shape[0] == 20001
    cell = np.ptp(out, axis=0).max() / int(np.cbrt(0.5 * out.shape[0]))
    assert np.ptp(out[:-1], axis=0).max() < cell                  # the whole cluster shares one cell
    p, where, ext = _extremes_cloud()
    assert np.array_equal(p[where], ext) and len(set(where.tolist())) == 6
    for a in range(3):
        assert int(p[:, a].argmin()) == where[2 * a] and int(p[:, a].argmax()) == where[2 * a + 1]
    for name, pts in GEOMETRY.items():
        assert pts.dtype == np.float32 and 2000 <= pts.shape[0] <= 20001, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_knn_geometry(built_lib, name):
    from oracle import knn_oracle as K
    pts = GEOMETRY[name]
    ref = K.mean_dist2(pts)
    got = _hip(pts)
    _check(got, ref, name)
    if name.startswith("lattice-16"):
        s = np.float32(1.25 if name.endswith("1.25") else 1.0)
        np.testing.assert_allclose(got, np.full(4096, s * s, np.float32), rtol=2e-7)   # three axis neighbours at one spacing
    if name == "lattice-12-doubled":
        d2 = np.float32(2.0 / 3.0)                                       # the twin at 0, then two axis neighbours at 1
        np.testing.assert_allclose(got, np.full(got.shape, d2), rtol=2e-7)
    if name == "cluster-plus-outlier":
        p64 = pts.astype(np.float64)
        d = np.sort(((p64[:-1] - p64[-1]) ** 2).sum(1))[:3].mean()
        np.testing.assert_allclose(got[-1], d, rtol=RTOL)
    if name == "distinct-extremes":
        _, where, _ = _extremes_cloud()
        p64 = pts.astype(np.float64)
        for i in where:
            d2 = ((p64 - p64[i]) ** 2).sum(1)
            d2[i] = np.inf
            np.testing.assert_allclose(got[i], np.sort(d2)[:3].mean(), rtol=RTOL, err_msg=f"extreme point {i}")


# ------------------------------------------------------------------------------------------------ 3. caller forms

@pytest.mark.gpu
def test_knn_caller_forms_bit_for_bit(built_lib):
    from oracle import knn_oracle as K
    from simple_knn._C import distCUDA2
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(3001, 3)).astype(np.float32)
    base_t = torch.tensor(pts, device=DEV)
    base = distCUDA2(base_t)
    _check(base.cpu().numpy(), K.mean_dist2(pts), "contiguous")

    wide = torch.full((3001, 4), 7.0, device=DEV)
    wide[:, :3] = base_t
    assert not wide[:, :3].is_contiguous()
    assert torch.equal(distCUDA2(wide[:, :3]), base)

    tr = base_t.t().contiguous()                                          # [3, N] storage
    assert not tr.t().is_contiguous()
    assert torch.equal(distCUDA2(tr.t()), base)

    rg = base_t.clone().requires_grad_(True)
    out = distCUDA2(rg)
    assert torch.equal(out, base) and not out.requires_grad

    assert torch.equal(distCUDA2(base_t), base)                           # determinism: equal bits on a second call

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = distCUDA2(base_t)
    side.synchronize()
    assert torch.equal(on_side, base)
    torch.cuda.current_stream().wait_stream(side)

    # converting inputs: the wrapper rounds to fp32 / widens from fp16; the oracle sees the converted values
    p64 = rng.normal(size=(2500, 3))
    got = distCUDA2(torch.tensor(p64, dtype=torch.float64, device=DEV))
    assert got.dtype == torch.float32
    _check(got.cpu().numpy(), K.mean_dist2(p64.astype(np.float32)), "float64")
    assert torch.equal(got, distCUDA2(torch.tensor(p64.astype(np.float32), device=DEV)))
    p16 = (rng.normal(size=(2500, 3)) * 4).astype(np.float16)             # coarse values: many exact ties and duplicates
    got = distCUDA2(torch.tensor(p16, device=DEV))
    assert got.dtype == torch.float32
    _check(got.cpu().numpy(), K.mean_dist2(p16.astype(np.float32)), "float16")
    assert torch.equal(got, distCUDA2(torch.tensor(p16.astype(np.float32), device=DEV)))


@pytest.mark.gpu
def test_knn_dirty_scratch(built_lib):
    """The scratch comes from the caching allocator: after a large call was freed, a small one gets its blocks back with
    the large call's keys, ranges and sort state still in them."""
    from simple_knn._C import distCUDA2
    small = [torch.tensor(_normal(54), device=DEV), torch.tensor(_normal(5000), device=DEV)]
    first = [distCUDA2(t).clone() for t in small]
    big = torch.tensor(_normal(128000), device=DEV)
    out = distCUDA2(big)
    lib = built_lib
    junk = torch.full((int(lib.gsr_knn_scratch_bytes(128000)),), 0xFF, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    del big, out, junk
    for t, f in zip(small, first):
        assert torch.equal(distCUDA2(t), f)
        assert torch.equal(distCUDA2(t), f)


# ------------------------------------------------------------------------------------------------ 4. without a GPU

GSR_OK, GSR_EINVAL, GSR_ESCRATCH = 0, -1, -4


def test_knn_refuses_bad_arguments_before_any_device_call(built_lib):
    lib = built_lib
    fake = ctypes.c_void_p(0x1000)                     # never dereferenced: every call below returns during validation
    need = int(lib.gsr_knn_scratch_bytes(100))
    assert lib.gsr_knn_mean_dist2(fake, -1, fake, fake, need, None) == GSR_EINVAL
    assert lib.gsr_knn_mean_dist2(fake, -2 ** 31, fake, fake, need, None) == GSR_EINVAL
    assert lib.gsr_knn_mean_dist2(None, 100, fake, fake, need, None) == GSR_EINVAL
    assert lib.gsr_knn_mean_dist2(fake, 100, None, fake, need, None) == GSR_EINVAL
    assert lib.gsr_knn_mean_dist2(fake, 100, fake, None, need, None) == GSR_ESCRATCH
    assert lib.gsr_knn_mean_dist2(fake, 100, fake, fake, need - 1, None) == GSR_ESCRATCH
    assert lib.gsr_knn_mean_dist2(fake, 100, fake, fake, 0, None) == GSR_ESCRATCH
    assert lib.gsr_knn_mean_dist2(None, 0, None, None, 0, None) == GSR_OK


def test_knn_scratch_bytes_is_monotone(built_lib):
    lib = built_lib
    sizes = [0, 1] + SIZES + [10 ** 6, 2 * 100 ** 3 - 1, 2 * 100 ** 3, 2 * 256 ** 3, 2 ** 31 - 1]
    b = [int(lib.gsr_knn_scratch_bytes(n)) for n in sizes]
    assert all(x > 0 for x in b)
    assert all(x <= y for x, y in zip(b, b[1:])), list(zip(sizes, b))
    assert int(lib.gsr_knn_scratch_bytes(-5)) == b[1]          # n <= 0 sizes as one point, never as a huge unsigned


def test_knn_scratch_covers_the_range_cells_for_both_roundings(built_lib):
    """The host sizes and clears (R + 1)^3 cells with R from a double cbrt; the device indexes R^3 cells with R from a float
    cbrtf. Whichever way either rounds at n = 2 k^3, the (start, end) pairs of (R + 1)^3 cells fit behind the other regions
    of the scratch (the layout of gsr_knn_mean_dist2: four n-word arrays, the sort's state, 256 totals, the bounding box)."""
    lib = built_lib
    src = open(os.path.join(ROOT, "dreamscene_amd", "csrc", "radix_sort.h")).read()
    items_legacy = int(re.search(r"constexpr\s+int\s+kItemsSmall\s*=\s*(\d+)\s*;", src).group(1))
    passes = int(re.search(r"constexpr\s+int\s+kOsMaxPasses\s*=\s*(\d+)\s*;", src).group(1))
    radix, threads, tile = 256, _sort_tile() // int(re.search(r"#define\s+GSR_OS_ITEMS_SMALL\s+(\d+)", src).group(1)), _sort_tile()
    a256 = lambda x: (x + 255) & ~255

    def others(n):
        legacy = radix * -(-n // (threads * items_legacy)) * 4
        one_sweep = (passes * radix + 16 + radix * -(-n // tile)) * 4
        return 4 * a256(4 * n) + a256(max(legacy, one_sweep)) + a256(256 * 4) + 256

    ns = set(SIZES)
    for k in range(1, 257):
        ns.update(2 * k ** 3 + d for d in (-1, 0, 1))
    for n in sorted(ns):
        room = int(lib.gsr_knn_scratch_bytes(n)) - others(n)
        r_double = int(np.cbrt(0.5 * float(n)))
        r_float = int(np.cbrt(np.float32(0.5) * np.float32(n)))
        for R in {max(1, min(256, r)) for r in (r_double, r_float)}:
            assert room >= 8 * min((R + 1) ** 3, 256 ** 3), (n, R, room)
