"""csrc/radix_sort.h on its own: both complete sorts (form 0: radix_sort_u32, the one-sweep passes; form 1:
radix_sort_u32_legacy, histogram -> scan -> scatter, which radix_sort_u32 takes from 2^28 keys on) in the product's two
instantiations, and the two scan kernels, against the numpy references of tests/sort_ref.py. The renderer and the knn grid
only ever hand the sort depth floats, tile ids of at most 17 bits and cell ids of 24; here the keys are whatever breaks a
radix sort. Everything is an integer artefact: every comparison is array_equal.

The header is reached through tests/hip/sort_harness.hip, a C ABI with no logic of its own, built by the fixture below
into a pytest temporary directory with build.py's COMMON flags (nothing lands in the tree; not part of libgsrast.so).

Both forms sort WHOLE 8-bit digits: `bits` key bits mean ceil(bits / 8) passes, so the low 8 * ceil(bits / 8) bits of a key
decide the order (sort_ref.sort_mask) and the keys come out unmasked.

Every call works on one slab per view (the views `bstride` apart, as tools/probe/sort_phases.hip lays its slab out) that is
0xA5A5A5A5 wherever the test put nothing else -- 64 guard words and more around each of the four key / value buffers, the
survivor count of the drop form included -- with `hist` and `totals` 0xFF bytes. After the call: the sorted lists are where
the return value (and the skip flag) say, the result buffers still hold what they held from the live count to `cap`, and no
guard word, count word or rectangle changed.

To see that these tests bite, GSR_TEST_SORT_INCLUDE=<dir> puts <dir> in front of the include path, so that the harness is
built against a deliberately wrong copy of radix_sort.h kept outside the tree."""
import ctypes
import hashlib
import os
import subprocess
import time
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.sort_ref import SENTINEL, ref_scan, ref_sort, ref_weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hip", "sort_harness.hip")
DEV = "cuda:0"
GUARD = 64
FILL = 0xA5A5A5A5
TILE = 4096                      # th_tile_keys(): keys per one-sweep tile (both instantiations) and per large legacy workgroup
BIG = 40 * TILE + 123            # two and a half look-back windows of 16 tiles
FORMS = [0, 1]
SMALL = [0, 1]
VP = ctypes.c_void_p


# ------------------------------------------------------------------------------------------------------- the harness
class Harness:
    def __init__(self, path: str, build_seconds: float):
        self.path, self.build_seconds = path, build_seconds
        lib = self.lib = ctypes.CDLL(path)
        lib.th_sort.restype = ctypes.c_int
        lib.th_sort.argtypes = [ctypes.c_int, ctypes.c_int, VP, VP, VP, VP, VP, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, VP,
                                VP, VP, VP, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, VP, VP]
        lib.th_scan.restype = None
        lib.th_scan.argtypes = [ctypes.c_int, VP, ctypes.c_uint32, VP, VP, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                ctypes.c_size_t, VP]
        lib.th_hist_bytes.restype = ctypes.c_size_t
        lib.th_hist_bytes.argtypes = [ctypes.c_uint64]
        lib.th_skip_flag_word.restype = ctypes.c_uint32
        lib.th_skip_flag_word.argtypes = []
        lib.th_tile_keys.restype = ctypes.c_uint32
        lib.th_tile_keys.argtypes = []


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    from dreamscene_amd import build as B
    out = tmp_path_factory.mktemp("sort_harness")
    so = str(out / "libsort_harness.so")
    inc = os.environ.get("GSR_TEST_SORT_INCLUDE")
    cmd = [B.hipcc(), "-x", "hip", SRC, "-shared", "-o", so] + (["-I" + inc] if inc else []) + B.COMMON
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(out))
    dt = time.perf_counter() - t0
    assert r.returncode == 0, "hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr
    print(f"\nsort harness built in {dt:.1f} s" + (f" (against {inc})" if inc else ""))
    return Harness(so, dt)


def test_harness_builds_for_gfx950_and_exports_its_symbols(harness):
    """CPU: a signature change in radix_sort.h breaks this build, not the next GPU visit."""
    for name in ("th_sort", "th_scan", "th_hist_bytes", "th_skip_flag_word", "th_tile_keys"):
        assert hasattr(harness.lib, name), name
    out = subprocess.run(["strings", "-n", "6", harness.path], capture_output=True, text=True).stdout
    assert "gfx950" in out
    for k in ("k_os_hist", "k_os_pass", "k_radix_hist", "k_radix_scatter", "k_radix_scan", "k_radix_scan_wide"):
        assert k in out, f"kernel {k} missing from the harness"
    lib = harness.lib
    assert lib.th_tile_keys() == TILE
    assert 0 < lib.th_skip_flag_word() < lib.th_hist_bytes(1) // 4
    for cap in (1, 1024, 1025, TILE + 1, BIG):
        legacy = 256 * ((cap + 1023) // 1024) * 4                    # 256 digits x workgroups of 1024 keys (kItemsSmall)
        one_sweep = (4 * 256 + 16 + 256 * ((cap + TILE - 1) // TILE)) * 4
        assert lib.th_hist_bytes(cap) >= max(legacy, one_sweep) and lib.th_hist_bytes(cap) % 256 == 0


# ------------------------------------------------------------------------------------------------------ key material
def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def k_uniform(n, rng):
    return rng.integers(0, 2 ** 32, n, dtype=np.uint32)


def k_equal(n, rng):
    return np.full(n, 0x9E3779B9, np.uint32)


def k_two(n, rng):
    return np.where(rng.integers(0, 2, n) == 1, np.uint32(0xF1E2D3C4), np.uint32(0x01020304)).astype(np.uint32)


def k_ascending(n, rng):
    return np.sort(k_uniform(n, rng))


def k_descending(n, rng):
    return np.sort(k_uniform(n, rng))[::-1].copy()


def k_live_digit(p):
    """only byte p varies: the identity-pass shortcut of the one-sweep form fires in every other pass and never in p"""
    def f(n, rng):
        const = np.uint32(0x5A3C6996 & ~(0xFF << (8 * p)))
        return (const | (rng.integers(0, 256, n, dtype=np.uint32) << np.uint32(8 * p))).astype(np.uint32)
    return f


def k_depth(n, rng):
    """float depths in [3.5, 7): the top byte is 0x40 for every key"""
    z = rng.uniform(3.5, 7.0, n).astype(np.float32)
    z = np.minimum(z, np.nextafter(np.float32(7.0), np.float32(0.0)))
    return z.view(np.uint32).copy()


def k_per_wave(group):
    """one key (so one digit value in every pass) per run of `group` consecutive elements, different across the runs:
    64 is one ballot round of a wave, 1024 a wave's whole share of a 4096-key tile"""
    def f(n, rng):
        g = np.arange(n, dtype=np.uint64) // np.uint64(group)
        return ((g * np.uint64(2654435761) + np.uint64(0x1234567)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return f


DISTRIBUTIONS = [("uniform", k_uniform), ("equal", k_equal), ("two", k_two), ("ascending", k_ascending),
                 ("descending", k_descending)] + [(f"live{p}", k_live_digit(p)) for p in range(4)] + [
                 ("depth", k_depth), ("wave64", k_per_wave(64)), ("wave1024", k_per_wave(1024))]


def dup_values(n, rng):
    """a values array full of duplicates (about 8 elements per value), spread over all 32 bits"""
    return ((rng.integers(0, n // 8 + 1, n).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def with_sentinels(keys, count, where, rng):
    keys = keys.copy()
    keys[keys == np.uint32(SENTINEL)] = np.uint32(0xFFFFFFFE)        # (only the chosen elements are culled)
    n = len(keys)
    idx = {"front": np.arange(count), "back": np.arange(n - count, n), "scattered": rng.choice(n, count, replace=False)}[where]
    keys[idx] = np.uint32(SENTINEL)
    return keys


class View:
    def __init__(self, keys, vals=None, n_dev=None, rects=None):
        self.keys, self.vals, self.n_dev, self.rects = keys, vals, n_dev, rects


# --------------------------------------------------------------------------------------------------------- one call
class Layout:
    """u32 word offsets inside one view's slab; every section starts on a multiple of 64 words (256 bytes)"""
    def __init__(self, cap: int, hist_words: int):
        al = lambda w: (w + 63) // 64 * 64
        self.cap, self.hist_words = cap, hist_words
        self.sec = GUARD + al(cap) + GUARD
        self.k0, self.v0, self.k1, self.v1 = (i * self.sec + GUARD for i in range(4))
        self.rects = 4 * self.sec
        self.hist = self.rects + al(cap)
        self.n_dev = self.hist + al(hist_words)          # one u64
        self.n_compact = self.n_dev + 2                  # one u64
        self.totals = self.n_dev + 64
        self.words = self.totals + 256 + GUARD


def _u64(row, off) -> int:
    return int(row[off]) | (int(row[off + 1]) << 32)


def run_sort(h, views, cap, form, small, bits=32, drop=False, use_n_dev=None, may_skip=False, early=False):
    """One th_sort call over len(views) views. Values: iota when the views carry none. use_n_dev: hand the device count
    words over (default: when any view has one)."""
    iota = views[0].vals is None
    assert all((v.vals is None) == iota for v in views) and (iota or not drop)
    if use_n_dev is None:
        use_n_dev = any(v.n_dev is not None for v in views)
    with_rects = views[0].rects is not None
    L = Layout(cap, h.lib.th_hist_bytes(cap) // 4)
    slab = np.full((len(views), L.words), FILL, np.uint32)
    for b, v in enumerate(views):
        assert len(v.keys) == cap and v.keys.dtype == np.uint32
        slab[b, L.k0:L.k0 + cap] = v.keys
        if not iota:
            slab[b, L.v0:L.v0 + cap] = v.vals
        if with_rects:
            slab[b, L.rects:L.rects + cap] = v.rects
        slab[b, L.hist:L.hist + L.hist_words] = 0xFFFFFFFF
        slab[b, L.totals:L.totals + 256] = 0xFFFFFFFF
        if use_n_dev:
            nd = cap if v.n_dev is None else v.n_dev
            slab[b, L.n_dev], slab[b, L.n_dev + 1] = nd & 0xFFFFFFFF, nd >> 32
    dev = torch.from_numpy(slab.view(np.int32)).to(DEV)
    early_dev = torch.from_numpy(np.full(2 * len(views), FILL, np.uint32).view(np.int32)).to(DEV)
    p = lambda off: VP(dev.data_ptr() + 4 * off)
    ret = h.lib.th_sort(form, small, p(L.k0), p(L.v0), p(L.k1), p(L.v1), p(L.n_dev) if use_n_dev else None, cap, bits,
                        1 if iota else 0, p(L.n_compact) if drop else None, p(L.hist), p(L.totals),
                        VP(torch.cuda.current_stream().cuda_stream), len(views), L.words * 4, 1 if may_skip else 0,
                        p(L.rects) if with_rects else None, VP(early_dev.data_ptr()) if early else None)
    torch.cuda.synchronize()
    r = SimpleNamespace(L=L, ret=ret, before=slab, views=views, form=form, bits=bits, drop=drop, may_skip=may_skip)
    r.after = dev.cpu().numpy().view(np.uint32)
    r.early = early_dev.cpu().numpy().view(np.uint32).view(np.uint64)
    r.skip_word = L.hist + h.lib.th_skip_flag_word()
    return r


def check_view(r, b, name=""):
    """View b of the call against ref_sort; returns (live count, skip flag)."""
    L, v, cap = r.L, r.views[b], r.L.cap
    before, after = r.before[b], r.after[b]
    passes = (r.bits + 7) // 8
    assert r.ret == (passes & 1), name
    n = cap if v.n_dev is None else min(v.n_dev, cap)
    rk, rv = ref_sort(v.keys, v.vals, n, r.bits, r.drop)
    live = len(rk)
    # a last pass that finds one digit value in all keys moves nothing when the caller allowed it: form 0 only, and never
    # with zero keys. Otherwise the word is 0 (the state was cleared by the sort, whatever it held).
    flag = 0
    if r.form == 0:
        flag = int(after[r.skip_word])
        last = (rk >> np.uint32(8 * (passes - 1))) & np.uint32(255)
        assert flag == int(bool(r.may_skip and passes > 1 and live > 0 and (last == last[0]).all())), name
    where = r.ret ^ flag
    ko, vo = (L.k1, L.v1) if where else (L.k0, L.v0)
    assert np.array_equal(after[ko:ko + live], rk), f"{name}: keys"
    assert np.array_equal(after[vo:vo + live], rv), f"{name}: values"
    assert np.array_equal(after[ko + live:ko + cap], before[ko + live:ko + cap]), f"{name}: keys stored past the live count"
    assert np.array_equal(after[vo + live:vo + cap], before[vo + live:vo + cap]), f"{name}: values stored past the live count"
    if flag:
        # the skipped pass wrote nothing: its output pair holds what the pass before the one before left there
        assert r.bits == 32, "the skip flag is tested for 4 passes"
        ko2, vo2 = (L.k0, L.v0) if where else (L.k1, L.v1)
        k2, v2 = ref_sort(v.keys, v.vals, n, 16, r.drop)
        assert np.array_equal(after[ko2:ko2 + live], k2) and np.array_equal(after[vo2:vo2 + live], v2), f"{name}: skipped pass wrote"
        assert np.array_equal(after[ko2 + live:ko2 + cap], before[ko2 + live:ko2 + cap]), f"{name}: skipped pass wrote"
        assert np.array_equal(after[vo2 + live:vo2 + cap], before[vo2 + live:vo2 + cap]), f"{name}: skipped pass wrote"
    for i in range(4):                                               # everything around the four buffers
        s = i * L.sec
        assert (after[s:s + GUARD] == FILL).all() and (after[s + GUARD + cap:s + L.sec] == FILL).all(), f"{name}: guard of buffer {i}"
    assert np.array_equal(after[L.rects:L.hist], before[L.rects:L.hist]), f"{name}: rectangles"
    assert np.array_equal(after[L.n_dev:L.n_dev + 2], before[L.n_dev:L.n_dev + 2]), f"{name}: n_dev"
    if r.drop:
        assert _u64(after, L.n_compact) == live, f"{name}: *n_compact"
        assert (after[L.n_compact + 2:L.totals] == FILL).all(), name
    else:
        assert (after[L.n_dev + 2:L.totals] == FILL).all(), name
    assert (after[L.totals + 256:] == FILL).all(), name
    return live, flag


def digest(r):
    """what a caller can see of the call: where the result is, the result pair up to cap, the survivor counts"""
    m = hashlib.sha1(str(r.ret).encode())
    for b in range(len(r.views)):
        a = r.after[b]
        where = r.ret ^ (int(a[r.skip_word]) if r.form == 0 else 0)
        ko, vo = (r.L.k1, r.L.v1) if where else (r.L.k0, r.L.v0)
        m.update(a[ko:ko + r.L.cap].tobytes())
        m.update(a[vo:vo + r.L.cap].tobytes())
        if r.drop:
            m.update(a[r.L.n_compact:r.L.n_compact + 2].tobytes())
    return m.hexdigest()


# ------------------------------------------------------------------------------------------------- the single-view cases
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 17 * TILE + 1, BIG]
DEV_CAP = 3 * TILE + 77


def _values(kind, n, rng):
    return dup_values(n, rng) if kind == "dup" else None


def _cases():
    """name -> (cap, bits, drop, builder of the view). Both forms accept every one of them."""
    C = {}

    def add(name, cap, build, bits=32, drop=False):
        assert name not in C
        C[name] = (cap, bits, drop, build)

    for n in SIZES:                                                  # sizes, n = cap
        for vk in ("iota", "dup"):
            add(f"size{n}-{vk}", n, lambda rng, n=n, vk=vk: View(k_uniform(n, rng), _values(vk, n, rng)))
    for n in (TILE + 1, BIG):                                        # key distributions
        for dn, df in DISTRIBUTIONS:
            for vk in ("iota", "dup"):
                add(f"{dn}-{n}-{vk}", n, lambda rng, n=n, df=df, vk=vk: View(df(n, rng), _values(vk, n, rng)))
    for n in (TILE + 1, BIG):                                        # bits: garbage above `bits` must not decide, nor be lost
        for bits in (8, 10, 16, 17, 24, 32):
            for vk in ("iota", "dup"):
                add(f"bits{bits}-{n}-{vk}", n, lambda rng, n=n, vk=vk: View(k_uniform(n, rng), _values(vk, n, rng)), bits=bits)
    # keys that never (or hardly) differ, in an odd number of passes: a pass that reverses equal digits inside one ballot
    # round is undone by the next such pass, so with 2 or 4 passes over equal keys an unstable rank goes unseen
    for n in (TILE + 1, BIG):
        for bits in (8, 24):
            for dn, df in (("equal", k_equal), ("two", k_two)):
                for vk in ("iota", "dup"):
                    add(f"{dn}-bits{bits}-{n}-{vk}", n, lambda rng, n=n, df=df, vk=vk: View(df(n, rng), _values(vk, n, rng)), bits=bits)
    for n in (TILE + 1, BIG):                                        # drop form, as the depth sort calls it
        shares = [("none", 0, ("front",)), ("64th", n // 64, ("front", "back", "scattered")),
                  ("half", n // 2, ("front", "back", "scattered")), ("allbut1", n - 1, ("front", "back", "scattered")),
                  ("all", n, ("front",))]
        for sn, count, places in shares:
            for pl in places:
                add(f"drop-{sn}-{pl}-{n}", n, lambda rng, n=n, count=count, pl=pl:
                    View(with_sentinels(k_uniform(n, rng), count, pl, rng)), drop=True)
    for n in (1, 65, 1025, TILE):                                    # ... at the small sizes, one key in two culled
        add(f"drop-half-scattered-{n}", n, lambda rng, n=n: View(with_sentinels(k_uniform(n, rng), (n + 1) // 2, "scattered", rng)),
            drop=True)
    add("drop-all-1", 1, lambda rng: View(np.full(1, SENTINEL, np.uint32)), drop=True)
    # device count: 0, 1, inside a tile, on a boundary of every tile size (1024, 2048, 4096), cap - 1, cap, beyond cap
    for cap, counts in ((DEV_CAP, (0, 1, 5000, 2 * TILE, DEV_CAP - 1, DEV_CAP, DEV_CAP + 1000)), (BIG, (17 * TILE, BIG + 1000))):
        for nd in counts:
            for vk in ("iota", "dup", "drop"):
                def build(rng, cap=cap, nd=nd, vk=vk):
                    keys = k_uniform(cap, rng)
                    if vk == "drop":
                        keys = with_sentinels(keys, cap // 4, "scattered", rng)
                    return View(keys, _values(vk, cap, rng), n_dev=nd)
                add(f"ndev{nd}-cap{cap}-{vk}", cap, build, drop=(vk == "drop"))
    return C


CASES = _cases()
_seen = {}          # (case, form, small) -> digest of the result: every case runs once, the agreement test reuses it


def _run_case(h, name, form, small):
    cap, bits, drop, build = CASES[name]
    view = build(_rng(name))
    r = run_sort(h, [view], cap, form, small, bits=bits, drop=drop)
    check_view(r, 0, name)
    _seen[(name, form, small)] = digest(r)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(CASES))
def test_sort_case(harness, name, form, small):
    _run_case(harness, name, form, small)


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
@pytest.mark.parametrize("name", list(CASES))
def test_forms_agree(harness, name, small):
    """what form 0 leaves is what form 1 leaves: the result pair up to cap, where it is, the survivor count"""
    for form in FORMS:
        if (name, form, small) not in _seen:
            _run_case(harness, name, form, small)
    assert _seen[(name, 0, small)] == _seen[(name, 1, small)]


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("vk", ["iota", "dup", "drop"])
def test_device_count_above_cap_is_cap(harness, vk, form, small):
    """n_dev = cap + 1000 behaves exactly like no device count at all"""
    def view(nd):
        rng = _rng("above-" + vk)
        keys = k_uniform(DEV_CAP, rng)
        if vk == "drop":
            keys = with_sentinels(keys, DEV_CAP // 4, "scattered", rng)
        return View(keys, _values(vk, DEV_CAP, rng), n_dev=nd)
    a = run_sort(harness, [view(DEV_CAP + 1000)], DEV_CAP, form, small, drop=(vk == "drop"))
    b = run_sort(harness, [view(None)], DEV_CAP, form, small, drop=(vk == "drop"))
    check_view(a, 0)
    check_view(b, 0)
    assert digest(a) == digest(b)


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
@pytest.mark.parametrize("form", FORMS)
def test_every_key_dropped_writes_nothing(harness, form, small):
    """the call returns, *n_compact == 0, and neither pair changed anywhere (the keys are still where they were)"""
    r = run_sort(harness, [View(np.full(BIG, SENTINEL, np.uint32))], BIG, form, small, drop=True)
    assert check_view(r, 0)[0] == 0
    L = r.L
    assert np.array_equal(r.after[0, :L.rects], r.before[0, :L.rects])


# ------------------------------------------------------------------------------------------------------------ batches
def _batch_views(cap, vk, rng):
    """three views of one call: different counts, distributions and sentinel shares; the middle one has no keys"""
    drop = vk == "drop"
    k0 = k_uniform(cap, rng)
    k1 = k_two(cap, rng)
    k2 = k_depth(cap, rng)
    if drop:
        k0 = with_sentinels(k0, cap // 64, "scattered", rng)
        k1 = with_sentinels(k1, cap // 3, "front", rng)
        k2 = with_sentinels(k2, cap // 2, "scattered", rng)
    return [View(k0, _values(vk, cap, rng), n_dev=cap + 1000), View(k1, _values(vk, cap, rng), n_dev=0),
            View(k2, _values(vk, cap, rng), n_dev=2 * TILE)]


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("vk", ["iota", "dup", "drop"])
@pytest.mark.parametrize("cap", [5 * TILE + 9, 17 * TILE + 1])
def test_batch_of_three_views(harness, cap, vk, form, small):
    name = f"batch-{cap}-{vk}"
    r = run_sort(harness, _batch_views(cap, vk, _rng(name)), cap, form, small, drop=(vk == "drop"))
    lives = [check_view(r, b, f"{name} view {b}")[0] for b in range(3)]
    assert lives[1] == 0 and lives[0] > 0 and lives[2] > 0
    _seen[(name, form, small)] = digest(r)


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
@pytest.mark.parametrize("vk", ["iota", "dup", "drop"])
@pytest.mark.parametrize("cap", [5 * TILE + 9, 17 * TILE + 1])
def test_batch_forms_agree(harness, cap, vk, small):
    name = f"batch-{cap}-{vk}"
    for form in FORMS:
        if (name, form, small) not in _seen:
            test_batch_of_three_views(harness, cap, vk, form, small)
    assert _seen[(name, 0, small)] == _seen[(name, 1, small)]


# ---------------------------------------------------------------------------------------- skip flag (one-sweep form only)
def _skip_view(kind, cap, vk, rng):
    keys = {"same_top": k_depth, "other_top": k_uniform}[kind](cap, rng)
    if vk == "drop":
        keys = with_sentinels(keys, cap // 64, "scattered", rng)
    return View(keys, _values(vk, cap, rng))


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
@pytest.mark.parametrize("vk", ["iota", "dup", "drop"])
@pytest.mark.parametrize("cap", [TILE + 1, BIG])
@pytest.mark.parametrize("kind", ["same_top", "other_top"])
def test_skip_flag(harness, kind, cap, vk, small):
    """may_skip, 32 bits. One top byte in all keys: the flag is 1, the sorted lists are in the pair the last pass would have
    read ((k1, v1): the return value says (k0, v0)) and that pass stored nothing. Otherwise the flag is 0 and the result is
    where the return value says (check_view asserts both placements)."""
    r = run_sort(harness, [_skip_view(kind, cap, vk, _rng(f"skip-{kind}-{cap}-{vk}"))], cap, 0, small, drop=(vk == "drop"),
                 may_skip=True)
    live, flag = check_view(r, 0)
    assert r.ret == 0 and live > 0 and flag == (1 if kind == "same_top" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
@pytest.mark.parametrize("vk", ["iota", "dup", "drop"])
def test_skip_flag_is_per_view(harness, vk, small):
    cap = 5 * TILE + 9
    rng = _rng("skip-batch-" + vk)
    views = [_skip_view("same_top", cap, vk, rng), _skip_view("other_top", cap, vk, rng), _skip_view("same_top", cap, vk, rng)]
    views[2].n_dev = 0                                               # no keys: nothing to skip
    r = run_sort(harness, views, cap, 0, small, drop=(vk == "drop"), may_skip=True)
    assert [check_view(r, b, f"view {b}")[1] for b in range(3)] == [1, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
def test_skip_flag_stays_0_without_survivors(harness, small):
    r = run_sort(harness, [View(np.full(TILE + 1, SENTINEL, np.uint32))], TILE + 1, 0, small, drop=True, may_skip=True)
    assert check_view(r, 0) == (0, 0)


# ---------------------------------------------------------------------------------- early weight sum (one-sweep form only)
UNTOUCHED = FILL | (FILL << 32)


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
@pytest.mark.parametrize("n_dev", [None, 0, 2 * TILE, TILE + 777])
@pytest.mark.parametrize("cap", [TILE + 1, BIG])
def test_early_weight_sum(harness, cap, n_dev, small):
    rng = _rng(f"early-{cap}-{n_dev}")
    v = View(with_sentinels(k_uniform(cap, rng), cap // 64, "scattered", rng), n_dev=n_dev, rects=k_uniform(cap, rng))
    r = run_sort(harness, [v], cap, 0, small, drop=True, early=True)
    check_view(r, 0)
    assert int(r.early[0]) == ref_weight(v.rects, v.keys, cap if n_dev is None else min(n_dev, cap))


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
def test_early_weight_sum_above_2_to_32(harness, small):
    """2^17 + 5 survivors that all carry the maximal 256 x 256 rectangle: the sum needs 34 bits"""
    live, cap = 2 ** 17 + 5, 2 ** 17 + 5 + 1000
    rng = _rng("early-max")
    keys = with_sentinels(k_uniform(cap, rng), 1000, "scattered", rng)
    rects = (np.uint32(0xFFFF0000) | rng.integers(0, 2 ** 16, cap, dtype=np.uint32)).astype(np.uint32)
    r = run_sort(harness, [View(keys, rects=rects)], cap, 0, small, drop=True, early=True)
    assert check_view(r, 0)[0] == live
    assert ref_weight(rects, keys, cap) == live * 65536 > 2 ** 32
    assert int(r.early[0]) == live * 65536


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
def test_early_weight_sum_is_per_view(harness, small):
    cap = 5 * TILE + 9
    rng = _rng("early-batch")
    views = _batch_views(cap, "drop", rng)
    for v in views:
        v.rects = k_uniform(cap, rng)
    r = run_sort(harness, views, cap, 0, small, drop=True, early=True)
    for b, v in enumerate(views):
        check_view(r, b, f"view {b}")
        assert int(r.early[b]) == ref_weight(v.rects, v.keys, min(v.n_dev, cap)), b
    assert int(r.early[1]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("small", SMALL)
@pytest.mark.parametrize("vk", ["iota", "dup"])
def test_early_weight_sum_only_in_the_drop_form(harness, vk, small):
    """rects and early_out without n_compact: radix_sort_u32 ignores both, early_out keeps what it held"""
    cap = TILE + 1
    rng = _rng("early-ignored-" + vk)
    v = View(k_uniform(cap, rng), _values(vk, cap, rng), rects=k_uniform(cap, rng))
    r = run_sort(harness, [v], cap, 0, small, early=True)
    check_view(r, 0)
    assert int(r.early[0]) == UNTOUCHED


def test_cap_0_launches_nothing(harness):
    """CPU: the harness answers -1 before any launch (the product's callers never pass cap == 0)"""
    assert harness.lib.th_sort(0, 0, None, None, None, None, None, 0, 32, 1, None, None, None, None, 1, 0, 0, None, None) == -1
    assert harness.lib.th_sort(1, 1, None, None, None, None, None, 0, 32, 1, None, None, None, None, 1, 0, 0, None, None) == -1


# ------------------------------------------------------------------------------------------------------------- the scans
STRIDES = [1, 4, 255, 256, 1023, 1024, 1025, 4095, 4096, 4097, 5000]
PER_BLOCK = 64
# entries in use, through *n_items = 64 used - 37: none, one, part of a chunk of either width (1024 / 4096 entries), exactly
# one chunk of either width, and more than the stride (clamped to the stride). None: n_items is NULL, the whole row.
USED = [None, 0, 1, 515, 1024, 2051, 4096, "over"]


def _scan_rows(rows, stride, rng):
    """row r mod 3 == 0: values just below 2^31, so the running carry wraps at every second entry; 1: all 32 bits;
    2: small counts, like a digit histogram"""
    x = np.empty((rows, stride), np.uint32)
    for r in range(rows):
        if r % 3 == 0:
            x[r] = np.uint32(2 ** 31) - rng.integers(1, 1000, stride, dtype=np.uint32)
        elif r % 3 == 1:
            x[r] = rng.integers(0, 2 ** 32, stride, dtype=np.uint32)
        else:
            x[r] = rng.integers(0, 1000, stride, dtype=np.uint32)
    return x


def _n_items(used, stride):
    if used is None:
        return None
    used = stride + 7 if used == "over" else used
    return max(0, PER_BLOCK * used - 37)


def run_scan(h, wide, rows, stride, inputs, n_items):
    """inputs: one [rows, stride] array per view; n_items: one count (or None, all views alike) per view. Returns the
    slabs before and after, and the offsets of the rows and totals in a view's slab."""
    al = lambda w: (w + 63) // 64 * 64
    o_hist = GUARD
    o_tot = o_hist + al(rows * stride) + GUARD
    o_n = o_tot + al(rows) + GUARD
    words = o_n + GUARD
    null = n_items[0] is None
    assert all((n is None) == null for n in n_items)
    slab = np.full((len(inputs), words), FILL, np.uint32)
    for b, x in enumerate(inputs):
        slab[b, o_hist:o_hist + rows * stride] = x.reshape(-1)
        if not null:
            slab[b, o_n], slab[b, o_n + 1] = n_items[b] & 0xFFFFFFFF, n_items[b] >> 32
    dev = torch.from_numpy(slab.view(np.int32)).to(DEV)
    p = lambda off: VP(dev.data_ptr() + 4 * off)
    h.lib.th_scan(wide, p(o_hist), stride, p(o_tot), None if null else p(o_n), PER_BLOCK, rows, len(inputs), words * 4,
                  VP(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return slab, dev.cpu().numpy().view(np.uint32), o_hist, o_tot


def check_scan(h, rows, stride, inputs, n_items, name):
    outs = []
    for wide in (0, 1):
        before, after, o_hist, o_tot = run_scan(h, wide, rows, stride, inputs, n_items)
        expect = before.copy()                                       # nothing else in the slab may change
        for b, x in enumerate(inputs):
            used = stride if n_items[b] is None else min((n_items[b] + PER_BLOCK - 1) // PER_BLOCK, stride)
            scanned, totals = ref_scan(x, used)
            expect[b, o_hist:o_hist + rows * stride] = scanned.reshape(-1)
            expect[b, o_tot:o_tot + rows] = totals
        assert np.array_equal(after, expect), f"{name}: {'wide' if wide else 'narrow'} scan"
        outs.append(after)
    assert np.array_equal(outs[0], outs[1]), f"{name}: the two widths differ"


@pytest.mark.gpu
@pytest.mark.parametrize("used", USED, ids=lambda u: f"used_{u}")
@pytest.mark.parametrize("rows", [1, 256])
@pytest.mark.parametrize("stride", STRIDES)
def test_scan(harness, stride, rows, used):
    name = f"scan-{stride}-{rows}-{used}"
    check_scan(harness, rows, stride, [_scan_rows(rows, stride, _rng(name))], [_n_items(used, stride)], name)


@pytest.mark.gpu
@pytest.mark.parametrize("used", [(2051, "over"), (0, 4096), (1, 515)], ids=lambda u: f"used_{u[0]}_{u[1]}")
@pytest.mark.parametrize("rows", [1, 256])
@pytest.mark.parametrize("stride", [1025, 4097])
def test_scan_batch_of_two(harness, stride, rows, used):
    name = f"scan2-{stride}-{rows}-{used}"
    rng = _rng(name)
    check_scan(harness, rows, stride, [_scan_rows(rows, stride, rng) for _ in used], [_n_items(u, stride) for u in used], name)
