"""K6 (csrc/render_fwd.hip) and K7 (csrc/render_bwd.hip) at CRAFTED tile-list lengths, stop points and block reach: the scenes of
tests/tile_list_scenes.py against oracle/gsr_oracle.c, through every K6 / K7 instantiation (seg_len 64 / 128 / 256 with the
list-parallel forward, the whole-tile forward), the score variant of K6, state buffers that inherit NaN bit patterns, and a
RasterContext reused from a deep scene to a shallow one.

CPU part (no GPU): test_cases_reach_what_they_claim asserts, from the oracle's outputs alone, that every case reaches the
boundary it is named for, and prints the list lengths, the n_contrib coverage and the per-wave pad table of `pads`:
  256-entry batch change .......... length[255 / 256 / 257 / 511 / 512 / 513 / 769], stop[256], stop[512]
  seg_len cut, every pad residue .. pads (candidate counts 0, 1, 2, 3 mod 4 over one quarter's four waves at the 64 and 128 cuts)
  wave with an empty candidate list  dots_only (14 of 16 4x4 blocks and two of four 8x8 blocks reached by nothing at all; the owner
                                     reached by nothing in one 64-entry chunk, the opposite block by nothing in the others)
  stop on each quad slot .......... stop[B]: pixels leave through T < 1e-4 with n_contrib on every value of [B - 4, B + 4]
  tile depth = seg_len, one past .. stop[B]: tile (2, 0) has depth exactly B, tile (2, 3) exactly B + 1; length[64 / 65 / 128 / ...]
  early all-done exit ............. opaque (769 entries, no pixel gets past the first batch)
  tile_depth 0 .................... transparent (lists of 257 entries, nothing composited)
  ragged tiles .................... ragged (17 x 17: tiles of one column, one row, one pixel), and the 8-row / 8-column tiles of all

Bars (BASELINE.json, tests/test_gpu_parity.py): radii, point_list, ranges, n_contrib and the bits of final_T bit-exact; colour,
depth, alpha and every per-Gaussian gradient within 1e-5 of the tensor's own largest reference entry (tests/util.py rel_scale).
These scenes are unlike the random ones (hundreds of coincident centres, low opacities), so the C oracle was first measured
against float64 autograd of oracle/torch_oracle.py on every case (test_c_oracle_vs_float64 repeats the measurement): where that
distance e_ref exceeds 2.5e-6 of a tensor's scale the C oracle cannot arbitrate 1e-5 and the tensor's bar is 4 e_ref, the rule of
tests/photometric_ref.parity. No bar comes from the HIP path's output. Measured e_ref (largest over the tensors of a case; the
tensors above 2.5e-6 are listed in E_REF):
  length[1] 6.6e-07   length[2] 5.0e-07 (8 pixels left out)   length[3] 6.5e-07   length[4] 2.3e-07   length[5] 1.0e-06
  length[63] 6.3e-07  length[64] 6.3e-07  length[65] 5.7e-07  length[127] 8.7e-07  length[128] 7.5e-07  length[129] 8.7e-07
  length[255] 1.0e-06  length[256] 1.0e-06  length[257] 1.2e-06  length[511] 1.6e-06  length[512] 2.1e-06  length[513] 1.5e-06
  length[769] 2.2e-06  opaque 5.2e-07 (16 pixels left out)  transparent 0  pads 1.4e-06  dots_only 2.3e-06  ragged 1.2e-06
  stop[64] 1.2e-05   stop[128] 2.1e-05   stop[192] 4.9e-06   stop[256] 7.6e-06   stop[512] 7.8e-06
  (the stop cases' largest: dL/dmeans of the pinning dots -- sigma 0.55 px, where the fp32 rounding of a pixel coordinate near 50
  moves alpha by ~2e-5 relative; that rounding is part of the fp32 definition the device shares with the C oracle)
  ("pixels left out": float64 takes a hard gate the other way there, see _float64_distance)
"""
import functools

import numpy as np
import pytest
import torch

from tests import tile_list_scenes as S
from tests.util import err, oracle_view, rel_scale, same_bits, settings_for

DEV = "cuda:0"
TOL = 1e-5
E_REF_FLOOR = 2.5e-6

# (case, tensor) -> e_ref, the C oracle's distance from float64 autograd relative to the tensor's largest entry, where it exceeds
# E_REF_FLOOR: the bar of that tensor on that case is 4 e_ref instead of 1e-5.
E_REF = {
    ("stop[64]", "dL_dmeans3D"): 1.21e-05, ("stop[64]", "dL_dmeans2D"): 1.2e-05,
    ("stop[128]", "dL_dmeans3D"): 2.06e-05, ("stop[128]", "dL_dmeans2D"): 2.14e-05, ("stop[128]", "dL_dscales"): 3.38e-06,
    ("stop[192]", "dL_dmeans3D"): 3.34e-06, ("stop[192]", "dL_dmeans2D"): 4.93e-06, ("stop[192]", "dL_dscales"): 3.27e-06,
    ("stop[256]", "dL_dmeans3D"): 4.81e-06, ("stop[256]", "dL_dmeans2D"): 7.62e-06, ("stop[256]", "dL_dscales"): 2.99e-06,
    ("stop[512]", "dL_dmeans3D"): 7.36e-06, ("stop[512]", "dL_dmeans2D"): 7.84e-06, ("stop[512]", "dL_dshs"): 6.13e-06,
    ("stop[512]", "dL_dscales"): 6.21e-06,
}

GRAD_PAIRS = (("dL_dmeans3D", "dL_dmeans3D"), ("dL_dmeans2D", "dL_dmeans2D"), ("dL_dopacities", "dL_dopacity"),
              ("dL_dshs", "dL_dshs"), ("dL_dscales", "dL_dscales"), ("dL_drotations", "dL_drotations"))
FORMS = ("seg64", "seg128", "seg256", "whole_tile")
SCORE_CASES = ("length[256]", "length[257]", "length[513]", "stop[256]", "opaque")


def bar(case, tensor):
    e = E_REF.get((case, tensor), 0.0)
    return 4.0 * e if e > E_REF_FLOOR else TOL


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's scene, the C oracle's forward and backward of it: computed once, shared by the tests, never written to."""
    from dreamscene_amd import synth
    from oracle import c_oracle as CO
    CO.build()
    g, cam, bg, ex = S.case(name)
    P = g["means3D"].shape[0]
    v = oracle_view(CO, cam, P, 1, 0, bg)
    f = CO.forward(v, g["means3D"], g["opacities"], shs=g["shs"], scales=g["scales"], rotations=g["rotations"])
    gi, gda = synth.upstream_grads(cam.image_height, cam.image_width, 11)
    b = CO.backward(v, f, gi, gda, g["means3D"], shs=g["shs"], scales=g["scales"], rotations=g["rotations"])
    for a in list(g.values()) + [gi, gda] + [x for d in (f, b) for x in d.values() if isinstance(x, np.ndarray)]:
        a.setflags(write=False)
    return dict(name=name, g=g, cam=cam, bg=bg, ex=ex, P=P, v=v, f=f, b=b, gi=gi, gda=gda)


@functools.lru_cache(maxsize=None)
def _score_ref(name, mode):
    from oracle import c_oracle as CO
    c = _case(name)
    g = c["g"]
    v = oracle_view(CO, c["cam"], c["P"], 1, 0, c["bg"], score_mode=mode)
    f = CO.forward(v, g["means3D"], g["opacities"], shs=g["shs"], scales=g["scales"], rotations=g["rotations"], score=True)
    return f["important_score"]


# ---------------------------------------------------------------------------------------------------------------------- CPU part
def _tile_stats(c):
    f, cam = c["f"], c["cam"]
    H, W = cam.image_height, cam.image_width
    gx, gy = (W + 15) // 16, (H + 15) // 16
    lens = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).reshape(gy, gx)
    nc = f["n_contrib"].astype(np.int64)
    depth = np.array([[nc[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].max() for tx in range(gx)] for ty in range(gy)])
    return lens, nc, depth


def _runs(values):
    """Sorted integers as a short string of runs: 1-3, 7, 9-12"""
    v = sorted(set(int(x) for x in values))
    out, i = [], 0
    while i < len(v):
        j = i
        while j + 1 < len(v) and v[j + 1] == v[j] + 1:
            j += 1
        out.append(str(v[i]) if i == j else f"{v[i]}-{v[j]}")
        i = j + 1
    return ", ".join(out)


@pytest.mark.parametrize("name", S.names())
def test_cases_reach_what_they_claim(c_oracle, name):
    c = _case(name)
    f, cam, ex = c["f"], c["cam"], c["ex"]
    lens, nc, depth = _tile_stats(c)
    stopped = S.stopped_mask(f, cam)
    kind = ex["kind"]
    print(f"\n[{name}] P {c['P']}, {cam.image_height} x {cam.image_width}; list lengths {_runs(lens.reshape(-1))}; tile depths "
          f"{depth.tolist()}; n_contrib {_runs(nc.reshape(-1))}; pixels stopped by T < 1e-4: {int(stopped.sum())} (n_contrib "
          f"{_runs(nc[stopped])}), run to the last entry: {int((nc == lens.max()).sum())}, took no entry: {int((nc == 0).sum())}")
    assert c["P"] <= 800 and cam.image_height <= 40 and cam.image_width <= 56
    assert np.array_equal((f["radii"] > 0), np.ones(c["P"], bool)), "a Gaussian of the scene is culled"
    if kind in ("length", "ragged"):
        L = ex["L"]
        assert (lens == L).all(), "every tile holds exactly L entries"
        assert (nc == L).any(), "no pixel runs to the last entry"
        # (tile_depth == L in every tile but the corner tile of length[769], whose pixels take the nearer sheets only)
        assert (depth == L).sum() >= depth.size - 1, "tile_depth == L"
        if ex["some_stopped"]:
            assert (stopped & (nc < L)).any(), "no pixel stops on T < 1e-4"
        else:
            assert not stopped.any()
        if kind == "ragged":
            assert (cam.image_height, cam.image_width) == (17, 17) and lens.shape == (2, 2)
    elif kind == "stop":
        B = ex["B"]
        got = set(int(x) for x in nc[stopped])
        assert got >= set(range(B - 4, B + 5)), f"T < 1e-4 stops with n_contrib {_runs(got)} do not cover [{B - 4}, {B + 4}]"
        assert depth[ex["depth_B"]] == B, f"tile {ex['depth_B']}: depth {depth[ex['depth_B']]}, not B"
        assert depth[ex["depth_B1"]] == B + 1, f"tile {ex['depth_B1']}: depth {depth[ex['depth_B1']]}, not B + 1"
        assert lens.max() > B + 4
        # the two pinned tiles composite their own dots only: the sheets reach none of their pixels
        for tile, n_dots in ((ex["depth_B"], S.STOP_PIN_DOTS), (ex["depth_B1"], S.STOP_PIN_DOTS)):
            assert lens[tile] == B + S.STOP_TAIL + n_dots
    elif kind == "opaque":
        assert (lens == ex["L"]).all()
        assert stopped[nc > 0].all() and nc.max() < 256 and nc.min() >= 1, "a pixel gets past the first batch"
        print(f"[{name}] every pixel stops inside the first batch (deepest n_contrib {nc.max()}): {ex['L'] // 256} batches unread")
    elif kind == "transparent":
        assert (lens == ex["L"]).all() and nc.max() == 0 and (depth == 0).all()
        assert (f["final_T"] == 1.0).all()
        assert np.array_equal(f["image"], np.broadcast_to(c["bg"][:, None, None], f["image"].shape))
    elif kind == "pads":
        ty, tx = S.PADS_TILE
        assert lens[ty, tx] == ex["L"]
        c4 = S.chunk_reach_counts(f, cam, ty, tx, 4, 64)
        print(f"[{name}] tile {S.PADS_TILE}, quarter 3 (K6 waves 0-3 = blocks {S.PADS_QUARTER}): candidates per 64-entry chunk; "
              "count and pad (-count & 3) at each seg_len-64 cut as K6 pads it; count at the seg_len-128 cut")
        res64, res128 = [], []
        for w, (br, bc) in enumerate(((2, 2), (2, 3), (3, 2), (3, 3))):
            per_chunk = c4[:4, br, bc]
            cnt, row = 0, []
            for k in range(3):                  # the cuts inside the first batch: after chunks 0, 1, 2 (KB = 64)
                cnt += int(per_chunk[k])
                row.append((cnt, (-cnt) & 3))
                cnt += (-cnt) & 3
            c128 = int(per_chunk[0] + per_chunk[1])
            res64.append(row[0][0] % 4)
            res128.append(c128 % 4)
            print(f"[{name}]   wave {w}: chunks {per_chunk.tolist()}; seg 64 cuts (count, pad) {row}; seg 128 cut count {c128} "
                  f"(residue {c128 % 4})")
        assert sorted(res64) == [0, 1, 2, 3], f"residues at the seg_len-64 cut: {res64}"
        assert sorted(res128) == [0, 1, 2, 3], f"residues at the seg_len-128 cut: {res128}"
        # the quarter's pixels are still compositing at both cuts (the pads are walked, the checkpoints written and read)
        q = nc[16 * ty + 8:16 * ty + 16, 16 * tx + 8:16 * tx + 16]
        assert q.min() > 192, f"a pixel of the quarter ends at {q.min()}"
        assert depth[ty, tx] > 256
    elif kind == "dots_only":
        ty, tx = S.DOTS_TILE
        assert lens[ty, tx] == ex["L"] and lens.sum() == ex["L"], "the dots are in one tile's list only"
        c4 = S.chunk_reach_counts(f, cam, ty, tx, 4, 64)
        c8 = S.chunk_reach_counts(f, cam, ty, tx, 8, 256)
        own, opp = c4[:, 1, 1], c4[:, 2, 2]
        print(f"[{name}] tile {S.DOTS_TILE}: candidates per 64-entry chunk: owner block {own.tolist()}, opposite block {opp.tolist()}, "
              f"the other 14 blocks {int(c4.sum() - own.sum() - opp.sum())}; per 256-entry batch and 8x8 block {c8.tolist()}")
        assert own.tolist() == [64, 0, 64, 64, 64] and opp.tolist() == [0, 64, 0, 0, 0]
        assert c4.sum() == own.sum() + opp.sum(), "another 4x4 block is reached"
        assert (c8[:, 0, 1] == 0).all() and (c8[:, 1, 0] == 0).all() and c8[1, 1, 1] == 0
        assert depth[ty, tx] == ex["L"]
    else:
        raise AssertionError(kind)


def _float64_distance(c):
    """-> {tensor: |C oracle - float64 autograd| / the tensor's largest float64 entry}, and the number of pixels on which float64
    takes a hard gate the other way (length[2] and opaque: alpha sits on the 0.99 cap and T = 0.01 x 0.01 ON the 1e-4 threshold --
    fp32's 1 - 0.99f is below 0.01, float64's is not). On such a pixel the two are different functions; the device shares the
    C oracle's gates bit for bit, so the distance that matters is the one over the pixels where the gates agree: the images are
    compared there, and the gradients of both sides are taken with the upstream gradient zeroed on the others."""
    from oracle import c_oracle as CO
    from tests.test_oracle_consistency import _torch_run
    f, b, g = c["f"], c["b"], c["g"]
    gi, gda = c["gi"], c["gda"]
    r = _torch_run(g, c["cam"], c["bg"], 0, gi=gi, gda=gda, cam_grad=False)
    same = f["n_contrib"] == r["aux"]["n_contrib"]
    if not same.all():
        gi, gda = gi * same[None], gda * same[None]
        r = _torch_run(g, c["cam"], c["bg"], 0, gi=gi, gda=gda, cam_grad=False)
        b = CO.backward(c["v"], f, gi, gda, g["means3D"], shs=g["shs"], scales=g["scales"], rotations=g["rotations"])
    rep = dict(color=err(f["image"][:, same], r["img"][:, same]) / rel_scale(r["img"]),
               depth=err(f["depth_alpha"][0][same], r["da"][0][same]) / rel_scale(r["da"][0]),
               alpha=err(f["depth_alpha"][1][same], r["da"][1][same]) / rel_scale(r["da"][1]))
    for tk, (hk, ck) in zip(("means3D", "means2D", "opacities", "shs", "scales", "rotations"), GRAD_PAIRS):
        a = r["grads"][tk]
        rep[hk] = err(a, np.asarray(b[ck]).reshape(a.shape)) / rel_scale(a)
    return rep, int((~same).sum())


@pytest.mark.parametrize("name", S.names())
def test_c_oracle_vs_float64(c_oracle, name):
    """The measurement behind E_REF, repeated: every tensor of every case within 2.5e-6 of float64 autograd (relative to the
    tensor's largest entry) except those listed in E_REF, and those no further off than listed."""
    c = _case(name)
    rep, n_other = _float64_distance(c)
    print(f"\n[{name}] C oracle vs float64 autograd (n_contrib " +
          ("equal" if n_other == 0 else f"differs on {n_other} pixels: left out") + "): " +
          " ".join(f"{k} {v:.2e}" for k, v in rep.items()))
    for k, e in rep.items():
        listed = E_REF.get((name, k), 0.0)
        assert e <= max(E_REF_FLOOR, listed * 1.02), f"{k}: e_ref {e:.3e}, listed {listed:.3e}"


# ---------------------------------------------------------------------------------------------------------------------- GPU part
def _context(form, **kw):
    from dreamscene_amd import rasterizer as R
    if form == "whole_tile":
        return R.RasterContext(fwd_variant=1, **kw)
    return R.RasterContext(seg_len=int(form[3:]), fwd_variant=0, **kw)


def _hip(c, form, rc=None, score=False, score_mode=0, backward=True, before=None):
    """Forward (and backward) of case c in one K6 / K7 form. -> (out, grads or None), synchronised.
    before: called between the upload of the inputs and the forward (test_state_buffer_full_of_nans)."""
    from dreamscene_amd import rasterizer as R
    rc = rc or _context(form, score_mode=score_mode)
    s = settings_for(c["cam"], c["bg"], 0, DEV, score_flag=score)
    t = {k: torch.tensor(v, device=DEV) for k, v in c["g"].items()}
    gi, gda = torch.tensor(c["gi"], device=DEV), torch.tensor(c["gda"], device=DEV)
    if before is not None:
        before()
    out, st = R.rasterize_forward_raw(s, t["means3D"], t["opacities"], t["shs"], None, t["scales"], t["rotations"], None, rc=rc)
    assert int(st.binning.fwd_mode) == (1 if form == "whole_tile" else 0)
    assert int(st.binning.seg_len) == (256 if form == "whole_tile" else int(form[3:]))
    grads = R.rasterize_backward_raw(st, gi, gda) if backward else None
    torch.cuda.synchronize()
    return out, grads


def _check(c, out, grads):
    """The bars of the module docstring, every figure printed before it is asserted."""
    name, f, b = c["name"], c["f"], c["b"]
    assert np.array_equal(out["radii"].cpu().numpy(), f["radii"]), "radii"
    assert out["N"] == f["N"], "pair count"
    assert np.array_equal(out["point_list"].cpu().numpy().view(np.uint32)[:f["N"]], f["point_list"]), "point_list"
    assert np.array_equal(out["ranges"].cpu().numpy().view(np.uint32), f["ranges"]), "ranges"
    nc = out["n_contrib"].cpu().numpy().view(np.uint32)
    bad = np.argwhere(nc != f["n_contrib"])
    assert bad.size == 0, f"n_contrib differs on {len(bad)} pixels, first (y, x) {bad[0]}: {nc[tuple(bad[0])]} vs {f['n_contrib'][tuple(bad[0])]}"
    assert np.array_equal(out["final_T"].cpu().numpy().view(np.uint32), f["final_T"].view(np.uint32)), "final_T bits"
    da = out["depth_alpha"].cpu().numpy()
    figures = []
    for what, a, r in (("color", out["color"].cpu().numpy(), f["image"]), ("depth", da[0], f["depth_alpha"][0]),
                       ("alpha", da[1], f["depth_alpha"][1])):
        figures.append((what, err(a, r), bar(name, what) * rel_scale(r)))
    if grads is not None:
        for hk, ok in GRAD_PAIRS:
            a, r = grads[hk].cpu().numpy().reshape(-1), np.asarray(b[ok]).reshape(-1)
            assert np.isfinite(a).all(), f"{hk}: not finite"
            figures.append((hk, err(a, r), bar(name, hk) * rel_scale(r)))
    print(f"[{name}] " + " ".join(f"{k} {e:.2e}/{lim:.2e}" for k, e, lim in figures))
    for k, e, lim in figures:
        assert e <= lim, f"{k}: max abs err {e:.3e}, bar {lim:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", S.names())
def test_forward_backward_vs_c_oracle(built_lib, c_oracle, name, form):
    c = _case(name)
    out, grads = _hip(c, form)
    _check(c, out, grads)
    if c["ex"]["kind"] == "transparent":
        # nothing composited: the image IS the background, no backward item exists, every gradient is exactly zero
        bg = np.broadcast_to(c["bg"][:, None, None], c["f"]["image"].shape)
        assert np.array_equal(out["color"].cpu().numpy().view(np.uint32), np.ascontiguousarray(bg).view(np.uint32))
        assert float(out["depth_alpha"].abs().max()) == 0.0
        for hk, _ in GRAD_PAIRS:
            assert float(grads[hk].abs().max()) == 0.0, hk


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("seg64", "seg256", "whole_tile"))
@pytest.mark.parametrize("name", SCORE_CASES)
def test_score_variant(built_lib, c_oracle, name, form):
    """K6<SCORE>: the pixel counts are flushed from LDS at every batch change (and after the early exit). Mode 0 = opacity x an
    integer count: the oracle's bits (test_autograd_module_and_score); mode 1 = sum of alpha T in fp32 atomics against the
    oracle's double sum: the bar of test_score_mode_alpha_T."""
    c = _case(name)
    out, _ = _hip(c, form, score=True, backward=False)
    ref = _score_ref(name, 0)
    got = out["score"].cpu().numpy()
    assert int((ref > 0).sum()) >= 100
    assert np.array_equal(got, ref), f"mode-0 scores differ on {int((got != ref).sum())} Gaussians: {err(got, ref):.3e}"
    assert np.array_equal(out["n_contrib"].cpu().numpy().view(np.uint32), c["f"]["n_contrib"])
    out, _ = _hip(c, form, score=True, score_mode=1, backward=False)
    ref = _score_ref(name, 1)
    e = err(out["score"].cpu().numpy(), ref)
    print(f"[{name}] mode-1 score err {e:.2e}/{1e-5 * rel_scale(ref):.2e}")
    assert e <= 1e-5 * rel_scale(ref)


def _poison(nbytes, times=4):
    """Best effort: blocks of 0xFF bytes (NaN bit patterns), a few times the state buffer's size, allocated and freed -- the
    caching allocator is likely to hand one of them to the forward's torch.empty."""
    blocks = [torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV) for _ in range(times)]
    torch.cuda.synchronize()
    del blocks


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ("stop[64]", "stop[256]", "dots_only"))
def test_state_buffer_full_of_nans(built_lib, c_oracle, name, form):
    """K6 writes no checkpoint for a wave whose pixels have all finished, so K7 must never read one: with the state buffer
    (torch.empty) likely to inherit NaN bit patterns, forward and backward still equal the oracle."""
    from dreamscene_amd import rasterizer as R
    c = _case(name)
    s = settings_for(c["cam"], c["bg"], 0, DEV)
    t = {k: torch.tensor(v, device=DEV) for k, v in c["g"].items()}
    _, st = R.rasterize_forward_raw(s, t["means3D"], t["opacities"], t["shs"], None, t["scales"], t["rotations"], None,
                                    rc=_context(form))
    nbytes = max(int(x.numel()) for x in st.keep[12] if isinstance(x, torch.Tensor))
    torch.cuda.synchronize()
    del st, _
    out, grads = _hip(c, form, before=lambda: _poison(nbytes))
    _check(c, out, grads)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_shallow_scene_after_a_deep_one_in_one_context(built_lib, c_oracle, form):
    """length[769] and then length[65] through the same RasterContext: nothing of the deep scene (checkpoints, work lists,
    tile depths) shows in the shallow one -- outputs bit-equal to a run in a fresh context, gradients by util.same_bits."""
    deep, shallow = _case("length[769]"), _case("length[65]")
    rc = _context(form)
    out, grads = _hip(deep, form, rc=rc)
    _check(deep, out, grads)
    out, grads = _hip(shallow, form, rc=rc)
    _check(shallow, out, grads)
    ref_out, ref_grads = _hip(shallow, form)
    for k in ("color", "depth_alpha", "radii", "final_T", "n_contrib", "ranges", "point_list"):
        assert torch.equal(out[k], ref_out[k]), k
    for hk, _ in GRAD_PAIRS:
        same_bits(grads[hk], ref_grads[hk], hk)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ("length[513]", "pads"))
def test_each_form_twice(built_lib, c_oracle, name, form):
    c = _case(name)
    out1, grads1 = _hip(c, form)
    out2, grads2 = _hip(c, form)
    for k in ("color", "depth_alpha", "radii", "final_T", "n_contrib", "ranges", "point_list"):
        assert torch.equal(out1[k], out2[k]), k
    for hk, _ in GRAD_PAIRS:
        same_bits(grads1[hk], grads2[hk], hk)
