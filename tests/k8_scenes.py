"""Scenes for K8's sparse form, built BY WORKGROUP: which rows a view can reach is laid out through tests/k8_layout.py, so that
chosen workgroups of k_preprocess_bwd_views<.., REACHED, KPER> receive exactly the list lengths at which the kernel takes another
path (tests/test_k8_scenes.py checks, on the CPU and from the C oracle's outputs, that they do; tests/test_k8_blocks.py runs them).

k8_scene(P, K, V, seed, pvs) -- everything derives from default_rng(8800 + seed):
  * designated rows: small translucent splats (scale ~0.004, opacity U(0.05, 0.3)) inside the unit-diameter ball: a few pixels
    each, nothing saturates by itself, so whether a view reaches one does not depend on the depth order;
  * every other row has opacity 0.002: it can never pass alpha >= 1/255. 5 % of them stay in place (seen, never blended: the
    statistics of wave_exit), the others have their means multiplied by 40 (mostly culled);
  * a group of 16 large splats at opacity 0.99 (the first rows of a `full` block) sits off-centre towards view 0: in that
    view it saturates a disc in front of designated rows (seen there, not reached: the kernel's `vis && !take`); from the
    opposite side the same rows lie in front of the group;
  * the views orbit at radius 3; with V >= 2 one view (the last but one; the last of two) stands inside the ball (radius 0.3)
    with a narrower lens: part of the designated rows is behind its near plane or off its screen (radii == 0) and reached by the
    other views. With V >= 3 the last view is the one opposite view 0, so some rows are reached by the last view ALONE.
The chosen blocks and their reached counts (PATTERNS; a block's rows in list order = k8_layout.rows_of_block):
  zero        nothing                    one       one row
  slot0..3    64 rows = one whole chunk, on a block with b % 4 = 0..3: the only busy wave is wave 0..3
  n255        255 rows                   n256 / n257   (blocks of 1 024 rows only) one full round / one entry into the second
  full        every row                  sprinkle  every row but one in 97
  last_chunk  only the rows of the block's last live chunk
  tail        the block that owns row P - 1: its final, partial chunk (and nothing else)
From 80 blocks on (the big form; 256-row blocks just below the switch, P = 262 143) there is room for all of them at once; the
nine blocks of P = 2125 take them in two halves (seed even / odd).
"""
import numpy as np

from dreamscene_amd.camera import orbit_camera
from tests import k8_layout as KL

H, W = 80, 96
FOVX = 0.46
SH_C0 = 0.28209479177387814


def plan_blocks(P, seed):
    """-> {block: pattern name}; the blocks not named get random extras."""
    rows, nb, nc = KL.sparse_layout(P)
    tail = int(KL.block_of_row(P, [P - 1])[0])
    if nb >= 80:                          # (room for every pattern at once: the big form, and 256-row blocks just below the switch)
        o = 4 * (2 + seed % 8)            # (a multiple of 4: block o + k has b % 4 = k)
        plan = {o + k: f"slot{k}" for k in range(4)}
        names = ("zero", "one", "n255", "n256", "n257", "full", "sprinkle", "last_chunk", "zero", "full")
        for j, name in enumerate(n for n in names if rows == 1024 or n not in ("n256", "n257")):
            plan[o + 4 + 3 * j + (seed % 3)] = name
        plan[nb - 2] = "last_chunk"       # (a block whose trailing chunk lies past P: its last LIVE chunk is chunk 14)
        assert tail not in plan
        plan[tail] = "tail"
        return plan
    assert nb == 9, "the small form of this builder is laid out for P = 2125"
    if seed % 2 == 0:
        return {0: "slot0", 1: "slot1", 2: "slot2", 3: "slot3", 4: "zero", 5: "one", tail: "tail", 7: "full", 8: "sprinkle"}
    return {0: "n255", 1: "full", 2: "sprinkle", 3: "zero", 4: "one", 7: "last_chunk", 8: "slot0"}   # 5, 6 (the tail): random


def pattern_rows(P, b, name, rng):
    """the rows of block b that pattern `name` designates"""
    r = KL.rows_of_block(P, b)
    c = KL.chunk_of_row(P, r)
    if name == "zero":
        return r[:0]
    if name == "one":
        return r[[int(rng.integers(r.size))]]
    if name.startswith("slot"):
        full = [k for k in np.unique(c) if (c == k).sum() == 64]
        return r[c == full[(5 + 3 * int(name[4])) % len(full)]]
    if name in ("n255", "n256", "n257"):
        return np.sort(rng.choice(r, size=int(name[1:]), replace=False))
    if name == "full":
        return r
    if name == "sprinkle":
        return r[np.arange(r.size) % 97 != 5]
    if name in ("last_chunk", "tail"):
        return r[c == c.max()]
    raise ValueError(name)


def expected_count(P, b, name):
    r = KL.rows_of_block(P, b)
    c = KL.chunk_of_row(P, r)
    return {"zero": 0, "one": 1, "n255": 255, "n256": 256, "n257": 257, "full": r.size,
            "sprinkle": r.size - len(range(5, r.size, 97)), "last_chunk": int((c == c.max()).sum()),
            "tail": int((c == c.max()).sum())}.get(name, 64)


def k8_cameras(V, seed):
    phis = [20.0 + 37.0 * (seed % 5) + 360.0 * j / max(V, 1) for j in range(V)]
    if V >= 3:
        phis.append(phis.pop(V // 2))     # the LAST view looks from the far side of view 0: only it reaches what the group hides there
    cams = [orbit_camera(3.0, 90.0, ph, FOVX, H, W) for ph in phis]
    if V >= 2:
        k = V - 2 if V >= 3 else 1
        cams[k] = orbit_camera(0.3, 90.0, phis[k], 0.3, H, W)
    return cams


def k8_scene(P, K, V, seed, pvs=False):
    """-> (g, cams, designated [P] bool, scales [V,P,3] or None); g: the float32 arrays the rasterizer takes."""
    rng = np.random.default_rng(8800 + seed)
    d = rng.normal(size=(P, 3))
    xyz = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.5 * rng.uniform(size=(P, 1)) ** (1.0 / 3.0))
    scales = 0.004 * np.exp(rng.normal(scale=0.3, size=(P, 3)))
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    shs = rng.normal(scale=0.05, size=(P, K, 3))
    shs[:, 0, :] = (rng.uniform(size=(P, 3)) - 0.5) / SH_C0
    plan = plan_blocks(P, seed)
    des = np.zeros(P, bool)
    for b, name in sorted(plan.items()):
        des[pattern_rows(P, b, name, rng)] = True
    rows, nb, _ = KL.sparse_layout(P)
    free = np.nonzero(~np.isin(KL.block_of_row(P, np.arange(P)), list(plan)))[0]
    extras = rng.choice(free, size=min(3000, int(0.3 * free.size)), replace=False)
    des[extras] = True
    des[(P - 1) // 64 * 64:] = True           # row P - 1 and the whole final partial chunk
    op = np.where(des, rng.uniform(0.05, 0.3, size=P), 0.002)
    rest = np.nonzero(~des)[0]
    far = rest[rng.uniform(size=rest.size) >= 0.05]
    xyz[far] *= 40.0
    cams = k8_cameras(V, seed)
    # the saturating group: towards view 0, a third of the way out
    grp = KL.rows_of_block(P, min(b for b, name in plan.items() if name == "full"))[:16]
    # (on ONE plane across view 0's axis, with the designated rows kept 0.02 clear of it: the views orbit on the equator, so a row
    #  is in front of the whole group either in view 0 or in the view opposite -- no row is lost to every view)
    c0 = np.asarray(cams[0].camera_center, np.float64)
    d0 = c0 / np.linalg.norm(c0)
    s = xyz @ d0 - 0.3
    near = des & (np.abs(s) < 0.02)
    xyz[near] += ((np.where(s >= 0, 0.02, -0.02) - s)[:, None] * d0)[near]
    jit = rng.normal(scale=0.01, size=(grp.size, 3))
    xyz[grp] = 0.3 * d0 + jit - (jit @ d0)[:, None] * d0
    scales[grp] = 0.15 * np.exp(rng.normal(scale=0.05, size=(grp.size, 3)))
    op[grp] = 0.99
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    g = dict(means3D=f(xyz), scales=f(scales), rotations=f(q), opacities=f(op.reshape(P, 1)), shs=f(shs))
    pv = None
    if pvs:
        pv = f(g["scales"][None] * (1.0 + 0.02 * np.sin(1.0 + np.arange(V, dtype=np.float64))).reshape(V, 1, 1))
    return g, cams, des, pv


BG = np.array([0.1, 0.3, 0.9], np.float32)
_CASES = {}


def oracle_case(CO, P, K, D, V, seed, pvs=False):
    """The scene and what the C oracle makes of it, computed once per (P, K, D, V, seed, pvs) and shared (read only!):
    dict(g, cams, des, pv, ups, views=[per view: radii, blended, reached, min_T, dL_dmeans2D, dL_dscales], reached=[V,P] bool,
    sum={name: float64 sum of the parameter gradients over the views})."""
    key = (P, K, D, V, seed, bool(pvs))
    if key in _CASES:
        return _CASES[key]
    from dreamscene_amd import synth
    from tests.util import oracle_view
    g, cams, des, pv = k8_scene(P, K, V, seed, pvs)
    ups = [synth.upstream_grads(H, W, seed=k) for k in range(V)]
    views, total = [], {}
    for j, cam in enumerate(cams):
        sc = pv[j] if pvs else g["scales"]
        v = oracle_view(CO, cam, P, K, D, BG)
        f = CO.forward(v, g["means3D"], g["opacities"], shs=g["shs"], scales=sc, rotations=g["rotations"])
        b = CO.backward(v, f, ups[j][0], ups[j][1], g["means3D"], shs=g["shs"], scales=sc, rotations=g["rotations"])
        for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dshs"):
            total[k] = total.get(k, 0.0) + np.asarray(b[k], dtype=np.float64)
        # (kept per view: only what the tests compare -- a big case's full outputs are 80 MB a view)
        views.append(dict(radii=f["radii"].copy(), blended=blended_rows(f, P), reached=reached_rows(b, P),
                          min_T=float(f["final_T"].min()), dL_dmeans2D=np.asarray(b["dL_dmeans2D"]).copy(),
                          dL_dscales=np.asarray(b["dL_dscales"]).copy() if pvs else None))
    reached = np.stack([v["reached"] for v in views])
    _CASES[key] = dict(g=g, cams=cams, des=des, pv=pv, ups=ups, views=views, reached=reached, sum=total)
    return _CASES[key]


def forget():
    """Drops the cached cases (the test modules call it when they are done: nothing stays with the session)."""
    _CASES.clear()


def blended_rows(f, P):
    """From ONE oracle forward `f` (c_oracle.forward): the rows some pixel blended -- an entry of the pixel's tile list that comes
    before the pixel's last contributor (n_contrib) with power <= 0 and alpha >= 1/255. That is the set the backward walks, found
    without the backward: K7 marks exactly these rows."""
    Hh, Ww = f["final_T"].shape
    gx = (Ww + 15) // 16
    out = np.zeros(P, bool)
    pl, rg = f["point_list"], f["ranges"]
    xy, co = f["xy"], f["conic_opacity"]
    for t in range(rg.shape[0]):
        lo, hi = int(rg[t, 0]), int(rg[t, 1])
        if hi <= lo:
            continue
        ids = pl[lo:hi].astype(np.int64)
        y0, x0 = (t // gx) * 16, (t % gx) * 16
        ys, xs = np.meshgrid(np.arange(y0, min(y0 + 16, Hh)), np.arange(x0, min(x0 + 16, Ww)), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        dx = xy[ids, 0][:, None] - xs[None].astype(np.float32)
        dy = xy[ids, 1][:, None] - ys[None].astype(np.float32)
        a, b, c, o = (co[ids, k][:, None] for k in range(4))
        power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
        alpha = np.minimum(0.99, o * np.exp(power))
        live = np.arange(ids.size)[:, None] < f["n_contrib"][ys, xs][None].astype(np.int64)
        hit = (live & (power <= 0) & (alpha >= 1.0 / 255.0)).any(1)
        out[ids[hit]] = True
    return out


def reached_rows(b, P):
    """From ONE oracle backward `b`: the rows with a non-zero gradient (the colour and opacity sums are never both zero for a
    blended row under a random upstream gradient)."""
    return (np.abs(np.asarray(b["dL_dopacity"]).reshape(P, -1)).sum(1) + np.abs(np.asarray(b["dL_dshs"]).reshape(P, -1)).sum(1)) > 0
