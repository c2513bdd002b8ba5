"""Constructed scenes for tests/test_tile_lists.py: tile lists whose LENGTHS, STOP POINTS and per-block REACH are set by design
(plain numpy, no GPU). The compositing kernels K6 (csrc/render_fwd.hip) and K7 (csrc/render_bwd.hip) turn on a handful of integer
boundaries -- the 256-entry staging batch, the checkpoint distance GsrBinning.seg_len (64 / 128 / 256), the quad of four
consecutive candidates of K6, K7's (tile, segment) items, the per-wave block test -- which seeded random clouds reach only by
accident. Two building blocks:

  sheets   isotropic Gaussians ON the optical axis of synth.object_cameras(1, H, W, radius=3.0)[0] at distinct depths: every
           sheet is in every tile's list (3 sigma covers the image), so every list is exactly as long as there are sheets, and the
           alpha falloff across the image spreads the T < 1e-4 stops over tens of list positions;
  dots     tiny Gaussians (the 0.3 px low-pass leaves sigma = 0.55 px, radius 2 px) unprojected to the centre of one 4x4 pixel
           block (x0 + 1.5, y0 + 1.5): they reach that block only (2.5 px to the nearest pixel of a neighbour: q = 20.8 > tau <= 11.1).

A scene is a list of such entries IN DEPTH ORDER (front to back); build() spreads them over [-0.2, 0.2] around the origin along
the axis and shuffles the Gaussian indices, so that list order differs from index order. Every named case returns
(g, cam, bg, expectations); what a case claims is asserted from the C oracle's outputs by test_cases_reach_what_they_claim
(CPU), so a case that drifts fails loudly."""
from __future__ import annotations

import numpy as np

from dreamscene_amd import synth

H_IMG, W_IMG = 40, 56          # 3 x 4 tiles; the last tile row has 8 pixel rows, the last tile column 8 pixel columns
RADIUS = 3.0
DEPTH_SPAN = 0.2
SHEET_SCALE = 0.5
DOT_SCALE = 1e-3
SH_C0 = 0.28209479177387814
T_MIN = 1e-4
ALPHA_MIN = 1.0 / 255.0

LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 769)
STOPS = (64, 128, 192, 256, 512)


def stop_opacity(L, frac=0.8):
    """The opacity at which a pixel on the axis falls below T = 1e-4 after frac * L sheets."""
    return float(1.0 - T_MIN ** (1.0 / (frac * L)))


def camera(H=H_IMG, W=W_IMG):
    return synth.object_cameras(1, H, W, radius=RADIUS)[0]


def sheet(opacity, scale=SHEET_SCALE, at=None):
    """at = None: on the optical axis; (px, py): centred on that pixel position."""
    return dict(kind="sheet", opacity=float(opacity), scale=float(scale), at=at)


def dot(px0, py0, opacity=0.05):
    """A dot over the centre of the 4x4 pixel block with origin (px0, py0) (image coordinates, multiples of 4)."""
    return dict(kind="dot", opacity=float(opacity), scale=DOT_SCALE, at=(px0 + 1.5, py0 + 1.5))


def build(entries, cam, seed=0):
    """entries: front to back. -> g (K = 1: DC colours only, D = 0) with shuffled Gaussian indices, and `order`: order[k] = the
    Gaussian index of entry k."""
    P = len(entries)
    rng = np.random.default_rng(9000 + seed)
    wvt = cam.world_view_transform.astype(np.float64)
    right, down, fwd = wvt[:3, 0], wvt[:3, 1], wvt[:3, 2]        # the camera's axes in world coordinates
    eye = cam.camera_center.astype(np.float64)
    z0 = float(np.linalg.norm(eye))                               # the camera looks at the origin: depth of the origin
    t = np.linspace(-DEPTH_SPAN, DEPTH_SPAN, P) if P > 1 else np.zeros(1)
    W, H = cam.image_width, cam.image_height
    means = np.zeros((P, 3))
    for k, e in enumerate(entries):
        z = z0 + t[k]
        x = y = 0.0
        if e["at"] is not None:
            # pixel = ((ndc + 1) size - 1) / 2  <=>  ndc = (2 pixel + 1) / size - 1; view-space x = ndc tanfov z
            x = ((2.0 * e["at"][0] + 1.0) / W - 1.0) * cam.tanfovx * z
            y = ((2.0 * e["at"][1] + 1.0) / H - 1.0) * cam.tanfovy * z
        means[k] = eye + z * fwd + x * right + y * down
    order = rng.permutation(P)
    g = dict(means3D=np.zeros((P, 3), np.float32), scales=np.zeros((P, 3), np.float32),
             rotations=np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (P, 1)), opacities=np.zeros((P, 1), np.float32),
             shs=((rng.uniform(size=(P, 1, 3)) - 0.5) / SH_C0).astype(np.float32))
    g["means3D"][order] = means.astype(np.float32)
    g["scales"][order] = np.array([[e["scale"]] * 3 for e in entries], np.float32).reshape(P, 3)
    g["opacities"][order] = np.array([e["opacity"] for e in entries], np.float32).reshape(P, 1)
    return g, order


def sheets(L, opacity, scale=SHEET_SCALE, H=H_IMG, W=W_IMG, seed=0):
    cam = camera(H, W)
    g, order = build([sheet(opacity, scale) for _ in range(L)], cam, seed)
    return g, cam, order


def dots(blocks, cam, opacity=0.05, seed=0):
    """One dot per entry of blocks (4x4 block origins, front to back); opacity: one value or one per dot."""
    op = np.broadcast_to(np.asarray(opacity, np.float64), (len(blocks),))
    g, order = build([dot(x0, y0, o) for (x0, y0), o in zip(blocks, op)], cam, seed)
    return g, order


# ------------------------------------------------------------------------------------------------------------- float64 helpers
def reach64(xy, conic_opacity, bx, by, w1):
    """block_reach of csrc/gsr_render.h in float64, for every Gaussian at once: can the splat pass the alpha gate anywhere on
    the w1 x w1 pixel block with origin (bx, by)? Minimum of q(d) = A dx^2 + 2 B dx dy + C dy^2 over the block's rectangle (in
    d = centre - pixel) against tau = 2 ln(255 opacity) (preprocess.hip's splat_tau, with its inflation). -> bool [P]"""
    xy = np.asarray(xy, np.float64)
    co = np.asarray(conic_opacity, np.float64)
    A, B, C, op = co[:, 0], co[:, 1], co[:, 2], co[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.where(op * 255.0 > 1.0, 2.0 * np.log(np.maximum(op * 255.0, 1e-300)) * 1.0001 + 0.001, -1.0)
        dx1, dy1 = xy[:, 0] - bx, xy[:, 1] - by
        dx0, dy0 = dx1 - (w1 - 1), dy1 - (w1 - 1)
        med = lambda lo, v, hi: np.minimum(np.maximum(v, lo), hi)
        ex, ey = med(dx0, 0.0, dx1), med(dy0, 0.0, dy1)
        y = med(dy0, -B / C * ex, dy1)
        q1 = A * ex * ex + (2.0 * B * ex + C * y) * y
        x = med(dx0, -B / A * ey, dx1)
        q2 = C * ey * ey + (2.0 * B * ey + A * x) * x
        return (tau >= 0.0) & (np.minimum(q1, q2) <= tau)


def tile_list(f, cam, ty, tx):
    """Gaussian ids of tile (ty, tx) in list order."""
    gx = (cam.image_width + 15) // 16
    a, b = f["ranges"][ty * gx + tx]
    return f["point_list"][int(a):int(b)].astype(np.int64)


def chunk_reach_counts(f, cam, ty, tx, w1, chunk):
    """-> int [n_chunks, 16 / w1, 16 / w1]: per chunk of `chunk` consecutive entries of tile (ty, tx)'s list and per w1 x w1 block of
    the tile (block row, block column), the number of entries that reach the block (reach64)."""
    ids = tile_list(f, cam, ty, tx)
    nb = 16 // w1
    n_chunks = (len(ids) + chunk - 1) // chunk
    out = np.zeros((n_chunks, nb, nb), np.int64)
    for br in range(nb):
        for bc in range(nb):
            r = reach64(f["xy"][ids], f["conic_opacity"][ids], 16 * tx + w1 * bc, 16 * ty + w1 * br, w1)
            for c in range(n_chunks):
                out[c, br, bc] = int(r[c * chunk:(c + 1) * chunk].sum())
    return out


def stopped_mask(f, cam):
    """Pixels that left through the T < 1e-4 stop: the entry after their last contributor (n_contrib counts list positions, so
    it is entry number n_contrib, 0-based) passes the alpha gate and takes T below the threshold. float64 from the oracle's xy /
    conic_opacity / final_T: a classification for the coverage report, not a parity artefact. -> bool [H, W]"""
    H, W = cam.image_height, cam.image_width
    gx = (W + 15) // 16
    out = np.zeros((H, W), bool)
    for py in range(H):
        for px in range(W):
            a, b = f["ranges"][(py // 16) * gx + px // 16]
            n = int(f["n_contrib"][py, px])
            # the stop is taken ON an entry behind the last contributor: the first one behind it that passes the alpha gate
            for pos in range(int(a) + n, int(b)):
                i = int(f["point_list"][pos])
                dx, dy = float(f["xy"][i, 0]) - px, float(f["xy"][i, 1]) - py
                A, B, C, op = (float(v) for v in f["conic_opacity"][i])
                power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
                alpha = min(0.99, op * np.exp(power))
                if power > 0.0 or alpha < ALPHA_MIN:
                    continue
                out[py, px] = float(f["final_T"][py, px]) * (1.0 - alpha) < T_MIN
                break
    return out


# ------------------------------------------------------------------------------------------------------------------ named cases
BG = np.array([0.2, 0.7, 1.0], np.float32)

# stop[B]: (number of sheets L, their opacity, their scale) -- tuned on the CPU (C oracle) so that the T < 1e-4 stops put
# n_contrib on every value of [B - 4, B + 4], and small enough sheets that the pixels of the bottom corner tiles (2, 0) and
# (2, 3) take none of them: those two tiles' depths are then pinned by dots -- the last dot of tile (2, 0) is entry B of its
# list (behind B - 1 sheets and earlier dots), the last dot of tile (2, 3) entry B + 1.
STOP_AT = (12.3, 9.2)       # the sheets' centre: off the axis (and off the pixel grid's symmetry: four times as many stop values)
STOP_TAIL = 40              # sheets behind entry B
STOP_PARAMS = {64: (0.14407424666813157, 0.35), 128: (0.07166483371507033, 0.40), 192: (0.048921678939885624, 0.45),
               256: (0.03594689278774789, 0.45), 512: (0.01796365083265533, 0.50)}
STOP_PIN_B = ((2, 0), (4, 36))        # (tile, block origin): the tile whose depth is exactly B
STOP_PIN_B1 = ((2, 3), (52, 36))      # ... exactly B + 1
STOP_PIN_DOTS = 12


def _with_dots_at(n_sheets, make_sheet, per_tile):
    """n_sheets sheets and, for every (block origin, 1-based positions in ITS tile's list, opacity) of per_tile, dots at those
    positions of that tile's list (a tile's list = all the sheets + its own dots). -> entries front to back"""
    keyed = [(k + 0.5, make_sheet()) for k in range(n_sheets)]
    for t, (origin, positions, opacity) in enumerate(per_tile):
        for j, p in enumerate(sorted(positions)):
            assert p - 1 - j <= n_sheets
            keyed.append((p - 1 - j + 0.01 * (j + 1) / (len(positions) + 1) + 0.001 * t, dot(*origin, opacity=opacity)))
    return [e for _, e in sorted(keyed, key=lambda ke: ke[0])]


def case_length(L, H=H_IMG, W=W_IMG):
    """L sheets at the opacity that stops the axis pixel at 0.8 L. (L = 1: alpha <= 0.99 leaves T = 0.01 -- no pixel can stop.)"""
    g, cam, order = sheets(L, stop_opacity(L), H=H, W=W, seed=L)
    return g, cam, BG, dict(kind="length", L=L, some_stopped=L >= 2)


def case_stop(B):
    """B + 40 sheets whose T < 1e-4 stops cover [B - 4, B + 4], and two tiles whose depth is pinned to B and B + 1 by dots."""
    opacity, scale = STOP_PARAMS[B]
    cam = camera()
    rng = np.random.default_rng(100 + B)
    pins = []
    for (tile, origin), last in ((STOP_PIN_B, B), (STOP_PIN_B1, B + 1)):
        pos = set(int(p) for p in rng.choice(np.arange(1, last), size=STOP_PIN_DOTS - 1, replace=False)) | {last}
        pins.append((origin, pos, 0.3))
    entries = _with_dots_at(B + STOP_TAIL, lambda: sheet(opacity, scale, STOP_AT), pins)
    g, order = build(entries, cam, seed=B)
    return g, cam, BG, dict(kind="stop", B=B, depth_B=STOP_PIN_B[0], depth_B1=STOP_PIN_B1[0])


def case_opaque():
    g, cam, order = sheets(769, 1.0, seed=1)
    return g, cam, BG, dict(kind="opaque", L=769)


def case_transparent():
    g, cam, order = sheets(257, 0.003, seed=2)
    return g, cam, BG, dict(kind="transparent", L=257)


PADS_TILE = (1, 1)
PADS_QUARTER = ((24, 24), (28, 24), (24, 28), (28, 28))     # the four 4x4 blocks of quarter 3 of tile (1, 1): K6's waves 0 .. 3
PADS_DOTS = ((0, 1, 2, 3), (0, 2, 0, 2), (1, 0, 2, 0), (0, 0, 0, 0), (3, 1, 0, 2))     # dots per block in the list's 64-entry chunks
PADS_LEN = 330


def case_pads():
    """Tile (1, 1): sheets (they reach every block) and, in each of the first 64-entry chunks of its list, a different number of
    dots over each 4x4 block of its quarter 3 -- the candidate counts of K6's four waves there differ mod 4 at the first seg_len-64
    cut (58 + 0 .. 3) and at the seg_len-128 cut (118 + 0, 3, 2, 5)."""
    cam = camera()
    rng = np.random.default_rng(77)
    opacity = stop_opacity(PADS_LEN)
    entries = []
    for c in range((PADS_LEN + 63) // 64):
        n = min(64, PADS_LEN - 64 * c)
        per_block = PADS_DOTS[c] if c < len(PADS_DOTS) else (0, 0, 0, 0)
        chunk = [sheet(opacity) for _ in range(n - sum(per_block))]
        for origin, k in zip(PADS_QUARTER, per_block):
            chunk += [dot(*origin, opacity=0.05) for _ in range(k)]
        entries += [chunk[i] for i in rng.permutation(len(chunk))]
    g, order = build(entries, cam, seed=3)
    return g, cam, BG, dict(kind="pads", L=PADS_LEN)


DOTS_TILE = (1, 1)
DOTS_OWNER, DOTS_OPPOSITE = (20, 20), (24, 24)     # blocks (1, 1) and (2, 2) of the tile's 4 x 4 blocks: quarters / 8x8 blocks 0 and 3
DOTS_LEN = 320
DOTS_MOVED = (64, 128)                             # the run of entries (depth order) that sits over the opposite block


def case_dots_only():
    """320 dots and no sheet, all in tile (1, 1)'s list: over one 4x4 block, except that entries 64 .. 127 sit over the diagonally
    opposite block -- 14 of the tile's 16 blocks (K6's waves) and two of its four 8x8 blocks (K7's) are reached by nothing in
    either batch, the owner has no candidate in the second 64-entry chunk and the opposite block none in any other."""
    cam = camera()
    rng = np.random.default_rng(78)
    blocks = [DOTS_OPPOSITE if DOTS_MOVED[0] <= k < DOTS_MOVED[1] else DOTS_OWNER for k in range(DOTS_LEN)]
    g, order = dots(blocks, cam, opacity=rng.uniform(0.02, 0.08, size=DOTS_LEN), seed=4)
    return g, cam, BG, dict(kind="dots_only", L=DOTS_LEN)


def case_ragged():
    g, cam, bg, ex = case_length(257, H=17, W=17)
    return g, cam, bg, dict(ex, kind="ragged")


def names():
    return [f"length[{L}]" for L in LENGTHS] + [f"stop[{B}]" for B in STOPS] + ["opaque", "transparent", "pads", "dots_only",
                                                                               "ragged"]


def case(name):
    """-> (g, cam, bg, expectations) of a named case."""
    if name.startswith("length["):
        return case_length(int(name[7:-1]))
    if name.startswith("stop["):
        return case_stop(int(name[5:-1]))
    return dict(opaque=case_opaque, transparent=case_transparent, pads=case_pads, dots_only=case_dots_only,
                ragged=case_ragged)[name]()
