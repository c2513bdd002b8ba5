"""CPU: the seeded point clouds' definition (tests/sample_ref.py, the numpy restatement of SEMANTICS.md section 17) against the
reference's own samplers as tests/golden/samplers.npz records them, and against the analytic distributions; and the host side of
dreamscene_amd.pointcloud (row counts, refusals, the OBJ reader). The device is held to the restatement by
tests/test_pointcloud_gpu.py.

Two samples of one distribution, n and n_ref rows: by the Dvoretzky-Kiefer-Wolfowitz inequality each empirical CDF is within
eps(m) = sqrt(ln(2 / 1e-9) / (2 m)) of the true one except with probability 1e-9, and a recorded quantile q_k has F_ref(q_k) within
1 / n_ref of k / 1024 (the fixture interpolates between order statistics and stores fp32: 1 / 1024 covers both). So
|F_n(q_k) - k / 1024| <= eps(n) + eps(n_ref) + 1 / 1024 for every k. The seeds are fixed, so a pass is a pass for good."""
import math
import os

import numpy as np
import pytest
import torch

from dreamscene_amd import _lib as L
from dreamscene_amd import pointcloud as PC
from dreamscene_amd.model import BasicPointCloud
from tests import noise_ref
from tests import sample_ref as SR

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samplers.npz"))
N = 65_536
SEED = 0x5EED_0123_4567_89AB
ENV_COLOR, FLOOR_COLOR = (135.0, 206.0, 300.0), (120.0, 90.0, 60.0)        # make_samplers_golden.py's


def eps(m: int) -> float:
    return math.sqrt(math.log(2.0 / 1e-9) / (2.0 * m))


def test_the_bar_of_the_analytic_test():
    assert abs(eps(N) - 0.01278) < 5e-6


def around_origin(p, R, disc=False):
    p = np.asarray(p, np.float64)
    r = np.linalg.norm(p, axis=1)
    first = (p[:, 0] ** 2 + p[:, 1] ** 2) / R ** 2 if disc else r ** 3 / R ** 3
    return [p[:, 0], p[:, 1], p[:, 2], first, p[:, 2] / r, np.arctan2(p[:, 1], p[:, 0])]


def against_quantiles(sample, q, n_ref, what):
    """max_k |F_n(q_k) - k / 1024| of the fp32 sample against the recorded quantiles; asserts the DKW bar."""
    sample = np.sort(np.asarray(sample, np.float64))
    F = np.searchsorted(sample, np.asarray(q, np.float64), side="right") / sample.shape[0]
    d = float(np.abs(F - np.arange(1025) / 1024.0).max())
    bar = eps(sample.shape[0]) + eps(n_ref) + 1.0 / 1024.0
    print(f"{what}: {d:.5f} (bar {bar:.5f})")
    assert d <= bar, f"{what}: {d:.5f} > {bar:.5f}"
    return d


def restated(name):
    """The restatement's cloud for a fixture entry, as (list of sheets, each a list of columns), and its colours."""
    kind, method, zg = name.split("_")
    zg = zg == "zg1"
    box, R = GOLD[f"{name}/box"], float(GOLD[f"{name}/R"])
    if kind == "env" and method == "indoor":
        p, c = SR.env_indoor(SEED, box, N)
        return [list(s.T) for s in np.split(p, 5)], c
    if kind == "floor" and method == "indoor":
        p, c = SR.floor_indoor(SEED, box, FLOOR_COLOR, N)
        return [list(p.T)], c
    if kind == "env":
        p, c = SR.env_outdoor(SEED, box, ENV_COLOR, N, zg)
        return [around_origin(p, R)], c
    p, c = SR.floor_outdoor(SEED, box, FLOOR_COLOR, N)
    return [around_origin(p, R, disc=True)], c


CLOUDS = [f"{k}_{m}_zg{z}" for k in ("env", "floor") for m in ("indoor", "outdoor") for z in (0, 1)
          if (k, m, z) != ("floor", "outdoor", 0)]


@pytest.mark.parametrize("name", CLOUDS)
def test_restatement_has_the_reference_s_distribution(name):
    sheets, colors = restated(name)
    q, n_ref = GOLD[f"{name}/q"], int(GOLD[f"{name}/rows"]) // len(sheets)
    assert q.shape[:2] == (len(sheets), len(sheets[0]))
    for s, cols in enumerate(sheets):
        for k, col in enumerate(cols):
            against_quantiles(col, q[s, k], n_ref, f"{name} sheet {s} column {k}")
    ref_colors = GOLD[f"{name}/colors"]
    mine = np.unique(colors, axis=0) if len(sheets) == 1 else np.stack([np.unique(c, axis=0)[0] for c in np.split(colors, 5)])
    assert mine.shape == ref_colors.shape and np.abs(mine - ref_colors).max() <= 1e-7, (mine, ref_colors)


def test_row_counts_grad_flags_and_lr_scales_are_the_reference_s():
    assert int(GOLD["env_indoor_zg0/rows"]) == 5 * PC.ENV_INDOOR_PTS and int(GOLD["floor_indoor_zg0/rows"]) == PC.FLOOR_INDOOR_PTS
    for zg in (0, 1):
        box = GOLD[f"env_outdoor_zg{zg}/box"]
        assert abs(PC.radius_base(box) - float(GOLD[f"env_outdoor_zg{zg}/R"])) < 1e-12
        assert math.ceil(PC.radius_base(box) * PC.ENV_OUTDOOR_DENSITY) == int(GOLD[f"env_outdoor_zg{zg}/rows"])
        assert SR.outdoor_rows(box, PC.ENV_OUTDOOR_DENSITY) == int(GOLD[f"env_outdoor_zg{zg}/rows"])
    box = GOLD["floor_outdoor_zg1/box"]
    assert math.ceil(PC.radius_base(box) * PC.FLOOR_OUTDOOR_DENSITY) == int(GOLD["floor_outdoor_zg1/rows"])
    assert bool(GOLD["floor_outdoor_zg0/raises"])                        # the reference dies there; here: ValueError (below)
    for name in CLOUDS:
        assert bool(GOLD[f"{name}/require_grad"]) == name.startswith("env") and float(GOLD[f"{name}/spatial_lr_scale"]) == 1
    assert float(GOLD["ball/spatial_lr_scale"]) == 10 and bool(GOLD["ball/require_grad"])
    assert float(GOLD["pointe/spatial_lr_scale"]) == 1
    assert int(GOLD["pointe/rows"]) == 4096 * PC.JITTER_COPIES and float(GOLD["pointe/offset_norm_max"]) <= PC.JITTER_RADIUS


def test_indoor_sheets_share_their_coordinates_as_the_reference_s_do():
    assert bool(GOLD["env_indoor_zg0/shared"]) and bool(GOLD["env_indoor_zg1/shared"])
    box = GOLD["env_indoor_zg0/box"]
    p, c = SR.env_indoor(SEED, box, 1000)
    s = np.split(p, 5)
    assert np.array_equal(s[0][:, 1:], s[1][:, 1:]) and np.array_equal(s[2][:, [0, 2]], s[3][:, [0, 2]])
    assert np.array_equal(s[4][:, 0], s[2][:, 0]) and np.array_equal(s[4][:, 1], s[0][:, 1]) and np.array_equal(s[0][:, 2], s[2][:, 2])
    b = box.astype(np.float32)
    assert (s[0][:, 0] <= b[0]).all() and (s[0][:, 0] >= b[0] - np.float32(0.0201)).all()
    assert (s[1][:, 0] >= b[3]).all() and (s[3][:, 1] >= b[4]).all() and (s[4][:, 2] >= b[5]).all() and (s[2][:, 1] <= b[1]).all()
    assert c.shape == p.shape and set(np.unique(c)) == {np.float32(0.5), np.float32(0.7), np.float32(0.9)}
    fp, fc = SR.floor_indoor(SEED, box, FLOOR_COLOR, 1000)
    assert (fp[:, 2] >= b[2] - np.float32(0.0101)).all() and (fp[:, 2] <= b[2] + np.float32(0.0101)).all()
    assert np.array_equal(np.unique(fc, axis=0), SR.colour(FLOOR_COLOR)[None])


def test_ball_has_the_reference_s_distribution():
    R, n_ref = float(GOLD["ball/R"]), int(GOLD["ball/rows"])
    p, c = SR.ball(SEED, N, R)
    for k, col in enumerate(around_origin(p, R)):
        against_quantiles(col, GOLD["ball/q"][0, k], n_ref, f"ball column {k}")
    for ch in range(3):
        against_quantiles(c[:, ch], GOLD["ball/qcolors"][ch], n_ref, f"ball colour {ch}")


def ks_uniform(x) -> float:
    x = np.sort(np.asarray(x, np.float64))
    n = x.shape[0]
    return float(max(np.abs(x - np.arange(1, n + 1) / n).max(), np.abs(x - np.arange(n) / n).max()))


def ball_statistics(p, R):
    p = np.asarray(p, np.float64)
    r = np.linalg.norm(p, axis=1)
    return (ks_uniform(r ** 3 / R ** 3), ks_uniform((p[:, 2] / r + 1.0) / 2.0),
            ks_uniform(np.mod(np.arctan2(p[:, 1], p[:, 0]), 2 * np.pi) / (2 * np.pi)))


@pytest.mark.parametrize("seed", [1, 2, SEED, 2 ** 64 - 1])
def test_ball_against_the_analytic_distributions(seed):
    """|p|^3 / R^3, z / |p| and the azimuth of a uniform ball are uniform. The bar is eps(65 536) = 0.01278; this restatement
    reaches 0.0018 ... 0.0050 over these seeds."""
    stats = ball_statistics(SR.ball(seed, N, 0.5)[0], 0.5)
    print(seed, stats)
    assert max(stats) <= 0.01278, stats


def test_the_analytic_test_tells_wrong_samplers_apart():
    """A radius without the cube root is 0.385 away, a polar angle that is uniform in the angle 0.106."""
    r3, _, _ = ball_statistics(SR.ball(1, N, 0.5, no_cbrt=True)[0], 0.5)
    _, z, _ = ball_statistics(SR.ball(1, N, 0.5, uniform_theta=True)[0], 0.5)
    print(r3, z)
    assert r3 > 0.3 and z > 0.09


def test_jitter_has_the_reference_s_structure():
    seeds, seed_colors = GOLD["pointe/seeds"], GOLD["pointe/seed_colors"]
    assert bool(GOLD["pointe/offsets_shared"])
    base = seeds * np.array([1.0, -1.0, 1.0]) + np.array([0.0, 0.0, 0.15])
    ref_off = GOLD["pointe/points"].reshape(64, 20, 3) - base[:, None, :]          # the row order: seed point major
    assert np.abs(ref_off - ref_off[:1]).max() < 1e-12
    p, c = SR.jitter(SEED, seeds, seed_colors, use_colors=True)
    assert p.shape == (64 * 20, 3) and c.shape == p.shape
    off = p.reshape(64, 20, 3).astype(np.float64) - base[:, None, :]
    assert np.abs(off - off[:1]).max() < 2e-7                                      # fp32 rounding of the sum only
    assert np.abs(off[0] - SR.jitter_offsets(SEED, 20, 0.05)).max() < 2e-7
    assert np.linalg.norm(off[0], axis=1).max() <= 0.05
    delta = (c.astype(np.float64) - np.repeat(seed_colors, 20, axis=0)) / 1e-4
    ref_delta = (GOLD["pointe/point_colors"] - np.repeat(seed_colors, 20, axis=0)) / 1e-4
    assert ref_delta.min() >= 0 and ref_delta.max() <= 1 and delta.min() > -1e-3 and delta.max() < 1 + 1e-3
    u = SR.uniforms(SEED, SR.JITTER_COLORS, np.arange(N), 3)
    for ch in range(3):
        against_quantiles(u[:, ch], GOLD["pointe/qdelta"][ch], 4096 * 20, f"jitter colour delta {ch}")
    _, c2 = SR.jitter(SEED, np.zeros((N // 16, 3)), None, copies=16)
    for ch in range(3):
        against_quantiles(c2[:, ch], GOLD["pointe/qcolors"][ch], 4096 * 20, f"jitter SH colour {ch}")


def test_prefix_property():
    box = GOLD["env_indoor_zg0/box"]
    big, small = SR.env_indoor(SEED, box, 4097), SR.env_indoor(SEED, box, 65)
    for a, b in zip(big, small):
        for sa, sb in zip(np.split(a, 5), np.split(b, 5)):
            assert np.array_equal(sa[:65], sb)
    obox = GOLD["env_outdoor_zg0/box"]
    draws = (lambda n: SR.floor_indoor(SEED, box, FLOOR_COLOR, n), lambda n: SR.env_outdoor(SEED, obox, ENV_COLOR, n, False),
             lambda n: SR.floor_outdoor(SEED, obox, FLOOR_COLOR, n), lambda n: SR.ball(SEED, n, 0.5),
             lambda n: SR.jitter(SEED, np.ones((n, 3)), np.ones((n, 3)), copies=3, use_colors=True))
    for draw in draws:
        for a, b in zip(draw(4097), draw(65)):
            assert np.array_equal(a[:len(b)], b)


def test_cloud_ids_tags_and_seeds_are_independent_streams():
    rows = np.arange(N)
    streams = [SR.uniforms(SEED, cloud, rows, 4) for cloud in range(6)] + [SR.uniforms(SEED + 1, SR.ENV, rows, 4)]
    for a in range(len(streams)):
        for b in range(a + 1, len(streams)):
            assert (streams[a] == streams[b]).mean() < 1e-3
            corr = np.corrcoef(streams[a].reshape(-1), streams[b].reshape(-1))[0, 1]
            assert abs(corr) < 6.0 / math.sqrt(4 * N), (a, b, corr)
    # tag 3 is not the scale noise's (1) or the SH noise's (2) block under the same seed, index, block and stream / cloud word
    from tests.trajectory_ref import _philox4x32_10
    z = np.zeros(64, np.uint64)
    blocks = [np.stack(_philox4x32_10(np.arange(64), z, z + np.uint64(2), z + np.uint64(tag), SEED & 0xFFFFFFFF, SEED >> 32))
              for tag in (0, noise_ref.TAG_SCALE, noise_ref.TAG_SH, SR.TAG_SAMPLE)]
    for a in range(4):
        for b in range(a + 1, 4):
            assert not (blocks[a] == blocks[b]).any()
    u = SR.uniforms(SEED, 0, rows, 9)
    assert u.dtype == np.float32 and u.min() > 0 and u.max() < 1


def test_mesh_restatement_on_a_mesh_with_a_degenerate_triangle():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 2], [0, 2, 0], [5, 0, 0], [0, 0, 1], [1, 0, 0]], np.float64)
    f = np.array([[0, 1, 2], [0, 3, 4], [0, 7, 1], [0, 5, 3]])                  # areas 1, 2, 0 (collinear), 5
    assert np.array_equal(SR.mesh_areas(v, f), np.array([1, 2, 0, 5], np.float32))
    p, c, tri = SR.mesh(SEED, v, f, N)
    assert not (tri == 2).any()
    share = np.bincount(tri, minlength=4) / N
    assert np.abs(np.cumsum(share) - np.array([1, 3, 3, 8]) / 8.0).max() <= eps(N)
    assert np.abs(p.astype(np.float64).mean(axis=0)).max() < 1e-6 and c.min() >= 0.5 and c.max() < 0.5012


# ---- the host side of dreamscene_amd.pointcloud --------------------------------------------------------------------------------

BOX = [-3.5, -2.5, 0.0, 3.5, 2.5, 5.0]


def test_refusals_come_before_any_launch():
    for bad in (0, -5, 2.5):
        with pytest.raises(ValueError):
            PC.sample_ball(bad, 0.5, seed=1)
        with pytest.raises(ValueError):
            PC.sample_env("indoor", BOX, seed=1, num_pts=bad)
        with pytest.raises(ValueError):
            PC.sample_floor("indoor", BOX, seed=1, floor_init_color=FLOOR_COLOR, num_pts=bad)
    for bad_box in ([0, 0, 0, 1, float("nan"), 1], [0, 0, 0, float("inf"), 1, 1], [0, 0, 0, 1, 1]):
        for method in ("indoor", "outdoor"):
            with pytest.raises(ValueError):
                PC.sample_env(method, bad_box, seed=1, env_init_color=ENV_COLOR)
            with pytest.raises(ValueError):
                PC.sample_floor(method, np.array(bad_box), seed=1, zero_ground=True, floor_init_color=FLOOR_COLOR)
    with pytest.raises(ValueError, match="zero_ground"):
        PC.sample_floor("outdoor", BOX, seed=1, zero_ground=False, floor_init_color=FLOOR_COLOR)
    with pytest.raises(ValueError):
        PC.sample_ball(10, float("nan"), seed=1)
    assert PC.sample_env("orbit", BOX, seed=1) is None and PC.sample_floor("orbit", BOX, seed=1) is None


def test_tensors_off_the_device_are_refused():
    with pytest.raises(L.GsrError):
        PC.jitter_cloud(torch.zeros(4, 3), torch.zeros(4, 3), seed=1)
    with pytest.raises(L.GsrError):
        PC.sample_mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), 10, seed=1)
    with pytest.raises(L.GsrError):
        PC.sample_ball(10, 0.5, seed=1, device="cpu")
    gm = PC.SeededGaussianModel({"sh_degree": 0}, "scene")
    with pytest.raises(L.GsrError):
        gm.create_from_cloud(PC.DeviceCloud(torch.zeros(4, 3), torch.zeros(4, 3)))


def test_model_refusals_and_the_empty_model(tmp_path):
    base = {"sh_degree": 0, "init_prompt": "a chair", "use_pointe_rgb": True}
    for mode in ("pointe", "pointe_330k", "pointe_825k"):
        with pytest.raises(ValueError, match="init_points"):
            PC.SeededGaussianModel(dict(base, init_guided=mode), "object", str(tmp_path))
    with pytest.raises(ValueError, match="OBJ"):
        PC.SeededGaussianModel(dict(base, init_guided="shapes", init_prompt="chair.ply"), "object", str(tmp_path))
    with pytest.raises(ValueError, match="obj"):
        PC.SeededGaussianModel(dict(base, init_guided="obj"), "object", str(tmp_path))
    with pytest.raises(ValueError):
        PC.SeededGaussianModel(dict(base, init_guided="default", num_pts=0, radius=0.5), "object", str(tmp_path))
    with pytest.raises(ValueError):
        PC.SeededGaussianModel({"sh_degree": 0, "cam_pose_method": "outdoor", "scene_box": BOX, "zero_ground": False,
                                "floor_init_color": FLOOR_COLOR}, "floor")
    for kind in ("env", "floor"):                                    # the reference's `pass`: an empty model
        gm = PC.SeededGaussianModel({"sh_degree": 0, "cam_pose_method": "orbit", "scene_box": BOX}, kind)
        assert gm._xyz.numel() == 0 and gm.spatial_lr_scale == 0
    assert PC.SeededGaussianModel.seed == 0 and PC.SeededGaussianModel({"sh_degree": 0}, "scene")._seed({"seed": 7}) == 7
    assert issubclass(PC.SeededGaussianModel, PC.GaussianModel) and isinstance(BasicPointCloud([], [], []), tuple)


def test_the_library_refuses_bad_arguments_before_any_hip_call(built_lib):
    lib = built_lib
    p = 0x1000                                                       # aligned, never dereferenced: every call below is refused
    assert lib.gsr_sample_ball(1, 0.5, 0, p, p, None) == -1
    assert lib.gsr_sample_ball(1, 0.5, 10, None, p, None) == -1
    assert lib.gsr_sample_ball(1, 0.5, 10, p + 2, p, None) == -1
    assert lib.gsr_sample_ball(1, float("inf"), 10, p, p, None) == -1
    assert lib.gsr_sample_env_indoor(1, p, 2 ** 31 // 5 + 1, p, p, None) == -1            # 5 n rows overflow the row counter
    assert lib.gsr_sample_env_indoor(1, None, 10, p, p, None) == -1
    assert lib.gsr_sample_floor_indoor(1, p, 0.5, 0.5, 0.5, -1, p, p, None) == -1
    assert lib.gsr_sample_shell(1, float("nan"), 0, 0.5, 0.5, 0.5, 10, p, p, None) == -1
    assert lib.gsr_sample_disc(1, 1.0, float("nan"), 0.5, 0.5, 0.5, 10, p, p, None) == -1
    assert lib.gsr_sample_jitter(1, p, None, 2 ** 20, 2 ** 12, 0.05, p, p, None) == -1
    assert lib.gsr_sample_jitter(1, None, None, 4, 20, 0.05, p, p, None) == -1
    assert lib.gsr_mesh_areas(p, 3, p, 1, p + 4, None) == -1                              # doubles: 8-byte alignment
    assert lib.gsr_sample_mesh(1, p, 3, p, 0, p, 10, p, p, None, None) == -1
    assert lib.gsr_mesh_center(p, 0, p, None) == -1


def test_read_obj(tmp_path):
    path = tmp_path / "m.obj"
    path.write_text("# a comment\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvt 0 0\nf 1 2 3 4\nv 0 0 1\nf -1 1/1/1 2//1\n"
                    "f 1 2 3 4 5\n\ng group\n")
    v, f = PC.read_obj(str(path))
    assert v.shape == (5, 3) and v.dtype == np.float64 and v[4].tolist() == [0, 0, 1]
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    for bad in ("v 0 0 0\nf 1 2 3\n", "v 0 0 0\nv 1 0 0\nv 1 1 0\nf 1 2\n", "v 0 0\n", "v 0 0 0\nf 0 1 1\n", "v 0 0 0\nf -2 1 1\n"):
        path.write_text(bad)
        with pytest.raises(ValueError, match="m.obj"):
            PC.read_obj(str(path))
    path.write_text("# nothing\n")
    v, f = PC.read_obj(str(path))
    assert v.shape == (0, 3) and f.shape == (0, 3)
