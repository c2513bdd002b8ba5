"""CPU: the host side of dreamscene_amd.compose (rotations, SH band matrices), the reference findings of SEMANTICS.md "Object
placement" as tests, the render invariance of the definition on the float64 oracle, and the C ABI's error paths. The kernels
themselves: tests/test_compose_gpu.py."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import compose_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the case of the issue: a generic unit quaternion, a translation, scale 1
CASE_Q = (0.3, -0.5, 0.7, 0.4)
CASE_T = (1.5, -2.0, 0.7)


def _rotations():
    from dreamscene_amd import compose
    rng = np.random.default_rng(11)
    Rs = [compose.rotation_matrix(rng.normal(size=4)) for _ in range(20)]
    Rs += [np.eye(3), compose.rotation_matrix((90, 0, 0)), compose.rotation_matrix((0, 90, 0)), compose.rotation_matrix((0, 0, 90))]
    return Rs


def _apply_bands(k: torch.Tensor, Ms) -> torch.Tensor:
    """k [P,16,3] -> k' with k'[j] = sum_i k[i] M[i,j] per band (DC unchanged)."""
    out = k.clone()
    for (first, n, _), M in zip(CR.BANDS, Ms):
        out[:, 1 + first:1 + first + n, :] = torch.einsum("pic,ij->pjc", k[:, 1 + first:1 + first + n, :], torch.as_tensor(M))
    return out


def test_band_matrices_rotate_the_colour_function():
    from dreamscene_amd import compose
    from oracle.torch_oracle import eval_sh_color
    rng = np.random.default_rng(5)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = torch.as_tensor(rng.normal(size=(200, 16, 3)))
    worst = 0.0
    for R in _rotations():
        Ms = compose.sh_band_matrices(R)
        a = eval_sh_color(3, _apply_bands(k, Ms), torch.as_tensor(d))          # before the + 0.5 and the clamp
        b = eval_sh_color(3, k, torch.as_tensor(d @ R))                        # rows of d @ R are R^T d
        worst = max(worst, float((a - b).abs().max()))
    print(f"[band matrices] rotated-colour identity: worst {worst:.2e}")
    assert worst <= 1e-12


def test_band_matrices_are_orthogonal_compose_and_fix_the_identity():
    from dreamscene_amd import compose
    Rs = _rotations()
    for R in Rs:
        for M in compose.sh_band_matrices(R):
            assert np.abs(M @ M.T - np.eye(M.shape[0])).max() <= 1e-12
    for M in compose.sh_band_matrices(np.eye(3)):
        assert np.abs(M - np.eye(M.shape[0])).max() <= 1e-12
    # Y((R1 R2)^T d) = M(R2) Y(R1^T d) = M(R2) M(R1) Y(d)
    for R1, R2 in zip(Rs[:8], Rs[8:16]):
        for M12, M1, M2 in zip(compose.sh_band_matrices(R1 @ R2), compose.sh_band_matrices(R1), compose.sh_band_matrices(R2)):
            assert np.abs(M12 - M2 @ M1).max() <= 1e-12
    # no random state: the same input gives the same bits
    a, b = compose.sh_band_matrices(Rs[3]), compose.sh_band_matrices(Rs[3].copy())
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_rotation_matrix_and_quaternion_of():
    from dreamscene_amd import compose
    a, b, c = 25.0, -40.0, 110.0
    ra, rb, rc = (math.radians(v) for v in (a, b, c))
    Rx = np.array([[1, 0, 0], [0, math.cos(ra), -math.sin(ra)], [0, math.sin(ra), math.cos(ra)]])
    Ry = np.array([[math.cos(rb), 0, math.sin(rb)], [0, 1, 0], [-math.sin(rb), 0, math.cos(rb)]])
    Rz = np.array([[math.cos(rc), -math.sin(rc), 0], [math.sin(rc), math.cos(rc), 0], [0, 0, 1]])
    R = compose.rotation_matrix((a, b, c))
    assert R.dtype == np.float64 and np.abs(R - Rx @ Ry @ Rz).max() <= 1e-15
    assert np.abs(compose.rotation_matrix((0, 0, 90)) @ np.array([1.0, 0, 0]) - np.array([0, 1.0, 0])).max() <= 1e-15
    rng = np.random.default_rng(2)
    for _ in range(20):
        q = rng.normal(size=4)
        Rq = compose.rotation_matrix(q)
        assert np.abs(Rq @ Rq.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(Rq) - 1) <= 1e-14
        for s in (1e-3, 7.0, -2.5):                                     # any non-zero length; -q is the same rotation
            assert np.abs(compose.rotation_matrix(s * q) - Rq).max() <= 1e-14
        u = compose.quaternion_of(Rq)
        want = q / np.linalg.norm(q) * (1 if q[0] >= 0 else -1)
        assert u[0] >= 0 and abs(np.linalg.norm(u) - 1) <= 1e-15 and np.abs(u - want).max() <= 1e-14
    for q in ((0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 0, 0), (0, 0.6, 0.8, 0)):      # half turns: w = 0
        u = compose.quaternion_of(compose.rotation_matrix(q))
        assert np.abs(np.abs(u) - np.abs(np.asarray(q, dtype=np.float64))).max() <= 1e-15 and u[0] >= 0
        assert np.abs(compose.rotation_matrix(u) - compose.rotation_matrix(q)).max() <= 1e-15
    with pytest.raises(ValueError):
        compose.rotation_matrix((0, 0, 0, 0))
    with pytest.raises(ValueError):
        compose.rotation_matrix((1, 2))


def test_reference_band_1_mixes_the_colour_axis():
    """scene_gaussian.py:303-316 / :357-360: transform_SHs is handed features_rest[:, :3, :], laid out [N, coefficient, rgb], and
    multiplies from the right: the COLOUR axis is mixed. The same formula on the coefficient axis with R^T is the render-preserving
    map (SEMANTICS.md "Object placement")."""
    from dreamscene_amd import compose
    rng = np.random.default_rng(9)
    R = compose.rotation_matrix(CASE_Q)
    M1 = compose.sh_band_matrices(R)[0]
    # v_to_sh of the reference: the band-1 basis is C1 * (d @ V), V a signed permutation (here derived from the basis itself)
    V = compose._sh_bands(np.eye(3))[0] / compose._C1
    assert np.array_equal(np.abs(V).sum(0), np.ones(3)) and np.array_equal(np.abs(V).sum(1), np.ones(3))
    k = rng.normal(size=(500, 3, 3))                                   # [N, coefficient, rgb]
    want = np.einsum("pic,ij->pjc", k, M1)
    as_executed = k @ (V.T @ R @ V)                                    # torch.bmm(shs, transforms): the last axis is rgb
    on_coefficients = np.swapaxes(np.swapaxes(k, 1, 2) @ (V.T @ R.T @ V), 1, 2)
    e_exec, e_coef = np.abs(as_executed - want).max(), np.abs(on_coefficients - want).max()
    print(f"[band 1] reference as executed: {e_exec:.2f} off; on the coefficient axis with R^T: {e_coef:.1e}")
    assert e_exec > 1.0
    assert e_coef <= 1e-14


def _case_400():
    from dreamscene_amd import synth
    g = synth.g_object(400, seed=3, K=16)
    cam = synth.object_cameras(4, 64, 64)[1]
    return g, cam


def invariance_pair(g, cam, rotation, scale, t, dtype, renormalise=True):
    """Oracle renders of (object, cam) and (placed object, moved camera) in `dtype`; the placement in float64 by compose_ref."""
    from oracle import torch_oracle as TO
    raw = CR.raw_leaves(g)
    if renormalise:
        raw["rotation"] = raw["rotation"] / np.linalg.norm(raw["rotation"], axis=1, keepdims=True)
    c = CR.constants(rotation, [scale], (0, 0, 0), fp32=False)
    ref = CR.place_ref(raw["xyz"], raw["scaling"], raw["rotation"], raw["f_rest"], c, ground=False, t_effective=t)
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    bg = [1.0, 1.0, 1.0]

    def render(xyz, scaling, rot, f_rest, settings):
        shs = torch.cat((T(raw["f_dc"]), T(f_rest)), dim=1)
        out, aux = TO.rasterize(T(xyz), torch.zeros((xyz.shape[0], 3), dtype=dtype), T(sig(raw["opacity"])), shs=shs,
                                scales=torch.exp(T(scaling)), rotations=T(rot), settings=settings, return_aux=True)
        return out[0].numpy(), out[1].numpy(), out[2].numpy(), aux["n_contrib"]
    a = render(raw["xyz"], raw["scaling"], raw["rotation"], raw["f_rest"], CR.oracle_settings(cam, bg, 3, dtype))
    moved = CR.moved_camera(cam, rotation, scale, t)
    b = render(ref["xyz"].numpy(), ref["scaling64"].numpy(), ref["rotation"].numpy(), ref["f_rest"].numpy(),
               CR.oracle_settings(cam, bg, 3, dtype, moved))
    return a, b


def test_placed_object_renders_as_the_original_from_the_moved_camera():
    """The definition end to end, oracle only: case of the issue (400 Gaussians, 64 x 64, degree 3, white background)."""
    g, cam = _case_400()
    a, b = invariance_pair(g, cam, CASE_Q, 1.0, CASE_T, torch.float64)
    e_img, e_da = np.abs(a[0] - b[0]).max(), np.abs(a[2] - b[2]).max()
    a32, b32 = invariance_pair(g, cam, CASE_Q, 1.0, CASE_T, torch.float32)
    f_img, f_da = np.abs(a32[0] - b32[0]).max(), np.abs(a32[2] - b32[2]).max()
    print(f"[invariance] float64: image {e_img:.2e}, depth_alpha {e_da:.2e}; float32: image {f_img:.2e}, depth_alpha {f_da:.2e}; "
          f"visible {int((a[1] > 0).sum())} of 400")
    assert int((a[1] > 0).sum()) >= 300 and float(np.abs(a[0] - 1.0).max()) > 0.2       # the picture is not empty
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert e_img <= 1e-9 and e_da <= 1e-9
    assert np.array_equal(a32[1], b32[1])


def test_place_abi_without_gpu(built_lib):
    from dreamscene_amd import _lib
    lib = built_lib
    sizes = [lib.gsr_place_scratch_bytes(P) for P in (0, 1, 255, 256, 257, 100_003, 1_200_000, 3_000_000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert lib.gsr_place_scratch_bytes(-1) == 0 and lib.gsr_place_scratch_bytes(2 ** 31 - 1) == 0
    assert lib.gsr_place(None, None, 0, None) == -1
    # host memory stands in for the device: every refusal below happens before any HIP call
    P = 10
    buf = [np.zeros(64, dtype=np.float32) for _ in range(12)]
    scratch = np.zeros(4096, dtype=np.uint8)
    al = lambda a: (a.ctypes.data + 15) & ~15

    def fresh(K=16):
        p = _lib.GsrPlacement()
        p.P, p.K = P, K
        big = [np.zeros(P * 45 + 8, dtype=np.float32) for _ in range(2)]
        buf.extend(big)
        p.xyz, p.scaling, p.rotation, p.opacity, p.features_dc, p.features_rest = (al(buf[0]), al(buf[1]), al(buf[2]), al(buf[3]),
                                                                                  al(buf[4]), al(big[0]))
        p.xyz_out, p.scaling_out, p.rotation_out, p.features_rest_out = al(buf[5]), al(buf[6]), al(buf[7]), al(big[1])
        p.bounds, p.t_effective = al(buf[8]), al(buf[9])
        return p
    sp, sb = al(scratch), lib.gsr_place_scratch_bytes(P)
    p = fresh(K=5)
    assert lib.gsr_place(ctypes.byref(p), sp, sb, None) == -1
    for field in ("xyz_out", "scaling_out", "rotation_out", "features_rest_out", "xyz", "bounds"):
        p = fresh()
        setattr(p, field, None)
        assert lib.gsr_place(ctypes.byref(p), sp, sb, None) == -1, field
    p = fresh()
    assert lib.gsr_place(ctypes.byref(p), sp, sb - 1, None) == -1           # too small a scratch
    assert lib.gsr_place(ctypes.byref(p), None, sb, None) == -1
    p = fresh()
    p.xyz_out = p.scaling                                                   # an output on another input
    assert lib.gsr_place(ctypes.byref(p), sp, sb, None) == -1
    p = fresh()
    p.xyz_out = p.xyz + 16                                                  # overlapping its own input, but not in place
    assert lib.gsr_place(ctypes.byref(p), sp, sb, None) == -1
    p = fresh()
    p.scaling_out = p.xyz_out                                               # two outputs on one buffer
    assert lib.gsr_place(ctypes.byref(p), sp, sb, None) == -1
    p = fresh()
    p.xyz += 4                                                              # not 16-byte aligned
    assert lib.gsr_place(ctypes.byref(p), sp, sb, None) == -1
    p = fresh()
    p.P = 0                                                                 # nothing to do, nothing launched
    assert lib.gsr_place(ctypes.byref(p), sp, sb, None) == 0
    # the ctypes mirror has the C compiler's size
    src = '#include <stdio.h>\n#include "gsrast.h"\nint main(){ printf("%zu\\n", sizeof(GsrPlacement)); return 0; }\n'
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(tmp, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        assert int(subprocess.check_output([exe])) == ctypes.sizeof(_lib.GsrPlacement)
    out = subprocess.run(["strings", "-n", "6", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "k_place_bounds" in out and "k_place_apply" in out


def test_place_host_side_errors(built_lib):
    from dreamscene_amd import compose
    from dreamscene_amd._lib import GsrError
    P = 8
    cpu = (torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 4), torch.zeros(P, 1), torch.zeros(P, 1, 3), torch.zeros(P, 15, 3))
    with pytest.raises(GsrError):                                           # no CPU fallback
        compose.place(cpu, (0, 0, 0), [1.0], (0, 0, 0))
    with pytest.raises(ValueError):
        compose.place(cpu, (0, 0, 0), [1.0, 2.0], (0, 0, 0))
    with pytest.raises(ValueError):
        compose.place(cpu, (0, 0, 0), [0.0], (0, 0, 0))
    with pytest.raises(ValueError):
        compose.add_objects_to_scene([])


def test_the_product_does_not_import_the_checker():
    for dp, _, fs in os.walk(os.path.join(ROOT, "dreamscene_amd")):
        for f in fs:
            if f.endswith(".py"):
                assert "compose_ref" not in open(os.path.join(dp, f)).read(), f
