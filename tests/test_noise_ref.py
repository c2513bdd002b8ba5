"""Seeded augmentation noise (SEMANTICS.md "Seeded noise"), without a device: the statistics and the layout properties of the
numpy restatement (tests/noise_ref.py), the argument checks of the Python interface, and the GSR_EINVAL answers of the C ABI
that precede any HIP call."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import noise_ref as NR

N = 50_000                      # rows = samples per column
SEEDS = (12345, 0, 2 ** 64 - 1)
KS = (1, 4, 9, 16)


@pytest.fixture(scope="module")
def samples():
    """(seed, K) -> (SH stream 7, SH stream 8, scale stream 7), each [N, columns], computed once."""
    out = {}
    for seed, K in itertools.product(SEEDS, KS):
        out[seed, K] = (NR.sh_noise(seed, N, K, 7).reshape(N, -1), NR.sh_noise(seed, N, K, 8).reshape(N, -1),
                        NR.scale_noise(seed, N, 7))
    return out


@pytest.mark.parametrize("seed,K", list(itertools.product(SEEDS, KS)))
def test_columns_are_standard_normal_and_uncorrelated(samples, seed, K):
    """Bars in units of the estimators' standard deviations at n = 50 000: mean 5, variance 5, correlation 6 (the worst
    cases of this layout are 2.4, 3.2 and 4.1)."""
    a, b, s = samples[seed, K]
    cols = np.concatenate([a, b, s], 1).astype(np.float64)
    assert np.isfinite(cols).all()
    worst_mean = np.abs(cols.mean(0)).max() * N ** 0.5
    worst_var = np.abs(cols.var(0) - 1.0).max() / (2.0 / N) ** 0.5
    c = np.corrcoef(cols.T)
    np.fill_diagonal(c, 0.0)
    worst_corr = np.abs(c).max() * N ** 0.5
    print(f"[noise_ref] seed {seed} K {K}: mean {worst_mean:.2f}, var {worst_var:.2f}, corr {worst_corr:.2f} sigma")
    assert worst_mean < 5.0
    assert worst_var < 5.0
    assert worst_corr < 6.0


def test_layout_properties(samples):
    seed = SEEDS[0]
    a16, b16, s = samples[seed, 16]
    a4 = samples[seed, 4][0]
    # a row depends on neither P nor where the call starts
    assert np.array_equal(NR.sh_noise(seed, 100, 16, 7).reshape(100, -1), a16[:100])
    assert np.array_equal(NR.sh_noise(seed, 50, 16, 7, first=300).reshape(50, -1), a16[300:350])
    assert np.array_equal(NR.scale_noise(seed, 64, 7, first=1000), s[1000:1064])
    # K = 4 is the prefix of K = 16; the K = 9 row ends inside a block
    assert np.array_equal(a4, a16[:, :12])
    assert np.array_equal(samples[seed, 9][0], a16[:, :27])
    # two streams differ; tag 1, block 0 differs from tag 2, block 0
    assert not np.array_equal(a16, b16)
    assert (a16 != b16).mean() > 0.99
    assert (s != a16[:, :3]).mean() > 0.99
    # |n| <= sqrt(-2 ln 2^-25)
    assert np.abs(np.concatenate([a16, b16, s], 1)).max() <= 5.89


def test_noise_spec_validation():
    from dreamscene_amd import scene
    sp = scene.NoiseSpec(3, 4)
    assert (sp.seed, sp.stream, sp.scales, sp.shs) == (3, 4, True, True)
    with pytest.raises(Exception):      # frozen
        sp.seed = 5
    scene.NoiseSpec(2 ** 64 - 1, 2 ** 32 - 1, scales=False)
    scene.NoiseSpec(0, torch.zeros(1, dtype=torch.int32))
    for bad in [dict(seed=-1, stream=0), dict(seed=2 ** 64, stream=0), dict(seed=1.5, stream=0), dict(seed=0, stream=-1),
                dict(seed=0, stream=2 ** 32), dict(seed=0, stream=0.5), dict(seed=0, stream=torch.zeros(1)),
                dict(seed=0, stream=torch.zeros((1, 1), dtype=torch.int32)), dict(seed=0, stream=0, scales=1)]:
        with pytest.raises(ValueError):
            scene.NoiseSpec(**bad)


def _cpu_model(n=8, K=4):
    z = lambda *s: torch.zeros(s)
    return (z(n, 3), z(n, 3), z(n, 4), z(n, 1), z(n, 1, 3), z(n, K - 1, 3))


def test_noise_arguments_raise_value_error():
    """A noise named by the spec AND given as a tensor, a spec of the wrong kind or count: ValueError before anything runs."""
    from dreamscene_amd import scene
    from dreamscene_amd.rasterizer import GaussianRasterizationSettings
    m, P, K = _cpu_model(), 8, 4
    s = GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                      scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=1,
                                      campos=torch.zeros(3), prefiltered=False, score_flag=False)
    m2d = torch.zeros(P, 3)
    sp = scene.NoiseSpec(1, 2)
    with pytest.raises(ValueError):
        scene.rasterize_models(s, [m], m2d, scale_noise=torch.zeros(P, 3), noise=sp)
    with pytest.raises(ValueError):
        scene.rasterize_models(s, [m], m2d, sh_noise=torch.zeros(P, K, 3), noise=sp)
    with pytest.raises(ValueError):
        scene.rasterize_models(s, [m], m2d, noise=(1, 2))
    with pytest.raises(ValueError):
        scene.rasterize_models(s, [m], m2d, noise=scene.NoiseSpec(1, torch.zeros(2, dtype=torch.int32)))
    m2dv = torch.zeros(2, P, 3)
    with pytest.raises(ValueError):
        scene.rasterize_models_views([s, s], [m], m2dv, scale_noise=torch.zeros(2, P, 3), noise=sp)
    with pytest.raises(ValueError):
        scene.rasterize_models_views([s, s], [m], m2dv, noise=[sp])
    with pytest.raises(ValueError):
        scene.rasterize_models_views([s, s], [m], m2dv, noise=scene.NoiseSpec(1, torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError):
        scene.noise_tensors(sp, 8, 17, "cuda:0")
    with pytest.raises(ValueError):
        scene.noise_tensors(sp, -1, 4, "cuda:0")
    # the one-spec form numbers the views (s + k) mod 2^32
    specs = scene._view_specs(scene.NoiseSpec(9, 2 ** 32 - 1, shs=False), 3, None, None)
    assert [x.stream for x in specs] == [2 ** 32 - 1, 0, 1] and all(x.seed == 9 and not x.shs for x in specs)


def test_noise_fill_einval_precedes_any_hip_call(built_lib):
    lib = built_lib
    buf = C.c_void_p(0x1000)           # never dereferenced: every call below is refused (or has nothing to do) on the host
    assert lib.gsr_noise_fill(1, 0, None, -1, 4, buf, buf, None) == -1
    assert lib.gsr_noise_fill(1, 0, None, -1, 0, None, None, None) == -1
    assert lib.gsr_noise_fill(1, 0, None, 8, 0, buf, buf, None) == -1
    assert lib.gsr_noise_fill(1, 0, None, 8, 17, buf, buf, None) == -1
    assert lib.gsr_noise_fill(1, 0, None, 8, 4, None, None, None) == -1
    assert lib.gsr_noise_fill(1, 0, None, 0, 4, buf, None, None) == 0
    assert lib.gsr_noise_fill(1, 0, None, 0, 4, None, None, None) == -1      # (both outputs NULL is checked before P == 0)


def test_scene_noise_flags_einval_precedes_any_hip_call(built_lib):
    """A flag together with ITS tensor, or an unknown flag bit: GSR_EINVAL from the host-side checks of the forward."""
    from dreamscene_amd import _lib as L
    lib = built_lib
    p = 0x1000                         # 16-byte aligned, never dereferenced
    v = L.GsrView()
    v.P, v.sh_stride, v.sh_degree, v.image_height, v.image_width = 8, 4, 1, 16, 16
    v.tanfovx = v.tanfovy = v.scale_modifier = 1.0
    v.bg = v.viewmatrix = v.projmatrix = v.campos = p

    def call(flags, scale_noise=None, sh_noise=None):
        sc = L.GsrScene()
        sc.n_models = 1
        m = sc.models[0]
        m.count = 8
        m.xyz = m.scaling = m.rotation = m.opacity = m.features_dc = m.features_rest = p
        sc.scale_noise, sc.sh_noise, sc.noise_flags, sc.noise_seed = scale_noise, sh_noise, flags, 7
        g = L.GsrGaussians()
        g.scene = C.pointer(sc)
        n, geom = C.c_uint64(123), L.GsrGeom()
        # an empty GsrGeom: a scene that passes its checks zeroes the pair count and is refused one step later for the NULL
        # buffers, still on the host -- (-1, 0); a refused scene leaves the word alone -- (-1, 123)
        rc = lib.gsr_forward_project(C.byref(v), C.byref(g), C.byref(geom), C.byref(n), None, None)
        return rc, n.value

    assert call(L.GSR_NOISE_SCALES, scale_noise=p) == (-1, 123)
    assert call(L.GSR_NOISE_SHS, sh_noise=p) == (-1, 123)
    assert call(L.GSR_NOISE_SCALES | L.GSR_NOISE_SHS, sh_noise=p) == (-1, 123)
    assert call(4) == (-1, 123)
    assert call(0x80000001) == (-1, 123)
    # legal: no flags; both flags; one flag together with the OTHER noise's tensor
    assert call(0, scale_noise=p, sh_noise=p) == (-1, 0)
    assert call(L.GSR_NOISE_SCALES | L.GSR_NOISE_SHS) == (-1, 0)
    assert call(L.GSR_NOISE_SCALES, sh_noise=p) == (-1, 0)
    assert call(L.GSR_NOISE_SHS, scale_noise=p) == (-1, 0)


def test_gsr_scene_layout_matches_header(built_lib, tmp_path):
    """_lib.GsrScene follows the fields appended to the header's GsrScene (size and the offsets of the new fields)."""
    from dreamscene_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast.h"\n'
                   'int main(){ printf("%zu %zu %zu %zu %zu %u %u\\n", sizeof(GsrScene), offsetof(GsrScene, noise_seed),'
                   ' offsetof(GsrScene, noise_stream_dev), offsetof(GsrScene, noise_stream), offsetof(GsrScene, noise_flags),'
                   ' GSR_NOISE_SCALES, GSR_NOISE_SHS); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = L.GsrScene
    assert got == [C.sizeof(S), S.noise_seed.offset, S.noise_stream_dev.offset, S.noise_stream.offset, S.noise_flags.offset,
                   L.GSR_NOISE_SCALES, L.GSR_NOISE_SHS]
