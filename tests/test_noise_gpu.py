"""Seeded augmentation noise on the GPU (SEMANTICS.md "Seeded noise"): the generator inside K1 / K8 against the tensor form fed
with the tensors gsr_noise_fill writes for the same (seed, stream) -- equal BITS, forward and backward -- and gsr_noise_fill
against the numpy restatement (tests/noise_ref.py).

The scene: three models of 300, 70 and 1 rows (P = 371: more than one 256-row workgroup, waves that end inside a model, a
one-row model), 64 x 48 pixels, cameras inside the cloud so that some Gaussians are behind the camera and some outside
the frustum."""
import functools

import numpy as np
import pytest
import torch

from tests import noise_ref as NR

pytestmark = pytest.mark.gpu

SIZES = (300, 70, 1)
P = sum(SIZES)
H, W = 48, 64
KD = [(1, 0), (4, 1), (9, 2), (16, 3)]
SEED, STREAM = 0x9E3779B97F4A7C15, 40


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _models(K):
    """Raw leaves of the three models (built as tests/test_scene.py builds its own), once per K."""
    from dreamscene_amd import synth
    models = []
    for mi, n in enumerate(SIZES):
        g = synth.g_object(max(n, 64), seed=70 + mi, K=K)     # (kNN scales need neighbours)
        g = {k: v[:n] for k, v in g.items()}
        sc = (g["scales"] * 0.5).astype(np.float32)         # (small splats: the frustum culls some)
        op = np.clip(g["opacities"], 1e-4, 1 - 1e-4)
        off = np.array([[0.4 * (mi - 1), 0.15 * mi, 0.0]], dtype=np.float32)
        raw = (g["means3D"] * 0.8 + off, np.log(sc), g["rotations"] * (0.6 + 0.5 * mi), np.log(op / (1 - op)),
               g["shs"][:, :1, :], g["shs"][:, 1:, :])
        models.append(tuple(torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=_dev(), requires_grad=True)
                            for a in raw))
    return models


@functools.lru_cache(maxsize=None)
def _cams(n=4):
    from dreamscene_amd import synth
    return synth.object_cameras(n, H, W, radius=0.45, fovx=0.46)


@functools.lru_cache(maxsize=None)
def _upstream(k=0):
    from dreamscene_amd import synth
    gi, gda = synth.upstream_grads(H, W, seed=k)
    return torch.tensor(gi, device=_dev()), torch.tensor(gda, device=_dev())


def _settings(k, D):
    from tests.util import settings_for
    return settings_for(_cams()[k], [0.2, 0.5, 0.8], D, _dev())


def _leaves(models):
    return [t for m in models for t in m]


def _single(models, s, bufs=None, hold=None, **noise):
    """One view, forward + backward. Returns (outputs, [means2D.grad] + leaf gradients or the buffers)."""
    from dreamscene_amd import scene
    m2d = torch.zeros((P, 3), device=_dev(), requires_grad=True)
    ctx = scene.SceneContext(model_grad_buffers=bufs) if bufs is not None else None
    img, radii, da, sc = scene.rasterize_models(s, models, m2d, context=ctx, **noise)
    gi, gda = _upstream()
    loss = (img * gi).sum() + (da * gda).sum() + 0.01 * sc.mean()
    if hold is not None:
        hold(loss)
        return None
    if bufs is not None:
        loss.backward(inputs=[m2d])
        return (img, radii, da, sc), [m2d.grad] + _leaves(bufs)
    return (img, radii, da, sc), list(torch.autograd.grad(loss, [m2d] + _leaves(models), allow_unused=True))


def _views(models, sets, **noise):
    from dreamscene_amd import scene
    V = len(sets)
    for rep in range(2):            # the first batched call of a (P, H, W) still runs view by view (no capacity hint yet)
        m2d = torch.zeros((V, P, 3), device=_dev(), requires_grad=True)
        outs = scene.rasterize_models_views(sets, models, m2d, **noise)
        loss = sum((img * _upstream(k)[0]).sum() + (da * _upstream(k)[1]).sum() + 0.01 * (k + 1) * sc.mean()
                   for k, (img, _, da, sc) in enumerate(outs))
        grads = list(torch.autograd.grad(loss, [m2d] + _leaves(models), allow_unused=True))
    return outs, grads


def _same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
    else:
        assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} entries differ, " \
                                  f"max |d| {(a.double() - b.double()).abs().max().item():.3e}"


def _same_run(x, y, what):
    (xo, xg), (yo, yg) = x, y
    for name, a, b in zip(("image", "radii", "depth_alpha", "scales"), xo, yo):
        _same(a, b, f"{what}: {name}")
    assert len(xg) == len(yg)
    for j, (a, b) in enumerate(zip(xg, yg)):
        _same(a, b, f"{what}: " + ("means2D.grad" if j == 0 else f"model {(j - 1) // 6} leaf {(j - 1) % 6} gradient"))


def test_scene_has_culled_and_behind_camera_gaussians(built_lib):
    """What the other tests rely on: every camera sees some Gaussians, culls some, and has some behind it."""
    xyz = torch.cat([m[0] for m in _models(4)]).detach().cpu().numpy()
    for k in range(4):
        out, _ = _single(_models(4), _settings(k, 1))
        vis = (out[1] > 0).cpu().numpy()
        z = xyz @ np.asarray(_cams()[k].world_view_transform, dtype=np.float32)[:3, 2] + \
            np.asarray(_cams()[k].world_view_transform, dtype=np.float32)[3, 2]
        print(f"[noise scene] view {k}: {vis.sum()} of {P} visible, {(z <= 0.2).sum()} behind the near plane")
        assert 0 < vis.sum() < P
        assert (z <= 0.2).sum() > 0 and ((z > 0.2) & ~vis).sum() > 0


@pytest.mark.parametrize("K", [1, 4, 9, 16])
def test_noise_fill_matches_the_numpy_restatement(built_lib, K):
    from dreamscene_amd import scene
    for seed, stream in [(12345, 7), (2 ** 64 - 1, 8), (0, 2 ** 32 - 1)]:
        sn, hn = scene.noise_tensors(scene.NoiseSpec(seed, stream), P, K, _dev())
        assert sn.shape == (P, 3) and hn.shape == (P, K, 3)
        es = np.abs(sn.cpu().numpy().astype(np.float64) - NR.scale_noise(seed, P, stream)).max()
        eh = np.abs(hn.cpu().numpy().astype(np.float64) - NR.sh_noise(seed, P, K, stream)).max()
        print(f"[noise fill] K {K} seed {seed} stream {stream}: max |d| scale {es:.2e}, sh {eh:.2e}")
        assert es <= 1e-5 and eh <= 1e-5
    # the stream by value and through a device word: equal bits; one output alone: the same values
    word = torch.tensor([7], dtype=torch.int32, device=_dev())
    sn, hn = scene.noise_tensors(scene.NoiseSpec(12345, 7), P, K, _dev())
    sn2, hn2 = scene.noise_tensors(scene.NoiseSpec(12345, word), P, K, _dev())
    assert torch.equal(sn, sn2) and torch.equal(hn, hn2)
    a, b = scene.noise_tensors(scene.NoiseSpec(12345, 7, shs=False), P, K, _dev())
    assert b is None and torch.equal(a, sn)
    a, b = scene.noise_tensors(scene.NoiseSpec(12345, 7, scales=False), P, K, _dev())
    assert a is None and torch.equal(b, hn)


@pytest.mark.parametrize("K,D", KD)
def test_seeded_equals_tensors_one_view(built_lib, K, D):
    from dreamscene_amd import scene
    models, s = _models(K), _settings(1, D)
    spec = scene.NoiseSpec(SEED, STREAM)
    sn, hn = scene.noise_tensors(spec, P, K, _dev())
    ref = _single(models, s, scale_noise=sn, sh_noise=hn)
    _same_run(_single(models, s, noise=spec), ref, f"K {K}")
    plain = _single(models, s)
    assert not torch.equal(plain[0][0], ref[0][0]) and not torch.equal(plain[0][3], ref[0][3])    # (the noise is there)


def test_seeded_equals_tensors_into_grad_buffers_and_mixed(built_lib):
    from dreamscene_amd import scene
    K, D = 16, 3
    models, s = _models(K), _settings(2, D)
    spec = scene.NoiseSpec(SEED, STREAM + 1)
    sn, hn = scene.noise_tensors(spec, P, K, _dev())
    zeros = lambda: [tuple(torch.zeros_like(t) for t in m) for m in models]
    _same_run(_single(models, s, bufs=zeros(), noise=spec), _single(models, s, bufs=zeros(), scale_noise=sn, sh_noise=hn),
              "model_grad_buffers")
    # mixed: the scales from the generator, the SH noise from a tensor -- and the other way round
    ref = _single(models, s, scale_noise=sn, sh_noise=hn)
    _same_run(_single(models, s, noise=scene.NoiseSpec(SEED, STREAM + 1, shs=False), sh_noise=hn), ref, "scales seeded")
    _same_run(_single(models, s, noise=scene.NoiseSpec(SEED, STREAM + 1, scales=False), scale_noise=sn), ref, "SH seeded")


@pytest.mark.parametrize("K,D", [(16, 3), (4, 1)])
def test_seeded_equals_tensors_batched(built_lib, K, D):
    from dreamscene_amd import scene
    from tests.util import tol_ok
    V = 3
    models = _models(K)
    sets = [_settings(k, D if k != 1 else 0) for k in range(V)]
    specs = [scene.NoiseSpec(SEED, STREAM + k) for k in range(V)]
    tens = [scene.noise_tensors(sp, P, K, _dev()) for sp in specs]
    sn, hn = torch.stack([t[0] for t in tens]), torch.stack([t[1] for t in tens])
    ref = _views(models, sets, scale_noise=sn, sh_noise=hn)
    got = _views(models, sets, noise=specs)
    one = _views(models, sets, noise=scene.NoiseSpec(SEED, STREAM))          # view k: stream STREAM + k
    for k in range(V):
        for name, a, b, c in zip(("image", "radii", "depth_alpha", "scales"), got[0][k], ref[0][k], one[0][k]):
            _same(a, b, f"view {k} {name}")
            _same(c, b, f"view {k} {name} (one spec)")
    for j, (a, b, c) in enumerate(zip(got[1], ref[1], one[1])):
        _same(a, b, f"gradient {j}")
        _same(c, b, f"gradient {j} (one spec)")
    # view k of the batch == the single-view call with stream STREAM + k; the summed gradients at the bar
    # tests/test_scene.py::test_fused_scene_views_match_per_view_calls holds this comparison to
    singles = []
    for k in range(V):
        m2d = torch.zeros((P, 3), device=_dev(), requires_grad=True)
        o = scene.rasterize_models(sets[k], models, m2d, noise=specs[k])
        singles.append((o, m2d))
        for name, a, b in zip(("image", "radii", "depth_alpha", "scales"), got[0][k], o):
            _same(a, b, f"view {k} {name} against the single-view call")
    loss = sum((o[0] * _upstream(k)[0]).sum() + (o[2] * _upstream(k)[1]).sum() + 0.01 * (k + 1) * o[3].mean()
               for k, (o, _) in enumerate(singles))
    leaves = _leaves(models)
    sg = torch.autograd.grad(loss, [m for _, m in singles] + leaves, allow_unused=True)
    assert tol_ok(got[1][0].cpu().numpy(), torch.stack(sg[:V]).cpu().numpy(), atol=3e-6)
    for a, b, t in zip(got[1][1:], sg[V:], leaves):
        if t.numel():
            assert tol_ok(a.cpu().numpy(), b.cpu().numpy(), atol=3e-6)


def test_noise_follows_the_index_not_the_layout(built_lib):
    from dreamscene_amd import scene
    K, D = 9, 2
    models, s = _models(K), _settings(1, D)
    spec = scene.NoiseSpec(SEED, STREAM)
    three = _single(models, s, noise=spec)
    again = _single(models, s, noise=spec)
    _same_run(again, three, "the same call twice")
    # the same 371 rows as ONE model: the same bits (a value depends on the concatenated index alone)
    one = [tuple(torch.cat([m[j] for m in models]).detach().requires_grad_(True) for j in range(6))]
    o1, g1 = _single(one, s, noise=spec)
    for name, a, b in zip(("image", "radii", "depth_alpha", "scales"), o1, three[0]):
        _same(a, b, f"one model: {name}")
    _same(g1[0], three[1][0], "one model: means2D.grad")
    for j in range(6):
        _same(g1[1 + j], torch.cat([three[1][1 + 6 * m + j] for m in range(len(SIZES))]), f"one model: leaf {j} gradient")
    # another stream: another image, other returned scales
    other = _single(models, s, noise=scene.NoiseSpec(SEED, STREAM + 1))
    assert not torch.equal(other[0][0], three[0][0]) and not torch.equal(other[0][3], three[0][3])


def test_tensor_stream(built_lib):
    from dreamscene_amd import scene
    K, D = 4, 1
    models, s = _models(K), _settings(3, D)
    word = torch.tensor([STREAM + 5], dtype=torch.int32, device=_dev())
    _same_run(_single(models, s, noise=scene.NoiseSpec(SEED, word)), _single(models, s, noise=scene.NoiseSpec(SEED, STREAM + 5)),
              "tensor stream")
    # K8 reads the word again: editing it between forward and backward is refused
    kept = []
    _single(models, s, hold=kept.append, noise=scene.NoiseSpec(SEED, word))
    word += 1
    with pytest.raises(RuntimeError, match="noise stream"):
        kept[0].backward()
    # the views of a batch read consecutive words of one int32[V] tensor
    V = 3
    sets = [_settings(k, D) for k in range(V)]
    words = torch.arange(STREAM, STREAM + V, dtype=torch.int32, device=_dev())
    got = _views(models, sets, noise=scene.NoiseSpec(SEED, words))
    ref = _views(models, sets, noise=scene.NoiseSpec(SEED, STREAM))
    for k in range(V):
        for name, a, b in zip(("image", "radii", "depth_alpha", "scales"), got[0][k], ref[0][k]):
            _same(a, b, f"view {k} {name}")
    for j, (a, b) in enumerate(zip(got[1], ref[1])):
        _same(a, b, f"gradient {j}")


def test_views_with_different_seeds_run_view_by_view(built_lib):
    """The views kernels carry one seed per batch; a batch whose specs differ in the seed takes K1 / K8 view by view and
    computes the same thing: outputs equal to the tensor form's, gradients at the bar of the batched-against-per-view test."""
    from dreamscene_amd import scene
    from tests.util import tol_ok
    K, D, V = 4, 1, 2
    models = _models(K)
    sets = [_settings(k, D) for k in range(V)]
    specs = [scene.NoiseSpec(SEED + k, STREAM) for k in range(V)]
    tens = [scene.noise_tensors(sp, P, K, _dev()) for sp in specs]
    ref = _views(models, sets, scale_noise=torch.stack([t[0] for t in tens]), sh_noise=torch.stack([t[1] for t in tens]))
    got = _views(models, sets, noise=specs)
    for k in range(V):
        for name, a, b in zip(("image", "radii", "depth_alpha", "scales"), got[0][k], ref[0][k]):
            _same(a, b, f"view {k} {name}")
    for a, b in zip(got[1], ref[1]):
        if a is not None and a.numel():
            assert tol_ok(a.cpu().numpy(), b.cpu().numpy(), atol=3e-6)
