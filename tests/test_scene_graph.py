"""dreamscene_amd/scene_graph.py without a device: the GSR_EINVAL answers of gsr_pack_views_streams that precede any HIP call,
the argument checks of CapturedModelsViews (before any device work), and the capture key (pure; what re-captures and what
does not)."""
import ctypes as C
import dataclasses

import pytest
import torch

GSR_EINVAL = -1


def _settings(H=16, W=16, **kw):
    from dreamscene_amd.rasterizer import GaussianRasterizationSettings
    base = dict(image_height=H, image_width=W, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3), scale_modifier=1.0,
                viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=1, campos=torch.zeros(3), prefiltered=False,
                score_flag=False)
    base.update(kw)
    return GaussianRasterizationSettings(**base)


def _cpu_model(n=8, K=4):
    z = lambda *s: torch.zeros(s)
    return (z(n, 3), z(n, 3), z(n, 4), z(n, 1), z(n, 1, 3), z(n, K - 1, 3))


def _view(L, p=0x1000):
    v = L.GsrView()
    v.P, v.sh_stride, v.sh_degree, v.image_height, v.image_width = 8, 4, 1, 16, 16
    v.tanfovx = v.tanfovy = v.scale_modifier = 1.0
    v.bg = v.viewmatrix = v.projmatrix = v.campos = p
    return v


def test_pack_views_streams_einval_precedes_any_hip_call(built_lib):
    from dreamscene_amd import _lib as L
    lib = built_lib
    buf = C.c_void_p(0x1000)            # 16-byte aligned, never dereferenced: every call below is refused on the host
    views = (L.GsrView * 17)(*[_view(L) for _ in range(17)])
    ids = (C.c_uint32 * 17)()
    assert lib.gsr_pack_views_streams(0, views, ids, buf, buf, None) == GSR_EINVAL
    assert lib.gsr_pack_views_streams(17, views, ids, buf, buf, None) == GSR_EINVAL
    assert lib.gsr_pack_views_streams(-1, views, ids, buf, buf, None) == GSR_EINVAL
    assert lib.gsr_pack_views_streams(2, None, ids, buf, buf, None) == GSR_EINVAL          # NULL views
    assert lib.gsr_pack_views_streams(2, views, ids, None, buf, None) == GSR_EINVAL        # NULL packed
    assert lib.gsr_pack_views_streams(2, views, ids, C.c_void_p(0x1004), buf, None) == GSR_EINVAL      # misaligned packed
    assert lib.gsr_pack_views_streams(2, views, ids, buf, C.c_void_p(0x1002), None) == GSR_EINVAL      # misaligned words
    # the checks are gsr_pack_views': a view that asks for more SH bands than stored is refused by both
    bad = (L.GsrView * 1)(_view(L))
    bad[0].sh_degree = 2
    assert lib.gsr_pack_views_streams(1, bad, ids, buf, buf, None) == GSR_EINVAL
    assert lib.gsr_pack_views(1, bad, buf, None) == GSR_EINVAL
    assert lib.gsr_pack_views(0, views, buf, None) == GSR_EINVAL and lib.gsr_pack_views(1, views, None, None) == GSR_EINVAL


def test_module_argument_checks_precede_any_device_work():
    from dreamscene_amd import scene
    from dreamscene_amd._lib import GsrError
    from dreamscene_amd.scene_graph import CapturedModelsViews
    m, P, K = _cpu_model(), 8, 4
    s = _settings()
    rast = CapturedModelsViews()
    ok = torch.zeros(2, P, 3)
    for bad in (torch.zeros(P, 3), torch.zeros(3, P, 3), torch.zeros(2, P + 1, 3), torch.zeros(2, P, 2)):
        with pytest.raises(ValueError, match="means2D"):
            rast([s, s], [m], bad)
    with pytest.raises(ValueError, match="same image size"):
        rast([s, _settings(H=32)], [m], ok)
    with pytest.raises(ValueError, match="same image size"):
        rast([s, _settings(scale_modifier=2.0)], [m], ok)
    with pytest.raises(ValueError, match="score_flag"):
        rast([s, _settings(score_flag=True)], [m], ok)
    sp = scene.NoiseSpec(1, 2)
    with pytest.raises(ValueError, match="not both"):
        rast([s, s], [m], ok, scale_noise=torch.zeros(2, P, 3), noise=sp)
    with pytest.raises(ValueError, match="not both"):
        rast([s, s], [m], ok, sh_noise=torch.zeros(2, P, K, 3), noise=sp)
    with pytest.raises(ValueError):
        rast([s, s], [m], ok, noise=[sp])
    with pytest.raises(ValueError):
        rast([s, s], [m], ok, noise=scene.NoiseSpec(1, torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError):
        rast([], [m], torch.zeros(0, P, 3))
    with pytest.raises(ValueError):
        rast([s] * 17, [m], torch.zeros(17, P, 3))
    with pytest.raises(GsrError, match="no CPU fallback"):      # CPU tensors, everything else in order
        rast([s, s], [m], ok, noise=scene.NoiseSpec(1, 2, shs=False), sh_noise=torch.zeros(2, P, K, 3))
    assert rast.stats == dict(captures=0, replays=0, eager_steps=0, overflows=0)


def test_capture_key_is_pure_and_names_what_is_baked_in():
    from dreamscene_amd import scene
    from dreamscene_amd.scene_graph import capture_key
    P, K, V = 8, 4, 2
    m0, m1 = _cpu_model(P, K), _cpu_model(5, K)
    s = _settings()
    sets = [s, s]
    spec = lambda **kw: scene._view_specs(scene.NoiseSpec(**{**dict(seed=7, stream=10), **kw}), V, None, None)
    bufs = [tuple(torch.zeros_like(t) for t in m0)]
    stats = tuple(torch.zeros(P) for _ in range(3))
    rc = scene.SceneContext(model_grad_buffers=bufs, densify_stats=stats)
    sn, hn = torch.zeros(V, P, 3), torch.zeros(V, P, K, 3)

    def key(sets=sets, models=(m0,), scale_noise=None, sh_noise=None, specs=spec(), rc=rc):
        return capture_key(sets, [tuple(m) for m in models], scale_noise, sh_noise, specs, rc)
    base = key()
    assert base == key() and hash(base) == hash(key())          # pure, hashable
    # ---- what lives in device memory rewritten per step: the same key
    moved = _settings(bg=torch.ones(3), viewmatrix=2 * torch.eye(4), projmatrix=3 * torch.eye(4), campos=torch.ones(3),
                      tanfovx=0.5, tanfovy=0.7, sh_degree=0)
    assert key(sets=[moved, s]) == base
    assert key(specs=spec(stream=2 ** 32 - 1)) == base
    assert key(specs=[scene.NoiseSpec(7, 99), scene.NoiseSpec(7, 3)]) == base
    # ---- what is baked into the captured structs: another key
    others = dict(
        V=key(sets=[s, s, s]), H=key(sets=[_settings(H=32)] * 2), W=key(sets=[_settings(W=32)] * 2),
        scale_modifier=key(sets=[_settings(scale_modifier=2.0)] * 2),
        prefiltered=key(sets=[s, _settings(prefiltered=True)]),
        model_count=key(models=(m0, m1)), model_size=key(models=(_cpu_model(P + 1, K),)),
        model_K=key(models=(_cpu_model(P, 9),)), leaf_address=key(models=(m0[:1] + (torch.zeros(P, 3),) + m0[2:],)),
        no_noise=key(specs=None), noise_tensors=key(specs=None, scale_noise=sn),
        both_tensors=key(specs=None, scale_noise=sn, sh_noise=hn),
        flags=key(specs=spec(shs=False)), flags2=key(specs=spec(scales=False)), mixed=key(specs=spec(shs=False), sh_noise=hn),
        seed=key(specs=spec(seed=8)),
        stream_tensor=key(specs=spec(stream=torch.zeros(V, dtype=torch.int32))),
        one_view_unseeded=key(specs=[scene.NoiseSpec(7, 10), None]),
        no_buffers=key(rc=dataclasses.replace(rc, model_grad_buffers=None)),
        other_buffers=key(rc=dataclasses.replace(rc, model_grad_buffers=[tuple(torch.zeros_like(t) for t in m0)])),
        no_stats=key(rc=dataclasses.replace(rc, densify_stats=None)),
        other_stats=key(rc=dataclasses.replace(rc, densify_stats=tuple(torch.zeros(P) for _ in range(3)))),
        stats_views=key(rc=dataclasses.replace(rc, stats_views=[0])), stats_all=key(rc=dataclasses.replace(rc, stats_views="all")),
        fwd_variant=key(rc=dataclasses.replace(rc, fwd_variant=1)),
    )
    for name, k in others.items():
        assert k != base, name
    assert len(set(others.values())) == len(others)             # and from each other
    # a caller's stream tensor is keyed by address: the same tensor again is the same key, another one is not
    words = torch.zeros(V, dtype=torch.int32)
    assert key(specs=spec(stream=words)) == key(specs=spec(stream=words))
    assert key(specs=spec(stream=words)) != key(specs=spec(stream=torch.zeros(V, dtype=torch.int32)))
