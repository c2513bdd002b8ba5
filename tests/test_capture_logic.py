"""The host decisions of the captured step modules (dreamscene_amd/graph.py, shared with scene_graph.py and dropin.py), without
a device: when inputs are staged, when a replay overflowed, the capacity grid, the declared capture records, the refusal of a
stale backward."""
import pytest


def test_staging_policy_switches_on_address_misses_and_back_on_repeats():
    from dreamscene_amd.graph import PTR_MISSES_TO_STAGE, PTR_REPEATS_TO_UNSTAGE, StagingPolicy
    shape = ("shape", 1)
    ptr = lambda n: ("ptr", n)
    # ---- no capture yet: keyed on addresses, nothing counted
    p = StagingPolicy()
    assert p.choose(shape, ptr(0), None) == (ptr(0), True) and not p.staged and p.misses == 0
    # ---- captures lost to new addresses and nothing else, PTR_MISSES_TO_STAGE times in a row: the shape key from then on
    for n in range(1, PTR_MISSES_TO_STAGE):
        assert p.choose(shape, ptr(n), (ptr(n - 1), shape)) == (ptr(n), True)
        assert not p.staged and p.misses == n
    n = PTR_MISSES_TO_STAGE
    assert p.choose(shape, ptr(n), (ptr(n - 1), shape)) == (shape, True) and p.staged
    assert p.choose(shape, ptr(n + 1), (shape, shape)) == (shape, False) and p.staged      # fresh addresses now hit
    # ---- a hit in between resets the miss count
    p = StagingPolicy()
    for n in range(1, PTR_MISSES_TO_STAGE):
        p.choose(shape, ptr(n), (ptr(n - 1), shape))
    assert p.misses == PTR_MISSES_TO_STAGE - 1
    assert p.choose(shape, ptr(n), (ptr(n), shape)) == (ptr(n), False) and p.misses == 0
    for k in range(1, PTR_MISSES_TO_STAGE):
        assert p.choose(shape, ptr(n + k), (ptr(n + k - 1), shape)) == (ptr(n + k), True) and not p.staged
    # ---- a changed shape signature never counts as a pointer miss
    p = StagingPolicy()
    for n in range(1, 3 * PTR_MISSES_TO_STAGE):
        sh = ("shape", 100 + n)
        assert p.choose(sh, ptr(n), (ptr(n - 1), ("shape", 100 + n - 1))) == (ptr(n), True)
    assert not p.staged and p.misses == 0
    # ---- while staged: PTR_REPEATS_TO_UNSTAGE identical pointer signatures in a row switch back and clear the counters
    def staged_policy():
        q = StagingPolicy()
        for n in range(1, PTR_MISSES_TO_STAGE + 1):
            q.choose(shape, ptr(n), (ptr(n - 1), shape))
        assert q.staged
        return q
    p = staged_policy()
    assert p.choose(shape, ptr(50), (shape, shape)) == (shape, False) and p.repeats == 0      # the first sighting
    for k in range(1, PTR_REPEATS_TO_UNSTAGE):
        assert p.choose(shape, ptr(50), (shape, shape)) == (shape, False) and p.staged and p.repeats == k
    assert p.choose(shape, ptr(50), (shape, shape)) == (ptr(50), True)        # back on addresses: the staged capture goes
    # (the counters were cleared; dropping the staged capture for an address-keyed one of the same shapes is then the first miss)
    assert (p.staged, p.misses, p.repeats) == (False, 1, 0)
    # ---- one different signature in between resets the repeat count
    p = staged_policy()
    for k in range(PTR_REPEATS_TO_UNSTAGE):
        p.choose(shape, ptr(50), (shape, shape))
    assert p.repeats == PTR_REPEATS_TO_UNSTAGE - 1
    assert p.choose(shape, ptr(51), (shape, shape)) == (shape, False) and p.repeats == 0 and p.staged
    for k in range(1, PTR_REPEATS_TO_UNSTAGE):
        assert p.choose(shape, ptr(51), (shape, shape)) == (shape, False) and p.staged
    assert p.choose(shape, ptr(51), (shape, shape)) == (ptr(51), True) and not p.staged


def test_captured_views_reports_the_policys_staged_flag_under_its_old_name():
    from dreamscene_amd.graph import CapturedViews
    rast = CapturedViews()
    assert rast._staged is False and rast.stats["staged_inputs"] is False
    rast._staging.staged = True
    assert rast._staged is True            # what dropin.py reads


def test_overflow_rule():
    from dreamscene_amd.graph import overflowed
    cap = 65536
    assert overflowed([10, cap + 1, 10], cap)              # a count above the capacity
    assert overflowed([10, -1, 10], cap)                   # a count that never arrived
    assert overflowed([-1], cap) and overflowed([cap + 1], cap)
    assert not overflowed([cap, cap, cap], cap)            # equal to the capacity: everything fitted
    assert not overflowed([0, 1, cap], cap)


@pytest.mark.parametrize("headroom", [1.0, 1.5, 2.25])
def test_capacity_for_is_the_eager_paths_grid(headroom):
    from dreamscene_amd import rasterizer as R
    from dreamscene_amd.graph import capacity_for

    def inline(pairs):          # rasterizer._forward_steps' three lines as they stood, with `pairs` for int(hint * 1.5)
        want = pairs + 65536
        q = max(65536, 1 << max(0, want.bit_length() - 4))
        return (want + q - 1) // q * q
    for peak in (0, 1, 65535, 65536, 10 ** 6, 2 ** 31):
        pairs = int(peak * headroom)
        got = capacity_for(peak, headroom)
        assert got == R.capacity_grid(pairs) == inline(pairs), (peak, headroom)
        assert got >= pairs + 65536 and got % 65536 == 0 and got >= 65536
        assert got - (pairs + 65536) < max(65536, (pairs + 65536) / 8)        # 1/8 octave: never more than an eighth too much


def test_capture_records_reject_undeclared_attributes():
    from dreamscene_amd.graph import Captured, _ViewsCapture
    from dreamscene_amd.scene_graph import _ModelsCapture
    shared = ("P", "K", "V", "cap", "packed", "pinned", "pinned_np", "generation", "proj_scratch", "sort_scratch", "views",
              "geoms", "gauss", "bins", "imgs", "gF", "evF", "states", "outs", "g_color", "g_da")
    own = {_ViewsCapture: ("sig", "shape_sig", "ptr_sig", "staged", "scales", "rc", "per_view", "gC", "gC0", "bwd", "bwd_zo",
                           "bwd_versions", "direct"),
           _ModelsCapture: ("sn", "hn", "words", "g_scales", "gC", "bwd", "bwd_m2d"),
           Captured: ()}
    for cls, fields in own.items():
        cap = cls()
        assert not hasattr(cap, "__dict__")
        for name in shared + fields:
            setattr(cap, name, 1)
            assert getattr(cap, name) == 1
        for typo in ("pined", "generaton", "ptr_sgi", "bwd_m2D", "shape_sig" if cls is not _ViewsCapture else "g_scales"):
            with pytest.raises(AttributeError):
                setattr(cap, typo, 1)


def test_stale_backward_refusal_names_the_module_the_replays_and_the_alternative():
    from types import SimpleNamespace
    from dreamscene_amd import graph as G
    from dreamscene_amd.graph import CapturedViews
    from dreamscene_amd.scene_graph import CapturedModelsViews
    for module, name, alternative in ((CapturedViews, "CapturedViews", "GaussianRasterizerViews"),
                                      (CapturedModelsViews, "CapturedModelsViews", "rasterize_models_views")):
        assert (module.NAME, module.ALTERNATIVE) == (name, alternative)
        text = G.stale_backward_message(module.NAME, module.ALTERNATIVE, 3, 5)
        assert text.startswith(name + ": backward of a forward whose captured state has been overwritten by a later forward")
        assert "(replay 3, now 5)" in text and f"the same {name}, or use {alternative} for calls" in text
        # the check the two autograd Functions run: the capture's generation against the one the forward saw
        ctx = SimpleNamespace(owner=module(), cap_state=SimpleNamespace(generation=5), generation=3)
        with pytest.raises(RuntimeError, match="overwritten by a later forward") as e:
            G.refuse_stale_backward(ctx)
        assert str(e.value) == text
        ctx.generation = 5
        G.refuse_stale_backward(ctx)                    # the latest replay's backward goes through
        ctx.cap_state, ctx.generation = None, -1
        G.refuse_stale_backward(ctx)                    # an eager step has no capture to be stale
    # byte for byte what the modules said before the helper existed
    assert G.stale_backward_message("CapturedViews", "GaussianRasterizerViews", 1, 2) == (
        "CapturedViews: backward of a forward whose captured state has been overwritten by a later forward "
        "(replay 1, now 2); run backward before the next forward of the same "
        "CapturedViews, or use GaussianRasterizerViews for calls whose graphs must stay alive")
