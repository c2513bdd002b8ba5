"""CPU self-checks of the lockstep trajectory harness (tests/trajectory_ref.py), so that tests/test_trajectory_gpu.py cannot pass
vacuously: the committed seed's schedule exercises what it is meant to exercise, the float64 shadow step is itself right (finite
differences), and the restated pieces (the densification kernel's generator, the Adam reference) are what they claim to be.
Everything here runs on the reference alone: the whole schedule in fp32 through the C oracle, torch's Adam and densify_ref."""
import numpy as np
import pytest
import torch

from tests import trajectory_ref as T


@pytest.fixture(scope="module")
def sched():
    return T.schedule()


@pytest.fixture(scope="module")
def traj(sched, c_oracle):
    return T.cpu_trajectory(sched)


@pytest.fixture(scope="module")
def anchors(sched, traj):
    return {i: T.anchor(traj["pre"][i], sched.steps[i]) for i in T.ANCHORS}


def test_schedule_is_a_function_of_the_seed_and_has_the_stated_shape(sched):
    again = T.schedule()
    assert sched.densify_seed == again.densify_seed and len(sched.steps) == T.N_STEPS == 18
    for a, b in zip(sched.steps, again.steps):
        assert torch.equal(a.noise, b.noise) and torch.equal(a.targets, b.targets) and torch.equal(a.bg, b.bg)
        assert a.sh_degree == b.sh_degree
        assert all(np.array_equal(x.full_proj_transform, y.full_proj_transform) for x, y in zip(a.cams, b.cams))
    other = T.schedule(T.SEED + 1)
    assert not torch.equal(sched.steps[0].noise, other.steps[0].noise)
    assert (T.K, T.D, T.V, T.H, T.W, T.P0) == (16, 3, 3, 40, 56, 400)
    assert T.H % 16 and T.W % 16 and T.P0 > 256 and T.P0 % 64 and T.V & (T.V - 1)
    assert sched.leaves["xyz"].shape == (T.P0, 3) and sched.leaves["f_rest"].shape == (T.P0, T.K - 1, 3)
    kinds = set()
    for st in sched.steps:
        assert len(st.cams) == T.V and st.noise.shape == (T.V, T.P_MAX, 3) and st.targets.shape == (T.V, 3, T.H, T.W)
        for k in range(T.V):
            kinds.add("white" if bool((st.bg[k] == 1).all()) else "black" if bool((st.bg[k] == 0).all()) else "random")
    assert kinds == {"white", "black", "random"}
    fovs = {round(c.FoVx, 6) for st in sched.steps for c in st.cams}
    assert len(fovs) == T.N_STEPS * T.V, "every view of every step has a field of view of its own"
    # every phase has a view with SH degree 0, and exactly one step renders an eval view: in phase B, behind capture + replay
    for ph in range(len(T.PHASES)):
        assert any(0 in st.sh_degree for st in sched.steps[ph * T.STEPS:(ph + 1) * T.STEPS])
    assert [i for i, st in enumerate(sched.steps) if st.eval_cam is not None] == [T.EVAL_STEP]
    assert T.STEPS + 3 <= T.EVAL_STEP < 2 * T.STEPS
    assert T.ANCHORS == (0, 6, 12, 17)


def test_the_trajectory_changes_P_as_stated(traj):
    """The densification yields survivors, clones and children and prunes at least one row; P1 > 512 (it crosses a workgroup
    boundary) and P2 < P0."""
    P0, P1, P2 = traj["sizes"]
    ref = traj["densify"]
    S, C, K0, K1 = ref.segments(T.DENSIFY["N"])
    print(f"P0 {P0} -> P1 {P1} (survivors {S}, clones {C}, children {K0} + {K1}) -> P2 {P2} ({traj['pruned']} pruned)")
    assert P0 == T.P0 and P1 == S + C + K0 + K1 and P1 > 512 and P2 < P0 and P1 <= T.P_MAX
    assert S > 0 and C > 0 and K0 == K1 > 0
    originals = set(ref.origin.tolist())
    assert len(originals) < P0, "the densification pruned no row"
    assert traj["pruned"] >= 1 and P2 == P1 - traj["pruned"]


def test_every_last_view_sees_some_gaussians_and_misses_others(traj):
    for i, radii in enumerate(traj["last_radii"]):
        vis = float((radii > 0).float().mean())
        assert 0.05 <= vis <= 0.95, (i, vis)


def test_the_anchor_can_arbitrate(anchors):
    """At every anchored step the float64 and the fp32 evaluation agree on radii in every view, and the fp32 evaluation is within
    1e-3 of float64 in every tensor: 4 e_ref + 1e-5 then catches a stale row, a missing view or a wrong P."""
    for i, a in anchors.items():
        print(f"step {i}: e_ref " + "  ".join(f"{n} {e:.1e}" for n, e in a["e_ref"].items()))
        assert a["radii_agree"], i
        for n, e in a["e_ref"].items():
            assert e <= 1e-3, (i, n, e)


def test_float64_step_equals_finite_differences(sched):
    """Central differences of the float64 step's loss on three entries: the largest gradient entry of xyz, opacity and f_dc among
    the Gaussians for which the oracle's gradient IS the derivative. Its two conventions (oracle/torch_oracle.py) make it differ
    on purpose elsewhere: alpha = min(0.99, opacity * G) back-propagates as if un-clamped -- so only rows with opacity < 0.9,
    which never clamp --, and the clamped view-space position has its own rule outside 1.3 x the frustum -- so only rows the close
    last view culls at its near plane and the far first view sees. h = 1e-6 keeps the truncation error h^2 |f'''| / 6 and the
    rounding error 2^-52 |loss| / h ~ 1e-10 both below 1e-4 of gradients of 1e-5 ... 1e-2."""
    st = sched.steps[0]
    r = T.shadow_step(sched.leaves, st, "f64")
    rows = (r["radii"][-1] == 0) & (r["radii"][0] > 0) & (torch.sigmoid(sched.leaves["opacity"]).reshape(-1) < 0.9)
    assert int(rows.sum()) >= 10
    h = 1e-6
    for n in ("xyz", "opacity", "f_dc"):
        g = r[n] * rows.reshape((-1,) + (1,) * (r[n].dim() - 1))
        idx = int(g.abs().reshape(-1).argmax())
        vals = []
        for sign in (1.0, -1.0):
            lv = {k: v.double().clone() for k, v in sched.leaves.items()}
            lv[n].reshape(-1)[idx] += sign * h
            vals.append(float(T.shadow_forward(lv, st, "f64")[0].detach()))
        fd, an = (vals[0] - vals[1]) / (2 * h), float(g.reshape(-1)[idx])
        print(f"{n}[{idx}]: autograd {an:.9e}  finite differences {fd:.9e}")
        assert an != 0.0 and abs(fd - an) <= 1e-4 * abs(an) + 1e-9, (n, fd, an)


def test_split_normals_restate_the_kernels_generator():
    """Philox-4x32-10's published known-answer vectors (Random123 kat_vectors), and the normals' first two moments."""
    f = lambda *a: tuple(int(x[0]) for x in T._philox4x32_10(*[np.array([v], dtype=np.uint64) for v in a[:4]], a[4], a[5]))
    assert f(0, 0, 0, 0, 0, 0) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert f(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert f(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0) == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    z = T.split_normals(12345, 50_000, 2)
    assert z.shape == (2, 50_000, 3) and bool(torch.isfinite(z).all())
    n = z.numel() / 3
    assert float(z.mean(dim=(0, 1)).abs().max()) < 5 / n ** 0.5 and float((z.var(dim=(0, 1)) - 1).abs().max()) < 5 * (2 / n) ** 0.5
    assert torch.equal(z, T.split_normals(12345, 50_000, 2)) and not torch.equal(z[0], z[1])
    assert torch.equal(T.split_normals(12345, 100, 2), z[:, :100]), "a row's normals do not depend on P"


def test_adam_reference_is_torchs_adam():
    g = torch.Generator().manual_seed(1)
    params = {n: torch.randn(5, *s, generator=g) for n, s in
              zip(T.NAMES, ((3,), (1, 3), (T.K - 1, 3), (1,), (3,), (4,)))}
    grads = {n: torch.randn(p.shape, generator=g) * 1e-3 for n, p in params.items()}
    p1, m1 = T.adam_reference(params, None, 0.0, grads)
    for n in T.NAMES:       # the first step of Adam moves every entry by lr * sign(g) (eps = 1e-15)
        np.testing.assert_allclose((p1[n] - params[n]).numpy(), (-T.LRS[n] * torch.sign(grads[n])).numpy(), rtol=1e-6, atol=5e-7)      # (2 ulp of parameters up to 4)
        np.testing.assert_allclose(m1[n][0].numpy(), (0.1 * grads[n]).numpy(), rtol=1e-6)
    p2, m2 = T.adam_reference(p1, m1, 1.0, grads)
    assert all(bool((p2[n] != p1[n]).any()) for n in T.NAMES)
