"""FusedAdam (csrc/optim.hip, dreamscene_amd/optim.py) where tests/test_epilogue.py does not reach: more than
GSR_MAX_ADAM_GROUPS parameters (several launches), differing `step` / `betas` / `eps` (the `batches` key), long horizons,
the gradient magnitudes the reference's eps = 1e-15 opens up, element counts around the float4 body / scalar tail / block
edge, empty groups, `grad None`, non-contiguous gradients, refused calls, version counters.

Reference: torch.optim.Adam in fp32 on the CPU (the optimizer the reference instantiates); yardstick: torch.optim.Adam in
float64 on the same fp32 inputs. Two kinds of bar:
 * well-conditioned values (|g| 1e-18 ... 1e15): per tensor, HIP may be at most 2x as far from float64 as torch-fp32 is
   (largest relative distance), plus one fp32 ulp of the entry. Both are fp32 evaluations with one rounding per operator;
   the factor 2 covers the different association in addcdiv ((value * m) / denom there, step_size * (m / denom) here).
 * where g*g is subnormal, zero or overflows (|g| <= 1e-19, one row at 1e20) float64 is no reference: HIP against torch-fp32
   at test_epilogue's rtol=2e-6, atol=1e-7 (parameters) and rtol=2e-6 + 2e-6 of the compared tensor's largest entry
   (moments), and the sets of zero, subnormal, inf and nan entries must coincide.
Plain comparisons with torch-fp32 elsewhere use test_epilogue's bars as they stand."""
import ctypes

import numpy as np
import pytest
import torch

DEV = torch.device("cuda:0")
P_RTOL, P_ATOL, M_RTOL = 2e-6, 1e-7, 2e-6          # tests/test_epilogue.py::test_fused_adam_matches_torch_adam


def _np(t):
    return t.detach().cpu().numpy()


def _groups(ps, lrs, extra=None):
    out = []
    for k, (p, lr) in enumerate(zip(ps, lrs)):
        g = {"params": [p], "lr": lr}
        if extra:
            g.update(extra(k))
        out.append(g)
    return out


class Trio:
    """The same parameters three times: FusedAdam on the device, torch Adam fp32 and torch Adam float64 on the CPU."""

    def __init__(self, init, lrs, extra=None, with_f64=True, **kw):
        from dreamscene_amd.optim import FusedAdam
        self.t32 = [t.clone().requires_grad_(True) for t in init]
        self.hip = [t.clone().to(DEV).requires_grad_(True) for t in init]
        self.t64 = [t.double().requires_grad_(True) for t in init] if with_f64 else []
        self.opt = FusedAdam(_groups(self.hip, lrs, extra), **kw)
        self.ref = torch.optim.Adam(_groups(self.t32, lrs, extra), **kw)
        self.ref64 = torch.optim.Adam(_groups(self.t64, lrs, extra), **kw) if with_f64 else None

    def set_grads(self, grads):
        for k, g in enumerate(grads):
            self.t32[k].grad = None if g is None else g.clone()
            self.hip[k].grad = None if g is None else g.to(DEV)
            if self.t64:
                self.t64[k].grad = None if g is None else g.double()

    def set_state(self, k, step, m, v):
        for ps, o, cast in ((self.t32, self.ref, lambda t: t.clone()), (self.hip, self.opt, lambda t: t.to(DEV)),
                            (self.t64, self.ref64, lambda t: t.double())):
            if o is not None:
                o.state[ps[k]] = {"step": torch.tensor(float(step)), "exp_avg": cast(m), "exp_avg_sq": cast(v)}

    def step(self, **kw):
        self.ref.step()
        if self.ref64 is not None:
            self.ref64.step()
        self.opt.step(**kw)

    def tensors(self, k):
        """(name, hip, torch-fp32, float64 or None) for the parameter and both moments of parameter k."""
        a, b = self.t32[k], self.hip[k]
        sa, sb = self.ref.state[a], self.opt.state[b]
        s64 = self.ref64.state[self.t64[k]] if self.t64 else None
        yield "param", _np(b), _np(a), (_np(self.t64[k]) if self.t64 else None)
        for key in ("exp_avg", "exp_avg_sq"):
            yield key, _np(sb[key]), _np(sa[key]), (_np(s64[key]) if s64 else None)

    def assert_matches_torch(self, what=""):
        for k in range(len(self.t32)):
            a, b = self.t32[k], self.hip[k]
            if a not in self.ref.state:
                assert b not in self.opt.state or len(self.opt.state[b]) == 0, f"{what} p{k}: state without a step"
                assert np.array_equal(_np(a), _np(b)), f"{what} p{k}"
                continue
            assert float(self.ref.state[a]["step"]) == float(self.opt.state[b]["step"]), f"{what} p{k} step"
            for name, h, t, _ in self.tensors(k):
                if name == "param":
                    np.testing.assert_allclose(h, t, rtol=P_RTOL, atol=P_ATOL, err_msg=f"{what} p{k}")
                else:
                    top = float(np.abs(t).max()) if t.size else 0.0
                    np.testing.assert_allclose(h, t, rtol=M_RTOL, atol=M_RTOL * top, err_msg=f"{what} p{k} {name}")


def _distances(h, t, r):
    """Largest relative distance of HIP and of torch-fp32 from float64, over the entries where float64 is not zero."""
    h, t = h.astype(np.float64), t.astype(np.float64)
    nz = r != 0
    if not nz.any():
        return 0.0, 0.0
    return float((np.abs(h - r)[nz] / np.abs(r)[nz]).max()), float((np.abs(t - r)[nz] / np.abs(r)[nz]).max())


def _assert_within_torch_bar(h, t, r, what):
    """|hip - f64| <= 2 * D_torch * |f64| + ulp32(f64) for every entry, D_torch = torch-fp32's largest relative distance."""
    d_h, d_t = _distances(h, t, r)
    print(f"{what}: largest relative distance from float64: HIP {d_h:.3e}, torch-fp32 {d_t:.3e}")
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(h)), what
    ulp = np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
    bad = np.abs(h.astype(np.float64) - r) > 2.0 * d_t * np.abs(r) + ulp
    assert not bad.any(), f"{what}: HIP {d_h:.3e} vs torch-fp32 {d_t:.3e} from float64; {int(bad.sum())} entries past the bar"
    return d_h, d_t


def _away_from_zero(shape, gen):
    return (1.0 + torch.rand(shape, generator=gen)) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()


def _classes(x):
    tiny = np.finfo(np.float32).tiny
    return {"zero": x == 0, "subnormal": (x != 0) & (np.abs(x) < tiny), "inf": np.isinf(x), "nan": np.isnan(x)}


def _assert_like_torch_fp32(name, h, t, what):
    for cls, mask in _classes(t).items():
        assert np.array_equal(_classes(h)[cls], mask), f"{what}: the {cls} entries differ from torch-fp32's"
    fin = np.isfinite(t)
    if name == "param":
        np.testing.assert_allclose(h[fin], t[fin], rtol=P_RTOL, atol=P_ATOL, err_msg=what)
    else:
        top = float(np.abs(t[fin]).max()) if fin.any() else 0.0
        np.testing.assert_allclose(h[fin], t[fin], rtol=M_RTOL, atol=M_RTOL * top, err_msg=what)
    assert np.array_equal(h[~fin], t[~fin], equal_nan=True), what


# ------------------------------------------------------------------------------------------------ 1. magnitudes

FIRST_WELL = 12          # row r carries |g| ~ 10^(r - 30): rows 0..11 are 1e-30 .. 1e-19, rows 12..45 are 1e-18 .. 1e15


@pytest.mark.gpu
def test_magnitude_sweep_fifty_steps(built_lib):
    """Measured on an MI355X (50 steps, lr 1e-3, eps 1e-15), largest relative distance from float64, HIP | torch-fp32:
    rows 1e-18 ... 1e15: parameter 6.228e-07 | 6.228e-07, exp_avg 1.979e-04 | 1.979e-04, exp_avg_sq 8.857e-07 | 8.857e-07;
    the two rows that stop receiving gradients: 5.191e-07 | 5.191e-07, 3.346e-05 | 3.346e-05, 9.796e-07 | 9.796e-07.
    (exp_avg nearly cancels where gradients change sign: one entry sets its figure, which is why the moments have to carry
    torch's own roundings for the 2x bar to mean anything. They do: equal figures are equal bits.)"""
    gen = torch.Generator().manual_seed(20)
    init = [torch.randn(46, 64, generator=gen), torch.randn(1, 64, generator=gen), torch.randn(2, 64, generator=gen)]
    trio = Trio(init, [1e-3] * 3, lr=0.0, eps=1e-15)
    scale = (10.0 ** (torch.arange(46, dtype=torch.float64) - 30.0))[:, None]
    start = [_np(t).copy() for t in init]
    mid = None
    for step in range(50):
        g0 = (torch.randn(46, 64, generator=gen).double() * scale).float()
        g1 = torch.randn(1, 64, generator=gen) * 1e20
        g2 = torch.randn(2, 64, generator=gen) * 1e-2
        g2[0] = 0.0                                        # never a gradient
        if step >= 10:
            g2[1] = 0.0                                    # none after step 10
        trio.set_grads([g0, g1, g2])
        trio.step()
        if step == 10:
            mid = [x[1].copy() for x in trio.tensors(2)]
    assert float(g0[0].abs().min()) > 0 and float((g0[10] * g0[10]).max()) < float(np.finfo(np.float32).tiny)   # g*g subnormal
    for name, h, t, r in trio.tensors(0):
        _assert_within_torch_bar(h[FIRST_WELL:], t[FIRST_WELL:], r[FIRST_WELL:], f"sweep {name} rows 1e-18..1e15")
        _assert_like_torch_fp32(name, h[:FIRST_WELL], t[:FIRST_WELL], f"sweep {name} rows 1e-30..1e-19")
    for name, h, t, _ in trio.tensors(1):
        _assert_like_torch_fp32(name, h, t, f"sweep {name} row 1e20")
    (_, p, pt, _), (_, m, _, _), (_, v, _, _) = list(trio.tensors(2))
    assert np.array_equal(p[0], start[2][0])                # zero gradient for ever: bit-unchanged, moments exactly zero
    assert not m[0].any() and not v[0].any()
    assert np.all(np.abs(m[1]) < np.abs(mid[1][1])) and np.all(v[1] < mid[2][1]) and np.all(v[1] > 0)   # the moments decay
    assert np.all(p[1] != mid[0][1])                        # ... and the parameter keeps moving
    for name, h, t, r in trio.tensors(2):
        _assert_within_torch_bar(h, t, r, f"sweep {name} zero rows")


# ------------------------------------------------------------------------------------------------ 2. element counts

NUMELS = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 2047, 2049, 4 * 1024 * 3 + 1]
GUARD = 12345.0


def _packed_layout():
    """Offsets (in floats, multiples of 4 = 16 bytes) of the tensors in one flat buffer; the words between them are guards."""
    offs, cur = [], 4
    for n in NUMELS:
        offs.append(cur)
        cur = (cur + n + 3) // 4 * 4 + 4
    return offs, cur


def test_packed_layout_is_aligned_and_guarded():
    offs, total = _packed_layout()
    used = np.zeros(total, bool)
    for o, n in zip(offs, NUMELS):
        assert o % 4 == 0 and not used[o:o + n].any()
        used[o:o + n] = True
        assert not used[o - 1] and not used[o + n]          # a guard word on either side of every tensor
    assert used.sum() == sum(NUMELS)


@pytest.mark.gpu
def test_element_counts_in_adjacent_memory(built_lib):
    """Float4 body, scalar tail and the 1024-element block edge, with every tensor's neighbours right behind it in memory:
    an element updated twice, skipped, or written past the end shows in the tensor, in its neighbour or in a guard word."""
    from dreamscene_amd.optim import FusedAdam
    offs, total = _packed_layout()
    gen = torch.Generator().manual_seed(21)
    bufs = {k: torch.full((total,), GUARD, device=DEV) for k in ("p", "g", "m", "v")}
    used = torch.zeros(total, dtype=torch.bool)
    view = lambda k, i: bufs[k][offs[i]:offs[i] + NUMELS[i]]
    cpu = []
    for i, n in enumerate(NUMELS):
        used[offs[i]:offs[i] + n] = True
        t = torch.randn(n, generator=gen)
        cpu.append(t.clone().requires_grad_(True))
        view("p", i).copy_(t)
        view("m", i).zero_()
        view("v", i).zero_()
    hip = [view("p", i).requires_grad_(True) for i in range(len(NUMELS))]
    assert all(p.data_ptr() % 16 == 0 and p.is_leaf for p in hip)
    lrs = [1e-2 * (1 + i) for i in range(len(NUMELS))]
    opt = FusedAdam(_groups(hip, lrs), eps=1e-15)
    ref = torch.optim.Adam(_groups(cpu, lrs), eps=1e-15)
    for i, p in enumerate(hip):
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": view("m", i), "exp_avg_sq": view("v", i)}
    guards = (~used).to(DEV)
    for step in range(3):
        for i, n in enumerate(NUMELS):
            g = torch.randn(n, generator=gen)
            cpu[i].grad = g.clone()
            view("g", i).copy_(g)
        ref.step()
        opt.step(grads=[view("g", i) for i in range(len(NUMELS))], zero_grad=(step == 1))
        for k in bufs:
            assert bool((bufs[k][guards] == GUARD).all()), f"step {step}: a guard word of the {k} buffer was written"
        if step == 1:
            assert not bool(bufs["g"][used.to(DEV)].any())
        for i, (a, b) in enumerate(zip(cpu, hip)):
            sa = ref.state[a]
            h, t = _np(b), _np(a)
            np.testing.assert_allclose(h, t, rtol=P_RTOL, atol=P_ATOL, err_msg=f"step {step} numel {NUMELS[i]}")
            for e in (0, -1):                               # the first element and the last one, next to the neighbour
                assert abs(float(h[e]) - float(t[e])) <= P_ATOL + P_RTOL * abs(float(t[e])), (step, NUMELS[i], e)
            for key, kb in (("exp_avg", "m"), ("exp_avg_sq", "v")):
                r = _np(sa[key])
                np.testing.assert_allclose(_np(view(kb, i)), r, rtol=M_RTOL, atol=M_RTOL * float(np.abs(r).max()),
                                           err_msg=f"step {step} numel {NUMELS[i]} {key}")
    assert all(float(opt.state[p]["step"]) == 3.0 for p in hip)


# ------------------------------------------------------------------------------------------------ 3. > 32 parameters

def _seventy(gen):
    sizes = [1, 5, 64, 1000, 1024, 1025, 3000, (7, 3), (33, 15, 3), 2]
    return [torch.randn(sizes[k % len(sizes)], generator=gen) for k in range(70)]


def _two_betas_two_eps(k):
    return {"betas": (0.9, 0.999) if k % 2 == 0 else (0.8, 0.99), "eps": 1e-15 if (k // 2) % 2 == 0 else 1e-8}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["distinct-lr", "two-betas-two-eps", "grad-none-on-second-step"])
def test_seventy_groups(built_lib, variant):
    """70 groups: three launches per step at least (32 + 32 + 6), each with its own step sizes; more when betas, eps or the
    step count split the batch."""
    gen = torch.Generator().manual_seed(22)
    init = _seventy(gen)
    lrs = [1e-3 * (1.0 + 0.37 * k) for k in range(70)]
    trio = Trio(init, lrs, extra=_two_betas_two_eps if variant == "two-betas-two-eps" else None, with_f64=False,
                lr=0.0, eps=1e-15)
    for step in range(3):
        grads = [torch.randn(t.shape, generator=gen) * (10.0 ** (k % 5 - 2)) for k, t in enumerate(init)]
        if variant == "grad-none-on-second-step" and step == 1:
            grads = [None if k % 3 == 0 else g for k, g in enumerate(grads)]
        trio.set_grads(grads)
        trio.step()
        trio.assert_matches_torch(f"{variant} step {step}")
    steps = [float(trio.opt.state[p]["step"]) for p in trio.hip]
    if variant == "grad-none-on-second-step":
        assert steps == [2.0 if k % 3 == 0 else 3.0 for k in range(70)]
    else:
        assert steps == [3.0] * 70


# ------------------------------------------------------------------------------------------------ 4. empty groups

@pytest.mark.gpu
def test_empty_parameters_and_empty_groups(built_lib):
    gen = torch.Generator().manual_seed(23)
    init = [torch.zeros(0), torch.randn(5, generator=gen), torch.zeros(0, 3), torch.randn(1030, generator=gen),
            torch.randn(2049, generator=gen), torch.zeros(0)]
    trio = Trio(init, [1e-2, 2e-2, 3e-2, 4e-2, 5e-2, 6e-2], with_f64=False, eps=1e-15)
    for o in (trio.opt, trio.ref):
        o.add_param_group({"params": [], "lr": 7e-2})
    for step in range(2):
        trio.set_grads([torch.randn(t.shape, generator=gen) for t in init])
        trio.step(zero_grad=(step == 1))
        trio.assert_matches_torch(f"step {step}")
    assert all(float(trio.opt.state[p]["step"]) == 2.0 for p in trio.hip)
    assert all(not bool(p.grad.any()) for p in trio.hip)


# ------------------------------------------------------------------------------------------------ 5. long horizons

@pytest.mark.gpu
@pytest.mark.parametrize("t", [9, 999, 9999, 29999])
def test_one_step_after_a_long_history(built_lib, t):
    """step_size = lr / (1 - beta1^t) and sqrt(1 - beta2^t) near their limits: one step from `step` = t with moments as a
    long run leaves them. Measured on an MI355X, 3 000 entries, HIP | torch-fp32 from float64: parameter 5.8e-08 | 5.8e-08 ...
    6.2e-08, exp_avg 5.3e-06 ... 3.7e-05 (equal), exp_avg_sq 1.2e-07 (equal) at every t."""
    gen = torch.Generator().manual_seed(24 + t)
    # |p| in [1, 2): a parameter that its own update nearly cancels has no well-conditioned relative distance
    init = [_away_from_zero((3000,), gen), _away_from_zero((5, 7), gen)]
    trio = Trio(init, [1e-2, 1.6e-4], lr=0.0, eps=1e-15)
    for k, p in enumerate(init):
        m = torch.randn(p.shape, generator=gen) * 0.1
        v = torch.rand(p.shape, generator=gen) * 1e-2 + 1e-6
        trio.set_state(k, t, m, v)
    trio.set_grads([torch.randn(p.shape, generator=gen) * 0.3 for p in init])
    trio.step()
    for k in range(2):
        assert float(trio.opt.state[trio.hip[k]]["step"]) == float(t + 1) == float(trio.ref.state[trio.t32[k]]["step"])
        for name, h, t32, r in trio.tensors(k):
            _assert_within_torch_bar(h, t32, r, f"t={t + 1} p{k} {name}")
    trio.assert_matches_torch(f"t={t + 1}")


# ------------------------------------------------------------------------------------------------ 6. grads= forms

def _sh_case(gen):
    from dreamscene_amd.optim import FusedAdam
    P = 777
    buf = torch.randn(P, 16, 3, generator=gen)
    dc, rest = torch.randn(P, 1, 3, generator=gen), torch.randn(P, 15, 3, generator=gen)
    cpu = [dc.clone().requires_grad_(True), rest.clone().requires_grad_(True)]
    hip = [dc.to(DEV).requires_grad_(True), rest.to(DEV).requires_grad_(True)]
    cpu[0].grad, cpu[1].grad = buf[:, :1].clone(), buf[:, 1:].clone()
    lrs = [2.5e-3, 1.25e-4]
    return buf.to(DEV), cpu, hip, FusedAdam(_groups(hip, lrs), eps=1e-15), torch.optim.Adam(_groups(cpu, lrs), eps=1e-15)


@pytest.mark.gpu
@pytest.mark.parametrize("zero_grad", [False, True])
def test_noncontiguous_grads_from_one_sh_buffer(built_lib, zero_grad):
    """f_dc and f_rest fed from shs_grad[:, :1] and shs_grad[:, 1:] of one [P, 16, 3] buffer. With zero_grad the CALLER's
    buffer must be zero afterwards (the kernel only sees a contiguous copy): otherwise the next backward accumulates onto
    stale values."""
    buf, cpu, hip, opt, ref = _sh_case(torch.Generator().manual_seed(25))
    before = buf.clone()
    views = [buf[:, :1], buf[:, 1:]]
    assert not views[0].is_contiguous() and not views[1].is_contiguous()
    opt.step(grads=views, zero_grad=zero_grad)
    ref.step()
    for a, b in zip(cpu, hip):
        np.testing.assert_allclose(_np(b), _np(a), rtol=P_RTOL, atol=P_ATOL)
    if zero_grad:
        assert not bool(buf.any()), "zero_grad=True left values in the caller's gradient buffer"
    else:
        assert torch.equal(buf, before)
    assert all(p.grad is None for p in hip)


@pytest.mark.gpu
@pytest.mark.parametrize("zero_grad", [False, True])
def test_noncontiguous_dot_grad(built_lib, zero_grad):
    from dreamscene_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(26)
    w = torch.randn(64, 64, generator=gen)
    buf = torch.randn(64, 64, generator=gen)
    a, b = w.clone().requires_grad_(True), w.to(DEV).requires_grad_(True)
    dbuf = buf.to(DEV)
    a.grad, b.grad = buf.t().clone(), dbuf.t()
    assert not b.grad.is_contiguous()
    opt, ref = FusedAdam([b], lr=1e-2, eps=1e-15), torch.optim.Adam([a], lr=1e-2, eps=1e-15)
    opt.step(zero_grad=zero_grad)
    ref.step()
    np.testing.assert_allclose(_np(b), _np(a), rtol=P_RTOL, atol=P_ATOL)
    if zero_grad:
        assert not bool(b.grad.any()) and not bool(dbuf.any())
    else:
        assert torch.equal(dbuf, buf.to(DEV))


@pytest.mark.gpu
def test_refused_calls_change_nothing(built_lib):
    from dreamscene_amd._lib import GsrError
    from dreamscene_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(27)
    ps = [torch.randn(100, 3, generator=gen).to(DEV).requires_grad_(True) for _ in range(3)]
    opt = FusedAdam(_groups(ps, [1e-2, 2e-2, 3e-2]), eps=1e-15)
    good = [torch.randn(100, 3, generator=gen).to(DEV) for _ in range(3)]
    opt.step(grads=good)

    def snapshot(o, params, grads):
        return ([p.detach().clone() for p in params], [g.clone() for g in grads],
                [(float(o.state[p]["step"]), o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone())
                 if len(o.state[p]) else None for p in params], [p._version for p in params])

    def same(x, y):
        assert all(torch.equal(a, b) for a, b in zip(x[0], y[0])) and all(torch.equal(a, b) for a, b in zip(x[1], y[1]))
        for s, t in zip(x[2], y[2]):
            assert (s is None) == (t is None)
            assert s is None or (s[0] == t[0] and torch.equal(s[1], t[1]) and torch.equal(s[2], t[2]))
        assert x[3] == y[3]

    # the offending entry is the LAST one: everything before it has been looked at when the call is refused
    bad_lists = {
        "too short": good[:2],
        "too long": good + [good[0]],
        "wrong shape": good[:2] + [torch.randn(3, 100, generator=gen).to(DEV)],
        "wrong dtype": good[:2] + [good[2].double()],
        "wrong device": good[:2] + [good[2].cpu()],
    }
    for what, grads in bad_lists.items():
        snap = snapshot(opt, ps, good)
        with pytest.raises(ValueError):
            opt.step(grads=grads, zero_grad=True)
        same(snap, snapshot(opt, ps, good))

    host = torch.randn(100, 3, generator=gen).requires_grad_(True)         # a CPU parameter behind two good ones
    mixed = ps[:2] + [host]
    opt2 = FusedAdam(_groups(mixed, [1e-2, 2e-2, 3e-2]), eps=1e-15)
    for p, g in zip(mixed, good):
        p.grad = g.to(p.device).clone()
    gl = [p.grad for p in mixed]
    snap = snapshot(opt2, mixed, gl)
    with pytest.raises(GsrError):
        opt2.step(zero_grad=True)
    same(snap, snapshot(opt2, mixed, gl))
    assert all(len(opt2.state[p]) == 0 for p in mixed)
    for p in mixed:
        p.grad = None


# ------------------------------------------------------------------------------------------------ 7. versions, set_to_none

@pytest.mark.gpu
def test_version_counters_and_set_to_none(built_lib):
    from dreamscene_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(28)
    ps = [torch.randn(n, generator=gen).to(DEV).requires_grad_(True) for n in (10, 2000, 3)]
    opt = FusedAdam(ps, lr=1e-2, eps=1e-15)
    ps[0].grad, ps[1].grad = torch.randn(10, generator=gen).to(DEV), torch.randn(2000, generator=gen).to(DEV)
    before = [p._version for p in ps]
    untouched = ps[2].detach().clone()
    opt.step()
    assert ps[0]._version > before[0] and ps[1]._version > before[1]
    assert ps[2]._version == before[2] and torch.equal(ps[2].detach(), untouched) and len(opt.state[ps[2]]) == 0
    assert ps[0].grad is not None                              # plain step(): the gradients stay
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen).to(DEV)
    before = [p._version for p in ps]
    opt.step(set_to_none=True)
    assert all(p.grad is None for p in ps)
    assert all(p._version > v for p, v in zip(ps, before))
    assert [float(opt.state[p]["step"]) for p in ps] == [2.0, 2.0, 1.0]


# ------------------------------------------------------------------------------------------------ 8. without a GPU

GSR_OK, GSR_EINVAL = 0, -1


def _group(L, numel=8, param=0x1000, grad=0x2000, m=0x3000, v=0x4000, lr=1e-3):
    g = L.GsrAdamGroup()
    g.param, g.grad, g.exp_avg, g.exp_avg_sq, g.numel, g.lr = param, grad, m, v, numel, lr
    return g


def test_adam_step_refuses_bad_arguments_before_any_device_call(built_lib):
    """Every call below returns from the host-side validation: the pointers are made up and never dereferenced."""
    from dreamscene_amd import _lib as L
    lib = built_lib
    arr = lambda *gs: (L.GsrAdamGroup * max(1, len(gs)))(*gs)
    call = lambda a, n, step=1, b1=0.9, b2=0.999, eps=1e-15: lib.gsr_adam_step(a, n, step, b1, b2, eps, 0, None)
    ok = _group(L)
    assert L.GSR_MAX_ADAM_GROUPS == 32
    assert call(arr(ok), -1) == GSR_EINVAL
    assert call((L.GsrAdamGroup * 33)(*[_group(L) for _ in range(33)]), 33) == GSR_EINVAL
    assert call(None, 1) == GSR_EINVAL
    assert call(arr(ok), 1, step=0) == GSR_EINVAL
    assert call(arr(ok), 1, step=-3) == GSR_EINVAL
    assert call(arr(ok), 1, b1=1.0) == GSR_EINVAL
    assert call(arr(ok), 1, b2=-1e-3) == GSR_EINVAL
    assert call(arr(ok), 1, b2=float("nan")) == GSR_EINVAL
    assert call(arr(ok, _group(L, numel=-1)), 2) == GSR_EINVAL
    for field in ("param", "grad", "m", "v"):
        assert call(arr(ok, _group(L, **{field: 0})), 2) == GSR_EINVAL, f"null {field}"
        assert call(arr(ok, _group(L, **{field: 0x5008})), 2) == GSR_EINVAL, f"misaligned {field}"
    assert call(arr(), 0) == GSR_OK
    empty = _group(L, numel=0, param=0, grad=0, m=0, v=0)
    assert call(arr(empty, empty, empty), 3) == GSR_OK
    assert call((L.GsrAdamGroup * 32)(*[empty] * 32), 32) == GSR_OK
