"""CPU: dreamscene_amd.filtering's host side. The yardstick tests/filter_ref.py reproduces the fixture recorded from the reference's
own functions (tests/golden/prune.npz); the two rank formulas agree with the reference's expressions; the launch shape the module
states is the one csrc/select.hip has; and the calls refuse bad arguments before any launch (there is no GPU here: a call that got
as far as a launch would fail differently)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import filter_ref
from tests.test_golden import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_ref_reproduces_the_reference_fixture():
    d = load("prune.npz")
    scaling, imp = torch.tensor(d["scaling"]), torch.tensor(d["imp"])
    v, mask = filter_ref.filtering(scaling, False, imp, float(d["v_pow"]), float(d["percent"]))
    np.testing.assert_allclose(v.numpy(), d["v_list"], rtol=1e-6)
    assert np.array_equal(mask.numpy(), d["mask"])
    assert np.array_equal(filter_ref.prune_mask(torch.tensor(d["v_list"]), float(d["percent"])).numpy(), d["mask"])
    # float64 takes the same decisions: the nearest other entry is 1.4e-3 of the threshold away
    v64, mask64 = filter_ref.filtering(scaling, False, imp, float(d["v_pow"]), float(d["percent"]), torch.float64)
    assert np.array_equal(mask64.numpy(), d["mask"])
    s = np.sort(v64.numpy())
    k = filter_ref.threshold_rank(len(s), float(d["percent"]))
    assert min(s[k] - s[k - 1], s[k + 1] - s[k]) > 1e-3 * s[k]


@pytest.mark.parametrize("n", range(1, 51))
def test_rank_formulas_are_the_reference_s(n):
    from dreamscene_amd import filtering as F
    x = torch.randperm(n, generator=torch.Generator().manual_seed(n)).float()
    descending, _ = torch.sort(x, descending=True)
    ascending, _ = torch.sort(x)
    k = F.volume_rank(n)
    assert 0 <= k < n and ascending[k] == descending[int(len(x) * 0.9)]
    for percent in (0, 0.3, 0.4, 1):
        k = F.threshold_rank(n, percent)
        assert 0 <= k < n and k == int(percent * (n - 1)) == filter_ref.threshold_rank(n, percent)
    assert F.threshold_rank(n, 0) == 0 and F.threshold_rank(n, 1) == n - 1


def test_module_states_the_kernels_launch_shape():
    from dreamscene_amd import filtering as F
    src = open(os.path.join(ROOT, "dreamscene_amd", "csrc", "select.hip")).read()
    const = {name: int(value) for name, value in re.findall(r"constexpr int (k\w+) = (\d+);", src)}
    assert F.BLOCK == const["kT"] and F.BLOCK_ITEMS == const["kT"] * const["kItems"] and F.MAX_BLOCKS == const["kMaxBlocks"]
    assert F.WAVE == 64 and const["kPasses"] == 4 and const["kBins"] == 256
    assert F.KTH_VALUE_LAUNCHES == 1 + const["kPasses"] + 1 and F.IMPORTANCE_FILTER_LAUNCHES == 1 + 2 * const["kPasses"] + 1


def test_select_is_built_without_fma_contraction():
    from dreamscene_amd import build
    assert "-ffp-contract=off" in build.SOURCES["select.hip"]


def test_arguments_are_checked_before_any_launch(built_lib):
    from dreamscene_amd import filtering as F
    from dreamscene_amd._lib import GsrError
    s, imp = torch.rand(5, 3) + 0.1, torch.rand(5)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="percent"):
            F.importance_filter(s, imp, 0.1, bad)
        with pytest.raises(ValueError, match="percent"):
            F.importance_prune_mask(imp, bad)
    with pytest.raises(ValueError, match="percent"):
        F.gaussian_filtering(None, [], torch.zeros(3), 0.1, 2.0, 0.6)      # 2.0 ** 1 * 0.6 > 1, before the model is looked at
    for call in (lambda: F.importance_filter(torch.zeros(0, 3), torch.zeros(0), 0.1, 0.4),
                 lambda: F.calculate_v_imp_score(torch.zeros(0, 3), torch.zeros(0), 0.1),
                 lambda: F.importance_prune_mask(torch.zeros(0), 0.4),
                 lambda: F.kth_value(torch.zeros(0), 0)):
        with pytest.raises(ValueError, match="n == 0"):
            call()
    for k in (-1, 5, 6):
        with pytest.raises(ValueError, match="outside"):
            F.kth_value(imp, k)
    # valid arguments on the CPU: refused, and the refusal names the device
    for call in (lambda: F.kth_value(imp, 2), lambda: F.kth_value(imp, 0, descending=True),
                 lambda: F.calculate_v_imp_score(s, imp, 0.1), lambda: F.importance_prune_mask(imp, 0.4),
                 lambda: F.importance_filter(s, imp, 0.1, 0.4), lambda: F.importance_filter(s.log(), imp, 0.1, 0.4, activated=False)):
        with pytest.raises(GsrError, match=r"on cpu.*no CPU\s+fallback"):
            call()


def test_c_entry_points_refuse_bad_counts_before_touching_anything(built_lib):
    """GSR_EINVAL for n <= 0 and for ranks outside [0, n) although every pointer is a made-up handle (a call that went on to
    a launch could not survive them quietly); the scratch size is 0 for an n that is not accepted and grows with n."""
    lib = built_lib
    assert lib.gsr_select_scratch_bytes(0) == 0 and lib.gsr_select_scratch_bytes(-3) == 0
    assert lib.gsr_select_scratch_bytes(1) % 16 == 0 and lib.gsr_select_scratch_bytes(1) >= 2 * 4 * 256 * 4 + 4
    assert lib.gsr_select_scratch_bytes(10_000) >= lib.gsr_select_scratch_bytes(1) + 4 * 9_999 - 16
    p = 0x1000
    for n, k in ((0, 0), (-1, 0), (5, -1), (5, 5)):
        assert lib.gsr_kth_value(p, n, k, p + 0x100, p + 0x1000, 1 << 20, None) == -1, (n, k)
    for n, kv, kt in ((0, 0, 0), (5, -1, 0), (5, 5, 0), (5, 0, 5), (5, 0, -1)):
        assert lib.gsr_importance_filter(p, 1, p + 0x100, n, 0.1, kv, kt, p + 0x200, p + 0x300, None, p + 0x1000, 1 << 20, None) == -1
    assert lib.gsr_kth_value(p, 5, 0, p + 0x100, p + 0x1000, 16, None) == -4              # GSR_ESCRATCH
    assert lib.gsr_kth_value(None, 5, 0, p + 0x100, p + 0x1000, 1 << 20, None) == -1
