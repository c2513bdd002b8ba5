"""3D Gaussian filtering as the reference computes it (scene_gaussian.py:1046-1061, gs_renderer.py:1082-1087), restated on the CPU
with torch.sort: the yardstick of tests/test_filtering.py and tests/test_filtering_gpu.py. `dtype` torch.float32 is the reference's
own chain; torch.float64 is the same chain with every operation in double (the inputs are widened exactly). Not product code."""
import torch


def volume_rank(n: int) -> int:
    """`sorted_volume[index]` of the DESCENDING order, index = int(len(volume) * 0.9)."""
    return int(n * 0.9)


def threshold_rank(n: int, percent: float) -> int:
    """`sortedvalues[index_nth_percentile]` of the ASCENDING order."""
    return int(percent * (n - 1))


def v_imp_score(scaling_activated: torch.Tensor, imp_list: torch.Tensor, v_pow: float, dtype=torch.float32) -> torch.Tensor:
    scaling, imp = scaling_activated.cpu().to(dtype), imp_list.cpu().to(dtype)
    volume = torch.prod(scaling, dim=1)
    sorted_volume, _ = torch.sort(volume, descending=True)
    kth_percent_largest = sorted_volume[volume_rank(len(volume))]
    return torch.pow(volume / kth_percent_largest, v_pow) * imp


def prune_mask(v_list: torch.Tensor, percent: float) -> torch.Tensor:
    v = v_list.cpu().reshape(-1)
    sortedvalues, _ = torch.sort(v)
    return v <= sortedvalues[threshold_rank(v.shape[0], percent)]


def activate(scaling: torch.Tensor, activated: bool, dtype=torch.float32) -> torch.Tensor:
    scaling = scaling.cpu().to(dtype)
    return scaling if activated else torch.exp(scaling)


def filtering(scaling: torch.Tensor, activated: bool, imp_list: torch.Tensor, v_pow: float, percent: float, dtype=torch.float32):
    """-> (v_list, mask) of the whole chain in `dtype`."""
    v = v_imp_score(activate(scaling, activated, dtype), imp_list, v_pow, dtype)
    return v, prune_mask(v, percent)


def rel_err(v: torch.Tensor, v64: torch.Tensor) -> float:
    """The worst |v - v64| / |v64| over the entries where v64 is finite and not zero; the others must be equal."""
    v, v64 = v.cpu().double().reshape(-1), v64.cpu().double().reshape(-1)
    ok = torch.isfinite(v64) & (v64 != 0)
    assert torch.equal(torch.nan_to_num(v[~ok], nan=-1.0), torch.nan_to_num(v64[~ok].float().double(), nan=-1.0))
    return float(((v[ok] - v64[ok]).abs() / v64[ok].abs()).max()) if ok.any() else 0.0
