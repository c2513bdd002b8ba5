"""Numpy restatement of the seeded augmentation noise of the scene path (SEMANTICS.md "Seeded noise"; csrc/gsr_rng.h): Philox-4x32-10
keyed by the seed, counter (Gaussian index, block, stream, tag), four Box-Muller normals per block, formed in fp32 in the
order the kernels form them. libm's logf / cosf / sinf are within a few ulp of the device's, so the device's values are
within 1e-5 of these (one ulp of the angle, <= 6.28, is 4.8e-7; the radius is <= 5.89) -- the bar tests/trajectory_ref.py
states for the same generator."""
from __future__ import annotations

import numpy as np

from tests.trajectory_ref import _philox4x32_10

TAG_SCALE, TAG_SH = 1, 2
_f = np.float32


def _u01(x):
    return ((x >> np.uint64(8)).astype(_f) + _f(0.5)) * _f(1.0 / 16777216.0)


def normals4(seed: int, i, j: int, stream: int, tag: int) -> np.ndarray:
    """[len(i), 4] fp32: the four normals of block j of the Gaussians i."""
    seed &= 0xFFFFFFFFFFFFFFFF
    i = np.asarray(i, dtype=np.uint64)
    z = np.zeros_like(i)
    r = _philox4x32_10(i, z + np.uint64(j), z + np.uint64(stream & 0xFFFFFFFF), z + np.uint64(tag), seed & 0xFFFFFFFF,
                       seed >> 32)
    ra, ta = np.sqrt(_f(-2.0) * np.log(_u01(r[0]))), _f(6.283185307179586) * _u01(r[1])
    rb, tb = np.sqrt(_f(-2.0) * np.log(_u01(r[2]))), _f(6.283185307179586) * _u01(r[3])
    return np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], 1).astype(_f)


def scale_noise(seed: int, P: int, stream: int, first: int = 0) -> np.ndarray:
    """[P,3]: the scale noise of the Gaussians first .. first + P - 1."""
    return normals4(seed, np.arange(first, first + P, dtype=np.uint64), 0, stream, TAG_SCALE)[:, :3]


def sh_noise(seed: int, P: int, K: int, stream: int, first: int = 0) -> np.ndarray:
    """[P,K,3]: element e of the flattened [K,3] row is normal e % 4 of block e // 4."""
    F = 3 * K
    i = np.arange(first, first + P, dtype=np.uint64)
    blocks = [normals4(seed, i, j, stream, TAG_SH) for j in range((F + 3) // 4)]
    return np.concatenate(blocks, 1)[:, :F].reshape(P, K, 3)
