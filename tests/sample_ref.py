"""Numpy fp32 restatement of the seeded point clouds (SEMANTICS.md section 17; csrc/sample.hip): Philox-4x32-10 keyed by the seed,
counter (row index, block, cloud id, 3), 24-bit uniforms in (0,1), uniform e of a row = slot e % 4 of block e // 4, every operation
in fp32 in the order the kernels have it. Indoor env and floor and every colour use +, -, *, / and sqrt only, which are correctly
rounded on both sides: equal bits. The spherical, jitter and mesh coordinates pass through cbrtf / sinf / cosf, where libm and the
device differ by a few ulp: within 1e-5 of the cloud's radius, the bar tests/noise_ref.py states for the same generator (one ulp of
an angle <= 2 pi is 4.8e-7).
Test infrastructure: nothing under dreamscene_amd/ imports it."""
from __future__ import annotations

import math

import numpy as np

from tests.trajectory_ref import _philox4x32_10

TAG_SAMPLE = 3
ENV, FLOOR, BALL, JITTER_OFFSETS, JITTER_COLORS, MESH = range(6)
_f = np.float32
C0 = _f(0.28209479177387814)
TWO_PI, PI = _f(6.283185307179586), _f(3.141592653589793)


def uniforms(seed: int, cloud: int, index, count: int) -> np.ndarray:
    """[len(index), count] fp32: uniforms 0 .. count-1 of the rows `index` of (seed, cloud)."""
    seed &= 0xFFFFFFFFFFFFFFFF
    i = np.asarray(index, dtype=np.uint64)
    z = np.zeros_like(i)
    cols = []
    for j in range((count + 3) // 4):
        r = _philox4x32_10(i, z + np.uint64(j), z + np.uint64(cloud), z + np.uint64(TAG_SAMPLE), seed & 0xFFFFFFFF, seed >> 32)
        cols += [((x >> np.uint64(8)).astype(_f) + _f(0.5)) * _f(1.0 / 16777216.0) for x in r]
    return np.stack(cols[:count], 1).astype(_f)


def _rows(n: int, first: int = 0) -> np.ndarray:
    return np.arange(first, first + n, dtype=np.uint64)


def colour(rgb) -> np.ndarray:
    return np.minimum(np.asarray(rgb, _f) / _f(255.0), _f(1.0)).astype(_f)


def radius_base(box) -> float:
    b = np.abs(np.asarray(box, np.float64))
    return float(np.sqrt(np.sum(np.maximum(b[:3], b[3:]) ** 2)))


def outdoor_rows(box, density: int) -> int:
    return int(math.ceil(radius_base(box) * density))


def _sphere(r, c, phi):
    s = np.sqrt(np.maximum(_f(0), _f(1) - c * c))
    return np.stack([r * s * np.cos(phi), r * s * np.sin(phi), r * c], 1).astype(_f)


def _sh_colour(u):
    return (u / _f(255.0) * C0 + _f(0.5)).astype(_f)


def env_indoor(seed: int, box, n: int):
    """(points [5n,3], colors [5n,3])"""
    b = np.asarray(box, _f)
    u = uniforms(seed, ENV, _rows(n), 9)
    lo = [b[k] - u[:, k] / _f(50) for k in range(3)]
    hi = [b[3 + k] + u[:, 3 + k] / _f(50) for k in range(3)]
    xs, ys, zs = (u[:, 6 + k] * (b[3 + k] - b[k]) + b[k] for k in range(3))
    sheets = [(lo[0], ys, zs), (hi[0], ys, zs), (xs, lo[1], zs), (xs, hi[1], zs), (xs, ys, hi[2])]
    pts = np.concatenate([np.stack(s, 1) for s in sheets]).astype(_f)
    col = np.repeat(np.array([0.5, 0.5, 0.7, 0.7, 0.9], _f), n)[:, None] * np.ones((1, 3), _f)
    return pts, col.astype(_f)


def floor_indoor(seed: int, box, rgb, n: int):
    b = np.asarray(box, _f)
    u = uniforms(seed, FLOOR, _rows(n), 3)
    xs = u[:, 1] * (b[3] - b[0]) + b[0]
    ys = u[:, 2] * (b[4] - b[1]) + b[1]
    z = b[2] + u[:, 0] / _f(50) - _f(0.01)
    return np.stack([xs, ys, z], 1).astype(_f), np.tile(colour(rgb), (n, 1))


def env_outdoor(seed: int, box, rgb, n: int, zero_ground: bool):
    R = _f(radius_base(box))
    u = uniforms(seed, ENV, _rows(n), 3)
    c = u[:, 1] if zero_ground else _f(2) * u[:, 1] - _f(1)
    mu = u[:, 2] / _f(10) + _f(0.95)
    return _sphere(R * np.cbrt(mu), c, TWO_PI * u[:, 0]), np.tile(colour(rgb), (n, 1))


def floor_outdoor(seed: int, box, rgb, n: int):
    R = _f(radius_base(box))
    u = uniforms(seed, FLOOR, _rows(n), 3)
    r, phi = R * np.sqrt(u[:, 0]), TWO_PI * u[:, 1]
    z = u[:, 2] / _f(10) - _f(0.1) + _f(np.asarray(box, np.float64)[2])
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(_f), np.tile(colour(rgb), (n, 1))


def ball(seed: int, n: int, radius: float, cloud: int = BALL, no_cbrt: bool = False, uniform_theta: bool = False):
    """no_cbrt / uniform_theta: two WRONG samplers (radius without the cube root; polar angle uniform in the angle), which the
    analytic test has to tell from the right one."""
    u = uniforms(seed, cloud, _rows(n), 6)
    mu = u[:, 2] if no_cbrt else np.cbrt(u[:, 2])
    c = np.cos(PI * u[:, 1]) if uniform_theta else _f(2) * u[:, 1] - _f(1)
    return _sphere(_f(radius) * mu, c, TWO_PI * u[:, 0]), _sh_colour(u[:, 3:6])


def jitter_offsets(seed: int, copies: int, radius: float) -> np.ndarray:
    u = uniforms(seed, JITTER_OFFSETS, _rows(copies), 3)
    theta, phi, rho = PI * u[:, 0], TWO_PI * u[:, 1], _f(radius) * u[:, 2]
    st = np.sin(theta)
    return np.stack([rho * st * np.sin(phi), rho * st * np.cos(phi), rho * np.cos(theta)], 1).astype(_f)


def jitter(seed: int, points, colors, copies: int = 20, radius: float = 0.05, use_colors: bool = False):
    p = np.asarray(points, _f)
    n = p.shape[0]
    off = jitter_offsets(seed, copies, radius)
    base = np.stack([p[:, 0], -p[:, 1], p[:, 2] + _f(0.15)], 1)
    pts = (base[:, None, :] + off[None, :, :]).reshape(-1, 3).astype(_f)
    u = uniforms(seed, JITTER_COLORS, _rows(n * copies), 3)
    if use_colors:
        col = np.repeat(np.asarray(colors, _f), copies, axis=0) + _f(1e-4) * u
    else:
        col = _sh_colour(u)
    return pts, col.astype(_f)


def mesh_areas(vertices, faces) -> np.ndarray:
    v, f = np.asarray(vertices, _f), np.asarray(faces, np.int64)
    e0, e1 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    nx = e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1]
    ny = e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2]
    nz = e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]
    return (_f(0.5) * np.sqrt(nx * nx + ny * ny + nz * nz)).astype(_f)


def mesh(seed: int, vertices, faces, n: int):
    """(points, colors, triangle [n])"""
    v, f = np.asarray(vertices, _f), np.asarray(faces, np.int64)
    cdf = np.cumsum(mesh_areas(v, f).astype(np.float64))
    cdf = cdf / cdf[-1]
    u = uniforms(seed, MESH, _rows(n), 6)
    tri = np.minimum(np.searchsorted(cdf, u[:, 0].astype(np.float64), side="right"), len(f) - 1)
    q = np.sqrt(u[:, 1])
    wa, wb, wc = (_f(1) - q)[:, None], (q * (_f(1) - u[:, 2]))[:, None], (q * u[:, 2])[:, None]
    p = wa * v[f[tri, 0]] + wb * v[f[tri, 1]] + wc * v[f[tri, 2]]
    p = p[:, [0, 2, 1]].astype(_f)
    mean = p.astype(np.float64).mean(axis=0).astype(_f)
    return ((p - mean) / _f(80)).astype(_f), _sh_colour(u[:, 3:6]), tri.astype(np.int32)
