"""The reference's frame tail (training/object_trainer.py:81-118, training/scene_trainer.py:261-340) in torch / numpy as the
reference writes it, and the crafted inputs of tests/test_frames.py and tests/test_frames_gpu.py."""
import numpy as np
import torch

H0, W0 = 37, 53                 # H*W = 1961 is odd: frames 1 and 2 start at odd byte addresses, every vector path has a tail
DIV_CROP = 25705                # offset of the 37x53 crop of division_plane() that keeps a division-sensitive pixel


def ref_rgb(image: torch.Tensor) -> np.ndarray:
    """[3,H,W] fp32 -> uint8 [H,W,3]"""
    a = torch.clamp(image, 0.0, 1.0).detach().cpu().permute(1, 2, 0).numpy()
    return (a * 255).round().astype(np.uint8)


def ref_depth(depth_alpha: torch.Tensor) -> np.ndarray:
    """[2,H,W] fp32 -> uint8 [H,W,1]. An all-zero depth plane is 0 / 0 in the reference and numpy's cast of NaN is undefined;
    the project defines byte 0 there (SEMANTICS.md "Frame export")."""
    depth = depth_alpha[0:1].detach().cpu()
    if float(depth.max()) == 0.0 and float(depth.min()) == 0.0:
        return np.zeros(tuple(depth.shape[1:]) + (1,), dtype=np.uint8)
    a = torch.clamp(depth / depth.max(), 0.0, 1.0).permute(1, 2, 0).numpy()
    return (a * 255).round().astype(np.uint8)


def ref_frames(images, depth_alphas=None):
    rgb = np.stack([ref_rgb(i) for i in images])
    return rgb, (None if depth_alphas is None else np.stack([ref_depth(d) for d in depth_alphas]))


def tie_candidates() -> np.ndarray:
    """x_k = fl32((k + 0.5) / 255), k = 0..254, each with both fp32 neighbours: 765 values around the rounding ties."""
    xk = ((np.arange(255) + 0.5) / 255).astype(np.float32)
    return np.concatenate([np.nextafter(xk, np.float32(-1)), xk, np.nextafter(xk, np.float32(2))]).astype(np.float32)


def tie_counts(x: np.ndarray):
    """(values whose fl32(x * 255) is exactly k + 0.5, values where rint and floor(y + 0.5) give different bytes)"""
    y = np.clip(np.asarray(x, np.float32), 0, 1) * np.float32(255)
    return int((y - np.floor(y) == 0.5).sum()), int((np.rint(y) != np.floor(y + np.float32(0.5))).sum())


def division_plane() -> np.ndarray:
    return np.random.default_rng(0).random(1 << 20, dtype=np.float32) * np.float32(7)


def division_sensitive(depth: np.ndarray) -> int:
    """Bytes of a depth plane that differ between depth / M and depth * (1 / M), all in fp32."""
    d = np.asarray(depth, np.float32).reshape(-1)
    M = d.max()
    byte = lambda q: (np.clip(q, 0, 1) * np.float32(255)).round().astype(np.uint8)
    return int((byte(d / M) != byte(d * (np.float32(1) / M))).sum())


def crafted_planes():
    """-> (images [3,3,37,53], depth_alphas [3,2,37,53]) fp32 CPU tensors.
    Every colour plane holds the 765 tie candidates, values < 0 and > 1, -0.0 and 1.0, at a different shift per plane (so
    they meet the dword and the byte stores, the full units and the tail). Depth: frame 0 = the division-sensitive crop with its
    maximum moved to the LAST pixel, frame 1 = all zero, frame 2 = its maximum in the FIRST pixel."""
    rng = np.random.default_rng(11)
    n = H0 * W0
    special = np.array([-0.0, 0.0, 1.0, -1.0, -1e-30, 1e-30, 2.0, 1.0000001, 0.99999994, 1e30, -1e30, 0.5], np.float32)
    base = np.concatenate([tie_candidates(), special])
    images = np.empty((3, 3, n), np.float32)
    for f in range(3):
        for c in range(3):
            fill = rng.uniform(-0.2, 1.2, n - base.size).astype(np.float32)
            images[f, c] = np.roll(np.concatenate([base, fill]), 7 * f + 3 * c + 1)
    da = rng.random((3, 2, n), dtype=np.float32)
    crop = division_plane()[DIV_CROP:DIV_CROP + n].copy()
    k = int(crop.argmax())
    crop[k], crop[n - 1] = crop[n - 1], crop[k]
    da[0, 0] = crop
    da[1, 0] = 0.0
    da[2, 0] = rng.random(n, dtype=np.float32) * np.float32(5)
    da[2, 0, 0] = 9.0
    return (torch.from_numpy(images.reshape(3, 3, H0, W0)), torch.from_numpy(da.reshape(3, 2, H0, W0)))


def random_planes(F, H, W, seed):
    """Colours a little outside [0, 1] and positive depths: what a render looks like, plus clamped ends."""
    g = torch.Generator().manual_seed(seed)
    images = torch.rand((F, 3, H, W), generator=g) * 1.2 - 0.1
    da = torch.rand((F, 2, H, W), generator=g)
    da[:, 0] *= 6.5
    return images, da
