"""The checker of dreamscene_amd.densify's densify_and_prune / prune / prune_points: GaussianModel's densification
(gs_renderer.py:854-1059) restated in plain torch ops over an optimizer whose groups are named xyz, f_dc, f_rest, opacity,
scaling, rotation (and, left alone, background), on any device. The one change: the split's `torch.normal(mean=0, std)` is
`noise[c, i] * std` with explicit standard normals `noise` [N, P0, 3], so results can be compared entry by entry.
tests/test_densify.py pins this file to the reference's own functions through tests/golden/densify.npz.

Test infrastructure: nothing under dreamscene_amd/ imports it. The statistics are [P] tensors as DensifyStats holds them
(the reference keeps xyz_gradient_accum and denom as [P,1]; no arithmetic depends on that)."""
import torch
from torch import nn

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def rotation_matrices(q: torch.Tensor) -> torch.Tensor:
    """build_rotation (gs_renderer.py:124-145): the rotation matrix of q / |q|, q = (r, x, y, z)."""
    n = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    u = q / n[:, None]
    r, x, y, z = u[:, 0], u[:, 1], u[:, 2], u[:, 3]
    R = torch.zeros((q.shape[0], 3, 3), dtype=q.dtype, device=q.device)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


class RefGaussians:
    """The six leaves live in the optimizer's groups (as in the reference, where GaussianModel._xyz IS group["params"][0]); this
    object adds the three statistics and, for the tests, where every row came from: origin [P] (row of the model the object was
    built on) and kind [P] (0 original, 1 clone, 2 + c child of copy c)."""

    def __init__(self, optimizer, xyz_gradient_accum, denom, max_radii2D, percent_dense=0.01):
        self.optimizer = optimizer
        self.percent_dense = percent_dense
        self.xyz_gradient_accum, self.denom, self.max_radii2D = xyz_gradient_accum, denom, max_radii2D
        P = self.leaf("xyz").shape[0]
        dev = self.leaf("xyz").device
        self.origin = torch.arange(P, device=dev)
        self.kind = torch.zeros(P, dtype=torch.long, device=dev)

    # ---- access
    def groups(self):
        return [g for g in self.optimizer.param_groups if g["name"] != "background"]

    def leaf(self, name):
        return next(g for g in self.optimizer.param_groups if g["name"] == name)["params"][0]

    def leaves(self):
        return {n: self.leaf(n) for n in NAMES}

    def moments(self):
        out = {}
        for n in NAMES:
            st = self.optimizer.state.get(self.leaf(n), None)
            if st is not None:
                out[n] = (st["exp_avg"], st["exp_avg_sq"])
        return out

    def scales(self):
        return torch.exp(self.leaf("scaling"))

    def opacities(self):
        return torch.sigmoid(self.leaf("opacity"))

    # ---- optimizer surgery (gs_renderer.py:870-939)
    def _swap(self, group, tensor, m1, m2):
        old = group["params"][0]
        st = self.optimizer.state.get(old, None)
        new = nn.Parameter(tensor.requires_grad_(True))
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = m1(st["exp_avg"]), m2(st["exp_avg_sq"])
            del self.optimizer.state[old]
            self.optimizer.state[new] = st
        group["params"][0] = new

    def keep_rows(self, keep):
        """prune_points with valid_points_mask = keep."""
        for g in self.groups():
            self._swap(g, g["params"][0][keep], lambda m: m[keep], lambda m: m[keep])
        self.xyz_gradient_accum = self.xyz_gradient_accum[keep]
        self.denom = self.denom[keep]
        self.max_radii2D = self.max_radii2D[keep]
        self.origin, self.kind = self.origin[keep], self.kind[keep]

    def append_rows(self, new, origin, kind):
        """densification_postfix: concatenate, zero moments for the new rows, statistics reset to zeros."""
        for g in self.groups():
            ext = new[g["name"]]
            grow = lambda m, ext=ext: torch.cat((m, torch.zeros_like(ext)), dim=0)
            self._swap(g, torch.cat((g["params"][0], ext), dim=0), grow, grow)
        P = self.leaf("xyz").shape[0]
        dev = self.leaf("xyz").device
        self.xyz_gradient_accum = torch.zeros(P, device=dev)
        self.denom = torch.zeros(P, device=dev)
        self.max_radii2D = torch.zeros(P, device=dev)
        self.origin, self.kind = torch.cat((self.origin, origin)), torch.cat((self.kind, kind))

    # ---- densification (gs_renderer.py:971-1059)
    def clone(self, grads, grad_threshold, scene_extent):
        sel = grads.abs() >= grad_threshold            # torch.norm over the reference's trailing dimension of one
        sel = torch.logical_and(sel, torch.max(self.scales(), dim=1).values <= self.percent_dense * scene_extent)
        new = {n: p[sel] for n, p in self.leaves().items()}
        self.append_rows(new, self.origin[sel], torch.ones_like(self.kind[sel]))

    def split(self, grads, grad_threshold, scene_extent, N, noise):
        P = self.leaf("xyz").shape[0]
        padded = torch.zeros(P, device=grads.device)
        padded[:grads.shape[0]] = grads
        sel = padded >= grad_threshold
        sel = torch.logical_and(sel, torch.max(self.scales(), dim=1).values > self.percent_dense * scene_extent)
        stds = self.scales()[sel].repeat(N, 1)
        means = torch.zeros((stds.size(0), 3), device=stds.device)
        # the reference: samples = torch.normal(mean=means, std=stds); here the standard normals are given, [N, P0, 3]. Only
        # rows of the original P0 can be selected (the clones' padded gradient is 0 < grad_threshold).
        z = noise[:, self.origin[sel]].reshape(-1, 3)
        samples = z * stds + means
        rots = rotation_matrices(self.leaf("rotation")[sel]).repeat(N, 1, 1)
        new = {
            "xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self.leaf("xyz")[sel].repeat(N, 1),
            "scaling": torch.log(self.scales()[sel].repeat(N, 1) / (0.8 * N)),
            "rotation": self.leaf("rotation")[sel].repeat(N, 1),
            "f_dc": self.leaf("f_dc")[sel].repeat(N, 1, 1),
            "f_rest": self.leaf("f_rest")[sel].repeat(N, 1, 1),
            "opacity": self.leaf("opacity")[sel].repeat(N, 1),
        }
        n_sel = int(sel.sum())
        kind = torch.arange(N, device=sel.device).repeat_interleave(n_sel) + 2
        self.append_rows(new, self.origin[sel].repeat(N), kind)
        parents = torch.cat((sel, torch.zeros(N * n_sel, device=sel.device, dtype=torch.bool)))
        self.keep_rows(~parents)

    def _prune_mask(self, min_opacity, extent, max_screen_size):
        mask = (self.opacities() < min_opacity).squeeze(-1)
        if max_screen_size:
            big_vs = self.max_radii2D > max_screen_size
            big_ws = self.scales().max(dim=1).values > 0.1 * extent
            mask = torch.logical_or(torch.logical_or(mask, big_vs), big_ws)
        return mask

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, N=2, noise=None):
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        self.clone(grads, max_grad, extent)
        self.split(grads, max_grad, extent, N, noise)
        self.keep_rows(~self._prune_mask(min_opacity, extent, max_screen_size))

    def prune(self, min_opacity, extent, max_screen_size):
        self.keep_rows(~self._prune_mask(min_opacity, extent, max_screen_size))

    def prune_points(self, mask):
        self.keep_rows(~mask.bool())

    def segments(self, N):
        """(surviving originals, surviving clones, children of copy 0, copy 1, ...); rows are in exactly this order."""
        return tuple(int((self.kind == k).sum()) for k in range(2 + N))
