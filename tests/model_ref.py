"""The model's lifecycle in plain torch ops: the yardstick of tests/test_model_gpu.py's lifecycle test. `TorchModel` is
dreamscene_amd.model.GaussianModel with every call that launches one of the library's kernels (create_from_pcd past the kNN,
FusedAdam, the statistics, reset_opacity, densify_and_prune, prune_points, prune_gaussians) replaced by the chain of torch
operations it stands for: boolean-mask indexing, torch.optim.Adam, sort. It keeps the class's torch restatements of the surgery
(cat / prune / replace on the optimizer), which is what those exist for."""
import torch
from torch import nn

from dreamscene_amd import knn
from dreamscene_amd import model as M
from dreamscene_amd.densify import DensifyStats

C0 = 0.28209479177387814


class TorchModel(M.GaussianModel):
    def create_from_pcd(self, pcd, require_grad=True, spatial_lr_scale=1, *, dist2=None):
        self.spatial_lr_scale = spatial_lr_scale
        dev = torch.device(self.device)
        points = torch.tensor(pcd.points).float().to(dev)
        colors = torch.tensor(pcd.colors).float().to(dev)
        P, K = points.shape[0], (self.max_sh_degree + 1) ** 2
        d = knn.distCUDA2(points) if dist2 is None else dist2.to(dev).float()
        scales = torch.log(torch.sqrt(torch.clamp_min(d, 1e-7)))[:, None].repeat(1, 3)
        rots = torch.zeros(P, 4, device=dev)
        rots[:, 0] = 1
        # a correctly rounded division by fp32 C0 (dividing by the Python float multiplies by a reciprocal on the device)
        f_dc = ((colors - 0.5) / torch.tensor(C0, dtype=torch.float32, device=dev))[:, None, :]
        opacity = M.inverse_sigmoid(0.1 * torch.ones(P, 1, device=dev))
        leaf = lambda t: nn.Parameter(t.contiguous().requires_grad_(require_grad))
        self._xyz, self._features_dc, self._features_rest = leaf(points), leaf(f_dc), leaf(torch.zeros(P, K - 1, 3, device=dev))
        self._scaling, self._rotation, self._opacity = leaf(scales), leaf(rots), leaf(opacity)
        self._background = nn.Parameter(torch.zeros(3, 1, 1, device=dev).requires_grad_(require_grad))
        self.stats = DensifyStats(P, dev)

    def training_setup(self, training_args):
        super().training_setup(training_args)
        self.optimizer = torch.optim.Adam(self.optimizer.param_groups, lr=0.0, eps=1e-15)

    def add_densification_stats_div(self, viewspace_point_tensor, update_filter, cut_start, cut_end=None):
        grad = viewspace_point_tensor.grad[cut_start:cut_end] if cut_end else viewspace_point_tensor.grad[cut_start:]
        self.xyz_gradient_accum[update_filter] += torch.norm(grad[update_filter, :2], dim=-1, keepdim=True)
        self.denom[update_filter] += 1

    @torch.no_grad()
    def reset_opacity(self):
        capped = torch.min(self.get_opacity, torch.full_like(self._opacity, 0.01))
        self._opacity = self.replace_tensor_to_optimizer(M.inverse_sigmoid(capped), "opacity")["opacity"]

    def prune_points(self, mask):
        self._prune_points_torch(mask)

    @torch.no_grad()
    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, *, noise, N=2):
        grads = self.stats.mean_grad()[:, None]
        self.densify_and_clone(grads, max_grad, extent)
        # the split with the caller's normals, indexed [copy, original row]; clones sit behind the originals and are never chosen
        P = self._xyz.shape[0]
        padded = torch.zeros(P, device=self._xyz.device)
        padded[:grads.shape[0]] = grads.reshape(-1)
        scale = self.get_scaling
        chosen = (padded >= max_grad) & (scale.max(dim=1).values > self.percent_dense * extent)
        first = chosen[:noise.shape[1]]
        std = scale[chosen].repeat(N, 1)
        offset = noise[:, first].reshape(-1, 3) * std
        rot = M._rotation_matrices(self._rotation[chosen]).repeat(N, 1, 1)
        self.densification_postfix(
            torch.bmm(rot, offset[:, :, None])[:, :, 0] + self._xyz[chosen].repeat(N, 1),
            self._features_dc[chosen].repeat(N, 1, 1), self._features_rest[chosen].repeat(N, 1, 1),
            self._opacity[chosen].repeat(N, 1), torch.log(std / (0.8 * N)), self._rotation[chosen].repeat(N, 1))
        self.prune_points(torch.cat((chosen, torch.zeros(N * int(chosen.sum()), dtype=torch.bool, device=chosen.device))))
        doomed = (self.get_opacity < min_opacity).squeeze()
        if max_screen_size:
            doomed = doomed | (self.max_radii2D > max_screen_size) | (self.get_scaling.max(dim=1).values > 0.1 * extent)
        self.prune_points(doomed)

    def prune_gaussians(self, percent, important_score):
        ordered, _ = torch.sort(important_score.reshape(-1))
        self.prune_points(important_score.reshape(-1) <= ordered[int(percent * (ordered.shape[0] - 1))])
