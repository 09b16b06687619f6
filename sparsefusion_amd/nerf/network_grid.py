"""Instant-NGP field (tiled grid 16x2 -> MLP 32-64-64-4) on the HIP backend.

Same constructor, state-dict keys and optimiser grouping as the reference's NeRFNetwork
(external/nerf/network_grid.py:36-234): `encoder.embeddings [929336,2]`, `encoder.offsets [17]`,
`sigma_net.net.{0,1,2}.{weight,bias}`, `aabb_train`, `aabb_infer`.  sigma = trunc_exp(h0 +
5 exp(-|x|^2/0.08)), albedo = sigmoid(h1..3) (:69-88).

Two execution routes, both on the GPU library:
  * `render` / `run` (inherited): the fused render node (renderer.py);
  * `common_forward` / `density` / `forward` on arbitrary points: fused sf_ngp_density when no
    gradient is needed, otherwise HIP grid-encode op + torch linears (differentiable);
  * `finite_difference_normal` / `normal` / `forward(shading='lambertian')`: fused sf_ngp_point_attrs
    (seven field evaluations per point in one launch) when no gradient is needed, otherwise six
    `common_forward` calls as the reference composes them."""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..gridencoder import GridEncoder
from .renderer import NeRFRenderer, _FieldHandle
from .utils import safe_normalize


class MLP(nn.Module):
    def __init__(self, dim_in, dim_out, dim_hidden, num_layers, bias=True):
        super().__init__()
        self.dim_in, self.dim_out, self.dim_hidden, self.num_layers = dim_in, dim_out, dim_hidden, num_layers
        widths = [dim_in] + [dim_hidden] * (num_layers - 1) + [dim_out]
        self.net = nn.ModuleList(nn.Linear(a, b, bias=bias) for a, b in zip(widths[:-1], widths[1:]))

    def forward(self, x):
        for i, layer in enumerate(self.net):
            x = layer(x)
            if i + 1 < self.num_layers:
                x = F.relu(x)
        return x


class _TruncExp(torch.autograd.Function):
    """exp forward, gradient clamped to exp(clamp(x, -15, 15)) (external/ngp_activation.py:10-23)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(x.clamp(-15, 15))


trunc_exp = _TruncExp.apply


class NeRFNetwork(NeRFRenderer):
    def __init__(self, opt, num_layers=3, hidden_dim=64, num_layers_bg=2, hidden_dim_bg=64):
        super().__init__(opt)
        if num_layers != 3 or hidden_dim != 64:
            raise NotImplementedError("the fused kernels are built for the reference 32-64-64-4 MLP")
        self.num_layers, self.hidden_dim = num_layers, hidden_dim
        # get_encoder('tiledgrid', input_dim=3, log2_hashmap_size=16, desired_resolution=2048*bound)
        # (network_grid.py:50, ngp_encoder.py:50-79)
        self.encoder = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=16,
                                   desired_resolution=2048 * self.bound, gridtype='tiled', align_corners=False)
        self.in_dim = self.encoder.output_dim
        self.sigma_net = MLP(self.in_dim, 4, hidden_dim, num_layers, bias=True)
        self.bg_net = None
        self._handle = None

    # ---- renderer hooks
    def _field_handle(self):
        if self._handle is None:
            self._handle = _FieldHandle(self)
        return self._handle

    def _field_params(self):
        lin = self.sigma_net.net
        return (self.encoder.embeddings, lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight,
                lin[2].bias)

    # ---- point queries
    def gaussian(self, x):
        d = (x ** 2).sum(-1)
        return 5 * torch.exp(-d / (2 * 0.2 ** 2))

    def _needs_grad(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def common_forward(self, x):
        """x [N,3] in [-bound,bound] -> sigma [N], albedo [N,3]."""
        if not self._needs_grad(x):
            _lib.require_cuda(x)
            xs = x.detach().reshape(-1, 3).float().contiguous()
            sigma = torch.empty(xs.shape[0], dtype=torch.float32, device=xs.device)
            albedo = torch.empty(xs.shape[0], 3, dtype=torch.float32, device=xs.device)
            params = [p.detach().contiguous() for p in self._field_params()]
            f = self._field_handle().struct(params)
            rc = _lib.lib().sf_ngp_density(C.byref(f), _lib.ptr(xs), xs.shape[0], _lib.ptr(sigma), _lib.ptr(albedo),
                                           _lib.stream_ptr())
            _lib.check(rc, "ngp_density")
            return sigma.view(x.shape[:-1]), albedo.view(*x.shape[:-1], 3)
        h = self.sigma_net(self.encoder(x, bound=self.bound))
        return trunc_exp(h[..., 0] + self.gaussian(x)), torch.sigmoid(h[..., 1:])

    def _point_attrs(self, x, epsilon, **want):
        """The fused route (no gradient): one sf_ngp_point_attrs launch, outputs shaped like x."""
        from .. import mesh
        out = mesh.point_attributes(self, x, epsilon, **want)
        return {k: v.view(x.shape[:-1]) if k == 'sigma' else v.view(*x.shape[:-1], 3) for k, v in out.items()}

    def finite_difference_normal(self, x, epsilon=1e-2):
        """network_grid.py:91-106: central differences of sigma over +-epsilon per axis, the offset points clamped to the box ->
        [..., 3] (not normalised).  Without a gradient it is one launch (the gradient output of sf_ngp_point_attrs); when a
        gradient is needed (the rule of common_forward) it is composed from six common_forward calls as the reference does."""
        if not self._needs_grad(x):
            return self._point_attrs(x, epsilon, sigma=False, albedo=False, normal=False)['grad']
        comps = []
        for a in range(3):
            side = []
            for e in (epsilon, -epsilon):
                o = [0.0, 0.0, 0.0]
                o[a] = e
                side.append(self.common_forward((x + torch.tensor([o], device=x.device)).clamp(-self.bound, self.bound))[0])
            comps.append(0.5 * (side[0] - side[1]) / epsilon)
        return torch.stack(comps, dim=-1)

    def normal(self, x, smooth=False):
        """network_grid.py:155-164: safe_normalize(finite_difference_normal(x)) with NaN set to 0."""
        if smooth:
            raise NotImplementedError(
                "normal(smooth=True) is not provided: the reference's smooth variant averages the field over torch.rand_like "
                "neighbourhoods of every offset point (network_grid.py:108-152), which is not a deterministic function of the field")
        if not self._needs_grad(x):
            return self._point_attrs(x, 1e-2, sigma=False, albedo=False, grad=False)['normal']
        normal = safe_normalize(self.finite_difference_normal(x))
        return torch.where(torch.isnan(normal), torch.zeros_like(normal), normal)

    def forward(self, x, d, l=None, ratio=1, shading='albedo'):
        """network_grid.py:167-197.  'albedo': (sigma, albedo, None).  'lambertian': (sigma, albedo * (ratio + (1 - ratio) *
        clamp(normal . (-l), min=0)), normal), with sigma, albedo and normal from ONE launch when no gradient is needed."""
        if shading == 'albedo':
            sigma, color = self.common_forward(x)
            return sigma, color, None
        if shading in ('normal', 'textureless'):
            raise NotImplementedError(
                f"shading={shading!r} uses the reference's smooth normal, an average over torch.rand_like neighbourhoods that is "
                "not a deterministic function of the field; 'albedo' and 'lambertian' are provided")
        if shading != 'lambertian':
            raise ValueError(f"unknown shading {shading!r}")
        if l is None:
            raise ValueError("shading='lambertian' needs the light direction l [3]")
        if not self._needs_grad(x):
            out = self._point_attrs(x, 1e-2, grad=False)
            sigma, albedo, normal = out['sigma'], out['albedo'], out['normal']
        else:
            sigma, albedo = self.common_forward(x)
            normal = self.normal(x)
        lambertian = ratio + (1 - ratio) * (normal @ -l).clamp(min=0)
        return sigma, albedo * lambertian.unsqueeze(-1), normal

    def density(self, x):
        sigma, albedo = self.common_forward(x)
        return {'sigma': sigma, 'albedo': albedo}

    def get_params(self, lr):
        """Adam groups of network_grid.py:223-234: table at 10x lr, MLP at lr."""
        return [{'params': self.encoder.parameters(), 'lr': lr * 10},
                {'params': self.sigma_net.parameters(), 'lr': lr}]
