"""Trainer-side geometry helpers of external/nerf/utils.py:174-204 with the marching cubes on the GPU (sparsefusion_amd.mesh),
and safe_normalize (:41)."""
import numpy as np
import torch

from .. import mesh


def safe_normalize(x, eps=1e-20):
    """external/nerf/utils.py:41: x / sqrt(clamp(sum(x^2, -1), min=eps))."""
    return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=eps))


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor):
            return x.device
    return torch.device("cpu")


@torch.no_grad()
def _fields(bound_min, bound_max, resolution, query_func, S=128):
    """The lattice of extract_fields as a float32 tensor on the device of query_func's output.  Points are built as the
    reference builds them (torch.linspace on the CPU, split into blocks of S, meshgrid indexing 'ij', x-major) and sent to the
    device of bound_min / bound_max before query_func sees them (there is no CPU path for the field)."""
    dev = _device_of(bound_min, bound_max)
    X = mesh.lattice_axis(bound_min[0], bound_max[0], resolution).split(S)
    Y = mesh.lattice_axis(bound_min[1], bound_max[1], resolution).split(S)
    Z = mesh.lattice_axis(bound_min[2], bound_max[2], resolution).split(S)
    u = None
    for xi, xs in enumerate(X):
        for yi, ys in enumerate(Y):
            for zi, zs in enumerate(Z):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).to(dev)      # [S^3, 3]
                val = query_func(pts).reshape(len(xs), len(ys), len(zs)).detach().float()
                if u is None:
                    u = torch.zeros(resolution, resolution, resolution, dtype=torch.float32, device=val.device)
                u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = val
    return u


def extract_fields(bound_min, bound_max, resolution, query_func, S=128):
    """external/nerf/utils.py:174-188: query_func on the resolution^3 lattice over [bound_min, bound_max], in blocks of S^3 in the
    reference's order -> u [R, R, R] float32 numpy (x-major)."""
    return _fields(bound_min, bound_max, resolution, query_func, S).cpu().numpy()


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func):
    """external/nerf/utils.py:191-204: marching cubes (on the GPU; no smoothing) of extract_fields at `threshold` ->
    (vertices [V, 3] float64 numpy scaled to the box as at :203, triangles [F, 3] int32 numpy)."""
    u = _fields(bound_min, bound_max, resolution, query_func)
    vertices, triangles = mesh.marching_cubes(u if u.is_cuda else u.numpy(), threshold)
    vertices = vertices.cpu().numpy() if isinstance(vertices, torch.Tensor) else vertices
    triangles = triangles.cpu().numpy() if isinstance(triangles, torch.Tensor) else triangles
    b_max_np = bound_max.detach().cpu().numpy() if isinstance(bound_max, torch.Tensor) else np.asarray(bound_max)
    b_min_np = bound_min.detach().cpu().numpy() if isinstance(bound_min, torch.Tensor) else np.asarray(bound_min)
    vertices = vertices / (resolution - 1.0) * (b_max_np - b_min_np)[None, :] + b_min_np[None, :]
    return vertices, triangles
