"""Mesh export on the GPU: the NGP density on a lattice, PyMCubes' Gaussian smoothing, fp64 volume statistics and marching cubes
(C ABI in include/sparsefusion_hip.h, kernels in csrc/mesh_kernels.h and csrc/mesh.hip).

The functions take and return device tensors; numpy input is run on the current HIP device and comes back as numpy, as a `mcubes`
user would expect.  There is no CPU path.

Parity: PyMCubes is not available to pin against.  The smoothing restates its definition (scipy.ndimage.gaussian_filter, mode
'reflect', truncate 4.0) and is tested against scipy; the marching cubes use the classic Lorensen / Bourke tables in a canonical
order of this library's own (vertices point-major x-major then edge axis, faces cell-major x-major then table order), which
PyMCubes' vertex order, welding and winding are not checked against."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _as_device(vol, what):
    """(float32 contiguous device tensor, came_from_numpy)"""
    if isinstance(vol, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(f"cuda:{torch.cuda.current_device()}"), True
    if not isinstance(vol, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor or a numpy array, got {type(vol).__name__}")
    _lib.require_cuda(vol)
    return vol.detach().float().contiguous(), False


def _dims(vol, what):
    if vol.dim() != 3:
        raise ValueError(f"{what}: expected a 3-D volume [nx, ny, nz], got shape {tuple(vol.shape)}")
    return tuple(int(s) for s in vol.shape)


def lattice_axis(lo, hi, resolution):
    """One lattice axis as the reference builds it: torch.linspace on the CPU in float32 (the device linspace rounds differently)."""
    return torch.linspace(float(lo), float(hi), int(resolution), dtype=torch.float32)


def density_lattice_axes(net, ax, ay, az):
    """sigma [len(ax), len(ay), len(az)] float32 on the field's device: the density at every (ax[i], ay[j], az[k]), bit-identical to
    net.density on the same fp32 points, evaluated straight from the lattice index (no point buffer)."""
    params = [p.detach().contiguous() for p in net._field_params()]
    dev = params[0].device
    _lib.require_cuda(*params)
    ax, ay, az = (torch.as_tensor(a, dtype=torch.float32).to(dev).contiguous() for a in (ax, ay, az))
    nx, ny, nz = ax.numel(), ay.numel(), az.numel()
    sigma = torch.empty(nx, ny, nz, dtype=torch.float32, device=dev)
    f = net._field_handle().struct(params)
    rc = _lib.lib().sf_ngp_density_lattice(C.byref(f), _lib.ptr(ax), _lib.ptr(ay), _lib.ptr(az), nx, ny, nz, _lib.ptr(sigma),
                                           _lib.stream_ptr())
    _lib.check(rc, "ngp_density_lattice")
    return sigma


@torch.no_grad()
def density_lattice(net, resolution, bound):
    """sigma [R, R, R] of a NeRFNetwork at the lattice of export_mesh (renderer_df.py:134-146): X = Y = Z =
    torch.linspace(-bound, bound, R) on the CPU, sigma[x, y, z] = net.density(point)['sigma'] (indexing 'ij')."""
    a = lattice_axis(-bound, bound, resolution)
    return density_lattice_axes(net, a, a, a)


def smooth_gaussian(vol, sigma=1.5, truncate=4.0, return_stats=False):
    """mcubes.smooth_gaussian on the GPU: scipy.ndimage.gaussian_filter(vol, sigma) with mode 'reflect' and `truncate`, one pass
    per axis (0, 1, 2), the taps in double, each output rounded to float32.

    PyMCubes subtracts 0.5 first; this does not.  The taps sum to one, so the constant shifts the smoothed volume, its mean and
    therefore mean + 0.25 * std by the same 0.5: neither the iso surface nor the level relative to it moves.

    return_stats: also return {mean, population std} of the result (float64 [2] on the device; numpy for numpy input), reduced in a
    fixed order (bit-reproducible)."""
    v, from_np = _as_device(vol, "smooth_gaussian")
    nx, ny, nz = _dims(v, "smooth_gaussian")
    lib = _lib.lib()
    wbytes = lib.sf_gaussian3d_workspace_bytes(nx, ny, nz)
    if wbytes == 0:
        raise RuntimeError(f"smooth_gaussian: unsupported volume shape {(nx, ny, nz)}")
    out = torch.empty_like(v)
    work = torch.empty(wbytes, dtype=torch.uint8, device=v.device)
    stats = torch.empty(2, dtype=torch.float64, device=v.device) if return_stats else None
    rc = lib.sf_gaussian3d(_lib.ptr(v), _lib.ptr(out), nx, ny, nz, float(sigma), float(truncate), _lib.ptr(stats), _lib.ptr(work),
                           wbytes, _lib.stream_ptr())
    _lib.check(rc, "gaussian3d")
    if from_np:
        out = out.cpu().numpy()
        stats = stats.cpu().numpy() if stats is not None else None
    return (out, stats) if return_stats else out


def marching_cubes(volume, isovalue):
    """mcubes.marching_cubes on the GPU -> (vertices [V, 3] float32 in index coordinates of the array axes, faces [F, 3] int32).

    A corner is inside when v < float32(isovalue).  Vertices are welded (one per crossing lattice edge) and ordered point-major in
    x-major order, then by edge axis x < y < z; a vertex on the edge from lattice point a to a + e_axis sits at
    a + (iso - v_a) / (v_b - v_a) (float32).  Faces are ordered by cell (x-major), then table order, and look toward decreasing
    values (outward on a density blob).  One device-to-host read of the counts sizes the outputs."""
    v, from_np = _as_device(volume, "marching_cubes")
    nx, ny, nz = _dims(v, "marching_cubes")
    lib = _lib.lib()
    wbytes = lib.sf_mc_workspace_bytes(nx, ny, nz)
    if wbytes == 0:
        raise RuntimeError(f"marching_cubes: unsupported volume shape {(nx, ny, nz)} (vertex or face ids could overflow int32)")
    iso = float(np.float32(isovalue))
    work = torch.empty(wbytes, dtype=torch.uint8, device=v.device)
    counts = torch.empty(2, dtype=torch.int32, device=v.device)
    st = _lib.stream_ptr()
    _lib.check(lib.sf_mc_count(_lib.ptr(v), nx, ny, nz, iso, _lib.ptr(work), wbytes, _lib.ptr(counts), st), "mc_count")
    V, F = (int(c) for c in counts.cpu())
    verts = torch.empty(V, 3, dtype=torch.float32, device=v.device)
    faces = torch.empty(F, 3, dtype=torch.int32, device=v.device)
    _lib.check(lib.sf_mc_emit(_lib.ptr(v), nx, ny, nz, iso, _lib.ptr(work), wbytes, _lib.ptr(verts), _lib.ptr(faces), st), "mc_emit")
    if from_np:
        return verts.cpu().numpy(), faces.cpu().numpy()
    return verts, faces


def export_obj(vertices, faces, filename):
    """mcubes.export_obj: one `v x y z` line per vertex, one `f a b c` line per face (1-based).  Each coordinate is printed with 9
    significant digits, which parse back to the same float32.  The text is formatted in two C-level calls, not per line."""
    v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(f, dtype=np.int64).reshape(-1, 3) + 1
    with open(filename, "w") as fh:
        fh.write(("v %.9g %.9g %.9g\n" * v.shape[0]) % tuple(v.astype(np.float64).ravel().tolist()))
        fh.write(("f %d %d %d\n" * f.shape[0]) % tuple(f.ravel().tolist()))
