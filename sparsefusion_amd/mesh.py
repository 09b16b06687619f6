"""Mesh export on the GPU: the NGP density on a lattice, PyMCubes' Gaussian smoothing, fp64 volume statistics and marching cubes
(C ABI in include/sparsefusion_hip.h, kernels in csrc/mesh_kernels.h and csrc/mesh.hip), and per-vertex
colour and normal from the field (sf_ngp_point_attrs, csrc/ngp_point_attrs.h) with OBJ / PLY writers that carry them.

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


def point_attributes(net, x, epsilon, sigma=True, albedo=True, grad=True, normal=True):
    """One launch of sf_ngp_point_attrs on x [P, 3] (device tensor): dict of the requested outputs among sigma [P], albedo [P, 3],
    grad [P, 3] (central finite difference of sigma over +-epsilon per axis, offset points clamped to the box) and normal [P, 3]
    (grad normalised, NaN -> 0).  sigma / albedo are bit-identical to net.density(x); every offset sigma is bit-identical to
    net.density on the clamped fp32 offset point."""
    params = [p.detach().contiguous() for p in net._field_params()]
    _lib.require_cuda(x, *params)
    eps = float(np.float32(epsilon))
    if not (np.isfinite(eps) and eps > 0.0):
        raise ValueError(f"point_attributes: epsilon must be finite and > 0 (as float32), got {epsilon!r}")
    if not (sigma or albedo or grad or normal):
        raise ValueError("point_attributes: at least one output is required")
    xs = x.detach().reshape(-1, 3).float().contiguous()
    P = xs.shape[0]
    if P >= 1 << 32:
        raise ValueError("point_attributes: at most 2^32 - 1 points per call")
    f32 = dict(dtype=torch.float32, device=xs.device)
    out = {}
    if sigma:
        out["sigma"] = torch.empty(P, **f32)
    for name, want in (("albedo", albedo), ("grad", grad), ("normal", normal)):
        if want:
            out[name] = torch.empty(P, 3, **f32)
    if P == 0:
        return out
    f = net._field_handle().struct(params)
    rc = _lib.lib().sf_ngp_point_attrs(C.byref(f), _lib.ptr(xs), P, eps, _lib.ptr(out.get("sigma")), _lib.ptr(out.get("albedo")),
                                       _lib.ptr(out.get("grad")), _lib.ptr(out.get("normal")), _lib.stream_ptr())
    _lib.check(rc, "ngp_point_attrs")
    return out


@torch.no_grad()
def vertex_attributes(net, vertices_world, epsilon):
    """Per-vertex colour and normal of a mesh of the field -> (colors [V, 3] float32 = albedo at the vertex, normals [V, 3]
    float32), one launch.  The normals point OUTWARD: -net.normal(x), because the density falls toward the outside (and the faces of
    marching_cubes already look toward decreasing values); unit length, or exactly zero where the gradient vanishes or is not
    finite.  Device tensor in -> device tensors out; numpy in -> numpy out."""
    if isinstance(vertices_world, np.ndarray):
        dev = net._field_params()[0].device
        v, from_np = torch.from_numpy(np.ascontiguousarray(vertices_world, dtype=np.float32)).to(dev), True
    else:
        v, from_np = _as_device(vertices_world, "vertex_attributes")
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"vertex_attributes: expected vertices [V, 3], got shape {tuple(v.shape)}")
    if v.shape[0] == 0:
        colors, normals = torch.empty_like(v), torch.empty_like(v)
    else:
        out = point_attributes(net, v, epsilon, sigma=False, grad=False)
        colors, normals = out["albedo"], -out["normal"] + 0.0            # + 0.0: a zero normal is +0, not -0
    if from_np:
        return colors.cpu().numpy(), normals.cpu().numpy()
    return colors, normals


def _mesh_arrays(vertices, faces, colors, normals, what):
    """float32 [V, 3] vertices, int64 [F, 3] faces (0-based), float32 [V, 3] colours / normals or None -- numpy on the host"""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)      # noqa: E731
    v = np.ascontiguousarray(host(vertices), dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(host(faces), dtype=np.int64).reshape(-1, 3)
    extra = []
    for name, a in (("colors", colors), ("normals", normals)):
        if a is not None:
            a = np.ascontiguousarray(host(a), dtype=np.float32).reshape(-1, 3)
            if a.shape[0] != v.shape[0]:
                raise ValueError(f"{what}: {name} has {a.shape[0]} rows for {v.shape[0]} vertices")
        extra.append(a)
    return v, f, extra[0], extra[1]


def export_obj(vertices, faces, filename, colors=None, normals=None):
    """mcubes.export_obj: one `v x y z` line per vertex, one `f a b c` line per face (1-based).  Each coordinate is printed with 9
    significant digits, which parse back to the same float32.  The text is formatted in two C-level calls, not per line.

    colors [V, 3] (clipped to [0, 1]): the vertex lines become `v x y z r g b` (9 digits each, the per-vertex colour extension
    mesh viewers read).  normals [V, 3]: one `vn x y z` line per vertex after the vertices, and the faces become
    `f a//a b//b c//c`.  With neither, the file is byte-identical to the plain form.  One C-level format per block of lines."""
    v, f, c, n = _mesh_arrays(vertices, faces, colors, normals, "export_obj")
    f = f + 1
    with open(filename, "w") as fh:
        if c is None:
            fh.write(("v %.9g %.9g %.9g\n" * v.shape[0]) % tuple(v.astype(np.float64).ravel().tolist()))
        else:
            vc = np.concatenate([v, np.clip(c, 0.0, 1.0)], axis=1)
            fh.write(("v %.9g %.9g %.9g %.9g %.9g %.9g\n" * v.shape[0]) % tuple(vc.astype(np.float64).ravel().tolist()))
        if n is None:
            fh.write(("f %d %d %d\n" * f.shape[0]) % tuple(f.ravel().tolist()))
        else:
            fh.write(("vn %.9g %.9g %.9g\n" * n.shape[0]) % tuple(n.astype(np.float64).ravel().tolist()))
            fh.write(("f %d//%d %d//%d %d//%d\n" * f.shape[0]) % tuple(np.repeat(f, 2, axis=1).ravel().tolist()))


def ply_header(V, F, colors=False, normals=False):
    """The header export_ply writes (ASCII, ends with `end_header\\n`)."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {V}", "property float x", "property float y",
             "property float z"]
    if normals:
        lines += ["property float nx", "property float ny", "property float nz"]
    if colors:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    lines += [f"element face {F}", "property list uchar int vertex_indices", "end_header"]
    return "\n".join(lines) + "\n"


def ply_dtypes(colors=False, normals=False):
    """(vertex, face) packed little-endian record types of export_ply's two elements"""
    vt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        vt += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors:
        vt += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(vt), np.dtype([("count", "u1"), ("vertex_indices", "<i4", (3,))])


def export_ply(vertices, faces, filename, colors=None, normals=None):
    """Binary little-endian PLY: per vertex `float x y z`, then `float nx ny nz` with normals, then `uchar red green blue` with
    colours (round(clip(c, 0, 1) * 255), halves to even, NaN as 0); per face `list uchar int vertex_indices` (0-based).  Each
    element is written from one structured numpy array, not per row."""
    v, f, c, n = _mesh_arrays(vertices, faces, colors, normals, "export_ply")
    vt, ft = ply_dtypes(c is not None, n is not None)
    rec = np.zeros(v.shape[0], dtype=vt)
    for k, name in enumerate(("x", "y", "z")):
        rec[name] = v[:, k]
    if n is not None:
        for k, name in enumerate(("nx", "ny", "nz")):
            rec[name] = n[:, k]
    if c is not None:
        c8 = np.rint(np.clip(np.nan_to_num(c.astype(np.float64), nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
        for k, name in enumerate(("red", "green", "blue")):
            rec[name] = c8[:, k]
    frec = np.zeros(f.shape[0], dtype=ft)
    frec["count"] = 3
    frec["vertex_indices"] = f.astype(np.int32)
    with open(filename, "wb") as fh:
        fh.write(ply_header(v.shape[0], f.shape[0], c is not None, n is not None).encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())
