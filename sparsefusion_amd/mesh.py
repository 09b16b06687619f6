"""Mesh export on the GPU: the NGP density on a lattice, PyMCubes' Gaussian smoothing, fp64 volume statistics and marching cubes
(C ABI in include/sparsefusion_hip.h, kernels in csrc/mesh_kernels.h and csrc/mesh.hip), and per-vertex
colour and normal from the field (sf_ngp_point_attrs, csrc/ngp_point_attrs.h) with OBJ / PLY writers that carry them, and a
texture atlas baked from the field (sf_ngp_texture_bake, csrc/ngp_texture.h) with its OBJ / MTL / PNG writers, and mesh clean-up:
connected components and floater removal (sf_mesh_components / sf_mesh_filter_*, csrc/mesh_clean.h).

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


# ------------------------------------------------------------------------------------------------------------------ texture atlas
# One right-angled chart per triangle, two charts per square cell: the layout of csrc/ngp_texture.h, restated.
ATLAS_MIN_CELL = 6

MTL_TEXT = ("newmtl mat0 \n"
            "Ka 1.000000 1.000000 1.000000 \n"
            "Kd 1.000000 1.000000 1.000000 \n"
            "Ks 0.000000 0.000000 0.000000 \n"
            "Tr 1.000000 \n"
            "illum 1 \n"
            "Ns 0.000000 \n"
            "map_Kd albedo.png \n")           # what renderer_df.py:298-306 writes (name = ''), trailing blanks included


def atlas_layout(F, W):
    """(G, c) of F faces in a W x W texture: faces are paired into G x G square cells of edge c = W // G texels,
    G = ceil(sqrt(ceil(F / 2))); face f is half f & 1 of cell f >> 1 at (row, col) = divmod(f >> 1, G).  F == 0 -> (0, 0).
    ValueError if c < 6 (a chart needs a leg of at least one texel, a margin and a gutter), naming the smallest W that works."""
    F, W = int(F), int(W)
    if F < 0 or W < 1:
        raise ValueError(f"atlas_layout: need F >= 0 and W >= 1, got F={F}, W={W}")
    if W * W >= 1 << 31:
        raise ValueError(f"atlas_layout: need W * W < 2^31, got W={W}")
    if F == 0:
        return 0, 0
    cells = (F + 1) // 2
    G = 1
    while G * G < cells:
        G += 1
    c = W // G
    if c < ATLAS_MIN_CELL:
        raise ValueError(f"atlas_layout: {F} faces in a {W} x {W} texture leave cells of {c} texels, below {ATLAS_MIN_CELL}: "
                         f"the smallest W is {ATLAS_MIN_CELL * G}")
    return G, c


def atlas_uv(F, W):
    """uv [F, 3, 2] float32, (u, v_atlas) of face corner 0 / 1 / 2: texel centres, (x + 0.5) / W with the division in float32.
    In cell-local texel indices and with leg l = c - 5 the lower half's corners are (1, 1), (1 + l, 1), (1, 1 + l) and the upper
    half's (c - 2, c - 2), (c - 2 - l, c - 2), (c - 2, c - 2 - l): the same winding.  Image row y holds v_atlas = (y + 0.5) / W, so a
    `vt` line carries 1 - v_atlas."""
    G, c = atlas_layout(F, W)
    f = np.arange(int(F), dtype=np.int64)
    if f.size == 0:
        return np.zeros((0, 3, 2), dtype=np.float32)
    q, half = f >> 1, f & 1
    row, col = q // G, q % G
    leg = c - 5
    ij = np.array([[1, 1], [1 + leg, 1], [1, 1 + leg]], dtype=np.int64)[None]                   # [1, 3, 2] (i, j), lower half
    ij = np.where(half[:, None, None] == 1, c - 1 - ij, ij)
    xy = ij + np.stack([col, row], -1)[:, None, :] * c
    return ((xy.astype(np.float32) + np.float32(0.5)) / np.float32(W)).astype(np.float32)


@torch.no_grad()
def bake_texture(net, vertices_world, faces, W, rgb8=True, albedo=False, xyz=False, face_id=False):
    """One launch of sf_ngp_texture_bake: the field's albedo at every texel of the atlas of atlas_layout(F, W).  vertices_world
    [V, 3] float32 and faces [F, 3] int32 are device tensors.  Returns a dict of the requested outputs among rgb8 [W, W, 3] uint8
    (truncation of clip(albedo, 0, 1) * 255, NaN -> 0), albedo [W, W, 3] float32 (bit-identical to net.density on the texel's
    point), xyz [W, W, 3] float32 (that point) and face_id [W, W] int32; row y, column x is the texel with its centre at
    (u, v_atlas) = ((x + 0.5) / W, (y + 0.5) / W).  A texel of no face, or of a face with a vertex index outside [0, V), holds
    0 / 0 / 0 / -1.  Every texel is a direct sample of the field: no supersampling, nothing to inpaint."""
    params = [p.detach().contiguous() for p in net._field_params()]
    _lib.require_cuda(vertices_world, faces, *params)
    if not (rgb8 or albedo or xyz or face_id):
        raise ValueError("bake_texture: at least one output is required")
    v = vertices_world.detach().reshape(-1, 3).float().contiguous()
    fc = faces.detach().reshape(-1, 3).to(torch.int32).contiguous()
    V, F, W = v.shape[0], fc.shape[0], int(W)
    atlas_layout(F, W)
    dev = v.device
    out = {}
    if rgb8:
        out["rgb8"] = torch.empty(W, W, 3, dtype=torch.uint8, device=dev)
    for name, want in (("albedo", albedo), ("xyz", xyz)):
        if want:
            out[name] = torch.empty(W, W, 3, dtype=torch.float32, device=dev)
    if face_id:
        out["face_id"] = torch.empty(W, W, dtype=torch.int32, device=dev)
    keep_v, keep_f = torch.zeros(1, 3, device=dev), torch.zeros(1, 3, dtype=torch.int32, device=dev)      # valid pointers for an empty mesh
    f = net._field_handle().struct(params)
    rc = _lib.lib().sf_ngp_texture_bake(C.byref(f), _lib.ptr(v if V else keep_v), V, _lib.ptr(fc if F else keep_f), F, W,
                                        _lib.ptr(out.get("rgb8")), _lib.ptr(out.get("albedo")), _lib.ptr(out.get("xyz")),
                                        _lib.ptr(out.get("face_id")), _lib.stream_ptr())
    _lib.check(rc, "ngp_texture_bake")
    return out


def write_png(path, rgb8):
    """8-bit RGB PNG of rgb8 [H, W, 3] uint8 (numpy or tensor), row 0 at the top: signature, IHDR, one IDAT (filter 0 on every
    row, zlib), IEND -- the standard library only."""
    import struct
    import zlib
    a = rgb8.detach().cpu().numpy() if isinstance(rgb8, torch.Tensor) else np.asarray(rgb8)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: expected uint8 [H, W, 3], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)                   # byte 0 of a row: filter type 0 (none)
    rows[:, 1:] = a.reshape(h, 3 * w)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                 chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def export_obj_textured(vertices, faces, uvs, filename, mtl_name, normals=None):
    """Textured OBJ: `mtllib <mtl_name>`, one `v x y z` per vertex, `vt u (1 - v_atlas)` for uvs [F, 3, 2] (3 F lines, corner k of
    face f is line 3 f + k), optional `vn x y z` per vertex, `usemtl mat0`, then `f a/ta b/tb c/tc` (`a/ta/a ..` with normals),
    1-based.  Coordinates and uvs are printed with 9 significant digits, which parse back to the same float32; 1 - v_atlas is taken
    in float32.  One C-level format per block of lines, as export_obj."""
    v, f, _, n = _mesh_arrays(vertices, faces, None, normals, "export_obj_textured")
    uv = uvs.detach().cpu().numpy() if isinstance(uvs, torch.Tensor) else np.asarray(uvs)
    uv = np.ascontiguousarray(uv, dtype=np.float32)
    if uv.shape != (f.shape[0], 3, 2):
        raise ValueError(f"export_obj_textured: uvs have shape {uv.shape} for {f.shape[0]} faces, expected [F, 3, 2]")
    vt = np.stack([uv[..., 0], np.float32(1.0) - uv[..., 1]], -1).astype(np.float32).reshape(-1, 2)
    f = f + 1
    ti = np.arange(1, 3 * f.shape[0] + 1, dtype=np.int64).reshape(-1, 3)
    with open(filename, "w") as fh:
        fh.write(f"mtllib {mtl_name}\n")
        fh.write(("v %.9g %.9g %.9g\n" * v.shape[0]) % tuple(v.astype(np.float64).ravel().tolist()))
        fh.write(("vt %.9g %.9g\n" * vt.shape[0]) % tuple(vt.astype(np.float64).ravel().tolist()))
        if n is not None:
            fh.write(("vn %.9g %.9g %.9g\n" * n.shape[0]) % tuple(n.astype(np.float64).ravel().tolist()))
        fh.write("usemtl mat0\n")
        if n is None:
            fh.write(("f %d/%d %d/%d %d/%d\n" * f.shape[0]) % tuple(np.stack([f, ti], -1).ravel().tolist()))
        else:
            fh.write(("f %d/%d/%d %d/%d/%d %d/%d/%d\n" * f.shape[0]) % tuple(np.stack([f, ti, f], -1).ravel().tolist()))


# -------------------------------------------------------------------------------------------------------------------- clean-up
# Connected components and floater removal (sf_mesh_components / sf_mesh_filter_*, csrc/mesh_clean.h).
def _faces_device(faces, what, device=None):
    """(int32 contiguous [F, 3] device tensor, came_from_numpy).  int64 indices outside int32 are clamped to -1 / 2^31 - 1 first,
    which no vertex count reaches: they stay invalid."""
    from_np = isinstance(faces, np.ndarray)
    if not from_np and not isinstance(faces, torch.Tensor):
        raise TypeError(f"{what}: faces: expected a torch tensor or a numpy array, got {type(faces).__name__}")
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: expected faces [F, 3], got shape {tuple(faces.shape)}")
    if from_np:
        if faces.dtype not in (np.int32, np.int64):
            raise TypeError(f"{what}: faces must be int32 or int64, got {faces.dtype}")
        if not torch.cuda.is_available():
            raise RuntimeError(f"{what}: numpy input runs on the current HIP device and there is none (no CPU path)")
        f = torch.tensor(faces).to(device or f"cuda:{torch.cuda.current_device()}")      # a copy: the array may be read-only
    else:
        if faces.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{what}: faces must be int32 or int64, got {faces.dtype}")
        _lib.require_cuda(faces)
        f = faces.detach()
    if f.dtype == torch.int64:
        f = f.clamp(-1, (1 << 31) - 1).to(torch.int32)
    return f.contiguous(), from_np


def _num_vertices(V, what):
    if isinstance(V, bool) or not isinstance(V, (int, np.integer)):
        raise TypeError(f"{what}: num_vertices must be an int, got {type(V).__name__}")
    if not 0 <= int(V) < 1 << 31:
        raise ValueError(f"{what}: need 0 <= num_vertices < 2^31, got {V}")
    return int(V)


def _components(f, V):
    """sf_mesh_components on f [F, 3] int32 (device, contiguous) -> vertex_label, face_label, faces_per_label, counts3 (device)"""
    F, dev = f.shape[0], f.device
    if F >= 1 << 31:
        raise ValueError(f"connected_components: need F < 2^31, got {F}")
    lib = _lib.lib()
    i32 = dict(dtype=torch.int32, device=dev)
    vertex_label, face_label, per = torch.empty(V, **i32), torch.empty(F, **i32), torch.empty(V, **i32)
    counts3 = torch.empty(3, **i32)
    wbytes = lib.sf_mesh_components_workspace_bytes(V, F)
    work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    pz = lambda t: _lib.ptr(t if t.numel() else None)      # noqa: E731
    rc = lib.sf_mesh_components(pz(f), F, V, pz(vertex_label), pz(face_label), pz(per), _lib.ptr(counts3), pz(work), wbytes,
                                _lib.stream_ptr())
    _lib.check(rc, "mesh_components")
    return vertex_label, face_label, per, counts3


def connected_components(faces, num_vertices):
    """Connected components of an indexed triangle mesh on the GPU: faces [F, 3] int32 (or int64) and the vertex count ->
    dict of vertex_label [V] int32, face_label [F] int32, faces_per_label [V] int32 (device tensors; numpy for numpy input) and the
    ints n_components, largest (face count of the largest component) and n_invalid (one read of three words).

    Two vertices are connected when a face names both.  Connectivity is by INDEX only: coincident but unwelded vertices are not
    merged (marching_cubes welds; a mesh read from a triangle soup does not).  The label of a component is the smallest vertex
    index in it, so the result is a function of the mesh alone (lock-free union-find, csrc/mesh_clean.h).  A face with an index
    outside [0, num_vertices), negative ones included, is invalid: it connects nothing, has face_label -1, belongs to no component
    and is counted in n_invalid.  A degenerate face with a repeated index is valid and connects what it names.  An unreferenced
    vertex is its own label with zero faces; faces_per_label is zero wherever v is not a label.  n_components counts the labels
    with at least one face."""
    V = _num_vertices(num_vertices, "connected_components")
    f, from_np = _faces_device(faces, "connected_components")
    vertex_label, face_label, per, counts3 = _components(f, V)
    n_components, largest, n_invalid = (int(c) for c in counts3.cpu())
    out = dict(vertex_label=vertex_label, face_label=face_label, faces_per_label=per)
    if from_np:
        out = {k: t.cpu().numpy() for k, t in out.items()}
    out.update(n_components=n_components, largest=largest, n_invalid=n_invalid)
    return out


def clean_mesh(vertices, faces, min_faces=8, min_fraction=0.0):
    """Floater removal on the GPU: drops every connected component (connected_components: by index, no welding) of fewer than
    min_faces faces or fewer than ceil(min_fraction * largest) faces (product in double; min_fraction = 1 keeps only the components
    tied for largest), every face that is invalid or belongs to a dropped component, and every vertex no kept face names
    (unreferenced vertices go too).  Returns (vertices' [V', 3] float32 -- bit copies of the kept rows --, faces' [F', 3] int32 with
    the indices remapped, vertex_ids [V'] int32, face_ids [F'] int32: the old index of every kept row).  Order is preserved:
    vertex_ids and face_ids are strictly increasing.  Device tensors in -> device tensors out; numpy in -> numpy out.  One
    device-to-host read of {V', F'} sizes the outputs.

    min_faces = 8 is the default of the `clean_mesh` step the torch-ngp / stable-dreamfusion lineage runs after marching cubes -- a
    choice of this library, not reference behaviour (the reference exports the raw mesh).  That step's other rule, pymeshlab's
    diameter threshold, is not reproduced; neither are welding, smoothing, remeshing or decimation."""
    if isinstance(min_faces, bool) or not isinstance(min_faces, (int, np.integer)):
        raise TypeError(f"clean_mesh: min_faces must be an int, got {type(min_faces).__name__}")
    if not 0 <= int(min_faces) < 1 << 32:
        raise ValueError(f"clean_mesh: need 0 <= min_faces < 2^32, got {min_faces}")
    frac = float(min_fraction)
    if not (np.isfinite(frac) and 0.0 <= frac <= 1.0):
        raise ValueError(f"clean_mesh: min_fraction must be finite and in [0, 1], got {min_fraction!r}")
    from_np = isinstance(vertices, np.ndarray)
    if not from_np and not isinstance(vertices, torch.Tensor):
        raise TypeError(f"clean_mesh: vertices: expected a torch tensor or a numpy array, got {type(vertices).__name__}")
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError(f"clean_mesh: expected vertices [V, 3], got shape {tuple(vertices.shape)}")
    if vertices.dtype != (np.float32 if from_np else torch.float32):
        raise TypeError(f"clean_mesh: vertices must be float32 (the kept rows are bit copies), got {vertices.dtype}")
    if isinstance(faces, np.ndarray) != from_np:
        raise TypeError("clean_mesh: vertices and faces must both be torch tensors or both numpy arrays")
    if from_np:
        f, _ = _faces_device(faces, "clean_mesh")
        v = torch.tensor(vertices).to(f.device)
    else:
        _lib.require_cuda(vertices)
        f, _ = _faces_device(faces, "clean_mesh")
        v = vertices.detach().contiguous()
        if f.device != v.device:
            raise ValueError(f"clean_mesh: vertices are on {v.device}, faces on {f.device}")
    V, F, dev = _num_vertices(v.shape[0], "clean_mesh"), f.shape[0], v.device
    vertex_label, _, per, counts3 = _components(f, V)
    lib = _lib.lib()
    wbytes = lib.sf_mesh_filter_workspace_bytes(V, F)
    work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    counts2 = torch.empty(2, dtype=torch.int32, device=dev)
    pz = lambda t: _lib.ptr(t if t.numel() else None)      # noqa: E731
    st = _lib.stream_ptr()
    _lib.check(lib.sf_mesh_filter_count(pz(f), F, V, pz(vertex_label), pz(per), _lib.ptr(counts3), int(min_faces), frac, _lib.ptr(work),
                                        wbytes, _lib.ptr(counts2), st), "mesh_filter_count")
    V2, F2 = (int(c) for c in counts2.cpu())
    out_v = torch.empty(V2, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(F2, 3, dtype=torch.int32, device=dev)
    vertex_ids, face_ids = torch.empty(V2, dtype=torch.int32, device=dev), torch.empty(F2, dtype=torch.int32, device=dev)
    _lib.check(lib.sf_mesh_filter_emit(pz(v), pz(f), F, V, _lib.ptr(work), wbytes, pz(out_v), pz(out_f), pz(vertex_ids), pz(face_ids), st),
               "mesh_filter_emit")
    out = (out_v, out_f, vertex_ids, face_ids)
    return tuple(t.cpu().numpy() for t in out) if from_np else out
