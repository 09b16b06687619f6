"""CPU tests of the mesh-export layer (sparsefusion_amd/mesh.py, nerf/utils.py, NeRFRenderer.export_mesh) that need no GPU: the
OBJ writer round trip, the C ABI's shape limits, the no-CPU-path rule, and the CPU restatement's own properties (tests/mesh_ref.py)."""
import os

import numpy as np
import pytest
import torch

import mesh_ref


def test_export_obj_round_trip_exact(tmp_path):
    from sparsefusion_amd.mesh import export_obj
    rng = np.random.default_rng(0)
    v = (rng.standard_normal((5000, 3)) * np.array([1e-3, 10.0, 3e4])).astype(np.float32)
    v[0] = [0.0, 1.0, 127.0]
    v[1] = np.nextafter(np.float32(1.0), np.float32(2.0))
    v[2] = [np.float32(1e-30), np.float32(-3.4e38), np.float32(1 / 3)]
    f = rng.integers(0, 5000, (7000, 3)).astype(np.int32)
    path = os.path.join(tmp_path, "m.obj")
    export_obj(v, f, path)
    pv, pf = mesh_ref.parse_obj(path)
    assert np.array_equal(pv.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(pf, f)
    text = open(path).read().splitlines()
    assert text[0].startswith("v ") and text[5000].startswith("f ") and len(text) == 12000
    assert min(int(x) for x in text[5000].split()[1:]) >= 1
    export_obj(torch.from_numpy(v), torch.from_numpy(f), path + "2")           # CPU tensors: only the file is written
    assert open(path + "2").read() == open(path).read()


def test_export_obj_empty(tmp_path):
    from sparsefusion_amd.mesh import export_obj
    path = os.path.join(tmp_path, "e.obj")
    export_obj(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), path)
    assert open(path).read() == ""


def test_mesh_functions_refuse_cpu_tensors():
    from sparsefusion_amd import mesh
    with pytest.raises(RuntimeError):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    with pytest.raises(RuntimeError):
        mesh.smooth_gaussian(torch.zeros(4, 4, 4))


def test_abi_shape_limits():
    """Workspace queries return 0 for the shapes the entry points reject: an empty axis, 3 N >= 2^31 vertex ids, 5 cells >= 2^31
    face ids, a lattice of 2^31 points."""
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    assert lib.sf_mc_workspace_bytes(0, 4, 4) == 0 and lib.sf_gaussian3d_workspace_bytes(4, 0, 4) == 0
    assert lib.sf_mc_workspace_bytes(1024, 1024, 1024) == 0                   # 3 N >= 2^31
    assert lib.sf_mc_workspace_bytes(812, 812, 812) == 0                      # 5 cells >= 2^31
    assert lib.sf_gaussian3d_workspace_bytes(2048, 1024, 1024) == 0           # N = 2^31
    assert lib.sf_gaussian3d_workspace_bytes(1024, 1024, 1024) > 4 * 1024 ** 3
    assert lib.sf_mc_workspace_bytes(256, 256, 256) >= 6 * 256 ** 3
    assert lib.sf_mc_workspace_bytes(1, 1, 1) > 0                             # no cells: vertices only


def test_reference_pipeline_properties():
    """The CPU pipeline the GPU one is tested against: gaussian_filter(vol - 0.5) = gaussian_filter(vol) - 0.5 up to rounding (why
    smooth_gaussian may omit the constant), and the reference's level mean + 0.25 std."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(2)
    vol = rng.random((12, 9, 15)).astype(np.float32) * 40
    a = mesh_ref.smooth_gaussian(vol, 1.5)
    b = gaussian_filter(vol.astype(np.float64), 1.5) - 0.5
    assert float(np.abs(a - b).max()) < 1e-12
    assert abs((mesh_ref.iso_level(a) + 0.5) - mesh_ref.iso_level(b + 0.5)) < 1e-12
    assert mesh_ref.iso_level(a) == a.mean() + a.std() * 0.25


def test_reference_marching_cubes_plane_and_sphere():
    R = 64
    x = np.arange(R, dtype=np.float64)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    plane = (Z - 20.6).astype(np.float32)
    v, f = mesh_ref.marching_cubes(plane, 0.0)
    area = 0.5 * np.linalg.norm(mesh_ref.face_normals(v, f), axis=1).sum()
    assert abs(area - (R - 1) ** 2) < 1e-6 * (R - 1) ** 2                   # flat sheet spanning the lattice
    assert v.shape[0] == R * R and f.shape[0] == 2 * (R - 1) ** 2
    r = 25.0
    ball = (r - np.sqrt((X - 31.5) ** 2 + (Y - 31.5) ** 2 + (Z - 31.5) ** 2)).astype(np.float32)
    v, f = mesh_ref.marching_cubes(ball, 0.0)
    edges, cnt = mesh_ref.edges_of(f)
    assert (cnt == 2).all() and v.shape[0] - edges.shape[0] + f.shape[0] == 2
    assert abs(mesh_ref.signed_volume(v, f) / (4 / 3 * np.pi * r ** 3) - 1) < 0.02


def test_export_mesh_and_extract_geometry_exist():
    """The public surface: NeRFRenderer.export_mesh(path, resolution=None, S=128), nerf.utils.extract_fields / extract_geometry."""
    import inspect
    from sparsefusion_amd.nerf import NeRFRenderer
    from sparsefusion_amd.nerf import utils
    sig = inspect.signature(NeRFRenderer.export_mesh)
    assert list(sig.parameters) == ["self", "path", "resolution", "S"]
    assert sig.parameters["resolution"].default is None and sig.parameters["S"].default == 128
    assert list(inspect.signature(utils.extract_fields).parameters) == ["bound_min", "bound_max", "resolution", "query_func", "S"]
    assert list(inspect.signature(utils.extract_geometry).parameters) == ["bound_min", "bound_max", "resolution", "threshold",
                                                                          "query_func"]


def test_extract_fields_reference_order_on_cpu_query():
    """extract_fields calls query_func on S^3 blocks in the reference's order and assembles them x-major (a CPU query function
    is fine: only the marching cubes need the GPU)."""
    from sparsefusion_amd.nerf.utils import extract_fields
    calls = []

    def q(p):
        calls.append(p.shape[0])
        return p[:, 0] * 100 + p[:, 1] * 10 + p[:, 2]

    lo, hi = torch.tensor([-1.0, -2.0, 0.0]), torch.tensor([1.0, 2.0, 3.0])
    u = extract_fields(lo, hi, 10, q, S=4)
    assert calls == [4 * 4 * 4, 4 * 4 * 4, 4 * 4 * 2] * 1 + [4 * 4 * 4, 4 * 4 * 4, 4 * 4 * 2] + [4 * 2 * 4, 4 * 2 * 4, 4 * 2 * 2] + \
        [4 * 4 * 4, 4 * 4 * 4, 4 * 4 * 2] * 2 + [4 * 2 * 4, 4 * 2 * 4, 4 * 2 * 2] + \
        [2 * 4 * 4, 2 * 4 * 4, 2 * 4 * 2] * 2 + [2 * 2 * 4, 2 * 2 * 4, 2 * 2 * 2]
    ax = [torch.linspace(float(lo[d]), float(hi[d]), 10) for d in range(3)]
    want = ax[0][:, None, None] * 100 + ax[1][None, :, None] * 10 + ax[2][None, None, :]
    assert u.dtype == np.float32 and np.array_equal(u, want.numpy())
