"""Kernel-logic tests of the mesh-export kernels (sparsefusion_amd/csrc/mesh_kernels.h) on CPU fibers against the CPU restatement
(tests/mesh_ref.py) and scipy: the marching-cubes tables, all 256 cube configurations, sphere / torus / non-cubic noise volumes,
the separable Gaussian (scipy 'reflect', dims shorter than the radius) and the fixed-order volume statistics."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_ref
from hostemu import fused

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
SO = os.path.join(HERE, "_build", "libmesh_emu.so")
pytestmark = pytest.mark.skipif(not fused.available(), reason="host clang not found")
_handle = None


def _lib():
    global _handle
    if _handle is None:
        csrc = os.path.join(HERE, "..", "..", "sparsefusion_amd", "csrc")
        srcs = [os.path.join(HERE, "mesh_emu.cpp"), os.path.join(HERE, "hip_emu.h")] + \
               [os.path.join(csrc, f) for f in ("mesh_kernels.h", "sf_dev.h")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call([fused.CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + HERE, "-Wall", "-Wno-unused-function",
                                   "-ffp-contract=off", srcs[0], "-o", SO, "-lpthread"])
        _handle = C.CDLL(SO)
        _handle.emu_gaussian3d.restype = C.c_int
        _handle.emu_gaussian3d.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_void_p]
        _handle.emu_mc.restype = None
        _handle.emu_mc.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    return _handle


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def emu_mc(vol, iso):
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    counts = np.zeros(2, dtype=np.uint32)
    lib = _lib()
    lib.emu_mc(_p(vol), *vol.shape, float(np.float32(iso)), _p(counts), None, None)
    V, F = int(counts[0]), int(counts[1])
    verts = np.full((max(V, 1), 3), np.nan, dtype=np.float32)
    faces = np.full((max(F, 1), 3), -1, dtype=np.int32)
    lib.emu_mc(_p(vol), *vol.shape, float(np.float32(iso)), _p(counts), _p(verts), _p(faces))
    return verts[:V], faces[:F]


def emu_gaussian(vol, sigma=1.5, truncate=4.0):
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    out = np.full_like(vol, np.nan)
    stats = np.zeros(2, dtype=np.float64)
    assert _lib().emu_gaussian3d(_p(vol), _p(out), *vol.shape, sigma, truncate, _p(stats)) == 0
    return out, stats


def test_tables_self_consistent():
    """The kernel's triangle table is mesh_ref's; each row uses exactly the edges whose corners classify differently (= the edge
    table); the edge owners are the lower corners of the classic edges."""
    tri = np.zeros((256, 16), dtype=np.int8)
    owner = np.zeros((12, 4), dtype=np.int8)
    _lib().emu_mc_tables(_p(tri), _p(owner))
    et = mesh_ref.edge_table()
    for c in range(256):
        row = [int(e) for e in tri[c] if e >= 0]
        assert tuple(row) == mesh_ref.TRI_TABLE[c], c
        assert all(e < 0 for e in tri[c][len(row):]) and len(row) % 3 == 0 and len(row) <= 15
        used = sum(1 << e for e in set(row))
        assert used == et[c], (c, used, et[c])                      # every crossing edge used, no other
        assert et[c] == et[255 - c]
    for e, ((dx, dy, dz), ax) in enumerate(mesh_ref.EDGE_OWNER):
        assert tuple(owner[e]) == (dx, dy, dz, ax), e


def test_all_256_configurations():
    """Every cube configuration as one 2x2x2 volume (corner c at the classic position, inside = below iso): identical faces and
    bit-identical vertices."""
    for c in range(256):
        vol = np.zeros((2, 2, 2), dtype=np.float32)
        for k, (dx, dy, dz) in enumerate(mesh_ref.CORNERS):
            vol[dx, dy, dz] = -1.0 - 0.37 * k if (c >> k) & 1 else 1.0 + 0.21 * k
        rv, rf = mesh_ref.marching_cubes(vol, 0.0)
        ev, ef = emu_mc(vol, 0.0)
        assert rf.shape[0] == len(mesh_ref.TRI_TABLE[c]) // 3
        assert np.array_equal(ef, rf), c
        assert np.array_equal(ev.view(np.uint32), rv.view(np.uint32)), c


@pytest.mark.parametrize("name", ["sphere", "torus", "noise"])
def test_volumes_match_reference(name):
    rng = np.random.default_rng(7)
    if name == "sphere":
        vol, iso = mesh_ref.sphere(24, 8.3), 0.0
    elif name == "torus":
        vol, iso = mesh_ref.torus(28, 7.5, 3.2), 0.0
    else:
        vol, iso = rng.standard_normal((23, 17, 29)).astype(np.float32), 0.1
    rv, rf = mesh_ref.marching_cubes(vol, iso)
    ev, ef = emu_mc(vol, iso)
    assert rf.shape[0] > 100
    assert np.array_equal(ef, rf)
    assert ev.shape == rv.shape and float(np.abs(ev - rv).max()) <= 2e-6


def test_sphere_mesh_properties():
    """R = 64 sphere (reference and emulated kernel agree): watertight (every edge in two faces, Euler characteristic 2), positive
    volume within 2 % of 4/3 pi r^3, every face normal against the analytic gradient (faces look toward decreasing values)."""
    R, r = 64, 22.0
    vol = mesh_ref.sphere(R, r)
    v, f = mesh_ref.marching_cubes(vol, 0.0)
    ev, ef = emu_mc(vol, 0.0)
    assert np.array_equal(ef, f) and float(np.abs(ev - v).max()) <= 2e-6
    edges, cnt = mesh_ref.edges_of(f)
    assert (cnt == 2).all()
    assert v.shape[0] - edges.shape[0] + f.shape[0] == 2
    vol_mesh = mesh_ref.signed_volume(v, f)
    exact = 4.0 / 3.0 * np.pi * r ** 3
    assert vol_mesh > 0 and abs(vol_mesh - exact) / exact < 0.02, (vol_mesh, exact)
    n = mesh_ref.face_normals(v, f)
    centre = v[f].astype(np.float64).mean(axis=1) - (R - 1) / 2
    grad = -centre                                                  # gradient of r - |x - c|
    assert (np.einsum("ij,ij->i", n, grad) < 0).all()


def test_random_closed_volumes_watertight_and_oriented():
    """Noise with an outside border: every edge in exactly two faces, each directed edge once (consistent orientation across
    neighbouring cells, the ambiguous faces included)."""
    rng = np.random.default_rng(3)
    for t in range(4):
        vol = np.pad(rng.standard_normal((11, 9, 13)).astype(np.float32), 1, constant_values=10.0)
        v, f = emu_mc(vol, 0.3 * t)
        _, cnt = mesh_ref.edges_of(f)
        assert (cnt == 2).all()
        d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        assert np.unique(d, axis=0).shape[0] == d.shape[0]


def test_plane_is_flat_sheet():
    R = 20
    X, _, _ = mesh_ref._grid(R)
    vol = (X - 7.3).astype(np.float32)
    v, f = emu_mc(vol, 0.0)
    rv, rf = mesh_ref.marching_cubes(vol, 0.0)
    assert np.array_equal(f, rf) and np.array_equal(v, rv)
    area = 0.5 * np.linalg.norm(mesh_ref.face_normals(v, f), axis=1).sum()
    assert abs(area - (R - 1) ** 2) < 1e-6 * (R - 1) ** 2
    assert np.allclose(v[:, 0], np.float32(7.3), atol=1e-5)
    assert (mesh_ref.face_normals(v, f)[:, 0] < 0).all()           # toward decreasing x


def test_empty_and_degenerate():
    v, f = emu_mc(np.ones((5, 4, 3), np.float32), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    vol = np.array([[[0.0, 1.0, 2.0]]], dtype=np.float32)          # 1 x 1 x 3: vertices, no cells
    v, f = emu_mc(vol, 0.5)
    rv, rf = mesh_ref.marching_cubes(vol, 0.5)
    assert np.array_equal(v, rv) and f.shape == (0, 3) and v.shape == (1, 3)


@pytest.mark.parametrize("shape", [(1, 1, 1), (4, 4, 4), (13, 13, 13), (37, 13, 4), (1, 37, 13), (4, 1, 37), (300, 2, 3), (3, 2, 300)])
def test_gaussian_matches_scipy(shape):
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(sum(shape))
    vol = (rng.standard_normal(shape) * 3 + 1).astype(np.float32)
    out, stats = emu_gaussian(vol)
    ref = gaussian_filter(vol.astype(np.float64), 1.5)               # mode 'reflect', truncate 4.0
    assert float(np.abs(out - ref).max()) <= 2e-6 * float(np.abs(vol).max())
    o = out.astype(np.float64)
    assert abs(stats[0] - o.mean()) <= 1e-12 * max(1.0, abs(o.mean()))
    assert abs(stats[1] - o.std()) <= 1e-9 * max(1.0, o.std())


def test_gaussian_other_sigma_and_bad_radius():
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(1)
    vol = rng.standard_normal((9, 21, 6)).astype(np.float32)
    out, _ = emu_gaussian(vol, sigma=2.7, truncate=3.0)
    ref = gaussian_filter(vol.astype(np.float64), 2.7, truncate=3.0)
    assert float(np.abs(out - ref).max()) <= 2e-6 * float(np.abs(vol).max())
    assert _lib().emu_gaussian3d(_p(vol), _p(np.empty_like(vol)), *vol.shape, 20.0, 4.0, None) == 1      # radius 80 > 64
