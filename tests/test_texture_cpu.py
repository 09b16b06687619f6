"""CPU tests of the texture atlas (sparsefusion_amd.mesh: atlas_layout, atlas_uv, write_png, export_obj_textured, MTL_TEXT) and of the
C ABI's argument checks (sf_ngp_texture_bake).  The layout properties are checked exhaustively in exact arithmetic:
  (P1) a bilinear lookup at any uv inside or on a face's chart triangle gives non-zero weight only to texels owned by that face;
  (P2) chart corners are texel centres;
  (P3) every texel of a used cell has an owner.
No GPU."""
import ctypes as C
import inspect
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import texture_common as tc


def _texel_of_uv(uv, W):
    """(P2) uv [..., 2] float32 are texel centres: -> integer texels, with (x + 0.5) / W in float32 giving uv back bit for bit"""
    t = uv.astype(np.float64) * W - 0.5
    xy = np.rint(t).astype(np.int64)
    assert np.abs(t - xy).max() < 1e-3
    assert np.array_equal(((xy.astype(np.float32) + np.float32(0.5)) / np.float32(W)).view(np.uint32), uv.view(np.uint32))
    return xy


def _owner_face(F, W, x, y):
    """owner of texel (x, y) by the restated rule, -1 outside the used cells"""
    G, c = tc.layout(F, W)
    col, row = x // c, y // c
    if col >= G or row >= G:
        return -1
    f = 2 * (row * G + col) + int(tc.owner_half(c, x - col * c, y - row * c))
    return f if f < F else -1


def _check_bilinear(F, W, f, corners, step=64):
    """(P1) for face f with integer corner texels `corners` [3, 2]: every barycentric grid point (step 1 / `step`, edges and corners
    included), in exact rational arithmetic: the taps of a bilinear lookup with non-zero weight are owned by f"""
    a, b, c = (tuple(int(v) for v in corners[k]) for k in range(3))
    for iu in range(step + 1):
        for iv in range(step + 1 - iu):
            u, v = Fraction(iu, step), Fraction(iv, step)
            w0 = 1 - u - v
            x = w0 * a[0] + u * b[0] + v * c[0]           # in texel units: centre of texel k is k
            y = w0 * a[1] + u * b[1] + v * c[1]
            x0, y0 = x.numerator // x.denominator, y.numerator // y.denominator
            fx, fy = x - x0, y - y0
            for dx, wx in ((0, 1 - fx), (1, fx)):
                for dy, wy in ((0, 1 - fy), (1, fy)):
                    if wx * wy != 0:
                        assert 0 <= x0 + dx < W and 0 <= y0 + dy < W
                        assert _owner_face(F, W, x0 + dx, y0 + dy) == f, (F, W, f, iu, iv, dx, dy)


@pytest.mark.parametrize("c", range(6, 41))
def test_layout_properties_every_cell_size(c):
    """One cell of edge c (F = 2, W = c), both halves: P1 on the 1 / 64 grid, P2, P3; the emulated kernel's own layout agrees."""
    from sparsefusion_amd.mesh import atlas_layout, atlas_uv
    assert atlas_layout(2, c) == (1, c) and tc.emu_atlas_make(2, c) == (0, 1, c)
    uv = atlas_uv(2, c)
    assert uv.dtype == np.float32 and uv.shape == (2, 3, 2)
    xy = _texel_of_uv(uv, c)
    assert np.array_equal(xy, tc.corner_texels(2, c))
    leg = c - 5
    assert [tuple(p) for p in xy[0]] == [(1, 1), (1 + leg, 1), (1, 1 + leg)]
    assert [tuple(p) for p in xy[1]] == [(c - 2, c - 2), (c - 2 - leg, c - 2), (c - 2, c - 2 - leg)]
    for f in (0, 1):
        e1, e2 = xy[f, 1] - xy[f, 0], xy[f, 2] - xy[f, 0]
        assert e1[0] * e2[1] - e1[1] * e2[0] > 0                      # the same winding in both halves
        _check_bilinear(2, c, f, xy[f])
    owners = np.array([[_owner_face(2, c, x, y) for x in range(c)] for y in range(c)])
    assert set(np.unique(owners)) == {0, 1}                           # P3: every texel of the cell is owned, by one of the two


@pytest.mark.parametrize("F,W", [(1, 6), (2, 7), (3, 12), (3, 13), (7, 12), (7, 29), (50, 64), (50, 30)])
def test_layout_edge_cases(F, W):
    """Several cells, W not a multiple of G, the last cell half empty: layout, uv, P1 on a coarser grid, P3, and the kernel's layout"""
    from sparsefusion_amd.mesh import atlas_layout, atlas_uv
    G, c = atlas_layout(F, W)
    assert (G, c) == tc.layout(F, W) and G * G >= (F + 1) // 2 > (G - 1) * (G - 1) and c == W // G and c >= 6
    assert tc.emu_atlas_make(F, W) == (0, G, c)
    uv = atlas_uv(F, W)
    assert uv.shape == (F, 3, 2) and float(uv.min()) > 0 and float(uv.max()) < 1
    xy = _texel_of_uv(uv, W)
    assert np.array_equal(xy, tc.corner_texels(F, W))
    for f in range(F):
        _check_bilinear(F, W, f, xy[f], step=8)
    owners = np.array([[_owner_face(F, W, x, y) for x in range(W)] for y in range(W)])
    used = owners[:G * c, :G * c]
    assert (owners[G * c:] == -1).all() and (owners[:, G * c:] == -1).all()
    for f in range(F):
        assert (used == f).sum() > 0
    for q in range((F + 1) // 2):                                     # P3; the last cell of an odd F has an empty upper half
        cell = used[(q // G) * c:(q // G + 1) * c, (q % G) * c:(q % G + 1) * c]
        assert set(np.unique(cell)) == ({2 * q, 2 * q + 1} if 2 * q + 1 < F else {2 * q, -1})


def test_layout_errors():
    from sparsefusion_amd.mesh import atlas_layout, atlas_uv
    assert atlas_layout(0, 16) == (0, 0) and atlas_uv(0, 16).shape == (0, 3, 2)
    assert tc.emu_atlas_make(0, 16) == (0, 0, 0)
    for F, W, smallest in ((1, 5, 6), (2, 5, 6), (3, 11, 12), (50, 29, 30), (51, 35, 36), (250000, 2048, 6 * 354)):
        with pytest.raises(ValueError, match=f"smallest W is {smallest}"):
            atlas_layout(F, W)
        with pytest.raises(ValueError):
            atlas_uv(F, W)
        rc, G, c = tc.emu_atlas_make(F, W)
        assert rc == 3 and 6 * G == smallest and c == W // G
        assert atlas_layout(F, smallest)[1] == 6
    with pytest.raises(ValueError):
        atlas_layout(1, 0)
    with pytest.raises(ValueError, match="2\\^31"):
        atlas_layout(1, 46341)
    assert tc.emu_atlas_make(1, 0)[0] == 1 and tc.emu_atlas_make(1, 46341)[0] == 2 and tc.emu_atlas_make(1, 46340)[0] == 0


# ------------------------------------------------------------------------------------------------------------------------ writers
def _small_mesh():
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((23, 3)) * np.array([1e-3, 10.0, 3e4])).astype(np.float32)
    f = rng.integers(0, 23, (50, 3)).astype(np.int32)
    n = rng.standard_normal((23, 3)).astype(np.float32)
    return v, f, n


@pytest.mark.parametrize("with_n", [False, True])
def test_export_obj_textured_round_trip(tmp_path, with_n):
    """`vt` text parses back to the same float32 (u, 1 - v_atlas); indices, block order, both face forms; tensors == numpy"""
    from sparsefusion_amd.mesh import atlas_uv, export_obj_textured
    v, f, n = _small_mesh()
    uv = atlas_uv(50, 125)
    a, b = os.path.join(tmp_path, "a.obj"), os.path.join(tmp_path, "b.obj")
    export_obj_textured(v, f, uv, a, "mesh.mtl", normals=n if with_n else None)
    export_obj_textured(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(uv), b, "mesh.mtl",
                        normals=torch.from_numpy(n) if with_n else None)
    assert open(a, "rb").read() == open(b, "rb").read()
    o = tc.parse_obj_textured(a)
    assert o["mtllib"] == "mesh.mtl" and o["usemtl"] == "mat0"
    assert o["order"] == ["mtllib", "v", "vt"] + (["vn"] if with_n else []) + ["usemtl", "f"]
    assert np.array_equal(o["v"].view(np.uint32), v.view(np.uint32)) and np.array_equal(o["f"], f)
    want_vt = np.stack([uv[..., 0], np.float32(1.0) - uv[..., 1]], -1).reshape(-1, 2).astype(np.float32)
    assert np.array_equal(o["vt"].view(np.uint32), want_vt.view(np.uint32))
    assert np.array_equal(o["ft"], np.arange(150).reshape(50, 3))
    if with_n:
        assert np.array_equal(o["vn"].view(np.uint32), n.view(np.uint32)) and np.array_equal(o["fn"], f)
    else:
        assert o["vn"] is None and o["fn"] is None
    lines = open(a).read().splitlines()
    assert lines[0] == "mtllib mesh.mtl" and len(lines) == 2 + 23 * (2 if with_n else 1) + 150 + 50
    first_f = lines[2 + 23 * (2 if with_n else 1) + 150]
    a0, b0, c0 = (int(x) + 1 for x in f[0])
    assert first_f == (f"f {a0}/1/{a0} {b0}/2/{b0} {c0}/3/{c0}" if with_n else f"f {a0}/1 {b0}/2 {c0}/3")
    with pytest.raises(ValueError):
        export_obj_textured(v, f, uv[:10], a, "mesh.mtl")


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (64, 64), (37, 200)])
def test_write_png_round_trip(tmp_path, shape):
    from sparsefusion_amd.mesh import write_png
    rng = np.random.default_rng(shape[0])
    img = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
    img[0, 0] = (255, 0, 128)
    path = os.path.join(tmp_path, "t.png")
    write_png(path, img)
    raw = open(path, "rb").read()
    assert np.array_equal(tc.decode_png(raw), img)
    write_png(path, torch.from_numpy(img))
    assert open(path, "rb").read() == raw
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            assert im.mode == "RGB" and im.size == (shape[1], shape[0]) and np.array_equal(np.asarray(im), img)
    for bad in (img.astype(np.float32), img[..., :2], img[0]):
        with pytest.raises(ValueError):
            write_png(path, bad)


def test_mtl_bytes():
    """the eight lines the reference writes for its material (renderer_df.py:298-306, name = ''), byte for byte"""
    from sparsefusion_amd.mesh import MTL_TEXT
    want = b"newmtl mat0 \nKa 1.000000 1.000000 1.000000 \nKd 1.000000 1.000000 1.000000 \nKs 0.000000 0.000000 0.000000 \n" \
           b"Tr 1.000000 \nillum 1 \nNs 0.000000 \nmap_Kd albedo.png \n"
    assert MTL_TEXT.encode("ascii") == want


# -------------------------------------------------------------------------------------------------------------------------- C ABI
def test_texture_bake_abi_argument_checks():
    """The symbol is in the built library under the declared signature; the argument checks run before any device call, so they
    answer on a machine without a GPU."""
    from sparsefusion_amd import _lib
    res, args = _lib.SIGNATURES["sf_ngp_texture_bake"]
    assert res is C.c_int and len(args) == 11 and args[0] is C.POINTER(_lib.SfNgpField)
    assert [args[k] for k in (2, 4, 5)] == [C.c_uint32] * 3
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparsefusion_hip.h")).read()
    assert "int sf_ngp_texture_bake(const sf_ngp_field* f, const float* verts, uint32_t V, const int32_t* faces, uint32_t F, uint32_t W," \
        in header
    lib = _lib.lib()
    fn = lib.sf_ngp_texture_bake
    f = _lib.SfNgpField()
    buf = (C.c_float * 9)()
    idx = (C.c_int32 * 3)(0, 1, 2)
    out = (C.c_float * 3)()
    pv, pi, po = C.cast(buf, C.c_void_p), C.cast(idx, C.c_void_p), C.cast(out, C.c_void_p)
    INVALID = 1
    assert fn(None, pv, 3, pi, 1, 6, po, None, None, None, None) == INVALID and b"null" in lib.sf_last_error()
    assert fn(C.byref(f), None, 3, pi, 1, 6, po, None, None, None, None) == INVALID
    assert fn(C.byref(f), pv, 3, None, 1, 6, po, None, None, None, None) == INVALID
    assert fn(C.byref(f), pv, 3, pi, 1, 6, None, None, None, None, None) == INVALID and b"output" in lib.sf_last_error()
    assert fn(C.byref(f), pv, 3, pi, 1, 0, po, None, None, None, None) == INVALID and b"W must" in lib.sf_last_error()
    assert fn(C.byref(f), pv, 3, pi, 1, 46341, po, None, None, None, None) == INVALID and b"2^31" in lib.sf_last_error()
    assert fn(C.byref(f), pv, 3, pi, 1, 5, po, None, None, None, None) == INVALID and b"smallest W is 6" in lib.sf_last_error()
    assert fn(C.byref(f), pv, 3, pi, 51, 35, None, None, None, po, None) == INVALID and b"smallest W is 36" in lib.sf_last_error()


def test_public_surface():
    from sparsefusion_amd import mesh
    from sparsefusion_amd.nerf import NeRFRenderer
    assert list(inspect.signature(mesh.atlas_layout).parameters) == ["F", "W"]
    assert list(inspect.signature(mesh.atlas_uv).parameters) == ["F", "W"]
    assert list(inspect.signature(mesh.bake_texture).parameters)[:4] == ["net", "vertices_world", "faces", "W"]
    assert list(inspect.signature(mesh.write_png).parameters) == ["path", "rgb8"]
    sig = inspect.signature(mesh.export_obj_textured)
    assert list(sig.parameters) == ["vertices", "faces", "uvs", "filename", "mtl_name", "normals"]
    assert sig.parameters["normals"].default is None
    sig = inspect.signature(NeRFRenderer.export_mesh_textured)
    assert list(sig.parameters) == ["self", "path", "resolution", "S", "texture_size", "normals"]
    assert sig.parameters["texture_size"].default == 2048 and sig.parameters["normals"].default is True
    assert list(inspect.signature(NeRFRenderer.export_mesh).parameters) == ["self", "path", "resolution", "S"]
    assert list(inspect.signature(mesh.export_obj).parameters) == ["vertices", "faces", "filename", "colors", "normals"]
