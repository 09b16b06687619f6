"""CPU tests of the mesh clean-up (sf_mesh_components / sf_mesh_filter_*; sparsefusion_amd/csrc/mesh_clean.h): the C ABI's
declarations, signatures, symbols and argument checks against the built library (they answer before any device call), the Python
surface -- signatures, docstrings, argument errors, no CPU path --, the unchanged signatures of the existing exporters, and the
references of mesh_clean_common against hand-worked results.  No GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import mesh_clean_common as mc

INVALID = 1
NAMES = ("sf_mesh_components_workspace_bytes", "sf_mesh_components", "sf_mesh_filter_workspace_bytes", "sf_mesh_filter_count",
         "sf_mesh_filter_emit")


# -------------------------------------------------------------------------------------------------------------------- 1. C ABI
def test_declarations_signatures_and_symbols_agree():
    from sparsefusion_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparsefusion_hip.h")).read()
    lib = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES and f" {name}(" in header and hasattr(lib, name)
    for name in (NAMES[0], NAMES[2]):
        assert _lib.SIGNATURES[name] == (C.c_uint64, [C.c_uint32, C.c_uint32])
    res, args = _lib.SIGNATURES["sf_mesh_components"]
    assert res is C.c_int and len(args) == 10 and [i for i, a in enumerate(args) if a is C.c_uint32] == [1, 2] and args[8] is C.c_uint64
    res, args = _lib.SIGNATURES["sf_mesh_filter_count"]
    assert res is C.c_int and len(args) == 12 and [i for i, a in enumerate(args) if a is C.c_uint32] == [1, 2, 6]
    assert args[7] is C.c_double and args[9] is C.c_uint64
    assert "uint32_t min_faces, double min_fraction," in header
    res, args = _lib.SIGNATURES["sf_mesh_filter_emit"]
    assert res is C.c_int and len(args) == 11 and [i for i, a in enumerate(args) if a is C.c_uint32] == [2, 3] and args[5] is C.c_uint64


def test_workspace_sizes():
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    assert lib.sf_mesh_components_workspace_bytes(0, 0) == 0 and lib.sf_mesh_components_workspace_bytes(0, 9) == 0
    assert lib.sf_mesh_components_workspace_bytes(1000, 1) >= 4000
    assert lib.sf_mesh_filter_workspace_bytes(0, 0) > 0
    assert lib.sf_mesh_filter_workspace_bytes(1000, 3000) >= 1000 + 3000 + 4000 + 2 * 8 * 3
    for fn in (lib.sf_mesh_components_workspace_bytes, lib.sf_mesh_filter_workspace_bytes):
        assert fn(1 << 31, 1) == 0 and fn(1, 1 << 31) == 0 and fn((1 << 31) - 1, (1 << 31) - 1) > 0      # 0: unsupported size


def test_argument_checks_answer_without_a_device():
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint32 * 4096)()
    pb = C.cast(buf, C.c_void_p)
    big = 1 << 20

    def comp(faces=pb, F=4, V=4, vl=pb, fl=pb, per=pb, counts=pb, ws=pb, wb=big):
        return lib.sf_mesh_components(faces, F, V, vl, fl, per, counts, ws, wb, None)

    for name in ("faces", "vl", "per", "counts", "ws"):
        assert comp(**{name: None}) == INVALID, name
        assert b"null pointer" in lib.sf_last_error()
    for kw in (dict(V=1 << 31), dict(F=1 << 31), dict(V=(1 << 32) - 1)):
        assert comp(**kw) == INVALID and b"2^31" in lib.sf_last_error()
    need = lib.sf_mesh_components_workspace_bytes(1000, 4)
    assert comp(V=1000, wb=need - 1) == INVALID and b"workspace too small" in lib.sf_last_error()

    def count(faces=pb, F=4, V=4, vl=pb, per=pb, c3=pb, mf=8, frac=0.0, ws=pb, wb=big, c2=pb):
        return lib.sf_mesh_filter_count(faces, F, V, vl, per, c3, mf, frac, ws, wb, c2, None)

    for name in ("faces", "vl", "per", "c3", "ws", "c2"):
        assert count(**{name: None}) == INVALID, name
        assert b"null pointer" in lib.sf_last_error()
    for kw in (dict(V=1 << 31), dict(F=1 << 31)):
        assert count(**kw) == INVALID and b"2^31" in lib.sf_last_error()
    need = lib.sf_mesh_filter_workspace_bytes(4, 4)
    assert count(wb=need - 1) == INVALID and b"workspace too small" in lib.sf_last_error()
    for frac in (-1e-9, 1.0 + 1e-9, 2.0, float("inf"), float("-inf"), float("nan")):
        assert count(frac=frac) == INVALID, frac
        assert b"min_fraction" in lib.sf_last_error()

    def emit(verts=pb, faces=pb, F=4, V=4, ws=pb, wb=big):
        return lib.sf_mesh_filter_emit(verts, faces, F, V, ws, wb, pb, pb, pb, pb, None)

    for name in ("verts", "faces", "ws"):
        assert emit(**{name: None}) == INVALID, name
        assert b"null pointer" in lib.sf_last_error()
    for kw in (dict(V=1 << 31), dict(F=1 << 31)):
        assert emit(**kw) == INVALID and b"2^31" in lib.sf_last_error()
    assert emit(wb=need - 1) == INVALID and b"workspace too small" in lib.sf_last_error()


# ------------------------------------------------------------------------------------------------------------ 2. Python surface
def test_public_surface():
    from sparsefusion_amd import mesh
    from sparsefusion_amd.nerf import NeRFRenderer
    assert list(inspect.signature(mesh.connected_components).parameters) == ["faces", "num_vertices"]
    sig = inspect.signature(mesh.clean_mesh)
    assert list(sig.parameters) == ["vertices", "faces", "min_faces", "min_fraction"]
    assert sig.parameters["min_faces"].default == 8 and sig.parameters["min_fraction"].default == 0.0
    sig = inspect.signature(NeRFRenderer.export_mesh_cleaned)
    assert list(sig.parameters) == ["self", "path", "resolution", "S", "min_faces", "min_fraction", "epsilon", "texture_size"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, 128, 8, 0.0, None, None]
    doc = " ".join(mesh.connected_components.__doc__.split())
    for phrase in ("by INDEX only", "unwelded", "smallest vertex index", "invalid", "degenerate", "unreferenced"):
        assert phrase in doc, phrase
    doc = " ".join(mesh.clean_mesh.__doc__.split())
    for phrase in ("ceil(min_fraction * largest)", "bit copies", "strictly increasing", "not reference behaviour", "diameter"):
        assert phrase in doc, phrase
    doc = " ".join(NeRFRenderer.export_mesh_cleaned.__doc__.split())
    for phrase in ("mcubes_mesh_clean.obj", "mcubes_mesh_clean.ply", "not reference behaviour", "vertex_ids"):
        assert phrase in doc, phrase


def test_existing_exporters_keep_their_signatures():
    from sparsefusion_amd import mesh
    from sparsefusion_amd.nerf import NeRFRenderer
    params = lambda fn: list(inspect.signature(fn).parameters)      # noqa: E731
    assert params(NeRFRenderer.export_mesh) == ["self", "path", "resolution", "S"]
    assert params(NeRFRenderer.export_mesh_attributes) == ["self", "path", "resolution", "S", "epsilon"]
    assert params(NeRFRenderer.export_mesh_textured) == ["self", "path", "resolution", "S", "texture_size", "normals"]
    assert params(NeRFRenderer._mesh_geometry) == ["self", "R"]
    assert params(mesh.export_obj) == ["vertices", "faces", "filename", "colors", "normals"]
    assert params(mesh.export_ply) == ["vertices", "faces", "filename", "colors", "normals"]
    assert params(mesh.export_obj_textured) == ["vertices", "faces", "uvs", "filename", "mtl_name", "normals"]
    assert params(mesh.vertex_attributes) == ["net", "vertices_world", "epsilon"]
    assert params(mesh.atlas_uv) == ["F", "W"] and params(mesh.atlas_layout) == ["F", "W"]
    assert params(mesh.marching_cubes) == ["volume", "isovalue"]


def test_argument_errors_and_no_cpu_path():
    from sparsefusion_amd import mesh
    f = torch.zeros(4, 3, dtype=torch.int32)
    v = torch.zeros(5, 3)
    with pytest.raises(TypeError):
        mesh.connected_components([[0, 1, 2]], 3)
    with pytest.raises(TypeError):
        mesh.connected_components(f.float(), 3)
    with pytest.raises(TypeError):
        mesh.connected_components(np.zeros((4, 3), dtype=np.uint8), 3)
    with pytest.raises(TypeError):
        mesh.connected_components(f, 3.0)
    for bad in (torch.zeros(4, 4, dtype=torch.int32), torch.zeros(12, dtype=torch.int32), np.zeros((2, 3, 1), dtype=np.int32)):
        with pytest.raises(ValueError, match=r"faces \[F, 3\]"):
            mesh.connected_components(bad, 3)
    for V in (-1, 1 << 31):
        with pytest.raises(ValueError, match="num_vertices"):
            mesh.connected_components(f, V)
    with pytest.raises(RuntimeError, match="HIP device"):               # there is no CPU path
        mesh.connected_components(f, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh.connected_components(f.long(), 5)
    if not torch.cuda.is_available():                                   # numpy input has no device to run on either
        with pytest.raises(RuntimeError, match="HIP device"):
            mesh.connected_components(f.numpy(), 5)
        with pytest.raises(RuntimeError, match="HIP device"):
            mesh.clean_mesh(v.numpy(), f.numpy())
    with pytest.raises(TypeError):
        mesh.clean_mesh([[0.0, 0.0, 0.0]], f)
    with pytest.raises(TypeError):
        mesh.clean_mesh(v.double(), f)
    with pytest.raises(TypeError):
        mesh.clean_mesh(v, f.numpy())
    with pytest.raises(TypeError):
        mesh.clean_mesh(v, f, min_faces=2.5)
    with pytest.raises(ValueError, match=r"vertices \[V, 3\]"):
        mesh.clean_mesh(torch.zeros(5, 2), f)
    with pytest.raises(ValueError, match="min_faces"):
        mesh.clean_mesh(v, f, min_faces=-1)
    for frac in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_fraction"):
            mesh.clean_mesh(v, f, min_fraction=frac)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh.clean_mesh(v, f)


# ----------------------------------------------------------------------------------------------------------------- 3. references
def test_references_on_a_hand_worked_mesh():
    c = mc.case("mixed")
    r = c["ref"]
    assert r["vertex_label"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 8, 8, 8, 11, 12, 12]
    assert r["faces_per_label"].tolist() == [4, 0, 0, 0, 4, 0, 0, 0, 1, 0, 0, 0, 1, 0]
    assert (r["n_components"], r["largest"], r["n_invalid"]) == (4, 4, 4)
    assert r["face_label"].tolist() == [4, 4, 4, 4, -1, 0, 0, 8, -1, 0, 0, 12, -1, -1]
    v2, f2, vi, fi = c["clean"][4, 0.0]                                 # the two tetrahedra stay, in their old order
    assert vi.tolist() == list(range(8)) and fi.tolist() == [0, 1, 2, 3, 5, 6, 9, 10]
    assert np.array_equal(f2, c["faces"][fi]) and np.array_equal(mc.bits(v2), mc.bits(c["vertices"][:8]))
    assert c["clean"][5, 0.0][1].shape[0] == 0 and c["clean"][5, 0.0][0].shape == (0, 3)
    v2, f2, vi, fi = c["clean"][1, 0.0]                                 # every valid face; the unreferenced vertex 11 goes
    assert vi.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13] and fi.size == 10 and f2[-1].tolist() == [11, 11, 12]
    assert np.array_equal(c["clean"][0, 0.25][3], fi) and np.array_equal(c["clean"][0, 0.26][3], c["clean"][4, 0.0][3])
    assert np.array_equal(c["clean"][0, 1.0][3], c["clean"][4, 0.0][3])   # both tetrahedra tie for largest


def test_blob_volume_reference_properties():
    vol = mc.blob_volume()
    assert vol.shape == (48, 48, 48) and vol.dtype == np.float32 and float(vol.max()) == 1.0 and float(vol.min()) == 0.0
    assert int((vol >= 0.5).sum()) > 5000
    closed, chi = mc.closed_and_euler(np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]]), 4)      # a tetrahedron
    assert closed and chi == 2
    assert mc.closed_and_euler(np.array([[0, 1, 2]]), 3) == (False, 1)
