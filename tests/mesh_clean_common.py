"""Shared by the mesh clean-up tests (sf_mesh_components / sf_mesh_filter_*; sparsefusion_amd/csrc/mesh_clean.h): the seeded cases,
the CPU references -- scipy.sparse.csgraph.connected_components on the vertex graph of the valid faces, re-labelled to the smallest
vertex index per component, and a numpy restatement of the keep rule and the order-preserving compaction --, the exact comparisons,
and the ctypes harness of tests/hostemu/mesh_clean_emu.cpp.  Every comparison is equality; vertex rows are compared as bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import scipy.sparse
import scipy.sparse.csgraph


# --------------------------------------------------------------------------------------------------------------------- references
def valid_faces(faces, V):
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    return ((f >= 0) & (f < V)).all(axis=1)


def reference_components(faces, V):
    """dict of vertex_label [V] int32, face_label [F] int32 (-1: invalid), faces_per_label [V] int32, n_components, largest,
    n_invalid -- scipy's components of the graph with an edge per pair of vertices a valid face names, labelled by their smallest
    vertex index"""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    valid = valid_faces(f, V)
    fv = f[valid]
    if V == 0:
        lab = np.zeros(0, dtype=np.int64)
    else:
        rows, cols = np.concatenate([fv[:, 0], fv[:, 1], fv[:, 2]]), np.concatenate([fv[:, 1], fv[:, 2], fv[:, 0]])
        g = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(V, V)).tocsr()
        n, comp = scipy.sparse.csgraph.connected_components(g, directed=False)
        smallest = np.full(n, V, dtype=np.int64)
        np.minimum.at(smallest, comp, np.arange(V))
        lab = smallest[comp]
    face_label = np.full(f.shape[0], -1, dtype=np.int64)
    face_label[valid] = lab[fv[:, 0]]
    per = np.bincount(face_label[valid], minlength=V).astype(np.int64)[:V] if V else np.zeros(0, dtype=np.int64)
    return dict(vertex_label=lab.astype(np.int32), face_label=face_label.astype(np.int32), faces_per_label=per.astype(np.int32),
                n_components=int((per > 0).sum()), largest=int(per.max()) if V else 0, n_invalid=int((~valid).sum()))


def reference_clean(vertices, faces, V, ref, min_faces, min_fraction):
    """(vertices' [V', 3], faces' [F', 3] int32, vertex_ids [V'] int32, face_ids [F'] int32) of the keep rule on `ref`"""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    per = ref["faces_per_label"].astype(np.int64)
    need = np.ceil(np.float64(min_fraction) * np.float64(ref["largest"]))
    comp_keep = (per >= int(min_faces)) & (per.astype(np.float64) >= need)
    fl = ref["face_label"].astype(np.int64)
    face_keep = fl >= 0
    face_keep[face_keep] = comp_keep[fl[face_keep]]
    vert_keep = np.zeros(V, dtype=bool)
    vert_keep[f[face_keep].ravel()] = True
    vertex_ids, face_ids = np.flatnonzero(vert_keep), np.flatnonzero(face_keep)
    remap = np.cumsum(vert_keep) - 1
    return (np.asarray(vertices).reshape(-1, 3)[vertex_ids], remap[f[face_keep]].astype(np.int32).reshape(-1, 3),
            vertex_ids.astype(np.int32), face_ids.astype(np.int32))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def assert_components_equal(got, ref):
    for k in ("vertex_label", "face_label", "faces_per_label"):
        g = np.asarray(got[k])
        assert g.shape == ref[k].shape and g.dtype == np.int32, (k, g.shape, g.dtype)
        assert np.array_equal(g, ref[k]), k
    for k in ("n_components", "largest", "n_invalid"):
        assert int(got[k]) == ref[k], (k, int(got[k]), ref[k])


def assert_clean_equal(got, want):
    (v, f, vi, fi), (rv, rf, rvi, rfi) = (tuple(np.asarray(a) for a in t) for t in (got, want))
    assert v.shape == rv.shape and f.shape == rf.shape and vi.shape == rvi.shape and fi.shape == rfi.shape, \
        (v.shape, rv.shape, f.shape, rf.shape)
    assert v.dtype == np.float32 and f.dtype == np.int32 and vi.dtype == np.int32 and fi.dtype == np.int32
    assert np.array_equal(vi, rvi) and np.array_equal(fi, rfi)
    assert np.array_equal(f, rf)
    assert np.array_equal(bits(v), bits(rv))
    assert bool((np.diff(vi) > 0).all()) and bool((np.diff(fi) > 0).all())


# -------------------------------------------------------------------------------------------------------------------------- cases
def _rows(rng, V):
    """vertex rows of arbitrary bit patterns (NaNs, infinities, -0 and denormals included): a copy must keep the bits"""
    v = rng.integers(0, 1 << 32, size=(V, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    if V:
        v[0] = np.array([-0.0, np.nan, np.inf], dtype=np.float32)
    return v


def _strips(rng, lengths, permute=True, shuffle_faces=True):
    """one triangle strip (a component of n faces on n + 2 vertices) per entry of lengths"""
    lengths = np.asarray(lengths, dtype=np.int64)
    F, K = int(lengths.sum()), lengths.size
    k = np.repeat(np.arange(K), lengths)
    first = np.arange(F) + 2 * k                                    # strip k starts 2 k vertices later than its faces do
    faces = np.stack([first, first + 1, first + 2], axis=1)
    V = F + 2 * K
    if permute:
        faces = rng.permutation(V)[faces]
    if shuffle_faces:
        faces = faces[rng.permutation(F)]
    return faces.astype(np.int32), V


def _clusters(rng, F, V, groups):
    """F random faces, each inside one of `groups` vertex groups (interleaved numbering): several components, unreferenced
    vertices, repeated indices"""
    grp = rng.integers(0, groups, size=F)
    per = V // groups
    local = rng.integers(0, per, size=(F, 3))
    return (local * groups + grp[:, None]).astype(np.int32)


def _mixed():
    tet = lambda o: [[o, o + 1, o + 2], [o, o + 1, o + 3], [o, o + 2, o + 3], [o + 1, o + 2, o + 3]]      # noqa: E731
    V = 14                                                          # 0-3, 4-7 tetrahedra; 8-10 triangle; 11 unreferenced; 12, 13 degenerate
    faces = tet(4) + [[0, 1, V]] + tet(0)[:2] + [[8, 9, 10], [-1, 2, 3]] + tet(0)[2:] + [[12, 12, 13], [5, 6, 1 << 30], [-5, -6, -7]]
    return np.array(faces, dtype=np.int32), V


DEFAULT_RULES = ((8, 0.0), (0, 0.0), (1, 1.0), (2, 0.5))


def make_case(name):
    """name -> dict(vertices [V, 3] float32, faces [F, 3] int32, V, rules = ((min_faces, min_fraction), ..)); seeded by the name"""
    rng = np.random.default_rng(sum(name.encode()) * 7919 + len(name))
    rules = DEFAULT_RULES
    if name == "f0":
        faces, V = np.zeros((0, 3), dtype=np.int32), 5
    elif name == "v0":
        faces, V = np.zeros((0, 3), dtype=np.int32), 0
    elif name == "v0_f2":
        faces, V = np.array([[0, 1, 2], [0, 0, 0]], dtype=np.int32), 0
    elif name == "one":
        faces, V = np.array([[2, 0, 1]], dtype=np.int32), 3
        rules = ((1, 0.0), (2, 0.0), (0, 1.0))
    elif name == "mixed":
        faces, V = _mixed()
        rules = ((4, 0.0), (5, 0.0), (1, 0.0), (2, 0.0), (0, 1.0), (0, 0.25), (0, 0.26))
    elif name == "clash":
        # faces 0..63 (one wave) build a star around vertex 1 (leaves 3, 5, ..) and one around vertex 2 (leaves 4, 6, ..); every face
        # of the next wave names a leaf of each and vertex 0: its 64 lanes all find the roots 1 and 2, then 0, and race for one word
        i, j = np.arange(32), np.arange(64)
        star = lambda r, leaf: np.stack([np.full(32, r), leaf, leaf], axis=1)      # noqa: E731
        bridge = np.stack([3 + 2 * (j % 32), 4 + 2 * ((j * 5) % 32), np.zeros(64, dtype=np.int64)], axis=1)
        faces, V = np.concatenate([star(1, 3 + 2 * i), star(2, 4 + 2 * i), bridge]).astype(np.int32), 67
        rules = ((8, 0.0), (129, 0.0), (0, 1.0))
    elif name.startswith("rand"):
        F = int(name[4:])
        V = (F * 7) // 10 + 3
        faces = _clusters(rng, F, V, groups=max(2, F // 40))
        rules = ((8, 0.0), (0, 0.0), (3, 0.3), (0, 1.0))
    elif name == "strip":
        faces, V = _strips(rng, [20011], shuffle_faces=False)
        rules = ((8, 0.0), (20012, 0.0), (0, 1.0))
    elif name == "many":
        faces, V = _strips(rng, 1 + (np.arange(1003) * 5) % 12)      # sizes 1..12, largest 12
        rules = ((5, 0.0), (6, 0.0), (7, 0.0), (0, 0.0), (0, 1.0), (0, 0.5), (3, 0.75), (12, 0.51))      # ceil: 6 and 9 exactly, 7
    elif name == "big":
        lengths = rng.integers(1, 2000, size=900)                    # about 0.9 M faces in short strips, the rest in one long strip
        lengths[0] = 1_100_000 - int(lengths[1:].sum())
        faces, V = _strips(rng, lengths)
        rules = ((8, 0.0), (100, 0.001), (0, 1.0))
    else:
        raise KeyError(name)
    return dict(name=name, vertices=_rows(rng, V), faces=faces, V=V, rules=rules)


SMALL_CASES = ("f0", "v0", "v0_f2", "one", "mixed", "clash", "rand255", "rand256", "rand257", "rand1025", "strip", "many")
BIG_CASE = "big"

_cache = {}


def case(name):
    """the case with its references: ref = reference_components, clean[rule] = reference_clean -- built once, shared, never
    modified"""
    if name not in _cache:
        c = make_case(name)
        c["ref"] = reference_components(c["faces"], c["V"])
        c["clean"] = {r: reference_clean(c["vertices"], c["faces"], c["V"], c["ref"], *r) for r in c["rules"]}
        for a in (c["vertices"], c["faces"], *c["ref"].values(), *(x for t in c["clean"].values() for x in t)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = c
    return _cache[name]


def blob_volume(n=48):
    """synthetic density of one large blob, one small blob and three single-cell specks, float32 [n, n, n]; the level is 0.5"""
    x = np.arange(n, dtype=np.float64)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    ball = lambda c, r: np.clip(r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2), 0.0, 1.0)      # noqa: E731
    vol = np.maximum(ball((20.3, 22.1, 24.7), 13.4), ball((40.2, 40.6, 8.9), 3.3))
    for p in ((4, 5, 40), (43, 6, 41), (7, 42, 42)):
        vol[p] = 1.0
    return vol.astype(np.float32)


def blob_case():
    """the marching-cubes mesh of blob_volume() at level 0.5 by the numpy marching cubes of tests/mesh_ref.py (the canonical order
    of the GPU's), as a case with its references -- built once, shared, never modified"""
    if "blob" not in _cache:
        import mesh_ref
        v, f = mesh_ref.marching_cubes(blob_volume(), 0.5)
        c = dict(name="blob", vertices=np.ascontiguousarray(v, dtype=np.float32), faces=np.ascontiguousarray(f, dtype=np.int32),
                 V=int(v.shape[0]), rules=((8, 0.5), (8, 0.0), (9, 0.0)))
        c["ref"] = reference_components(c["faces"], c["V"])
        c["clean"] = {r: reference_clean(c["vertices"], c["faces"], c["V"], c["ref"], *r) for r in c["rules"]}
        for a in (c["vertices"], c["faces"], *c["ref"].values(), *(x for t in c["clean"].values() for x in t)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache["blob"] = c
    return _cache["blob"]


def closed_and_euler(faces, V):
    """(every undirected edge lies in exactly two faces, V - E + F)"""
    f = np.asarray(faces).astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return bool((counts == 2).all()), V - counts.size + f.shape[0]


# ------------------------------------------------------------------------------------------------------------------ host emulation
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
_SO = os.path.join(_HERE, "_build", "libmesh_clean_emu.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
_handle = None


def emu_available():
    return os.path.exists(CLANG)


def _emu():
    global _handle
    if _handle is None:
        csrc = os.path.join(_HERE, "..", "..", "sparsefusion_amd", "csrc")
        deps = [os.path.join(_HERE, f) for f in ("mesh_clean_emu.cpp", "hip_emu.h")] + \
               [os.path.join(csrc, f) for f in ("mesh_clean.h", "mesh_kernels.h", "sf_dev.h", "sf_operand.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(s) for s in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call([CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + _HERE, "-Wall", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-Wno-source-uses-openmp", "-ffp-contract=off", deps[0], "-o", _SO,
                                   "-lpthread"])
        _handle = C.CDLL(_SO)
        _handle.emu_mesh_components.restype = None
        _handle.emu_mesh_filter.restype = None
    return _handle


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else C.c_void_p(0)


SENTINEL = -77


def emu_components(faces, V, nt=256, max_blocks=0, with_face_label=True):
    """sf_mesh_components on CPU fibers -> the dict of connected_components; the outputs are pre-filled with a sentinel"""
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    F = f.shape[0]
    vl, fl = np.full(V, SENTINEL, dtype=np.int32), np.full(F, SENTINEL, dtype=np.int32)
    per, counts = np.full(V, SENTINEL, dtype=np.int32), np.full(3, SENTINEL, dtype=np.int32)
    _emu().emu_mesh_components(_p(f), C.c_uint32(F), C.c_uint32(V), _p(vl), _p(fl if with_face_label else None), _p(per), _p(counts),
                               C.c_uint32(nt), C.c_uint32(max_blocks))
    return dict(vertex_label=vl, face_label=fl, faces_per_label=per, n_components=int(counts[0]), largest=int(counts[1]),
                n_invalid=int(counts[2]))


def emu_clean(vertices, faces, V, comp, min_faces, min_fraction, nt=256, max_blocks=0):
    """sf_mesh_filter_count + sf_mesh_filter_emit on CPU fibers over the components `comp` -> (vertices', faces', vertex_ids, face_ids)"""
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    F = f.shape[0]
    counts3 = np.array([comp["n_components"], comp["largest"], comp["n_invalid"]], dtype=np.uint32)
    counts2 = np.full(2, 0xdeadbeef, dtype=np.uint32)
    args = lambda *out: (_p(v), _p(f), C.c_uint32(F), C.c_uint32(V), _p(comp["vertex_label"]), _p(comp["faces_per_label"]),      # noqa: E731
                         _p(counts3), C.c_uint32(min_faces), C.c_double(min_fraction), _p(counts2), *out, C.c_uint32(nt),
                         C.c_uint32(max_blocks))
    _emu().emu_mesh_filter(*args(None, None, None, None))
    V2, F2 = int(counts2[0]), int(counts2[1])
    assert 0 <= V2 <= V and 0 <= F2 <= F, (V2, F2)
    pad = 4                                                        # rows past V' / F' must stay untouched
    ov = np.full((V2 + pad, 3), SENTINEL, dtype=np.float32)
    of, vi, fi = (np.full(s, SENTINEL, dtype=np.int32) for s in ((F2 + pad, 3), V2 + pad, F2 + pad))
    _emu().emu_mesh_filter(*args(_p(ov), _p(of), _p(vi), _p(fi)))
    assert (int(counts2[0]), int(counts2[1])) == (V2, F2)
    assert bool((ov[V2:] == SENTINEL).all() and (of[F2:] == SENTINEL).all() and (vi[V2:] == SENTINEL).all() and (fi[F2:] == SENTINEL).all())
    return ov[:V2], of[:F2], vi[:V2], fi[:F2]
