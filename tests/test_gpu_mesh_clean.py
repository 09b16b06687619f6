"""GPU tests of the mesh clean-up: sf_mesh_components / sf_mesh_filter_count / sf_mesh_filter_emit through the C ABI and through
mesh.connected_components / mesh.clean_mesh, and NeRFRenderer.export_mesh_cleaned, against scipy's connected components re-labelled
to the smallest vertex index and the numpy restatement of the keep rule and compaction (mesh_clean_common).  Every comparison is
equality; vertex rows are compared as bits.  Field: `teacher` of tests/golden/ngp_render.pt."""
import os

import numpy as np
import pytest
import torch

import mesh_clean_common as mc
import point_attrs_common as pc
import texture_common as tc
from ngp_common import params_from_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_CASES = mc.SMALL_CASES + (mc.BIG_CASE,)
PAD = 5                                                            # rows past the end of every output: they must stay untouched
INVALID = 1


def _pz(t):
    from sparsefusion_amd import _lib
    return _lib.ptr(t if t is not None and t.numel() else None)


def _entry_components(faces, V, with_face_label=True):
    """sf_mesh_components into sentinel-filled buffers with PAD spare rows -> (dict of host arrays, device tensors for the filter)"""
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    f = torch.tensor(faces).to(DEV)
    F = f.shape[0]
    full = lambda n: torch.full((n + PAD,), mc.SENTINEL, dtype=torch.int32, device=DEV)      # noqa: E731
    vl, fl, per, counts = full(V), full(F), full(V), full(3)
    wb = lib.sf_mesh_components_workspace_bytes(V, F)
    ws = torch.empty(wb, dtype=torch.uint8, device=DEV)
    rc = lib.sf_mesh_components(_pz(f), F, V, _lib.ptr(vl), _lib.ptr(fl) if with_face_label else None, _lib.ptr(per), _lib.ptr(counts),
                                _pz(ws), wb, _lib.stream_ptr())
    _lib.check(rc, "mesh_components")
    torch.cuda.synchronize()
    for t, n in ((vl, V), (fl, F), (per, V), (counts, 3)):
        assert bool((t[n:] == mc.SENTINEL).all())                  # nothing past the end
    h = lambda t, n: t[:n].cpu().numpy()                           # noqa: E731
    c3 = h(counts, 3)
    return dict(vertex_label=h(vl, V), face_label=h(fl, F), faces_per_label=h(per, V), n_components=int(c3[0]), largest=int(c3[1]),
                n_invalid=int(c3[2])), (f, vl, per, counts)


def _entry_clean(vertices, dev, V, min_faces, min_fraction):
    """sf_mesh_filter_count + sf_mesh_filter_emit into sentinel-filled buffers of V' + PAD / F' + PAD rows"""
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    f, vl, per, counts = dev
    F = f.shape[0]
    v = torch.tensor(vertices).to(DEV)
    wb = lib.sf_mesh_filter_workspace_bytes(V, F)
    ws = torch.empty(wb, dtype=torch.uint8, device=DEV)
    c2 = torch.full((2 + PAD,), mc.SENTINEL, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr()
    _lib.check(lib.sf_mesh_filter_count(_pz(f), F, V, _lib.ptr(vl), _lib.ptr(per), _lib.ptr(counts), min_faces, min_fraction, _lib.ptr(ws),
                                        wb, _lib.ptr(c2), st), "mesh_filter_count")
    V2, F2 = (int(x) for x in c2[:2].cpu())
    assert bool((c2[2:] == mc.SENTINEL).all()) and 0 <= V2 <= V and 0 <= F2 <= F
    ov = torch.full((V2 + PAD, 3), float(mc.SENTINEL), dtype=torch.float32, device=DEV)
    of = torch.full((F2 + PAD, 3), mc.SENTINEL, dtype=torch.int32, device=DEV)
    vi = torch.full((V2 + PAD,), mc.SENTINEL, dtype=torch.int32, device=DEV)
    fi = torch.full((F2 + PAD,), mc.SENTINEL, dtype=torch.int32, device=DEV)
    _lib.check(lib.sf_mesh_filter_emit(_pz(v), _pz(f), F, V, _lib.ptr(ws), wb, _lib.ptr(ov), _lib.ptr(of), _lib.ptr(vi), _lib.ptr(fi), st),
               "mesh_filter_emit")
    torch.cuda.synchronize()
    assert bool((ov[V2:] == mc.SENTINEL).all() and (of[F2:] == mc.SENTINEL).all() and (vi[V2:] == mc.SENTINEL).all()
                and (fi[F2:] == mc.SENTINEL).all())
    return tuple(t[:n].cpu().numpy() for t, n in ((ov, V2), (of, F2), (vi, V2), (fi, F2)))


# ------------------------------------------------------------------------------------------------------------------ 1. C entries
@pytest.mark.parametrize("name", ALL_CASES)
def test_entries_equal_the_references_and_touch_nothing_else(name):
    c = mc.case(name)
    got, dev = _entry_components(c["faces"], c["V"])
    mc.assert_components_equal(got, c["ref"])
    for rule in c["rules"]:
        mc.assert_clean_equal(_entry_clean(c["vertices"], dev, c["V"], *rule), c["clean"][rule])
    if c["faces"].shape[0] == 0 or c["V"] == 0:                    # the defined empty result
        assert np.array_equal(got["vertex_label"], np.arange(c["V"])) and not got["faces_per_label"].any()
        assert (got["n_components"], got["largest"]) == (0, 0) and got["n_invalid"] == c["faces"].shape[0]
        assert all(t[1].shape[0] == 0 and t[0].shape[0] == 0 for t in c["clean"].values())


@pytest.mark.parametrize("name", ("mixed", "rand1025", "strip", "many", mc.BIG_CASE))
def test_a_second_run_gives_identical_bits_on_another_stream(name):
    c = mc.case(name)
    first, dev1 = _entry_components(c["faces"], c["V"])
    a = _entry_clean(c["vertices"], dev1, c["V"], *c["rules"][0])
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        second, dev2 = _entry_components(c["faces"], c["V"], with_face_label=False)
        b = _entry_clean(c["vertices"], dev2, c["V"], *c["rules"][0])
    assert bool((second.pop("face_label") == mc.SENTINEL).all())    # a NULL face_label is skipped
    first.pop("face_label")
    assert all(np.array_equal(first[k], second[k]) for k in first)
    assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


def test_invalid_arguments_are_rejected_with_device_pointers():
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    buf = torch.zeros(12, 4096, dtype=torch.int32, device=DEV)     # one row per argument: nothing aliases
    faces, vl, per, c3, ws, c2, verts, fl, o0, o1, o2, o3 = (_lib.ptr(buf[k]) for k in range(12))
    big = 4096 * 4
    comp = lambda faces=faces, F=4, V=4, vl=vl, per=per, counts=c3, ws=ws, wb=big: lib.sf_mesh_components(      # noqa: E731
        faces, F, V, vl, fl, per, counts, ws, wb, None)
    count = lambda faces=faces, F=4, V=4, vl=vl, per=per, c3=c3, frac=0.0, ws=ws, wb=big, c2=c2: lib.sf_mesh_filter_count(      # noqa: E731
        faces, F, V, vl, per, c3, 2, frac, ws, wb, c2, None)
    emit = lambda verts=verts, faces=faces, F=4, V=4, ws=ws, wb=big: lib.sf_mesh_filter_emit(      # noqa: E731
        verts, faces, F, V, ws, wb, o0, o1, o2, o3, None)
    for fn, names in ((comp, ("faces", "vl", "per", "counts", "ws")), (count, ("faces", "vl", "per", "c3", "ws", "c2")),
                      (emit, ("verts", "faces", "ws"))):
        for n in names:
            assert fn(**{n: None}) == INVALID, n
        assert fn(V=1 << 31) == INVALID and fn(F=1 << 31) == INVALID
        assert fn(V=4000, wb=4000) == INVALID and b"workspace too small" in lib.sf_last_error()
    for frac in (-0.5, 1.25, float("nan"), float("inf")):
        assert count(frac=frac) == INVALID and b"min_fraction" in lib.sf_last_error()
    torch.cuda.synchronize()
    assert not buf.any()                                           # rejected before any device call
    assert comp() == 0 and count() == 0 and emit() == 0            # and the same arguments, valid, run: four faces (0, 0, 0)
    torch.cuda.synchronize()
    assert buf[1, :4].tolist() == [0, 1, 2, 3] and buf[2, :4].tolist() == [4, 0, 0, 0] and buf[3, :3].tolist() == [1, 4, 0]
    assert buf[5, :2].tolist() == [1, 4] and buf[10, :1].tolist() == [0] and buf[11, :4].tolist() == [0, 1, 2, 3]


# --------------------------------------------------------------------------------------------------------------- 2. Python wrappers
@pytest.mark.parametrize("name", ALL_CASES)
def test_wrappers_on_device_tensors(name):
    from sparsefusion_amd import mesh
    c = mc.case(name)
    f, v = torch.tensor(c["faces"]).to(DEV), torch.tensor(c["vertices"]).to(DEV)
    got = mesh.connected_components(f, c["V"])
    assert all(got[k].is_cuda and got[k].dtype == torch.int32 for k in ("vertex_label", "face_label", "faces_per_label"))
    assert all(type(got[k]) is int for k in ("n_components", "largest", "n_invalid"))
    mc.assert_components_equal({k: (t.cpu().numpy() if isinstance(t, torch.Tensor) else t) for k, t in got.items()}, c["ref"])
    for rule in c["rules"]:
        out = mesh.clean_mesh(v, f, *rule)
        assert all(t.is_cuda for t in out)
        mc.assert_clean_equal(tuple(t.cpu().numpy() for t in out), c["clean"][rule])


@pytest.mark.parametrize("name", mc.SMALL_CASES)
def test_wrappers_on_numpy_int64_and_views(name):
    from sparsefusion_amd import mesh
    c = mc.case(name)
    rule = c["rules"][0]
    got = mesh.connected_components(c["faces"], c["V"])                                       # numpy in -> numpy out
    assert all(isinstance(got[k], np.ndarray) for k in ("vertex_label", "face_label", "faces_per_label"))
    mc.assert_components_equal(got, c["ref"])
    out = mesh.clean_mesh(c["vertices"], c["faces"], *rule)
    assert all(isinstance(t, np.ndarray) for t in out)
    mc.assert_clean_equal(out, c["clean"][rule])
    wide = torch.full((c["faces"].shape[0], 7), -3, dtype=torch.int64, device=DEV)            # a strided int64 view
    wide[:, 1::2] = torch.tensor(c["faces"]).to(DEV)
    view = wide[:, 1::2]
    assert view.shape[0] == 0 or not view.is_contiguous()
    got = mesh.connected_components(view, c["V"])
    mc.assert_components_equal({k: (t.cpu().numpy() if isinstance(t, torch.Tensor) else t) for k, t in got.items()}, c["ref"])
    vwide = torch.zeros(c["V"], 6, device=DEV)
    vwide[:, ::2] = torch.tensor(c["vertices"]).to(DEV)
    with torch.cuda.stream(torch.cuda.Stream(device=DEV)):
        out = mesh.clean_mesh(vwide[:, ::2], view.to(torch.int32), *rule)
        torch.cuda.current_stream().synchronize()
    mc.assert_clean_equal(tuple(t.cpu().numpy() for t in out), c["clean"][rule])


def test_int64_indices_beyond_int32_stay_invalid():
    from sparsefusion_amd import mesh
    f = torch.tensor([[0, 1, 2], [0, 1, (1 << 32) + 2], [0, 1, -(1 << 32) + 1], [1, 2, 3]], dtype=torch.int64, device=DEV)
    got = mesh.connected_components(f, 4)
    assert got["face_label"].tolist() == [0, -1, -1, 0] and got["n_invalid"] == 2 and got["largest"] == 2


# --------------------------------------------------------------------------------------------------------------- 3. marching cubes
def test_marching_cubes_blobs_only_the_large_one_remains():
    from sparsefusion_amd import mesh
    v, f = mesh.marching_cubes(torch.from_numpy(mc.blob_volume()).to(DEV), 0.5)
    V = v.shape[0]
    fh, vh = f.cpu().numpy(), v.cpu().numpy()
    ref = mc.reference_components(fh, V)
    assert ref["n_components"] == 5 and ref["n_invalid"] == 0       # one large blob, one small blob, three specks
    sizes = np.sort(ref["faces_per_label"][ref["faces_per_label"] > 0])
    assert sizes[:3].tolist() == [8, 8, 8] and sizes[4] > 4 * sizes[3] > 4 * 8
    got = mesh.connected_components(f, V)
    mc.assert_components_equal({k: (t.cpu().numpy() if isinstance(t, torch.Tensor) else t) for k, t in got.items()}, ref)
    v2, f2, vi, fi = (t.cpu().numpy() for t in mesh.clean_mesh(v, f, min_faces=8, min_fraction=0.5))
    mc.assert_clean_equal((v2, f2, vi, fi), mc.reference_clean(vh, fh, V, ref, 8, 0.5))
    assert f2.shape[0] == int(sizes[4]) and np.array_equal(mc.bits(v2), mc.bits(vh[vi]))
    after = mc.reference_components(f2, v2.shape[0])
    assert after["n_components"] == 1 and not after["vertex_label"].any()
    closed, chi = mc.closed_and_euler(f2, v2.shape[0])
    assert closed and chi == 2
    assert bool((np.diff(vi) > 0).all()) and bool((np.diff(fi) > 0).all())
    keep8 = mesh.clean_mesh(v, f)                                   # the default: a speck's octahedron has exactly 8 faces and stays
    assert keep8[1].shape[0] == f.shape[0]
    assert mesh.clean_mesh(v, f, min_faces=9)[1].shape[0] == int(sizes[3] + sizes[4])


# ----------------------------------------------------------------------------------------------------------- 4. export_mesh_cleaned
@pytest.fixture(scope="module")
def teacher(golden_dir):
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    p = params_from_cfg(torch.load(f"{golden_dir}/ngp_render.pt")["teacher"]["cfg"])
    net = NeRFNetwork(get_default_torch_ngp_opt())
    net.load_state_dict({k: p[k] for k in net.state_dict().keys() if k in p})
    return net.to(DEV).eval()


def _read_ply(path):
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n") + len(b"end_header\n")].decode("ascii")
    V = int(head.split("element vertex ")[1].split("\n")[0])
    F = int(head.split("element face ")[1].split("\n")[0])
    vt = np.dtype([("xyz", "<f4", (3,)), ("n", "<f4", (3,)), ("rgb", "u1", (3,))])
    ft = np.dtype([("k", "u1"), ("idx", "<i4", (3,))])
    body = raw[len(head):]
    assert len(body) == V * vt.itemsize + F * ft.itemsize
    return head, np.frombuffer(body[:V * vt.itemsize], dtype=vt), np.frombuffer(body[V * vt.itemsize:], dtype=ft)


@pytest.mark.parametrize("min_faces,min_fraction,texture_size", [(8, 0.0, None), (8, 1.0, 512)])
def test_export_mesh_cleaned(teacher, tmp_path, min_faces, min_fraction, texture_size):
    from sparsefusion_amd import mesh
    net, R = teacher, 64
    d0, d1, d2 = (os.path.join(tmp_path, s) for s in "abc")
    v0, f0 = net.export_mesh(d0, resolution=R)
    _, _, c1, n1 = net.export_mesh_attributes(d1, resolution=R)
    vw, fc, cc, nc, vid = net.export_mesh_cleaned(d2, resolution=R, min_faces=min_faces, min_fraction=min_fraction,
                                                  texture_size=texture_size)
    want = mesh.clean_mesh(v0, f0, min_faces=min_faces, min_fraction=min_fraction)
    assert torch.equal(vw.view(torch.int32), want[0].view(torch.int32)) and torch.equal(fc, want[1]) and torch.equal(vid, want[2])
    assert fc.shape[0] > 100 and vid.dtype == torch.int32
    ids = vid.long()
    assert torch.equal(cc.view(torch.int32), c1[ids].view(torch.int32)) and torch.equal(nc.view(torch.int32), n1[ids].view(torch.int32))
    # every component of the result meets the rule, by scipy, against the components of the uncleaned mesh
    before = mc.reference_components(f0.cpu().numpy(), v0.shape[0])
    mc.assert_clean_equal(tuple(t.cpu().numpy() for t in want),
                          mc.reference_clean(v0.cpu().numpy(), f0.cpu().numpy(), v0.shape[0], before, min_faces, min_fraction))
    after = mc.reference_components(fc.cpu().numpy(), vw.shape[0])
    sizes = after["faces_per_label"][after["faces_per_label"] > 0]
    need = max(min_faces, int(np.ceil(np.float64(min_fraction) * before["largest"])))
    assert after["n_invalid"] == 0 and bool((sizes >= need).all()) and int(sizes.sum()) == fc.shape[0]
    assert bool((after["faces_per_label"][after["vertex_label"]] > 0).all())        # no unreferenced vertex is left
    print(f"teacher R={R}: {before['n_components']} components, F {f0.shape[0]} -> {fc.shape[0]}, V {v0.shape[0]} -> {vw.shape[0]}")
    # files
    vi = net._mesh_geometry(R)[0][ids].cpu().numpy()
    fw = fc.cpu().numpy()
    pv, pcol, pn, pf, pfn = pc.parse_obj_attrs(os.path.join(d2, "mcubes_mesh_clean.obj"))
    assert np.array_equal(pv.view(np.uint32), vi.view(np.uint32)) and np.array_equal(pf, fw) and np.array_equal(pfn, fw)
    assert np.array_equal(pcol.view(np.uint32), pc.bits(cc)) and np.array_equal(pn.view(np.uint32), pc.bits(nc))
    head, vrec, frec = _read_ply(os.path.join(d2, "mcubes_mesh_clean.ply"))
    assert head == mesh.ply_header(vw.shape[0], fw.shape[0], colors=True, normals=True)
    assert np.array_equal(vrec["xyz"].view(np.uint32), pc.bits(vw)) and np.array_equal(vrec["n"].view(np.uint32), pc.bits(nc))
    assert np.array_equal(vrec["rgb"], np.round(np.clip(cc.cpu().numpy().astype(np.float64), 0, 1) * 255).astype(np.uint8))
    assert (frec["k"] == 3).all() and np.array_equal(frec["idx"], fw)
    assert not os.path.exists(os.path.join(d2, "mcubes_mesh.obj"))
    if texture_size is None:
        assert not os.path.exists(os.path.join(d2, "mesh.obj")) and not os.path.exists(os.path.join(d2, "albedo.png"))
        return
    assert mesh.atlas_layout(fc.shape[0], texture_size)[1] >= mesh.atlas_layout(f0.shape[0], texture_size)[1]
    o = tc.parse_obj_textured(os.path.join(d2, "mesh.obj"))
    assert o["mtllib"] == "mesh.mtl" and np.array_equal(o["v"].view(np.uint32), pc.bits(vw)) and np.array_equal(o["f"], fw)
    assert np.array_equal(o["vn"].view(np.uint32), pc.bits(nc))
    assert np.array_equal(o["vt"].view(np.uint32).reshape(-1, 3, 2)[..., 0], mesh.atlas_uv(fc.shape[0], texture_size)[..., 0].view(np.uint32))
    assert open(os.path.join(d2, "mesh.mtl")).read() == mesh.MTL_TEXT
    assert tc.decode_png(open(os.path.join(d2, "albedo.png"), "rb").read()).shape == (texture_size, texture_size, 3)
