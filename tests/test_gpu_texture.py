"""GPU tests of the texture bake (sf_ngp_texture_bake, mesh.bake_texture) and of NeRFRenderer.export_mesh_textured.  The anchors are
bit-level: a texel's point is the numpy restatement of layout + clamp + weighted sum (tests/texture_common.py), its albedo is
net.density on that fp32 point, its bytes are the truncation rule.  Fields: `teacher` / `default_init` of tests/golden/ngp_render.pt.
Every output buffer is pre-filled with NaN / 0xFF, so an unwritten element fails the comparisons."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import texture_common as tc
from ngp_common import params_from_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("rgb8", "albedo", "xyz", "face_id")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_render.pt")


def _net(p):
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    net = NeRFNetwork(get_default_torch_ngp_opt())
    net.load_state_dict({k: p[k] for k in net.state_dict().keys() if k in p})
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def nets(golden):
    return {name: _net(params_from_cfg(golden[name]["cfg"])) for name in ("teacher", "default_init")}


def _launch(net, verts, faces, W, want=NAMES):
    """sf_ngp_texture_bake through the C ABI into pre-filled buffers; outputs not in `want` are passed as NULL"""
    from sparsefusion_amd import _lib
    v = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).to(DEV)
    f = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).to(DEV)
    out = {}
    if "rgb8" in want:
        out["rgb8"] = torch.full((W, W, 3), 255, dtype=torch.uint8, device=DEV)
    for k in ("albedo", "xyz"):
        if k in want:
            out[k] = torch.full((W, W, 3), float("nan"), dtype=torch.float32, device=DEV)
    if "face_id" in want:
        out["face_id"] = torch.full((W, W), -2 ** 31, dtype=torch.int32, device=DEV)
    params = [t.detach().contiguous() for t in net._field_params()]
    fld = net._field_handle().struct(params)
    rc = _lib.lib().sf_ngp_texture_bake(C.byref(fld), _lib.ptr(v), v.shape[0], _lib.ptr(f), f.shape[0], W,
                                        *[_lib.ptr(out.get(k)) for k in NAMES], _lib.stream_ptr())
    _lib.check(rc, "ngp_texture_bake")
    return out


def _check(net, verts, faces, W, got):
    """the equalities of the composition anchor on a full set of outputs"""
    face_id, xyz = tc.np_bake_points(verts, faces, W)
    used = face_id >= 0
    assert np.array_equal(got["face_id"].cpu().numpy(), face_id)
    assert np.array_equal(tc.bits(got["xyz"]), tc.bits(xyz))
    with torch.no_grad():
        want = net.density(got["xyz"].view(-1, 3))["albedo"].view(W, W, 3)
    albedo = got["albedo"].cpu().numpy()
    assert np.array_equal(tc.bits(albedo[used]), tc.bits(want.cpu().numpy()[used]))
    assert np.array_equal(got["rgb8"].cpu().numpy(), tc.np_quantise(albedo))
    assert (albedo[~used] == 0).all() and (got["rgb8"].cpu().numpy()[~used] == 0).all() and (xyz[~used] == 0).all()
    return used


# ------------------------------------------------------------------------------------------------------- 1. composition, bit-exact
@pytest.mark.parametrize("F,W", tc.SMALL_CASES)
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_bake_bit_equal_to_composed_density(nets, name, F, W):
    net = nets[name]
    verts, faces = tc.random_mesh(F)
    full = _launch(net, verts, faces, W)
    used = _check(net, verts, faces, W, full)
    assert set(np.unique(full["face_id"].cpu().numpy()[used])) == set(range(F))
    for skip in NAMES:                                               # every nullable output skipped in turn
        want = tuple(n for n in NAMES if n != skip)
        got = _launch(net, verts, faces, W, want)
        assert sorted(got) == sorted(want)
        for n in want:
            assert torch.equal(got[n].view(torch.uint8), full[n].view(torch.uint8)), (skip, n)


# ----------------------------------------------------------------------------------------------------------------- 2. grid-stride
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_bake_grid_stride(nets, name):
    """W = 725: 525 625 texels against the 2 048 x 256 threads of the capped grid, so the loop wraps once and ends on a tail.
    F = 5 000: G = 50, c = 14, 25 margin texels right of / below the cells."""
    verts, faces = tc.random_mesh(5000)
    assert tc.layout(5000, 725) == (50, 14)
    got = _launch(nets[name], verts, faces, 725)
    used = _check(nets[name], verts, faces, 725, got)
    assert used.sum() == 5000 * 14 * 14 // 2


def test_bake_texture_wrapper_and_argument_checks(nets):
    from sparsefusion_amd import mesh
    net = nets["teacher"]
    verts, faces = tc.random_mesh(7)
    v, f = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    full = _launch(net, verts, faces, 13)
    out = mesh.bake_texture(net, v, f, 13, albedo=True, xyz=True, face_id=True)
    for n in NAMES:
        assert out[n].shape == full[n].shape and torch.equal(out[n].view(torch.uint8), full[n].view(torch.uint8)), n
    assert sorted(mesh.bake_texture(net, v, f, 13)) == ["rgb8"]
    with pytest.raises(ValueError, match="smallest W is 12"):
        mesh.bake_texture(net, v, f, 11)
    with pytest.raises(ValueError):
        mesh.bake_texture(net, v, f, 13, rgb8=False)
    with pytest.raises(RuntimeError):
        mesh.bake_texture(net, v.cpu(), f, 13)
    empty = mesh.bake_texture(net, v, f[:0], 9, face_id=True)        # F == 0: every texel unused
    assert (empty["face_id"] == -1).all() and (empty["rgb8"] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ 3. end to end
def test_export_mesh_textured(golden, tmp_path):
    from sparsefusion_amd import mesh
    net = _net(params_from_cfg(golden["teacher"]["cfg"]))
    R, W = 64, 512
    d0, d1, d2, d3 = (os.path.join(tmp_path, s) for s in "pabc")
    v0, f0 = net.export_mesh(d0, resolution=R)
    v1, f1, uv, tex = net.export_mesh_textured(d1, resolution=R, texture_size=W)
    assert torch.equal(v1, v0) and torch.equal(f1, f0) and f1.shape[0] > 100
    V, F = v1.shape[0], f1.shape[0]
    assert tex.shape == (W, W, 3) and tex.dtype == torch.uint8 and uv.shape == (F, 3, 2) and uv.dtype == torch.float32
    assert np.array_equal(uv.cpu().numpy(), mesh.atlas_uv(F, W))
    assert sorted(os.listdir(d1)) == ["albedo.png", "mesh.mtl", "mesh.obj"]
    # the float albedo texel at a face corner's uv is the vertex colour of export_mesh_attributes: texel centre = corner, point = vertex
    _, _, colors, normals = net.export_mesh_attributes(d2, resolution=R)
    baked = mesh.bake_texture(net, v1, f1, W, albedo=True, xyz=True, face_id=True)
    assert torch.equal(baked["rgb8"], tex)
    xy = np.rint(uv.cpu().numpy().astype(np.float64) * W - 0.5).astype(np.int64)            # [F, 3, 2] texel (x, y)
    assert np.array_equal(xy, tc.corner_texels(F, W))
    ys, xs = torch.from_numpy(xy[..., 1]).to(DEV), torch.from_numpy(xy[..., 0]).to(DEV)
    fl = f1.long()
    assert torch.equal(baked["face_id"][ys, xs], torch.arange(F, dtype=torch.int32, device=DEV)[:, None].expand(F, 3))
    assert np.array_equal(tc.bits(baked["xyz"][ys, xs]), tc.bits(v1[fl]))
    assert np.array_equal(tc.bits(baked["albedo"][ys, xs]), tc.bits(colors[fl]))
    _check(net, v1.cpu().numpy(), f1.cpu().numpy(), W, baked)
    assert len(np.unique(tex.cpu().numpy().reshape(-1, 3), axis=0)) > 100
    # files
    assert np.array_equal(tc.decode_png(open(os.path.join(d1, "albedo.png"), "rb").read()), tex.cpu().numpy())
    assert open(os.path.join(d1, "mesh.mtl")).read() == mesh.MTL_TEXT
    o = tc.parse_obj_textured(os.path.join(d1, "mesh.obj"))
    assert o["mtllib"] == "mesh.mtl" and o["usemtl"] == "mat0" and o["order"] == ["mtllib", "v", "vt", "vn", "usemtl", "f"]
    assert o["v"].shape == (V, 3) and o["vt"].shape == (3 * F, 2) and o["vn"].shape == (V, 3) and o["f"].shape == (F, 3)
    assert np.array_equal(o["v"].view(np.uint32), tc.bits(v1)) and np.array_equal(o["f"], f1.cpu().numpy())
    assert np.array_equal(o["vn"].view(np.uint32), tc.bits(normals)) and np.array_equal(o["fn"], o["f"])
    assert o["f"].min() >= 0 and o["f"].max() < V and np.array_equal(o["ft"], np.arange(3 * F).reshape(F, 3))
    uvn = uv.cpu().numpy()
    want_vt = np.stack([uvn[..., 0], np.float32(1.0) - uvn[..., 1]], -1).reshape(-1, 2)
    assert np.array_equal(o["vt"].view(np.uint32), want_vt.view(np.uint32))
    # without normals: no vn lines, the same texture
    _, _, _, tex3 = net.export_mesh_textured(d3, resolution=R, texture_size=W, normals=False)
    o3 = tc.parse_obj_textured(os.path.join(d3, "mesh.obj"))
    assert torch.equal(tex3, tex) and o3["vn"] is None and o3["fn"] is None and np.array_equal(o3["ft"], o["ft"])
    with pytest.raises(ValueError, match="smallest W"):
        net.export_mesh_textured(d3, resolution=R, texture_size=64)
