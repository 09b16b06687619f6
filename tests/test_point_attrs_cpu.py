"""CPU tests of the point attributes (sigma, albedo, finite-difference gradient, normal) and of the mesh writers that carry them:
the per-point device function of k_ngp_point_attrs (sparsefusion_amd/csrc/ngp_point_attrs.h) run thread by thread against the
oracle and against its own single evaluations, the OBJ / PLY writers, and the C ABI's argument checks.  No GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import mesh_ref
import point_attrs_common as pc
from ngp_common import BOUND, params_from_cfg

N_UNIFORM = 2000


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_render.pt")


@pytest.fixture(scope="module")
def cases(golden):
    """(field, eps) -> (params, points, emulated kernel outputs, oracle) -- computed once, shared, never modified"""
    x = pc.points(N_UNIFORM)
    out = {}
    for name in ("teacher", "default_init"):
        p = params_from_cfg(golden[name]["cfg"])
        for eps in pc.EPSILONS:
            out[name, eps] = (p, x, pc.emu_point_attrs(p, x, eps), pc.oracle_attrs(p, x, eps))
    return out


# ------------------------------------------------------------------------------------------------- 1. kernel logic vs the oracle
@pytest.mark.parametrize("eps", pc.EPSILONS)
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_emulated_kernel_against_oracle(cases, name, eps):
    """Centre sigma / albedo within the tolerances of test_density_matches_oracle; each gradient component within the bound those
    tolerances imply for 0.5 * (sp - sn) / eps, plus 4 ulp of the reference value.  The points run over three emulated
    workgroups, so the grid-stride loop makes three rounds and ends on a tail; every output element is written."""
    p, x, got, ref = cases[name, eps]
    assert x.shape[0] == N_UNIFORM + 12
    for k in ("sigma", "albedo", "grad", "normal"):
        assert not torch.isnan(got[k]).any(), k
    assert torch.allclose(got["sigma"], ref["sigma"], rtol=pc.SIGMA_RTOL, atol=pc.SIGMA_ATOL)
    assert torch.allclose(got["albedo"], ref["albedo"], rtol=pc.SIGMA_RTOL, atol=pc.ALBEDO_ATOL)
    err = np.abs(got["grad"].double().numpy() - ref["grad"].double().numpy())
    bound = pc.grad_bound(ref, eps)
    worst = float((err / bound).max())
    print(f"{name} eps={eps:.5f}: max |grad err| / bound = {worst:.3f}, max |grad| = {float(ref['grad'].abs().max()):.3e}")
    assert (err <= bound).all(), worst


# --------------------------------------------------------------------------------------------------- 2. normals vs the oracle
@pytest.mark.parametrize("eps", pc.EPSILONS)
def test_emulated_normals_against_oracle(cases, eps):
    """r = |bound vector| / |reference gradient| per point; where r <= 5e-2 the normals agree within 2 r + 1e-6 (a perturbation d
    of g moves g / |g| by at most 2 |d| / |g|); at most 0.5 % of the points fall outside the compared set."""
    from sparsefusion_amd.nerf.utils import safe_normalize
    p, x, got, ref = cases["teacher", eps]
    n_ref = safe_normalize(ref["grad"])
    n_ref[torch.isnan(n_ref)] = 0
    with np.errstate(divide="ignore"):
        r = np.linalg.norm(pc.grad_bound(ref, eps), axis=1) / np.linalg.norm(ref["grad"].double().numpy(), axis=1)
    keep = r <= 5e-2
    out_share = 1.0 - keep.mean()
    d = np.linalg.norm(got["normal"].double().numpy() - n_ref.double().numpy(), axis=1)
    print(f"eps={eps:.5f}: {100 * out_share:.2f} % outside the compared set, max (|n - n_ref| / (2 r + 1e-6)) = "
          f"{float((d[keep] / (2 * r[keep] + 1e-6)).max()):.3f}")
    assert out_share <= 0.005
    assert (d[keep] <= 2 * r[keep] + 1e-6).all()
    length = np.linalg.norm(got["normal"].double().numpy(), axis=1)
    assert (np.abs(length[keep] - 1.0) <= 1e-6).all()


# ------------------------------------------------------------------------- bit-level anchor of the composition, on the emulation
@pytest.mark.parametrize("eps", pc.EPSILONS)
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_emulated_kernel_is_its_own_single_evaluations(cases, name, eps):
    """The seven evaluations inside the loop are the single evaluation: sigma / albedo bit-equal to a centre-only run, the gradient
    bit-equal to 0.5f * (sp - sn) / eps of centre-only runs on the clamped fp32 offset points, the normal bit-equal to the numpy
    float32 restatement.  Null outputs leave the others unchanged."""
    p, x, got, _ = cases[name, eps]
    centre = pc.emu_point_attrs(p, x, eps, blocks=2, grad=False, normal=False)
    assert centre["grad"] is None and centre["normal"] is None
    assert np.array_equal(pc.bits(centre["sigma"]), pc.bits(got["sigma"]))
    assert np.array_equal(pc.bits(centre["albedo"]), pc.bits(got["albedo"]))
    side = {}
    for sign in (1.0, -1.0):
        side[sign] = np.stack([pc.emu_point_attrs(p, pc.offset_points(x, np.float32(eps).item(), a, sign), eps, blocks=5, albedo=False,
                                                  grad=False, normal=False)["sigma"].numpy() for a in range(3)], -1)
    g = pc.np_grad(side[1.0], side[-1.0], eps)
    assert np.array_equal(pc.bits(g), pc.bits(got["grad"]))
    assert np.array_equal(pc.bits(pc.np_normal(got["grad"].numpy())), pc.bits(got["normal"]))
    only_n = pc.emu_point_attrs(p, x, eps, blocks=1, sigma=False, albedo=False, grad=False)
    assert np.array_equal(pc.bits(only_n["normal"]), pc.bits(got["normal"]))


def test_normal_formula_special_values():
    """safe_normalize's floor and the NaN rule on the restatement the GPU test compares with: a zero gradient gives a zero normal,
    an infinite component gives 0 there (inf / inf) and 0 elsewhere, NaN gives 0."""
    g = np.array([[0, 0, 0], [3, 0, 4], [np.inf, 1, 0], [np.nan, 0, 0], [1e-30, 0, 0]], dtype=np.float32)
    n = pc.np_normal(g)
    assert np.array_equal(n[0], [0, 0, 0]) and np.allclose(n[1], [0.6, 0, 0.8], rtol=1e-7)
    assert np.array_equal(n[2], [0, 0, 0]) and n[3][0] == 0
    assert n[4][0] == np.float32(1e-30) / np.sqrt(np.float32(1e-20))


# ------------------------------------------------------------------------------------------------------------------ 3. writers
def _small_mesh():
    rng = np.random.default_rng(4)
    v = (rng.standard_normal((37, 3)) * np.array([1e-3, 10.0, 3e4])).astype(np.float32)
    v[0] = [0.0, 1.0, 127.0]
    v[1] = np.nextafter(np.float32(1.0), np.float32(2.0))
    f = rng.integers(0, 37, (61, 3)).astype(np.int32)
    c = rng.random((37, 3)).astype(np.float32)
    c[0], c[1] = [0.0, 1.0, 0.5], np.nextafter(np.float32(1.0), np.float32(0.0))
    n = rng.standard_normal((37, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[2] = 0.0
    return v, f, c, n.astype(np.float32)


def test_export_obj_plain_bytes_unchanged(tmp_path):
    from sparsefusion_amd.mesh import export_obj
    v, f, _, _ = _small_mesh()
    path = os.path.join(tmp_path, "m.obj")
    export_obj(v, f, path)
    assert open(path, "rb").read() == pc.plain_obj_bytes(v, f)
    export_obj(torch.from_numpy(v), torch.from_numpy(f), path, colors=None, normals=None)
    assert open(path, "rb").read() == pc.plain_obj_bytes(v, f)
    pv, pf = mesh_ref.parse_obj(path)
    assert np.array_equal(pv.view(np.uint32), v.view(np.uint32)) and np.array_equal(pf, f)


@pytest.mark.parametrize("with_c,with_n", [(True, True), (True, False), (False, True)])
def test_export_obj_attributes_round_trip(tmp_path, with_c, with_n):
    from sparsefusion_amd.mesh import export_obj
    v, f, c, n = _small_mesh()
    a, b = os.path.join(tmp_path, "a.obj"), os.path.join(tmp_path, "b.obj")
    export_obj(v, f, a, colors=c if with_c else None, normals=n if with_n else None)
    export_obj(torch.from_numpy(v), torch.from_numpy(f), b, colors=torch.from_numpy(c) if with_c else None,
               normals=torch.from_numpy(n) if with_n else None)
    assert open(a, "rb").read() == open(b, "rb").read()
    pv, pc_, pn, pf, pfn = pc.parse_obj_attrs(a)
    assert np.array_equal(pv.view(np.uint32), v.view(np.uint32)) and np.array_equal(pf, f)
    if with_c:
        assert np.array_equal(pc_.view(np.uint32), c.view(np.uint32))
        assert float(pc_.min()) >= 0.0 and float(pc_.max()) <= 1.0
    else:
        assert pc_ is None
    if with_n:
        assert np.array_equal(pn.view(np.uint32), n.view(np.uint32)) and np.array_equal(pfn, f)
    else:
        assert pn is None and pfn is None
    lines = open(a).read().splitlines()
    assert len(lines) == 37 * (2 if with_n else 1) + 61
    with pytest.raises(ValueError):
        export_obj(v, f, a, colors=c[:5])


def test_export_obj_colours_are_clipped(tmp_path):
    from sparsefusion_amd.mesh import export_obj
    v = np.zeros((2, 3), np.float32)
    path = os.path.join(tmp_path, "c.obj")
    export_obj(v, np.zeros((0, 3), np.int32), path, colors=np.array([[-0.5, 0.25, 1.5], [0, 1, 2]], np.float32))
    assert open(path).read() == "v 0 0 0 0 0.25 1\nv 0 0 0 0 1 1\n"


@pytest.mark.parametrize("with_c,with_n", [(True, True), (True, False), (False, True), (False, False)])
def test_export_ply_round_trip(tmp_path, with_c, with_n):
    from sparsefusion_amd.mesh import export_ply
    v, f, c, n = _small_mesh()
    a, b = os.path.join(tmp_path, "a.ply"), os.path.join(tmp_path, "b.ply")
    export_ply(v, f, a, colors=c if with_c else None, normals=n if with_n else None)
    export_ply(torch.from_numpy(v), torch.from_numpy(f), b, colors=torch.from_numpy(c) if with_c else None,
               normals=torch.from_numpy(n) if with_n else None)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    want = "ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\nproperty float y\nproperty float z\n"
    if with_n:
        want += "property float nx\nproperty float ny\nproperty float nz\n"
    if with_c:
        want += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    want += "element face 61\nproperty list uchar int vertex_indices\nend_header\n"
    assert raw.startswith(want.encode("ascii"))
    body = raw[len(want):]
    vsize = 12 + (12 if with_n else 0) + (3 if with_c else 0)
    assert len(body) == 37 * vsize + 61 * 13
    vt = [("xyz", "<f4", (3,))] + ([("n", "<f4", (3,))] if with_n else []) + ([("rgb", "u1", (3,))] if with_c else [])
    rec = np.frombuffer(body[:37 * vsize], dtype=np.dtype(vt))
    assert np.array_equal(rec["xyz"].view(np.uint32), v.view(np.uint32))
    if with_n:
        assert np.array_equal(rec["n"].view(np.uint32), n.view(np.uint32))
    if with_c:
        assert np.array_equal(rec["rgb"], np.round(np.clip(c.astype(np.float64), 0, 1) * 255).astype(np.uint8))
        assert tuple(rec["rgb"][0]) == (0, 255, 128)
    frec = np.frombuffer(body[37 * vsize:], dtype=np.dtype([("k", "u1"), ("idx", "<i4", (3,))]))
    assert (frec["k"] == 3).all() and np.array_equal(frec["idx"], f)


def test_export_ply_colour_rounding(tmp_path):
    from sparsefusion_amd.mesh import export_ply, ply_header
    c = np.array([[0.0, 1.0, 0.5], [-3.0, 7.0, np.nan], [0.25, 0.999, 1 / 255], [0.5 / 255 + 1e-4, 0.5 / 255 - 1e-4, 254.4 / 255]],
                 dtype=np.float32)
    path = os.path.join(tmp_path, "c.ply")
    export_ply(np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32), path, colors=c)
    raw = open(path, "rb").read()
    head = ply_header(4, 0, colors=True)
    assert raw.startswith(head.encode()) and "element face 0\n" in head
    rec = np.frombuffer(raw[len(head):], dtype=np.dtype([("xyz", "<f4", (3,)), ("rgb", "u1", (3,))]))
    assert rec["rgb"].tolist() == [[0, 255, 128], [0, 255, 0], [64, 255, 1], [1, 0, 254]]


def test_export_ply_empty(tmp_path):
    from sparsefusion_amd.mesh import export_ply, ply_header
    path = os.path.join(tmp_path, "e.ply")
    export_ply(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), path)
    assert open(path, "rb").read() == ply_header(0, 0).encode()


# -------------------------------------------------------------------------------------------------------------------- 4. C ABI
def test_point_attrs_abi_argument_checks():
    """The symbol is in the built library under the declared signature; the argument checks run before any device call, so they
    answer on a machine without a GPU: null field or points, no output, a bad epsilon -> SF_ERR_INVALID; P == 0 -> SF_OK."""
    from sparsefusion_amd import _lib
    res, args = _lib.SIGNATURES["sf_ngp_point_attrs"]
    assert res is C.c_int and len(args) == 9 and args[0] is C.POINTER(_lib.SfNgpField) and args[2] is C.c_uint32 and args[3] is C.c_float
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparsefusion_hip.h")).read()
    assert "int sf_ngp_point_attrs(const sf_ngp_field* f, const float* xyz, uint32_t P, float epsilon," in header
    lib = _lib.lib()
    fn = lib.sf_ngp_point_attrs
    f = _lib.SfNgpField()
    xyz = (C.c_float * 3)(0.0, 0.0, 0.0)
    out = (C.c_float * 3)()
    px, po = C.cast(xyz, C.c_void_p), C.cast(out, C.c_void_p)
    OK, INVALID = 0, 1
    assert fn(None, px, 1, 1e-2, po, None, None, None, None) == INVALID
    assert b"null" in lib.sf_last_error()
    assert fn(C.byref(f), None, 1, 1e-2, po, None, None, None, None) == INVALID
    assert fn(C.byref(f), px, 1, 1e-2, None, None, None, None, None) == INVALID
    assert b"output" in lib.sf_last_error()
    for eps in (0.0, -1e-2, float("inf"), float("nan")):
        assert fn(C.byref(f), px, 1, eps, po, None, None, None, None) == INVALID, eps
        assert b"epsilon" in lib.sf_last_error()
    assert fn(C.byref(f), px, 0, 1e-2, None, None, po, None, None) == OK
    assert fn(C.byref(f), px, 0, 1e-2, None, None, None, None, None) == INVALID      # the checks come before P == 0


# -------------------------------------------------------------------------------------------------------------- public surface
def test_public_surface():
    from sparsefusion_amd import mesh
    from sparsefusion_amd.nerf import NeRFNetwork, NeRFRenderer
    from sparsefusion_amd.nerf import utils
    assert list(inspect.signature(utils.safe_normalize).parameters) == ["x", "eps"]
    assert inspect.signature(utils.safe_normalize).parameters["eps"].default == 1e-20
    sig = inspect.signature(NeRFNetwork.finite_difference_normal)
    assert list(sig.parameters) == ["self", "x", "epsilon"] and sig.parameters["epsilon"].default == 1e-2
    sig = inspect.signature(NeRFNetwork.normal)
    assert list(sig.parameters) == ["self", "x", "smooth"] and sig.parameters["smooth"].default is False
    assert list(inspect.signature(NeRFNetwork.forward).parameters) == ["self", "x", "d", "l", "ratio", "shading"]
    assert list(inspect.signature(mesh.vertex_attributes).parameters) == ["net", "vertices_world", "epsilon"]
    for fn in (mesh.export_obj, mesh.export_ply):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["vertices", "faces", "filename", "colors", "normals"]
        assert sig.parameters["colors"].default is None and sig.parameters["normals"].default is None
    sig = inspect.signature(NeRFRenderer.export_mesh_attributes)
    assert list(sig.parameters) == ["self", "path", "resolution", "S", "epsilon"] and sig.parameters["epsilon"].default is None
    x = torch.tensor([[3.0, 0.0, 4.0], [0.0, 0.0, 0.0]])
    assert torch.equal(utils.safe_normalize(x), torch.tensor([[0.6, 0.0, 0.8], [0.0, 0.0, 0.0]]))


def test_smooth_and_unsupported_shadings_raise_without_a_gpu():
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    net = NeRFNetwork(get_default_torch_ngp_opt())
    x = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="rand_like"):
        net.normal(x, smooth=True)
    for shading in ("normal", "textureless"):
        with pytest.raises(NotImplementedError, match="smooth normal"):
            net(x, None, l=torch.tensor([0.0, 0.0, 1.0]), ratio=0.5, shading=shading)
    with pytest.raises(RuntimeError):                          # no CPU path for the fused route
        with torch.no_grad():
            net.normal(x)
