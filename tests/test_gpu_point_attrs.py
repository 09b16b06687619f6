"""GPU tests of the point attributes (sf_ngp_point_attrs: sigma, albedo, finite-difference gradient and normal in one launch), of
NeRFNetwork.finite_difference_normal / normal / forward(shading='lambertian') and of export_mesh_attributes.  The anchors are
bit-level: every one of the kernel's seven evaluations is net.density on that fp32 point, and the gradient / normal are the numpy
float32 restatement of their formulas on those values.  Fields: `teacher` / `default_init` of tests/golden/ngp_render.pt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import point_attrs_common as pc
from ngp_common import BOUND, params_from_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("sigma", "albedo", "grad", "normal")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_render.pt")


def _net(p, cuda_ray=False):
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    opt = get_default_torch_ngp_opt()
    opt.cuda_ray = cuda_ray
    net = NeRFNetwork(opt)
    net.load_state_dict({k: p[k] for k in net.state_dict().keys() if k in p}, strict=not cuda_ray)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def nets(golden):
    return {name: _net(params_from_cfg(golden[name]["cfg"])) for name in ("teacher", "default_init")}


def _launch(net, x, eps, want=NAMES):
    """sf_ngp_point_attrs through the C ABI into NaN-filled buffers (an unwritten element fails the comparisons); outputs not in
    `want` are passed as NULL"""
    from sparsefusion_amd import _lib
    P = x.shape[0]
    out = {k: torch.full((P,) if k == "sigma" else (P, 3), float("nan"), dtype=torch.float32, device=DEV) for k in want}
    params = [t.detach().contiguous() for t in net._field_params()]
    f = net._field_handle().struct(params)
    rc = _lib.lib().sf_ngp_point_attrs(C.byref(f), _lib.ptr(x), P, float(np.float32(eps)), *[_lib.ptr(out.get(k)) for k in NAMES],
                                       _lib.stream_ptr())
    _lib.check(rc, "ngp_point_attrs")
    return out


def _composed(net, x, eps):
    """the same quantities from net.density: centre, then the six clamped fp32 offset points, combined in numpy float32"""
    with torch.no_grad():
        c = net.density(x)
        sp = np.stack([net.density(pc.offset_points(x, eps, a, 1.0))["sigma"].cpu().numpy() for a in range(3)], -1)
        sn = np.stack([net.density(pc.offset_points(x, eps, a, -1.0))["sigma"].cpu().numpy() for a in range(3)], -1)
    g = pc.np_grad(sp, sn, eps)
    return dict(sigma=c["sigma"].cpu().numpy(), albedo=c["albedo"].cpu().numpy(), grad=g, normal=pc.np_normal(g), sp=sp, sn=sn)


# ---------------------------------------------------------------------------------------------------- 5. composition anchor
@pytest.mark.parametrize("P", [1, 255, 256, 257, 524288 + 300])
@pytest.mark.parametrize("eps", pc.EPSILONS)
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_point_attrs_bit_equal_to_composed_density(nets, name, eps, P):
    """P = 524 588 is one tail past the 2 048 x 256 threads of the capped grid: the grid-stride loop runs twice."""
    net = nets[name]
    x = pc.spliced_points(P).to(DEV)
    got = _launch(net, x, eps)
    want = _composed(net, x, eps)
    for k in NAMES:
        assert np.array_equal(pc.bits(got[k]), pc.bits(want[k])), k
    if P > 1000:
        n = got["normal"].cpu().numpy().astype(np.float64)
        length = np.linalg.norm(n, axis=1)
        assert ((np.abs(length - 1.0) <= 1e-6) | (length == 0.0)).all()
        assert float((length > 0).mean()) > 0.9


@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_point_attrs_null_outputs(nets, name):
    """every combination of NULL outputs but the empty one, once: the outputs that are asked for do not change"""
    net, eps = nets[name], pc.EPSILONS[1]
    x = pc.spliced_points(257).to(DEV)
    full = _launch(net, x, eps)
    for mask in range(1, 15):
        want = [k for i, k in enumerate(NAMES) if mask >> i & 1]
        got = _launch(net, x, eps, want)
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(pc.bits(got[k]), pc.bits(full[k])), (mask, k)


def test_point_attributes_wrapper_and_argument_checks(nets):
    from sparsefusion_amd import mesh
    net = nets["teacher"]
    x = pc.spliced_points(300).to(DEV)
    full = _launch(net, x, 1e-2)
    out = mesh.point_attributes(net, x, 1e-2)
    for k in NAMES:
        assert np.array_equal(pc.bits(out[k]), pc.bits(full[k])), k
    assert sorted(mesh.point_attributes(net, x, 1e-2, sigma=False, grad=False)) == ["albedo", "normal"]
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            mesh.point_attributes(net, x, bad)
    with pytest.raises(ValueError):
        mesh.point_attributes(net, x, 1e-2, sigma=False, albedo=False, grad=False, normal=False)
    with pytest.raises(RuntimeError):
        mesh.point_attributes(net, x.cpu(), 1e-2)
    assert mesh.point_attributes(net, x[:0], 1e-2)["grad"].shape == (0, 3)


# ------------------------------------------------------------------------------------------------------------- 6. field API
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_field_normal_api_without_gradient(nets, name):
    from sparsefusion_amd.nerf.utils import safe_normalize
    net = nets[name]
    x = pc.points(2000).to(DEV)
    k1 = _launch(net, x, 1e-2)
    with torch.no_grad():
        g, n = net.finite_difference_normal(x), net.normal(x)
        assert torch.equal(g, k1["grad"]) and torch.equal(n, k1["normal"])
        g2 = net.finite_difference_normal(x.view(4, 503, 3), epsilon=pc.EPSILONS[1])
        assert g2.shape == (4, 503, 3) and torch.equal(g2.view(-1, 3), _launch(net, x, pc.EPSILONS[1])["grad"])
        t = safe_normalize(g)
        t[torch.isnan(t)] = 0
        assert float((t - n).abs().max()) <= 5e-7                  # the torch formula on the kernel's gradient: a few ulp of 1
        light = torch.tensor([0.3, -0.5, 0.8], device=DEV)
        light = light / light.norm()
        for ratio in (0.1, 1):
            sigma, color, normal = net(x, None, l=light, ratio=ratio, shading='lambertian')
            assert torch.equal(sigma, k1["sigma"]) and torch.equal(normal, k1["normal"])
            assert torch.equal(color, k1["albedo"] * (ratio + (1 - ratio) * (k1["normal"] @ -light).clamp(min=0)).unsqueeze(-1))
        s0, c0, n0 = net(x, None, shading='albedo')
        assert n0 is None and torch.equal(s0, k1["sigma"]) and torch.equal(c0, k1["albedo"])
        with pytest.raises(NotImplementedError):
            net.normal(x, smooth=True)
        for shading in ("normal", "textureless"):
            with pytest.raises(NotImplementedError):
                net(x, None, l=light, ratio=0.5, shading=shading)
        with pytest.raises(ValueError):
            net(x, None, l=None, ratio=0.5, shading='lambertian')


@pytest.mark.parametrize("eps", pc.EPSILONS)
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_field_normal_api_composed_route_with_gradient(golden, name, eps):
    """With gradients enabled the six differentiable common_forward calls agree with the fused launch: each sigma within the density
    tolerances (rtol 2e-5, atol 1e-7), so each gradient component within ((2e-5 |sp| + 1e-7) + (2e-5 |sn| + 1e-7)) * 0.5 / eps
    plus 4 ulp; on the teacher, normals within 2 r + 1e-6 where r = |bound| / |gradient| <= 5e-2 (at most 0.5 % fall out)."""
    net = _net(params_from_cfg(golden[name]["cfg"])).train()
    x = pc.points(2000).to(DEV)
    fused = _composed(net, x, eps)
    g = net.finite_difference_normal(x, epsilon=eps)
    assert g.requires_grad and g.shape == (2012, 3)
    ref = {k: torch.from_numpy(fused[k]) for k in ("sp", "sn", "grad")}
    bound = pc.grad_bound(ref, eps)
    err = np.abs(g.detach().cpu().double().numpy() - fused["grad"].astype(np.float64))
    print(f"{name} eps={eps:.5f}: composed vs fused max |grad err| / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    g.sum().backward()
    assert float(net.encoder.embeddings.grad.abs().sum()) > 0
    if name == "teacher" and eps == 1e-2:
        n = net.normal(x)
        light = torch.tensor([0.0, 0.6, 0.8], device=DEV)
        sigma, color, n2 = net(x, None, l=light, ratio=0.3, shading='lambertian')
        assert n.requires_grad and color.requires_grad and torch.equal(n, n2)
        with np.errstate(divide="ignore"):
            r = np.linalg.norm(bound, axis=1) / np.linalg.norm(fused["grad"].astype(np.float64), axis=1)
        keep = r <= 5e-2
        d = np.linalg.norm(n.detach().cpu().double().numpy() - fused["normal"].astype(np.float64), axis=1)
        assert 1.0 - keep.mean() <= 0.005
        assert (d[keep] <= 2 * r[keep] + 1e-6).all()
        assert torch.allclose(sigma.detach().cpu(), torch.from_numpy(fused["sigma"]), rtol=pc.SIGMA_RTOL, atol=pc.SIGMA_ATOL)


# ------------------------------------------------------------------------------------------------------------ 7. mesh export
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


def _outward_share(v, f, n):
    """share of faces whose geometric normal (b - a) x (c - a) has a positive dot product with the mean of its vertex normals"""
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    return float((np.einsum("ij,ij->i", np.cross(b - a, c - a), n[f].astype(np.float64).mean(axis=1)) > 0).mean())


@pytest.mark.parametrize("cuda_ray", [False, True])
def test_export_mesh_attributes(golden, tmp_path, cuda_ray):
    from sparsefusion_amd import mesh
    from sparsefusion_amd.nerf.utils import safe_normalize
    p = params_from_cfg(golden["teacher"]["cfg"])
    net = _net(p, cuda_ray=cuda_ray)
    R = 64
    d0, d1, d2 = (os.path.join(tmp_path, s) for s in "pab")
    v0, f0 = net.export_mesh(d0, resolution=R)
    v1, f1, c1, n1 = net.export_mesh_attributes(d1, resolution=R)
    v2, f2, c2, n2 = net.export_mesh_attributes(d2, resolution=R)
    assert torch.equal(v1, v0) and torch.equal(f1, f0) and f1.shape[0] > 100
    assert all(torch.equal(a, b) for a, b in ((v1, v2), (f1, f2), (c1, c2), (n1, n2)))
    for name in ("mcubes_mesh.obj", "mcubes_mesh.ply"):
        assert open(os.path.join(d1, name), "rb").read() == open(os.path.join(d2, name), "rb").read()
    assert not os.path.exists(os.path.join(d0, "mcubes_mesh.ply"))
    # geometry-only export: the bytes of the formatting rule it had before colours and normals existed
    sm, stats = mesh.smooth_gaussian(mesh.density_lattice(net, R, BOUND), sigma=1.5, return_stats=True)
    mean, std = (float(s) for s in stats.cpu())
    vi, fi = mesh.marching_cubes(sm, mean + std * 0.25)
    vi, fi = vi.cpu().numpy(), fi.cpu().numpy()
    assert open(os.path.join(d0, "mcubes_mesh.obj"), "rb").read() == pc.plain_obj_bytes(vi, fi)
    # attributes: albedo of the field at the vertices, unit or zero normals, one lattice spacing as epsilon
    assert c1.dtype == torch.float32 and n1.dtype == torch.float32 and c1.shape == v1.shape and n1.shape == v1.shape
    with torch.no_grad():
        assert torch.equal(c1, net.density(v1)["albedo"])
    eps = 2.0 * BOUND / (R - 1)
    k = _launch(net, v1.contiguous(), eps)
    assert torch.equal(n1, -k["normal"] + 0.0)
    length = n1.double().norm(dim=1).cpu().numpy()
    assert ((np.abs(length - 1.0) <= 1e-6) | (length == 0.0)).all()
    _, _, c3, n3 = net.export_mesh_attributes(os.path.join(tmp_path, "c"), resolution=R, epsilon=1e-2)
    assert torch.equal(c3, c1) and torch.equal(n3, -_launch(net, v1.contiguous(), 1e-2)["normal"] + 0.0)
    # orientation against the oracle's normals at the same vertices
    vw, fw, nw = v1.cpu().numpy(), f1.cpu().numpy(), n1.cpu().numpy()
    ref = pc.oracle_attrs(p, v1.cpu(), float(np.float32(eps)))
    n_ref = -safe_normalize(ref["grad"])
    n_ref[torch.isnan(n_ref)] = 0
    share, share_ref = _outward_share(vw, fw, nw), _outward_share(vw, fw, n_ref.numpy())
    print(f"cuda_ray={cuda_ray}: V={vw.shape[0]} F={fw.shape[0]} outward share {share:.4f} (oracle normals {share_ref:.4f})")
    assert share > 0.5 and abs(share - share_ref) <= 0.02
    # files
    pv, pcol, pn, pf, pfn = pc.parse_obj_attrs(os.path.join(d1, "mcubes_mesh.obj"))
    assert np.array_equal(pv.view(np.uint32), vi.view(np.uint32)) and np.array_equal(pf, fw) and np.array_equal(pfn, fw)
    assert np.array_equal(pcol.view(np.uint32), pc.bits(c1)) and np.array_equal(pn.view(np.uint32), pc.bits(n1))
    head, vrec, frec = _read_ply(os.path.join(d1, "mcubes_mesh.ply"))
    assert head == mesh.ply_header(vw.shape[0], fw.shape[0], colors=True, normals=True)
    assert np.array_equal(vrec["xyz"].view(np.uint32), pc.bits(v1)) and np.array_equal(vrec["n"].view(np.uint32), pc.bits(n1))
    assert np.array_equal(vrec["rgb"], np.round(np.clip(c1.cpu().numpy().astype(np.float64), 0, 1) * 255).astype(np.uint8))
    assert (frec["k"] == 3).all() and np.array_equal(frec["idx"], fw)


def test_vertex_attributes_numpy_in_numpy_out(nets):
    from sparsefusion_amd import mesh
    net = nets["teacher"]
    x = pc.points(100)
    c, n = mesh.vertex_attributes(net, x.numpy(), 1e-2)
    k = _launch(net, x.to(DEV), 1e-2)
    assert isinstance(c, np.ndarray) and isinstance(n, np.ndarray)
    assert np.array_equal(pc.bits(c), pc.bits(k["albedo"])) and np.array_equal(pc.bits(n), pc.bits(-k["normal"] + 0.0))
    c0, n0 = mesh.vertex_attributes(net, torch.empty(0, 3, device=DEV), 1e-2)
    assert c0.shape == (0, 3) and n0.shape == (0, 3)
