"""GPU test of the matrix-core field forward (sparsefusion_amd/csrc/ngp_field_mfma.h) against the lane-per-point k_ngp_field it
replaces as the default: the f32 MFMA is a k-ordered fmaf chain from the bias, so the two kernels must give the SAME bits --
the render, every per-sample workspace row and the field cache are compared with torch.equal; the parameter gradients (the
backward's atomics) agree to summation order, the rule of test_gpu_ngp.py::test_field_cache_equals_regather."""
import ctypes as C

import pytest
import torch

from oracle import ngp_ref
from ngp_common import params_from_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 64


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_render.pt")


@pytest.fixture(scope="module")
def scene(golden):
    """Teacher field, circle_rays(8) = 64 rays, injected jitter, one fixed upstream gradient."""
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    p = params_from_cfg(golden["teacher"]["cfg"])
    net = NeRFNetwork(get_default_torch_ngp_opt())
    net.load_state_dict({k: p[k] for k in net.state_dict().keys()})
    net = net.to(DEV).train()
    o, d = ngp_ref.circle_rays(8, view=3)
    g = torch.Generator().manual_seed(5)
    N = o.shape[0]
    return dict(p=p, net=net, o=o.to(DEV), d=d.to(DEV), uc=torch.rand(N, T, generator=g).to(DEV), uf=torch.rand(N, T, generator=g).to(DEV),
                gi=torch.randn(N, 3, generator=g).to(DEV), gw=torch.randn(N, generator=g).to(DEV))


@pytest.fixture
def restore_switch():
    """The library's switch is process-wide: whatever a test does, the default (the renderer's module attribute) is back afterwards."""
    from sparsefusion_amd import _lib
    from sparsefusion_amd.nerf import renderer as R
    yield
    _lib.lib().sf_ngp_field_mfma(1 if R._FIELD_MFMA else 0)


def test_switch_defaults_to_the_mfma_kernel(restore_switch):
    from sparsefusion_amd import _lib
    from sparsefusion_amd.nerf import renderer as R
    lib = _lib.lib()
    assert R._FIELD_MFMA is True
    assert lib.sf_ngp_field_mfma(-1) == 1 and lib.sf_ngp_field_mfma(-1) == 1      # asking changes nothing
    assert lib.sf_ngp_field_mfma(0) == 1 and lib.sf_ngp_field_mfma(1) == 0 and lib.sf_ngp_field_mfma(-1) == 1


@pytest.mark.parametrize("n_rays", [64, 7])
def test_render_and_gradients_equal_the_per_point_kernel(scene, monkeypatch, restore_switch, n_rays):
    """net.render with the switch on / off / on: image, depth, weights_sum bit for bit; gradients to summation order."""
    from sparsefusion_amd.nerf import renderer as R
    s, net = scene, scene["net"]
    o, d = s["o"][:n_rays].contiguous(), s["d"][:n_rays].contiguous()
    noise = dict(u_coarse=s["uc"][:n_rays].contiguous(), u_fine=s["uf"][:n_rays].contiguous())
    gi, gw = s["gi"][:n_rays], s["gw"][:n_rays]
    kw = dict(staged=False, perturb=True, bg_color=0, shading='albedo', noise=noise, **vars(net.opt))
    out = []
    for mfma in (True, False, True):
        monkeypatch.setattr(R, "_FIELD_MFMA", mfma)
        net.zero_grad()
        r = net.render(o[None], d[None], **kw)
        ((r["image"][0] * gi).sum() + (r["weights_sum"] * gw).sum()).backward()
        out.append(({k: r[k].detach().clone() for k in ("image", "depth", "weights_sum")}, [q.grad.clone() for q in net.parameters()]))
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(out[0][0][k], out[1][0][k]), k
        assert torch.equal(out[0][0][k], out[2][0][k]), k
    assert float(out[1][0]["weights_sum"].max()) > 0                          # the rays cross the field
    for a, b, c in zip(out[0][1], out[1][1], out[2][1]):
        assert b.abs().max() > 0                                              # every parameter tensor receives a gradient
        assert (a - b).norm() <= 1e-5 * b.norm(), float((a - b).norm() / b.norm())
        assert (c - b).norm() <= 1e-5 * b.norm(), float((c - b).norm() / b.norm())


def _forward_c_abi(s, n_rays, mfma, with_cache):
    """sf_ngp_render_forward through the C ABI into NaN-filled buffers; returns the workspace rows, the cache and the ray results."""
    from sparsefusion_amd import _lib
    from sparsefusion_amd.nerf.renderer import _FieldHandle
    net = s["net"]
    N = n_rays
    params = [t.detach().contiguous() for t in net._field_params()]
    f = _FieldHandle(net).struct(params)
    lib = _lib.lib()
    nan = float("nan")
    full = lambda *shape: torch.full(shape, nan, dtype=torch.float32, device=DEV)
    od, dd, aabb = s["o"][:N].contiguous(), s["d"][:N].contiguous(), s["p"]["aabb_train"].to(DEV).contiguous()
    lin = net._table(T, torch.device(DEV))[0]
    ucd, ufd = s["uc"][:N].contiguous(), s["uf"][:N].contiguous()
    nears, fars = full(N), full(N)
    z_s, sig_s, rgb_s = full(N, 2 * T), full(N, 2 * T), full(N, 2 * T, 3)
    image, depth, ws = full(N, 3), full(N), full(N)
    wb = lib.sf_ngp_render_forward_workspace_bytes(N, T)
    work = full(wb // 4)
    cache = full(lib.sf_ngp_render_cache_bytes(N, T) // 4) if with_cache else None
    lib.sf_ngp_field_mfma(1 if mfma else 0)
    rc = lib.sf_ngp_render_forward(C.byref(f), _lib.ptr(od), _lib.ptr(dd), _lib.ptr(aabb), N, T, 0.1, _lib.ptr(lin), _lib.ptr(ucd),
                                   _lib.ptr(ufd), T, 0.0, _lib.ptr(nears), _lib.ptr(fars), _lib.ptr(z_s), _lib.ptr(sig_s), _lib.ptr(rgb_s),
                                   _lib.ptr(image), _lib.ptr(depth), _lib.ptr(ws), _lib.ptr(cache), _lib.ptr(work), wb, _lib.stream_ptr())
    _lib.check(rc)
    torch.cuda.synchronize()
    NT = N * T
    rows = dict(z_c=work[:NT], sig_c=work[NT:2 * NT], rgb_c=work[2 * NT:5 * NT], z_f=work[5 * NT:6 * NT], sig_f=work[6 * NT:7 * NT],
                rgb_f=work[7 * NT:10 * NT], image=image, depth=depth, weights_sum=ws, z_sorted=z_s, sigma_s=sig_s, rgb_s=rgb_s)
    if with_cache:
        rows["cache"] = cache
    return {k: v.cpu() for k, v in rows.items()}


@pytest.mark.parametrize("n_rays,with_cache", [(64, True), (7, True), (7, False)])
def test_workspace_rows_and_cache_equal_the_per_point_kernel(scene, restore_switch, n_rays, with_cache):
    """z_c, sig_c, rgb_c, z_f, sig_f, rgb_f and the field cache (features of both passes + the sort permutation) of the two kernels,
    bit for bit (int32 views: a NaN -- an element one kernel left unwritten -- cannot pass as equal to itself unnoticed)."""
    a = _forward_c_abi(scene, n_rays, True, with_cache)
    b = _forward_c_abi(scene, n_rays, False, with_cache)
    c = _forward_c_abi(scene, n_rays, True, with_cache)
    for k in b:
        assert not bool(torch.isnan(b[k]).any()) or k in ("cache", "depth"), k
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (k, int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum()))
        assert torch.equal(c[k].view(torch.int32), b[k].view(torch.int32)), k
    NT = n_rays * T
    for k in ("z_c", "sig_c", "rgb_c", "z_f", "sig_f", "rgb_f"):
        assert not bool(torch.isnan(a[k]).any()), k
    if with_cache:
        feats = b["cache"][:2 * NT * 32]
        assert not bool(torch.isnan(feats).any()) and float(feats.abs().max()) > 0
