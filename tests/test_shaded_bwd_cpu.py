"""CPU checks of the shaded render's backward: the closed form k_ngp_shade_bwd evaluates against torch.autograd in float64,
the oracle restatement against the real reference's gradients (tests/golden/ngp_render_shaded_grad.pt), the Python surface and the
argument checks of the two new C entries (they answer before any device call)."""
import ctypes as C
import os

import pytest
import torch

import shaded_bwd_common as sb
import shaded_common as sc
from ngp_common import params_from_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------- 1. closed form, float64
def _random_inputs(seed, P=64):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    s_off = torch.rand(P, 6, generator=g, dtype=torch.float64) * 5
    alb = torch.rand(P, 3, generator=g, dtype=torch.float64)
    w = torch.rand(P, generator=g, dtype=torch.float64)
    d = r(P, 3)
    d = d / d.norm(dim=-1, keepdim=True)
    light = torch.tensor([0.3, -0.5, 0.81], dtype=torch.float64)
    light = light / light.norm()
    # the special samples: 0, 1 face away from the light / the camera on purpose; 2, 3 have G < 1e-20; 4 has a NaN component, 5 an
    # infinite one; 6 is exactly flat (G = 0, n = 0: both dot products sit ON the clamp's boundary)
    eps = sc.EPS
    grad_of = lambda v: torch.stack([v[0] * 2 * eps, torch.zeros(()), v[1] * 2 * eps, torch.zeros(()), v[2] * 2 * eps, torch.zeros(())]).double()
    s_off[0] = 1.0 + grad_of(light * 3.0)                              # n = l: n . (-l) = -1 < 0
    s_off[1] = 1.0 + grad_of(-d[1] * 2.0)                              # n = -d: n . d = -1 < 0
    s_off[2] = 1.0 + grad_of(torch.tensor([3e-11, -2e-11, 1e-11], dtype=torch.float64))      # G = 1.4e-21
    s_off[3] = 2.0 + grad_of(torch.tensor([-1e-12, 4e-12, 2e-12], dtype=torch.float64))      # G = 2.1e-23
    s_off[6] = 2.0                                                     # G = 0
    s_off[4, 0] = float("nan")
    s_off[5, 2] = float("inf")
    return dict(s_off=s_off, alb=alb, w=w, d=d, light=light, dcol=r(P, 3), g_orient=r(P))


@pytest.mark.parametrize("ratio", [0.0, 0.1, 1.0])
def test_closed_form_equals_autograd_float64(ratio):
    """d(albedo), d(n), d(g) and d(s_e) of section 1 against torch.autograd on the reference's graph in float64: random samples plus
    n . (-l) < 0, n . d < 0, G < 1e-20 (zero and non-zero), a NaN and an infinite component; ratio 0, 0.1, 1.  1e-12."""
    I = _random_inputs(7)
    eps = sc.EPS
    s_off = I["s_off"].clone().requires_grad_(True)
    alb = I["alb"].clone().requires_grad_(True)
    sh = sb.shade_graph(s_off, alb, I["w"], I["d"], I["light"], ratio, eps)
    sh["g"].retain_grad(); sh["n"].retain_grad()
    ((sh["col"] * I["dcol"]).sum() + (sh["orient"] * I["g_orient"]).sum()).backward()
    got = sb.shade_bwd_closed(I["dcol"], I["alb"], sh["n"].detach(), sh["g"].detach(), I["w"], I["d"], I["light"], ratio, eps, I["g_orient"])
    finite = torch.isfinite(sh["g"].detach()).all(-1)
    assert int((~finite).sum()) == 2
    # n . (-l) == 0 and n . d == 0 EXACTLY (sample 6, n = 0): the selects of section 1 are strict (> 0), so nothing passes; torch.clamp
    # passes its gradient on the boundary.  The one place the formulas and torch's subgradient differ; left out of the comparison.
    assert bool((sh["n"].detach()[6] == 0).all()) and bool((got["dn"][6] == 0).all()) and bool((got["ds"][6] == 0).all())
    finite[6] = False
    lit, nd, G = sh["n"].detach() @ -I["light"], (sh["n"].detach() * I["d"]).sum(-1), (sh["g"].detach() ** 2).sum(-1)
    assert bool((lit[finite] < 0).any()) and bool((nd[finite] < 0).any()) and int((G[finite] < 1e-20).sum()) == 2
    assert float(lit[0]) < -0.999 and float(nd[1]) < -0.999
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(got["da"][finite], alb.grad[finite])
    assert close(got["dn"][finite], sh["n"].grad[finite])
    assert close(got["dg"][finite], sh["g"].grad[finite])
    assert close(got["ds"][finite], s_off.grad[finite])
    # the deviation: torch carries NaN through a non-finite gradient, the closed form passes nothing through that sample's normal
    assert not bool(torch.isfinite(s_off.grad[4:6]).all())
    assert bool((got["ds"][4:6] == 0).all()) and bool(torch.isfinite(got["da"]).all())
    if ratio == 1.0:                                                    # no diffuse term: only the orientation term reaches the normal
        only_image = sb.shade_bwd_closed(I["dcol"], I["alb"], sh["n"].detach(), sh["g"].detach(), I["w"], I["d"], I["light"], ratio, eps,
                                         torch.zeros_like(I["g_orient"]))
        assert bool((only_image["ds"] == 0).all()) and torch.equal(only_image["da"], I["dcol"])


def test_rounding_bound_of_the_closed_form_holds_for_its_fp32_evaluation():
    """shade_bwd_bound (the per-element bound the host emulation and the GPU test use) against the same closed form evaluated in fp32
    by torch: every element inside, and the bound is tight enough to mean something (median bound / |want| below 1e-5)."""
    I = _random_inputs(11, P=512)
    f = lambda t: t.float()
    sh = sb.shade_graph(f(I["s_off"]), f(I["alb"]), f(I["w"]), f(I["d"]), f(I["light"]), 0.1, sc.EPS)
    args = (f(I["dcol"]), f(I["alb"]), sh["n"], sh["g"], f(I["w"]), f(I["d"]), f(I["light"]), 0.1, sc.EPS, f(I["g_orient"]))
    got = sb.shade_bwd_closed(*args)
    ref = sb.shade_bwd_bound(*args)
    keep = ~ref["ambiguous"]
    for k in ("da", "dn", "dg", "ds"):
        err = (got[k].double() - ref["want"][k]).abs()[keep]
        bound = ref[k + "_bound"][keep]
        assert bool((err <= bound).all()), (k, float((err / bound).max()))
    nz = ref["want"]["ds"][keep] != 0
    assert float((ref["ds_bound"][keep][nz] / ref["want"]["ds"][keep][nz].abs()).median()) < 1e-5


# --------------------------------------------------------------------------------------------- 2. the oracle against the reference
@pytest.fixture(scope="module")
def grad_golden(golden_dir):
    return torch.load(os.path.join(golden_dir, "ngp_render_shaded_grad.pt"))


def test_oracle_restatement_reproduces_reference_gradients(golden_dir, grad_golden):
    """The real reference's gradients of loss = (image g_image).sum() + (weights_sum g_ws).sum() + lambda loss_orient through
    run(shading='lambertian') in train mode (tests/golden/make_golden_shaded_grad.py) against restated_grad: both are fp32 torch on the
    CPU evaluating the same graph -- 1e-5 relative per MLP tensor and per-level table sum."""
    G = grad_golden
    base = torch.load(os.path.join(golden_dir, "ngp_render.pt"))["teacher"]
    assert G["cfg"] == base["cfg"]
    assert 0.1 <= G["orient_share"] <= 0.9
    p = params_from_cfg(G["cfg"])
    o, d = sc.golden_rays(G["cfg"])
    uc, uf = sc.golden_draws(G["noise_seed"], o.shape[0])
    rs = sb.restated_grad(p, o, d, G["light_d"], G["ambient_ratio"], G["bg_color"], uc, uf, base["g_image"], base["g_ws"], G["lambda_orient"])
    for k, ref in G["grad_mlp"].items():
        got = rs["params"]["sigma_net." + k].grad
        rel = float((got - ref).norm() / ref.norm())
        print(f"{k}: rel {rel:.2e}")
        assert rel <= 1e-5, (k, rel)
    norm, lvl = sb.table_summary(rs["params"]["encoder.embeddings"].grad, p["encoder.offsets"])
    assert abs(float(norm) - float(G["grad_table_norm"])) <= 1e-5 * float(G["grad_table_norm"])
    assert torch.allclose(lvl, G["grad_table_level_abs"], rtol=1e-5, atol=0)
    live = torch.isfinite(G["dsigma"])
    assert torch.allclose(rs["dsigma"][live], G["dsigma"][live], rtol=1e-5, atol=1e-9 * float(G["dsigma"][live].abs().max()))
    assert abs(float(rs["loss_orient"]) - float(G["loss_orient"])) <= 1e-6 * float(G["loss_orient"])


def test_oracle_descent_figures_are_what_the_gpu_test_assumes(golden_dir):
    """The CPU oracle's own ten Adam steps of the descent problem (shaded_bwd_common.oracle_descent): the loss falls on every step, from
    DESCENT_ORACLE[0] to DESCENT_ORACLE[1] -- the margin tests/test_gpu_shaded_backward.py::test_ten_adam_steps_lower_the_loss halves."""
    cfg = torch.load(os.path.join(golden_dir, "ngp_render.pt"))["teacher"]["cfg"]
    losses = sb.oracle_descent(params_from_cfg(cfg))
    print("oracle descent:", [round(v, 5) for v in losses])
    assert len(losses) == sb.DESCENT["steps"] + 1 and all(b < a for a, b in zip(losses, losses[1:]))
    assert abs(losses[0] - sb.DESCENT_ORACLE[0]) <= 2e-5 and abs(losses[-1] - sb.DESCENT_ORACLE[1]) <= 2e-5
    assert sb.DESCENT_ORACLE[0] - sb.DESCENT_ORACLE[1] > 0.03


# ------------------------------------------------------------------------------------------------------------ 3. Python surface
def _net(trainable):
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    net = NeRFNetwork(get_default_torch_ngp_opt())
    for q in net.parameters():
        q.requires_grad_(trainable)
    return net


def test_shading_backward_is_opt_in():
    from sparsefusion_amd.nerf import NeRFRenderer, get_default_torch_ngp_opt
    assert get_default_torch_ngp_opt().shading_backward is False
    assert "shading_backward" in NeRFRenderer.run.__doc__
    net = _net(True)
    o, d = torch.zeros(1, 4, 3), torch.ones(1, 4, 3)
    kw = dict(num_steps=8, upsample_steps=8, shading='lambertian', light_d=torch.tensor([0.0, 0.0, 1.0]))
    with pytest.raises(NotImplementedError, match="the shaded render has no backward"):
        net.run(o, d, **kw)
    with pytest.raises(NotImplementedError, match="the shaded render has no backward"):
        net.run(o, d, shading_backward=False, **kw)
    # with the key the call passes that check and stops at the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        net.run(o, d, shading_backward=True, **kw)
    # ... and through render / **vars(opt), the way w / h travel
    opt = dict(vars(net.opt), shading_backward=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        net.render(o, d, staged=False, shading='lambertian', light_d=torch.tensor([0.0, 0.0, 1.0]), **opt)
    with pytest.raises(NotImplementedError, match="the shaded render has no backward"):
        net.render(o, d, staged=False, shading='lambertian', light_d=torch.tensor([0.0, 0.0, 1.0]), **vars(net.opt))
    # the key changes nothing for the albedo render (it stops at the same device check either way)
    with pytest.raises(RuntimeError, match="HIP device"):
        net.run(o, d, num_steps=8, upsample_steps=8, shading='albedo', shading_backward=True)


# -------------------------------------------------------------------------------------------------------------------- 4. C ABI
def test_shaded_backward_abi_argument_checks():
    """The new symbols are declared in the header and in _lib under the same argument counts, sf_abi_version is unchanged, and the
    argument checks answer without a device: a null required pointer, T outside [4, 64], a bad epsilon, a non-finite ratio, a short
    workspace -> SF_ERR_INVALID; N == 0 -> SF_OK."""
    from sparsefusion_amd import _lib
    header = open(os.path.join(ROOT, "include", "sparsefusion_hip.h")).read()
    for name, n_args in (("sf_ngp_render_shaded_forward_train", 32), ("sf_ngp_render_shaded_backward", 27),
                         ("sf_ngp_render_shaded_backward_workspace_bytes", 2)):
        assert name + "(" in header
        assert len(_lib.SIGNATURES[name][1]) == n_args
    lib = _lib.lib()
    N, T = 256, 64
    assert lib.sf_ngp_render_shaded_backward_workspace_bytes(N, T) == lib.sf_ngp_render_workspace_bytes(N, T) + 6 * N * 2 * T * 4
    f, g = _lib.SfNgpField(), _lib.SfNgpFieldGrad()
    buf = (C.c_float * 64)()
    pb = C.cast(buf, C.c_void_p)
    OK, INVALID = 0, 1
    big = 1 << 40

    def bwd(N=4, T=8, light=pb, ratio=0.1, eps=1e-2, wbytes=big, grad_s=pb, g_image=pb, work=pb, w_s=pb):
        return lib.sf_ngp_render_shaded_backward(C.byref(f), C.byref(g), pb, pb, pb, N, T, pb, pb, pb, pb, pb, pb, pb, grad_s, w_s, light,
                                                 ratio, eps, 1.0, g_image, None, None, 0, work, wbytes, None)

    for kw in (dict(light=None), dict(grad_s=None), dict(w_s=None), dict(g_image=None)):
        assert bwd(**kw) == INVALID, kw
        assert b"null pointer" in lib.sf_last_error()
    for eps in (0.0, -1e-2, float("inf"), float("nan")):
        assert bwd(eps=eps) == INVALID, eps
        assert b"epsilon" in lib.sf_last_error()
    for ratio in (float("inf"), float("nan")):
        assert bwd(ratio=ratio) == INVALID, ratio
        assert b"ambient_ratio" in lib.sf_last_error()
    for T_ in (0, 3, 65):
        assert bwd(T=T_) == INVALID, T_
        assert b"T must be" in lib.sf_last_error()
    assert bwd(wbytes=lib.sf_ngp_render_shaded_backward_workspace_bytes(4, 8) - 1) == INVALID
    assert b"workspace" in lib.sf_last_error()
    assert bwd(work=None) == INVALID
    assert bwd(N=0) == OK and bwd(N=0, T=1000, wbytes=0, work=None) == OK
    assert bwd(N=0, eps=0.0) == INVALID                                 # the value checks come before N == 0

    def fwd(N=4, T=8, grad_s=pb, w_s=pb, eps=1e-2, wbytes=1 << 20):
        return lib.sf_ngp_render_shaded_forward_train(C.byref(f), pb, pb, pb, N, T, 0.1, pb, None, pb, 0, 1.0, pb, 0.1, eps, pb, pb, pb, pb, pb,
                                                      pb, pb, grad_s, w_s, pb, None, None, pb, pb, pb, wbytes, None)

    assert fwd(grad_s=None) == INVALID and fwd(w_s=None) == INVALID
    assert b"grad_s" in lib.sf_last_error()
    assert fwd(eps=0.0) == INVALID and fwd(T=3) == INVALID and fwd(wbytes=16) == INVALID
    assert fwd(N=0) == OK

    # one offset pass on its own (sf_ngp_render_offset_backward): e in [1, 6], and the checks of the full entry
    assert "sf_ngp_render_offset_backward(" in header and len(_lib.SIGNATURES["sf_ngp_render_offset_backward"][1]) == 15

    def one(e=2, N=4, T=8, ds=pb, eps=1e-2, wbytes=big):
        return lib.sf_ngp_render_offset_backward(C.byref(f), C.byref(g), pb, pb, pb, N, T, pb, ds, e, eps, 0, pb, wbytes, None)

    for e in (0, 7):
        assert one(e=e) == INVALID, e
        assert b"e must be" in lib.sf_last_error()
    assert one(ds=None) == INVALID and one(eps=0.0) == INVALID and one(T=65) == INVALID
    assert one(wbytes=lib.sf_ngp_render_workspace_bytes(4, 8) - 1) == INVALID
    assert one(N=0) == OK
