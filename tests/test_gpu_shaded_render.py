"""GPU tests of the Lambertian-shaded render (sf_ngp_render_shaded_forward, sparsefusion_amd/csrc/ngp_shade.h) and of
NeRFRenderer.run / render_batched with shading='lambertian'.  Bit-level anchors tie every stage to a kernel that is already pinned:
the bookkeeping to sf_ngp_render_forward, the points to the float32 formula and sf_ngp_density, the normals to sf_ngp_point_attrs,
the colour to its numpy float32 restatement, the ratio-1 image to the albedo render; the real reference's render
(tests/golden/ngp_render_shaded.pt) is held within a per-ray bound derived from the density tolerances.  Fields: `teacher` /
`default_init` of tests/golden/ngp_render.pt."""
import ctypes as C

import numpy as np
import pytest
import torch

import point_attrs_common as pc
import shaded_common as sc
from ngp_common import params_from_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIGHTS = ((0.3, -0.5, 0.81), (-0.7, 0.2, -0.4))
# N = 1, 3, 4, 5: partial 4-ray workgroups; 2T = 8 and 14 leave most lanes dead, 128 fills the wave; N = 4099 at T = 64: 524 672 sorted
# samples, one tail past the 524 288 threads of the capped grid -- the shade loop runs twice
SHAPES = [(1, 4), (3, 7), (4, 64), (5, 64), (4099, 64)]
BOOK = ("nears", "fars", "z_sorted", "sigma_s", "rgb_s", "depth", "weights_sum")
NULLABLE = ("xyz_s", "normal_image", "orient")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_render.pt")


@pytest.fixture(scope="module")
def shaded_golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_render_shaded.pt")


def _net(p):
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    net = NeRFNetwork(get_default_torch_ngp_opt())
    net.load_state_dict({k: p[k] for k in net.state_dict().keys() if k in p})
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def nets(golden):
    return {name: _net(params_from_cfg(golden[name]["cfg"])) for name in ("teacher", "default_init")}


def _light(k):
    l = torch.tensor(LIGHTS[k], dtype=torch.float32)
    return (l / l.norm()).to(DEV)


def _rays(N):
    if N <= 16:
        o, d = sc.small_rays(N)
    else:                                                        # the golden teacher view (one miss ray per 256), repeated
        o, d = sc.golden_rays(dict(view=3, unit_dir=False))
        reps = (N + 255) // 256
        o, d = o.repeat(reps, 1)[:N], d.repeat(reps, 1)[:N]
    return o.contiguous().to(DEV), d.contiguous().to(DEV)


def _nan(*s):
    return torch.full(s, float("nan"), dtype=torch.float32, device=DEV)


def _common(net, o, T, uc, uf):
    from sparsefusion_amd import _lib
    lin, _ = net._table(T, o.device)
    params = [t.detach().contiguous() for t in net._field_params()]
    return _lib, lin, params, net._field_handle().struct(params)


def _albedo(net, o, d, T, uc, uf, bg):
    """sf_ngp_render_forward through the C ABI (no field cache) into NaN-filled buffers"""
    _lib, lin, params, f = _common(net, o, T, uc, uf)
    N = o.shape[0]
    out = dict(nears=_nan(N), fars=_nan(N), z_sorted=_nan(N, 2 * T), sigma_s=_nan(N, 2 * T), rgb_s=_nan(N, 2 * T, 3), image=_nan(N, 3),
               depth=_nan(N), weights_sum=_nan(N))
    lib = _lib.lib()
    wbytes = lib.sf_ngp_render_forward_workspace_bytes(N, T)
    work = torch.empty(wbytes // 4, dtype=torch.float32, device=DEV)
    rc = lib.sf_ngp_render_forward(C.byref(f), _lib.ptr(o), _lib.ptr(d), _lib.ptr(net.aabb_train), N, T, float(net.min_near), _lib.ptr(lin),
                                   _lib.ptr(uc), _lib.ptr(uf), T, float(bg), *[_lib.ptr(out[k]) for k in
                                                                              ("nears", "fars", "z_sorted", "sigma_s", "rgb_s", "image",
                                                                               "depth", "weights_sum")],
                                   None, _lib.ptr(work), wbytes, _lib.stream_ptr())
    _lib.check(rc, "ngp_render_forward")
    return out


def _shaded(net, o, d, T, uc, uf, bg, light, ratio, skip=()):
    """sf_ngp_render_shaded_forward through the C ABI into NaN-filled buffers (an unwritten element fails the comparisons); the
    nullable outputs named in `skip` are passed as NULL"""
    _lib, lin, params, f = _common(net, o, T, uc, uf)
    N = o.shape[0]
    out = dict(nears=_nan(N), fars=_nan(N), z_sorted=_nan(N, 2 * T), sigma_s=_nan(N, 2 * T), rgb_s=_nan(N, 2 * T, 3),
               normal_s=_nan(N, 2 * T, 3), rgb_shaded_s=_nan(N, 2 * T, 3), xyz_s=_nan(N, 2 * T, 3), image=_nan(N, 3),
               normal_image=_nan(N, 3), orient=_nan(N), depth=_nan(N), weights_sum=_nan(N))
    for k in skip:
        out[k] = None
    lib = _lib.lib()
    wbytes = lib.sf_ngp_render_shaded_workspace_bytes(N, T)
    work = torch.empty(wbytes // 4, dtype=torch.float32, device=DEV)
    rc = lib.sf_ngp_render_shaded_forward(C.byref(f), _lib.ptr(o), _lib.ptr(d), _lib.ptr(net.aabb_train), N, T, float(net.min_near),
                                          _lib.ptr(lin), _lib.ptr(uc), _lib.ptr(uf), T, float(bg), _lib.ptr(light), float(ratio),
                                          float(sc.EPS), *[_lib.ptr(out[k]) for k in
                                                           ("nears", "fars", "z_sorted", "sigma_s", "rgb_s", "normal_s", "rgb_shaded_s",
                                                            "xyz_s", "image", "normal_image", "orient", "depth", "weights_sum")],
                                          _lib.ptr(work), wbytes, _lib.stream_ptr())
    _lib.check(rc, "ngp_render_shaded_forward")
    return out


def _same(a, b, what):
    assert np.array_equal(pc.bits(a), pc.bits(b)), what


# ------------------------------------------------------------------------------------------------- 1-4, 6. the bit-level anchors
@pytest.mark.parametrize("N,T", SHAPES)
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_shaded_entry_anchors(nets, name, N, T):
    from sparsefusion_amd import mesh
    net = nets[name]
    o, d = _rays(N)
    g = torch.Generator().manual_seed(100 * N + T)
    uc, uf = torch.rand(N, T, generator=g).to(DEV), torch.rand(N, T, generator=g).to(DEV)     # perturbed coarse, unsorted fine depths
    bg = 0.25
    alb = _albedo(net, o, d, T, uc, uf, bg)
    runs = {(r, k): _shaded(net, o, d, T, uc, uf, bg, _light(k), r) for r, k in ((0.1, 0), (0.0, 1), (1.0, 0))}
    first = runs[0.1, 0]
    if N > 1:
        miss = N - 2 if N <= 16 else 5
        assert not bool(first["nears"][miss] < first["fars"][miss])
        assert float(first["weights_sum"][miss]) == 0.0 and float(first["orient"][miss]) == 0.0
    # 2. points: the float32 formula on every finite depth, and the field values the albedo pass already holds
    z = first["z_sorted"].cpu().numpy()
    x_np = sc.np_points(o.cpu().numpy(), d.cpu().numpy(), z, net.aabb_train.cpu().numpy())
    finite = np.isfinite(z)
    assert np.array_equal(pc.bits(first["xyz_s"])[finite], x_np.view(np.uint32)[finite])
    assert not torch.isnan(first["xyz_s"]).any()
    x = first["xyz_s"].view(-1, 3)
    with torch.no_grad():
        dens = net.density(x)
    _same(dens["sigma"], first["sigma_s"].view(-1), "sigma at xyz_s")
    _same(dens["albedo"], first["rgb_s"].view(-1, 3), "albedo at xyz_s")
    normal = mesh.point_attributes(net, x, sc.EPS, sigma=False, albedo=False, grad=False)["normal"].view(N, 2 * T, 3)
    for (ratio, k), got in runs.items():
        # 1. bookkeeping: what sf_ngp_render_forward leaves, at any ratio
        for key in BOOK:
            _same(got[key], alb[key], (key, ratio))
        _same(got["xyz_s"], first["xyz_s"], ("xyz_s", ratio))
        # 3. normals: sf_ngp_point_attrs at the same points; colour: the numpy float32 restatement from that normal
        _same(got["normal_s"], normal, ("normal_s", ratio))
        want = sc.np_shade(got["rgb_s"].cpu().numpy(), got["normal_s"].cpu().numpy(), _light(k).cpu().numpy(), ratio)
        _same(got["rgb_shaded_s"], want, ("rgb_shaded_s", ratio))
        for key in ("image", "normal_image", "orient"):
            assert not torch.isnan(got[key]).any(), (key, ratio)
        _same(got["normal_image"], first["normal_image"], ("normal_image", ratio))
        _same(got["orient"], first["orient"], ("orient", ratio))
    # 4. ratio 1: the albedo render's image
    _same(runs[1.0, 0]["image"], alb["image"], "image at ratio 1")
    _same(runs[1.0, 0]["rgb_shaded_s"], alb["rgb_s"], "colour at ratio 1")
    if name == "teacher" and T == 64:
        assert not np.array_equal(pc.bits(first["image"]), pc.bits(alb["image"]))      # the shading is visible
    # the sums against a front-to-back float32 loop (small shapes: the loop is Python)
    if N <= 16:
        ref = sc.np_composite(*(first[k].cpu().numpy() for k in ("z_sorted", "sigma_s", "rgb_shaded_s", "normal_s")), d.cpu().numpy(),
                              first["nears"].cpu().numpy(), first["fars"].cpu().numpy(), T, bg)
        for key, want in zip(("image", "depth", "weights_sum", "normal_image", "orient"), ref):
            a = first[key].cpu().numpy()
            live = ~np.isnan(want)
            assert np.array_equal(np.isnan(a), ~live), key
            assert float(np.abs(a[live] - want[live]).max(initial=0.0)) <= 1e-5, key
    # 6. every nullable output skipped in turn: the others do not change
    for skip in NULLABLE:
        part = _shaded(net, o, d, T, uc, uf, bg, _light(0), 0.1, skip=(skip,))
        for key, v in part.items():
            if key != skip:
                _same(v, first[key], (skip, key))


# ------------------------------------------------------------------------------------------------------------------ 5. the golden
@pytest.fixture(scope="module")
def oracle_cases(golden, shaded_golden):
    """case -> (draws, oracle restatement with its weights and per-sample bound ratios) -- computed once on the CPU, never modified"""
    G = shaded_golden
    p = params_from_cfg(G["cfg"])
    o, d = sc.golden_rays(G["cfg"])
    out = {}
    for case in ("eval", "train"):
        uc, uf = sc.golden_draws(G[case]["noise_seed"], o.shape[0]) if case == "train" else (None, None)
        out[case] = (uc, uf, sc.restated(p, o, d, G["light_d"], G["ambient_ratio"], G["bg_color"], uc, uf, training=case == "train"))
    return out


@pytest.mark.parametrize("case", ["eval", "train"])
def test_shaded_render_against_reference_golden(nets, shaded_golden, oracle_cases, case):
    """The real reference's render of the teacher field.  With the oracle's weights w_i and r_i = |gradient bound_i| / |gradient_i|
    (point_attrs_common), delta_i = min(2, 2 r_i + 1e-6) bounds how far a normal may move:
      |image - golden| <= 2e-5 + (1 - ratio) sum_i w_i delta_i                     per ray and channel
      |loss_orient - golden| <= mean_i w_i (2 c_i |d| delta_i + |d|^2 delta_i^2) + 1e-5 golden,    c_i = max(n_i . d, 0)
    and the image bound itself is at most 1e-2 on every ray (the shaded-minus-albedo contrast of this scene is 0.115 mean)."""
    G = shaded_golden
    net = nets["teacher"]
    uc, uf, rs = oracle_cases[case]
    o, d = sc.golden_rays(G["cfg"])
    o, d = o[None].to(DEV), d[None].to(DEV)
    kw = dict(num_steps=64, upsample_steps=64, light_d=G["light_d"], ambient_ratio=G["ambient_ratio"], shading='lambertian',
              bg_color=G["bg_color"])
    try:
        if case == "train":
            net.train()
            with torch.no_grad():
                r = net.run(o, d, perturb=True, noise=dict(u_coarse=uc.to(DEV), u_fine=uf.to(DEV)), **kw)
        else:
            with torch.no_grad():
                r = net.run(o, d, perturb=False, **kw)
    finally:
        net.eval()
    assert sorted(r) == ["depth", "image", "loss_orient", "mask", "normal", "weights_sum"]
    bound = sc.image_bound(rs, G["ambient_ratio"])
    err = (r["image"][0].cpu() - G[case]["image"]).abs().double().numpy().max(axis=1)
    ob = sc.orient_bound(rs, G[case]["loss_orient"])
    oerr = abs(float(r["loss_orient"]) - float(G[case]["loss_orient"]))
    print(f"{case}: image err max {err.max():.2e} (max err / bound {float((err / bound).max()):.3f}); bound median "
          f"{float(np.median(bound)):.2e} max {float(bound.max()):.2e}; loss_orient {float(r['loss_orient']):.6e} vs "
          f"{float(G[case]['loss_orient']):.6e}, err {oerr:.2e}, bound {ob:.2e}; weights_sum err "
          f"{float((r['weights_sum'].cpu() - G[case]['weights_sum']).abs().max()):.2e}")
    assert float(bound.max()) <= 1e-2
    assert (err <= bound).all()
    assert oerr <= ob
    assert r["normal"].shape == (1, 256, 3) and r["image"].shape == (1, 256, 3) and r["loss_orient"].dim() == 0


# ------------------------------------------------------------------------------------------------------------------- 7. Python
def _golden_view():
    o, d = sc.golden_rays(dict(view=3, unit_dir=False))
    return o[None].to(DEV), d[None].to(DEV)


def test_render_batched_chunks_equal_one_call(nets):
    net = nets["teacher"]
    o, d = _golden_view()
    kw = dict(num_steps=64, upsample_steps=64, light_d=_light(0), ambient_ratio=0.1, shading='lambertian', bg_color=1, perturb=False)
    one = net.render_batched(o, d, batched=False, **kw)
    many = net.render_batched(o, d, batched=True, max_ray_batch=100, **kw)
    assert sorted(many) == ["depth", "image", "normal", "weights_sum"]
    for k in ("image", "normal", "weights_sum"):
        _same(many[k].reshape(-1), one[k].reshape(-1), k)
    _same(many["depth"], one["depth"], "depth")
    alb = net.render_batched(o, d, batched=True, max_ray_batch=100, **dict(kw, shading='albedo'))
    assert sorted(alb) == ["depth", "image", "weights_sum"]                          # albedo results are what they were


@pytest.mark.parametrize("training", [False, True])
def test_random_light_consumes_one_draw(nets, training):
    """light_d=None: the light is safe_normalize(rays_o[0] + randn(3)), the one draw an albedo render consumes at the same place, so
    the generator stands where it stands after an albedo render (eval: one draw; train + perturb: the same three)."""
    from sparsefusion_amd.nerf.utils import safe_normalize
    net = nets["teacher"]
    o, d = _golden_view()
    kw = dict(num_steps=64, upsample_steps=64, ambient_ratio=0.1, bg_color=1, perturb=training)
    net.train(training)
    try:
        with torch.no_grad():
            torch.manual_seed(11)
            net.run(o, d, shading='albedo', **kw)
            after_albedo = torch.cuda.get_rng_state(0)
            torch.manual_seed(11)
            got = net.run(o, d, shading='lambertian', **kw)
            after_shaded = torch.cuda.get_rng_state(0)
            assert torch.equal(after_albedo, after_shaded)
            torch.manual_seed(11)
            light = safe_normalize(o[0, 0] + torch.randn(3, device=DEV, dtype=torch.float))
            if not training:
                assert torch.equal(torch.cuda.get_rng_state(0), after_shaded)         # exactly one randn(3)
            torch.manual_seed(11)
            torch.randn(3, device=DEV, dtype=torch.float)                             # an explicit light consumes no draw: stand in for it
            want = net.run(o, d, shading='lambertian', light_d=light, **kw)
    finally:
        net.eval()
    _same(got["image"], want["image"], "image")
    _same(got["normal"], want["normal"], "normal")


def test_fixed_light_matches_the_torch_formula(nets):
    from sparsefusion_amd.nerf.utils import safe_normalize
    net = nets["teacher"]
    o, d = _golden_view()
    kw = dict(num_steps=64, upsample_steps=64, ambient_ratio=0.1, bg_color=1, perturb=False, shading='lambertian')
    rot_m = torch.tensor([[0.63, .65, -0.43], [-.43, .75, -0.5], [-.65, .13, .75]], device=DEV, dtype=torch.float)
    light = safe_normalize(o[0, 0] @ rot_m)
    with torch.no_grad():
        state = torch.cuda.get_rng_state(0)
        got = net.run(o, d, fixed_light=True, **kw)
        assert torch.equal(torch.cuda.get_rng_state(0), state)                       # no draw
        want = net.run(o, d, light_d=light, **kw)
        other = net.run(o, d, light_d=_light(1), **kw)
    _same(got["image"], want["image"], "image")
    assert not np.array_equal(pc.bits(got["image"]), pc.bits(other["image"]))
    # the same render through the C ABI (the deterministic fine-sample table as one row per ray): image and the orientation mean
    N, T = 256, 64
    det = net._table(T, o.device)[1].expand(N, T).contiguous()
    raw = _shaded(net, o[0].contiguous(), d[0].contiguous(), T, None, det, 1, light, 0.1)
    _same(got["image"][0], raw["image"], "image through the C ABI")
    _same(got["normal"][0], raw["normal_image"], "normal image through the C ABI")
    _same(got["loss_orient"], raw["orient"].sum() / (N * 2 * T), "loss_orient")
    assert float(got["loss_orient"]) > 0.0
