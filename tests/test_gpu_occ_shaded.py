"""Shaded occupancy-grid evaluation render on the GPU: sf_ngp_render_occ_eval_shaded / run_cuda(shading='lambertian') in eval mode
(sparsefusion_amd/csrc/ngp_occ_shade.h, eight lanes per ray).  Anchors: (1) at ambient_ratio = 1 it IS the albedo kernel, bit for bit;
(2) the route composed from entry points that are already pinned (march_rays -> point_attributes -> torch shading -> composite_rays);
(3) the real reference's render (tests/golden/ngp_occ_render_shaded.pt), every ray within a bound derived from the density
tolerances; (4) the Python surface."""
import numpy as np
import pytest
import torch

import occ_shaded_common as oc
import point_attrs_common as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 7, 8, 9, 31, 32, 33, 256)           # groups of a wave, a workgroup's 32 rays and one more, several workgroups


@pytest.fixture(scope="module")
def net():
    return oc.make_net(oc.params(), DEV)[0]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_occ_render_shaded.pt")


@pytest.fixture(scope="module")
def scenes():
    """name -> (scene on the CPU, the same on the device) -- built once, shared, never modified"""
    out = {"golden": oc.golden_scene(), "small": oc.small_scene(33)}
    return {k: (v, oc.to_dev(v, DEV)) for k, v in out.items()}


@pytest.fixture(scope="module")
def golden_restated(golden, scenes):
    return oc.restated(oc.params(), scenes["golden"][0], golden["light_d"], golden["ambient_ratio"], golden["cfg"]["T_thresh"])


def _same(a, b):
    return np.array_equal(pc.bits(a), pc.bits(b))


# ----------------------------------------------------------------------------------------------- 1. ratio 1 is the albedo kernel
@pytest.mark.parametrize("N", SIZES)
def test_ratio_one_is_the_albedo_kernel_bit_for_bit(net, N):
    light = oc.unit(oc.LIGHT)
    for max_steps in (64, 256):
        sd = oc.to_dev(oc.small_scene(N, max_steps), DEV)
        for noises in (None, torch.rand(N, generator=torch.Generator().manual_seed(N)).to(DEV)):
            alb = oc.gpu_entry(net, sd, None, 1.0, 1e-4, noises=noises, shaded=False)
            one = oc.gpu_entry(net, sd, light, 1.0, 1e-4, noises=noises)
            low = oc.gpu_entry(net, sd, light, oc.RATIO, 1e-4, noises=noises)
            for k in ("image", "depth", "weights_sum"):
                assert not torch.isnan(one[k]).any() and not torch.isnan(low[k]).any(), k
                assert _same(one[k], alb[k]), (max_steps, noises is not None, k)
            for k in ("depth", "weights_sum", "normal_image", "n_samples"):          # they do not depend on the colour
                assert torch.equal(low[k], one[k]), (max_steps, noises is not None, k)
            assert float(one["weights_sum"][0]) > 0.5                                # the first ray goes through the ball


# ------------------------------------------------------------------------------------------------------- 2. the composed route
@pytest.mark.parametrize("scene,T_thresh,light,ratio", [("golden", 1e-4, oc.LIGHT, 0.1), ("small", 1e-4, oc.LIGHT, 0.1),
                                                        ("small", 0.3, oc.LIGHT2, 0.1), ("small", 0.0, oc.LIGHT, 0.0),
                                                        ("golden", 1e-4, oc.LIGHT2, 0.0)])
def test_equals_the_route_composed_from_pinned_entry_points(net, scenes, scene, T_thresh, light, ratio):
    """Same per-sample formulas on both sides, so bit-equality is expected; all four outputs (depth un-normalised) are asserted at
    the absolute 2e-6 that tests/test_gpu_occ.py gives this compositor against the C oracle; the number of elements that differ in
    bits is printed."""
    sd = scenes[scene][1]
    light = oc.unit(light)
    got = oc.gpu_entry(net, sd, light, ratio, T_thresh)
    ws, depth, image, nimg, count = oc.composed_gpu(net, sd, light, ratio, T_thresh)
    want = dict(weights_sum=ws, depth=depth, image=image, normal_image=nimg)
    diff = {k: int((pc.bits(got[k]) != pc.bits(want[k])).sum()) for k in want}
    print(f"{scene} T_thresh={T_thresh} ratio={ratio}: elements that differ in bits {diff}, "
          + ", ".join(f"max |{k}| diff {float((got[k] - want[k]).abs().max()):.2e}" for k in want))
    for k in ("weights_sum", "depth", "image", "normal_image"):
        assert torch.allclose(got[k], want[k], rtol=0, atol=2e-6), k
    n = got["n_samples"].long()
    if T_thresh == 0.0:
        assert torch.equal(n, count)
        assert int(count.max()) == sd["max_steps"] and int(count.min()) == 0      # a capped ray and a miss
    else:
        hit = count > 0
        assert (n[hit] >= 1).all() and (n <= count).all() and (n[~hit] == 0).all()
        assert (n < count).any()                                                   # rays ended by the threshold


# --------------------------------------------------------------------------------------------------------- 3. golden, every ray
def test_reference_golden_every_ray(net, scenes, golden, golden_restated):
    """|image - golden| <= 2e-5 + T_thresh + (1 - ratio) sum_i w_i delta_i on EVERY ray (the bitfield is analytic: no cell sits on
    a threshold), delta_i = min(2, 2 r_i + 1e-6) from the density tolerances; the bound is capped at 1e-2.  Depth and weights_sum:
    test (1) ties them to the albedo kernel bit for bit, and the albedo kernel is held to the golden's albedo render here at the
    tolerances of test_gpu_occ_render.py."""
    G, (sc, sd), rs = golden, scenes["golden"], golden_restated
    cfg = G["cfg"]
    got = oc.gpu_entry(net, sd, G["light_d"], G["ambient_ratio"], cfg["T_thresh"])
    img, _ = oc.finish(sc, got["image"].cpu(), got["depth"].cpu(), got["weights_sum"].cpu(), G["bg_color"])
    bound = oc.image_bound(rs)
    err = (img.double() - G["shaded"]["image"].double()).abs().amax(-1).numpy()
    print(f"golden: max |image - golden| {err.max():.2e}, max err / bound {float((err / bound).max()):.3f}, bound median "
          f"{float(np.median(bound)):.2e} max {bound.max():.2e}")
    assert bound.max() <= oc.IMAGE_BOUND_CAP
    assert (err <= bound).all()
    alb = oc.gpu_entry(net, sd, None, 1.0, cfg["T_thresh"], shaded=False)
    img_a, dep_a = oc.finish(sc, alb["image"].cpu(), alb["depth"].cpu(), alb["weights_sum"].cpu(), G["bg_color"])
    hit = sc["nears"] < sc["fars"]
    e_img = (img_a - G["albedo"]["image"]).abs().amax(-1)
    e_ws = (alb["weights_sum"].cpu() - G["albedo"]["weights_sum"]).abs()
    e_dep = (dep_a[hit] - G["albedo"]["depth"][hit]).abs()
    print(f"albedo kernel vs golden albedo: image {float(e_img.max()):.2e}, weights_sum {float(e_ws.max()):.2e}, depth "
          f"{float(e_dep.max()):.2e}")
    assert float((e_img <= 1e-4).float().mean()) > 0.98 and float((e_ws <= 1e-4).float().mean()) > 0.98
    assert float((e_dep <= 1e-3).float().mean()) > 0.98
    assert _same(got["weights_sum"], alb["weights_sum"]) and _same(got["depth"], alb["depth"])


# ------------------------------------------------------------------------------------------------------------------- 4. surface
def test_run_cuda_surface(net, scenes, golden):
    from sparsefusion_amd import raymarching
    from sparsefusion_amd.nerf.utils import safe_normalize
    sc, sd = scenes["golden"]
    net.density_bitfield.copy_(sd["bits"])
    o, d, light = sd["o"], sd["d"], golden["light_d"].to(DEV)
    kw = dict(shading='lambertian', ambient_ratio=oc.RATIO, bg_color=oc.BG, perturb=False, max_steps=sc["max_steps"], T_thresh=1e-4)
    with torch.no_grad():
        r = net.run_cuda(o[None], d[None], light_d=light, **kw)
    assert set(r) == {'image', 'depth', 'weights_sum', 'mask', 'normal'} and r['normal'].shape == (1, 256, 3)
    nears, fars = raymarching.near_far_from_aabb(o, d, net.aabb_infer)          # run_cuda's own near / far
    assert torch.allclose(nears.cpu(), sc["nears"], rtol=1e-6, atol=0) and torch.allclose(fars.cpu(), sc["fars"], rtol=1e-6, atol=0)
    sd = dict(sd, nears=nears, fars=fars)
    got = oc.gpu_entry(net, sd, light, oc.RATIO, 1e-4)
    img = got["image"] + (1 - got["weights_sum"]).unsqueeze(-1) * oc.BG
    dep = torch.clamp(got["depth"] - nears, min=0) / (fars - nears)
    assert torch.equal(r['image'][0], img) and torch.equal(r['weights_sum'][0], got["weights_sum"])
    assert torch.equal(r['depth'][0], dep) and torch.equal(r['normal'][0], got["normal_image"])
    assert float(r['normal'][0].norm(dim=-1).max()) > 0.5
    # chunks of 100 rays: bit-identical, and the normal map travels through _chunked
    b = net.render_batched(o[None], d[None], batched=True, max_ray_batch=100, light_d=light, **kw)
    assert set(b) == {'image', 'depth', 'weights_sum', 'normal'}
    for k in b:
        assert torch.equal(b[k], r[k]), k
    # light_d=None: safe_normalize(rays_o[0] + randn(3)) drawn on the device from the current generator
    torch.manual_seed(11)
    with torch.no_grad():
        drawn = net.run_cuda(o[None], d[None], **kw)
    torch.manual_seed(11)
    l2 = safe_normalize(o[0] + torch.randn(3, device=DEV, dtype=torch.float))
    with torch.no_grad():
        given = net.run_cuda(o[None], d[None], light_d=l2, **kw)
    for k in drawn:
        assert torch.equal(drawn[k], given[k]), k
    assert not torch.equal(drawn['image'], r['image'])
    # shading='albedo' consumes no random draw and is what it was: the fused albedo kernel's outputs
    torch.manual_seed(12)
    first = torch.rand(4, device=DEV)
    torch.manual_seed(12)
    with torch.no_grad():
        a = net.run_cuda(o[None], d[None], **dict(kw, shading='albedo'))
    assert torch.equal(torch.rand(4, device=DEV), first)
    alb = oc.gpu_entry(net, sd, None, 1.0, 1e-4, shaded=False)
    assert torch.equal(a['image'][0], alb["image"] + (1 - alb["weights_sum"]).unsqueeze(-1) * oc.BG) and 'normal' not in a
    # training mode and the smooth-normal shadings keep raising
    with pytest.raises(NotImplementedError, match="has no shaded form"):
        net.train().run_cuda(o[None], d[None], light_d=light, **kw)
    net.eval()
    for shading in ("textureless", "normal"):
        with pytest.raises(NotImplementedError):
            net.run_cuda(o[None], d[None], **dict(kw, shading=shading))


def test_every_output_written_missing_ray_and_nullable_outputs(net, scenes):
    sc, sd = scenes["small"]
    sd = dict(sd)
    o, d = sc["o"].clone(), sc["d"].clone()
    o[5] = torch.tensor([20.0, 20.0, 20.0]); d[5] = torch.tensor([1.0, 0.0, 0.0])      # misses the box: near = far = FLT_MAX
    nears, fars = oc.near_far(o, d)
    assert float(nears[5]) == float(fars[5]) > 1e38
    sd.update(o=o.to(DEV), d=d.to(DEV), nears=nears.to(DEV), fars=fars.to(DEV))
    light = oc.unit(oc.LIGHT)
    full = oc.gpu_entry(net, sd, light, oc.RATIO, 1e-4)
    for k, v in full.items():
        assert not torch.isnan(v.float()).any() and (k != "n_samples" or (v >= 0).all()), k
    for m in (1, 5):                                                    # misses the ball / misses the box: all zero
        for k, v in full.items():
            assert float(v[m].float().abs().max()) == 0.0, (m, k)
    for skip in ("normal", "count"):
        part = oc.gpu_entry(net, sd, light, oc.RATIO, 1e-4, **{skip: False})
        assert part["normal_image" if skip == "normal" else "n_samples"] is None
        for k, v in part.items():
            if v is not None:
                assert torch.equal(v, full[k]), (skip, k)
    none = oc.gpu_entry(net, sd, light, oc.RATIO, 1e-4, normal=False, count=False)
    assert torch.equal(none["image"], full["image"])
