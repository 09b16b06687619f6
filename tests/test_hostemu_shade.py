"""Kernel-logic tests of the shaded render on CPU fibers (sparsefusion_amd/csrc/ngp_shade.h through tests/hostemu/shade_emu.cpp):
k_ngp_shade and k_ngp_composite_sorted_wave on sorted rays taken from the oracle's albedo render (ngp_ref.render_run), for the
teacher and the default-init field; then the golden of the real reference's shading='lambertian' render against the oracle
restatement the GPU tests derive their bounds from; then the Python surface and the C ABI's argument checks.  No GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import point_attrs_common as pc
import shaded_common as sc
from ngp_common import params_from_cfg

SHAPES = [(5, 64), (3, 7), (1, 4)]            # T = 64 fills the wave; 2T = 14 and 8 leave most lanes dead; partial 4-ray workgroups
LIGHT = (0.3, -0.5, 0.81)
RATIO, BG = 0.1, 0.25
needs_clang = pytest.mark.skipif(not sc.emu_available(), reason="host clang not found")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_render.pt")


@pytest.fixture(scope="module")
def shaded_golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_render_shaded.pt")


def _light():
    l = torch.tensor(LIGHT, dtype=torch.float32)
    return l / l.norm()


@pytest.fixture(scope="module")
def cases(golden):
    """(field, N, T) -> oracle restatement + emulated kernels at RATIO and at ratio 1 -- computed once, shared, never modified"""
    out = {}
    light = _light()
    for name in ("teacher", "default_init"):
        p = params_from_cfg(golden[name]["cfg"])
        for N, T in SHAPES:
            o, d = sc.small_rays(N)
            g = torch.Generator().manual_seed(100 * N + T)
            uc, uf = torch.rand(N, T, generator=g), torch.rand(N, T, generator=g)
            rs = sc.restated(p, o, d, light, RATIO, BG, uc, uf, training=True, T=T)
            aux = rs["aux"]
            sh = {r: sc.emu_shade(p, o, d, p["aabb_train"], aux["z_sorted"], aux["rgb_sorted"], light, r) for r in (RATIO, 1.0)}
            co = {r: sc.emu_composite_sorted(aux["z_sorted"], aux["sigma_sorted"], sh[r]["rgb_shaded_s"], sh[r]["normal_s"], d,
                                             aux["nears"], aux["fars"], BG) for r in (RATIO, 1.0)}
            out[name, N, T] = dict(p=p, o=o, d=d, rs=rs, shade=sh, comp=co)
    return out


# -------------------------------------------------------------------------------------------------------- 1. per-sample outputs
@needs_clang
@pytest.mark.parametrize("N,T", SHAPES)
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_emulated_shade_points_normals_and_colour(cases, name, N, T):
    """Per sorted sample: the point is the float32 min(max(o + d z, lo), hi) of the oracle, bit for bit; the normal is the one
    k_ngp_point_attrs' emulation gives at that point, bit for bit (the six offset evaluations are the same code), and within the
    bounds of test_point_attrs_cpu.py of the oracle's (2 r + 1e-6 where r = |bound| / |gradient| <= 5e-2); the shaded colour is the
    numpy float32 restatement applied to the emulated normal, bit for bit.  Every element is written (NaN pre-fill); the 2 x 256
    emulated threads walk N * 2T = 640 samples in two rounds with a tail, 42 and 8 samples with idle threads.  On the default-init
    field no sample has r <= 5e-2 (its gradients are below the density tolerance): the oracle comparison is empty there and the
    bit-level anchors carry it."""
    c = cases[name, N, T]
    rs, sh = c["rs"], c["shade"][RATIO]
    aux = rs["aux"]
    for k in ("normal_s", "rgb_shaded_s", "xyz_s"):
        assert not torch.isnan(sh[k]).any(), k
    x = sh["xyz_s"].reshape(-1, 3)
    assert np.array_equal(pc.bits(x), pc.bits(rs["x"]))
    assert np.array_equal(pc.bits(x), pc.bits(sc.np_points(c["o"], c["d"], aux["z_sorted"], c["p"]["aabb_train"]).reshape(-1, 3)))
    attrs = pc.emu_point_attrs(c["p"], x.contiguous(), sc.EPS, sigma=False, albedo=False, grad=False)
    assert np.array_equal(pc.bits(attrs["normal"]), pc.bits(sh["normal_s"].reshape(-1, 3)))
    r = rs["r"].reshape(-1)
    keep = r <= 5e-2
    dn = np.linalg.norm(sh["normal_s"].reshape(-1, 3).double().numpy() - rs["normal"].reshape(-1, 3).double().numpy(), axis=1)
    worst = float((dn[keep] / (2 * r[keep] + 1e-6)).max()) if keep.any() else 0.0
    print(f"{name} N={N} T={T}: {100 * keep.mean():.1f} % of the samples compared, max |n - n_ref| / (2 r + 1e-6) = {worst:.3f}")
    assert (dn[keep] <= 2 * r[keep] + 1e-6).all()
    if name == "teacher" and T == 64:
        assert keep.mean() > 0.5                                # the oracle comparison is not empty where the field has a surface
    want = sc.np_shade(aux["rgb_sorted"].numpy(), sh["normal_s"].numpy(), _light().numpy(), RATIO)
    assert np.array_equal(pc.bits(want), pc.bits(sh["rgb_shaded_s"]))
    no_xyz = sc.emu_shade(c["p"], c["o"], c["d"], c["p"]["aabb_train"], aux["z_sorted"], aux["rgb_sorted"], _light(), RATIO, blocks=3,
                          xyz=False)
    assert no_xyz["xyz_s"] is None
    for k in ("normal_s", "rgb_shaded_s"):                      # another grid, the nullable output skipped: same values
        assert np.array_equal(pc.bits(no_xyz[k]), pc.bits(sh[k])), k


# ------------------------------------------------------------------------------------------------------------------ 2. the sums
@needs_clang
@pytest.mark.parametrize("N,T", SHAPES)
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_emulated_composite_sums(cases, name, N, T):
    """image, depth, weights_sum, normal image and orientation sum within 1e-5 of a front-to-back float32 loop over the same sorted
    ray and the same per-sample colours / normals; the miss ray composites to the background with a NaN depth; null outputs are
    skipped and leave the others unchanged."""
    c = cases[name, N, T]
    aux, sh, got = c["rs"]["aux"], c["shade"][RATIO], c["comp"][RATIO]
    ref = sc.np_composite(aux["z_sorted"], aux["sigma_sorted"], sh["rgb_shaded_s"], sh["normal_s"], c["d"], aux["nears"], aux["fars"],
                          T, BG)
    for k, want in zip(("image", "depth", "weights_sum", "normal_image", "orient"), ref):
        a = got[k].numpy()
        live = ~np.isnan(want)
        assert np.array_equal(np.isnan(a), ~live), k
        err = float(np.abs(a[live] - want[live]).max())
        assert err <= 1e-5, (k, err)
    if N > 1:
        m = N - 2
        assert bool(torch.isnan(got["depth"][m])) and float(got["weights_sum"][m]) == 0.0
        assert torch.equal(got["image"][m], torch.full((3,), BG)) and float(got["orient"][m]) == 0.0
    # against the oracle restatement (torch float32, normals of the oracle): the albedo render's 1e-5 on depth / weights_sum
    assert torch.allclose(got["weights_sum"], c["rs"]["weights_sum"], rtol=0, atol=1e-5)
    for skip in ("normal_image", "orient"):
        part = sc.emu_composite_sorted(aux["z_sorted"], aux["sigma_sorted"], sh["rgb_shaded_s"], sh["normal_s"], c["d"], aux["nears"],
                                       aux["fars"], BG, **{skip: False})
        assert part[skip] is None
        for k in got:
            if k != skip:
                assert np.array_equal(pc.bits(part[k]), pc.bits(got[k])), (skip, k)


@needs_clang
@pytest.mark.parametrize("N,T", SHAPES)
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_ratio_one_is_the_albedo_composite_bit_for_bit(cases, name, N, T):
    """ambient_ratio = 1: lambertian is exactly 1, the shaded colour is the albedo's bits, and image / depth / weights_sum of
    k_ngp_composite_sorted_wave equal k_ngp_composite_wave's on the same ray bit for bit -- same arithmetic, same order."""
    c = cases[name, N, T]
    aux, sh, got = c["rs"]["aux"], c["shade"][1.0], c["comp"][1.0]
    assert np.array_equal(pc.bits(sh["rgb_shaded_s"]), pc.bits(aux["rgb_sorted"]))
    assert np.array_equal(pc.bits(sh["normal_s"]), pc.bits(c["shade"][RATIO]["normal_s"]))
    alb = sc.emu_composite_wave(aux["z_sorted"], aux["sigma_sorted"], aux["rgb_sorted"], aux["nears"], aux["fars"], BG)
    assert np.array_equal(pc.bits(alb["z_s"]), pc.bits(aux["z_sorted"]))            # fed sorted: the rank sort is the identity
    for k in ("image", "depth", "weights_sum"):
        assert np.array_equal(pc.bits(got[k]), pc.bits(alb[k])), k
    for k in ("depth", "weights_sum", "normal_image", "orient"):                       # and they do not depend on the ratio
        assert np.array_equal(pc.bits(got[k]), pc.bits(c["comp"][RATIO][k])), k


# ---------------------------------------------------------------------------------------------------------------- 3. the golden
@pytest.mark.parametrize("case", ["eval", "train"])
def test_oracle_restatement_reproduces_reference_golden(golden, shaded_golden, case):
    """The real reference's shading='lambertian' render (tests/golden/make_golden_shaded.py) against the restatement composed from
    ngp_ref.render_run + oracle_attrs + np_normal: image within 1e-6, loss_orient within 1e-6 relative; depth and weights_sum are
    the albedo render's."""
    G = shaded_golden
    cfg = G["cfg"]
    assert cfg == golden["teacher"]["cfg"]
    p = params_from_cfg(cfg)
    o, d = sc.golden_rays(cfg)
    assert torch.equal(o, golden["teacher"]["rays_o"]) and torch.equal(d, golden["teacher"]["rays_d"])
    uc, uf = sc.golden_draws(G[case]["noise_seed"], o.shape[0]) if case == "train" else (None, None)
    rs = sc.restated(p, o, d, G["light_d"], G["ambient_ratio"], G["bg_color"], uc, uf, training=case == "train")
    err = float((rs["image"] - G[case]["image"]).abs().max())
    rel = abs(float(rs["loss_orient"]) - float(G[case]["loss_orient"])) / float(G[case]["loss_orient"])
    contrast = float((rs["image"] - rs["image_albedo"]).abs().mean())
    print(f"{case}: image {err:.2e}, loss_orient rel {rel:.2e}, shaded - albedo mean {contrast:.3f}")
    assert err <= 1e-6 and rel <= 1e-6
    live = ~torch.isnan(G[case]["depth"])
    assert int((~live).sum()) == 1
    assert torch.allclose(rs["depth"][live], G[case]["depth"][live], rtol=0, atol=1e-6)
    assert torch.allclose(rs["weights_sum"], G[case]["weights_sum"], rtol=0, atol=1e-6)
    assert contrast > 0.05                                      # the shading is visible in this scene
    assert float(sc.image_bound(rs, G["ambient_ratio"]).max()) <= 1e-2      # the GPU test's derived bound is not vacuous here


# ------------------------------------------------------------------------------------------------------------ 4. Python surface
def _net(trainable):
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    net = NeRFNetwork(get_default_torch_ngp_opt())
    for q in net.parameters():
        q.requires_grad_(trainable)
    return net


def test_run_signature_and_unsupported_shadings_raise():
    from sparsefusion_amd.nerf import NeRFRenderer
    sig = inspect.signature(NeRFRenderer.run)
    assert list(sig.parameters) == ["self", "rays_o", "rays_d", "num_steps", "upsample_steps", "light_d", "ambient_ratio", "shading",
                                    "bg_color", "perturb", "fixed_light", "noise", "kwargs"]
    assert "loss_smooth" in NeRFRenderer.run.__doc__ and "extension" in NeRFRenderer.run.__doc__
    net = _net(False)
    o, d = torch.zeros(1, 4, 3), torch.ones(1, 4, 3)
    for shading in ("textureless", "normal"):
        with pytest.raises(NotImplementedError, match="smooth normal"):
            net.run(o, d, num_steps=8, upsample_steps=8, shading=shading)
        with pytest.raises(NotImplementedError):
            net.run_cuda(o, d, shading=shading)
    with pytest.raises(NotImplementedError):
        net.run_cuda(o, d, shading='lambertian')
    with pytest.raises(NotImplementedError):
        net.run(o, d, num_steps=8, upsample_steps=8, shading='phong')


def test_shaded_run_needs_no_grad_or_a_frozen_field():
    trainable = _net(True)
    o, d = torch.zeros(1, 4, 3), torch.ones(1, 4, 3)
    with pytest.raises(NotImplementedError, match="the shaded render has no backward"):
        trainable.run(o, d, num_steps=8, upsample_steps=8, shading='lambertian', light_d=torch.tensor([0.0, 0.0, 1.0]))
    # allowed combinations get past that check and stop at the device check: there is no CPU path
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="HIP device"):
            trainable.run(o, d, num_steps=8, upsample_steps=8, shading='lambertian', light_d=torch.tensor([0.0, 0.0, 1.0]))
    with pytest.raises(RuntimeError, match="HIP device"):
        _net(False).run(o, d, num_steps=8, upsample_steps=8, shading='lambertian', light_d=(0.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="3-vector"):
        _net(False).run(o, d, num_steps=8, upsample_steps=8, shading='lambertian', light_d=torch.zeros(4))


# -------------------------------------------------------------------------------------------------------------------- 5. C ABI
def test_shaded_render_abi_argument_checks():
    """The symbols are in the built library under the declared signatures; the argument checks run before any device call, so they
    answer on a machine without a GPU: null light_d, a bad epsilon, a non-finite ratio, T out of range, a short workspace ->
    SF_ERR_INVALID; N == 0 -> SF_OK."""
    from sparsefusion_amd import _lib
    res, args = _lib.SIGNATURES["sf_ngp_render_shaded_forward"]
    assert res is C.c_int and len(args) == 31 and args[0] is C.POINTER(_lib.SfNgpField)
    assert [i for i, a in enumerate(args) if a is C.c_float] == [6, 11, 13, 14]
    assert _lib.SIGNATURES["sf_ngp_render_shaded_workspace_bytes"] == (C.c_uint64, [C.c_uint32, C.c_uint32])
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparsefusion_hip.h")).read()
    assert "int sf_ngp_render_shaded_forward(const sf_ngp_field* f, const float* rays_o, const float* rays_d, const float* aabb," in header
    assert "const float* light_d,\n" in header and "float ambient_ratio, float epsilon, float* nears" in header
    lib = _lib.lib()
    assert lib.sf_ngp_render_shaded_workspace_bytes(256, 64) == lib.sf_ngp_render_forward_workspace_bytes(256, 64) == 10 * 256 * 64 * 4
    fn = lib.sf_ngp_render_shaded_forward
    f = _lib.SfNgpField()
    buf = (C.c_float * 64)()
    pb = C.cast(buf, C.c_void_p)
    OK, INVALID = 0, 1

    def call(N=4, T=8, light=pb, ratio=0.1, eps=1e-2, wbytes=1 << 20, normal_s=pb):
        return fn(C.byref(f), pb, pb, pb, N, T, 0.1, pb, None, pb, 0, 1.0, light, ratio, eps, pb, pb, pb, pb, pb, normal_s, pb, None,
                  pb, None, None, pb, pb, pb, wbytes, None)

    assert call(light=None) == INVALID
    assert b"light_d" in lib.sf_last_error()
    for eps in (0.0, -1e-2, float("inf"), float("nan")):
        assert call(eps=eps) == INVALID, eps
        assert b"epsilon" in lib.sf_last_error()
    for ratio in (float("inf"), float("-inf"), float("nan")):
        assert call(ratio=ratio) == INVALID, ratio
        assert b"ambient_ratio" in lib.sf_last_error()
    for T in (0, 3, 65):
        assert call(T=T) == INVALID, T
        assert b"T must be" in lib.sf_last_error()
    assert call(wbytes=10 * 4 * 8 * 4 - 1) == INVALID
    assert b"workspace" in lib.sf_last_error()
    assert call(normal_s=None) == INVALID
    assert b"null pointer" in lib.sf_last_error()
    assert call(N=0) == OK and call(N=0, T=1000, wbytes=0) == OK
    assert call(N=0, light=None) == INVALID and call(N=0, eps=0.0) == INVALID            # the value checks come before N == 0
