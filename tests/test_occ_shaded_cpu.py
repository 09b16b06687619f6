"""CPU tests of the shaded occupancy-grid evaluation render (run_cuda with shading='lambertian'; sf_ngp_render_occ_eval_shaded): the
golden of the real reference's render (tests/golden/make_golden_occ_shaded.py) against the CPU restatement the GPU tests derive their
bounds from, the Python surface without a device, and the C ABI's argument checks against the built library.  No GPU."""
import ctypes as C
import inspect
import os

import pytest
import torch

import occ_shaded_common as oc


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_occ_render_shaded.pt")


# ---------------------------------------------------------------------------------------------------------------- 1. the golden
def test_restatement_reproduces_reference_golden(golden):
    """One march_rays round at n_step = max_steps + oracle_attrs + np_normal + torch shading + composite_rays against the reference's
    own round loop: image within 1e-6 (shaded and albedo), weights_sum and depth within 1e-6; the scene holds what the GPU tests
    rely on (rays ended by T_thresh, none at the step cap, visible shading, a per-ray image bound below its cap)."""
    G = golden
    assert G["cfg"] == oc.CFG and G["ambient_ratio"] == oc.RATIO and G["bg_color"] == oc.BG and G["epsilon"] == oc.EPS
    assert torch.equal(G["light_d"], oc.unit(oc.LIGHT))
    sc = oc.golden_scene()
    rs = oc.restated(oc.params(), sc, G["light_d"], G["ambient_ratio"], G["cfg"]["T_thresh"])
    img, dep = oc.finish(sc, rs["image"], rs["depth"], rs["weights_sum"])
    img_a, dep_a = oc.finish(sc, rs["image_albedo"], rs["depth_albedo"], rs["weights_sum_albedo"])
    hit = sc["nears"] < sc["fars"]
    errs = dict(image=float((img - G["shaded"]["image"]).abs().max()), albedo_image=float((img_a - G["albedo"]["image"]).abs().max()),
                weights_sum=float((rs["weights_sum"] - G["shaded"]["weights_sum"]).abs().max()),
                depth=float((dep[hit] - G["shaded"]["depth"][hit]).abs().max()))
    bound = oc.image_bound(rs)
    ended = int(((rs["n_samples"] < rs["count"]) & (rs["count"] > 0)).sum())
    contrast = float((G["shaded"]["image"] - G["albedo"]["image"]).abs().mean())
    print(errs, f"hit {int((rs['count'] > 0).sum())} ended {ended} most samples {int(rs['count'].max())} contrast {contrast:.3f} "
                f"bound max {float(bound.max()):.2e}")
    assert all(e <= 1e-6 for e in errs.values()), errs
    assert torch.equal(G["shaded"]["weights_sum"], G["albedo"]["weights_sum"]) and \
        torch.equal(G["shaded"]["depth"][hit], G["albedo"]["depth"][hit])                 # they do not depend on the colour
    assert ended >= 1
    assert int(rs["count"].max()) < G["cfg"]["max_steps"]
    assert int((rs["count"] > 0).sum()) == 113
    assert contrast > 0.05
    assert float(bound.max()) <= oc.IMAGE_BOUND_CAP


# ------------------------------------------------------------------------------------------------------------ 2. Python surface
def _net(training):
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    opt = get_default_torch_ngp_opt()
    opt.cuda_ray = True
    return NeRFNetwork(opt).train(training)


def test_run_cuda_surface_without_a_device():
    from sparsefusion_amd.nerf import NeRFRenderer
    sig = inspect.signature(NeRFRenderer.run_cuda)
    assert list(sig.parameters) == ["self", "rays_o", "rays_d", "dt_gamma", "light_d", "ambient_ratio", "shading", "bg_color", "perturb",
                                    "force_all_rays", "max_steps", "T_thresh", "noise", "kwargs"]
    assert "lambertian" in NeRFRenderer.run_cuda.__doc__ and "extension" in NeRFRenderer.run_cuda.__doc__
    o, d = torch.zeros(1, 4, 3), torch.ones(1, 4, 3)
    light = torch.tensor([0.0, 0.0, 1.0])
    with pytest.raises(NotImplementedError, match="has no shaded form"):
        _net(True).run_cuda(o, d, shading='lambertian', light_d=light)
    for training in (True, False):
        for shading in ("textureless", "normal", "phong"):
            with pytest.raises(NotImplementedError):
                _net(training).run_cuda(o, d, shading=shading, light_d=light)
    ev = _net(False)
    with pytest.raises(RuntimeError, match="HIP device"):                       # there is no CPU path
        ev.run_cuda(o, d, shading='lambertian', light_d=light)
    with pytest.raises(RuntimeError, match="HIP device"):
        ev.run_cuda(o, d, shading='lambertian', light_d=(0.0, 0.0, 1.0))
    with pytest.raises(RuntimeError, match="HIP device"):
        ev.render_batched(o, d, batched=True, max_ray_batch=2, shading='lambertian', light_d=light)
    for bad in (torch.zeros(4), (1.0, 2.0), torch.zeros(2, 3)):
        with pytest.raises(ValueError, match="light_d must be a 3-vector"):
            ev.run_cuda(o, d, shading='lambertian', light_d=bad)


# -------------------------------------------------------------------------------------------------------------------- 3. C ABI
def test_occ_eval_shaded_abi_argument_checks():
    """The symbol is in the built library under the declared signature; every argument check runs before any device call, so it
    answers on a machine without a GPU: whatever sf_ngp_render_occ_eval rejects, a null light_d, a bad epsilon, a non-finite ratio,
    N >= 2^29 -> SF_ERR_INVALID; N == 0 -> SF_OK without a launch."""
    from sparsefusion_amd import _lib
    res, args = _lib.SIGNATURES["sf_ngp_render_occ_eval_shaded"]
    assert res is C.c_int and len(args) == 22 and args[0] is C.POINTER(_lib.SfNgpField)
    assert [i for i, a in enumerate(args) if a is C.c_float] == [6, 11, 14, 15]
    assert args[:13] == _lib.SIGNATURES["sf_ngp_render_occ_eval"][1][:13]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparsefusion_hip.h")).read()
    assert "int sf_ngp_render_occ_eval_shaded(const sf_ngp_field* f, const float* rays_o, const float* rays_d," in header
    assert "const float* light_d /* 3 floats ON THE DEVICE */, float ambient_ratio, float epsilon," in header
    assert "float* normal_image /* [N,3] sum w n, or NULL */, uint32_t* n_samples /* [N] samples composited, or NULL */," in header
    lib = _lib.lib()
    fn = lib.sf_ngp_render_occ_eval_shaded
    f = _lib.SfNgpField()
    buf = (C.c_float * 64)()
    pb = C.cast(buf, C.c_void_p)
    OK, INVALID = 0, 1

    def call(N=4, field=C.byref(f), o=pb, d=pb, nears=pb, fars=pb, grid=pb, max_steps=64, Cc=3, H=128, light=pb, ratio=0.1, eps=1e-2,
             ws=pb, depth=pb, image=pb, normal=pb, count=pb):
        return fn(field, o, d, nears, fars, grid, 0.0, max_steps, Cc, H, None, 1e-4, N, light, ratio, eps, ws, depth, image, normal,
                  count, None)

    assert call(light=None) == INVALID
    assert b"light_d" in lib.sf_last_error()
    for eps in (0.0, -1e-2, float("inf"), float("nan")):
        assert call(eps=eps) == INVALID, eps
        assert b"epsilon" in lib.sf_last_error()
    for ratio in (float("inf"), float("-inf"), float("nan")):
        assert call(ratio=ratio) == INVALID, ratio
        assert b"ambient_ratio" in lib.sf_last_error()
    for N in (1 << 29, (1 << 32) - 1):
        assert call(N=N) == INVALID, N
        assert b"2^29" in lib.sf_last_error()
    for name in ("field", "o", "d", "nears", "fars", "grid", "ws", "depth", "image"):       # what sf_ngp_render_occ_eval rejects
        assert call(**{name: None}) == INVALID, name
        assert b"null tensor" in lib.sf_last_error()
    for kw in (dict(Cc=0), dict(Cc=17), dict(H=0), dict(H=1025), dict(max_steps=0)):
        assert call(**kw) == INVALID, kw
        assert b"out of range" in lib.sf_last_error()
    assert call(N=0) == OK and call(N=0, o=None, image=None, Cc=0) == OK               # N == 0: nothing is read, nothing launched
    assert call(N=0, light=None) == INVALID and call(N=0, eps=0.0) == INVALID and call(N=0, ratio=float("nan")) == INVALID
