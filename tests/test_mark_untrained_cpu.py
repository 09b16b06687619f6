"""CPU tests of mark_untrained_grid (sf_occ_mark_untrained; sparsefusion_amd/csrc/occ_mark.h): the C ABI's declaration, signature,
symbol and argument checks against the built library; restatement (a) -- the kernel's float32 arithmetic, which the emulation and GPU
tests compare with bit for bit -- against the float64 restatement (b) of the reference's formula on scenes A-C at H = 128 and against
the golden of the reference's own function; poses_from_cameras against PinholeCameras.transform_points_ndc; the Python surface
without a device.  No GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import mark_untrained_common as mc

H = 128


# -------------------------------------------------------------------------------------------------------------------- 1. C ABI
def test_declaration_signature_and_symbol_agree():
    from sparsefusion_amd import _lib
    res, args = _lib.SIGNATURES["sf_occ_mark_untrained"]
    assert res is C.c_int and len(args) == 10
    assert [i for i, a in enumerate(args) if a is C.c_float] == [3] and [i for i, a in enumerate(args) if a is _lib.u32] == [2, 4, 5]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparsefusion_hip.h")).read()
    assert "int sf_occ_mark_untrained(const float* poses /* [B,4,4] c2w, row-major */, const float* intrinsics /* [B,4] fx fy cx cy */," in header
    assert "uint32_t B, float bound, uint32_t C /* cascades */, uint32_t H /* power of two */," in header
    assert "float* density_grid /* [C,H^3] in place */, int32_t* count /* [C,H^3] or NULL */," in header
    assert "uint32_t* n_marked /* 1 word, zeroed by the entry */, void* stream);" in header
    assert hasattr(_lib.lib(), "sf_occ_mark_untrained")                      # exported by the built library


def test_argument_checks_answer_without_a_device():
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 64)()
    pb = C.cast(buf, C.c_void_p)
    INVALID = 1

    def call(poses=pb, intr=pb, B=1, bound=4.0, Cc=3, Hh=128, grid=pb, count=pb, n=pb):
        return lib.sf_occ_mark_untrained(poses, intr, B, bound, Cc, Hh, grid, count, n, None)

    for name in ("poses", "intr", "grid", "n"):
        assert call(**{name: None}) == INVALID, name
        assert b"null tensor" in lib.sf_last_error()
    for name in ("grid", "n"):                                                   # also with no camera
        assert call(B=0, poses=None, intr=None, **{name: None}) == INVALID, name
    for Cc in (0, 17):
        assert call(Cc=Cc) == INVALID
        assert b"cascades" in lib.sf_last_error()
    for Hh in (0, 1, 3, 96, 127, 129, 2048):
        assert call(Hh=Hh) == INVALID, Hh
        assert b"power of two" in lib.sf_last_error()
    for bound in (0.0, -1.0, float("inf"), float("nan")):
        assert call(bound=bound) == INVALID, bound
        assert b"bound" in lib.sf_last_error()


# ------------------------------------------------------------------------------------------------------- 2. (a) against (b), H = 128
@pytest.fixture(scope="module")
def compared():
    """scene -> compare_a_b at H = 128 -- computed once, shared, never modified"""
    return {name: mc.compare_a_b(mc.scene(name), H) for name in mc.SCENES}


@pytest.mark.parametrize("name", sorted(mc.SCENES))
def test_float32_restatement_agrees_with_float64_outside_the_margin(compared, name):
    """Every pair whose float64 margin is at least 1e-5 is classified alike; at most 0.02 % of the pairs lie below it; both classes
    of cells are well populated (the fractions of the scene table, within two points)."""
    r = compared[name]
    frac = float((r["count_a"] == 0).float().mean())
    print(f"scene {name}: {r['pairs']} pairs, {r['excluded']} below the margin ({r['excluded'] / r['pairs']:.4%}), "
          f"{r['disagree_kept']} kept pairs disagree, {int(r['ambiguous'].sum())} ambiguous cells, marked {frac:.1%}")
    assert r["disagree_kept"] == 0
    assert r["excluded"] <= mc.EXCLUDED_MAX * r["pairs"]
    assert abs(frac - dict(A=0.59, B=0.59, C=0.33)[name]) < 0.02


# ----------------------------------------------------------------------------------------------------------- 3. (a) against the golden
def test_float32_restatement_reproduces_the_reference_golden(compared, golden_dir):
    G = torch.load(f"{golden_dir}/ngp_mark_untrained.pt")
    sc = mc.scene(mc.GOLDEN_SCENE)
    assert G["cfg"] == dict(scene=mc.GOLDEN_SCENE, H=H, **mc.SCENES[mc.GOLDEN_SCENE])
    assert torch.equal(G["poses"], sc["poses"]) and torch.equal(G["intrinsics"], sc["intrinsics"])
    assert torch.equal(G["rows"], mc.golden_rows(sc["C"] * H ** 3))
    r = compared[mc.GOLDEN_SCENE]
    amb = r["ambiguous"]
    print(f"golden: {G['n_marked']} marked, per cascade {G['per_cascade']}; cells holding an excluded pair and no kept covering pair: "
          f"{int(amb.sum())}")
    count = r["count_a"]
    exact = mc.check_against_golden(G, count, int((count == 0).sum()), ambiguous=amb)
    print("restatement (a) and the reference's float32 matmul mark the same cells" if exact else
          "restatement (a) and the reference's float32 matmul differ, on cells that hold an excluded pair only")


# ------------------------------------------------------------------------------------------------------------ 4. poses_from_cameras
def test_poses_from_cameras_frustum_contains_the_image():
    """Random cameras (rotation, translation, focal, principal point) and random world points: every point with z_cam > 0 and
    |ndc x|, |ndc y| < 1 under PinholeCameras.transform_points_ndc passes the marking test in the pose / intrinsics form with
    hg = 0, in float64 with the float32 poses."""
    from sparsefusion_amd.utils.cameras import PinholeCameras, poses_from_cameras
    g = torch.Generator().manual_seed(3)
    B, N = 6, 20000
    Q, _ = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))
    Q = Q * torch.sign(torch.linalg.det(Q))[:, None, None]
    T = torch.randn(B, 3, generator=g) + torch.tensor([0.0, 0.0, 3.0])
    focal = 1.5 + torch.rand(B, 2, generator=g)
    pp = 0.3 * (torch.rand(B, 2, generator=g) - 0.5)
    cams = PinholeCameras(Q, T, focal, pp)
    poses, K = poses_from_cameras(cams)
    assert poses.shape == (B, 4, 4) and K.shape == (B, 4) and poses.dtype == torch.float32 and K.dtype == torch.float32
    assert torch.equal(poses[:, :3, :3], cams.R) and torch.allclose(poses[:, :3, 3], cams.get_camera_center(), atol=1e-6)
    assert torch.equal(K[:, :2], focal) and torch.equal(K[:, 2:], 1 + pp.abs())
    pts = 4 * (torch.rand(1, N, 3, generator=g) - 0.5)
    ndc = cams.transform_points_ndc(pts)
    cam_ref = torch.bmm(pts.expand(B, -1, -1), cams.R) + cams.T[:, None]
    inside = (cam_ref[..., 2] > 1e-4) & (ndc[..., 0].abs() < 1 - 1e-5) & (ndc[..., 1].abs() < 1 - 1e-5)
    P = poses.double()
    cam = torch.bmm(pts.double().expand(B, -1, -1) - P[:, None, :3, 3], P[:, :3, :3])
    Kd = K.double()
    covered = (cam[..., 2] > 0) & (cam[..., 0].abs() < (Kd[:, 2] / Kd[:, 0])[:, None] * cam[..., 2]) & \
        (cam[..., 1].abs() < (Kd[:, 3] / Kd[:, 1])[:, None] * cam[..., 2])
    assert int(inside.sum()) > 1000 and bool(covered[inside].all())
    assert bool((~covered).any())                                               # the frustum is not everything
    # the same through restatement (a) on a small grid with hg2 = 0: a cell centre inside some image is counted
    Hs, bound = 16, 2.0
    cnt = mc.count_a(poses, K, bound, 1, Hs, zero_hg=True)[0]
    w = mc.unit_coords_a(Hs).t()
    s, _ = mc.cascade_consts_a(bound, 0, Hs)
    centres = (w * s)[None]
    ndc_c = cams.transform_points_ndc(centres)
    cam_c = torch.bmm(centres.expand(B, -1, -1), cams.R) + cams.T[:, None]
    seen = ((cam_c[..., 2] > 1e-3) & (ndc_c[..., 0].abs() < 1 - 1e-4) & (ndc_c[..., 1].abs() < 1 - 1e-4)).sum(0)
    assert int((seen > 0).sum()) > 100 and bool((cnt >= seen).all())


# --------------------------------------------------------------------------------------------------------------- 5. Python surface
def test_surface_without_a_device():
    from sparsefusion_amd.nerf import NeRFNetwork, NeRFRenderer, get_default_torch_ngp_opt
    sig = inspect.signature(NeRFRenderer.mark_untrained_grid)
    assert list(sig.parameters) == ["self", "poses", "intrinsic", "S", "return_count"]
    assert sig.parameters["S"].default == 64 and sig.parameters["return_count"].default is False
    doc = NeRFRenderer.mark_untrained_grid.__doc__
    assert "extension" in doc and "ignored" in doc
    opt = get_default_torch_ngp_opt()
    net = NeRFNetwork(opt)                                                      # cuda_ray=False: a no-op returning None, as the reference
    assert net.mark_untrained_grid(np.eye(4, dtype=np.float32)[None], [1.0, 1.0, 1.0, 1.0]) is None
    assert not hasattr(net, "density_grid")
    opt.cuda_ray = True
    occ = NeRFNetwork(opt)
    with pytest.raises(RuntimeError):                                           # there is no CPU path
        occ.mark_untrained_grid(torch.eye(4)[None], (1.0, 1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="intrinsics"):
        occ.mark_untrained_grid(torch.eye(4)[None].repeat(2, 1, 1), torch.ones(3, 4))
