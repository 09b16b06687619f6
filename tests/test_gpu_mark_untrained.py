"""GPU tests of mark_untrained_grid: sf_occ_mark_untrained (sparsefusion_amd/csrc/occ_mark.h) against restatement (a) of
mark_untrained_common bit for bit -- the shapes, camera counts, `count` modes and pre-filled grids of the emulation tests, a non-default
stream, strided / CPU / numpy poses through the Python wrapper --; NeRFNetwork.mark_untrained_grid on scene B (bound 4, H = 128) against
the golden of the reference's own function; scene C (70 cameras) at H = 128 against (a); the integration with update_extra_state, the
marcher and reset_extra_state; the no-op without cuda_ray."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mark_untrained_common as mc

SHAPES, BOUND, cameras = mc.SHAPES, mc.SHAPE_BOUND, mc.shape_cameras

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 128


@pytest.fixture(scope="module")
def expected():
    """(H, C, B) -> cameras, pre-filled grid, count of restatement (a) on the CPU -- computed once, shared, never modified"""
    out = {}
    for Hs, C_, B in SHAPES:
        P, K = cameras(B, C_)
        out[Hs, C_, B] = dict(P=P, K=K, grid=mc.prefilled_grid(C_, Hs), count=mc.count_a(P, K, BOUND[C_], C_, Hs))
    return out


@pytest.mark.parametrize("with_count", (True, False))
@pytest.mark.parametrize("Hs,C_,B", SHAPES)
def test_entry_equals_the_restatement(expected, Hs, C_, B, with_count):
    from sparsefusion_amd import raymarching
    e = expected[Hs, C_, B]
    want_grid, want_n = mc.apply_a(e["grid"], e["count"])
    grid = e["grid"].to(DEV)
    r = raymarching.mark_untrained(e["P"].to(DEV), e["K"].to(DEV), BOUND[C_], grid, return_count=with_count)
    n, count = r if with_count else (r, None)
    assert n == want_n
    assert torch.equal(grid.cpu().view(torch.int32), want_grid.view(torch.int32))      # covered cells keep their bits, the others are -1
    if with_count:
        assert count.dtype == torch.int32 and torch.equal(count.cpu(), e["count"])
    if B == 0:
        assert n == C_ * Hs ** 3


def test_stream_and_pose_forms_through_the_wrapper(expected):
    """a non-default stream; poses as a strided device tensor, a CPU tensor and a numpy array; intrinsics as 4 numbers"""
    from sparsefusion_amd import raymarching
    Hs, C_, B = 32, 2, 3
    P = expected[Hs, C_, B]["P"]
    K4 = (300.0, 320.0, 64.0, 48.0)
    K = torch.tensor(K4).repeat(B, 1)
    want = mc.count_a(P, K, BOUND[C_], C_, Hs)
    want_grid, want_n = mc.apply_a(expected[Hs, C_, B]["grid"], want)
    wide = torch.zeros(B, 4, 8, device=DEV)
    wide[..., ::2] = P.to(DEV)
    strided = wide[..., ::2]
    assert not strided.is_contiguous()
    stream = torch.cuda.Stream()
    for poses, intr in ((strided, K4), (P, list(K4)), (P.numpy(), np.asarray(K4)), (P.to(DEV), torch.tensor(K4))):
        grid = expected[Hs, C_, B]["grid"].to(DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            n, count = raymarching.mark_untrained(poses, intr, BOUND[C_], grid, return_count=True)
        stream.synchronize()
        assert n == want_n and torch.equal(count.cpu(), want)
        assert torch.equal(grid.cpu().view(torch.int32), want_grid.view(torch.int32))


def _net(bound, p=None):
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    opt = get_default_torch_ngp_opt()
    opt.cuda_ray = True
    opt.bound = bound
    net = NeRFNetwork(opt)
    if p is not None:
        sd = net.state_dict()
        sd.update({k: p[k] for k in p if k in sd})
        net.load_state_dict(sd)
    return net.to(DEV), opt


def test_network_method_reproduces_the_reference_golden(golden_dir):
    """scene B, the project's default bound: returned n_marked, per-cascade counts, checksum and sampled rows equal the golden's (a
    difference would be allowed only on cells that hold an excluded pair, named by the float64 restatement -- computed only if
    needed); return_count=False and True leave the same grid; covered cells keep what they held."""
    G = torch.load(f"{golden_dir}/ngp_mark_untrained.pt")
    sc = mc.scene(mc.GOLDEN_SCENE)
    net, _ = _net(int(sc["bound"]))
    assert net.grid_size == H and net.cascade == sc["C"]
    net.density_grid.fill_(0.5)
    n, count = net.mark_untrained_grid(G["poses"], [float(v) for v in G["intrinsics"][0]], return_count=True)
    assert isinstance(n, int) and count.shape == (sc["C"], H ** 3) and count.dtype == torch.int32
    grid_true = net.density_grid.clone()
    count = count.cpu()
    try:
        mc.check_against_golden(G, count, n)
    except AssertionError:
        mc.check_against_golden(G, count, n, ambiguous=mc.compare_a_b(sc, H)["ambiguous"])
    assert torch.equal(grid_true.cpu(), torch.where(count == 0, torch.tensor(-1.0), torch.tensor(0.5)))
    net.density_grid.fill_(0.5)
    n2 = net.mark_untrained_grid(G["poses"].numpy(), G["intrinsics"], S=17)          # per-camera intrinsics, numpy poses, S ignored
    assert n2 == n and torch.equal(net.density_grid, grid_true)


def test_seventy_cameras_at_full_resolution():
    """scene C: 70 cameras in the loop, 8192 tiles for 2048 workgroups, with and without the early exit, against (a) evaluated with elementwise torch ops on the device"""
    from sparsefusion_amd import raymarching
    sc = mc.scene("C")
    want = mc.count_a(sc["poses"], sc["intrinsics"], sc["bound"], sc["C"], H, device=DEV)
    grid = torch.full((sc["C"], H ** 3), 2.0, device=DEV)
    n, count = raymarching.mark_untrained(sc["poses"], sc["intrinsics"], sc["bound"], grid, return_count=True)
    assert torch.equal(count, want) and n == int((want == 0).sum())
    assert 0.31 < n / want.numel() < 0.35
    grid2 = torch.full((sc["C"], H ** 3), 2.0, device=DEV)
    assert raymarching.mark_untrained(sc["poses"], sc["intrinsics"], sc["bound"], grid2) == n
    assert torch.equal(grid2, grid) and torch.equal(grid == -1, want == 0)


def test_marked_cells_stay_out_of_the_update_the_bitfield_and_the_march():
    from oracle import ngp_ref
    sc = mc.scene("B")
    p = ngp_ref.init_params(bound=4, seed=1, table_std=3.0, sigma_bias=1.0)               # a dense field: density everywhere
    net, opt = _net(4, p)
    C_ = net.cascade
    n, count = net.mark_untrained_grid(sc["poses"], sc["intrinsics"][0], return_count=True)
    marked = count == 0
    assert n == int(marked.sum()) and 0.5 < n / marked.numel() < 0.7
    g = torch.Generator().manual_seed(9)
    net.update_extra_state(noise=lambda t: torch.rand(t.shape, generator=g).to(t.device))
    assert bool((net.density_grid[marked] == -1).all()) and bool((net.density_grid[~marked] > 0).all())
    bits = ((net.density_bitfield[:, None] >> torch.arange(8, device=DEV, dtype=torch.uint8)) & 1).reshape(C_, H ** 3).bool()
    assert not bool(bits[marked].any()) and bool(bits[~marked].any())
    assert net.mean_density == torch.mean(net.density_grid.clamp(min=0).reshape(-1)).item()
    assert abs(net.mean_density - torch.mean(net.density_grid.clamp(min=0)).item()) <= 1e-6 * net.mean_density
    # rays of a camera outside the training set, along the top edge of the box; a ray qualifies when every point of its span, at a
    # spacing of a third of the finest cell, lies -- in every cascade that contains it -- in a cell whose 3 x 3 x 3 neighbourhood is marked
    cells = mc.cells(H).to(DEV)
    lin = torch.empty(H, H, H, dtype=torch.long, device=DEV)
    lin[cells[:, 0], cells[:, 1], cells[:, 2]] = torch.arange(H ** 3, device=DEV)
    unmarked = (~marked)[:, lin.reshape(-1)].reshape(C_, 1, H, H, H).float()
    near_unmarked = F.max_pool3d(unmarked, 3, 1, 1).reshape(C_, H, H, H) > 0
    gr = torch.Generator().manual_seed(4)
    N = 256
    o = torch.tensor([-3.9, 3.4, -3.6]) + 0.3 * torch.rand(N, 3, generator=gr)
    d = torch.tensor([1.0, 0.0, 0.1]) + 0.6 * (torch.rand(N, 3, generator=gr) - 0.5)
    d = d / d.norm(dim=-1, keepdim=True)
    o, d = o.to(DEV), d.to(DEV)
    t = torch.arange(0.0, 16.0, 2.0 / H / 3, device=DEV)
    pts = o[:, None] + t[None, :, None] * d[:, None]                                  # [N, T, 3]
    inside = (pts.abs() <= 4.0).all(-1)
    clear = torch.ones(N, dtype=torch.bool, device=DEV)
    for cas in range(C_):
        b = min(2.0 ** cas, 4.0)
        within = inside & (pts.abs() <= b).all(-1)
        c = ((pts / b + 1) * 0.5 * H).floor().long().clamp(0, H - 1)
        hit = near_unmarked[cas][c[..., 0], c[..., 1], c[..., 2]] & within
        clear &= ~hit.any(-1)
    assert int(clear.sum()) >= 16, (int(clear.sum()), N)
    net.eval()
    kw = dict(vars(opt))
    with torch.no_grad():
        r = net.run_cuda(o[None], d[None], perturb=False, bg_color=0, shading='albedo', **kw)
    ws = r["weights_sum"].reshape(-1)
    assert bool((ws[clear] == 0).all())
    # reset_extra_state clears the marks: the same rays then meet the dense field
    net.reset_extra_state()
    assert bool((net.density_grid == 0).all())
    net.train()
    net.update_extra_state(noise=lambda t: torch.rand(t.shape, generator=g).to(t.device))
    assert bool((net.density_grid > 0).all())
    net.eval()
    with torch.no_grad():
        r2 = net.run_cuda(o[None], d[None], perturb=False, bg_color=0, shading='albedo', **kw)
    ws2 = r2["weights_sum"].reshape(-1)[clear]
    # (not all of them: packbits keeps only the cells above min(mean_density, density_thresh), a ray may thread the others)
    assert float((ws2 > 0).float().mean()) > 0.5


def test_without_cuda_ray_it_is_a_no_op_that_allocates_nothing():
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    net = NeRFNetwork(get_default_torch_ngp_opt()).to(DEV)
    poses = mc.ring_cameras(3, 2.0).to(DEV)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert net.mark_untrained_grid(poses, (300.0, 300.0, 64.0, 64.0)) is None
    assert net.mark_untrained_grid(poses, (300.0, 300.0, 64.0, 64.0), return_count=True) is None
    assert torch.cuda.memory_allocated() == before and not hasattr(net, "density_grid")
