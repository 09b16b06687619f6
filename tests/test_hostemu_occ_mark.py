"""Kernel-logic tests of the camera-coverage culling on CPU fibers: k_occ_mark_untrained (sparsefusion_amd/csrc/occ_mark.h through
tests/hostemu/occ_mark_emu.cpp) against restatement (a) of mark_untrained_common, bit for bit -- counts, grid and n_marked.  Shapes:
H = 4 (64 cells: one wave of a 256-lane workgroup, the rest idle), 8, 32; C = 1, 2, 3; B = 0, 1, 3, 70 and 130 (130: two camera chunks in LDS,
restaged per cascade and tile); with and without `count` (the early-exit path must mark the same cells).  The emulator's ballot, shuffle and
__syncthreads() are rendezvous: a lane that returned early or a wave that skipped a barrier aborts the run.  No GPU."""
import pytest
import torch

import mark_untrained_common as mc

pytestmark = pytest.mark.skipif(not mc.emu_available(), reason="host clang not found")

SHAPES, BOUND, cameras = mc.SHAPES, mc.SHAPE_BOUND, mc.shape_cameras


@pytest.fixture(scope="module")
def expected():
    """(H, C, B) -> cameras, pre-filled grid, count of restatement (a) -- computed once, shared, never modified"""
    out = {}
    for H, C_, B in SHAPES:
        P, K = cameras(B, C_)
        out[H, C_, B] = dict(P=P, K=K, grid=mc.prefilled_grid(C_, H), count=mc.count_a(P, K, BOUND[C_], C_, H))
    return out


@pytest.mark.parametrize("with_count", (True, False))
@pytest.mark.parametrize("H,C_,B", SHAPES)
def test_emulated_kernel_equals_the_restatement(expected, H, C_, B, with_count):
    e = expected[H, C_, B]
    want_grid, want_n = mc.apply_a(e["grid"], e["count"])
    grid, count, n = mc.emu_mark(e["P"], e["K"], BOUND[C_], e["grid"], with_count)
    assert n == want_n
    assert torch.equal(grid.view(torch.int32), want_grid.view(torch.int32))          # covered cells keep their bits, the others are -1
    if with_count:
        assert torch.equal(count, e["count"])
    if B == 0:
        assert n == C_ * H ** 3 and bool((grid == -1).all())
    elif H >= 8:
        assert 0 < want_n < C_ * H ** 3                                           # both classes are populated


@pytest.mark.parametrize("with_count", (True, False))
@pytest.mark.parametrize("H,C_,B,blocks", [(32, 3, 70, 5), (32, 2, 3, 128 // 3), (8, 3, 1, 1), (8, 2, 130, 1)])
def test_fewer_workgroups_than_tiles_stride_over_them(expected, H, C_, B, blocks, with_count):
    """the launch at 128^3 has 8192 tiles for 1024 workgroups; here 128 tiles for 5 (an uneven tail) or 42, and 2 tiles for 1"""
    e = expected[H, C_, B]
    want_grid, want_n = mc.apply_a(e["grid"], e["count"])
    grid, count, n = mc.emu_mark(e["P"], e["K"], BOUND[C_], e["grid"], with_count, max_blocks=blocks)
    assert n == want_n and torch.equal(grid.view(torch.int32), want_grid.view(torch.int32))
    if with_count:
        assert torch.equal(count, e["count"])


def test_prefill_holds_all_three_kinds_and_covered_cells_keep_them(expected):
    e = expected[8, 3, 1]
    covered = e["count"] > 0
    g = e["grid"][covered]
    assert bool((g == 0).any()) and bool((g > 0).any()) and bool((g == -1).any())
    grid, _, _ = mc.emu_mark(e["P"], e["K"], 4.0, e["grid"], False)
    assert torch.equal(grid[covered].view(torch.int32), g.view(torch.int32))


def test_cam_z_zero_is_not_covered():
    """A camera at the origin looking along +z with a 90-degree-wide frustum: the cell centres of the plane z = 0 do not exist for an
    even H, so the camera sits at a cell-centre plane instead: t_z = p_z of cell layer 5 (the float32 the kernel forms), R = I.  That
    whole layer has cam_z == 0 exactly and must be uncovered (z > 0 is strict) although |cam_x| < hg2 holds for the cells near the
    axis; the layer above it is covered near the axis."""
    H, C_, bound = 8, 1, 1.0
    w = mc.unit_coords_a(H)
    s, hg2 = mc.cascade_consts_a(bound, 0, H)
    pz = (w * s)[2]
    layer = mc.cells(H)[:, 2]
    tz = pz[layer == 5][0]
    assert bool((pz[layer == 5] == tz).all())
    P = torch.eye(4).reshape(1, 4, 4).clone()
    P[0, 2, 3] = tz
    K = torch.tensor([[1.0, 1.0, 1.0, 1.0]])
    grid, count, n = mc.emu_mark(P, K, bound, torch.zeros(C_, H ** 3), True)
    assert torch.equal(count, mc.count_a(P, K, bound, C_, H))
    assert bool((count[0][layer == 5] == 0).all()) and bool((grid[0][layer == 5] == -1).all())
    assert bool((count[0][layer == 6] == 1).any()) and bool((count[0][layer <= 5] == 0).all())
    assert n == int((count == 0).sum())
