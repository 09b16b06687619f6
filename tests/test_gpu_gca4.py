"""The 4x4-level compile-time-geometry kernels (csrc/fused_gca4.h) and the (256, 16) row of k_gca_net0_t on the GPU through the C ABI: the cases
of tests/gca4_cases.py are torch.equal between the new kernel and the general one (selected by the op's keep bit), the launch counters show
which kernel ran; one canonical B = 1 eval is torch.equal with the switch gca4 all on and at 0 and really launches the seven new kernels; a
dim-64 eval (no geometry of the table: 256-channel 4x4 maps, no 16-fragment net0 of 256 channels) and a B = 2 eval launch none of them and do not change with the switch."""
import pytest
import torch

import gca4_cases as gc
from sparsefusion_amd import unet as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BACKEND = "gpu"


@pytest.mark.parametrize("case", sorted(gc.POOL_CASES))
def test_pool4_bit_identical(case):
    kw = gc.POOL_CASES[case]
    pp_t, pm_t, h2_t, n_t = gc.run_pool(BACKEND, False, **kw)
    pp_g, pm_g, h2_g, n_g = gc.run_pool(BACKEND, True, **kw)
    assert n_t == (1, 0, 0, 0) and n_g == (0, 0, 0, 0)
    for t in (pp_t, pm_t, h2_t):
        assert not torch.isnan(t).any()
    assert torch.equal(pp_t, pp_g) and torch.equal(pm_t, pm_g) and torch.equal(h2_t, h2_g)
    h2_ref, pooled_ref = gc.pool_reference(**kw)
    assert torch.allclose(h2_g.double(), h2_ref, rtol=1e-5, atol=1e-5)
    assert torch.allclose(pp_g[0].double() / pm_g[0, 1].double(), pooled_ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("case", sorted(gc.CONV_CASES))
def test_conv4_1x1_bit_identical(case):
    kw = gc.CONV_CASES[case]
    out_t, n_t = gc.run_conv(BACKEND, False, **kw)
    out_g, n_g = gc.run_conv(BACKEND, True, **kw)
    assert n_t == (0, 1, 0, 0) and n_g == (0, 0, 0, 0)
    assert not torch.isnan(out_t).any() and torch.equal(out_t, out_g)
    assert torch.allclose(out_g.double(), gc.conv_reference(BACKEND, **kw), rtol=1e-4, atol=2e-4)


@pytest.mark.parametrize("groups", (4, 0))
def test_pool4_rc_pair_bit_identical(groups):
    new = gc.run_pair(BACKEND, False, False, groups=groups, bias=bool(groups))
    old = gc.run_pair(BACKEND, True, True, groups=groups, bias=bool(groups))
    assert new[4] == (0, 0, 1, 0) and old[4] == (0, 0, 0, 0)
    for a, b in zip(new[:4], old[:4]):
        assert not torch.isnan(a).any() and torch.equal(a, b)
    assert gc.run_pair(BACKEND, True, False, groups=groups, bias=bool(groups))[4] == (0, 0, 0, 0)
    assert gc.run_pair(BACKEND, False, True, groups=groups, bias=bool(groups))[4] == (0, 0, 0, 0)


def test_net0_row_256_16_bit_identical():
    for chunks in (16, 9):
        hid_t, n_t = gc.run_net0(BACKEND, False, chunks)
        hid_g, n_g = gc.run_net0(BACKEND, True, chunks)
        assert n_t == (0, 0, 0, 1) and n_g == (0, 0, 0, 0)
        assert not torch.isnan(hid_t).any() and torch.equal(hid_t, hid_g)
        assert torch.allclose(hid_g[0].double(), gc.net0_reference(BACKEND, chunks), rtol=2e-4, atol=2e-5)


def _eval(net, x, cond, B):
    ctx = net.begin_sampling(cond[:B], torch.linspace(-3, 3, 4, device=DEV))
    net.eval_prepared(ctx, x[:B], 1)                                                    # (warm: plans built, weights packed)
    n0 = gc.launches(BACKEND)
    y = net.eval_prepared(ctx, x[:B], 1).clone()
    torch.cuda.synchronize()
    return y.cpu(), tuple(b - a for a, b in zip(n0, gc.launches(BACKEND)))


def _net(dim):
    net = U.Unet(channels=4, dim=dim, dim_mults=(1, 2, 4, 4), num_resnet_blocks=(2, 2, 2, 2), layer_attns=(False, False, False, True),
                 layer_cross_attns=(False,) * 4, cond_images_channels=256, attn_pool_text=False).to(DEV)
    net.use_hip_graph = False                                                           # plain launches: the counters see every eval
    return net


def test_canonical_eval_dispatch_and_bit_identity():
    net = _net(256)
    gen = torch.Generator().manual_seed(3)
    x, cond = torch.randn(2, 4, 32, 32, generator=gen).to(DEV), torch.randn(2, 256, 32, 32, generator=gen).to(DEV)
    y1, n1 = _eval(net, x, cond, 1)
    y2, n2 = _eval(net, x, cond, 2)
    net.set_switches("gca4=0")
    y0, n0 = _eval(net, x, cond, 1)
    y20, n20 = _eval(net, x, cond, 2)
    assert n1 == (2, 1, 2, 2) and n0 == n2 == n20 == (0, 0, 0, 0)
    assert torch.isfinite(y1).all() and torch.equal(y1, y0) and torch.equal(y2, y20)


def test_dim64_eval_falls_through_to_the_general_kernels():
    net = _net(64)
    gen = torch.Generator().manual_seed(4)
    x, cond = torch.randn(1, 4, 32, 32, generator=gen).to(DEV), torch.randn(1, 256, 32, 32, generator=gen).to(DEV)
    y1, n1 = _eval(net, x, cond, 1)
    net.set_switches("gca4=0")
    y0, n0 = _eval(net, x, cond, 1)
    assert n1 == n0 == (0, 0, 0, 0)
    assert torch.isfinite(y1).all() and torch.equal(y1, y0)
