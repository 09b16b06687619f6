"""The 4x4-level compile-time-geometry kernels (csrc/fused_gca4.h) and the (256, 16) row of k_gca_net0_t against the general kernels on CPU
threads (tests/gca4_cases.py, tests/hostemu/gca4_emu.cpp): on identical inputs every output -- part_pool, part_ms and the written-back h2 of the
pooling, the 1x1 conv's output, net0's hidden vector -- is torch.equal between the two kernels, every element is written (NaN prefill), the
launch counters show which kernel ran, and the general kernel's result is the op (a float64 reference; the yardstick computes the layer)."""
import pytest
import torch

import gca4_cases as gc
from hostemu import fused

pytestmark = pytest.mark.skipif(not fused.available(), reason="host clang not found")
BACKEND = "emu"


@pytest.mark.parametrize("case", sorted(gc.POOL_CASES))
def test_pool4_is_bit_identical_to_gca_pool_body(case):
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
def test_conv4_1x1_is_bit_identical_to_conv_fused_body(case):
    kw = gc.CONV_CASES[case]
    out_t, n_t = gc.run_conv(BACKEND, False, **kw)
    out_g, n_g = gc.run_conv(BACKEND, True, **kw)
    assert n_t == (0, 1, 0, 0) and n_g == (0, 0, 0, 0)
    assert not torch.isnan(out_t).any() and torch.equal(out_t, out_g)
    assert torch.allclose(out_g.double(), gc.conv_reference(BACKEND, **kw), rtol=1e-4, atol=2e-4)


@pytest.mark.parametrize("groups", (4, 0))
def test_pool4_rc_pair_is_bit_identical_to_gca_pool_rc(groups):
    new = gc.run_pair(BACKEND, False, False, groups=groups, bias=bool(groups))
    old = gc.run_pair(BACKEND, True, True, groups=groups, bias=bool(groups))
    assert new[4] == (0, 0, 1, 0) and old[4] == (0, 0, 0, 0)
    for a, b in zip(new[:4], old[:4]):
        assert not torch.isnan(a).any() and torch.equal(a, b)
    assert gc.run_pair(BACKEND, True, False, groups=groups, bias=bool(groups))[4] == (0, 0, 0, 0)         # either keep bit keeps the whole launch general
    assert gc.run_pair(BACKEND, False, True, groups=groups, bias=bool(groups))[4] == (0, 0, 0, 0)
    assert torch.equal(new[0], gc.run_conv(BACKEND, True, resid=False)[0])                                  # the conv half = the stand-alone conv


def test_net0_row_256_16_is_bit_identical_to_gca_net0():
    for chunks in (16, 9):
        hid_t, n_t = gc.run_net0(BACKEND, False, chunks)
        hid_g, n_g = gc.run_net0(BACKEND, True, chunks)
        assert n_t == (0, 0, 0, 1) and n_g == (0, 0, 0, 0)
        assert not torch.isnan(hid_t).any() and torch.equal(hid_t, hid_g)
        assert torch.allclose(hid_g[0].double(), gc.net0_reference(BACKEND, chunks), rtol=2e-4, atol=2e-5)
