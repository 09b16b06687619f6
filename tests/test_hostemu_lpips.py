"""Kernel-logic tests of the perceptual-loss kernels on CPU fibers: the cases of tests/lpips_cases.py (Part A: max pooling, the LPIPS heads,
ReLU backward on both operand types, the scaling layer) run the source of sparsefusion_amd/csrc/lpips_kernels.h through
tests/hostemu/lpips_emu.cpp -- the same shapes, planted inputs, sentinels, float64 references and derived bounds as on the GPU
(tests/test_gpu_lpips_ops.py).  The emulator's shuffles and __syncthreads() are rendezvous: a wave that diverges across one aborts the run.
No GPU."""
import pytest

import lpips_cases as lc
from hostemu import lpips_emu

pytestmark = pytest.mark.skipif(not lpips_emu.available(), reason="host clang not found")


@pytest.mark.parametrize("B,H,W,C", lc.POOL_SHAPES)
def test_pool_forward_and_backward_emulated(B, H, W, C):
    lc.run_pool_case("emu", B, H, W, C)


@pytest.mark.parametrize("V,HW,C", lc.HEAD_SHAPES)
def test_head_forward_emulated(V, HW, C):
    lc.run_head_fwd_case("emu", V, HW, C)


def test_two_heads_into_one_accumulator_emulated():
    lc.run_head_pair_case("emu")


@pytest.mark.parametrize("V,HW,C", lc.HEAD_SHAPES)
def test_head_backward_emulated(V, HW, C):
    lc.run_head_bwd_case("emu", V, HW, C)


@pytest.mark.parametrize("operand", ["bf16", "f16"])
@pytest.mark.parametrize("n", [4, 1028])
def test_relu_backward_emulated(n, operand):
    lc.run_relu_bwd_case("emu", n, operand)


@pytest.mark.parametrize("B,HW,Cp", lc.SCALE_SHAPES)
def test_scaling_layer_emulated(B, HW, Cp):
    lc.run_scale_case("emu", B, HW, Cp)


def test_a_bad_op_is_refused_not_run():
    with pytest.raises(RuntimeError, match="pool: H, W must be even"):
        lpips_emu.run([lc.mkop(lc.OP_POOL, 0, p=(1, None, None, 1), i=(1, 3, 2, 4))])
