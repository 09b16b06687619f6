"""GPU parity of the perceptual-loss kernels through the C ABI (sf_plan_run): the cases of tests/lpips_cases.py.

Part A: the eight small kernels of csrc/lpips_kernels.h, one op at a time, at the shapes where they can go wrong --
  pool (B, H, W, C): (1, 2, 2, 4) the smallest legal shape; (3, 6, 10, 64) non-square, work not a multiple of the workgroup; (2, 16, 16, 512);
    planted windows: the maximum at each position in each channel lane of a float4, ties, all-equal, all-zero, signed zeros;
  heads (V, HW, C): (1, 1, 64) lanes 16..63 idle; (2, 5, 128) a last workgroup with waves without a pixel; (3, 64, 256);
    (2, 16, 512) two channel trips; (1, 1100, 512) more than 1024 pixels: the 256-workgroup cap makes each wave stride;
  ReLU backward on both operand builds, the scaling layer and its gradient.
Part B: every launch of the LPIPS forward and backward plans, stepped one op at a time and compared with float64 on the values the launch
actually read (lpips_cases.run_plan_case), in the smallest configurations that reach every kind of launch the 256^2 plans hold
(tests/test_plans_lpips_cpu.py asserts that they do).  Each case prints its margins; profiles/lpips_op_parity_margins.log holds those of
the first recorded run."""
import pytest

import lpips_cases as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,W,C", lc.POOL_SHAPES)
def test_pool_forward_and_backward_on_gpu(B, H, W, C):
    lc.run_pool_case("gpu", B, H, W, C)


@pytest.mark.parametrize("V,HW,C", lc.HEAD_SHAPES)
def test_head_forward_on_gpu(V, HW, C):
    lc.run_head_fwd_case("gpu", V, HW, C)


def test_two_heads_into_one_accumulator_on_gpu():
    lc.run_head_pair_case("gpu")


@pytest.mark.parametrize("V,HW,C", lc.HEAD_SHAPES)
def test_head_backward_on_gpu(V, HW, C):
    lc.run_head_bwd_case("gpu", V, HW, C)


@pytest.mark.parametrize("operand", ["bf16", "f16"])
@pytest.mark.parametrize("n", [4, 1028])
def test_relu_backward_on_gpu(n, operand):
    lc.run_relu_bwd_case("gpu", n, operand)


@pytest.mark.parametrize("B,HW,Cp", lc.SCALE_SHAPES)
def test_scaling_layer_on_gpu(B, HW, Cp):
    lc.run_scale_case("gpu", B, HW, Cp)


@pytest.mark.parametrize("name", list(lc.PLAN_CONFIGS))
def test_every_launch_of_the_plans_on_gpu(name):
    lc.run_plan_case(name, "gpu")
