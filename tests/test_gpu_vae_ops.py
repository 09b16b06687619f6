"""Every launch of the SD-VAE encode and decode plans on the GPU, stepped one op at a time through the C ABI (sf_plan_run of a single op)
and compared with float64 on the values the launch actually read: tests/vae_plan_cases.py.  The configurations are the smallest that reach
every kind of launch the canonical 256^2 plans hold at B = 1, 2 and 8 (tests/test_plans_vae_cpu.py asserts that they do), and k_gn_one on
GroupNorm(32) at B = 8.  Each case prints one margin line per launch; profiles/vae_op_parity_margins.log holds those of the first
recorded run."""
import pytest

import vae_plan_cases as vc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(vc.CONFIGS))
def test_every_launch_of_the_plans_on_gpu(name):
    vc.run_plan_case(name, "gpu")


@pytest.mark.parametrize("kind", list(vc.EXCEPTION_OPS))
def test_exception_kinds_on_the_128_channel_tile(kind):
    """The three kinds of launch of the canonical plans that no stepped configuration holds (vae_plan_cases.EXCEPTIONS), as hand-built ops at
    M = 256: the same decoder, references, bounds and guard."""
    vc.run_exception_case(kind, "gpu")
