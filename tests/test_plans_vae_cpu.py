"""The configurations tests/test_gpu_vae_ops.py steps launch by launch (vae_plan_cases.CONFIGS) hold every kind of launch the canonical
256^2 SD-VAE plans hold at B = 1, 2 and 8 -- checked WITHOUT a GPU on plans built in sizing mode, as tests/test_plans_lpips_cpu.py does.
And the conditions on the float64 references alone, on the same stepping harness with the reference standing in for the launches."""
import pytest

import vae_plan_cases as vc
from oracle import vae_ref

MAX_EXCEPTIONS = 3          # a condition, not a measurement


def _ops(cfg, switches, B):
    return [o for plan in vc.sizing_plans(cfg, switches, B) for o in plan.ops]


@pytest.fixture(scope="module")
def held():
    """configuration -> the kinds of launch of its two plans"""
    return {name: {vc.launch_kind(o) for o in _ops(cfg, switches, B)} for name, (cfg, switches, B, _) in vc.CONFIGS.items()}


def test_every_kind_of_launch_of_the_canonical_plans_is_stepped_at_a_small_size(held):
    stepped = set().union(*held.values())
    canon = {vc.launch_kind(o) for B in vc.CANONICAL_BATCHES for o in _ops(vae_ref.CANONICAL, dict(), B)}
    assert len(canon) == 39, sorted(canon, key=str)
    missing = sorted(canon - stepped - set(vc.EXCEPTIONS), key=str)
    assert not missing, f"kinds of launch of the canonical plans that no stepped configuration holds: {missing}"
    # the exceptions: named, at most three, each still needed, each next to a stepped kind that differs in the channel-tile width alone, and each
    # run at a small size through the stepper's own decoder (test_gpu_vae_ops.py::test_exception_kinds_on_the_128_channel_tile)
    assert len(vc.EXCEPTIONS) <= MAX_EXCEPTIONS
    for kind, (near, where) in vc.EXCEPTIONS.items():
        assert kind in canon and kind not in stepped, f"{kind} is no exception (any more)"
        assert near in stepped and near[6] != kind[6] and near[:6] + near[7:] == kind[:6] + kind[7:], f"{kind}: {near} is not its stepped neighbour"
        assert kind in vc.EXCEPTION_OPS and where
    # the same instantiations as the exceptions run inside stepped configurations at other runtime geometries
    assert ("conv", 129, "lds", False, 3, 1, 8, False, False) in stepped          # k_conv_lds_gn<8, true>, the 3x3 form


def test_each_configuration_holds_the_kinds_it_is_listed_for(held):
    for name, (_, _, _, listed) in vc.CONFIGS.items():
        assert listed <= held[name], f"{name}: {sorted(listed - held[name], key=str)}"
    canon = {vc.launch_kind(o) for B in vc.CANONICAL_BATCHES for o in _ops(vae_ref.CANONICAL, dict(), B)}
    listed_all = set().union(*(c[3] for c in vc.CONFIGS.values()))
    assert canon - set(vc.EXCEPTIONS) <= listed_all, "a canonical kind is held by a configuration only by accident (not listed)"


def test_one_configuration_holds_k_gn_one_on_32_groups(held):
    """ADVICE.md, third item: k_gn_one on VAE GroupNorms (G = 32, 4 .. 16 channels per group) at B >= 8 -- the canonical plans take their
    statistics from the conv epilogues instead, so this is asked for on its own."""
    cfg, switches, B, _ = vc.CONFIGS["small_b8"]
    gns = [o for o in _ops(cfg, switches, B) if o.type == vc.OP_GN_ACT and vc.launch_kind(o)[2] == "k_gn_one"]
    assert B >= 8 and gns and all(o.i[8] == 32 and o.i[0] == B for o in gns)
    assert {vc.launch_kind(o)[5] for o in gns} == {4, 8}          # channels per group


def test_lds_tiled_convs_of_a_stepped_plan_on_cpu_fibers():
    """The smallest configuration on the LDS-tiled kernels with its k_conv_lds / k_conv_glds / k_conv3_halo launches run from the kernel
    source on CPU fibers (backend "emu", tests/hostemu/conv_lds_emu.cpp): the stepper's restatement of those launches -- the nearest-x2
    view, the accumulate form, the twin, the partials in each family's tile geometry -- meets the kernels without a GPU.  Without a host
    compiler the references stand in (backend "ref")."""
    from hostemu import fused
    vc.run_plan_case("small_lds_b1", "emu" if fused.available() else "ref")


@pytest.mark.parametrize("name", ["small_b3", "m44_r32_b1"])
def test_reference_conditions_and_wiring_without_a_gpu(name):
    """The stepping harness with the float64 reference in place of the launches (backend "ref", host memory): the decoding of every op
    record, the arena guard, the dataflow check, the chained references against oracle/vae_ref.py, and the conditions on the references
    alone -- median(bound) / rms(want) <= 1e-3 for every conv; every bf16 destination under MISMATCH_MAX when the rounded reference is
    compared with itself; the median over rows of max_j p_j * HW >= 2 in every attention; no GroupNorm group without variance."""
    kinds = vc.run_plan_case(name, "ref")
    assert vc.CONFIGS[name][3] <= kinds


@pytest.mark.parametrize("kind", list(vc.EXCEPTION_OPS))
def test_exception_ops_on_cpu_fibers(kind):
    from hostemu import fused
    vc.run_exception_case(kind, "emu" if fused.available() else "ref")
