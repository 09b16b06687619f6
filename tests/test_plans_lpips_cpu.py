"""The configurations tests/test_gpu_lpips_ops.py steps launch by launch (lpips_cases.PLAN_CONFIGS) hold every kind of launch the 256^2
plans of the benchmark hold -- checked WITHOUT a GPU on plans built in sizing mode (fake device pointers), as tests/test_plans_cpu.py does.
And the conditions on the float64 reference alone (a bound tight enough to see an error, non-trivial taps and distance), on the same
stepping harness with the reference standing in for the launches."""
import pytest

import lpips_cases as lc

CPU = "cpu"


def _sizing_plans(switches, V, R):
    from sparsefusion_amd.lpips import _LpipsPlan
    net = lc.make_module(switches, CPU)
    fwd = _LpipsPlan(net, V, R, CPU).build_forward()
    return fwd, _LpipsPlan(net, V, R, CPU, fwd=fwd).build_backward()


def _keys(switches, V, R):
    fwd, bwd = _sizing_plans(switches, V, R)
    return {lc.op_key(o) for plan in (fwd, bwd) for o in plan.ops}, [o for plan in (fwd, bwd) for o in plan.ops]


@pytest.fixture(scope="module")
def covered():
    """key -> the configurations that hold it; and per configuration the conv families of its plans"""
    out, fams = {}, {}
    for name, (switches, V, R, _) in lc.PLAN_CONFIGS.items():
        keys, ops = _keys(switches, V, R)
        for k in keys:
            out.setdefault(k, []).append(name)
        fams[name] = {(lc.conv_family(o), lc.conv_has_twin(o)) for o in ops if o.type == lc.OP_CONV}
    return out, fams


@pytest.mark.parametrize("V", [1, 2])
def test_every_kind_of_launch_of_the_256_plans_is_stepped_at_a_small_size(covered, V):
    keys, ops = _keys(dict(), V, 256)
    missing = sorted(k for k in keys if k not in covered[0])
    assert not missing, f"(op type, flags, conv kernel family, twin) of the V = {V}, R = 256 plans that no stepped configuration holds: {missing}"
    # the 256^2 plans themselves: LDS-tiled and halo kernels with and without twins next to the implicit-GEMM tail, every small kernel
    fams = {(k[2], k[3]) for k in keys if k[0] == lc.OP_CONV}
    assert fams == {("lds", True), ("halo", False), ("halo", True), ("igemm", False)}
    assert {(k[0], k[1]) for k in keys if k[0] != lc.OP_CONV} == {(lc.OP_MEMSET, 0), (lc.OP_ELTWISE, 8), (lc.OP_ELTWISE, 7), (lc.OP_ELTWISE, 4),
                                                                 (lc.OP_ELTWISE, 9), (lc.OP_POOL, 0), (lc.OP_POOL, 1), (lc.OP_LPIPS, 0),
                                                                 (lc.OP_LPIPS, 1), (lc.OP_LPIPS, 2)}
    # What the key does not distinguish, stated so that it cannot grow unseen: the 128-channel workgroup tile (tile code 264) of the two
    # relu2 layers needs >= 256 such tiles, i.e. 32768 output rows -- no plan smaller than the 256^2 one has it.  Those instantiations
    # (k_conv_lds<8>, k_conv3_halo<8, ..>) share every line of source with the 64-channel ones stepped here; the 128-channel tile is
    # run at its own shapes by tests/test_gpu_unet_ops.py (test_conv_lds_tiled and the k_conv3_halo cases with bnf = 8: whole-tensor norm)
    # and tests/test_hostemu_conv_lds.py -- it has no per-element float64 check.
    wide = {(lc.conv_family(o), o.i[14]) for o in ops if o.type == lc.OP_CONV and o.i[14] >= 256 and (o.i[14] & 15) == 8}
    assert wide == {("lds", 264), ("halo", 264)}
    small_tiles = {o.i[14] & 15 for name in lc.PLAN_CONFIGS for o in _keys(*lc.PLAN_CONFIGS[name][:3])[1] if o.type == lc.OP_CONV and o.i[14] >= 256}
    assert small_tiles == {4}


def test_each_configuration_holds_the_kernel_families_it_is_there_for(covered):
    for name, (_, _, _, families) in lc.PLAN_CONFIGS.items():
        assert covered[1][name] == families, f"{name}: {sorted(covered[1][name])}"
    # (3, 16): a 1x1 map at the last tap -- HW = 1 in the head and a 2x2 -> 1x1 pool
    _, ops = _keys(dict(), 3, 16)
    assert any(o.type == lc.OP_LPIPS and o.flags == 0 and o.i[1] == 1 for o in ops) and any(o.type == lc.OP_POOL and o.i[1] == 2 for o in ops)


@pytest.mark.parametrize("name", ["default_v1_r32", "default_v3_r16", "lds_v2_r32"])
def test_reference_conditions_and_wiring_without_a_gpu(name):
    """The stepping harness with the float64 reference in place of the launches (backend "ref", host memory): the decoding of every op record,
    the dataflow check, and the conditions on the reference alone -- median(bound) / rms <= 1e-3 for every conv, forward and backward-data,
    on every kernel family's addition count; >= 25 % non-zero features at every tap; a distance > 1e-3."""
    keys = lc.run_plan_case(name, "ref")
    assert any(k[0] == lc.OP_CONV for k in keys)
