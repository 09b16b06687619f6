"""Planner side of the 4x4-level compile-time-geometry kernels (csrc/fused_gca4.h), without a GPU: the switch gca4 is a bit mask over four kernel
families, default all on; it only ever SETS keep bits (pooling op field i[8] bit 0, fconv op flag 256, net0 op field i[5] bit 0), so the all-on
B = 1 op array carries none of them and the array at 0 is the same array plus exactly the keep bits of the seven launches concerned; plans of
B >= 2 and of the other models never change with the switch; the instantiated geometry of the host (SF_POOL4_C, SF_CONV4_1X1_*) is the canonical
B = 1 plan's."""
import functools
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@functools.lru_cache(maxsize=None)
def _net(dim=256):
    """One model per width for the whole module; every test leaves its switches at the defaults."""
    from sparsefusion_amd import unet as U
    return U.Unet(channels=4, dim=dim, dim_mults=(1, 2, 4, 4), num_resnet_blocks=(2, 2, 2, 2), layer_attns=(False, False, False, True),
                  layer_cross_attns=(False,) * 4, cond_images_channels=256, attn_pool_text=False)


def _ops(net, B):
    from sparsefusion_amd import unet as U
    return [(o.type, o.flags, list(o.i), list(o.f)) for o in U._Plan(net, B, CPU).build().ops]


def _keeps(ops):
    """(index, family) of every op that carries a keep bit of the switch; family as in sf_gca4_launches."""
    from sparsefusion_amd import unet as U
    out = []
    for k, (t, fl, i, _) in enumerate(ops):
        if t == U.OP_GCA and fl == 1 and i[8] & 1:
            out.append((k, 2 if ops[k - 1][0] == U.OP_FCONV and ops[k - 1][1] & 16 else 0))
        if t == U.OP_FCONV and fl & 256:
            out.append((k, 2 if fl & 16 else 1))
        if t == U.OP_GCA and fl == 2 and i[5] & 1:
            out.append((k, 3))
    return out


def _strip(ops):
    from sparsefusion_amd import unet as U
    out = []
    for t, fl, i, f in ops:
        i = list(i)
        if t == U.OP_GCA and fl == 1:
            i[8] &= ~1
        if t == U.OP_GCA and fl == 2:
            i[5] &= ~1
        out.append((t, fl & ~256 if t == U.OP_FCONV else fl, i, f))
    return out


def test_switch_is_declared_all_on():
    from sparsefusion_amd import unet as U
    assert dict((n, d) for n, d, _ in U.SWITCHES)["gca4"] == 15 and _net().gca4 == 15


def test_b1_plan_keep_bits():
    net = _net()
    on = _ops(net, 1)
    assert _keeps(on) == [] and _strip(on) == on                   # all on: no keep bit anywhere = the op array of a tree without the switch
    net.set_switches("gca4=0")
    off = _ops(net, 1)
    assert _strip(off) == on                                        # the keep bits are the whole difference
    fam = [f for _, f in _keeps(off)]
    assert sorted(fam) == [0, 0, 1, 2, 2, 2, 2, 3, 3]              # 2 poolings, 1 res_conv, 2 pairs (both ops), 2 net0
    for j in range(4):                                              # one bit = one family
        net.set_switches(f"gca4={15 ^ (1 << j)}")
        assert {f for _, f in _keeps(_ops(net, 1))} == {j}
    net.set_switches("gca4=15")
    assert _ops(net, 1) == on


def test_other_batches_and_models_never_change():
    net = _net()
    for B in (2, 4, 8, 16):
        on = _ops(net, B)
        net.set_switches("gca4=0")
        off = _ops(net, B)
        net.set_switches("gca4=15")
        assert off == on and _keeps(on) == [], B
    for dim in (128, 64):                                           # the test models: other channel counts, the host keeps the general kernels
        net = _net(dim)
        assert _keeps(_ops(net, 1)) == []


def test_host_geometry_is_the_canonical_plans():
    from sparsefusion_amd import unet as U
    txt = open(os.path.join(ROOT, "sparsefusion_amd", "csrc", "fused_host.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define (SF_POOL4_C|SF_CONV4_1X1_CIN|SF_CONV4_1X1_COUT) (\d+)", txt)}
    ops = _ops(_net(), 1)
    pools = [i for t, fl, i, _ in ops if t == U.OP_GCA and fl == 1]
    assert len(pools) == 4 and all(i[:8] == [16, const["SF_POOL4_C"], 16, 16, 1, 4 * const["SF_POOL4_C"] // 16, 4, const["SF_POOL4_C"]] for i in pools)
    convs = [(fl, i) for t, fl, i, _ in ops if t == U.OP_FCONV and i[1] == 4 and i[8] == 1 and i[12] == U.FNORM_NONE]
    assert [fl for fl, _ in convs] == [0, 16, 16]
    assert all(i[3] + i[4] == const["SF_CONV4_1X1_CIN"] and i[5] == i[6] == const["SF_CONV4_1X1_COUT"] and i[17] == 1 and i[7] == 0 for _, i in convs)
    net0 = [i for t, fl, i, _ in ops if t == U.OP_GCA and fl == 2 and not any(
        i[1] == c and i[4] <= n and (n == 8 or i[4] > n // 2) for c, n in ((256, 64), (256, 8), (512, 16), (512, 8), (1024, 8)))]
    assert len(net0) == 2 and all(i[:5] == [1, 256, 256, 128, 16] for i in net0)      # the only (C, chunks) pair without a row before: (256, 16)
