"""Planner side of k_conv_igemm_t (csrc/conv_igemm_t.h), without a GPU: unet.IGEMM_T_VARIANTS and SF_IGEMM_T_VARIANTS are one table in
one order (the switch igemm_t is a bit mask over its rows); the canonical B = 1 plan marks exactly its seven tile-code < 256 implicit
GEMMs (op flag 512), each with a geometry of the table; igemm_t = 0, single bits, B >= 2 and the other models' plans mark what they should."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _net():
    from sparsefusion_amd import unet as U
    return U.Unet(channels=4, dim=256, dim_mults=(1, 2, 4, 4), num_resnet_blocks=(2, 2, 2, 2), layer_attns=(False, False, False, True),
                  layer_cross_attns=(False,) * 4, cond_images_channels=256, attn_pool_text=False)


def _key(o):
    B, H, W, Cin, Ho, Wo, Cout, ldc, co_off, kh, kw, stride, pad, groups, tile = list(o.i)[:15]
    return (H.bit_length() - 1, Cin, Cout, kh, stride, pad, 1 if o.flags & 16 else 0, tile // 16, tile % 16, groups, o.flags & 1, 1 if o.flags & 2 else 0)


def test_variant_tables_agree():
    from sparsefusion_amd import unet as U
    txt = open(os.path.join(ROOT, "sparsefusion_amd", "csrc", "conv_igemm_t.h")).read()
    body = re.search(r"#define SF_IGEMM_T_VARIANTS\(X\)((?:\s*\\\n(?:\s*X\([^)]*\))+)+)", txt).group(1)
    host = tuple(tuple(int(v) for v in m.split(",")) for m in re.findall(r"X\(([^)]*)\)", body))
    assert host == U.IGEMM_T_VARIANTS and len(set(host)) == len(host)
    assert dict((n, d) for n, d, _ in U.SWITCHES)["igemm_t"] == (1 << len(host)) - 1


def test_b1_plan_marks_its_seven_and_nothing_else_is_marked():
    from sparsefusion_amd import unet as U
    net = _net()
    convs = lambda B: [o for o in U._Plan(net, B, CPU).build().ops if o.type == U.OP_CONV]
    body = lambda B: (lambda p: [p.body_array[k] for k in range(p.n_body_ops)])(U._Plan(net, B, CPU).build())
    small = [o for o in body(1) if o.type == U.OP_CONV and o.i[14] < 256]
    assert len(small) == 7 and all(o.flags & 512 for o in small)                       # every k_conv_igemm launch of the sampler's eval
    assert sorted(_key(o) for o in small) == sorted(U.IGEMM_T_VARIANTS)
    assert all(_key(o) in U.IGEMM_T_VARIANTS and o.i[0] == 1 for o in convs(1) if o.flags & 512)
    for B in (2, 4, 16):
        assert not any(o.flags & 512 for o in convs(B)), B
    for j, row in enumerate(U.IGEMM_T_VARIANTS):                                       # the per-variant mask
        net.set_switches(f"igemm_t={1 << j}")
        assert [_key(o) for o in convs(1) if o.flags & 512] == [row]
    net.set_switches("igemm_t=0")
    base = [(o.type, o.flags, list(o.i)) for o in U._Plan(net, 1, CPU).build().ops]
    assert not any(f & 512 for t, f, _ in base if t == U.OP_CONV)
    net.set_switches("igemm_t=127")
    marked = [(o.type, o.flags & ~512 if o.type == U.OP_CONV else o.flags, list(o.i)) for o in U._Plan(net, 1, CPU).build().ops]
    assert marked == base                                                              # the flag is the whole difference


def test_other_plan_owners_never_mark():
    from sparsefusion_amd import unet as U
    from sparsefusion_amd.lpips import LPIPS, _LpipsPlan
    from sparsefusion_amd.vae import AutoencoderKL, _VaePlan
    ops = list(_VaePlan(AutoencoderKL(), "dec", 1, CPU).build().ops) + list(_LpipsPlan(LPIPS(), 1, 256, CPU).build_forward().ops)
    assert ops and not any(o.type == U.OP_CONV and o.flags & 512 for o in ops)
