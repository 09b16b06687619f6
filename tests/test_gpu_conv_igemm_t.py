"""k_conv_igemm_t (csrc/conv_igemm_t.h) on the GPU through the C ABI: every row of SF_IGEMM_T_VARIANTS is bit-identical to k_conv_igemm on
the same op (output, split-K workspace, statistics slots) and inside the per-element bound of the float64 reference that rounds where the
kernel rounds (tests/igemm_t_cases.py); the launch counter shows which kernel ran; a marked op without an instantiation runs on the general
kernel; the canonical B = 1 eval is bit-identical with the switch on and off."""
import pytest
import torch

import fused_cases as fc
import igemm_t_cases as ic
from sparsefusion_amd import _lib
from sparsefusion_amd import unet as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _op(flags, p, i):
    o = _lib.SfOp()
    o.type, o.flags = U.OP_CONV, flags
    for k, v in enumerate(p):
        o.p[k] = v.data_ptr() if v is not None else None
    for k, v in enumerate(i):
        o.i[k] = int(v)
    return o


def _run(op):
    n0 = _lib.lib().sf_conv_igemm_t_launches()
    fc.run_ops([op], "gpu")
    return _lib.lib().sf_conv_igemm_t_launches() - n0


def _variant(j, marked):
    """Runs variant j as the planner emits it (deferred split-K; the final conv with its NCHW reduction): (out, ws, slots, launches)."""
    g = ic.geometry(ic.VARIANTS[j])
    x, w, b = ic.operands(j)
    xd, wd, bd = x.to(DEV), ic.pack(w).to(DEV), b.to(DEV)
    nan = float("nan")
    if g["pixshuf"]:
        out = torch.full((4 * g["M"], g["Cout"] // 4), nan, device=DEV)
        slots = torch.full((4 * g["M"] // 16, g["Cout"] // 64, 2), nan, device=DEV)
        ws, flags, ldc = None, 1 | 2, g["Cout"] // 4
    else:
        nchw = g["Cout"] < 16                                                           # the final conv: its split-K reduction writes NCHW
        out, slots = torch.full((g["Cout"], g["M"]) if nchw else (g["M"], g["Cout"]), nan, device=DEV), None
        ws = torch.full((g["groups"], g["M"], g["npad"]), nan, device=DEV)
        flags, ldc = 1 | (256 if nchw else 8), g["Cout"]
    op = _op(flags | (512 if marked else 0), (xd, wd, bd, out, None, ws, None, slots),
             (1, g["H"], g["H"], g["Cin"], g["Ho"], g["Ho"], g["Cout"], ldc, 0, g["k"], g["k"], g["stride"], g["pad"], g["groups"], g["WM"] * 16 + g["WN"]))
    n = _run(op)
    return out.cpu(), None if ws is None else ws.cpu(), None if slots is None else slots.cpu(), n


@pytest.mark.parametrize("j", range(len(ic.VARIANTS)), ids=ic.IDS)
def test_variant_bit_identical_and_within_bound(j):
    g = ic.geometry(ic.VARIANTS[j])
    out_t, ws_t, slots_t, n_t = _variant(j, True)
    out_g, ws_g, slots_g, n_g = _variant(j, False)
    assert (n_t, n_g) == (1, 0)                                                         # the marked op ran k_conv_igemm_t, the other did not
    want, bound = ic.reference64(j, _lib.operand_dtype())
    if g["pixshuf"]:
        assert not torch.isnan(out_t).any() and not torch.isnan(slots_t).any()
        assert torch.equal(out_t, out_g) and torch.equal(slots_t, slots_g)
        got = out_t
    else:
        assert not torch.isnan(ws_t).any() and torch.equal(ws_t, ws_g)
        assert torch.equal(out_t, out_g) or (torch.isnan(out_t).all() and torch.isnan(out_g).all())       # deferred: nobody writes the output
        got = ws_t[:, :, :g["Cout"]].double().sum(0)
    ratio, msg = fc.check_elements(f"igemm_t variant {ic.IDS[j]}", got, want, bound, got.shape[1], 1, got.shape[0], 1, g["WM"], g["WN"], 0)
    print(f"variant {ic.IDS[j]}: worst err / bound {ratio:.3g}")
    assert msg is None, msg


def test_marked_op_without_an_instantiation_runs_on_the_general_kernel():
    gen = torch.Generator().manual_seed(7)
    H, Cin, Cout = 8, 64, 48
    x, w, b = torch.randn(H, H, Cin, generator=gen), torch.randn(Cout, Cin, 3, 3, generator=gen) / 24, torch.randn(Cout, generator=gen)
    xd, wd, bd = x.to(DEV), ic.pack(w).to(DEV), b.to(DEV)
    outs = []
    for flags in (1 | 512, 1):
        out = torch.full((H * H, Cout), float("nan"), device=DEV)
        n = _run(_op(flags, (xd, wd, bd, out, None, None, None, None), (1, H, H, Cin, H, H, Cout, Cout, 0, 3, 3, 1, 1, 1, 17)))
        assert n == 0
        outs.append(out.cpu())
    assert not torch.isnan(outs[0]).any() and torch.equal(outs[0], outs[1])
    want = torch.nn.functional.conv2d(fc.bf(x).permute(2, 0, 1)[None], fc.bf(w), b, padding=1)[0].permute(1, 2, 0).reshape(H * H, Cout)
    assert torch.allclose(outs[0], want, rtol=1e-4, atol=2e-4)


def test_canonical_eval_dispatch_and_bit_identity():
    net = U.Unet(channels=4, dim=256, dim_mults=(1, 2, 4, 4), num_resnet_blocks=(2, 2, 2, 2), layer_attns=(False, False, False, True),
                 layer_cross_attns=(False,) * 4, cond_images_channels=256, attn_pool_text=False).to(DEV)
    net.use_hip_graph = False                                                           # plain launches: the counter sees every eval
    gen = torch.Generator().manual_seed(3)
    x, cond = torch.randn(2, 4, 32, 32, generator=gen).to(DEV), torch.randn(2, 256, 32, 32, generator=gen).to(DEV)
    count = _lib.lib().sf_conv_igemm_t_launches

    def eval_b(B):
        ctx = net.begin_sampling(cond[:B], torch.linspace(-3, 3, 4, device=DEV))
        net.eval_prepared(ctx, x[:B], 1)                                                # (warm: plans built, weights packed)
        n0 = count()
        y = net.eval_prepared(ctx, x[:B], 1).clone()
        torch.cuda.synchronize()
        return y.cpu(), count() - n0

    y1, n1 = eval_b(1)
    _, n2 = eval_b(2)
    net.set_switches("igemm_t=0")
    y0, n0 = eval_b(1)
    assert (n1, n2, n0) == (7, 0, 0)
    assert torch.isfinite(y1).all() and torch.equal(y1, y0)
