"""k_conv_igemm_t (csrc/conv_igemm_t.h) against k_conv_igemm (csrc/conv_igemm.h) on CPU threads: for every row of SF_IGEMM_T_VARIANTS, on
random operands with bias (the k 4 / pad 1 and k 3 / pad 1 rows have out-of-image taps along every edge), output, split-K workspace and
statistics slots are torch.equal between the two kernels on the same ConvArgs, the general kernel's result is the convolution, and the
pixel-shuffle form writes every output element (NaN prefill)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import igemm_t_cases as ic
from hostemu import fused

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
SO = os.path.join(HERE, "_build", "libconv_igemm_t_emu" + "".join("_" + d.replace("=", "") for d in fused._DEFS) + ".so")
pytestmark = pytest.mark.skipif(not fused.available(), reason="host clang not found")


def _lib():
    csrc = os.path.join(HERE, "..", "..", "sparsefusion_amd", "csrc")
    srcs = [os.path.join(HERE, "conv_igemm_t_emu.cpp"), os.path.join(HERE, "hip_emu.h")] + \
           [os.path.join(csrc, f) for f in ("conv_igemm_t.h", "conv_igemm.h", "conv_lds.h", "conv_lds_body.inc", "sf_dev.h", "sf_operand.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call([fused.CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + HERE, "-Wall", "-Wno-unused-function",
                               "-ffp-contract=off"] + ["-D" + d for d in fused._DEFS] + [srcs[0], "-o", SO, "-lpthread"])
    return C.CDLL(SO)


def _run(lib, j, general):
    g = ic.geometry(ic.VARIANTS[j])
    x, w, b = ic.operands(j)
    wp = ic.pack(w)
    xa = x if g["a_f32"] else x.to(torch.bfloat16)
    nan = float("nan")
    if g["pixshuf"]:
        out = torch.full((4 * g["M"], g["Cout"] // 4), nan)
        slots = torch.full((4 * g["M"] // 16, g["Cout"] // 64, 2), nan)
        ws = None
    else:
        out, slots = torch.full((g["M"], g["Cout"]), nan), None
        ws = torch.full((g["groups"], g["M"], g["npad"]), nan)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    assert lib.emu_igemm_t_run(j, int(general), ptr(xa), ptr(wp), ptr(b), ptr(out), ptr(ws), ptr(slots)) == 0
    return out, ws, slots


@pytest.mark.parametrize("j", range(len(ic.VARIANTS)), ids=ic.IDS)
def test_variant_is_bit_identical_to_the_general_kernel(j):
    lib = _lib()
    g = ic.geometry(ic.VARIANTS[j])
    out_t, ws_t, slots_t = _run(lib, j, False)
    out_g, ws_g, slots_g = _run(lib, j, True)
    ref, _ = ic.reference64(j)
    if g["pixshuf"]:
        assert not torch.isnan(out_g).any() and not torch.isnan(out_t).any()             # every element written
        assert torch.equal(out_t, out_g) and torch.equal(slots_t, slots_g) and not torch.isnan(slots_t).any()
        assert torch.allclose(out_g.double(), ref, rtol=1e-4, atol=2e-4)                 # (the yardstick itself computes the layer)
    else:
        assert torch.isnan(out_t).all() and torch.isnan(out_g).all()                     # partial tiles only: the output is the reduction's
        assert not torch.isnan(ws_t).any() and torch.equal(ws_t, ws_g)
        assert torch.allclose(ws_g[:, :, :g["Cout"]].double().sum(0), ref, rtol=1e-4, atol=2e-4)
