"""Operands of the k_conv_igemm_t variants (csrc/conv_igemm_t.h), shared by the CPU-emulation and the GPU tests: one seeded random case per
row of unet.IGEMM_T_VARIANTS at the instantiated geometry (compile-time geometry: there is no smaller shape the kernel could run)."""
import functools

import torch
import torch.nn.functional as F

from sparsefusion_amd import unet as U

VARIANTS = U.IGEMM_T_VARIANTS
IDS = ["x".join(str(v) for v in row) for row in VARIANTS]


def geometry(row):
    hl, cin, cout, k, stride, pad, ups, wm, wn, groups, a_f32, epi = row
    H = 1 << hl
    Ho = (H + 2 * pad - k) // stride + 1
    return dict(H=H, Ho=Ho, M=Ho * Ho, Cin=cin, Cout=cout, k=k, stride=stride, pad=pad, ups=ups, WM=wm, WN=wn, groups=groups, a_f32=a_f32,
                pixshuf=epi == 1, npad=(cout + 15) // 16 * 16)


@functools.lru_cache(maxsize=None)
def operands(j):
    """(x NHWC fp32 [H, H, Cin], w [Cout, Cin, k, k], bias [Cout]) of variant j; built once, never modified."""
    g = geometry(VARIANTS[j])
    gen = torch.Generator().manual_seed(1000 + j)
    x = torch.randn(g["H"], g["H"], g["Cin"], generator=gen)
    w = torch.randn(g["Cout"], g["Cin"], g["k"], g["k"], generator=gen) / (g["Cin"] * g["k"] * g["k"]) ** 0.5
    b = torch.randn(g["Cout"], generator=gen)
    return x, w, b


def pack(w, dtype=None):
    """The packed B operand of the library ([n_frag][k-step][lane][8], operand type) as an int16 tensor."""
    from sparsefusion_amd import _lib as L
    lib = L.lib()
    co, ci, kh, kw = w.shape
    assert ci % 32 == 0
    buf = torch.empty(lib.sf_conv_packed_elems(co, ci, kh, kw), dtype=torch.int16)
    L.check(lib.sf_conv_pack_weights(w.contiguous().data_ptr(), co, ci, ci, kh, kw, buf.data_ptr()))
    return buf


def reference64(j, dt=torch.bfloat16):
    """(want, bound) in float64 on operands rounded where the kernel rounds (fp32 -> operand type `dt` for A and B; the rounding is of
    exactly known fp32 values, so there is no tie allowance): the conv [M, Cout] without bias for a split-K variant (its slabs, summed
    exactly, are compared), the pixel-shuffled SiLU(conv + bias) [4 M, Cout / 4] otherwise.  The bound is the one of tests/fused_cases.py:
    (b) accumulation in any order, c u sum |a b| with c = ceil(K / (128 S)) + 32 + 8 + S; the bias add is one more rounding on |y|; SiLU
    carries d(y) through its local slope, + d(y)^2 / 4, + (|y| + 6) u |s| for the exponential, the add, the division and the product."""
    import math
    from fused_cases import U24
    g = geometry(VARIANTS[j])
    x, w, b = operands(j)
    rnd = lambda t: t.to(dt).double()
    xi, wi = rnd(x).permute(2, 0, 1)[None], rnd(w)
    conv = F.conv2d(xi, wi, None, stride=g["stride"], padding=g["pad"])
    mag = F.conv2d(xi.abs(), wi.abs(), None, stride=g["stride"], padding=g["pad"])
    S = g["groups"]
    c = math.ceil(g["Cin"] * g["k"] * g["k"] / (128 * S)) + 32 + 8 + S
    rows = lambda t: t[0].permute(1, 2, 0).reshape(g["M"], g["Cout"])
    if not g["pixshuf"]:
        return rows(conv), c * U24 * rows(mag)
    y = conv + b.double()[None, :, None, None]
    dy = c * U24 * mag + U24 * y.abs()
    sg = torch.sigmoid(y)
    sv = y * sg
    ds = (sg * (1 + y * (1 - sg))).abs() * dy + dy * dy / 4 + (y.abs() + 6) * U24 * sv.abs()
    shuf = lambda t: F.pixel_shuffle(t, 2)[0].permute(1, 2, 0).reshape(4 * g["M"], g["Cout"] // 4)
    return shuf(sv), shuf(ds)
