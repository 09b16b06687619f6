"""Shared cases of the 4x4-level compile-time-geometry kernels (sparsefusion_amd/csrc/fused_gca4.h: k_gca_pool4_t, k_conv4_1x1_t, k_gca_pool4_rc_t)
and of the (256, 16) row of k_gca_net0_t.  Every case is ONE op (or one fconv + pooling pair) in the kernels' own geometry (16 pixels), run twice
on identical inputs: as the planner emits it (the new kernel) and with its keep bit set (the general kernel: k_gca_pool, k_conv_fused<1, 1, 12,
FNORM_NONE, 0, 8>, k_gca_pool_rc, k_gca_net0<16>).  Backend "emu" = both kernel sources on CPU threads (tests/hostemu/gca4_emu.cpp), "gpu" = the
C ABI (sf_plan_run).  The inputs are built once per case and shared by both runs; outputs start as NaN so an unwritten element shows."""
import ctypes as C
import functools
import os
import subprocess

import torch

import fused_cases as fc
from hostemu import fused
from sparsefusion_amd import _lib

OP_FCONV, OP_GCA = fc.OP_FCONV, fc.OP_GCA
POOL_C = 1024                        # SF_POOL4_C: the 4x4 channel count of the canonical UNet
CONV_CIN, CONV_COUT = 2048, 1024     # SF_CONV4_1X1_CIN / _COUT: its res_conv on the concat of two 1024-channel sources
FAMILIES = ("pool4", "conv4_1x1", "pool4_rc", "net0_256_16")        # index = family of sf_gca4_launches / emu_gca4_launches, bit of the switch gca4

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
_SO = os.path.join(_HERE, "_build", "libgca4_emu" + "".join("_" + d.replace("=", "") for d in fused._DEFS) + ".so")
_handle = None


def emu_lib():
    global _handle
    if _handle is None:
        csrc = os.path.join(_HERE, "..", "..", "sparsefusion_amd", "csrc")
        srcs = [os.path.join(_HERE, f) for f in ("gca4_emu.cpp", "hip_emu.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + \
               [os.path.join(_HERE, "..", "..", "include", "sparsefusion_hip.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(s) for s in srcs):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call([fused.CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + _HERE, "-Wall", "-Wno-unused-function",
                                   "-ffp-contract=off"] + ["-D" + d for d in fused._DEFS] + [srcs[0], "-o", _SO, "-lpthread"])
        _handle = C.CDLL(_SO)
        _handle.emu_gca4_run.restype = C.c_int
        _handle.emu_gca4_run.argtypes = [C.POINTER(_lib.SfOp), C.c_uint32, C.c_char_p, C.c_int]
    return _handle


def launches(backend):
    """Launch counters of the four families so far."""
    f = emu_lib().emu_gca4_launches if backend == "emu" else _lib.lib().sf_gca4_launches
    return tuple(int(f(k)) for k in range(4))


def run_ops(ops, backend):
    """Runs the ops; returns how many launches each family made."""
    n0 = launches(backend)
    if backend == "emu":
        arr = (_lib.SfOp * len(ops))(*ops)
        err = C.create_string_buffer(512)
        if emu_lib().emu_gca4_run(arr, len(ops), err, 512):
            raise RuntimeError(err.value.decode())
    else:
        fc.run_ops(ops, "gpu")
    return tuple(b - a for a, b in zip(n0, launches(backend)))


def _dev(backend):
    return "cpu" if backend == "emu" else "cuda:0"


# ---- pooling: M = HW = CH = 16, one chunk, nparts = 4 * C / 16; groups = 4 (lazy split-K source with row stride C) or 0 (materialised h2)
POOL_CASES = {f"g{g}_{'bias' if b else 'nobias'}_{'dominant' if d else 'random'}": dict(groups=g, bias=b, dominant=d)
              for g, b, d in ((4, True, False), (4, False, False), (0, False, False), (4, True, True), (0, False, True))}


@functools.lru_cache(maxsize=None)
def pool_inputs(groups, bias, dominant, seed=11):
    g = torch.Generator().manual_seed(seed + groups + 2 * bias + 4 * dominant)
    C = POOL_C
    nparts = 4 * C // 16
    lpart = torch.randn(nparts, 16, generator=g) * 0.2
    if dominant:
        lpart[:, 5] += 0.2                                    # pixel 5 wins by ~51: every other numerator is ~1e-22 of the sum
    h2 = torch.randn(16, C, generator=g)
    ws = torch.randn(4, 16, C, generator=g) if groups else None
    bv = torch.randn(C, generator=g) if (groups and bias) else None
    return lpart, h2, ws, bv


def pool_op(t, keep):
    return fused.mkop(OP_GCA, 1, p=(t["h2"], t["ws"], t["bias"], t["lpart"], t["pp"], t["pm"]),
                      i=(16, POOL_C, 16, 16, 1, 4 * POOL_C // 16, 4 if t["ws"] is not None else 0, POOL_C if t["ws"] is not None else 0, 1 if keep else 0))


def pool_tensors(backend, groups, bias, dominant):
    dev = _dev(backend)
    lpart, h2, ws, bv = pool_inputs(groups, bias, dominant)
    nan = float("nan")
    return dict(lpart=lpart.to(dev), h2=torch.full((16, POOL_C), nan, device=dev) if groups else h2.to(dev), ws=ws.to(dev) if groups else None,
                bias=bv.to(dev) if bv is not None else None, pp=torch.full((1, POOL_C), nan, device=dev), pm=torch.full((1, 2), nan, device=dev))


def run_pool(backend, keep, groups, bias, dominant):
    """(part_pool, part_ms, h2, launches per family)"""
    t = pool_tensors(backend, groups, bias, dominant)
    n = run_ops([pool_op(t, keep)], backend)
    return t["pp"].cpu(), t["pm"].cpu(), t["h2"].cpu(), n


def pool_reference(groups, bias, dominant):
    """float64: (h2, softmax-pooled row / sum of numerators)"""
    lpart, h2, ws, bv = pool_inputs(groups, bias, dominant)
    if groups:
        h2 = ws.double().sum(0) + (bv.double() if bv is not None else 0.0)
    sm = torch.softmax(lpart.double().sum(0), 0)
    return h2.double(), (sm[:, None] * h2.double()).sum(0)


# ---- the plain 1x1 conv: 16 pixels, concat of two plain sources (the second scaled by 2^-1/2), bias, with / without a residual
CONV_CASES = {"resid": dict(resid=True), "plain": dict(resid=False)}


@functools.lru_cache(maxsize=None)
def conv_inputs(seed=23):
    g = torch.Generator().manual_seed(seed)
    C1 = CONV_CIN // 2
    xa, xb = torch.randn(16, C1, generator=g) * 1.5 + 0.3, torch.randn(16, CONV_CIN - C1, generator=g)
    w = torch.randn(CONV_COUT, CONV_CIN, 1, 1, generator=g) / CONV_CIN ** 0.5
    return xa, xb, w, torch.randn(CONV_COUT, generator=g), torch.randn(16, CONV_COUT, generator=g)


def conv_tensors(backend, resid):
    dev = _dev(backend)
    xa, xb, w, b, r = conv_inputs()
    return dict(xa=xa.to(dev), xb=xb.to(dev), w=fused.pack_conv_weights(w, fc.opnd_dtype(backend)).to(dev), b=b.to(dev),
                r=r.to(dev) if resid else None, out=torch.full((16, CONV_COUT), float("nan"), device=dev))


def conv_op(t, keep, pair=False):
    C1 = t["xa"].shape[1]
    return fused.mkop(OP_FCONV, (16 if pair else 0) | (256 if keep else 0),
                      p=(t["xa"], None, None, None, None, t["xb"], None, t["w"], t["b"], t["out"], t["r"]),
                      i=(1, 4, 4, C1, CONV_CIN - C1, CONV_COUT, CONV_COUT, 0, 1, 0, 0, 0, fc.NONE, 8, 4, 1, 1, 1, 0), f=(1e-5, 1.0, 2 ** -0.5))


def run_conv(backend, keep, resid):
    t = conv_tensors(backend, resid)
    n = run_ops([conv_op(t, keep)], backend)
    return t["out"].cpu(), n


def conv_reference(backend, resid):
    """float64 on operands rounded as the kernel rounds them (the scale is one fp32 product, then the operand type)"""
    xa, xb, w, b, r = conv_inputs()
    dt = fc.opnd_dtype(backend)
    x = torch.cat([xa, xb * torch.tensor(2 ** -0.5, dtype=torch.float32)], 1).to(dt).double()
    y = x @ w[:, :, 0, 0].to(dt).double().t() + b.double()
    return y + r.double() if resid else y


def run_pair(backend, keep_pool, keep_conv, groups=4, bias=True):
    """res_conv || pooling in one launch: (res_conv output, part_pool, part_ms, h2, launches)"""
    tc, tp = conv_tensors(backend, False), pool_tensors(backend, groups, bias, False)
    n = run_ops([conv_op(tc, keep_conv, pair=True), pool_op(tp, keep_pool)], backend)
    return tc["out"].cpu(), tp["pp"].cpu(), tp["pm"].cpu(), tp["h2"].cpu(), n


# ---- net0 of a B = 1 plan's 16x16 down blocks: C = 256, 16 epilogue-pooled 16-pixel fragments, HID = 128
@functools.lru_cache(maxsize=None)
def net0_inputs(chunks, seed=31):
    g = torch.Generator().manual_seed(seed + chunks)
    C, HID = 256, 128
    pp, mj = torch.randn(chunks, C, generator=g) * 3, torch.randn(chunks, generator=g) * 2
    ms = torch.stack([mj, torch.rand(chunks, generator=g) * 8 + 1], 1).contiguous()
    return pp, ms, torch.randn(HID, C, generator=g) / C ** 0.5, torch.randn(HID, generator=g) * 0.1


def run_net0(backend, keep, chunks=16):
    dev = _dev(backend)
    pp, ms, W0, b0 = net0_inputs(chunks)
    t = dict(pp=pp.to(dev), ms=ms.to(dev), W0=W0.to(fc.opnd_dtype(backend)).contiguous().to(dev), b0=b0.to(dev),
             hid=torch.full((1, 128), float("nan"), device=dev))
    n = run_ops([fused.mkop(OP_GCA, 2, p=(t["pp"], t["ms"], t["W0"], t["b0"], t["hid"]), i=(1, 256, 256, 128, chunks, 1 if keep else 0))], backend)
    return t["hid"].cpu(), n


def net0_reference(backend, chunks=16):
    pp, ms, W0, b0 = net0_inputs(chunks)
    wj = (ms[:, 0].double() - ms[:, 0].double().max()).exp()
    pooled = (wj[:, None] * pp.double()).sum(0) / (wj * ms[:, 1].double()).sum()
    return torch.nn.functional.silu(pooled @ W0.to(fc.opnd_dtype(backend)).double().t() + b0.double())
