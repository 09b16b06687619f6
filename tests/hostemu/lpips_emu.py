"""ctypes harness for tests/hostemu/lpips_emu.cpp: runs SF_OP_POOL / SF_OP_LPIPS / SF_OP_ELTWISE (7, 8, 9) ops of the product's kernel
source (sparsefusion_amd/csrc/lpips_kernels.h) on CPU fibers (host pointers).  One library per MFMA operand type ("bf16" | "f16": the
type k_relu_bwd writes).  Test infrastructure only."""
import ctypes as C
import os
import subprocess

from sparsefusion_amd import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "sparsefusion_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
_handles = {}


def available():
    return os.path.exists(CLANG)


def lib(operand="bf16"):
    if operand not in _handles:
        so = os.path.join(_HERE, "_build", f"liblpips_emu_{operand}.so")
        deps = [os.path.join(_HERE, f) for f in ("lpips_emu.cpp", "hip_emu.h")] + \
               [os.path.join(_CSRC, f) for f in ("lpips_kernels.h", "sf_dev.h", "sf_fix.h", "sf_operand.h")] + \
               [os.path.join(_HERE, "..", "..", "include", "sparsefusion_hip.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in deps):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + _HERE, "-Wall", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-Wno-source-uses-openmp", f"-DSF_OPERAND_F16={int(operand == 'f16')}", deps[0], "-o", so,
                                   "-lpthread"])
        h = C.CDLL(so)
        h.emu_lpips_plan_run.restype = C.c_int
        h.emu_lpips_plan_run.argtypes = [C.POINTER(_lib.SfOp), C.c_uint32, C.c_char_p, C.c_int]
        _handles[operand] = h
    return _handles[operand]


def run(ops, operand="bf16"):
    arr = (_lib.SfOp * len(ops))(*ops)
    err = C.create_string_buffer(512)
    if lib(operand).emu_lpips_plan_run(arr, len(ops), err, 512):
        raise RuntimeError(err.value.decode())
