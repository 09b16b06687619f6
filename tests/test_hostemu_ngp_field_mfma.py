"""Kernel-logic test of the matrix-core field-forward kernel (sparsefusion_amd/csrc/ngp_field_mfma.h) on CPU threads against the
per-point math of k_ngp_field (ngp_encode + ngp_mlp_forward + activations of ngp_device.h): z, sigma, rgb and the field-cache
rows must be EQUAL, bit for bit, in both modes -- the emulated sf_mfma4 is the k-ordered fmaf chain the hardware instruction is
documented to be, so this pins the kernel's own logic: lane / fragment maps, k order, bias as the initial accumulator, the
in-place H2, the grid stride, dead lanes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import ngp_ref
from hostemu import fused

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
SO = os.path.join(HERE, "_build", "libngp_field_mfma_emu.so")
pytestmark = pytest.mark.skipif(not fused.available(), reason="host clang not found")
FLT_MAX = 3.402823466e+38


def _lib():
    srcs = [os.path.join(HERE, "ngp_field_mfma_emu.cpp"), os.path.join(HERE, "hip_emu.h"), os.path.join(HERE, "ngp_emu_common.h")] + \
           [os.path.join(HERE, "..", "..", "sparsefusion_amd", "csrc", f) for f in ("ngp_field_mfma.h", "ngp_device.h", "sf_dev.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call([fused.CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + HERE, "-Wall", "-Wno-unused-function",
                               "-ffp-contract=off", srcs[0], "-o", SO, "-lpthread"])
    lib = C.CDLL(SO)
    lib.emu_count_outside.restype = C.c_uint32
    return lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def problem():
    """Rays, depths and a field for every case: 23 rays x 13 samples at most, ray 2 misses the box (near = far = FLT_MAX, as
    sf_near_far_from_aabb reports a miss), a box larger than the grid's bound so that clipped points leave the unit cube."""
    p = ngp_ref.init_params(bound=4, seed=3, table_std=0.5, sigma_bias=-1.0)
    g = torch.Generator().manual_seed(7)
    N, T = 23, 13
    o, d = ngp_ref.circle_rays(5, view=2)
    o, d = o[:N].clone().contiguous(), d[:N].clone().contiguous()
    d[2] = -d[2]
    nears, fars = 2.0 + torch.rand(N, generator=g), 9.0 + torch.rand(N, generator=g)
    nears[2] = fars[2] = FLT_MAX
    aabb = torch.tensor([-4.5] * 3 + [4.5] * 3)
    lin = torch.linspace(0.0, 1.0, T)
    u = torch.rand(N, T, generator=g)
    z_fine = (torch.rand(N, T, generator=g) * 9.0 + 1.0).contiguous()      # unsorted, as sample_pdf leaves them
    z_fine[2] = FLT_MAX
    ws = [p[f"sigma_net.net.{i}.{w}"].contiguous() for i in range(3) for w in ("weight", "bias")]
    return dict(p=p, N=N, T=T, o=o, d=d, nears=nears, fars=fars, aabb=aabb, lin=lin, u=u, z_fine=z_fine, ws=ws)


def _tables(kind, p):
    """(embeddings, offsets, gridtype): the product geometry (tiled, 2^16-row map), or a hashed grid with a map of 3000 rows (not
    a power of two)."""
    if kind == "tiled":
        return p["encoder.embeddings"], p["encoder.offsets"].to(torch.int32).contiguous(), 1
    S = float(np.log2(ngp_ref.per_level_scale(4)))
    sizes = [min(3000, (int(np.ceil(16 * 2.0 ** (l * S))) + 1) ** 3) for l in range(16)]
    offs = torch.tensor(np.concatenate([[0], np.cumsum([(n + 7) // 8 * 8 for n in sizes])]), dtype=torch.int32)
    emb = (torch.rand(int(offs[-1]), 2, generator=torch.Generator().manual_seed(11)) - 0.5).contiguous()
    return emb, offs, 0


def _run(lib, pb, kind, mode, N, grid, use_ref, with_cache, with_u=True):
    T = pb["T"]
    P = N * T
    emb, offs, gridtype = _tables(kind, pb["p"])
    S = float(np.log2(ngp_ref.per_level_scale(4)))
    nan = float("nan")
    z_out, sigma, rgb = torch.full((P,), nan), torch.full((P,), nan), torch.full((P, 3), nan)
    feat = torch.full((P, 32), nan) if with_cache else None
    u = pb["u"][:N].contiguous() if with_u else None
    z_in = pb["z_fine"][:N].contiguous()
    lib.emu_field_fwd(C.c_int(mode), _ptr(emb), _ptr(offs), C.c_uint32(offs.numel() - 1), C.c_float(S), C.c_uint32(16), C.c_uint32(gridtype),
                      *[_ptr(w) for w in pb["ws"]], C.c_float(4.0), _ptr(pb["o"]), _ptr(pb["d"]), _ptr(pb["aabb"]), _ptr(pb["nears"]),
                      _ptr(pb["fars"]), _ptr(pb["lin"]), _ptr(u), _ptr(z_in), C.c_uint32(N), C.c_uint32(T), C.c_uint32(grid),
                      C.c_int(use_ref), _ptr(z_out), _ptr(sigma), _ptr(rgb), _ptr(feat))
    return dict(z=z_out, sigma=sigma, rgb=rgb, feat=feat)


# T = 13; N = 5 / 7: P = 65 / 91, a partial last trip and ray boundaries inside a trip; N = 23: P = 299 = 10 trips, so that with one
# workgroup (4 waves) a wave runs three trips and with two workgroups two (the grid stride)
@pytest.mark.parametrize("kind,N,grid,with_cache", [("tiled", 5, 1, True), ("tiled", 7, 1, False), ("tiled", 7, 3, True),
                                                    ("tiled", 23, 1, True), ("tiled", 23, 2, False), ("hash", 23, 1, True)])
@pytest.mark.parametrize("mode", [0, 1])
def test_field_forward_mfma_equals_per_point_math(problem, kind, N, grid, with_cache, mode):
    lib = _lib()
    ref = _run(lib, problem, kind, mode, N, 1, 1, True)
    got = _run(lib, problem, kind, mode, N, grid, 0, with_cache)
    keys = (["z"] if mode == 0 else []) + ["sigma", "rgb"] + (["feat"] if with_cache else [])
    for k in keys:
        assert not bool(torch.isnan(ref[k]).any()), k                      # every element written by the reference ...
        assert torch.equal(_bits(got[k]), _bits(ref[k])), (k, int((_bits(got[k]) != _bits(ref[k])).sum()))      # ... and equal, bit for bit
    if mode == 1:
        assert bool(torch.isnan(got["z"]).all())                           # mode 1 writes no z
    assert float(ref["feat"].abs().max()) > 0 and float(ref["sigma"].min()) > 0
    if N > 2:                                                              # the ray that misses: clipped to the box, outside the grid
        T = problem["T"]
        assert float(ref["feat"][2 * T:3 * T].abs().max()) == 0.0
        z = ref["z"] if mode == 0 else problem["z_fine"][:N].contiguous()
        n_out = lib.emu_count_outside(C.c_float(4.0), _ptr(problem["o"]), _ptr(problem["d"]), _ptr(problem["aabb"]), _ptr(z.contiguous()),
                                      C.c_uint32(N), C.c_uint32(T))
        assert T <= n_out < N * T


def test_field_forward_mfma_without_jitter(problem):
    """mode 0 with u = null (perturb off): the plain linspace depths."""
    lib = _lib()
    ref = _run(lib, problem, "tiled", 0, 7, 1, 1, True, with_u=False)
    got = _run(lib, problem, "tiled", 0, 7, 2, 0, True, with_u=False)
    for k in ("z", "sigma", "rgb", "feat"):
        assert torch.equal(_bits(got[k]), _bits(ref[k])), k
