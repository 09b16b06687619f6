"""Kernel-logic test of the pipelined field-backward kernel (sparsefusion_amd/csrc/ngp_bwd_pipe.h) on CPU threads against the
emulation of k_ngp_field_bwd_mfma (ngp_bwd_mfma.h) on the same field cache: d(feat) and the six MLP gradients must be EQUAL (==).
The emulated sf_mfma4 is the k-ordered fmaf chain, so this pins the new kernel's own logic: the operands read a trip (perm: two)
ahead and their clamping, the register-resident weight fragments, the matrix-core forms of phases C, D and E and their lane maps,
the flush.  Every wave sum here is far below thr (2^16 / grid), so the sums are integers and do not depend on the order of the adds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import ngp_ref
import ngp_bwd_cases
from hostemu import fused

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
SO = os.path.join(HERE, "_build", "libngp_bwd_pipe_emu.so")
pytestmark = pytest.mark.skipif(not fused.available(), reason="host clang not found")
FLT_MAX = 3.402823466e+38
N, T = 37, 11                                                 # 814 points: 25 full trips and a ragged one of 14 points; rays end inside trips
NAMES = ("g_w0", "g_b0", "g_w1", "g_b1", "g_w2", "g_b2", "dfeat")


def _lib():
    srcs = [os.path.join(HERE, "ngp_bwd_pipe_emu.cpp"), os.path.join(HERE, "hip_emu.h"), os.path.join(HERE, "ngp_emu_common.h")] + \
           [os.path.join(HERE, "..", "..", "sparsefusion_amd", "csrc", f) for f in ("ngp_bwd_pipe.h", "ngp_bwd_mfma.h", "ngp_device.h", "sf_dev.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call([fused.CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + HERE, "-Wall", "-Wno-unused-function",
                               "-ffp-contract=off", srcs[0], "-o", SO, "-lpthread"])
    lib = C.CDLL(SO)
    lib.emu_field_bwd_pipe.restype = C.c_uint32
    return lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.fixture(scope="module")
def problem():
    """37 rays x 22 sorted samples; ray 2 misses the box (every depth FLT_MAX, as near = far = FLT_MAX leaves them) and the box is
    larger than the grid's bound, so clipped points leave the unit cube."""
    p = ngp_ref.init_params(bound=4, seed=3, table_std=0.5, sigma_bias=-1.0)
    g = torch.Generator().manual_seed(5)
    T2, P = 2 * T, N * 2 * T
    o, d = ngp_ref.circle_rays(7, view=2)
    o, d = o[:N].clone().contiguous(), d[:N].clone().contiguous()
    d[2] = -d[2]
    z = (torch.rand(N, T2, generator=g) * 9.0 + 1.0).sort(1).values.contiguous()
    z[2] = FLT_MAX
    dsig = torch.randn(P, generator=g)
    drgb = torch.randn(P, 3, generator=g)
    offs = p["encoder.offsets"].to(torch.int32).contiguous()
    ws = [p[f"sigma_net.net.{i}.{w}"].contiguous() for i in range(3) for w in ("weight", "bias")]
    aabb = torch.tensor([-4.5] * 3 + [4.5] * 3)
    return dict(p=p, o=o, d=d, z=z, dsig=dsig, drgb=drgb, offs=offs, ws=ws, aabb=aabb)


def _run(lib, pb, pipe, starts, grids, with_dfeat=True, dfeat_P=None):
    P = N * 2 * T
    L = pb["offs"].numel() - 1
    S = float(np.log2(ngp_ref.per_level_scale(4)))
    dfeat_P = P if dfeat_P is None else dfeat_P
    thr = ngp_bwd_cases.fix_thr(4.0 * sum(grids))
    out = [torch.zeros(64, 32), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(4, 64), torch.zeros(4)]
    dfeat = torch.full((L, dfeat_P, 2), float("nan")) if with_dfeat else None
    st, gr = torch.tensor(starts, dtype=torch.int32), torch.tensor(grids, dtype=torch.int32)
    n_out = lib.emu_field_bwd_pipe(C.c_int(pipe), _ptr(pb["p"]["encoder.embeddings"]), _ptr(pb["offs"]), C.c_uint32(L), C.c_float(S), C.c_uint32(16),
                                   C.c_uint32(1), *[_ptr(w) for w in pb["ws"]], C.c_float(4.0), _ptr(pb["o"]), _ptr(pb["d"]), _ptr(pb["aabb"]),
                                   _ptr(pb["z"]), _ptr(pb["dsig"]), _ptr(pb["drgb"]), C.c_uint32(N), C.c_uint32(2 * T), C.c_uint32(len(grids)),
                                   _ptr(st), _ptr(gr), C.c_float(thr), C.c_uint32(dfeat_P), *[_ptr(t) for t in out], _ptr(dfeat))
    assert 2 * T <= n_out < P                                  # the miss ray and more are outside the grid; most points are inside
    return out + [dfeat]


def _equal(got, ref, what):
    for name, a, b in zip(NAMES, got, ref):
        if b is None:
            assert a is None
            continue
        assert a.shape == b.shape
        # ==, with NaN = NaN for the d(feat) elements neither kernel writes (rows past the point count)
        same = (a == b) | (torch.isnan(a) & torch.isnan(b))
        assert bool(same.all()), (what, name, int((~same).sum()))


# grid 1: six or seven trips per wave; grid 2: waves with three and four trips (a prefetched ragged trip, and waves whose next trip does
# not exist); grid 7: 28 waves for 26 trips, two waves run no trip at all
@pytest.mark.parametrize("grid", [1, 2, 7])
def test_pipe_equals_mfma_one_chunk(problem, grid):
    lib = _lib()
    ref = _run(lib, problem, 0, [0, N], [grid])
    got = _run(lib, problem, 1, [0, N], [grid])
    _equal(got, ref, f"grid {grid}")
    P = N * 2 * T
    assert not bool(torch.isnan(ref[6]).any()) and float(ref[6].abs().max()) > 0 and float(ref[2].abs().max()) > 0
    assert float(ref[6][:, 2 * 2 * T:3 * 2 * T].abs().max()) == 0.0                   # the miss ray: outside, no feature gradient
    assert ref[6].shape[1] == P


def test_pipe_equals_mfma_without_dfeat(problem):
    """dfeat_out null (table frozen): the MLP gradients alone."""
    lib = _lib()
    ref = _run(lib, problem, 0, [0, N], [2], with_dfeat=False)
    got = _run(lib, problem, 1, [0, N], [2], with_dfeat=False)
    _equal(got, ref, "no dfeat")
    assert float(ref[0].abs().max()) > 0


def test_pipe_equals_mfma_chunk_at_offset_unaligned(problem):
    """Two chunks (the second at p_off = 110 points) into a d(feat) image with an ODD level stride: every trip takes the unaligned
    store path; the chunks' trips do not line up with the whole set's."""
    lib = _lib()
    P = N * 2 * T
    ref = _run(lib, problem, 0, [0, 5, N], [1, 2], dfeat_P=P + 1)
    got = _run(lib, problem, 1, [0, 5, N], [1, 2], dfeat_P=P + 1)
    _equal(got, ref, "two chunks, odd stride")
    assert not bool(torch.isnan(ref[6][:, :P]).any()) and bool(torch.isnan(ref[6][:, P:]).all())
    one = _run(lib, problem, 1, [0, N], [2])
    assert torch.equal(one[6], got[6][:, :P])                  # d(feat) does not depend on the chunking
