"""k_ngp_field_bwd_pipe (csrc/ngp_bwd_pipe.h) against k_ngp_field_bwd_mfma on the GPU: the seven gradients of sf_ngp_render_backward with the
library's sf_ngp_field_bwd_pipe switch on must be torch.equal to those with it off, on the ray sets of tests/test_gpu_ngp_bwd.py (whose
forwards are shared), and the switch must select the kernel only where a field cache is passed.

Precondition, on the reference path alone: two runs with the switch off are themselves torch.equal.  That holds where every addend of every
gradient sum stays below its fixed-point threshold (sf_grad_add: integer sums do not depend on the order of the adds; an fp32 atomic's does).
The table gradient's threshold is the tight one -- 2^18 / (8 * 2 N T), 1 / 4 and 1 / 8 for the larger cases -- so the upstream gradients are
scaled by 2^-6 (a power of two scales every fp32 value of the backward exactly)."""
import ctypes as C

import pytest
import torch

import test_gpu_ngp_bwd as tb

pytestmark = pytest.mark.gpu
DEV = tb.DEV
NAMES = ("embeddings", "w0", "b0", "w1", "b1", "w2", "b2")
SCALE = 2.0 ** -6


@pytest.fixture
def switch():
    """The library's switch, put back to the renderer's setting afterwards."""
    from sparsefusion_amd import _lib
    from sparsefusion_amd.nerf import renderer as R
    lib = _lib.lib()
    yield lib
    lib.sf_ngp_field_bwd_pipe(1 if R._FIELD_BWD_PIPE else 0)


def _launches(lib):
    counts = (C.c_uint64 * 2)()
    lib.sf_ngp_field_bwd_launches(C.cast(counts, C.c_void_p))
    return int(counts[0]), int(counts[1])


def _grads(lib, fwd, gi, gw, pipe, use_cache=True):
    """The seven gradients (table first) and d(feat) of one sf_ngp_render_backward, on the GPU."""
    from sparsefusion_amd import _lib
    N, T = fwd["N"], fwd["T"]
    M = N * 2 * T
    grads = [torch.zeros_like(t) for t in fwd["params"]]
    gs = _lib.SfNgpFieldGrad()
    (gs.g_embeddings, gs.g_w0, gs.g_b0, gs.g_w1, gs.g_b1, gs.g_w2, gs.g_b2) = (t.data_ptr() for t in grads)
    f = fwd["handle"].struct(fwd["params"])
    wb = lib.sf_ngp_render_workspace_bytes(N, T)
    work = torch.empty(wb // 4, device=DEV)
    lib.sf_ngp_field_bwd_pipe(1 if pipe else 0)
    _lib.check(lib.sf_ngp_render_backward(C.byref(f), C.byref(gs), _lib.ptr(fwd["o"]), _lib.ptr(fwd["d"]), _lib.ptr(fwd["aabb"]), N, T,
                                          _lib.ptr(fwd["nears"]), _lib.ptr(fwd["fars"]), _lib.ptr(fwd["z_s"]), _lib.ptr(fwd["sig_s"]),
                                          _lib.ptr(fwd["rgb_s"]), 0.0, _lib.ptr(gi), _lib.ptr(gw), 0, _lib.ptr(fwd["cache"]) if use_cache else None,
                                          _lib.ptr(work), wb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return grads, work[4 * M:36 * M].clone()


# (n_side, rays, T, view, seed of the forward, seed of the upstream gradients, launches of the field backward): the cases of test_gpu_ngp_bwd.py
CASES = {"ragged": (7, 37, 11, 2, 11, 1, 1),                   # one chunk, 26 trips on 7 workgroups: at most one trip per wave, a ragged one, idle waves
         "two_chunks": (64, 4096, 16, 3, 12, 2, 2),            # two chunks of 2048 trips on 256 workgroups: two trips per wave
         "unequal_chunks": (100, 10000, 8, 4, 13, 3, 2)}       # 8192 + 1808 rays: four trips per wave, then 226 workgroups


@pytest.mark.parametrize("case", list(CASES))
def test_pipe_gradients_equal_mfma_gradients(golden_dir, switch, case):
    lib = switch
    n_side, N, T, view, seed, useed, n_launch = CASES[case]
    fwd = tb._circle_forward(golden_dir, n_side, N, T, view, seed)
    gi, gw = tb._upstream(N, useed)
    gi, gw = (gi * SCALE).to(DEV).contiguous(), (gw * SCALE).to(DEV).contiguous()
    c0 = _launches(lib)
    off1, df_off1 = _grads(lib, fwd, gi, gw, pipe=False)
    off2, df_off2 = _grads(lib, fwd, gi, gw, pipe=False)
    c1 = _launches(lib)
    assert c1 == (c0[0] + 2 * n_launch, c0[1])                 # the reference kernel ran, n_launch chunks per backward
    for name, a, b in zip(NAMES, off1, off2):                  # the precondition: the reference path repeats itself
        assert torch.equal(a, b), ("precondition", case, name, int((a != b).sum()))
    assert torch.equal(df_off1, df_off2)
    assert all(bool(torch.isfinite(t).all()) for t in off1) and all(float(t.abs().max()) > 0 for t in off1)
    on, df_on = _grads(lib, fwd, gi, gw, pipe=True)
    assert _launches(lib) == (c1[0], c1[1] + n_launch)         # the pipelined kernel ran
    for name, a, b in zip(NAMES, on, off1):
        assert torch.equal(a, b), (case, name, int((a != b).sum()), float((a - b).abs().max()))
    assert torch.equal(df_on, df_off1), (case, "dfeat", int((df_on != df_off1).sum()))


def test_switch_and_dispatch(golden_dir, switch):
    """The switch starts at the renderer's setting; with a field cache it selects the kernel, without one k_ngp_field_bwd_mfma runs."""
    from sparsefusion_amd.nerf import renderer as R
    lib = switch
    want = 1 if R._FIELD_BWD_PIPE else 0
    assert lib.sf_ngp_field_bwd_pipe(-1) == want and lib.sf_ngp_field_bwd_pipe(-1) == want      # asking changes nothing
    assert lib.sf_ngp_field_bwd_pipe(0) == want and lib.sf_ngp_field_bwd_pipe(1) == 0 and lib.sf_ngp_field_bwd_pipe(-1) == 1
    fwd = tb._circle_forward(golden_dir, 7, 37, 11, 2, 11)
    gi, gw = tb._upstream(37, 1)
    gi, gw = (gi * SCALE).to(DEV).contiguous(), (gw * SCALE).to(DEV).contiguous()
    c0 = _launches(lib)
    _grads(lib, fwd, gi, gw, pipe=True)
    c1 = _launches(lib)
    assert c1 == (c0[0], c0[1] + 1)                            # cache + switch on: the pipelined kernel
    _grads(lib, fwd, gi, gw, pipe=True, use_cache=False)
    c2 = _launches(lib)
    assert c2 == (c1[0] + 1, c1[1])                            # no cache: k_ngp_field_bwd_mfma whatever the switch says
    _grads(lib, fwd, gi, gw, pipe=False)
    assert _launches(lib) == (c2[0] + 1, c2[1])                # cache + switch off
