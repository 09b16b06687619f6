"""Kernel-logic test of the MFMA field-backward kernel (sparsefusion_amd/csrc/ngp_bwd_mfma.h) on CPU threads against the
per-point reference math of ngp_device.h (the functions the oracle-pinned host emulation of the render uses): MLP weight /
bias gradients and the per-level feature gradients for random rays, and a ragged last trip."""
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
SO = os.path.join(HERE, "_build", "libngp_bwd_emu.so")
pytestmark = pytest.mark.skipif(not fused.available(), reason="host clang not found")


def _lib():
    srcs = [os.path.join(HERE, "ngp_bwd_emu.cpp"), os.path.join(HERE, "hip_emu.h"), os.path.join(HERE, "ngp_emu_common.h")] + \
           [os.path.join(HERE, "..", "..", "sparsefusion_amd", "csrc", f)
            for f in ("ngp_bwd_mfma.h", "ngp_scatter_bin.h", "ngp_bwd_plan.h", "ngp_point_attrs.h", "ngp_device.h", "sf_dev.h", "sf_fix.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call([fused.CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + HERE, "-Wall", "-Wno-unused-function",
                               "-ffp-contract=off", srcs[0], "-o", SO, "-lpthread"])
    return C.CDLL(SO)


def test_field_backward_mfma_matches_per_point_math():
    lib = _lib()
    p = ngp_ref.init_params(bound=4, seed=3, table_std=0.5, sigma_bias=-1.0)
    g = torch.Generator().manual_seed(0)
    N, T2 = 9, 22                                             # P = 198: six full trips of 32 points + a ragged one
    P = N * T2
    o, d = ngp_ref.circle_rays(3, view=2)
    o, d = o[:N].contiguous(), d[:N].contiguous()
    z = (torch.rand(N, T2, generator=g) * 9.0 + 1.0).sort(1).values.contiguous()      # some samples leave the box
    dsig = torch.randn(P, generator=g)
    drgb = torch.randn(P, 3, generator=g)
    offs = p["encoder.offsets"].to(torch.int32).contiguous()
    L = offs.numel() - 1
    S = float(np.log2(ngp_ref.per_level_scale(4)))
    ws = [p[f"sigma_net.net.{i}.{w}"].contiguous() for i in range(3) for w in ("weight", "bias")]
    aabb = p["aabb_train"].contiguous()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def run(use_ref, grid):
        out = [torch.zeros(64, 32), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(4, 64), torch.zeros(4),
               torch.zeros(L, P, 2)]
        lib.emu_field_bwd(ptr(p["encoder.embeddings"]), ptr(offs), C.c_uint32(L), C.c_float(S), C.c_uint32(16), C.c_uint32(1),
                          *[ptr(w) for w in ws], C.c_float(4.0), ptr(o), ptr(d), ptr(aabb), ptr(z), ptr(dsig), ptr(drgb),
                          C.c_uint32(P), C.c_uint32(T2), C.c_uint32(grid), C.c_int(use_ref), *[ptr(t) for t in out])
        return out

    ref = run(1, 1)
    for grid in (1, 3):                                       # one workgroup (4 waves share the trips) and several
        got = run(0, grid)
        for name, a, b in zip(("g_w0", "g_b0", "g_w1", "g_b1", "g_w2", "g_b2", "dfeat"), got, ref):
            err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-20)
            assert err < 2e-5, (grid, name, err)
    assert float(ref[6].abs().max()) > 0 and float(ref[2].abs().max()) > 0
    # r03: the same kernel reading the forward's field cache (features of every sample through the sort permutation) instead of
    # re-gathering them
    got = run(2, 3)
    for name, a, b in zip(("g_w0", "g_b0", "g_w1", "g_b1", "g_w2", "g_b2", "dfeat"), got, ref):
        err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-20)
        assert err < 2e-5, ("cache", name, err)


@pytest.fixture(scope="module")
def field_problem():
    """One small field-backward problem for the per-element checks of tests/ngp_bwd_cases.py: 13 rays x 22 sorted samples (P = 286: eight full
    trips and a ragged one), the features ngp_encode gives them (emu_features), random upstream gradients."""
    lib = _lib()
    p = ngp_ref.init_params(bound=4, seed=3, table_std=0.5, sigma_bias=-1.0)
    g = torch.Generator().manual_seed(0)
    N, T2 = 13, 22
    P = N * T2
    o, d = ngp_ref.circle_rays(4, view=2)
    o, d = o[:N].contiguous(), d[:N].contiguous()
    z = (torch.rand(N, T2, generator=g) * 9.0 + 1.0).sort(1).values.contiguous()
    dsig = torch.randn(P, generator=g)
    drgb = torch.randn(P, 3, generator=g)
    offs = p["encoder.offsets"].to(torch.int32).contiguous()
    L = offs.numel() - 1
    S = float(np.log2(ngp_ref.per_level_scale(4)))
    ws = [p[f"sigma_net.net.{i}.{w}"].contiguous() for i in range(3) for w in ("weight", "bias")]
    aabb = p["aabb_train"].contiguous()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    feat, xyz, inside = torch.zeros(P, 32), torch.zeros(P, 3), torch.zeros(P)
    lib.emu_features(ptr(p["encoder.embeddings"]), ptr(offs), C.c_uint32(L), C.c_float(S), C.c_uint32(16), C.c_uint32(1), C.c_float(4.0), ptr(o),
                     ptr(d), ptr(aabb), ptr(z), C.c_uint32(P), C.c_uint32(T2), ptr(feat), ptr(xyz), ptr(inside))
    x, ins = ngp_bwd_cases.sample_points(o, d, z, aabb, 4.0)
    assert torch.equal(x.reshape(P, 3), xyz) and torch.equal(ins.reshape(P), inside.bool())      # sample_points restates ngp_point / ngp_unit

    def run(starts, grids, thr, cache, dsig=dsig, drgb=drgb):
        out = [torch.zeros(64, 32), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(4, 64), torch.zeros(4), torch.zeros(L, P, 2)]
        st, gr = torch.tensor(starts, dtype=torch.int32), torch.tensor(grids, dtype=torch.int32)
        lib.emu_field_bwd_chunks(ptr(p["encoder.embeddings"]), ptr(offs), C.c_uint32(L), C.c_float(S), C.c_uint32(16), C.c_uint32(1),
                                 *[ptr(w) for w in ws], C.c_float(4.0), ptr(o), ptr(d), ptr(aabb), ptr(z), ptr(dsig), ptr(drgb), C.c_uint32(N),
                                 C.c_uint32(T2), C.c_uint32(len(grids)), ptr(st), ptr(gr), C.c_float(thr), ptr(feat if cache else None),
                                 *[ptr(t) for t in out])
        return out

    return dict(N=N, T=T2 // 2, P=P, W=ws, feat=feat, xyz=xyz, inside=inside.bool(), dsig=dsig, drgb=drgb, run=run)


def _check_field(name, fp, got, geo, dsig=None, drgb=None):
    """d(feat) and the six MLP gradients of an emulated run against the float64 reference, per element (tests/ngp_bwd_cases.py (B))."""
    dsig, drgb = fp["dsig"] if dsig is None else dsig, fp["drgb"] if drgb is None else drgb
    fw = ngp_bwd_cases.field_forward64(fp["feat"], fp["W"], fp["xyz"], dsig, drgb)
    k, n_amb, n_left, P = ngp_bwd_cases.ambiguity(fw)
    assert n_amb <= ngp_bwd_cases.AMBIGUOUS_CAP * P and n_left <= ngp_bwd_cases.LEFT_OUT_CAP * P, (n_amb, n_left, P)     # the reference alone
    bk = ngp_bwd_cases.field_backward_check(name, fw, fp["W"], fp["inside"], got[6].permute(1, 0, 2).reshape(fp["P"], 32))
    ref = ngp_bwd_cases.weight_grads_ref64(fw, bk, geo)
    for key, t in zip(("w0", "b0", "w1", "b1", "w2", "b2"), got):
        ngp_bwd_cases.check_elements(f"{name} d{key}", t, ref[key]["want"], ref[key]["bound"])
    return ref


@pytest.mark.parametrize("cache,starts,grids", [(False, [0, 13], [1]), (False, [0, 13], [3]), (True, [0, 13], [3]), (True, [0, 5, 13], [2, 1]),
                                                (False, [0, 5, 13], [1, 2])])
def test_field_backward_per_element_float64(field_problem, cache, starts, grids):
    """k_ngp_field_bwd_mfma under the emulation against the float64 per-point reference and the derived per-element bounds: the re-gather
    and the cache path, one workgroup (a wave runs three trips) and several, and two chunks launched as sf_ngp_render_backward launches them
    (p_off = 110 points into the whole set's d(feat) image)."""
    fp = field_problem
    thr = ngp_bwd_cases.fix_thr(4.0 * sum(grids))
    geo = ngp_bwd_cases.bwd_geometry(fp["N"], fp["T"], starts=starts, grids=grids, thr=thr)
    ref = _check_field(f"emu cache={int(cache)} starts={starts} grids={grids}", fp, fp["run"](starts, grids, thr, cache), geo)
    assert all(int(r["maybe_fp32"].sum()) == 0 for r in ref.values())                # every wave sum in fixed point here


def test_field_backward_large_addends_take_the_fp32_path(field_problem):
    """Upstream gradients scaled by 64 and thr = 8, so that some waves' sums reach thr and take sf_grad_add's fp32 atomic while others stay in
    fixed point -- within one gradient element too (asserted on the reference's own wave sums)."""
    fp = field_problem
    starts, grids, thr = [0, 5, 13], [2, 1], 8.0
    geo = ngp_bwd_cases.bwd_geometry(fp["N"], fp["T"], starts=starts, grids=grids, thr=thr)
    dsig, drgb = fp["dsig"] * 64.0, fp["drgb"] * 64.0
    ref = _check_field("emu large addends", fp, fp["run"](starts, grids, thr, True, dsig, drgb), geo, dsig, drgb)
    n_waves = geo["n_waves"]
    for key in ("w0", "w1", "w2"):
        sure = ref[key]["sure_fp32"]
        assert int((sure > 0).sum()) > 0 and int(((sure > 0) & (sure < n_waves)).sum()) > 0, key       # fp32 adds, and elements with both kinds


@pytest.mark.parametrize("case", ["roomy", "overflow", "tiled"])
def test_binned_scatter_matches_per_corner_adds(case):
    """k_ngp_bin + k_ngp_bin_reduce (csrc/ngp_scatter_bin.h, r04: the hashed levels' table gradient without per-corner device
    atomics) against ngp_scatter of ngp_device.h on the same feature gradients: roomy buckets, buckets so small that most
    contributions take the overflow path (direct adds), and a `tiled` grid (z-dropped levels, skewed buckets); two chunks share the
    entries buffer, several tiles per workgroup, a ragged last tile."""
    lib = _lib()
    g = torch.Generator().manual_seed(1)
    N, T2 = 150, 22                                           # P = 3300: tiles of 1024 samples, the last one ragged
    P = N * T2
    o, d = ngp_ref.circle_rays(13, view=1)
    o, d = o[:N].contiguous(), d[:N].contiguous()
    z = (torch.rand(N, T2, generator=g) * 9.0 + 1.0).sort(1).values.contiguous()
    L, S = 16, float(np.log2(ngp_ref.per_level_scale(4)))
    sizes = [min(1 << 12, (int(np.ceil(16 * 2.0 ** (l * S))) + 1) ** 3) for l in range(L)]      # a 2^12-row hash map: 4 buckets per level
    offs = torch.tensor(np.concatenate([[0], np.cumsum([(n + 7) // 8 * 8 for n in sizes])]), dtype=torch.int32)
    dfeat = torch.randn(L, P, 2, generator=g)
    dfeat[:, ::7] = 0.0                                       # dead samples
    aabb = torch.tensor([-4.0] * 3 + [4.0] * 3)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    first, cap, gridtype = {"roomy": (6, 16384, 0), "overflow": (10, 8, 0), "tiled": (9, 1024, 1)}[case]

    def run(use_ref, chunks=1, grid=1):
        tab = torch.zeros(int(offs[-1]), 2)
        rc = lib.emu_bin_scatter(ptr(offs), C.c_uint32(L), C.c_float(S), C.c_uint32(16), C.c_uint32(gridtype), C.c_float(4.0), ptr(o), ptr(d),
                                 ptr(aabb), ptr(z), ptr(dfeat), C.c_uint32(N), C.c_uint32(T2), C.c_uint32(first), C.c_uint32(cap),
                                 C.c_uint32(chunks), C.c_uint32(grid), C.c_int(use_ref), ptr(tab))
        assert rc == 0, rc
        return tab

    ref = run(1)
    lo = int(offs[first])
    assert float(ref[lo:].abs().max()) > 0 and float(ref[:lo].abs().max()) == 0
    for chunks, grid in ((1, 1), (2, 3)) if case == "roomy" else ((2, 2),):
        got = run(0, chunks, grid)
        err = float((got - ref).abs().max()) / float(ref.abs().max())
        assert err < 1e-5, (case, chunks, grid, err)


def test_binned_scatter_keeps_large_and_non_finite_contributions():
    """The table gradient sums addends below a threshold in 64-bit fixed point (sf_dev.h sf_grad_add) and adds every other one -- large,
    Inf, NaN -- to the fp32 table as before: contributions far above the threshold still match the per-corner fp32 adds, and a NaN
    feature gradient still reaches the table (it is neither dropped nor turned into a finite number)."""
    lib = _lib()
    g = torch.Generator().manual_seed(2)
    N, T2 = 150, 22
    P = N * T2
    o, d = ngp_ref.circle_rays(13, view=1)
    o, d = o[:N].contiguous(), d[:N].contiguous()
    z = (torch.rand(N, T2, generator=g) * 9.0 + 1.0).sort(1).values.contiguous()
    L, S = 16, float(np.log2(ngp_ref.per_level_scale(4)))
    sizes = [min(1 << 12, (int(np.ceil(16 * 2.0 ** (l * S))) + 1) ** 3) for l in range(L)]
    offs = torch.tensor(np.concatenate([[0], np.cumsum([(n + 7) // 8 * 8 for n in sizes])]), dtype=torch.int32)
    aabb = torch.tensor([-4.0] * 3 + [4.0] * 3)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    first = 6

    def run(dfeat, use_ref):
        tab = torch.zeros(int(offs[-1]), 2)
        rc = lib.emu_bin_scatter(ptr(offs), C.c_uint32(L), C.c_float(S), C.c_uint32(16), C.c_uint32(0), C.c_float(4.0), ptr(o), ptr(d),
                                 ptr(aabb), ptr(z), ptr(dfeat), C.c_uint32(N), C.c_uint32(T2), C.c_uint32(first), C.c_uint32(16384),
                                 C.c_uint32(2), C.c_uint32(3), C.c_int(use_ref), ptr(tab))
        assert rc == 0, rc
        return tab

    dfeat = torch.randn(L, P, 2, generator=g)
    big = torch.rand(L, P, 1, generator=g) < 0.2
    dfeat = torch.where(big, dfeat * 1e6, dfeat).contiguous()        # threshold here: 8 (sf_fix_thr(8 P)); these are ~1e6
    ref, got = run(dfeat, 1), run(dfeat, 0)
    assert float((got - ref).abs().max()) / float(ref.abs().max()) < 1e-5
    dfeat[first + 2, 5 * T2 + 3, 0] = float("nan")
    ref, got = run(dfeat, 1), run(dfeat, 0)
    nan_g, nan_r = torch.isnan(got), torch.isnan(ref)
    assert bool(nan_g.any()) and not bool((nan_g & ~nan_r).any())      # NaN where the reference has it (a zero-weight corner may be skipped)
    ok = ~nan_r
    assert float((got[ok] - ref[ok]).abs().max()) / float(ref[ok].abs().max()) < 1e-5


def _c_plan(lib, N):
    n, max_rays, start = C.c_uint32(0), C.c_uint32(0), (C.c_uint32 * 66)()
    lib.emu_bwd_plan(C.c_uint32(N), C.byref(n), C.byref(max_rays), start)
    return n.value, max_rays.value, list(start[:n.value + 1])


def test_host_plan_matches_the_restatement():
    """ngp_bwd_plan, the field backward's grid rule and the thr_mlp rule of csrc/ngp_bwd_plan.h -- the functions sf_ngp_render_backward calls,
    exported by the harness -- against tests/ngp_bwd_cases.py's restatement (bwd_plan; chunk, grid and thr of bwd_geometry), with ==: the ray
    counts of CASES, the counts around every branch of the plan, every multiple of 256 up to 70000."""
    lib = _lib()
    lib.emu_field_bwd_grid.restype = C.c_uint32
    lib.emu_bwd_thr_mlp.restype = C.c_float
    Ns = {c["N"]: c["T"] for c in ngp_bwd_cases.CASES.values()}
    for N in [1, 37, 2048, 4096, 10000, 16384, 32768, 40000, 51712, 65535, 65536] + list(range(256, 70001, 256)):
        Ns.setdefault(N, 4)
    for N, T in Ns.items():
        n, max_rays, start = _c_plan(lib, N)
        assert start == ngp_bwd_cases.bwd_plan(N), N
        assert 1 <= n <= 64 and start[0] == 0 and start[-1] == N and all(a < b for a, b in zip(start, start[1:])), (N, start)
        assert all(b - a <= max_rays for a, b in zip(start, start[1:])), (N, max_rays, start)
        geo = ngp_bwd_cases.bwd_geometry(N, T)
        assert [p0 for p0, *_ in geo["chunks"]] == [s * 2 * T for s in start[:-1]] and [P for _, P, *_ in geo["chunks"]] == \
            [(b - a) * 2 * T for a, b in zip(start, start[1:])], N
        assert [g for *_, g in geo["chunks"]] == [lib.emu_field_bwd_grid(C.c_uint32(P)) for _, P, *_ in geo["chunks"]], N
        assert geo["thr"] == lib.emu_bwd_thr_mlp(C.c_uint32(n)), N


def _c_scatter_plan(lib, offs, L, S, table_grad, N, T):
    out = (C.c_uint32 * (6 + 17))()
    offs = offs.to(torch.int32).contiguous()
    lib.emu_scatter_plan(C.c_void_p(offs.data_ptr()), C.c_uint32(L), C.c_float(S), C.c_uint32(16), C.c_uint32(1), C.c_int(table_grad),
                         C.c_uint32(N), C.c_uint32(T), out)
    return dict(cached=out[0], first_bin=out[1], binned=bool(out[2]), last=out[3], total_buckets=out[4], bin_cap=out[5], bucket0=list(out[6:]))


def test_scatter_plan_on_the_reference_levels_and_on_an_oversized_level():
    """ngp_scatter_plan (csrc/ngp_bwd_plan.h) on the reference field's 16 levels at H = 16: with a table gradient the hashed levels are binned
    (the numbers follow from the scales, the cut-offs 60 and 640 and 1024-row buckets), without one every level is k_ngp_scatter's; a level set
    with one level of more than SB_MAX_BUCKETS = 512 buckets keeps the atomics (binned == false)."""
    lib = _lib()
    p = ngp_ref.init_params(bound=4, seed=3, table_std=0.5, sigma_bias=-1.0)
    offs = p["encoder.offsets"].to(torch.int64)
    L, S, N, T = offs.numel() - 1, float(np.log2(ngp_ref.per_level_scale(4))), 16384, 64
    assert L == 16
    scale = [float(np.float32(np.exp2(np.float32(l) * np.float32(S)) * np.float32(16) - np.float32(1))) for l in range(L)]
    n60, n640 = sum(s <= 60.0 for s in scale), sum(s <= 640.0 for s in scale)
    assert 0 < n60 < n640 <= L
    hsize = [int(offs[l + 1] - offs[l]) for l in range(L)]
    sp = _c_scatter_plan(lib, offs, L, S, 1, N, T)
    assert sp["binned"] and sp["cached"] <= sp["first_bin"] and sp["last"] == sp["first_bin"]
    assert sp["first_bin"] == n60 and sp["cached"] == n60
    nb = [(hsize[l] + 1023) // 1024 if l >= n60 else 0 for l in range(L)]
    assert sp["bucket0"] == [sum(nb[:l]) for l in range(L + 1)] and sp["total_buckets"] == sum(nb)
    max_rays = max(b - a for a, b in zip(ngp_bwd_cases.bwd_plan(N), ngp_bwd_cases.bwd_plan(N)[1:]))
    assert sp["bin_cap"] == (max_rays * 2 * T * 4 * 24 + 16 * 512 * 64) // sum(nb)
    sp0 = _c_scatter_plan(lib, offs, L, S, 0, N, T)
    assert sp0["last"] == L and not sp0["binned"] and sp0["first_bin"] == L and sp0["cached"] == n640 and sp0["bin_cap"] == 0
    big = offs.clone()
    big[L:] += (1 << 19) + 1024 - hsize[L - 1]               # the last level: 513 buckets
    spb = _c_scatter_plan(lib, big, L, S, 1, N, T)
    assert not spb["binned"] and spb["first_bin"] == L and spb["cached"] == n640 and spb["last"] == n640 and spb["bin_cap"] == 0
