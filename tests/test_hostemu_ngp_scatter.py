"""Kernel-logic test of the atomic table-gradient scatter (sparsefusion_amd/csrc/ngp_scatter.h) on CPU fibers: k_ngp_scatter<1024, OFF>
(LDS tag cache, its collision fall-through, the register run-merge, a ragged last run) and k_ngp_scatter_fine<OFF>, OFF = 0 and 1, on the
teacher geometry (`tiled`, 2^16 rows: dense, wrapped and z-dropped levels) and on `hash` levels.  Every element of the table gradient of
every level a launch walks is compared with the float64 corner sums of emu_scatter_ref64 (tests/hostemu/shade_bwd_emu.cpp) under
scatter_bound (tests/shaded_bwd_common.py)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import ngp_bwd_cases as nb
import shaded_bwd_common as sb
from ngp_common import BOUND, log2_scale
from oracle import ngp_ref
from hostemu import fused

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
SO = os.path.join(HERE, "_build", "libngp_scatter_emu.so")
pytestmark = pytest.mark.skipif(not fused.available(), reason="host clang not found")
EPS = sb.EPS
TILED, HASH = 1, 0


def _lib():
    srcs = [os.path.join(HERE, "ngp_scatter_emu.cpp"), os.path.join(HERE, "hip_emu.h"), os.path.join(HERE, "ngp_emu_common.h")] + \
           [os.path.join(HERE, "..", "..", "sparsefusion_amd", "csrc", f)
            for f in ("ngp_scatter.h", "ngp_point_attrs.h", "ngp_device.h", "sf_dev.h", "sf_fix.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call([fused.CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + HERE, "-Wall", "-Wno-unused-function",
                               "-ffp-contract=off", srcs[0], "-o", SO, "-lpthread"])
    lib = C.CDLL(SO)
    lib.emu_ngp_scatter.restype = C.c_int
    lib.emu_level_kind.restype = None
    return lib


@pytest.fixture(scope="module")
def problems():
    """The two ray layouts, each with random sorted depths that leave the box and a random d(feat) with dead samples:
    "linear"  37 rays x 22 samples, no image layout: a partly filled 64-ray tile, one run shorter than SC_RUN = 32;
    "patches" 128 rays x 40 samples, 16 rays per row: two 8 x 8 patches, two runs per ray, the second of 8 samples."""
    p = ngp_ref.init_params(bound=BOUND, seed=3, table_std=0.5, sigma_bias=-1.0)
    offs = p["encoder.offsets"].to(torch.int32).contiguous()
    out = {}
    for name, side, N, T2, rpr, seed in (("linear", 7, 37, 22, 0, 0), ("patches", 16, 128, 40, 16, 1)):
        g = torch.Generator().manual_seed(seed)
        o, d = ngp_ref.circle_rays(side, view=2)
        o, d = o[:N].contiguous(), d[:N].contiguous()
        z = (torch.rand(N, T2, generator=g) * 9.0 + 1.0).sort(1).values.contiguous()
        dfeat = torch.randn(16, N * T2, 2, generator=g)
        dfeat[:, ::7] = 0.0                                      # dead samples
        out[name] = dict(N=N, T2=T2, rpr=rpr, o=o, d=d, z=z, dfeat=dfeat.contiguous(), offs=offs, aabb=p["aabb_train"].contiguous())
    return out


def _run(pr, gridtype, kernel, e, levels, cached=0, chunks=1, grid=3, thr=None):
    """One launch set of the harness -> (table gradient [rows, 2], stats); thr defaults to the product's sf_fix_thr(8 P)."""
    lib = _lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    N, T2, offs = pr["N"], pr["T2"], pr["offs"]
    tab = torch.zeros(int(offs[-1]), 2)
    stats = (C.c_uint64 * 6)()
    thr = nb.fix_thr(8.0 * N * T2) if thr is None else thr
    rc = lib.emu_ngp_scatter(ptr(offs), C.c_uint32(16), C.c_float(log2_scale()), C.c_uint32(16), C.c_uint32(gridtype), C.c_float(float(BOUND)),
                             ptr(pr["o"]), ptr(pr["d"]), ptr(pr["aabb"]), ptr(pr["z"]), ptr(pr["dfeat"]), C.c_uint32(N), C.c_uint32(T2),
                             C.c_int(kernel), C.c_uint32(pr["rpr"]), C.c_uint32(cached), C.c_uint32(levels), C.c_uint32(chunks), C.c_uint32(grid),
                             C.c_float(thr), C.c_uint32(e), C.c_float(EPS), ptr(tab), stats)
    assert rc == 0, rc
    st = dict(cached=stats[0], fell_through=stats[1], fixed=stats[2], fp32=stats[3], max_row=stats[4], reserved=stats[5])
    assert st["reserved"] == 0                                   # no walked cell names the row SC_EMPTY reserves
    return tab, st


def _check(name, pr, gridtype, tab, e, levels, merged, fp32_addends=False):
    """every element of every level in `levels` against the float64 corner sums; every other level untouched"""
    offs = pr["offs"]
    df = pr["dfeat"].permute(1, 0, 2).reshape(-1, 32)
    for level in range(16):
        got = tab[int(offs[level]):int(offs[level + 1])]
        if level not in levels:
            assert float(got.abs().max()) == 0, (name, level)
            continue
        want, sum_abs, count = sb.scatter_ref64({"encoder.offsets": offs}, pr["o"], pr["d"], pr["aabb"], pr["z"], df, level, e, gridtype=gridtype)
        assert float(want.abs().max()) > 0, (name, level)
        nb.check_elements(f"{name} level {level}", got, want, sb.scatter_bound(want, sum_abs, count, merged, fp32_addends))


def test_teacher_levels_are_dense_wrapped_and_z_dropped(problems):
    """what the level choice of the cases below rests on: level 0 dense, level 5 wrapped but not z-dropped, level 9 z-dropped"""
    lib = _lib()
    offs = problems["linear"]["offs"]
    kind = {}
    for level in (0, 5, 9):
        out = (C.c_uint32 * 3)()
        lib.emu_level_kind(C.c_void_p(offs.data_ptr()), C.c_uint32(16), C.c_float(log2_scale()), C.c_uint32(16), C.c_uint32(TILED), C.c_uint32(level), out)
        kind[level] = (out[1], out[2])
    assert kind == {0: (0, 0), 5: (1, 0), 9: (1, 1)}, kind
    assert int(offs[10] - offs[9]) == 1 << 16


@pytest.mark.parametrize("e", [0, 3])
@pytest.mark.parametrize("layout", ["linear", "patches"])
@pytest.mark.parametrize("cached", [10, 0], ids=["cache", "no_cache"])
def test_cached_scatter_on_the_teacher_levels(problems, layout, cached, e):
    """k_ngp_scatter<1024, OFF> over levels 0 .. 9 of the teacher geometry (dense, wrapped, z-dropped), every level through the LDS cache
    (cached_levels == last_level, the only setting ngp_scatter_plan produces today) and none"""
    pr = problems[layout]
    tab, st = _run(pr, TILED, 0, e, 10, cached=cached)
    assert (st["cached"] > 0) == (cached > 0) and st["fp32"] == 0
    _check(f"k_ngp_scatter {layout} cached={cached} e={e}", pr, TILED, tab, e, range(10), merged=True)


@pytest.mark.parametrize("e", [0, 3])
@pytest.mark.parametrize("layout,chunks", [("linear", 1), ("patches", 2)])
def test_fine_scatter_on_the_teacher_levels(problems, layout, chunks, e):
    """k_ngp_scatter_fine<OFF> over all 16 levels of the teacher geometry; the 128 rays in two chunks (p_off = 2560 in the second)"""
    pr = problems[layout]
    tab, st = _run(pr, TILED, 1, e, 0, chunks=chunks)
    assert st["fixed"] > 0 and st["fp32"] == 0
    _check(f"k_ngp_scatter_fine {layout} chunks={chunks} e={e}", pr, TILED, tab, e, range(16), merged=False)


@pytest.mark.parametrize("e", [0, 3])
def test_hashed_levels_collide_in_the_cache(problems, e):
    """`hash` levels through k_ngp_scatter's LDS cache on the 128 x 40 rays: a workgroup's 2560 samples x 8 corners name far more distinct
    rows of a hashed level than the 4096 slots hold, so the fall-through to the global table runs beside the cached sums"""
    pr = problems["patches"]
    tab, st = _run(pr, HASH, 0, e, 10, cached=10)
    assert st["cached"] > 0 and st["fell_through"] > 0, st
    _check(f"k_ngp_scatter hash e={e}", pr, HASH, tab, e, range(10), merged=True)


@pytest.mark.parametrize("e", [0, 3])
def test_fine_scatter_on_hashed_levels(problems, e):
    pr = problems["linear"]
    tab, st = _run(pr, HASH, 1, e, 12)
    _check(f"k_ngp_scatter_fine hash e={e}", pr, HASH, tab, e, range(12, 16), merged=False)


def test_addends_on_both_sides_of_the_threshold(problems):
    """thr = 2^-6, below the median |w d(feat)| (the fine kernel makes one sf_grad_add per addend: more of them take the fp32 atomic than
    the fixed-point sum), so both routes carry addends in both kernels -- within one element too.  The bound gains the chain term of the
    fp32 addends (scatter_bound)."""
    pr = problems["linear"]
    thr = 2.0 ** -6
    tab, st = _run(pr, TILED, 1, 0, 0, thr=thr)
    assert st["fp32"] > st["fixed"] > 0, st
    _check("k_ngp_scatter_fine thr=2^-6", pr, TILED, tab, 0, range(16), merged=False, fp32_addends=True)
    tab, st = _run(pr, TILED, 0, 0, 10, cached=10, thr=thr)
    assert st["fp32"] > 0 and st["cached"] > 0, st
    _check("k_ngp_scatter thr=2^-6", pr, TILED, tab, 0, range(10), merged=True, fp32_addends=True)


@pytest.mark.parametrize("gridtype", [TILED, HASH], ids=["tiled", "hash"])
def test_no_cell_names_the_reserved_tag(problems, gridtype):
    """SC_EMPTY = 0xffffffff marks a free slot of the tag cache: a table row of that index would be taken for one.  Rows are reduced
    modulo the level size (ngp_row3), so every row a cell names lies below it; the harness scans every walked cell (checked in _run).
    This states the invariant the tag rests on; it cannot fail for a table below 2^32 rows."""
    pr = problems["patches"]
    _, st = _run(pr, gridtype, 1, 0, 0)
    assert st["reserved"] == 0 and st["max_row"] < int((pr["offs"][1:] - pr["offs"][:-1]).max()) < 0xffffffff
