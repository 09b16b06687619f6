"""Kernel-logic tests of the texture bake (k_ngp_texture_bake, sparsefusion_amd/csrc/mesh.hip): the kernel's own per-texel function and
layout check (sparsefusion_amd/csrc/ngp_texture.h) compiled for the CPU and run thread by thread over the kernel's grid-stride
schedule (tests/hostemu/texture_emu.cpp), against the numpy restatement of layout + clamp + weighted sum (bit for bit), the oracle's
albedo (the centre tolerances of tests/point_attrs_common.py) and the truncation rule.  No GPU."""
import numpy as np
import pytest
import torch

import point_attrs_common as pc
import texture_common as tc
from ngp_common import BOUND, params_from_cfg
from oracle import ngp_ref


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(f"{golden_dir}/ngp_render.pt")


@pytest.fixture(scope="module")
def cases(golden):
    """(field, F, W) -> (params, verts, faces, emulated outputs) -- computed once, shared, never modified"""
    out = {}
    for name in ("teacher", "default_init"):
        p = params_from_cfg(golden[name]["cfg"])
        for F, W in tc.SMALL_CASES:
            v, f = tc.random_mesh(F)
            rc, got = tc.emu_texture_bake(p, v, f, W)
            assert rc == 0
            out[name, F, W] = (p, v, f, got)
    return out


@pytest.mark.parametrize("F,W", tc.SMALL_CASES)
@pytest.mark.parametrize("name", ["teacher", "default_init"])
def test_emulated_bake(cases, name, F, W):
    """face_id and xyz equal the restatement bit for bit; albedo within the oracle's centre tolerances on the used texels; rgb8 is the
    truncation of the albedo; unused texels hold 0 / 0 / 0 / -1; every element is written.  W * W runs over three emulated
    workgroups: F = 50 at W = 64 makes six rounds and ends on a full one, F = 7 at W = 12 is one partial round."""
    p, v, f, got = cases[name, F, W]
    face_id, xyz = tc.np_bake_points(v, f, W)
    G, c = tc.layout(F, W)
    assert np.array_equal(got["face_id"], face_id)
    assert np.array_equal(tc.bits(got["xyz"]), tc.bits(xyz))
    used = face_id >= 0
    assert set(np.unique(face_id[used])) == set(range(F)) and not used[G * c:].any() and not used[:, G * c:].any()
    assert not np.isnan(got["albedo"]).any()
    with torch.no_grad():
        _, ref = ngp_ref.common_forward(p, torch.from_numpy(xyz[used]), BOUND)
    assert torch.allclose(torch.from_numpy(got["albedo"][used]), ref, rtol=pc.SIGMA_RTOL, atol=pc.ALBEDO_ATOL)
    assert np.array_equal(got["rgb8"], tc.np_quantise(got["albedo"]))
    assert (got["albedo"][~used] == 0).all() and (got["rgb8"][~used] == 0).all() and (got["xyz"][~used] == 0).all()
    if F == 50 and name == "teacher":
        assert len(np.unique(got["rgb8"][used])) > 10                # a texture, not a constant
    # the texel at a chart corner is the vertex, bit for bit
    xy = tc.corner_texels(F, W)
    for k in range(3):
        at = got["xyz"][xy[:, k, 1], xy[:, k, 0]]
        assert np.array_equal(tc.bits(at), tc.bits(v[f[:, k]])), k
        assert np.array_equal(got["face_id"][xy[:, k, 1], xy[:, k, 0]], np.arange(F))


def test_points_lie_on_their_faces(cases):
    """every used texel's point is a convex combination of its face's vertices (the gutter clamp keeps it on the triangle): the
    barycentrics recovered in float64 are within 1e-5 of [0, 1] and sum to one"""
    p, v, f, got = cases["teacher", 50, 64]
    used = got["face_id"] >= 0
    tri = v[f[got["face_id"][used]]].astype(np.float64)              # [n, 3, 3]
    x = got["xyz"][used].astype(np.float64)
    m = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]], -1)  # [n, 3, 2]
    uv = np.stack([np.linalg.lstsq(m[i], x[i] - tri[i, 0], rcond=None)[0] for i in range(x.shape[0])])
    res = np.abs(np.einsum("nij,nj->ni", m, uv) + tri[:, 0] - x).max()
    assert res < 1e-5 and uv.min() > -1e-5 and (uv.sum(-1)).max() < 1 + 1e-5


@pytest.mark.parametrize("blocks", [1, 2, 5])
def test_emulated_schedule_and_null_outputs(cases, blocks):
    """another number of workgroups and every nullable output skipped in turn leave the others unchanged"""
    p, v, f, full = cases["teacher", 7, 12]
    names = ("rgb8", "albedo", "xyz", "face_id")
    for skip in names:
        want = tuple(n for n in names if n != skip)
        rc, got = tc.emu_texture_bake(p, v, f, 12, blocks=blocks, want=want)
        assert rc == 0 and got[skip] is None
        for n in want:
            assert np.array_equal(got[n].view(np.uint8), full[n].view(np.uint8)), (skip, n)


def test_out_of_range_face_is_left_unused(golden):
    """a face with a vertex index outside [0, V) -- V itself, a negative one -- gets no vertex read and no evaluation: its texels are
    written as unused and the other faces do not change.  Emulation only: this case never runs on a GPU."""
    p = params_from_cfg(golden["teacher"]["cfg"])
    v, f = tc.random_mesh(7)
    _, good = tc.emu_texture_bake(p, v, f, 12)
    bad = f.copy()
    bad[2, 1] = v.shape[0]
    bad[5, 0] = -1
    bad[6, 2] = 2 ** 31 - 1
    rc, got = tc.emu_texture_bake(p, v, bad, 12)
    assert rc == 0
    face_id, xyz = tc.np_bake_points(v, bad, 12)
    assert np.array_equal(got["face_id"], face_id) and np.array_equal(tc.bits(got["xyz"]), tc.bits(xyz))
    dropped = np.isin(good["face_id"], (2, 5, 6))
    assert dropped.any() and (got["face_id"][dropped] == -1).all()
    for n in ("rgb8", "albedo", "xyz"):
        assert (got[n][dropped] == 0).all() and np.array_equal(got[n][~dropped].view(np.uint8), good[n][~dropped].view(np.uint8))
    assert np.array_equal(got["face_id"][~dropped], good["face_id"][~dropped])


def test_small_cell_is_refused_before_anything_runs(golden):
    """c < 6: the argument check answers 3 and no output element is touched; F == 0 writes every texel as unused"""
    p = params_from_cfg(golden["teacher"]["cfg"])
    v, f = tc.random_mesh(7)
    rc, got = tc.emu_texture_bake(p, v, f, 11)
    assert rc == 3
    assert (got["rgb8"] == 255).all() and np.isnan(got["albedo"]).all() and np.isnan(got["xyz"]).all()
    assert (got["face_id"] == -2 ** 31).all()
    rc, got = tc.emu_texture_bake(p, v, f[:0], 9)
    assert rc == 0 and (got["face_id"] == -1).all()
    assert (got["rgb8"] == 0).all() and (got["albedo"] == 0).all() and (got["xyz"] == 0).all()
