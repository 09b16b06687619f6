"""Kernel-logic tests of the shaded occupancy-grid evaluation render on CPU fibers: k_render_occ_eval_shaded
(sparsefusion_amd/csrc/ngp_occ_shade.h through tests/hostemu/occ_shade_emu.cpp) -- eight lanes per ray, a wave-uniform sample loop with
the shuffles outside every predicate.  The emulator's shuffle is a whole-wave rendezvous: a lane that left the loop early, or a wave that
diverged across a shuffle, aborts the run.  Scenes of 1, 7, 8, 9 and 33 rays (a lone group, a wave's last group, a second wave, a second
workgroup) against the radius-2 ball at max_steps = 64, with a ray that misses, rays capped at max_steps and, at T_thresh = 0.3, rays
ended by the threshold.  No GPU."""
import numpy as np
import pytest
import torch

import occ_shaded_common as oc
import point_attrs_common as pc

pytestmark = pytest.mark.skipif(not oc.emu_available(), reason="host clang not found")
THRESHOLDS = (0.0, 0.3)


@pytest.fixture(scope="module")
def cases():
    """(N, T_thresh) -> scene, CPU restatement, emulated kernel at RATIO and at ratio 1 -- computed once, shared, never modified"""
    p, light = oc.params(), oc.unit(oc.LIGHT)
    out = {}
    for N in oc.SMALL_N:
        sc = oc.small_scene(N)
        for T in THRESHOLDS:
            out[N, T] = dict(p=p, sc=sc, light=light, rs=oc.restated(p, sc, light, oc.RATIO, T),
                             emu={r: oc.emu_shaded(p, sc, light, r, T) for r in (oc.RATIO, 1.0)})
    return out


@pytest.mark.parametrize("N", oc.SMALL_N)
def test_scene_holds_a_miss_a_capped_ray_and_a_threshold_ray(cases, N):
    rs0, rs3 = cases[N, 0.0]["rs"], cases[N, 0.3]["rs"]
    S = cases[N, 0.0]["sc"]["max_steps"]
    assert int(rs0["count"][0]) == S                                            # the first ray is capped at max_steps
    assert int(rs3["n_samples"][0]) < int(rs3["count"][0])                      # and ended by T_thresh = 0.3
    if N > 1:
        assert int(rs0["count"][1]) == 0                                        # the second one meets no occupied cell
        assert ((rs0["count"] > 0) & (rs0["count"] < S)).any()                  # some leave the ball before the cap


@pytest.mark.parametrize("N", oc.SMALL_N)
def test_sample_counts_equal_the_oracle_march(cases, N):
    """T_thresh = 0: no ray ends early, n_samples is the C oracle's per-ray march count on every ray (the host build of Marcher takes
    the oracle's steps: no contraction difference); T_thresh = 0.3: the restatement's count of composited samples, give or take the
    one sample at the threshold."""
    for T in THRESHOLDS:
        c = cases[N, T]
        for r in (oc.RATIO, 1.0):
            got = c["emu"][r]["n_samples"].long()
            if T == 0.0:
                assert torch.equal(got, c["rs"]["count"]), (r, got.tolist(), c["rs"]["count"].tolist())
            else:                                   # float32 against float64 transmittance: the threshold may fall one sample apart
                hit = c["rs"]["count"] > 0
                assert ((got - c["rs"]["n_samples"]).abs() <= 1).all() and (got <= c["rs"]["count"]).all() and (got[hit] >= 1).all()


@pytest.mark.parametrize("T", THRESHOLDS)
@pytest.mark.parametrize("N", oc.SMALL_N)
def test_outputs_within_the_derived_bounds_of_the_restatement(cases, N, T):
    """image within 2e-5 + T_thresh + (1 - ratio) sum w delta per ray; weights_sum, depth and normal_image within the bounds
    occ_shaded_common derives from the same density tolerances.  Every element is written (NaN pre-fill), the miss ray is all zero."""
    c = cases[N, T]
    rs, got, sc = c["rs"], c["emu"][oc.RATIO], c["sc"]
    for k in ("image", "weights_sum", "depth", "normal_image"):
        assert not torch.isnan(got[k]).any(), k
    err = {k: (got[k].double() - rs[k].double()).abs().numpy() for k in ("image", "weights_sum", "depth", "normal_image")}
    bounds = dict(image=oc.image_bound(rs)[:, None], weights_sum=oc.weights_bound(rs), depth=oc.depth_bound(rs, sc["fars"]),
                  normal_image=oc.normal_bound(rs)[:, None])
    print(f"N={N} T_thresh={T}: " + ", ".join(f"{k} {float(err[k].max()):.2e} (bound {float(np.max(bounds[k])):.2e})" for k in err))
    for k in err:
        assert (err[k] <= bounds[k]).all(), k
    if T == 0.0:
        assert float(oc.image_bound(rs).max()) <= oc.IMAGE_BOUND_CAP                # the bound is not vacuous here
    if N > 1:
        for k in ("image", "weights_sum", "depth", "normal_image"):
            assert float(got[k][1].abs().max()) == 0.0, k
        assert int(got["n_samples"][1]) == 0


@pytest.mark.parametrize("T", THRESHOLDS)
@pytest.mark.parametrize("N", oc.SMALL_N)
def test_ratio_one_is_the_albedo_kernel_bit_for_bit(cases, N, T):
    """ambient_ratio = 1: lambertian is exactly 1 and image / depth / weights_sum equal the emulated k_render_occ_eval's bit for bit
    -- same arithmetic, same order; depth, weights_sum, normal_image and n_samples do not depend on the ratio."""
    c = cases[N, T]
    alb = oc.emu_albedo(c["p"], c["sc"], T)
    for k in ("image", "depth", "weights_sum"):
        assert np.array_equal(pc.bits(c["emu"][1.0][k]), pc.bits(alb[k])), k
    for k in ("depth", "weights_sum", "normal_image"):
        assert np.array_equal(pc.bits(c["emu"][1.0][k]), pc.bits(c["emu"][oc.RATIO][k])), k
    if T == 0.0:
        assert float((c["emu"][1.0]["image"] - c["emu"][oc.RATIO]["image"]).abs().max()) > 1e-2 or N == 1      # the shading shows


def test_nullable_outputs_are_skipped_in_turn_and_jitter_moves_the_samples(cases):
    c = cases[9, 0.0]
    full = c["emu"][oc.RATIO]
    for skip in ("normal", "count"):
        part = oc.emu_shaded(c["p"], c["sc"], c["light"], oc.RATIO, 0.0, **{skip: False})
        assert part["normal_image" if skip == "normal" else "n_samples"] is None
        for k, v in part.items():
            if v is not None:
                assert np.array_equal(v.numpy().view(np.uint32), full[k].numpy().view(np.uint32)), (skip, k)
    # a jittered first sample (the `noises` input): still the albedo kernel at ratio 1, and not the unjittered render
    nz = torch.rand(9, generator=torch.Generator().manual_seed(3))
    jit = oc.emu_shaded(c["p"], c["sc"], c["light"], 1.0, 0.0, noises=nz)
    alb = oc.emu_albedo(c["p"], c["sc"], 0.0, noises=nz)
    for k in ("image", "depth", "weights_sum"):
        assert np.array_equal(pc.bits(jit[k]), pc.bits(alb[k])), k
    assert not np.array_equal(pc.bits(jit["depth"]), pc.bits(c["emu"][1.0]["depth"]))
