"""Kernel-logic tests of the mesh clean-up on CPU fibers: the kernels of sparsefusion_amd/csrc/mesh_clean.h (through
tests/hostemu/mesh_clean_emu.cpp) against scipy's connected components, re-labelled to the smallest vertex index, and the numpy
restatement of the keep rule and compaction (mesh_clean_common) -- exact equality, vertex rows as bits.  Every case of the list
except the 1.1 M-face one, the marching-cubes mesh of the 48^3 blob volume included (from the numpy marching cubes of
tests/mesh_ref.py); workgroups of 256 and of 64 lanes, one thread per element and a few workgroups striding over the elements.

The hook, flatten and count kernels run with the emulator's atomics as rendezvous: the lanes of ONE WAVE advance one atomic at a
time, in alternating order, so a compare-and-swap does meet a word that changed after it was read.  That is the limit of the
schedule: the emulator runs a wave to its end before the next wave and workgroups one after the other, so words are never contended
across waves or workgroups here; that contention is met on the GPU only (the two-run and large cases of test_gpu_mesh_clean.py).
The `clash` case makes the in-wave contention intentional: 64 lanes of one wave unite the same two roots, then the same root with
vertex 0.  A lane that waited for another would never return here: lanes run one after the other.  No GPU."""
import numpy as np
import pytest

import mesh_clean_common as mc

pytestmark = pytest.mark.skipif(not mc.emu_available(), reason="host clang not found")

GEOMETRIES = ((256, 0), (64, 0), (256, 3), (64, 5))            # (lanes per workgroup, cap on the workgroups; 0: none)


@pytest.mark.parametrize("nt,max_blocks", GEOMETRIES)
@pytest.mark.parametrize("name", mc.SMALL_CASES)
def test_components_equal_scipy(name, nt, max_blocks):
    c = mc.case(name)
    got = mc.emu_components(c["faces"], c["V"], nt, max_blocks)
    mc.assert_components_equal(got, c["ref"])
    if c["faces"].shape[0] == 0 or c["V"] == 0:                  # the defined empty result
        assert np.array_equal(got["vertex_label"], np.arange(c["V"])) and not got["faces_per_label"].any()
        assert (got["n_components"], got["largest"]) == (0, 0) and got["n_invalid"] == c["faces"].shape[0]


@pytest.mark.parametrize("nt,max_blocks", GEOMETRIES[:1] + GEOMETRIES[3:])
@pytest.mark.parametrize("name", mc.SMALL_CASES)
def test_clean_equals_the_restatement(name, nt, max_blocks):
    c = mc.case(name)
    for rule in c["rules"]:
        got = mc.emu_clean(c["vertices"], c["faces"], c["V"], c["ref"], *rule, nt=nt, max_blocks=max_blocks)
        mc.assert_clean_equal(got, c["clean"][rule])


def test_face_label_is_optional():
    c = mc.case("mixed")
    got = mc.emu_components(c["faces"], c["V"], with_face_label=False)
    assert bool((got["face_label"] == mc.SENTINEL).all())
    got["face_label"] = c["ref"]["face_label"]
    mc.assert_components_equal(got, c["ref"])


def test_the_cases_hold_what_they_are_for():
    m = mc.case("mixed")["ref"]
    assert (m["n_components"], m["largest"], m["n_invalid"]) == (4, 4, 4)          # two tetrahedra, a triangle, a degenerate face
    assert m["vertex_label"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 8, 8, 8, 11, 12, 12] and m["faces_per_label"][11] == 0
    s = mc.case("strip")["ref"]
    assert s["n_components"] == 1 and s["largest"] == 20011 and not s["vertex_label"].any()
    many = mc.case("many")
    sizes = many["ref"]["faces_per_label"][many["ref"]["faces_per_label"] > 0]
    assert many["ref"]["n_components"] == 1003 and set(sizes.tolist()) == set(range(1, 13))
    kept = {r: len(set(many["ref"]["face_label"][t[3]].tolist())) for r, t in many["clean"].items()}
    assert kept[5, 0.0] > kept[6, 0.0] > kept[7, 0.0] and kept[0, 0.5] == kept[6, 0.0] and kept[12, 0.51] == kept[0, 1.0]
    assert kept[0, 0.0] == 1003 and kept[3, 0.75] == int((sizes >= 9).sum())
    for F in (255, 256, 257, 1025):
        r = mc.case(f"rand{F}")
        assert r["faces"].shape[0] == F and r["ref"]["n_components"] > 1


@pytest.mark.parametrize("nt,max_blocks", GEOMETRIES)
def test_marching_cubes_blobs_only_the_large_one_remains(nt, max_blocks):
    """one large blob, one small blob and three single-cell specks: five components; min_fraction = 0.5 leaves the large blob, a
    closed surface of Euler characteristic 2"""
    c = mc.blob_case()
    ref, V = c["ref"], c["V"]
    sizes = np.sort(ref["faces_per_label"][ref["faces_per_label"] > 0])
    assert ref["n_components"] == 5 and ref["n_invalid"] == 0 and sizes[:3].tolist() == [8, 8, 8] and sizes[4] > 4 * sizes[3] > 4 * 8
    got = mc.emu_components(c["faces"], V, nt, max_blocks)
    mc.assert_components_equal(got, ref)
    v2, f2, vi, fi = mc.emu_clean(c["vertices"], c["faces"], V, got, 8, 0.5, nt=nt, max_blocks=max_blocks)
    mc.assert_clean_equal((v2, f2, vi, fi), c["clean"][8, 0.5])
    assert f2.shape[0] == int(sizes[4]) and np.array_equal(mc.bits(v2), mc.bits(c["vertices"][vi]))
    assert bool((np.diff(vi) > 0).all()) and bool((np.diff(fi) > 0).all())
    after = mc.reference_components(f2, v2.shape[0])
    assert after["n_components"] == 1 and not after["vertex_label"].any()
    assert mc.closed_and_euler(f2, v2.shape[0]) == (True, 2)
    # the default keeps a speck's octahedron of exactly 8 faces; min_faces = 9 drops the three specks
    for rule, n_faces in (((8, 0.0), int(sizes.sum())), ((9, 0.0), int(sizes[3] + sizes[4]))):
        out = mc.emu_clean(c["vertices"], c["faces"], V, got, *rule, nt=nt, max_blocks=max_blocks)
        mc.assert_clean_equal(out, c["clean"][rule])
        assert out[1].shape[0] == n_faces


def test_the_clash_case_is_one_component_through_three_roots():
    c = mc.case("clash")
    assert c["faces"].shape == (128, 3) and c["ref"]["n_components"] == 1 and c["ref"]["largest"] == 128
    assert not c["ref"]["vertex_label"].any() and set(c["faces"][:64, 0].tolist()) == {1, 2} and not c["faces"][64:, 2].any()
