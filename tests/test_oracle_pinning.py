"""Pin the CPU oracle to the reference (CPU-only tests).

tests/golden/ref_*.npz hold inputs and the outputs the reference's OWN sources produced for
them: DistributionRayTracer/{vector,boundingBox,bvh,grid}.cpp and the header-only camera.h,
maths.h, color.h and scene.h:Light, compiled unmodified with g++ -O2 outside this repository
(tests/golden/README.md).  Every comparison below is bitwise.

Parts that cannot be compiled without stand-ins (scene.cpp primitives/loader, main.cpp
rayTracing/renderScene) are pinned end to end by reference-run numbers the survey recorded
(SURVEY.md §6): 1 436 437 BVH traversals for the Whitted dragon_assignment1 frame, and the
814 318-cell uniform grid of dragon.p3f.
"""
from pathlib import Path

import numpy as np
import pytest

GOLD = Path(__file__).resolve().parent / "golden"
CASES = ["tiny", "mixed", "tris2k"]


def load(case):
    return np.load(GOLD / f"ref_{case}.npz")


def scene_of(O, g, tmp_path):
    p = tmp_path / "scene.p3f"
    p.write_bytes(g["scene_text"].tobytes())
    return O.Scene.load_p3f(p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", CASES)
def test_bvh_build_identical_to_reference(oracle_mod, tmp_path, case):
    O = oracle_mod
    g = load(case)
    s = scene_of(O, g, tmp_path)
    s.set_accel("bvh")
    s.build()
    mine = s.bvh_export()
    for k in ("leaf", "index", "nobjs", "order"):
        np.testing.assert_array_equal(mine[k], g["bvh_" + k], err_msg=k)
    np.testing.assert_array_equal(bits(mine["boxes"]), bits(g["bvh_boxes"]))


@pytest.mark.parametrize("case", CASES)
def test_bvh_traversal_identical_to_reference(oracle_mod, tmp_path, case):
    O = oracle_mod
    g = load(case)
    s = scene_of(O, g, tmp_path)
    s.set_accel("bvh")
    s.build()
    t, n, obj = s.trace_closest(g["rays"])
    assert (g["bvh_obj"] >= 0).sum() > len(t) // 10
    np.testing.assert_array_equal(obj, g["bvh_obj"])
    np.testing.assert_array_equal(bits(t), bits(g["bvh_t"]))
    np.testing.assert_array_equal(bits(n), bits(g["bvh_n"]))
    np.testing.assert_array_equal(s.trace_shadow(g["shadow_rays"]), g["bvh_occ"])


@pytest.mark.parametrize("case", ["mixed", "tris2k"])
def test_grid_identical_to_reference(oracle_mod, tmp_path, case):
    O = oracle_mod
    g = load(case)
    s = scene_of(O, g, tmp_path)
    s.set_accel("grid")
    s.build()
    gr = s.grid_export()
    assert tuple(gr["dims"]) == tuple(g["grid_dims"])
    np.testing.assert_array_equal(bits(gr["bmin"]), bits(g["grid_bmin"]))
    np.testing.assert_array_equal(bits(gr["bmax"]), bits(g["grid_bmax"]))
    np.testing.assert_array_equal(gr["cell_start"], g["grid_cell_start"])
    np.testing.assert_array_equal(gr["cell_objs"], g["grid_cell_objs"])
    t, n, obj = s.trace_closest(g["grid_rays"])
    np.testing.assert_array_equal(obj, g["grid_obj"])
    np.testing.assert_array_equal(bits(t), bits(g["grid_t"]))
    np.testing.assert_array_equal(bits(n), bits(g["grid_n"]))
    np.testing.assert_array_equal(s.trace_shadow(g["grid_rays"]), g["grid_occ"])


def test_aabb_hit_identical_to_reference(oracle_mod):
    O = oracle_mod
    g = load("misc")
    hit, t, ins = O.aabb_hit(g["aabb_boxes"], g["aabb_rays"])
    np.testing.assert_array_equal(hit, g["aabb_hit"])
    np.testing.assert_array_equal(ins, g["aabb_inside"])
    m = hit == 1
    np.testing.assert_array_equal(bits(t[m]), bits(g["aabb_t"][m]))


def test_camera_identical_to_reference(oracle_mod):
    O = oracle_mod
    g = load("misc")
    for ci, c in enumerate(g["cam_params"]):
        s = O.Scene.new()
        s.set_camera(c[0:3], c[3:6], c[6:9], c[9], c[10], int(c[11]), int(c[12]), c[13], c[14])
        np.testing.assert_array_equal(bits(s.camera_frame()), bits(g["cam_frames"][ci]))
        for dof in (0, 1):
            mine = s.primary_rays(g["cam_samples"][ci], dof=bool(dof))
            np.testing.assert_array_equal(bits(mine), bits(g["cam_rays"][ci, dof]))


def test_light_vector_color_identical_to_reference(oracle_mod):
    O = oracle_mod
    g = load("misc")
    q = g["light_quad"]
    s = O.Scene.new()
    s.add_light_quad(q[0:3], [1, 1, 1], q[3:6], q[6:9], 16)
    np.testing.assert_array_equal(bits(s.light_points(0, g["light_samples"])), bits(g["light_points"]))
    nrm, ln, cr, dt = O.vector_ops(g["vec_a"], g["vec_b"])
    for mine, key in ((nrm, "vec_normalize"), (ln, "vec_length"), (cr, "vec_cross"), (dt, "vec_dot")):
        np.testing.assert_array_equal(bits(mine), bits(g[key]), err_msg=key)
    cl, ex, u8 = O.color_ops(g["col_in"])
    np.testing.assert_array_equal(bits(cl), bits(g["col_clamp"]))
    np.testing.assert_array_equal(bits(ex), bits(g["col_exp"]))
    np.testing.assert_array_equal(u8, g["col_u8"])


@pytest.mark.parametrize("sphere", [0, 1])
def test_rng_draw_order_identical_to_reference(oracle_mod, sphere):
    """maths.h rnd_unit_disk/sphere as compiled by g++: same values AND the same number of
    rand() calls per draw — this pins the right-to-left argument evaluation (first draw lands
    in the last component) that keyed-RNG parity depends on."""
    O = oracle_mod
    g = load("misc")
    vals, calls = O.rnd(99, 1234, len(g[f"rnd{sphere}_calls"]), sphere, glibc_rand_max=True)
    np.testing.assert_array_equal(calls, g[f"rnd{sphere}_calls"])
    np.testing.assert_array_equal(bits(vals), bits(g[f"rnd{sphere}_vals"]))


def test_crt_rand_mode_is_the_msvc_sequence(oracle_mod):
    """The oracle's lcg mode (orc_options.lcg: the reference runs' own RNG) draws
    the MSVC CRT sequence: after srand(1), rand() returns 41, 18467, 6334, 26500, 19169, ... (the
    published first values of that generator), and 15-bit draws for any seed."""
    assert oracle_mod.crt_rand(1, 8) == [41, 18467, 6334, 26500, 19169, 15724, 11478, 29358]
    d = oracle_mod.crt_rand(12345, 1000)
    assert min(d) >= 0 and max(d) <= 0x7FFF and len(set(d)) > 900


def test_dragon_assignment1_traversal_count_matches_reference_run(oracle_mod, tmp_path):
    """the reference renders dragon_assignment1 (Whitted, BVH, 512x512) with
    1 436 437 BVH::Traverse calls (closest + shadow).  RNG-independent, so it pins primitive
    intersection, the BVH and the rayTracing recursion/branching end to end.  The scene comes
    from the shipped-scenes data fixture (tests/golden/shipped_scenes.npz)."""
    from tests import shipped

    O = oracle_mod
    s = O.Scene.load_p3f(shipped.write(tmp_path, "dragon_assignment1"),
                         skybox_faces=shipped.skybox_faces("dragon_assignment1"))
    s.build()
    img, st = s.render(seed=1)
    assert st["closest_calls"] + st["shadow_calls"] == 1436437
    assert np.isfinite(img).all()


def test_dragon_grid_cell_count_matches_reference_run(oracle_mod, tmp_path):
    """dragon.p3f builds a uniform grid of 814 318 cells."""
    from tests import shipped

    O = oracle_mod
    s = O.Scene.load_p3f(shipped.write(tmp_path, "dragon"), skybox_faces=shipped.skybox_faces("dragon"))
    s.build()
    d = s.grid_export()["dims"]
    assert d[0] * d[1] * d[2] == 814318


def test_shipped_scene_fixture_is_byte_identical_to_reference():
    """tests/golden/shipped_scenes.npz rebuilds every shipped P3F file byte for byte: the text put
    together from the fixture's head and mesh blocks has the SHA-1 that make_shipped_scenes.py
    recorded of the reference's file."""
    import hashlib

    from tests import shipped

    assert len(shipped.names()) == 10
    for name in shipped.names():
        raw = shipped.text(name)
        assert hashlib.sha1(raw).hexdigest().encode() == shipped._npz()[f"{name}/sha1"].tobytes(), name
