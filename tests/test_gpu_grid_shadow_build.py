"""The Grid scene's shadow tree built and committed on the device (drt_build_grid_device with
DRT_GRID_SHADOW_LBVH / DRT_GRID_SHADOW_PLOC, csrc/hip/drt_grid_tree_commit.hip) through
Renderer.upload(scene, build="device", shadow_tree="device" | "ploc"): frames against the Grid walk's bit for
bit with the tree taking the queries, the device commit against the host commit of the same tree
(drt_upload_grid_shadow_bvh) frame for frame and counter for counter, and the cases that keep no tree.

Sizes of the commit test: 2 (one record with two leaf children), 3, 65 (one over a wave), 257 (one over a
workgroup), 20 000; two triangles whose cell ranges span the grid; plane values far from the origin.
"""
import numpy as np
import pytest

import tests.test_gpu_grid_build as B
from tests.test_gpu_grid_tree import CASES, bits, grid_scene

pytestmark = pytest.mark.gpu

KIND = {"device": 1, "ploc": 2}
WHITTED = {"max_depth": 3, "light_spp": 1, "roughness": 0.0}  # on a spp = 0 scene: the Whitted quad-light frame


@pytest.fixture(scope="module")
def drt():
    import distributionraytracer_amd as d

    return d


@pytest.fixture(scope="module")
def renderer(drt):
    r = drt.Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("nocert", [False, True])
@pytest.mark.parametrize("commit", ["host", "device"])
@pytest.mark.parametrize("shadow_tree", ["device", "ploc"])
@pytest.mark.parametrize("spp,first,light_spp,md,rough", [CASES[0], CASES[2], CASES[4]])
def test_frame_is_the_walks_and_the_tree_takes_the_queries(drt, renderer, monkeypatch, spp, first, light_spp, md,
                                                           rough, shadow_tree, commit, nocert):
    if nocert:
        monkeypatch.setenv("DRT_GRID_TREE_NOCERT", "1")  # read by the upload
    s = grid_scene(drt, first, 20_000, spp=spp)
    renderer.upload(s, build="device", commit=commit, shadow_tree=shadow_tree)
    kw = {"max_depth": md, "light_spp": light_spp, "roughness": rough}
    plan = renderer.plan(renderer.frame_params(seed=6, **kw))
    assert plan["passes"] == 2 and plan["wavefront"]
    assert renderer.grid_build_info()["shadow_tree"] == KIND[shadow_tree]
    tree = renderer.render(seed=6, **kw)
    monkeypatch.setenv("DRT_GRID_SHADOW_TREE", "0")
    walk = renderer.render(seed=6, **kw)
    np.testing.assert_array_equal(bits(tree), bits(walk))
    wst_img = renderer.render(seed=6, stats=True, **kw)
    wst = renderer.stats()
    monkeypatch.setenv("DRT_GRID_SHADOW_TREE", "2")
    tst_img = renderer.render(seed=6, stats=True, **kw)
    tst = renderer.stats()
    np.testing.assert_array_equal(bits(tst_img), bits(walk))
    np.testing.assert_array_equal(bits(wst_img), bits(walk))
    assert tst["samples"] == wst["samples"] and tst["shadow_rays"] == wst["shadow_rays"] > 0
    assert tst["wide_shadow_rays"] > 0.95 * tst["shadow_rays"], (tst["wide_shadow_rays"], tst["shadow_rays"])


def commit_scene(drt, name):
    """-> the scene and its stats frame's arguments"""
    if name == "floor":
        return B.grid_scene(drt, name)[0], {}
    if name == "far":  # the camera moved with the triangles (the point light stays: every query is long)
        import bench

        s, c = grid_scene(drt, "quad", 8_000, spp=9, seed=3, scale=(3.0, 250.0)), bench.CAMERA
        s.set_camera(3.0 * np.asarray(c["eye"]) + 250.0, 3.0 * np.asarray(c["at"]) + 250.0, c["up"], c["fovy"],
                     c["hither"], 40, 36, 0.0, 1.0)
        return s, {"max_depth": 3}
    return (grid_scene(drt, "quad", name, spp=0), WHITTED) if name < 1024 else (grid_scene(drt, "quad", name), {})


@pytest.mark.parametrize("shadow_tree", ["device", "ploc"])
@pytest.mark.parametrize("name", [2, 3, 65, 257, 20_000, "floor", "far"])
def test_device_commit_is_the_host_commit_of_the_same_tree(drt, renderer, monkeypatch, name, shadow_tree):
    scene, kw = commit_scene(drt, name)
    renderer.upload(scene, build="device", commit="device", install=True, shadow_tree=shadow_tree)
    assert renderer.grid_build_info()["shadow_tree"] == KIND[shadow_tree]
    plan = renderer.plan(renderer.frame_params(seed=6, **kw))
    if not (plan["passes"] == 2 and plan["wavefront"]):  # the plan keeps scenes under 1 024 objects in one pass
        monkeypatch.setenv("DRT_WHITTED_TWO_PASS", "2")
        monkeypatch.setenv("DRT_AA_TWO_PASS_MIN_PRIMS", "1")
        plan = renderer.plan(renderer.frame_params(seed=6, **kw))
    assert plan["passes"] == 2 and plan["wavefront"]
    monkeypatch.setenv("DRT_GRID_SHADOW_TREE", "2")  # stats frames on the tree
    dev_img = renderer.render(seed=6, stats=True, **kw)
    dev = renderer.stats()
    renderer.upload(scene)  # the host path: the installed tree through drt_upload_grid_shadow_bvh
    host_img = renderer.render(seed=6, stats=True, **kw)
    host = renderer.stats()
    np.testing.assert_array_equal(bits(dev_img), bits(host_img))
    timing = [k for k in dev if k.endswith("_ms") or k.startswith("cycles_") or k.startswith("wave_")]
    diff = {k: (dev[k], host[k]) for k in dev if k not in timing and dev[k] != host[k]}
    print(name, shadow_tree, {k: dev[k] for k in dev if k.startswith("wide_")}, "counters differing:", diff)
    assert not diff


@pytest.mark.parametrize("name", ["soup1", "mixed"])
def test_scenes_without_a_tree_keep_the_walk(drt, renderer, name):
    renderer.upload(B.grid_scene(drt, name)[0], build="device", commit="device", shadow_tree="device")
    assert renderer.grid_build_info()["shadow_tree"] == 0
    frame = renderer.render(seed=7)
    renderer.upload(B.grid_scene(drt, name)[0])
    np.testing.assert_array_equal(bits(frame), bits(renderer.render(seed=7)))


def test_no_install_brings_nothing_back(drt, renderer):
    scene = B.grid_scene(drt, "soup20k")[0]
    unbuilt = scene.grid_export()
    renderer.upload(scene, build="device", commit="device", install=False, shadow_tree="ploc")
    assert renderer.grid_build_info()["shadow_tree"] == 2
    B.same_grid(scene.grid_export(), unbuilt)
    frame = renderer.render(seed=7)
    renderer.upload(B.grid_scene(drt, "soup20k")[0], build="device", shadow_tree="ploc")
    np.testing.assert_array_equal(bits(frame), bits(renderer.render(seed=7)))


def test_bad_shadow_tree_arguments(drt, renderer):
    grid, bvh = B.grid_scene(drt, "soup65")[0], B.make_scene(drt, "soup65", accel="bvh")[0]
    for scene, kw in [(grid, {"build": "device", "shadow_tree": "sah"}), (grid, {"build": "host", "shadow_tree": "ploc"}),
                      (bvh, {"build": "device", "shadow_tree": "device"})]:
        with pytest.raises(ValueError):
            renderer.upload(scene, **kw)
