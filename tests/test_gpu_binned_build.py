"""The device binned-SAH builder (drt_build_bvh_device_ex, csrc/hip/drt_bvh_binned.hip) through
Renderer.upload(scene, build="binned"): its tree against the host's (drt_scene_build) and against the reference
program's own (tests/golden/ref_*.npz) — leaf, index, nobjs and the boxes' bits equal, every leaf the same set of
objects, and the same sequence wherever a leaf's centroids are pairwise distinct on all three axes (elsewhere the
host's order is its sort's history); then the installed tree's answers and frames against the host tree's.

The scenes are tests/test_gpu_bvh_build.py's: 1, 2 (a leaf root), 3, 65 objects (one over the wave path's limit:
one level-wise round feeds two wave-built subtrees), 2 049 (one over a tile), 20 000 (several tiles, many nodes per
tile in late rounds); every centroid equal (the root is a fallback leaf of 600: the large-leaf sort, scene-order
ties); a zero-extent axis (scale 0); two far clusters (runs of empty buckets, +-FLT_MAX boxes in the costs); all
four primitive types.
"""
import pathlib

import numpy as np
import pytest

from tests.test_gpu_bvh_build import CASES, SOUPS, bits, drt, make_rays, make_scene, renderer  # noqa: F401

pytestmark = pytest.mark.gpu
GOLD = pathlib.Path(__file__).parent / "golden"


def compare(got, want, cen=None):
    """-> the exempt leaves, as (got's slice, the host's slice): those whose sequence may differ from the host's,
    because two of their objects share a centroid coordinate (cen: per-object centroids; without them no leaf
    is exempt).  An exempt leaf must still be in the builder's documented order on some axis: ascending
    centroid, equal keys in scene order."""
    for k in ("leaf", "index", "nobjs"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(bits(got["boxes"]), bits(want["boxes"]))
    exempt = []
    for i in np.flatnonzero(want["leaf"]):
        a, b = (t["order"][want["index"][i]: want["index"][i] + want["nobjs"][i]] for t in (got, want))
        assert sorted(a.tolist()) == sorted(b.tolist()), i
        if cen is None or all(len(np.unique(cen[b, x])) == len(b) for x in range(3)):
            assert (a == b).all(), (i, a, b)
        else:
            exempt.append((a.tolist(), b.tolist()))
            assert any((a == b[np.lexsort((b, cen[b, x]))]).all() for x in range(3)), (i, a, b)
    return exempt


def centroids(boxes):
    return (boxes[:, :3] + boxes[:, 3:]) / np.float32(2.0)


@pytest.mark.parametrize("name", CASES)
def test_equals_the_host_tree(name, drt, renderer):
    scene, boxes = make_scene(drt, name)[:2]
    renderer.upload(scene, build="binned")
    twin = make_scene(drt, name)[0]
    twin.build()
    cen = centroids(boxes)
    exempt = compare(scene.bvh_export(), twin.bvh_export(), cen)
    info = renderer.bvh_build_info()
    print(name, "exempt leaves:", len(exempt), "rounds:", info["rounds"], "depth:", info["depth"])
    assert info["builder"] == 2
    if name == "soup20k":
        # The one tie of the random soups: triangles 5710 and 18695 share a leaf and a centroid coordinate, so the
        # host's sequence there is its sort's history (it is the reverse); the builder's is scene order.
        assert exempt == [([5710, 18695], [18695, 5710])]
        assert (cen[5710] == cen[18695]).any()
    elif name in SOUPS:
        assert exempt == []


@pytest.mark.parametrize("case", ["tiny", "mixed", "tris2k"])
def test_equals_the_reference_tree(case, drt, renderer, tmp_path):
    g = np.load(GOLD / f"ref_{case}.npz")
    p = tmp_path / "s.p3f"
    p.write_bytes(g["scene_text"].tobytes())
    s = drt.Scene.load_p3f(p)
    s.set_accel("bvh")
    renderer.upload(s, build="binned")
    cen = None  # tiny, mixed: every leaf is held to the reference's sequence
    if case == "tris2k":  # one mesh ("mesh NV NT", vertices, 1-based triangles): its boxes by Triangle's formula
        rows = g["scene_text"].tobytes().decode().splitlines()
        at = next(k for k, r in enumerate(rows) if r.startswith("mesh "))
        nv, nt = map(int, rows[at].split()[1:])
        v = np.array([r.split() for r in rows[at + 1: at + 1 + nv]], np.float32)
        t = v[np.array([r.split() for r in rows[at + 1 + nv: at + 1 + nv + nt]], int) - 1]
        cen = centroids(np.concatenate([t.min(1) - np.float32(0.001), t.max(1) + np.float32(0.001)], 1))
    exempt = compare(s.bvh_export(), {k: g["bvh_" + k] for k in ("leaf", "index", "nobjs", "order", "boxes")}, cen)
    print(case, "exempt leaves:", exempt)
    if case == "tris2k":  # the two floor triangles, the scene's last two: same box, same leaf
        assert len(cen) == 2002 and (cen[2000] == cen[2001]).all()
        assert exempt == [([2000, 2001], [2001, 2000])]  # scene order here, the sort's history in the reference


@pytest.mark.parametrize("commit", ["host", "device"])
@pytest.mark.parametrize("name", ["soup20k", "mixed"])
def test_installed_tree_answers(name, commit, drt, renderer):
    scene, _, eye, lo, hi = make_scene(drt, name)
    rays = make_rays(name, eye, lo, hi)
    renderer.upload(scene, build="binned", commit=commit)
    assert renderer.bvh_commit_info()["on_device"] == (commit == "device")
    t, nrm, obj = renderer.trace_closest(rays)
    ht, hn, ho = scene.trace_cpu(rays)
    assert (bits(t) == bits(ht)).all() and (bits(nrm) == bits(hn)).all() and (obj == ho).all()
    length = np.random.default_rng(5).uniform(0.05, 4.0, (len(rays), 1)).astype(np.float32)
    sh = np.concatenate([rays[:, :3], rays[:, 3:] * length], 1)
    assert (renderer.trace_shadow(sh) == scene.trace_cpu(sh, shadow=True)).all()
    counts = ("closest_rays", "shadow_rays", "closest_inner", "closest_leaf", "shadow_inner", "shadow_leaf",
              "closest_prims", "shadow_prims")
    frame, stats = renderer.render(seed=7, stats=True), renderer.stats()
    renderer.upload(make_scene(drt, name)[0], build="host")
    assert renderer.render(seed=7, stats=True).tobytes() == frame.tobytes()
    assert [renderer.stats()[k] for k in counts] == [stats[k] for k in counts]


def test_arguments(drt, renderer):
    with pytest.raises(ValueError):
        renderer.upload(make_scene(drt, "soup3", accel="grid")[0], build="binned")
    scene = make_scene(drt, "soupT1")[0]
    frame = renderer.upload(scene, build="binned").render(seed=7)
    group = drt.RendererGroup([0])
    try:
        assert group.upload(make_scene(drt, "soupT1")[0], build="binned").render(seed=7).tobytes() == frame.tobytes()
    finally:
        group.close()
