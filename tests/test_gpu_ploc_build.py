"""The device PLOC builder (drt_build_bvh_device_ex, csrc/hip/drt_bvh_ploc.hip) through Renderer.upload(scene,
build="ploc"): the tree's structure and boxes exactly, the device walk against the host walk of the same tree
under both commits, closest hits against the tree-free scan, frames against the host-built tree's, determinism,
and a surface-area cost below the LBVH's.

Sizes: 1, 2 (a leaf root), 3, 65 (one over a wave), 257 (one over a workgroup: the halo crosses its edge), 2049
(one over the sort tile), 20 000; every surface tying; one flat axis; mixed primitives; and chain800, a geometric
progression on which the search merges about two pairs a round (a numpy restatement of the rounds leaves 679 of
800 clusters after the 64 search rounds), so the forced rounds must run.
"""
from unittest import mock

import numpy as np
import pytest

import tests.test_gpu_bvh_build as B
from tests.test_gpu_bvh_build import bits

pytestmark = pytest.mark.gpu

OWN = {"soup257": 257, "chain800": 800}
CASES = ["soup1", "soup2", "soup3", "soup65", "soup257", "soupT1", "soup20k", "same_centroid", "flat", "mixed", "chain800"]
TRIANGLE_CASES = [c for c in CASES if c not in ("mixed", "chain800")]  # chain800: the 1e-3 padding is below float spacing


def own_triangles(name):
    import bench

    if name == "soup257":
        return bench.synthetic_triangles(257, 3)[:257]
    b = np.array([(0, 0, 0), (0.01, 0, 0.01), (0, 0.01, 0.01)]) + (1, 0, 0)
    return (1.04 ** np.arange(800)[:, None, None] * b).reshape(-1, 9).astype(np.float32)


def make(drt, name, accel="bvh"):
    """-> (scene, boxes, rays): B.make_scene's recipe, with this file's triangles for the cases B does not have"""
    if name in OWN:
        with mock.patch.object(B, "triangles", own_triangles):
            scene, boxes, eye, lo, hi = B.make_scene(drt, name, accel)
    else:
        scene, boxes, eye, lo, hi = B.make_scene(drt, name, accel)
    return scene, boxes, B.make_rays("soup3" if name in OWN else name, eye, lo, hi)


@pytest.fixture(scope="module")
def drt():
    import distributionraytracer_amd as d

    return d


@pytest.fixture(scope="module")
def renderer(drt):
    r = drt.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module", params=CASES)
def case(request, drt, renderer):
    scene, boxes, rays = make(drt, request.param)
    renderer.upload(scene, build="ploc")
    return dict(name=request.param, scene=scene, boxes=boxes, rays=rays, tree=scene.bvh_export(),
                info=renderer.bvh_build_info())


def sa_cost(tr):
    """(sum of inner surfaces + sum of leaf surfaces x objects) / the root's surface, in float64"""
    e = tr["boxes"][:, 3:].astype(np.float64) - tr["boxes"][:, :3]
    area = e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]
    leaf = tr["leaf"].astype(bool)
    return (area[~leaf].sum() + (area[leaf] * tr["nobjs"][leaf]).sum()) / area[0]


def test_structure(case):
    tr, ob, info = case["tree"], case["boxes"], case["info"]
    box, leaf, index, nobjs, order = tr["boxes"], tr["leaf"], tr["index"], tr["nobjs"], tr["order"]
    n, n_nodes = len(ob), len(leaf)
    assert sorted(order.tolist()) == list(range(n))
    seen, covered, depth, stack = np.zeros(n_nodes, int), np.zeros(n, int), 0, [(0, 1)]
    while stack:
        i, d = stack.pop()
        seen[i] += 1
        depth = max(depth, d)
        if leaf[i]:
            assert 1 <= nobjs[i] <= 2
            objs = order[index[i]: index[i] + nobjs[i]]
            covered[objs] += 1
            want = np.concatenate([ob[objs, :3].min(0), ob[objs, 3:].max(0)])
        else:
            l = int(index[i])
            assert i < l and l + 1 < n_nodes
            stack += [(l, d + 1), (l + 1, d + 1)]
            want = np.concatenate([np.minimum(box[l, :3], box[l + 1, :3]), np.maximum(box[l, 3:], box[l + 1, 3:])])
        assert (bits(box[i]) == bits(want)).all(), i
    assert (seen == 1).all() and (covered == 1).all()
    n_leaves = int(leaf.astype(bool).sum())
    assert n_nodes == 2 * n_leaves - 1 and (n > 2 or n_nodes == 1)
    assert depth <= 91 and (info["n_nodes"], info["n_leaves"], info["depth"]) == (n_nodes, n_leaves, depth)
    print(case["name"], "depth", depth, "rounds", info["rounds"], "forced", info["forced_rounds"])
    assert info["builder"] == 1
    if case["name"] == "chain800":
        assert info["rounds"] == 64 and info["forced_rounds"] > 0
    else:
        assert info["rounds"] <= 64 and info["forced_rounds"] == 0


@pytest.mark.parametrize("commit", ["host", "device"])
def test_device_walk_equals_host_walk_of_the_same_tree(case, renderer, commit):
    rays, scene = case["rays"], case["scene"]
    renderer.upload(scene, build="ploc", commit=commit)
    assert renderer.bvh_commit_info()["on_device"] == (commit == "device")
    t, nrm, obj = renderer.trace_closest(rays)
    ht, hn, ho = scene.trace_cpu(rays)
    assert (bits(t) == bits(ht)).all() and (bits(nrm) == bits(hn)).all() and (obj == ho).all()
    length = np.random.default_rng(5).uniform(0.05, 4.0, (len(rays), 1)).astype(np.float32)
    sh = np.concatenate([rays[:, :3], rays[:, 3:] * length], 1)
    assert (renderer.trace_shadow(sh) == scene.trace_cpu(sh, shadow=True)).all()


@pytest.mark.parametrize("case", TRIANGLE_CASES, indirect=True)
def test_closest_t_equals_the_tree_free_scan(case, renderer, drt):
    flat = make(drt, case["name"], accel="none")[0]
    flat.build()
    renderer.upload(case["scene"], build="ploc")
    t = renderer.trace_closest(case["rays"])[0]
    assert (bits(t) == bits(flat.trace_cpu(case["rays"])[0])).all()


@pytest.mark.parametrize("name", ["soup20k", "mixed"])
def test_frames(name, drt, renderer):
    frames = []
    for kw in (dict(build="host"), dict(build="ploc"), dict(build="ploc", commit="device")):
        renderer.upload(make(drt, name)[0], **kw)
        frames.append((renderer.render(seed=7, stats=True), renderer.stats()))
    (host, sh), (ploc, sp), (dploc, _) = frames
    print(name, "max |diff| to the host tree's frame", np.abs(host.astype(np.float64) - ploc).max())
    assert np.abs(host.astype(np.float64) - ploc).max() <= 1e-5
    assert (sh["closest_rays"], sh["shadow_rays"]) == (sp["closest_rays"], sp["shadow_rays"])
    assert ploc.tobytes() == dploc.tobytes()


def test_build_is_deterministic(drt, renderer):
    trees = []
    for _ in range(2):
        scene = make(drt, "soup20k")[0]
        renderer.upload(scene, build="ploc")
        trees.append(scene.bvh_export())
    for k in trees[0]:
        assert trees[0][k].tobytes() == trees[1][k].tobytes(), k


@pytest.mark.parametrize("case", ["soup20k", "flat"], indirect=True)
def test_surface_area_cost_is_below_the_lbvh(case, drt, renderer):
    """The search does something: not a measured threshold."""
    scene = make(drt, case["name"])[0]
    renderer.upload(scene, build="device")
    ploc, lbvh = sa_cost(case["tree"]), sa_cost(scene.bvh_export())
    print(case["name"], "surface-area cost: PLOC", ploc, "LBVH", lbvh)
    assert ploc < lbvh


def test_bad_build_arguments(drt, renderer):
    with pytest.raises(ValueError):
        renderer.upload(make(drt, "soup3", accel="grid")[0], build="ploc")
    with pytest.raises(ValueError):
        renderer.upload(make(drt, "soup3")[0], build="sah")
