"""The device LBVH builder (drt_build_bvh_device, csrc/hip/drt_bvh_build.hip) through Renderer.upload(scene,
build="device"): the returned tree's structure and boxes exactly, the device walk against the host walk of
the same tree, closest hits against the tree-free scan, frames against the host-built tree's, determinism.

Scene sizes are the smallest at which a stage can go wrong: 1, 2 (a leaf root), 3, 65 (one over a wave),
T + 1 (one over the sort tile) and 20 000 (several workgroups everywhere, a partial last tile); all Morton
keys equal; one axis of zero extent; long shared key prefixes; mixed primitives.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 2048  # keys per sort workgroup (kBvhSortTile)
SOUPS = {"soup1": 1, "soup2": 2, "soup3": 3, "soup65": 65, "soupT1": T + 1, "soup20k": 20000}
CASES = list(SOUPS) + ["same_centroid", "flat", "clusters", "mixed"]
N_RAYS = 4096


def triangles(name):
    import bench

    rng = np.random.default_rng(CASES.index(name) + 1)
    if name in SOUPS:
        return bench.synthetic_triangles(SOUPS[name], 3)[: SOUPS[name]]
    if name == "same_centroid":  # vertices a, -a, b with |b| <= |a|: the padded box is symmetric, its centroid 0
        a = rng.uniform(0.1, 1.0, (300, 3)) * rng.choice([-1.0, 1.0], (300, 3))
        v = np.concatenate([a, -a, a * rng.uniform(-1, 1, (300, 3))], 1)
        return np.concatenate([v, np.repeat(v[:1], 300, 0)]).astype(np.float32)
    if name == "flat":  # z spans [-h, h] exactly: every centroid has z = 0
        c = rng.uniform(-1, 1, (2000, 1, 3)) * (1, 1, 0)
        v = c + rng.uniform(-0.05, 0.05, (2000, 3, 3))
        v[:, 0, 2], v[:, 1, 2] = 0.03125, -0.03125
        v[:, 2, 2] = rng.uniform(-0.03, 0.03, 2000)
        return v.reshape(-1, 9).astype(np.float32)
    c = np.repeat([[0.0, 0, 0], [1e3, 0, 0]], 1000, 0)[:, None, :]  # clusters
    return (c + rng.uniform(-5e-4, 5e-4, (2000, 3, 3))).reshape(-1, 9).astype(np.float32)


def make_scene(drt, name, accel="bvh", res=(64, 48)):
    """-> (scene, per-object boxes (n, 6) in float32 by the formulas of GetBoundingBox())."""
    import bench

    rng = np.random.default_rng(11)
    s = drt.Scene()
    boxes = []
    s.set_background((0.078, 0.361, 0.753))
    s.set_accel(accel)
    s.set_spp(16)
    s.add_light_quad((4, 3, 2), (1, 1, 1), (4, 2, 2), (3, 3, 2), 16)
    s.add_material((1, 0.9, 0.7), 0.5, (1, 1, 1), 0.5, 30.0827, 0, 1)
    if name == "mixed":  # the recipe of tests/test_gpu_cell_tree.py::mixed_scene
        sph = np.concatenate([rng.uniform(-1, 1, (300, 3)), rng.uniform(0.02, 0.12, (300, 1))], 1).astype(np.float32)
        for x, y, z, r in sph:
            s.add_sphere((x, y, z), float(r))
        boxes.append(np.concatenate([sph[:, :3] - sph[:, 3:], sph[:, :3] + sph[:, 3:]], 1))
        for mn in rng.uniform(-1, 0.8, (12, 3)):
            mx = mn + rng.uniform(0.05, 0.3, 3)
            s.add_box(mn, mx)
            boxes.append(np.concatenate([mn, mx]).astype(np.float32)[None])
        s.add_plane_nd((0.0, 0.0, 1.0), 1.0)
        boxes.append(np.array([[-1, -1, -1, 1, 1, 1]], np.float32))
        tris = bench.synthetic_triangles(720, 5)[:720]
    else:
        tris = triangles(name)
    s.add_triangles(tris)
    v = tris.reshape(-1, 3, 3)
    boxes.append(np.concatenate([v.min(1) - np.float32(0.001), v.max(1) + np.float32(0.001)], 1))
    boxes = np.concatenate(boxes).astype(np.float32)
    lo, hi = boxes[:, :3].min(0).astype(np.float64), boxes[:, 3:].max(0).astype(np.float64)
    eye = (lo + hi) / 2 + (hi - lo + 1.0) * (1.1, 0.9, 0.7)
    s.set_camera(eye, (lo + hi) / 2, (0, 0, 1), 45.0, 0.01, res[0], res[1], 0.0, 1.0)
    return s, boxes, eye, lo, hi


def make_rays(name, eye, lo, hi):
    """camera rays, axis-parallel rays, random origins inside the scene box: (3 * N_RAYS, 6), unit d"""
    rng = np.random.default_rng(100 + CASES.index(name))
    n = N_RAYS
    target = rng.uniform(lo, hi, (n, 3))
    cam = np.concatenate([np.broadcast_to(eye, (n, 3)), target - eye], 1)
    ax = rng.integers(0, 3, n)
    o = rng.uniform(lo, hi, (n, 3))
    o[np.arange(n), ax] = lo[ax] - 1.0
    d = np.zeros((n, 3))
    d[np.arange(n), ax] = 1.0
    inside = np.concatenate([rng.uniform(lo, hi, (n, 3)), rng.normal(size=(n, 3))], 1)
    r = np.concatenate([cam, np.concatenate([o, d], 1), inside])
    r[:, 3:] /= np.linalg.norm(r[:, 3:], axis=1, keepdims=True)
    return r.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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
    """One device build per scene; the scene stays resident for the tests of this parameter."""
    name = request.param
    scene, boxes, eye, lo, hi = make_scene(drt, name)
    renderer.upload(scene, build="device")
    return dict(name=name, scene=scene, boxes=boxes, rays=make_rays(name, eye, lo, hi), tree=scene.bvh_export(),
                info=renderer.bvh_build_info())


def resident(case, renderer):
    """The case's scene on the renderer (another test may have uploaded its own since; the build is
    deterministic, so the tree is the one exported)."""
    if renderer.scene is not case["scene"]:
        renderer.upload(case["scene"], build="device")
    return renderer


def test_structure(case):
    tr, ob = case["tree"], case["boxes"]
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
            assert l > i and l + 1 < n_nodes
            stack += [(l, d + 1), (l + 1, d + 1)]
            want = np.concatenate([np.minimum(box[l, :3], box[l + 1, :3]), np.maximum(box[l, 3:], box[l + 1, 3:])])
        assert (bits(box[i]) == bits(want)).all(), i
    assert (seen == 1).all() and (covered == 1).all()
    n_leaves = int(leaf.astype(bool).sum())
    assert n_nodes == 2 * n_leaves - 1 and depth <= 95
    assert (case["info"]["n_nodes"], case["info"]["n_leaves"], case["info"]["depth"]) == (n_nodes, n_leaves, depth)
    if n <= 2:
        assert n_nodes == 1


def test_device_walk_equals_host_walk_of_the_same_tree(case, renderer):
    rays, scene = case["rays"], case["scene"]
    t, nrm, obj = resident(case, renderer).trace_closest(rays)
    ht, hn, ho = scene.trace_cpu(rays)
    assert (bits(t) == bits(ht)).all() and (bits(nrm) == bits(hn)).all() and (obj == ho).all()
    length = np.random.default_rng(5).uniform(0.05, 4.0, (len(rays), 1)).astype(np.float32)
    sh = np.concatenate([rays[:, :3], rays[:, 3:] * length], 1)
    assert (renderer.trace_shadow(sh) == scene.trace_cpu(sh, shadow=True)).all()


@pytest.mark.parametrize("case", CASES[:-1], indirect=True)
def test_closest_hits_equal_the_tree_free_scan(case, renderer, drt):
    """The triangle scenes: their boxes are padded by 1e-3, far above the slab test's rounding, so the
    boxes of a hit primitive are always entered and the closest t is the scan's."""
    flat = make_scene(drt, case["name"], accel="none")[0]
    flat.build()
    t, _, obj = resident(case, renderer).trace_closest(case["rays"])
    ft, _, fo = flat.trace_cpu(case["rays"])
    print(case["name"], "rays differing in t:", int((bits(t) != bits(ft)).sum()), "in object:", int((obj != fo).sum()))
    assert (bits(t) == bits(ft)).all()
    if case["name"] in SOUPS:  # elsewhere equal t on several objects is decided by the visit order
        assert (obj == fo).all()


@pytest.mark.parametrize("name", ["soup20k", "mixed"])
def test_frames_equal_the_host_tree_frames(name, drt, renderer):
    frames = []
    for build in ("host", "device"):
        scene = make_scene(drt, name)[0]
        renderer.upload(scene, build=build)
        frames.append((renderer.render(seed=7, stats=True).astype(np.float64), renderer.stats()))
    (a, sa), (b, sb) = frames
    print(name, "max |diff|", np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-5
    assert (sa["closest_rays"], sa["shadow_rays"]) == (sb["closest_rays"], sb["shadow_rays"])


def test_build_is_deterministic(drt, renderer):
    trees = []
    for _ in range(2):
        scene = make_scene(drt, "soup20k")[0]
        renderer.upload(scene, build="device")
        trees.append(scene.bvh_export())
    for k in trees[0]:
        assert trees[0][k].tobytes() == trees[1][k].tobytes(), k
