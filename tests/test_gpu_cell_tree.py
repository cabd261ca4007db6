"""A Grid scene of any primitives: shadow queries on the cell tree (cell_tree_stream).

Grid::Traverse(Ray&) (grid.cpp:309-358) tests an object exactly when the ray crosses the object's cell
range, so a tree over the cell ranges with the walk's own primitive tests gives the walk's answers; the
queries it cannot decide within its margin are walked on the Grid.  The reference is the walk itself,
so every comparison here is exact equality.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAMILIES = ["uniform", "axis", "faces", "outside", "plane", "grazing"]


@pytest.fixture(scope="module", autouse=True)
def cell_tree_on():
    """The knob is off by default (profiles/grid_cell_tree_ab.jsonl); Scene.build and the upload read it."""
    mp = pytest.MonkeyPatch()
    mp.setenv("DRT_GRID_CELL_TREE", "1")
    yield
    mp.undo()


@pytest.fixture(scope="module")
def drt():
    import distributionraytracer_amd as d

    return d


@pytest.fixture(scope="module")
def renderer(drt):
    r = drt.Renderer(0)
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mixed_scene(drt, res=(40, 36), spp=16, first="quad"):
    """300 spheres, 12 boxes, the plane z = -1 (its box is [-1, 1]^3, scene.h:116) and 720 triangles:
    1033 objects, past the 1024 from which a frame is planned in two passes."""
    import bench

    rng = np.random.default_rng(11)
    s = drt.Scene()
    c = bench.CAMERA
    s.set_camera(c["eye"], c["at"], c["up"], c["fovy"], c["hither"], res[0], res[1], 0.0, 1.0)
    s.set_background((0.078, 0.361, 0.753))
    s.set_accel("grid")
    s.set_spp(spp)
    lights = [lambda: s.add_light_quad((4, 3, 2), (1, 1, 1), (4, 2, 2), (3, 3, 2), 16),
              lambda: s.add_light_point((-3, 1, 5), (1, 1, 1))]
    for add in (lights if first == "quad" else lights[::-1]):
        add()
    s.add_material((1, 0.9, 0.7), 0.5, (1, 1, 1), 0.5, 30.0827, 0, 1)
    spheres = np.concatenate([rng.uniform(-1, 1, (300, 3)), rng.uniform(0.02, 0.12, (300, 1))], 1).astype(np.float32)
    for x, y, z, r in spheres:
        s.add_sphere((x, y, z), float(r))
    for mn in rng.uniform(-1, 0.8, (12, 3)):
        s.add_box(mn, mn + rng.uniform(0.05, 0.3, 3))
    s.add_plane_nd((0.0, 0.0, 1.0), 1.0)
    s.add_triangles(bench.synthetic_triangles(720, 5)[:720])
    s.build()
    return s, spheres


def make_rays(family, scene, spheres, n=4096):
    """n shadow rays (origin, L): the range is |L|; about half the ranges are set just short of / just
    past the ray's first hit."""
    rng = np.random.default_rng(FAMILIES.index(family) + 1)
    g = scene.grid_export()
    lo, hi, dims = g["bmin"].astype(np.float64), g["bmax"].astype(np.float64), np.array(g["dims"])
    o = rng.uniform(-1, 1, (n, 3))
    u = rng.normal(size=(n, 3))
    if family == "axis":
        u[np.arange(n), rng.integers(0, 3, n)] = 0.0
        u[: n // 2, 0] = 0.0
    elif family == "faces":  # origins on a cell face of axis a; half the rays lie in that face's plane
        # (an inner face for those: in the grid's own boundary plane Init_Traverse's 0 * inf makes the start
        # cell (int)NaN, grid.cpp:170-190 — undefined in the reference)
        a = rng.integers(0, 3, n)
        k = np.where(np.arange(n) < n // 2, rng.integers(1, dims[a]), rng.integers(0, dims[a] + 1))
        o[np.arange(n), a] = (lo[a] + k * ((hi[a] - lo[a]) / dims[a])).astype(np.float32)
        u[np.arange(n // 2), a[: n // 2]] = 0.0
    elif family == "outside":
        o = rng.normal(size=(n, 3))
        o *= rng.uniform(2.5, 6.0, (n, 1)) / np.linalg.norm(o, axis=1, keepdims=True)
        u = rng.uniform(-1.6, 1.6, (n, 3)) - o
    elif family == "plane":  # shallow, downwards: the plane is hit far outside the grid
        o[:, 2] = rng.uniform(-0.9, 1.0, n)
        u[:, 2] = -rng.uniform(0.02, 0.2, n) * np.linalg.norm(u[:, :2], axis=1)
    elif family == "grazing":  # tangent to a sphere within 1e-5 of its radius, inside and outside
        sp = spheres[rng.integers(0, len(spheres), n)].astype(np.float64)
        w = np.cross(u, rng.normal(size=(n, 3)))
        w *= (sp[:, 3:] * (1 + rng.uniform(-1e-5, 1e-5, (n, 1)))) / np.linalg.norm(w, axis=1, keepdims=True)
        o = sp[:, :3] + w - u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.2, 1.0, (n, 1))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    length = np.exp(rng.uniform(np.log(0.05), np.log(60.0 if family == "plane" else 8.0), n))
    t, _, _ = scene.trace_cpu(np.concatenate([o, u], 1).astype(np.float32))
    near = (t < 1e30) & (rng.random(n) < 0.5)
    length[near] = t[near] * rng.choice([0.7, 1.3], near.sum())
    return np.concatenate([o, u * length[:, None]], 1).astype(np.float32)


@pytest.fixture(scope="module")
def batched(drt, renderer):
    s, spheres = mixed_scene(drt)
    return s, spheres


@pytest.mark.parametrize("family", FAMILIES)
def test_cell_tree_batched_shadow_equals_grid_walk(renderer, batched, family):
    s, spheres = batched
    renderer.upload(s)
    rays = make_rays(family, s, spheres)
    ref = s.trace_cpu(rays, shadow=True)
    assert 0 < ref.sum() < len(ref)
    renderer.set_trace_stats(True, grid_tree=True)
    tree = renderer.trace_shadow(rays)
    st = renderer.trace_stats()
    renderer.set_trace_stats(False)
    walk = renderer.trace_shadow(rays)
    print(family, {k: st[k] for k in st if k.startswith("wide_") or k == "shadow_rays"}, int(ref.sum()))
    np.testing.assert_array_equal(walk, ref)
    np.testing.assert_array_equal(tree, ref)
    assert st["shadow_rays"] == len(rays) and st["wide_shadow_rays"] > 0
    if family == "uniform":
        assert st["wide_grid_walks"] <= 0.05 * st["shadow_rays"], (st["wide_grid_walks"], st["shadow_rays"])


FRAMES = [
    # (spp, first light, max_depth, roughness)
    (16, "quad", 4, 0.0),  # AA
    (0, "quad", 3, 0.0),   # Whitted with a quad light
    (9, "quad", 3, 0.2),   # in-order glossy
    (16, "point", 8, 0.0),  # deep mirror chains
]


@pytest.mark.parametrize("spp,first,md,rough", FRAMES)
def test_cell_tree_frame_equals_grid_walk(drt, renderer, monkeypatch, spp, first, md, rough):
    s, _ = mixed_scene(drt, spp=spp, first=first)
    renderer.upload(s)
    kw = {"max_depth": md, "roughness": rough}
    plan = renderer.plan(renderer.frame_params(seed=6, **kw))
    assert plan["passes"] == 2 and plan["wavefront"]
    tree = renderer.render(seed=6, **kw)
    monkeypatch.setenv("DRT_GRID_SHADOW_TREE", "0")
    walk = renderer.render(seed=6, stats=True, **kw)
    wst = renderer.stats()
    np.testing.assert_array_equal(bits(tree), bits(walk))
    monkeypatch.setenv("DRT_GRID_SHADOW_TREE", "2")
    tst_img = renderer.render(seed=6, stats=True, **kw)
    tst = renderer.stats()
    np.testing.assert_array_equal(bits(tst_img), bits(walk))
    assert tst["samples"] == wst["samples"] and tst["shadow_rays"] == wst["shadow_rays"] > 0
    assert tst["wide_shadow_rays"] > 0 and wst["wide_shadow_rays"] == 0


def test_cell_tree_triangle_scene_equals_grid_walk(drt, renderer, monkeypatch):
    """DRT_GRID_CELL_TREE=2: a triangle scene's queries on the cell tree in place of the widened tree."""
    from tests.test_gpu_grid_tree import grid_scene

    monkeypatch.setenv("DRT_GRID_CELL_TREE", "2")  # read by the upload and by the frame
    renderer.upload(grid_scene(drt, "quad", 20_000))
    tree = renderer.render(seed=6)
    renderer.set_trace_stats(True, grid_tree=True)
    renderer.trace_shadow(np.array([[0, 0, 0.5, 1, 1, 1]], np.float32))
    assert renderer.trace_stats()["wide_shadow_rays"] == 1  # the scene has a cell tree
    renderer.set_trace_stats(False)
    monkeypatch.setenv("DRT_GRID_SHADOW_TREE", "0")
    np.testing.assert_array_equal(bits(tree), bits(renderer.render(seed=6)))
