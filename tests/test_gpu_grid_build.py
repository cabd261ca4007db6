"""The device grid builder and commit (drt_build_grid_device, csrc/hip/drt_grid_build.hip) through
Renderer.upload(scene, build="device", commit=...) on Grid scenes: the lists against Grid::Build's bit for bit,
the device walk against the host walk, frames and work counts against the host path's.

Scene sizes are the smallest at which a stage can go wrong: 1, 2, 65 (one over a wave), one more than the
reference-slot tile, 20 000 (more cells than the macro-cell bitmap holds, a partial last tile everywhere); one
axis of a single cell; long runs of empty cells; mixed primitives on the 48-B records; two triangles that span
the whole box, so one object's references cover many workgroups and cells hold odd counts; 70 000 triangles,
whose grid has more than 256 scan tiles of cells, so the one-workgroup scan of the tile sums
(block_scan_array, csrc/hip/drt_scan_sort.hpp, which every builder's chunked scan runs) takes a second
256-wide round with a carry.
"""
import numpy as np
import pytest

from tests.test_gpu_bvh_build import bits, make_rays, make_scene, triangles  # noqa: F401

pytestmark = pytest.mark.gpu

T = 2048  # reference slots per workgroup (kGridTile)
SIZES = {"soup1": 1, "soup2": 2, "soup65": 65, "soupT1": T + 1, "soup20k": 20000}
BIG = "soup70k"  # more than T * 256 cells
CASES = list(SIZES) + ["flat", "clusters", "mixed", "floor", BIG]
FRAMES = ["soup20k", "mixed", "floor"]


def grid_scene(drt, name):
    if name not in ("floor", BIG):
        return make_scene(drt, name, accel="grid")
    import bench

    n = 70000 if name == BIG else 2000
    tris = bench.synthetic_triangles(n, 3)[:n]
    v = tris.reshape(-1, 3, 3)
    lo, hi = v.min((0, 1)).astype(np.float64), v.max((0, 1)).astype(np.float64)
    floor = np.array([[lo[0], lo[1], lo[2], hi[0], lo[1], lo[2], hi[0], hi[1], hi[2]],
                      [lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], lo[0], hi[1], hi[2]]], np.float32)
    s = drt.Scene()
    s.set_background((0.078, 0.361, 0.753))
    s.set_accel("grid")
    s.set_spp(16)
    s.add_light_quad((4, 3, 2), (1, 1, 1), (4, 2, 2), (3, 3, 2), 16)
    s.add_material((1, 0.9, 0.7), 0.5, (1, 1, 1), 0.5, 30.0827, 0, 1)
    s.add_triangles(np.concatenate([tris, floor]) if name == "floor" else tris)
    eye = (lo + hi) / 2 + (hi - lo + 1.0) * (1.1, 0.9, 0.7)
    s.set_camera(eye, (lo + hi) / 2, (0, 0, 1), 45.0, 0.01, 64, 48, 0.0, 1.0)
    return s, None, eye, lo, hi


def rays_of(name, eye, lo, hi):
    import tests.test_gpu_bvh_build as B

    return make_rays(name if name in B.CASES else "soup3", eye, lo, hi)


def same_grid(a, b):
    assert a["dims"] == b["dims"]
    for k in ("bmin", "bmax"):
        assert (bits(a[k]) == bits(b[k])).all(), k
    for k in ("cell_start", "cell_objs"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def drt():
    import distributionraytracer_amd as d

    return d


@pytest.fixture(scope="module")
def renderer(drt):
    r = drt.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def host(drt):
    """name -> the host-built twin and its export, built once"""
    cache = {}

    def get(name):
        if name not in cache:
            s = grid_scene(drt, name)[0]
            s.build()
            cache[name] = (s, s.grid_export())
        return cache[name]

    return get


@pytest.mark.parametrize("commit", ["host", "device"])
@pytest.mark.parametrize("name", CASES)
def test_lists_and_walks_equal_the_host_grid(name, commit, drt, renderer, host):
    scene, _, eye, lo, hi = grid_scene(drt, name)
    renderer.upload(scene, build="device", commit=commit)
    got, info = scene.grid_export(), renderer.grid_build_info()
    shift = 0
    while np.prod([(d + (1 << shift) - 1) >> shift for d in got["dims"]]) > 131072:
        shift += 1
    print(name, commit, "dims", got["dims"], "n_refs", len(got["cell_objs"]), "macro shift", shift)
    same_grid(got, host(name)[1])
    assert name != BIG or info["n_cells"] > T * 256  # or the case no longer reaches the scan's second round
    assert info["dims"] == got["dims"] and info["n_refs"] == len(got["cell_objs"])
    assert info["n_cells"] == len(got["cell_start"]) - 1 and info["on_device"] == (commit == "device")
    assert (bits(info["bmin"]) == bits(got["bmin"])).all() and (bits(info["bmax"]) == bits(got["bmax"])).all()
    rays = rays_of(name, eye, lo, hi)
    t, nrm, obj = renderer.trace_closest(rays)
    ht, hn, ho = scene.trace_cpu(rays)
    assert (bits(t) == bits(ht)).all() and (bits(nrm) == bits(hn)).all() and (obj == ho).all()
    length = np.random.default_rng(5).uniform(0.05, 4.0, (len(rays), 1)).astype(np.float32)
    sh = np.concatenate([rays[:, :3], rays[:, 3:] * length], 1)
    assert (renderer.trace_shadow(sh) == scene.trace_cpu(sh, shadow=True)).all()


@pytest.fixture(scope="module")
def host_frames(drt, renderer):
    """name -> (frame with the shadow tree, frame and stats without it), rendered once"""
    cache = {}

    def get(name, monkeypatch):
        if name not in cache:
            s = grid_scene(drt, name)[0]
            renderer.upload(s)
            tree = renderer.render(seed=7, stats=True)
            monkeypatch.setenv("DRT_GRID_SHADOW_TREE", "0")
            s = grid_scene(drt, name)[0]
            s.build()
            monkeypatch.delenv("DRT_GRID_SHADOW_TREE")
            renderer.upload(s)
            cache[name] = (tree, renderer.render(seed=7, stats=True), renderer.stats())
        return cache[name]

    return get


@pytest.mark.parametrize("commit,install", [("host", True), ("device", True), ("device", False)])
@pytest.mark.parametrize("name", FRAMES)
def test_frames_and_counts_equal_the_host_path(name, commit, install, drt, renderer, host_frames, monkeypatch):
    tree, walk, stats = host_frames(name, monkeypatch)
    scene = grid_scene(drt, name)[0]
    unbuilt = scene.grid_export()
    renderer.upload(scene, build="device", commit=commit, install=install)
    frame = renderer.render(seed=7, stats=True)
    got = renderer.stats()
    assert frame.tobytes() == tree.tobytes() and frame.tobytes() == walk.tobytes()
    # every counter but the readings of a clock and the per-wave loop counts: a wave of the persistent kernel
    # refills its lanes from a work counter all waves share, so how often it loops varies from run to run on
    # the same buffers; the per-lane and per-ray counts do not
    timing = [k for k in got if k.endswith("_ms") or k.startswith("cycles_") or k.startswith("wave_")]
    diff = {k: (got[k], stats[k]) for k in got if k not in timing and got[k] != stats[k]}
    print(name, commit, install, "counters differing:", diff)
    assert not diff
    if not install:
        same_grid(scene.grid_export(), unbuilt)


def test_build_is_deterministic(drt, renderer):
    grids = []
    for _ in range(2):
        scene = grid_scene(drt, "soup20k")[0]
        renderer.upload(scene, build="device", commit="device")
        grids.append(scene.grid_export())
    same_grid(*grids)


def test_group_upload_builds_on_the_first_device(drt, host):
    g = drt.RendererGroup([0])
    scene = grid_scene(drt, "floor")[0]
    g.upload(scene, build="device")
    frame = g.render(seed=7)
    same_grid(scene.grid_export(), host("floor")[1])
    twin = grid_scene(drt, "floor")[0]
    g.upload(twin)
    assert frame.tobytes() == g.render(seed=7).tobytes()
    g.close()
