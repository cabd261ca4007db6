"""The device commit of a device-built tree (drt_build_bvh_device_commit, csrc/hip/drt_bvh_commit.hip) through
Renderer.upload(scene, build="device", commit="device"), against the host commit (drt_upload_bvh) of the same
tree: every answer bit-equal, every traversal count equal — equal 4-ary counts show the same collapse, child
order and quantised planes.  Nothing in the commit is inexact, so there is no tolerance.

Sizes: 1, 2 (a leaf root: no inner record, no 4-ary tree), 3 (a 4-ary node with an unused slot), 4, 5 (the first
collapse that chooses between two inner children), 65 (one over a wave), 257 (one over a workgroup of the
scans), 20 000 (many workgroups and frontier levels, a partial last workgroup); all Morton keys equal (a
tree too deep for the 4-ary stack: both sides must agree); coordinates near 1e3 with extents of 1e-3 (the
exponent search); mixed primitives (the record gather of every type).
"""
import numpy as np
import pytest

from tests.test_gpu_bvh_build import bits, make_rays, make_scene

pytestmark = pytest.mark.gpu

SOUPS = {"soup1": 1, "soup2": 2, "soup3": 3, "soup4": 4, "soup5": 5, "soup65": 65, "soup257": 257, "soup20k": 20000}
CASES = list(SOUPS) + ["same_centroid", "clusters", "mixed"]


def scene_of(drt, name):
    """-> (scene, rays): the recipes of tests/test_gpu_bvh_build.py, with the soup sizes of this file"""
    import bench

    if name not in SOUPS:
        s, _, eye, lo, hi = make_scene(drt, name)
        return s, make_rays(name, eye, lo, hi)
    tris = bench.synthetic_triangles(SOUPS[name], 3)[: SOUPS[name]]
    s = drt.Scene()
    s.set_background((0.078, 0.361, 0.753))
    s.set_accel("bvh")
    s.set_spp(16)
    s.add_light_quad((4, 3, 2), (1, 1, 1), (4, 2, 2), (3, 3, 2), 16)
    s.add_material((1, 0.9, 0.7), 0.5, (1, 1, 1), 0.5, 30.0827, 0, 1)
    s.add_triangles(tris)
    v = tris.reshape(-1, 3, 3).astype(np.float64)
    lo, hi = v.min((0, 1)) - 0.001, v.max((0, 1)) + 0.001
    eye = (lo + hi) / 2 + (hi - lo + 1.0) * (1.1, 0.9, 0.7)
    s.set_camera(eye, (lo + hi) / 2, (0, 0, 1), 45.0, 0.01, 64, 48, 0.0, 1.0)
    return s, make_rays("soup3", eye, lo, hi)


@pytest.fixture(scope="module")
def drt():
    import distributionraytracer_amd as d

    return d


@pytest.fixture(scope="module")
def renderers(drt):
    ra, rb = drt.Renderer(0), drt.Renderer(0)
    yield ra, rb
    ra.close()
    rb.close()


@pytest.fixture(scope="module", params=CASES)
def pair(request, drt, renderers):
    """Scene A built and committed on the device (ra); scene B, the same primitives with A's tree installed,
    through the host commit (rb)."""
    ra, rb = renderers
    a, rays = scene_of(drt, request.param)
    ra.upload(a, build="device", commit="device")
    b = scene_of(drt, request.param)[0]
    b.set_bvh(**a.bvh_export())
    rb.upload(b)
    return dict(name=request.param, a=a, rays=rays)


def counts(stats):
    """Every counter but the times: *_ms, the cycle counters, and the per-wave iteration counters, which count
    a loop once per wave and so depend on which lanes the kernels' dynamic work claims put into one wave —
    scheduling, like the times (measured on soup20k frames of one tree: wave_node_iters 135894 / 135899 with
    every per-lane counter equal)."""
    return {k: v for k, v in stats.items() if not k.endswith("_ms") and not k.startswith(("cycles_", "wave_"))}


def test_answers_and_counts_equal_the_host_commit(pair, renderers):
    ra, rb = renderers
    rays, a = pair["rays"], pair["a"]
    length = np.random.default_rng(5).uniform(0.05, 4.0, (len(rays), 1)).astype(np.float32)
    sh = np.concatenate([rays[:, :3], rays[:, 3:] * length], 1)
    got = []
    for r in (ra, rb):
        r.set_trace_stats(True)
        t, nrm, obj = r.trace_closest(rays)
        out = [bits(t), bits(nrm), obj, counts(r.trace_stats())]
        out += [r.trace_shadow(sh), counts(r.trace_stats())]
        r.set_trace_stats(True, reference_order=True)
        out += [r.trace_shadow(sh), counts(r.trace_stats())]
        r.set_trace_stats(False)
        got.append(out)
    ht, hn, ho = a.trace_cpu(rays)
    hocc = a.trace_cpu(sh, shadow=True)
    for x, y, want in zip(got[0], got[1], [bits(ht), bits(hn), ho, None, hocc, None, hocc, None]):
        if isinstance(x, dict):
            print(pair["name"], "counts differing:", {k: (x[k], y[k]) for k in x if x[k] != y[k]})
            assert x == y
        else:
            print(pair["name"], "differing from the host commit:", int((x != y).sum()), "from the host walk:",
                  int((x != want).sum()), "host commit from the host walk:", int((y != want).sum()))
            assert (x == y).all() and (x == want).all()
    ia, ib, n_inner = ra.bvh_commit_info(), rb.bvh_commit_info(), ra.bvh_build_info()["n_leaves"] - 1
    print(pair["name"], ia, ib)
    assert (ia["on_device"], ib["on_device"]) == (1, 0)
    assert (ia["has_wide"], ia["n_wide"]) == (ib["has_wide"], ib["n_wide"])
    assert n_inner <= ia["n_slots"] <= 2 * n_inner
    if pair["name"] in ("soup1", "soup2"):
        assert (ia["has_wide"], ia["n_slots"]) == (0, 0)


@pytest.mark.parametrize("pair", ["soup20k", "mixed"], indirect=True)
def test_frames_equal_the_host_commit_frames(pair, renderers):
    ra, rb = renderers
    fa, fb = ra.render(seed=7, stats=True), rb.render(seed=7, stats=True)
    assert fa.tobytes() == fb.tobytes()
    assert counts(ra.stats()) == counts(rb.stats())


def test_a_small_tree_after_a_large_one(drt, renderers):
    """Grown buffers keep their tails: the second commit must not read them."""
    ra = renderers[0]
    ra.upload(scene_of(drt, "soup20k")[0], build="device", commit="device")
    s, rays = scene_of(drt, "soup3")
    ra.upload(s, build="device", commit="device")
    t, nrm, obj = ra.trace_closest(rays)
    ht, hn, ho = s.trace_cpu(rays)
    assert (bits(t) == bits(ht)).all() and (bits(nrm) == bits(hn)).all() and (obj == ho).all()
    sh = np.concatenate([rays[:, :3], rays[:, 3:] * np.float32(2.5)], 1)
    assert (ra.trace_shadow(sh) == s.trace_cpu(sh, shadow=True)).all()
    assert ra.bvh_commit_info() == dict(on_device=1, has_wide=1, n_slots=2, n_wide=1)
