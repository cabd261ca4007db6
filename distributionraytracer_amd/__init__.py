"""MI355X-native distribution ray tracer (drop-in for rita-mota/DistributionRayTracer's hot path).

Python host layer over libdrt.so:

  Scene     — P3F scenes (Scene::load_p3f, scene.cpp:474) or programmatic scenes; the host
              BVH / Grid build (bvh.cpp:27-227, grid.cpp:30-97) runs in C++.
  Renderer  — one HIP context on one gfx950 device: upload, render (renderScene,
              main.cpp:525-738), batched BVH/Grid Traverse queries, tile-sharded frames.

Everything that touches a ray runs in hand-written HIP kernels; there is no CPU render path.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import _lib
from ._lib import ACCEL, FRAME_REFERENCE_ORDER, FRAME_STATS, TRACE_GRID_TREE, DrtCamera, DrtFrameParams, DrtFrameStats, DrtOptions, DrtSceneInfo, check

__all__ = ["Scene", "Renderer", "RendererGroup", "ACCEL", "load_skybox_dir", "SKY_FACES", "build"]

SKY_FACES = ("right", "left", "top", "bottom", "front", "back")  # scene.cpp:333, CubeMap enum


def build(force=False):
    return _lib.build(force=force)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _fp(a):
    return a.ctypes.data_as(_lib._f)


def image_rgb8(frame):
    """u8fromfloat of a (RES_Y, RES_X, 3) float frame, row 0 = bottom (main.cpp:716-718)."""
    f = np.ascontiguousarray(frame, np.float32)
    out = np.empty(f.shape, np.uint8)
    check(_lib.load().drt_image_rgb8(f.ctypes.data, f.shape[1], f.shape[0], out.ctypes.data), what="drt_image_rgb8")
    return out


def write_png(path, frame):
    """saveImgFile (main.cpp:251-266): 8-bit RGB PNG, displayed upright (top row = frame row RES_Y-1)."""
    f = np.ascontiguousarray(frame, np.float32)
    check(_lib.load().drt_image_write_png(str(path).encode(), f.ctypes.data, f.shape[1], f.shape[0]),
          what="drt_image_write_png")


def load_skybox_dir(path, max_size=None):
    """Decode the six cube faces (DevIL in the reference, scene.cpp:329-378) with PIL, rows
    bottom-up (IL_ORIGIN_LOWER_LEFT)."""
    from PIL import Image

    faces = []
    for name in SKY_FACES:
        im = Image.open(os.path.join(path, name + ".jpg")).convert("RGB")
        if max_size is not None and im.width > max_size:
            im = im.resize((max_size, max_size), Image.NEAREST)
        faces.append(np.asarray(im, dtype=np.uint8)[::-1].copy())
    return faces


class Scene:
    """Host scene (drt_scene*): the reference's Scene + its accelerator."""

    def __init__(self, handle=None):
        L = _lib.load()
        self.h = C.c_void_p(handle if handle is not None else L.drt_scene_new())
        if not self.h:
            raise RuntimeError("scene creation failed")

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _lib.load().drt_scene_free(self.h)
                self.h = None
        except Exception:
            pass

    @classmethod
    def load_p3f(cls, path, skybox_root=None, skybox_faces=None, skybox_max_size=None):
        L = _lib.load()
        h = L.drt_scene_load_p3f(str(path).encode())
        if not h:
            raise FileNotFoundError(path)
        s = cls(h)
        env = s.env
        if env:
            if skybox_faces is None and s.info().skybox_loaded:
                return s  # Scene::load_p3f's LoadSkybox found the faces (PPM / registered decoder)
            if skybox_faces is None:
                root = Path(skybox_root) if skybox_root else Path(path).resolve().parent.parent
                skybox_faces = load_skybox_dir(root / env, skybox_max_size)
            s.set_skybox(skybox_faces)
        return s

    @property
    def env(self):
        return _lib.load().drt_scene_env(self.h).decode()

    def set_skybox(self, faces):
        for i, a in enumerate(faces):
            a = np.ascontiguousarray(a, dtype=np.uint8)
            h, w, bpp = a.shape
            check(_lib.load().drt_scene_set_skybox_face(self.h, i, w, h, bpp, a.ctypes.data_as(_lib._u8)),
                  what="set_skybox")

    def info(self):
        i = DrtSceneInfo()
        check(_lib.load().drt_scene_info(self.h, C.byref(i)), what="scene_info")
        return i

    def set_camera(self, eye, at, up, fovy, hither, res_x, res_y, aperture=0.0, focal=1.0):
        check(_lib.load().drt_scene_set_camera(self.h, _fp(_f32(eye)), _fp(_f32(at)), _fp(_f32(up)), fovy, hither,
                                               res_x, res_y, aperture, focal), what="set_camera")

    def set_eye(self, eye):
        """Camera::SetEye (camera.h:63-72): the interactive camera motion of main.cpp:530-533."""
        check(_lib.load().drt_scene_set_eye(self.h, _fp(_f32(eye))), what="set_eye")

    def set_background(self, rgb):
        _lib.load().drt_scene_set_background(self.h, _fp(_f32(rgb)))

    def set_accel(self, accel):
        check(_lib.load().drt_scene_set_accel(self.h, ACCEL[accel] if isinstance(accel, str) else int(accel)),
              what="set_accel")

    def set_spp(self, spp):
        _lib.load().drt_scene_set_spp(self.h, int(spp))

    def add_material(self, diff, kd, spec, ks, shine, t, ior):
        return _lib.load().drt_scene_add_material(self.h, _fp(_f32(diff)), kd, _fp(_f32(spec)), ks, shine, t, ior)

    def add_sphere(self, c, r):
        return _lib.load().drt_scene_add_sphere(self.h, _fp(_f32(c)), r)

    def add_triangles(self, verts):
        v = _f32(verts).reshape(-1, 9)
        return _lib.load().drt_scene_add_triangles(self.h, _fp(v), len(v))

    def add_plane_pts(self, a, b, c):
        return _lib.load().drt_scene_add_plane_pts(self.h, _fp(_f32(a)), _fp(_f32(b)), _fp(_f32(c)))

    def add_plane_nd(self, n, d):
        return _lib.load().drt_scene_add_plane_nd(self.h, _fp(_f32(n)), d)

    def add_box(self, mn, mx):
        return _lib.load().drt_scene_add_box(self.h, _fp(_f32(mn)), _fp(_f32(mx)))

    def add_light_point(self, pos, rgb=(1, 1, 1)):
        return _lib.load().drt_scene_add_light_point(self.h, _fp(_f32(pos)), _fp(_f32(rgb)))

    def add_light_quad(self, pos, rgb, v1, v2, grid_res):
        return _lib.load().drt_scene_add_light_quad(self.h, _fp(_f32(pos)), _fp(_f32(rgb)), _fp(_f32(v1)),
                                                    _fp(_f32(v2)), grid_res)

    def build(self):
        check(_lib.load().drt_scene_build(self.h), what="scene_build")

    def camera_frame(self):
        c = DrtCamera()
        check(_lib.load().drt_scene_camera_frame(self.h, C.byref(c)), what="camera_frame")
        return c

    def bvh_export(self):
        n = self.info().bvh_nodes
        no = self.info().n_objects
        boxes = np.zeros((n, 6), np.float32)
        leaf = np.zeros(n, np.uint32)
        index = np.zeros(n, np.uint32)
        nobj = np.zeros(n, np.uint32)
        order = np.zeros(no, np.int32)
        check(_lib.load().drt_scene_bvh_export(self.h, _fp(boxes), leaf.ctypes.data_as(_lib._u32),
                                               index.ctypes.data_as(_lib._u32), nobj.ctypes.data_as(_lib._u32),
                                               order.ctypes.data_as(_lib._i32)), what="bvh_export")
        return dict(boxes=boxes, leaf=leaf, index=index, nobjs=nobj, order=order)

    def set_bvh(self, boxes, leaf, index, nobjs, order):
        """drt_scene_set_bvh, the inverse of bvh_export: install a tree (e.g. a device-built one) as the
        scene's BVH; trace_cpu, bvh_export and info() then use it.  Refused (DRT_E_INVALID) unless it is
        a well-formed tree over every object with nested boxes."""
        b = _f32(boxes).reshape(-1, 6)
        nodes = np.zeros(len(b), np.dtype([("box", np.float32, 6), ("leaf", np.uint32), ("index", np.uint32),
                                           ("n_objs", np.uint32)]))
        nodes["box"], nodes["leaf"], nodes["index"], nodes["n_objs"] = b, leaf, index, nobjs
        o = np.ascontiguousarray(order, np.uint32)
        check(_lib.load().drt_scene_set_bvh(self.h, nodes.ctypes.data, len(nodes), o.ctypes.data_as(_lib._u32),
                                            len(o)), what="drt_scene_set_bvh")

    def set_grid(self, dims, bmin, bmax, cell_start, cell_objs):
        """drt_scene_set_grid, the inverse of grid_export: install cell lists (e.g. a device-built grid's) as
        the scene's grid; trace_cpu, grid_export and upload then use them.  Refused (DRT_E_INVALID) unless
        the starts are monotone over nx*ny*nz + 1 entries and every index is an object of the scene."""
        d = np.ascontiguousarray(dims, np.int32)
        cs = np.ascontiguousarray(cell_start, np.int64)
        co = np.ascontiguousarray(cell_objs, np.int32)
        check(_lib.load().drt_scene_set_grid(self.h, d.ctypes.data_as(_lib._i32), _fp(_f32(bmin)), _fp(_f32(bmax)),
                                             cs.ctypes.data_as(_lib._i64), len(cs), co.ctypes.data_as(_lib._i32),
                                             len(co)), what="drt_scene_set_grid")

    def trace_cpu(self, rays, shadow=False):
        """The scalar host path (BVH::Traverse / Grid::Traverse / the NONE scan on the CPU, one ray
        at a time): closest -> (t, normal, object); shadow -> occluded (uint8)."""
        r = _f32(rays).reshape(-1, 6)
        n = len(r)
        L = _lib.load()
        if shadow:
            occ = np.zeros(n, np.uint8)
            check(L.drt_scene_trace_cpu(self.h, 1, _fp(r), n, None, None, None, occ.ctypes.data_as(_lib._u8)),
                  what="trace_cpu")
            return occ
        t = np.zeros(n, np.float32)
        nrm = np.zeros((n, 3), np.float32)
        obj = np.zeros(n, np.int32)
        check(L.drt_scene_trace_cpu(self.h, 0, _fp(r), n, _fp(t), _fp(nrm), obj.ctypes.data_as(_lib._i32), None),
              what="trace_cpu")
        return t, nrm, obj

    def skybox_color_cpu(self, dirs):
        """Scene::GetSkyboxColor for n directions (n x 3 floats)."""
        d = _f32(dirs).reshape(-1, 3)
        out = np.zeros((len(d), 3), np.float32)
        check(_lib.load().drt_scene_skybox_color_cpu(self.h, _fp(d), len(d), _fp(out)), what="skybox_color_cpu")
        return out

    def load_skybox(self, sky_dir):
        """Scene::LoadSkybox: <dir>/<face>.ppm (or .jpg through a registered decoder)."""
        check(_lib.load().drt_scene_load_skybox(self.h, str(sky_dir).encode()), what="load_skybox")

    def grid_export(self):
        L = _lib.load()
        dims = np.zeros(3, np.int32)
        bmin = np.zeros(3, np.float32)
        bmax = np.zeros(3, np.float32)
        nref = C.c_int64()
        check(L.drt_scene_grid_export_dims(self.h, dims.ctypes.data_as(_lib._i32), _fp(bmin), _fp(bmax),
                                           C.byref(nref)), what="grid_export")
        cs = np.zeros(int(np.prod(dims)) + 1, np.int64)
        co = np.zeros(nref.value, np.int32)
        check(L.drt_scene_grid_export(self.h, cs.ctypes.data_as(_lib._i64), co.ctypes.data_as(_lib._i32)),
              what="grid_export")
        return dict(dims=tuple(int(d) for d in dims), bmin=bmin, bmax=bmax, cell_start=cs, cell_objs=co)


class Renderer:
    """One HIP context (drt_ctx*) on one gfx950 device."""

    def __init__(self, device=0):
        L = _lib.load()
        opt = DrtOptions()
        opt.device = int(device)
        h = C.c_void_p()
        rc = L.drt_create(C.byref(h), C.byref(opt))
        if rc != 0:
            raise RuntimeError(f"drt_create(device={device}) failed: {_lib.STATUS.get(rc, rc)} "
                               "(a gfx950 / MI355X device is required; there is no CPU path)")
        self.h = h
        self.scene = None

    def close(self):
        if getattr(self, "h", None):
            _lib.load().drt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, scene: Scene, build="host", commit="host", install=True, shadow_tree=None):
        """build="host": the reference's binned-SAH tree, built on the CPU (drt_scene_build) if the scene
        is not built yet.  build="device" (BVH scenes): a linear BVH built by HIP kernels from the
        primitives on the device (drt_build_bvh_device) and installed in `scene` too — far quicker to
        build, slower to trace (README.md, Use).  With build="device", commit="device" also lays out the
        records and the shadow tree by HIP kernels (drt_build_bvh_device_commit; the same answers and
        traversal counts), and install=False leaves `scene` without the tree: nothing but status words
        comes back from the device, and scene.trace_cpu / scene.bvh_export behave as on an unbuilt scene.
        A Grid scene with build="device" gets its grid from HIP kernels too (drt_build_grid_device): exactly
        the host's cell lists, bit for bit, committed by drt_upload_grid (commit="host") or by kernels
        (commit="device").  shadow_tree="device" or "ploc" (Grid scenes with build="device" only) also builds
        its shadow tree on the device: the LBVH or the PLOC builder's tree of the primitives, committed by
        HIP kernels (csrc/hip/drt_grid_tree_commit.hip) with the cell ranges the grid build left there, and
        with install=True stored in `scene`, so that a later upload(scene) commits the same tree on the host.
        grid_build_info()["shadow_tree"] says which tree is resident (0: none — a scene with other
        primitives than triangles, DRT_GRID_SHADOW_TREE=0, a tree the commit refused).  With shadow_tree=None
        no tree is built: shadow queries take the Grid walk, which renders the same frame at a lower rate.
        build="ploc" (BVH scenes only): as build="device" with the PLOC builder (drt_build_bvh_device_ex,
        csrc/hip/drt_bvh_ploc.hip) in place of the LBVH: more kernel rounds to build, a tree of lower
        surface-area cost (README.md, Use); commit and install as with build="device".
        build="binned" (BVH scenes only): the binned-SAH builder (csrc/hip/drt_bvh_binned.hip), which builds
        the tree of build="host" itself on the device, node for node, so it renders at the host tree's rate
        and counts; commit and install as with build="device".  A tree with a leaf of 31 objects or more
        (degenerate scenes) is committed by the host even with commit="device": bvh_commit_info() says so."""
        if build not in ("host", "device", "ploc", "binned"):
            raise ValueError(f"build must be 'host', 'device', 'ploc' or 'binned', not {build!r}")
        if commit not in ("host", "device"):
            raise ValueError(f"commit must be 'host' or 'device', not {commit!r}")
        if build == "host" and (commit == "device" or not install):
            raise ValueError("commit='device' and install=False need build='device', 'ploc' or 'binned'")
        if shadow_tree not in (None, "device", "ploc"):
            raise ValueError(f"shadow_tree must be None, 'device' or 'ploc', not {shadow_tree!r}")
        if build in ("ploc", "binned") and scene.info().accel == ACCEL["grid"]:
            raise ValueError(f"build={build!r} is a BVH builder: a Grid scene has one device builder, build='device'")
        if shadow_tree is not None and (build == "host" or scene.info().accel != ACCEL["grid"]):
            raise ValueError("shadow_tree needs a Grid scene and build='device'")
        if build == "host":
            check(_lib.load().drt_scene_upload(self.h, scene.h), self.h, "drt_scene_upload")
        elif scene.info().accel == ACCEL["grid"]:
            flags = ((_lib.GRID_COMMIT_DEVICE if commit == "device" else 0) | (0 if install else _lib.GRID_NO_INSTALL) |
                     {None: 0, "device": _lib.GRID_SHADOW_LBVH, "ploc": _lib.GRID_SHADOW_PLOC}[shadow_tree])
            check(_lib.load().drt_scene_upload_device_grid(self.h, scene.h, flags), self.h,
                  "drt_scene_upload_device_grid")
        elif build == "device" and commit == "host" and install:
            check(_lib.load().drt_scene_upload_device_bvh(self.h, scene.h), self.h, "drt_scene_upload_device_bvh")
        else:
            flags = ((_lib.BVH_COMMIT_DEVICE if commit == "device" else 0) | (0 if install else _lib.BVH_NO_INSTALL) |
                     {"device": 0, "ploc": _lib.BVH_BUILDER_PLOC_FLAG, "binned": _lib.BVH_BUILDER_BINNED_FLAG}[build])
            check(_lib.load().drt_scene_upload_device_bvh_ex(self.h, scene.h, flags), self.h,
                  "drt_scene_upload_device_bvh_ex")
        self.scene = scene
        return self

    def bvh_commit_info(self):
        """drt_bvh_commit_info of the resident BVH: on_device (1 after commit="device"), has_wide, n_slots
        (64-B inner record slots, padding included), n_wide (4-ary shadow-tree records)."""
        i = _lib.DrtBvhCommitInfo()
        check(_lib.load().drt_get_bvh_commit_info(self.h, C.byref(i)), self.h, "drt_get_bvh_commit_info")
        return {n: int(getattr(i, n)) for n, _ in i._fields_}

    def grid_build_info(self):
        """drt_grid_build_info of the last build="device" upload of a Grid scene: dims, box, cells,
        references, the build / fetch / commit times in ms, whether the device committed, and the shadow tree
        built with it (0 none, 1 LBVH, 2 PLOC; its figures: bvh_build_info())."""
        i = _lib.DrtGridBuildInfo()
        check(_lib.load().drt_get_grid_build_info(self.h, C.byref(i)), self.h, "drt_get_grid_build_info")
        out = {n: getattr(i, n) for n, _ in i._fields_}
        return {k: (tuple(v) if k in ("dims", "bmin", "bmax") else (float(v) if k.endswith("_ms") else int(v)))
                for k, v in out.items()}

    def bvh_build_info(self):
        """drt_bvh_build_info of the last build="device", "ploc" or "binned" upload: nodes, leaves, depth, the
        build / fetch / commit times in ms, the builder (0 LBVH, 1 PLOC, 2 binned SAH), PLOC's search and forced
        round counts, and in `rounds` the binned builder's level-wise rounds."""
        i = _lib.DrtBvhBuildInfo()
        check(_lib.load().drt_get_bvh_build_info(self.h, C.byref(i)), self.h, "drt_get_bvh_build_info")
        return {n: (float(getattr(i, n)) if n.endswith("_ms") else int(getattr(i, n))) for n, _ in i._fields_}

    def set_camera(self, camera=None):
        """drt_set_camera: the uploaded scene's camera alone (the per-frame SetEye of the interactive
        renderer, main.cpp:530-533); `camera` is a Scene (its current camera) or a DrtCamera frame,
        default the uploaded Scene.  Primitives and the accelerator stay resident."""
        cam = self.scene if camera is None else camera
        if isinstance(cam, Scene):
            check(_lib.load().drt_scene_upload_camera(self.h, cam.h), self.h, "drt_scene_upload_camera")
        else:
            check(_lib.load().drt_set_camera(self.h, C.byref(cam)), self.h, "drt_set_camera")
        return self

    def frame_params(self, seed=1, max_depth=4, roughness=0.0, shard=0, n_shards=1, tile=16, stats=False,
                     light_spp=1, progressive_frame=0, slot=0, reference_order=False):
        p = DrtFrameParams()
        p.slot = slot
        p.light_spp = light_spp
        p.progressive_frame = progressive_frame
        p.seed = seed
        p.max_depth = max_depth
        p.roughness = roughness
        p.shard = shard
        p.n_shards = n_shards
        p.tile = tile
        p.flags = (FRAME_STATS if stats else 0) | (FRAME_REFERENCE_ORDER if reference_order else 0)
        return p

    def render(self, seed=1, max_depth=4, roughness=0.0, stats=False, tile=16, light_spp=1, progressive_frame=0,
               accum=None, reference_order=False):
        """Whole frame to host memory.  progressive_frame n >= 1: zone A frame n lerped into
        `accum` (updated in place and returned).  reference_order: shadow queries walk the
        reference's binary tree in its visit order (DRT_FRAME_REFERENCE_ORDER), so stats() counts
        the reference's shadow work; the frame is the same either way."""
        info = self.scene.info()
        if accum is not None:
            if accum.dtype != np.float32 or accum.shape != (info.res_y, info.res_x, 3) or not accum.flags.c_contiguous:
                raise ValueError("accum must be a C-contiguous float32 (res_y, res_x, 3) array")
            out = accum
        else:
            out = np.zeros((info.res_y, info.res_x, 3), np.float32)
        p = self.frame_params(seed, max_depth, roughness, tile=tile, stats=stats, light_spp=light_spp,
                              progressive_frame=progressive_frame, reference_order=reference_order)
        check(_lib.load().drt_render(self.h, C.byref(p), _fp(out)), self.h, "drt_render")
        return out

    def plan(self, params):
        """drt_plan_frame: work items, sample slots, mode and kernel choice of a frame (no device work)."""
        out = _lib.DrtFramePlan()
        check(_lib.load().drt_plan_frame(self.h, C.byref(params), C.byref(out)), self.h, "drt_plan_frame")
        return dict(work_items=int(out.work_items), sample_slots=int(out.sample_slots), mode=int(out.mode),
                    persistent=bool(out.persistent), tiles_in_shard=int(out.tiles_in_shard), passes=int(out.passes), wavefront=bool(out.wavefront))

    def render_device(self, params, d_out_ptr, stream=None):
        """Asynchronous: shard (or whole frame) into a device pointer on `stream` (int handle)."""
        check(_lib.load().drt_render_device(self.h, C.byref(params), C.c_void_p(d_out_ptr),
                                            C.c_void_p(stream or 0)), self.h, "drt_render_device")

    def shard_layout(self, params):
        tiles = C.c_int64()
        floats = C.c_int64()
        check(_lib.load().drt_shard_layout(self.h, C.byref(params), C.byref(tiles), C.byref(floats)), self.h,
              "drt_shard_layout")
        return tiles.value, floats.value

    def unshard_device(self, params, d_shards_ptr, d_frame_ptr, stream=None):
        check(_lib.load().drt_unshard_device(self.h, C.byref(params), C.c_void_p(d_shards_ptr),
                                             C.c_void_p(d_frame_ptr), C.c_void_p(stream or 0)), self.h,
              "drt_unshard_device")

    def stats(self):
        s = DrtFrameStats()
        check(_lib.load().drt_get_stats(self.h, C.byref(s)), self.h, "drt_get_stats")
        return s.as_dict()

    def frame_times(self, max_frames=512):
        """(path-kernel ms, kernel+reduce ms) per recent frame, oldest first (HIP events)."""
        a = (C.c_double * max_frames)()
        b = (C.c_double * max_frames)()
        n = _lib.load().drt_frame_times(self.h, max_frames, a, b)
        if n < 0:
            check(n, self.h, "drt_frame_times")
        return np.array(a[:n]), np.array(b[:n])

    def frame_pass_times(self, max_frames=512):
        """(pass-1 ms, pass-2 ms) per recent frame, oldest first (HIP events): a two-pass frame's
        closest-chain and replay launches; a one-pass frame's kernel and 0."""
        a = (C.c_double * max_frames)()
        b = (C.c_double * max_frames)()
        n = _lib.load().drt_frame_pass_times(self.h, max_frames, a, b)
        if n < 0:
            check(n, self.h, "drt_frame_pass_times")
        return np.array(a[:n]), np.array(b[:n])

    def frame_stage_times(self):
        """{wf_gen, stream, wf_combine} ms of the last wavefront frame's pass-2 launches (drt_frame_stage_times)."""
        out = (C.c_double * 3)()
        n = _lib.load().drt_frame_stage_times(self.h, out)
        if n < 0:
            check(n, self.h, "drt_frame_stage_times")
        return {"wf_gen": out[0], "stream": out[1], "wf_combine": out[2], "chunks": n}

    def wave_times(self, pass_index=0, max_waves=1 << 14):
        """Per resident wave of the last stats frame's persistent launch (pass 0 or 1): (start, end)
        s_memrealtime stamps in us (100 MHz clock), rows of waves that ran; (drt_frame_wave_times)."""
        buf = (C.c_uint64 * (2 * max_waves))()
        n = _lib.load().drt_frame_wave_times(self.h, pass_index, buf, max_waves)
        if n < 0:
            check(n, self.h, "drt_frame_wave_times")
        a = np.frombuffer(buf, dtype=np.uint64, count=2 * n).reshape(n, 2)
        a = a[(a[:, 0] > 0) & (a[:, 1] > 0)]
        return a.astype(np.float64) / 100.0

    def frame_spans(self, max_frames=512):
        """(path start, path end, frame end) of recent frames in ms on one device clock, from the
        oldest frame's path-kernel start (HIP events on each frame's stream)."""
        a, b, e = ((C.c_double * max_frames)() for _ in range(3))
        n = _lib.load().drt_frame_spans(self.h, max_frames, a, b, e)
        if n < 0:
            check(n, self.h, "drt_frame_spans")
        return np.array(a[:n]), np.array(b[:n]), np.array(e[:n])

    def trace_closest(self, rays):
        r = _f32(rays).reshape(-1, 6)
        n = len(r)
        t = np.zeros(n, np.float32)
        nrm = np.zeros((n, 3), np.float32)
        obj = np.zeros(n, np.int32)
        check(_lib.load().drt_trace_closest(self.h, _fp(r), n, _fp(t), _fp(nrm), obj.ctypes.data_as(_lib._i32)),
              self.h, "drt_trace_closest")
        return t, nrm, obj

    def trace_shadow(self, rays):
        r = _f32(rays).reshape(-1, 6)
        occ = np.zeros(len(r), np.uint8)
        check(_lib.load().drt_trace_shadow(self.h, _fp(r), len(r), occ.ctypes.data_as(_lib._u8)), self.h,
              "drt_trace_shadow")
        return occ

    def trace_device(self, shadow, d_rays, n, d_t=0, d_normal=0, d_object=0, d_occluded=0, stream=None):
        """Asynchronous batched queries on device pointers (ints), on `stream` (int handle)."""
        v = C.c_void_p
        check(_lib.load().drt_trace_device(self.h, int(bool(shadow)), v(d_rays), int(n), v(d_t), v(d_normal),
                                           v(d_object), v(d_occluded), v(stream or 0)), self.h, "drt_trace_device")

    def set_trace_stats(self, on=True, reference_order=False, grid_tree=False):
        """Count traversal work (rays, nodes, leaves, primitives) of later batched queries;
        reference_order: later shadow queries walk the reference's binary tree; grid_tree: a Grid
        scene's later shadow queries run on its cell tree (DRT_TRACE_GRID_TREE), the answers unchanged."""
        flags = (FRAME_STATS if on else 0) | (FRAME_REFERENCE_ORDER if reference_order else 0) | (
            TRACE_GRID_TREE if grid_tree else 0)
        check(_lib.load().drt_set_trace_flags(self.h, flags), self.h, "drt_set_trace_flags")

    def trace_stats(self):
        """Streaming-kernel time (kernel_ms) and counters of the last BVH batched query."""
        s = DrtFrameStats()
        check(_lib.load().drt_trace_stats(self.h, C.byref(s)), self.h, "drt_trace_stats")
        return s.as_dict()


class RendererGroup:
    """Several GPUs behind one handle (drt_group_*, include/drt.h): the scene replicated on every
    device, each frame tile-sharded over them, all-gathered over RCCL and reassembled on the first
    device — a single process, no torch.distributed."""

    def __init__(self, devices):
        L = _lib.load()
        devs = list(devices)
        arr = (C.c_int32 * len(devs))(*devs)
        h = C.c_void_p()
        rc = L.drt_group_create(C.byref(h), len(devs), arr)
        if rc != 0:
            raise RuntimeError(f"drt_group_create({devs}) failed: {_lib.STATUS.get(rc, rc)}")
        self.h = h
        self.devices = devs
        self.scene = None

    def close(self):
        if getattr(self, "h", None):
            _lib.load().drt_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {_lib.STATUS.get(rc, rc)} "
                               f"{_lib.load().drt_group_last_error(self.h).decode()}".strip())

    def upload(self, scene: Scene, build="host"):
        """build="device": the tree is built once, on the first device (Renderer.upload), and the same
        arrays are committed on every device.  build="ploc" or "binned": the same with the PLOC or the
        binned-SAH builder (BVH scenes).
        Renderer.upload's shadow_tree (a Grid scene's shadow tree built on the device) is not offered here:
        a group's device-built grid answers shadow queries by the Grid walk."""
        if build not in ("host", "device", "ploc", "binned"):
            raise ValueError(f"build must be 'host', 'device', 'ploc' or 'binned', not {build!r}")
        if build in ("ploc", "binned") and scene.info().accel == ACCEL["grid"]:
            raise ValueError(f"build={build!r} is a BVH builder: a Grid scene has one device builder, build='device'")
        if build in ("ploc", "binned"):
            flag = _lib.BVH_BUILDER_PLOC_FLAG if build == "ploc" else _lib.BVH_BUILDER_BINNED_FLAG
            self._check(_lib.load().drt_group_scene_upload_device_bvh_ex(self.h, scene.h, flag),
                        "drt_group_scene_upload_device_bvh_ex")
        elif build == "device" and scene.info().accel == ACCEL["grid"]:
            self._check(_lib.load().drt_group_scene_upload_device_grid(self.h, scene.h),
                        "drt_group_scene_upload_device_grid")
        elif build == "device":
            self._check(_lib.load().drt_group_scene_upload_device_bvh(self.h, scene.h),
                        "drt_group_scene_upload_device_bvh")
        else:
            self._check(_lib.load().drt_group_scene_upload(self.h, scene.h), "drt_group_scene_upload")
        self.scene = scene
        return self

    def set_camera(self, camera=None):
        """drt_group_set_camera on every device (see Renderer.set_camera)."""
        cam = self.scene if camera is None else camera
        if isinstance(cam, Scene):
            self._check(_lib.load().drt_group_scene_upload_camera(self.h, cam.h), "drt_group_scene_upload_camera")
        else:
            self._check(_lib.load().drt_group_set_camera(self.h, C.byref(cam)), "drt_group_set_camera")
        return self

    def render(self, seed=1, max_depth=4, roughness=0.0, light_spp=1, progressive_frame=0, accum=None, slot=0):
        info = self.scene.info()
        out = accum if accum is not None else np.zeros((info.res_y, info.res_x, 3), np.float32)
        p = DrtFrameParams()
        p.seed, p.max_depth, p.roughness, p.light_spp, p.progressive_frame = seed, max_depth, roughness, light_spp, \
            progressive_frame
        p.slot = slot
        self._check(_lib.load().drt_group_render(self.h, C.byref(p), _fp(out)), "drt_group_render")
        return out

    def render_device(self, d_frame_ptr, seed=1, max_depth=4, roughness=0.0, light_spp=1, stream=None, slot=0):
        p = DrtFrameParams()
        p.seed, p.max_depth, p.roughness, p.light_spp = seed, max_depth, roughness, light_spp
        p.slot = slot
        self._check(_lib.load().drt_group_render_device(self.h, C.byref(p), C.c_void_p(d_frame_ptr),
                                                        C.c_void_p(stream or 0)), "drt_group_render_device")

    def synchronize(self):
        self._check(_lib.load().drt_group_synchronize(self.h), "drt_group_synchronize")
