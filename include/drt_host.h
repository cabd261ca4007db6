/*
 * drt_host.h — C ABI of the host-side scene library (also in libdrt.so).
 *
 * Flat C entry points over the C++ host API (distributionraytracer_amd/csrc/host/
 * drt_scene.hpp), for callers that cannot use C++ (Python ctypes, other FFIs):
 *
 *   drt_scene_load_p3f     <- Scene::load_p3f            (scene.cpp:474-740)
 *   drt_scene_set_camera   <- Camera::Camera             (camera.h:32-61)
 *   drt_scene_add_*        <- Scene::addObject / addLight and the Sphere/Triangle/Plane/aaBox/
 *                             Light/Material constructors (scene.h:34-180)
 *   drt_scene_build        <- main.cpp:1023-1049: BVH::Build / Grid::Build (bvh.cpp:27-227,
 *                             grid.cpp:30-97), tree-identical to the reference
 *   drt_scene_upload       <- the hand-off renderScene() relied on through globals
 *                             (main.cpp:79-93): scene + accelerator into a drt_ctx
 *   drt_scene_load_skybox  <- Scene::LoadSkybox          (scene.cpp:329-378)
 *   drt_scene_trace_cpu    <- BVH::Traverse / Grid::Traverse on the host (bvh.cpp:231-391,
 *                             grid.cpp:247-358), the scalar path for CPU callers and tests
 *   drt_scene_skybox_color_cpu <- Scene::GetSkyboxColor  (scene.cpp:380-458)
 *
 * C++ callers use the class API of include/drt_scene.hpp directly (same library).
 *
 * Conventions as in drt.h: 0 / negative drt_status, caller-owned host memory.
 */
#ifndef DRT_HOST_H
#define DRT_HOST_H
#include <stdint.h>

#include "drt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct drt_scene drt_scene;

typedef struct {
  int32_t res_x, res_y;
  uint32_t spp;
  int32_t accel;
  int32_t n_objects, n_lights, n_materials;
  int32_t has_env, skybox_loaded;
  float aperture;
  int32_t bvh_nodes;
  double build_ms;
} drt_scene_info_t;

drt_scene* drt_scene_new(void);
drt_scene* drt_scene_load_p3f(const char* path);
void drt_scene_free(drt_scene* s);
int drt_scene_info(const drt_scene* s, drt_scene_info_t* out);
const char* drt_scene_env(const drt_scene* s);
int drt_scene_set_skybox_face(drt_scene* s, int face, int w, int h, int bpp, const uint8_t* bottom_up_rgb);
int drt_scene_set_camera(drt_scene* s, const float eye[3], const float at[3], const float up[3], float fovy,
                         float hither, int res_x, int res_y, float aperture_ratio, float focal_ratio);
int drt_scene_set_background(drt_scene* s, const float rgb[3]);
int drt_scene_set_accel(drt_scene* s, int accel);
int drt_scene_set_spp(drt_scene* s, uint32_t spp);
int drt_scene_add_material(drt_scene* s, const float diff[3], double kd, const float spec[3], double ks,
                           double shine, double t, double ior);
int drt_scene_use_material(drt_scene* s, int mat);
int drt_scene_add_sphere(drt_scene* s, const float c[3], float r);
int drt_scene_add_triangles(drt_scene* s, const float* verts, int64_t n);
int drt_scene_add_plane_pts(drt_scene* s, const float p0[3], const float p1[3], const float p2[3]);
int drt_scene_add_plane_nd(drt_scene* s, const float n[3], float d);
int drt_scene_add_box(drt_scene* s, const float mn[3], const float mx[3]);
int drt_scene_add_light_point(drt_scene* s, const float pos[3], const float rgb[3]);
int drt_scene_add_light_quad(drt_scene* s, const float pos[3], const float rgb[3], const float v1[3],
                             const float v2[3], uint32_t grid_res);

int drt_scene_build(drt_scene* s);
int drt_scene_bvh_export(const drt_scene* s, float* boxes, uint32_t* leaf, uint32_t* index, uint32_t* nobjs,
                         int32_t* object_order);
int drt_scene_grid_export_dims(const drt_scene* s, int32_t dims[3], float bmin[3], float bmax[3], int64_t* n_refs);
int drt_scene_grid_export(const drt_scene* s, int64_t* cell_start, int32_t* cell_objs);
int drt_scene_camera_frame(const drt_scene* s, drt_camera* out);
/* Camera::SetEye (camera.h:63-72): new eye, frame u/v/n and plane distance recomputed; the view
 * window (w, h) and aperture keep their construction values, as in the reference.  DRT_E_STATE
 * without a camera. */
int drt_scene_set_eye(drt_scene* s, const float eye[3]);

int drt_scene_upload(drt_ctx* ctx, drt_scene* s);
/* drt_scene_upload to every device of a group (include/drt.h, drt_group_*). */
int drt_group_scene_upload(drt_group* g, drt_scene* s);
/* Install a caller's tree as a BVH scene's BVH (the inverse of drt_scene_bvh_export): records and object
 * order as drt_upload_bvh takes them.  Validated as there, and further: every node reached exactly once
 * from the root, every object in exactly one leaf, every child box inside its parent's (DRT_E_INVALID
 * otherwise, the scene unchanged; DRT_E_STATE for a scene whose accelerator is not the BVH).  Marks the
 * scene built: drt_scene_trace_cpu, drt_scene_bvh_export, drt_scene_info and drt_scene_upload use it. */
int drt_scene_set_bvh(drt_scene* s, const drt_bvh_node* nodes, uint32_t n_nodes, const uint32_t* object_order,
                      uint32_t n_objects);
/* drt_scene_upload of a BVH scene without the host build: the scene description, then
 * drt_build_bvh_device (include/drt.h), whose tree is installed with drt_scene_set_bvh, so the host
 * scene and the device walk the same tree.  The group form builds once, on rank 0, and commits the same
 * host arrays on every rank with drt_upload_bvh. */
int drt_scene_upload_device_bvh(drt_ctx* ctx, drt_scene* s);
int drt_group_scene_upload_device_bvh(drt_group* g, drt_scene* s);
/* drt_scene_upload_device_bvh with flags (0: the same call).  DRT_BVH_COMMIT_DEVICE commits on the device
 * (drt_build_bvh_device_commit).  DRT_BVH_NO_INSTALL skips the fetch of the tree and drt_scene_set_bvh: the
 * host scene is not marked built by this call, so drt_scene_trace_cpu and drt_scene_bvh_export behave as on
 * an unbuilt scene (they build, or keep, the host's own tree, which is not the one the device walks).  Other
 * DRT_BVH_BUILDER_PLOC_FLAG builds with the PLOC builder (drt_build_bvh_device_ex, DRT_BVH_BUILDER_PLOC) instead
 * of the LBVH, and composes with both; DRT_BVH_BUILDER_BINNED_FLAG likewise with the binned-SAH builder
 * (DRT_BVH_BUILDER_BINNED: the tree drt_scene_build builds, built on the device).  The two builder flags exclude
 * each other.  Other flag bits are DRT_E_INVALID.  The group form keeps the host commit and takes one builder
 * flag alone. */
enum { DRT_BVH_COMMIT_DEVICE = 1, DRT_BVH_NO_INSTALL = 2, DRT_BVH_BUILDER_PLOC_FLAG = 4, DRT_BVH_BUILDER_BINNED_FLAG = 8 };
int drt_scene_upload_device_bvh_ex(drt_ctx* ctx, drt_scene* s, int flags);
int drt_group_scene_upload_device_bvh_ex(drt_group* g, drt_scene* s, int flags);
/* Install a caller's cell lists as a Grid scene's grid (the inverse of drt_scene_grid_export*): dims, box, CSR
 * starts (n_starts = nx*ny*nz + 1) and cell objects (scene indices).  No geometry is computed.  DRT_E_INVALID,
 * the scene unchanged, unless dims > 0, the starts run monotonically from 0 to n_refs, n_starts fits dims and
 * every index is an object of the scene; DRT_E_STATE for a scene whose accelerator is not the Grid.  Marks the
 * scene built, without a BVH for the shadow tree. */
int drt_scene_set_grid(drt_scene* s, const int32_t dims[3], const float bmin[3], const float bmax[3],
                       const int64_t* cell_start, int64_t n_starts, const int32_t* cell_objs, int64_t n_refs);
/* drt_scene_upload of a Grid scene without the host build: the scene description, drt_build_grid_device
 * (include/drt.h) with the scene's cell factor, then drt_fetch_grid_device and drt_scene_set_grid, so the host
 * scene holds the grid the device walks.  DRT_GRID_COMMIT_DEVICE (include/drt.h) commits on the device;
 * DRT_GRID_NO_INSTALL skips the fetch and the install (the host scene is then not marked built by this call).
 * DRT_GRID_SHADOW_LBVH / DRT_GRID_SHADOW_PLOC (include/drt.h) are passed on: the shadow tree is built and
 * committed on the device, and an installing call also stores the binary tree behind it in the host scene, so
 * that a later drt_scene_upload commits the same tree through drt_upload_grid_shadow_bvh.  Without them no
 * shadow tree is uploaded: shadow queries take the Grid walk.  The group form builds once, on rank 0,
 * installs, and uploads to the other ranks by the host path; it takes no shadow bits. */
enum { DRT_GRID_NO_INSTALL = 2 };
int drt_scene_upload_device_grid(drt_ctx* ctx, drt_scene* s, int flags);
int drt_group_scene_upload_device_grid(drt_group* g, drt_scene* s);
/* The scene's current camera frame to a context / every device of a group (drt_set_camera): the
 * per-frame camera of the interactive renderer (main.cpp:530-533) with the scene resident. */
int drt_scene_upload_camera(drt_ctx* ctx, const drt_scene* s);
int drt_group_scene_upload_camera(drt_group* g, const drt_scene* s);

/* ---- skybox faces from files (Scene::LoadSkybox, scene.cpp:329-378) ---- */
/* A decoder for <dir>/<face>.jpg: fills *w, *h, *bpp (3 or 4) and *pixels (malloc'd, rows
 * top-down; the library frees it and flips to the lower-left origin DevIL gives the reference);
 * returns 0 on success.  With none registered (or on failure) LoadSkybox reads binary PPM (P6)
 * <dir>/<face>.ppm.  Process-wide; fn = NULL unregisters. */
typedef int (*drt_image_decoder)(const char* path, int32_t* w, int32_t* h, int32_t* bpp, uint8_t** pixels,
                                 void* user);
int drt_set_image_decoder(drt_image_decoder fn, void* user);
/* Scene::LoadSkybox(dir) + SetSkyBoxFlg(true); DRT_E_INVALID if a face does not decode. */
int drt_scene_load_skybox(drt_scene* s, const char* dir);

/* ---- the scalar host path (include/drt_scene.hpp), one ray at a time on the CPU ---- */
/* BVH::Traverse / Grid::Traverse (bvh.cpp:231-391, grid.cpp:247-358) or the NONE scan
 * (main.cpp:315-326, :430-441) of the built scene for n rays {ox,oy,oz,dx,dy,dz}: closest fills
 * t (FLT_MAX on a miss), normal (n x 3) and object (scene index, -1 on a miss); shadow fills
 * occluded with the accelerator's own range rule.  DRT_E_STATE before drt_scene_build. */
int drt_scene_trace_cpu(const drt_scene* s, int shadow, const float* rays, int64_t n, float* t, float* normal,
                        int32_t* object, uint8_t* occluded);
/* Scene::GetSkyboxColor (scene.cpp:380-458) for n directions -> n x 3 floats. */
int drt_scene_skybox_color_cpu(const drt_scene* s, const float* dirs, int64_t n, float* rgb);

/* ---- output image ---- */
/* u8fromfloat (maths.h:126-130: x*255.99f >= 255 ? 255 : (uint8_t)(x*255.99f), negatives -> 0)
 * of a float RGB frame, out[3*(x + RES_X*y) + c] — the img_Data fill of main.cpp:716-718
 * without its counter++ race (row 0 = bottom, as the frame). */
int drt_image_rgb8(const float* rgb, int32_t res_x, int32_t res_y, uint8_t* out);
/* saveImgFile (main.cpp:251-266) as DevIL writes a lower-left-origin image: an 8-bit RGB PNG
 * whose first (top) row is the frame's row RES_Y-1.  Returns 0 or DRT_E_INVALID / DRT_E_OOM /
 * -7 (file error). */
int drt_image_write_png(const char* path, const float* rgb, int32_t res_x, int32_t res_y);

#ifdef __cplusplus
}
#endif
#endif
