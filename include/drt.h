/*
 * drt.h — C ABI of the MI355X distribution ray tracer (libdrt.so).
 *
 * This is the drop-in boundary for the reference's hot path (rita-mota/DistributionRayTracer,
 * paths relative to DistributionRayTracer/).  The reference has no FFI: its hot path is the
 * C++ class API called from main.cpp.  Each entry point below names the reference interface
 * it replaces:
 *
 *   drt_upload_scene   <- Scene / Camera / Light / Material / Object state read by
 *                         rayTracing() (scene.h:24-231, camera.h:12-101)
 *   drt_set_camera     <- Camera::SetEye (camera.h:63-72), called by renderScene() every frame
 *                         in draw mode (main.cpp:530-533): the camera alone, scene resident
 *   drt_upload_bvh     <- BVH::Build result (rayAccelerator.h:87-94, bvh.cpp:27-227)
 *   drt_upload_grid    <- Grid::Build result (rayAccelerator.h:12-37, grid.cpp:30-97)
 *   drt_trace_closest  <- BVH::Traverse(Ray&, Object**, HitRecord&)  (bvh.cpp:231-314)
 *                         Grid::Traverse(Ray&, Object**, HitRecord&) (grid.cpp:247-306)
 *                         the NONE linear scan                       (main.cpp:310-336)
 *   drt_trace_shadow   <- BVH::Traverse(Ray&) (bvh.cpp:316-391), Grid::Traverse(Ray&)
 *                         (grid.cpp:309-358)
 *   drt_render         <- renderScene() zone B (main.cpp:525-738) incl. rayTracing()
 *                         (main.cpp:294-521): jittered AA, light-sample shuffle, thin-lens
 *                         DoF, Whitted area-light grid, Phong + shadows, refraction/reflection
 *
 * Conventions: plain C types only; caller owns all host memory; the context owns all device
 * memory.  Every function returns 0 (DRT_OK) or a negative drt_status and never exits the
 * process; drt_last_error() describes the last failure.  One host thread per context.
 * Calls are blocking except drt_render_device, which is asynchronous on the given stream.
 *
 * Frame buffer layout (main.cpp:705-714): float RGB, index 3*(x + RES_X*y), row y = 0 is the
 * BOTTOM row of the image (OpenGL / DevIL lower-left origin).
 *
 * RNG: the reference uses CRT rand() seeded with time()^2; parity is defined on the keyed
 * stream of SURVEY.md §8c — the k-th rand() call inside pixel P = y*RES_X + x returns
 * mix32(seed ^ mix32(P*0x9E3779B9 ^ mix32(k))) >> 17, RAND_MAX = 0x7FFF.
 */
#ifndef DRT_H
#define DRT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRT_ABI_VERSION 3
#define DRT_FRAME_SLOTS 4 /* drt_frame_params.slot: 0 .. DRT_FRAME_SLOTS-1 */

typedef enum {
  DRT_OK = 0,
  DRT_E_INVALID = -1,     /* bad argument / malformed scene                         */
  DRT_E_HIP = -2,         /* HIP runtime error                                        */
  DRT_E_NODEVICE = -3,    /* no usable gfx950 device                                  */
  DRT_E_OOM = -4,         /* device allocation failed                                 */
  DRT_E_STATE = -5,       /* call order (e.g. render before upload)                   */
  DRT_E_UNSUPPORTED = -6  /* feature outside this build                               */
} drt_status;

enum { DRT_ACCEL_NONE = 0, DRT_ACCEL_GRID = 1, DRT_ACCEL_BVH = 2 };               /* scene.h:22 */
enum { DRT_PRIM_TRIANGLE = 0, DRT_PRIM_SPHERE = 1, DRT_PRIM_PLANE = 2, DRT_PRIM_BOX = 3 };
enum { DRT_LIGHT_POINT = 0, DRT_LIGHT_QUAD = 1 };                                  /* scene.h:16 */

typedef struct drt_ctx drt_ctx;

typedef struct {
  int32_t device;       /* HIP device ordinal                                        */
  int32_t reserved[7];
} drt_options;

/* Camera frame exactly as the host Camera constructor computes it (camera.h:32-61). */
typedef struct {
  float eye[3], u[3], v[3], n[3];
  float w, h, plane_dist, focal_ratio, aperture;
  int32_t res_x, res_y;
} drt_camera;

/* Light (scene.h:68-107): quad lights span pos + e1*s + e2*t. */
typedef struct {
  int32_t type;
  float pos[3];
  float e1[3], e2[3];
  uint32_t grid_res;
} drt_light;

/* Material (scene.h:34-66); refl is m_Refl (= Ks for P3F materials, scene.h:42). */
typedef struct {
  float diff[3];
  float kd;
  float spec[3];
  float ks, shine, refl, trans, ior;
} drt_material;

/* Object (scene.h:109-180).  triangle: a,b,c = P0,P1,P2; sphere: a = centre, r = radius;
 * plane: a = PN, r = D; box: a = min, b = max.  material < 0 = none (reference UB). */
typedef struct {
  int32_t type;
  int32_t material;
  float a[3], b[3], c[3];
  float r;
} drt_prim;

typedef struct {
  drt_camera camera;
  const drt_material* materials;
  int32_t n_materials;
  const drt_prim* prims;
  int32_t n_prims;
  const drt_light* lights;
  int32_t n_lights;
  float background[3];          /* bclr (scene.cpp:680)                                  */
  int32_t accel;                /* DRT_ACCEL_*                                           */
  uint32_t spp;                 /* 0 = Whitted (main.cpp:1005-1010)                      */
  int32_t has_skybox;           /* env (scene.cpp:687)                                   */
  const uint8_t* skybox[6];     /* faces RIGHT..BACK, rows bottom-up (scene.cpp:345)     */
  int32_t sky_w[6], sky_h[6], sky_bpp[6];
} drt_scene_desc;

/* One BVHNode (rayAccelerator.h:50-67) in the reference's node numbering: inner nodes keep
 * their two children at index and index+1 (bvh.cpp:206-222); leaves cover
 * object_order[index .. index+n_objs). */
typedef struct {
  float bmin[3], bmax[3];
  uint32_t leaf;
  uint32_t index;
  uint32_t n_objs;
} drt_bvh_node;

/* drt_frame_params.flags: DRT_FRAME_STATS counts rays / node visits / primitive tests;
 * DRT_FRAME_SHARD_LAYOUT makes drt_render_device write the shard-compact tile buffer of
 * drt_shard_layout() even for n_shards == 1 (a one-device drt_group);
 * DRT_FRAME_REFERENCE_ORDER (also a drt_set_trace_flags flag) walks every shadow query
 * (BVH::Traverse(Ray&), bvh.cpp:316-391) on the reference's binary tree in its visit order, so
 * that the shadow node / leaf / primitive counts equal the reference's.  Without it, shadow
 * queries of finite rays walk a 4-ary tree collapsed from the same BVH: the occlusion answer,
 * hence every frame, is identical (an any-hit query does not depend on the visit order), and
 * drt_frame_stats counts that work in its wide_* fields. */
enum { DRT_FRAME_STATS = 1, DRT_FRAME_SHARD_LAYOUT = 2, DRT_FRAME_REFERENCE_ORDER = 4 };
/* drt_set_trace_flags only: a Grid scene's batched shadow queries (drt_trace_shadow, drt_trace_device) run
 * on its cell tree (drt_upload_grid_shadow_bvh) with the Grid walk for the queries the tree leaves
 * undecided; drt_trace_stats then reports the wide_* counters.  The answers are the walk's.  Without a cell
 * tree the flag changes nothing. */
enum { DRT_TRACE_GRID_TREE = 8 };

typedef struct {
  uint32_t seed;       /* keyed-RNG seed                                                */
  int32_t max_depth;   /* MAX_DEPTH (main.cpp:34) = 4                                   */
  float roughness;     /* roughness_param (main.cpp:507) = 0                            */
  int32_t shard;       /* this rank's shard: the tiles at dealing positions p with
                          p % n_shards == shard (sharding.py: row ty rotated by ty tiles)  */
  int32_t n_shards;    /* 1 = whole frame                                               */
  int32_t tile;        /* tile edge in pixels (0 -> 16)                                 */
  int32_t flags;       /* DRT_FRAME_STATS: count rays / node visits / prim tests        */
  int32_t light_spp;   /* extension: shadow samples per quad light per
                          hit, 0 or 1 = the reference (main.cpp:391: one sample)          */
  int32_t progressive_frame; /* 0: renderScene zone B.  n >= 1: zone A (main.cpp:536-599) with
                          FrameCount n — one jittered sample per pixel, written (n = 1) or
                          lerped into the output with weight 1/n (n > 1: the output buffer is
                          read, so pass the previous frame back); n >= MAX_SAMPLES (10000)
                          leaves the output untouched (main.cpp:537)                     */
  int32_t slot;        /* frame scratch slot, 0 .. DRT_FRAME_SLOTS-1: frames on different
                          slots of one context may run concurrently on different streams
                          (pipelining); a frame on a slot whose previous frame ran on another
                          stream waits for that frame on the device; other values are
                          DRT_E_INVALID                                                    */
  int32_t reserved[2];
} drt_frame_params;

typedef struct {
  uint64_t closest_rays, shadow_rays;     /* Traverse() calls                            */
  uint64_t closest_inner, closest_leaf;   /* node-loop iterations (bvh.cpp:245)           */
  uint64_t shadow_inner, shadow_leaf;     /* (bvh.cpp:331)                                */
  uint64_t closest_prims, shadow_prims;   /* Object::hit calls                           */
  uint64_t samples;                       /* rayTracing(depth = 1) calls                 */
  double render_ms;                        /* device time of the last drt_render*        */
  double kernel_ms;                        /* device time of the path-tracing kernel     */
  uint64_t wave_node_iters;                /* node-loop iterations counted once per wave */
  uint64_t wave_path_iters, lane_path_iters; /* path-loop iterations per wave / per lane  */
  uint64_t cycles_refill, cycles_node, cycles_shade; /* persistent kernel: s_memtime cycles */
  uint64_t stack_pushes, stack_spills;   /* traversal-stack pushes / those beyond the LDS part */
  uint64_t wave_leaf_iters, cycles_leaf; /* node-loop iterations that ran the leaf block / its cycles */
  /* in-order keyed-stream frames (DoF / glossy): pixels handed between waves at the frame's tail
   * and taken up again (0 when the hand-over was off for the frame); filled for every frame */
  uint64_t seq_pushed, seq_popped;
  int32_t seq_handover;                   /* the hand-over was on for the frame                  */
  int32_t reserved;
  /* shadow queries that walked the 4-ary shadow tree (not DRT_FRAME_REFERENCE_ORDER): queries,
   * inner-node visits, leaf visits, primitive tests, exact leaf-box checks of in-range hits.
   * shadow_inner / shadow_leaf / shadow_prims then count only the queries (non-finite rays)
   * that walked the reference's binary tree. */
  uint64_t wide_shadow_rays, wide_inner, wide_leaf, wide_prims, wide_verify;
  /* a Grid scene's shadow tree (drt_upload_grid_shadow_bvh): its queries left to the Grid walk */
  uint64_t wide_grid_walks;
} drt_frame_stats;

int drt_create(drt_ctx** out, const drt_options* opt);
void drt_destroy(drt_ctx* ctx);
const char* drt_last_error(const drt_ctx* ctx);
int drt_abi_version(void);

int drt_upload_scene(drt_ctx* ctx, const drt_scene_desc* scene);
/* Replace the camera of the resident scene (Camera::SetEye, camera.h:63-72; the interactive
 * renderer calls it every frame, main.cpp:530-533).  Primitives, lights, materials, skybox and
 * the BVH / grid stay resident: nothing is re-packed or copied.  The next frame issued uses the
 * new camera; frames already issued keep theirs.  DRT_E_STATE without a scene. */
int drt_set_camera(drt_ctx* ctx, const drt_camera* camera);
int drt_upload_bvh(drt_ctx* ctx, const drt_bvh_node* nodes, uint32_t n_nodes, const uint32_t* object_order,
                   uint32_t n_objects);
/* A second builder, on the device: a linear BVH (Karras 2012) of the resident primitives — Morton keys of
 * the box centroids, a stable radix sort, the binary radix tree, a refit — in hand-written HIP
 * (csrc/hip/drt_bvh_build.hip).  The tree is not the reference's binned-SAH tree (drt_scene_build keeps that
 * one, node for node); it has the same shape rules (leaves of one or two objects, children side by side),
 * every object's box is the host's GetBoundingBox() bit for bit, and it is committed through drt_upload_bvh
 * itself, so closest hits and occlusion answers are the scene's.  The build is deterministic. */
typedef struct {
  uint32_t n_nodes, n_leaves, depth;
  double build_ms;   /* device time of the build kernels, HIP events; the first build after a
                        drt_upload_scene also stages the primitives' vertices on the device (the resident
                        records hold triangle edges, which do not give the vertices back bit for bit),
                        and that copy is inside this time                                             */
  double fetch_ms;   /* device -> host copy of nodes and order                  */
  double commit_ms;  /* host clock around the existing drt_upload_bvh commit    */
  uint32_t builder;        /* DRT_BVH_BUILDER_LBVH, DRT_BVH_BUILDER_PLOC or DRT_BVH_BUILDER_BINNED       */
  uint32_t rounds;         /* PLOC: search rounds run; binned: level-wise rounds run (0 for the LBVH)    */
  uint32_t forced_rounds;  /* PLOC: rounds after them that paired neighbours whatever their boxes        */
} drt_bvh_build_info;

/* After drt_upload_scene: build a BVH of the resident primitives on the device and commit it
 * exactly as drt_upload_bvh would.  nodes_out (capacity 2*n_prims-1) / order_out (n_prims) may be
 * NULL; otherwise they receive the tree.  DRT_E_STATE without a scene, DRT_E_INVALID for a scene without
 * primitives, DRT_E_OOM / DRT_E_HIP as elsewhere. */
int drt_build_bvh_device(drt_ctx* ctx, drt_bvh_node* nodes_out, uint32_t* order_out, drt_bvh_build_info* info);
/* The same with the builder chosen, one of three.  DRT_BVH_BUILDER_PLOC (csrc/hip/drt_bvh_ploc.hip) is parallel locally-ordered
 * clustering (Meister and Bittner 2018) over the LBVH's Morton order: every round each cluster looks 8 clusters
 * to each side for the one whose union box has the least surface, mutual nearest neighbours merge, and the
 * cluster array is compacted; after 64 such rounds neighbours are paired whatever their boxes, so the depth is
 * at most 91.  The tree has the LBVH's shape rules and goes through the same commits; it costs more rounds of
 * kernels to build and has a lower surface-area cost (README.md, Use, for the measured figures).  flags: 0 or
 * DRT_BVH_EX_COMMIT_DEVICE (the commit of drt_build_bvh_device_commit).  drt_build_bvh_device and
 * drt_build_bvh_device_commit are this call with DRT_BVH_BUILDER_LBVH.
 * DRT_BVH_BUILDER_BINNED (csrc/hip/drt_bvh_binned.hip) builds the reference's binned-SAH tree itself, the one
 * drt_scene_build builds on the host: leaf, index, n_objs and every box equal it bit for bit, and every leaf
 * holds the same objects, in ascending centroid on the leaf's sort axis with equal keys in scene order (the
 * host's sequence wherever a leaf's keys are distinct).  One exception to the boxes' bits: where the objects of
 * one bucket have both +0 and -0 as a bound, the host keeps the zero its sort met first and this builder -0 as a
 * minimum, +0 as a maximum.  Nodes above 64 objects are split level by level
 * (info->rounds rounds, forced_rounds 0), smaller ones by one wave each.  The reference's tree may hold leaves of
 * any size: with DRT_BVH_EX_COMMIT_DEVICE a tree with a leaf of 31 objects or more is committed by the host
 * (drt_get_bvh_commit_info says so), every other one on the device.  DRT_E_INVALID for a tree deeper than the 96
 * levels drt_upload_bvh takes.
 * DRT_E_INVALID for any other builder or flag. */
#define DRT_BVH_BUILDER_LBVH 0
#define DRT_BVH_BUILDER_PLOC 1
#define DRT_BVH_BUILDER_BINNED 2
#define DRT_BVH_EX_COMMIT_DEVICE 1
int drt_build_bvh_device_ex(drt_ctx* ctx, int builder, int flags, drt_bvh_node* nodes_out, uint32_t* order_out,
                            drt_bvh_build_info* info);
/* The figures of the context's last device build (DRT_E_STATE before one). */
int drt_get_bvh_build_info(const drt_ctx* ctx, drt_bvh_build_info* info);
/* drt_build_bvh_device with the commit on the device too (csrc/hip/drt_bvh_commit.hip): the inner records and
 * their placement in 128-B lines, the leaf boxes, the primitive records in tree order and the 4-ary shadow
 * tree are written by HIP kernels from the builder's output, and every query answers and counts exactly as
 * after the host commit of the same tree; only where a record sits in memory differs.  With nodes_out and
 * order_out both NULL the tree never leaves the device: 64 B of status words are all that is copied back, and
 * info->fetch_ms is 0.  info->commit_ms is the device time of the commit kernels (HIP events).  The host
 * commits instead (and drt_get_bvh_commit_info says so) under DRT_NODE_LAYOUT != 1, DRT_WIDE_ORDER != 2 or a
 * library built with DRT_WIDE8.  Errors as drt_build_bvh_device. */
int drt_build_bvh_device_commit(drt_ctx* ctx, drt_bvh_node* nodes_out, uint32_t* order_out, drt_bvh_build_info* info);
typedef struct {
  uint32_t on_device; /* 1: committed by the device kernels, 0: by the host (drt_upload_bvh)          */
  uint32_t has_wide;  /* the tree has a 4-ary shadow tree                                              */
  uint32_t n_slots;   /* 64-B inner record slots, padding slots included                              */
  uint32_t n_wide;    /* 4-ary records (0 without a shadow tree)                                       */
} drt_bvh_commit_info;
/* The context's last BVH commit, by drt_upload_bvh or on the device (DRT_E_STATE without a committed BVH). */
int drt_get_bvh_commit_info(const drt_ctx* ctx, drt_bvh_commit_info* info);
int drt_upload_grid(drt_ctx* ctx, const int32_t dims[3], const float bmin[3], const float bmax[3],
                    const int64_t* cell_start /* nx*ny*nz+1 */, const int32_t* cell_objs, int64_t n_refs);
/* The uniform grid built on the device too (csrc/hip/drt_grid_build.hip): object boxes and the world box, the
 * cell ranges, a reference expansion balanced by reference, a stable radix sort of the (cell, object) pairs and
 * a scan over the cells, in hand-written HIP.  Unlike the device BVH, the result is exactly the host's:
 * Grid::Build is a deterministic function of the object boxes, and dims, the grown box, cell_start and
 * cell_objs come out bit for bit as drt_scene_build makes them (the cell counts are computed on the host with
 * the same pow, from the world box alone).  Frames and every work count equal the host path's.
 * The Grid scene's shadow tree is built here too when asked for (DRT_GRID_SHADOW_LBVH / DRT_GRID_SHADOW_PLOC
 * below); without it a device-built grid answers shadow queries by the Grid walk, which renders the same frame
 * bit for bit at a lower frame rate, until drt_upload_grid_shadow_bvh adds a tree. */
typedef struct {
  int32_t dims[3];
  float bmin[3], bmax[3]; /* the grown box                                                              */
  int64_t n_cells, n_refs;
  double build_ms;   /* device time from the first build kernel to the last, HIP events; the first build after
                        a drt_upload_scene also stages the primitives on the device inside this time, and
                        the two short host steps between the stages (cell counts, allocation) are inside  */
  double fetch_ms;   /* device -> host copy of the lists (0 when they stayed on the device)               */
  double commit_ms;  /* host clock around drt_upload_grid, or device time of the commit kernels           */
  uint32_t on_device; /* 1: committed by the device kernels, 0: by the host (drt_upload_grid)             */
  uint32_t shadow_tree; /* the shadow tree built with the grid: 0 none (the walk answers), 1 LBVH, 2 PLOC   */
} drt_grid_build_info;
#define DRT_GRID_COMMIT_DEVICE 1
/* (bit 2 is the host wrapper's DRT_GRID_NO_INSTALL, include/drt_host.h) */
#define DRT_GRID_SHADOW_LBVH 4
#define DRT_GRID_SHADOW_PLOC 8
/* After drt_upload_scene: build the grid of the resident primitives on the device with Grid::Build's cell
 * factor m (2 in the reference).  flags = 0: the lists are fetched and committed through drt_upload_grid itself.
 * DRT_GRID_COMMIT_DEVICE: the buffers drt_upload_grid fills (cell lists, inline records, tpos, macro-cell
 * bitmap, scene-order primitives) are written by HIP kernels from the device-resident lists, byte for byte the
 * same, and nothing but status words is copied back; drt_upload_grid_shadow_bvh then answers DRT_E_STATE until a
 * drt_fetch_grid_device has brought the objects' cell ranges to the host.
 * DRT_GRID_SHADOW_LBVH or DRT_GRID_SHADOW_PLOC (one of them, with either commit): once the grid is committed,
 * the LBVH or the PLOC builder (drt_build_bvh_device_ex) builds a tree of the resident primitives and HIP
 * kernels (csrc/hip/drt_grid_tree_commit.hip) commit it as the Grid scene's shadow tree — what
 * drt_upload_grid_shadow_bvh uploads for a triangle scene, from the cell ranges the grid build left on the
 * device, with one 64-B status read.  info->shadow_tree says which tree is resident; drt_get_bvh_build_info
 * then reports that tree's figures, its commit_ms the device time of the commit kernels.  No tree
 * (shadow_tree = 0, the Grid walk answers, no error) for a scene with other primitives than triangles, under
 * DRT_GRID_SHADOW_TREE=0, or when the tree has a leaf root, a record that does not quantise or too many
 * levels for the shadow stack.  DRT_E_STATE without a scene,
 * DRT_E_INVALID for a scene without primitives, other flag bits or both shadow bits, DRT_E_UNSUPPORTED for an
 * object box with a non-finite component, 2^31 cells or references or more; DRT_E_OOM / DRT_E_HIP as
 * elsewhere. */
int drt_build_grid_device(drt_ctx* ctx, float m, int flags, drt_grid_build_info* info);
/* The lists of the resident device-built grid: cell_start (n_cells + 1) and cell_objs (n_refs) as
 * drt_upload_grid takes them, sizes from the info.  Either may be NULL.  DRT_E_STATE unless the resident grid
 * came from drt_build_grid_device. */
int drt_fetch_grid_device(drt_ctx* ctx, int64_t* cell_start, int32_t* cell_objs);
/* The figures of the context's last drt_build_grid_device (DRT_E_STATE before one). */
int drt_get_grid_build_info(const drt_ctx* ctx, drt_grid_build_info* info);
/* Optional, after drt_upload_grid: a BVH of the same objects (the BVH::Build result, as drt_upload_bvh
 * takes it).  A triangle scene's wavefront shadow queries then walk a 4-ary tree collapsed from it with
 * widened boxes, and a hit counts only with a Grid cell certificate (the ray's point at the hit lies well
 * inside a cell the object is listed in, so Grid::Traverse(Ray&), grid.cpp:309-358, finds it too).
 * A scene with other primitives (spheres, planes, boxes) gets a cell tree instead: the BVH's topology over
 * the objects' cell ranges, in integer cell coordinates.  The walk tests an object exactly when the ray
 * crosses its cell range, so a hit counts when the ray passes well inside that range and is ignored when
 * the ray stays well outside it, whatever the primitive's own extent (a plane's reaches past its box).
 * Queries neither tree decides are walked on the Grid, so the answers are Grid::Traverse(Ray&)'s.
 * DRT_GRID_CELL_TREE: 0 (default) no cell tree (DRT_E_UNSUPPORTED for such a scene), 1 scenes with
 * non-triangle primitives, 2 triangle scenes too, in place of the widened tree.  It is off by default
 * because the shipped balls_high scene measured 0.46-0.50x the walk's frame rate on it
 * (profiles/grid_cell_tree_ab.jsonl).  A grid with an axis over
 * 1024 cells gets no cell tree (DRT_E_UNSUPPORTED; the walk answers).  Any drt_upload_scene /
 * drt_upload_grid / drt_upload_bvh drops the trees.  DRT_GRID_SHADOW_TREE=0 keeps the Grid walk for every
 * query. */
#define DRT_GRID_CELL_TREE_DEFAULT 0
int drt_upload_grid_shadow_bvh(drt_ctx* ctx, const drt_bvh_node* nodes, uint32_t n_nodes,
                               const uint32_t* object_order, uint32_t n_objects);

/* How a frame would run (no device work): work items (a (pixel, sample) pair, or a pixel whose
 * samples run in order), float4 sample slots, the frame mode (0 AA, 1 in-order keyed stream,
 * 2 Whitted quad grid, 3 Whitted point, 4 progressive) and whether the persistent kernel takes it
 * (frames of >= 0xF0000000 work items run the 64-bit one-item-per-thread kernel instead). */
typedef struct {
  uint64_t work_items;
  uint64_t sample_slots;
  int32_t mode;
  int32_t persistent;
  int32_t tiles_in_shard;
  int32_t passes;      /* 2: a pass over the samples' closest hits and a pass over every sample with
                          its closest hits read back; 1 otherwise.  Two passes for:
                          - in-order frames (DoF / glossy) of scenes without refraction (a pixel's
                            samples in order);
                          - AA frames of BVH (shadow tree uploaded) / Grid scenes of >= 1024 objects
                            whose whole frame has >= 2^23 samples or whose scene has >= 2^19 objects,
                            and at any size when the scene has non-triangle primitives and no
                            refracting material;
                          - Whitted frames of such scenes: quad light 0 at any size (one closest-hit
                            chain per pixel shared by its gridRes light samples); point light by the
                            AA size rule, and at any size on a Grid scene of mixed primitives without
                            a refracting material.
                          With a refracting material the AA / Whitted passes record each sample's
                          whole closest-hit tree (<= 2^(max_depth+1) - 1 hits) if it fits 32 GB.  The
                          plan depends on the params and the uploaded scene only, and drt_render
                          follows it.  Both plans render the same frame; the stats differ only in
                          where shadow work is counted (shadow_* on the reference tree, wide_* on
                          the shadow tree) and, for quad-light Whitted frames, in closest_* (gridRes
                          times fewer traversals). */
  int32_t wavefront;   /* 1: pass 2 of this two-pass frame runs as a wavefront — every shadow query of
                          the frame generated from the recorded closest hits, answered by a streaming
                          kernel (BVH: trace_stream on the shadow tree; Grid: its stepper's query
                          stream), then combined per sample with the frame's reduce folded in.  Every
                          two-pass frame without refraction: AA, Whitted and in-order (DoF / glossy)
                          frames, BVH and Grid (< 2^32 query slots; the query buffers in chunks of at
                          most DRT_WAVEFRONT_CHUNK_BYTES, default 24 GB, per frame slot).
                          DRT_WAVEFRONT=0 (DRT_WAVEFRONT_GRID=0, DRT_WAVEFRONT_INORDER=0 per kind):
                          the persistent replay.  A frame whose query buffers cannot be allocated runs
                          the persistent replay, which renders the same frame. */
  int32_t reserved[3];
} drt_frame_plan;
int drt_plan_frame(const drt_ctx* ctx, const drt_frame_params* params, drt_frame_plan* out);

/* RES_X, RES_Y of the uploaded scene's camera (DRT_E_STATE without a scene). */
int drt_frame_resolution(const drt_ctx* ctx, int32_t res_xy[2]);

/* Whole frame into host memory (RES_Y*RES_X*3 floats). */
int drt_render(drt_ctx* ctx, const drt_frame_params* params, float* rgb_out);

/* Tile-sharded frame into DEVICE memory, asynchronous on `hip_stream` (a hipStream_t, NULL =
 * the context's stream).  With n_shards == 1 the output is the full frame; otherwise it is
 * the shard-compact tile buffer of drt_shard_layout(). */
int drt_shard_layout(const drt_ctx* ctx, const drt_frame_params* params, int64_t* tiles_in_shard,
                     int64_t* floats_per_shard);
int drt_render_device(drt_ctx* ctx, const drt_frame_params* params, float* d_out, void* hip_stream);
/* Reassemble n_shards shard-compact buffers (laid end to end, floats_per_shard apart) into a
 * full device frame. */
int drt_unshard_device(drt_ctx* ctx, const drt_frame_params* params, const float* d_shards, float* d_frame,
                       void* hip_stream);

/* Batched ray queries against the uploaded scene (rays: n x {ox,oy,oz,dx,dy,dz}).
 * closest: t (FLT_MAX on miss), the HitRecord normal, object index (-1 on miss).
 * shadow: 1 if occluded, with the accelerator's own range rule. */
int drt_trace_closest(drt_ctx* ctx, const float* rays, int32_t n, float* t, float* normal, int32_t* object);
int drt_trace_shadow(drt_ctx* ctx, const float* rays, int32_t n, uint8_t* occluded);

/* The same queries on DEVICE buffers, asynchronous on `hip_stream` (NULL = the context's
 * stream): d_rays n x 6 floats; closest fills d_t / d_normal / d_object, shadow d_occluded.
 * BVH scenes run the streaming traversal kernel (one query per lane, lanes refilled as they
 * finish).  Replaces the same BVH/Grid Traverse calls as drt_trace_closest / drt_trace_shadow.
 * Batched queries of one context are serialised: a query issued on another stream waits (on
 * the device) for the previous one, whose scratch records and claim counter it reuses. */
int drt_trace_device(drt_ctx* ctx, int shadow, const float* d_rays, int32_t n, float* d_t, float* d_normal,
                     int32_t* d_object, uint8_t* d_occluded, void* hip_stream);
/* flags for later batched queries: DRT_FRAME_STATS counts their traversal work, DRT_FRAME_REFERENCE_ORDER,
 * DRT_TRACE_GRID_TREE */
int drt_set_trace_flags(drt_ctx* ctx, int flags);
/* Device time of the streaming traversal kernel of the most recent BVH batched query
 * (kernel_ms) and, with DRT_FRAME_STATS set, its ray / node / leaf / primitive counters;
 * zeroes for Grid / NONE queries.  Waits for that query. */
int drt_trace_stats(drt_ctx* ctx, drt_frame_stats* out);

/* Counters (frames rendered with DRT_FRAME_STATS) and device times of the most recent frame;
 * waits for that frame. */
int drt_get_stats(drt_ctx* ctx, drt_frame_stats* out);

/* Device durations of the most recent min(max_frames, 512) frames, oldest first: the
 * path-tracing kernel (path_ms) and kernel + reduce (total_ms), from HIP events recorded on the
 * stream each frame ran on.  Waits for those frames.  Returns the count written (>= 0). */
int drt_frame_times(drt_ctx* ctx, int max_frames, double* path_ms, double* total_ms);
/* The same frames as absolute spans on one device clock, in ms from the path-kernel start of the
 * oldest frame returned: path-kernel start / end and frame end.  Frames on different streams
 * overlap; the union of their path-kernel spans is the device time the path kernel held. */
int drt_frame_spans(drt_ctx* ctx, int max_frames, double* path_start, double* path_end, double* frame_end);

/* Diagnostics of the last stats frame (DRT_FRAME_STATS) rendered by the persistent kernel: per resident
 * wave of its pass-1 (pass = 0) or pass-2 (pass = 1, the persistent replay or the Grid's query stream)
 * launch, the (start, end) s_memrealtime stamps (100 MHz) in start_end[2 * w], [2 * w + 1]; 0 = no such
 * wave.  Returns the number of wave slots written (<= max_waves).  No reference counterpart: it measures
 * the tail of a launch. */
int drt_frame_wave_times(drt_ctx* ctx, int pass, uint64_t* start_end, int64_t max_waves);

/* Device time of each launch of the last wavefront frame's pass 2 (the frame issued last whose plan
 * has `wavefront`): out_ms = {wf_gen, shadow-query stream (trace_stream / the Grid's MODE_QSTREAM),
 * wf_combine}, summed over its chunks (HIP events between the launches on the frame's stream; the first
 * 64 chunks).  Waits for that frame.  Returns the chunks counted; DRT_E_STATE before any wavefront
 * frame.  Read it before the next frame is issued. */
int drt_frame_stage_times(drt_ctx* ctx, double out_ms[3]);
/* The same frames' passes: a two-pass frame (drt_frame_plan.passes == 2) is the closest-chain pass
 * then the replay pass, timed from the path-kernel start to the end of the first launch and from
 * there to the path-kernel end (HIP events on the frame's stream; pass1 + pass2 = path_ms of
 * drt_frame_times).  A one-pass frame reports its path kernel as pass 1 and ~0 for pass 2 (two
 * events recorded back to back: a few microseconds).  For a
 * frame rendered alone these are the launches' device times; with frames in flight a pass's span
 * also holds its waits for CU room.  Waits for those frames.  Returns the count written (>= 0). */
int drt_frame_pass_times(drt_ctx* ctx, int max_frames, double* pass1_ms, double* pass2_ms);

/* ---- several GPUs behind one handle (main.cpp:603 is the loop being split) ----
 * One drt_ctx per device, one HIP stream per device and an RCCL clique over them
 * (ncclCommInitAll, librccl loaded at run time).  A frame: every device renders its interleaved
 * 16x16 tiles (shard r of n, the drt_frame_params.shard dealing) into a shard buffer, one
 * ncclAllGather moves the shards over xGMI, device 0 reassembles the frame.  Upload the scene
 * to every device's context (drt_group_ctx + drt_upload_*, or drt_group_scene_upload in
 * drt_host.h).  Progressive frames need a one-device group. */
typedef struct drt_group drt_group;
/* devices: n_devices distinct ordinals, or NULL for 0 .. n_devices-1 */
int drt_group_create(drt_group** out, int n_devices, const int32_t* devices);
void drt_group_destroy(drt_group* g);
const char* drt_group_last_error(const drt_group* g);
int drt_group_size(const drt_group* g);
drt_ctx* drt_group_ctx(drt_group* g, int rank);
/* Whole frame into host memory (RES_Y*RES_X*3 floats, row 0 = bottom); blocking.  params:
 * n_shards 0 or 1 (the group deals the tiles). */
int drt_group_render(drt_group* g, const drt_frame_params* params, float* rgb_out);
/* Whole frame into DEVICE memory on device 0 (d_frame: RES_Y*RES_X*3 floats), asynchronous:
 * device 0's work on `stream0` (NULL = the group's), the other devices' on the group's streams.
 * Shard and gather buffers belong to params->slot: frames on different slots do not share them,
 * and a frame on a slot whose last frame ran on another stream0 waits for that frame's reassembly
 * (on the device). */
int drt_group_render_device(drt_group* g, const drt_frame_params* params, float* d_frame, void* stream0);
/* drt_set_camera on every device of the group. */
int drt_group_set_camera(drt_group* g, const drt_camera* camera);
/* Wait for every device's stream. */
int drt_group_synchronize(drt_group* g);

#ifdef __cplusplus
}
#endif
#endif
