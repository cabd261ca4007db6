// drt_grid_build.hpp — the device uniform-grid builder and commit (drt_grid_build.hip) as drt_capi.hip calls them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../../include/drt.h"
#include "drt_layout.hpp"

namespace drt {

enum : uint32_t { kGridNonFinite = 1u };  // GridBuildStatus::flags: an object box has a non-finite component

// The words the host reads back between the stages (64 B).
struct GridBuildStatus {
  uint32_t wbox[6];     // the world box as order-preserving unsigned words: min xyz, max xyz
  uint32_t flags;
  uint32_t scan_total;  // the last device-wide scan's total (the commit: 40-B record slots, padding included)
  uint64_t n_refs;      // sum of the objects' cell counts
  uint32_t pad[6];
};
static_assert(sizeof(GridBuildStatus) == 64, "the grid build status is 64 B");

// float of an order-preserving word of wbox
inline float grid_unordered(uint32_t o) { return bits_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

struct GridDims {
  int32_t n[3];
  float bmin[3], bmax[3];  // the grown box (grid_dims, include/drt_scene.hpp)
};

// device scratch of the per-object stages and of the per-reference stages
size_t grid_object_scratch_bytes(uint32_t n_prims);
size_t grid_refs_scratch_bytes(uint32_t n_refs);

// Stage 1: object boxes into obj_scratch, the world box and the non-finite flag into *status (cleared first).
hipError_t launch_grid_bounds(const drt_prim* d_prims, uint32_t n, void* obj_scratch, GridBuildStatus* status,
                              hipStream_t st);
// Stage 2: per object its cell range (24 B: ix, iy, iz min, then max) and the exclusive scan of the objects'
// cell counts (kept in obj_scratch); status->n_refs.
hipError_t launch_grid_ranges(uint32_t n, const GridDims& g, void* obj_scratch, int32_t* ranges,
                              GridBuildStatus* status, hipStream_t st);
// Stage 3 (n_refs < 2^31, n_cells < 2^31): cell_start[n_cells + 1] and cell_objs[n_refs] exactly as
// Grid::Build's, each cell's objects in ascending scene index.
hipError_t launch_grid_lists(uint32_t n, const GridDims& g, uint32_t n_refs, const void* obj_scratch,
                             const int32_t* ranges, void* refs_scratch, uint32_t* cell_start, uint32_t* cell_objs,
                             hipStream_t st);

struct GridCommitArgs {
  const drt_prim* prims_raw;   // scene order
  uint32_t n_prims, n_refs;
  uint32_t default_material;
  GridDims g;
  const uint32_t* cell_start;  // n_cells + 1
  const uint32_t* cell_objs;   // n_refs
  void* refs_scratch;          // grid_refs_scratch_bytes(n_refs)
  PrimRecord* prims;           // out: n_prims, scene order
  uint32_t* macro;             // out: cleared words of the macro-cell bitmap
  int macro_shift, macro_dim[2];
  uint32_t* tpos;              // triangle scenes: out, n_cells + 1
  float* tris;                 // triangle scenes: out, cleared; 40-B records in pairs
  PrimRecord* recs;            // other scenes: out, 48-B records, q2.w = scene index
  GridBuildStatus* status;
};
// Triangle scenes, first: tpos from cell_start; status->scan_total = record slots (size tris by it).
hipError_t launch_grid_commit_tpos(const GridCommitArgs& a, hipStream_t st);
// Then: the scene-order primitive records, the inline records of every reference, the macro-cell bitmap.
hipError_t launch_grid_commit(const GridCommitArgs& a, hipStream_t st);

}  // namespace drt
