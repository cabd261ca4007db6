// drt_grid_tree_commit.hpp — the device commit of a Grid scene's shadow tree (drt_grid_tree_commit.hip) as
// drt_capi.hip calls it: what drt_upload_grid_shadow_bvh uploads, written by kernels from a device-built tree.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../../include/drt.h"
#include "drt_layout.hpp"

namespace drt {

// GridTreeStatus::flags: why the grid keeps no tree (the Grid walk then answers every shadow query)
enum : uint32_t { kGridTreeLeafRoot = 1u, kGridTreeNoQuant = 2u, kGridTreeBigLeaf = 4u };

// The one thing the host reads back after the commit (64 B).
struct GridTreeStatus {
  uint32_t flags;
  uint32_t n_wide;      // 4-ary records
  uint32_t wide_depth;  // levels of the 4-ary tree reached (at most the launched ones)
  uint32_t pad0;
  double widen;         // what every child box was grown by on each side
  uint32_t pad[10];
};
static_assert(sizeof(GridTreeStatus) == 64, "the commit status is 64 B");

struct GridTreeCommitArgs {
  // in: a builder's output (launch_bvh_build / launch_ploc_build), the scene-order primitives it was built
  // from, the objects' cell ranges (launch_grid_ranges: six int32 per object)
  const drt_bvh_node* nodes;
  const uint32_t* order;
  const drt_prim* prims_raw;
  const int32_t* ranges;
  uint32_t n_prims, n_nodes, depth;
  uint32_t default_material;  // of a primitive without one (drt_upload_scene)
  int widen_log2;             // child boxes grow by 2^widen_log2 of the root box's largest absolute coordinate
  int nocert;                 // every range record inverted: no hit is certified (DRT_GRID_TREE_NOCERT)
  int max_wide_levels;        // a 4-ary tree deeper than this is refused anyway: no more frontier launches
  void* scratch;              // grid_tree_commit_scratch_bytes(n_prims)
  // out
  WideNodeRecord4* wide_recs;  // n_prims - 1 (at least one)
  PrimRecord* prims;           // n_prims in tree order, then kPrimPadBytes (64 B) of zeros
  LeafBoxRecord* range_recs;   // n_prims + 2: box[k] = (float)range[k], the two tail records zero
  GridTreeStatus* status;
};

size_t grid_tree_commit_scratch_bytes(uint32_t n_prims);

// Enqueue the commit on `st`; nothing is synchronised.  Returns the first launch error.
hipError_t launch_grid_tree_commit(const GridTreeCommitArgs& a, hipStream_t st);

}  // namespace drt
