// drt_bvh_commit.hpp — the device commit of a device-built tree (drt_bvh_commit.hip) as drt_capi.hip calls it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../../include/drt.h"
#include "drt_layout.hpp"

namespace drt {

// BvhCommitStatus::flags: why the tree gets no 4-ary shadow tree
enum : uint32_t { kCommitLeafRoot = 1u, kCommitNoQuant = 2u };

// The one thing the host reads back after a commit (64 B).
struct BvhCommitStatus {
  uint32_t flags;
  uint32_t n_lines;     // 128-B lines of inner records: the records fill slots [0, 2 * n_lines)
  uint32_t n_wide;      // 4-ary records
  uint32_t wide_depth;  // levels of the 4-ary tree reached (at most the launched ones)
  uint32_t root_desc;
  float root_box[6];
  uint32_t pad[5];
};
static_assert(sizeof(BvhCommitStatus) == 64, "the commit status is 64 B");

struct BvhCommitArgs {
  // in: the builder's output (launch_bvh_build) and the scene-order primitives it was built from
  const drt_bvh_node* nodes;
  const uint32_t* order;
  const drt_prim* prims_raw;
  uint32_t n_prims, n_nodes, depth;
  uint32_t default_material;  // of a primitive without one (drt_upload_scene)
  int wide;                   // build the 4-ary shadow tree and the leaf boxes
  int max_wide_levels;        // a 4-ary tree deeper than this is refused anyway: no more frontier launches
  void* scratch;              // bvh_commit_scratch_bytes(n_prims)
  // out
  NodeRecord* recs;           // 2 * n_inner slots (at least one)
  WideNodeRecord4* wide_recs; // n_inner
  LeafBoxRecord* leaf_boxes;  // n_prims + 2
  PrimRecord* prims;          // n_prims, tree order
  BvhCommitStatus* status;
};

size_t bvh_commit_scratch_bytes(uint32_t n_prims);

// Enqueue the commit on `st`.  Returns the first launch error.
hipError_t launch_bvh_commit(const BvhCommitArgs& a, hipStream_t st);

}  // namespace drt
