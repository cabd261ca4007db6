// drt_bvh_ploc.hpp — the device PLOC builder (drt_bvh_ploc.hip) as drt_capi.hip calls it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../../include/drt.h"

namespace drt {

#ifndef DRT_PLOC_RADIUS
#define DRT_PLOC_RADIUS 8  // 16: more rounds, a costlier tree, a slower frame (profiles/gpu_bvh_ploc.jsonl)
#endif
constexpr int kPlocRadius = DRT_PLOC_RADIUS;  // R: a cluster looks R clusters to each side
constexpr int kPlocSearchRounds = 64;  // after these, rounds pair neighbours whatever their boxes
constexpr int kPlocBatch = 8;          // rounds enqueued between two read-backs of the live count
constexpr int kPlocInfoWords = 8;      // d_info: {n_nodes, n_leaves, depth, 0, search rounds, forced rounds, 0, 0}

// bytes of device scratch a PLOC build of n_prims primitives needs (the LBVH builder's slices come first)
size_t ploc_build_scratch_bytes(uint32_t n_prims);

// The build on `st`, with the arguments and the output of launch_bvh_build; d_info has kPlocInfoWords words.
// Unlike launch_bvh_build it synchronises `st`: after every kPlocBatch rounds the live cluster count (4 bytes)
// is copied to the pinned word h_count.  Returns the first launch, copy or synchronisation error.
hipError_t launch_ploc_build(const drt_prim* d_prims, uint32_t n, void* d_scratch, drt_bvh_node* d_nodes,
                             uint32_t* d_order, uint32_t* d_info, uint32_t* h_count, hipStream_t st);

}  // namespace drt
