// drt_bvh_binned.hpp — the device binned-SAH builder (drt_bvh_binned.hip) as drt_capi.hip calls it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../../include/drt.h"

namespace drt {

#ifndef DRT_BINNED_WAVE
#define DRT_BINNED_WAVE 64  // 0: the level-wise rounds alone build every tree (a check of that path)
#endif
constexpr int kBinnedWave = DRT_BINNED_WAVE;  // a node of at most this many objects is finished by one wave
constexpr int kBinnedMaxRounds = 96;   // level-wise rounds: the traversal stack's bound (BVH::Set, drt_upload_bvh)
constexpr int kBinnedBatch = 8;        // rounds enqueued between two read-backs of the live node count
constexpr int kBinnedInfoWords = 8;    // d_info: {n_nodes, n_leaves, depth, 0, level-wise rounds, 0, largest leaf, 0}
constexpr int kBinnedHostWords = 4;    // h_count: {live nodes, wave-finished nodes, leaves above 64 objects, node ids}
static_assert(kBinnedWave >= 0 && kBinnedWave <= 64, "a wave holds one object per lane");

// bytes of device scratch a binned build of n_prims primitives needs
size_t binned_build_scratch_bytes(uint32_t n_prims);

// The build on `st`, with the arguments and the output of launch_ploc_build; d_info has kBinnedInfoWords words
// and the pinned h_count kBinnedHostWords.  It synchronises `st` after every kBinnedBatch rounds.  Returns the
// first launch, copy or synchronisation error.  A tree that still has unsplit nodes after kBinnedMaxRounds
// rounds is deeper than a traversal takes: h_count[0] is then not 0 and nothing has been written to d_nodes.
hipError_t launch_binned_build(const drt_prim* d_prims, uint32_t n, void* d_scratch, drt_bvh_node* d_nodes,
                               uint32_t* d_order, uint32_t* d_info, uint32_t* h_count, hipStream_t st);

}  // namespace drt
