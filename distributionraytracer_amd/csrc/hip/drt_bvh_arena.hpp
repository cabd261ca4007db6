// drt_bvh_arena.hpp — what the two device BVH builders (drt_bvh_build.hip: the LBVH, drt_bvh_ploc.hip: PLOC)
// share: the scratch slices, the sort plan, and the launch of the stages both begin with (clear, primitive
// boxes, Morton keys, the stable radix sort), whose kernels live in drt_bvh_build.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../../include/drt.h"
#include "drt_scan_sort.hpp"

namespace drt {

// keys one sort workgroup ranks and stages in LDS: 16 KB of keys + 8 KB of payloads + 6 KB of counters, of
// the 64 KB a workgroup may hold
constexpr int kBvhSortTile = kTile;

// node data of the refit, 8 words per node id: box min, box max, depth, inner count
constexpr int kNodeWords = 8;

struct SortPlan {
  uint32_t skip[8];   // the pass's digit is the same for every key
  uint32_t src[8];    // the pass reads buffer B (1) or A (0)
  uint32_t final_sel; // the sorted keys / payloads are in buffer B (1) or A (0)
  uint32_t pad[3];
  uint32_t gbase[8][256];  // per pass: exclusive scan of the digit totals
};

// Everything the kernels share, sliced from one scratch allocation (bvh_build_scratch_bytes).
struct BvhArena {
  float4* pbox;        // 2 per primitive, scene order: (min, 0), (max, 0)
  uint64_t* key[2];
  uint32_t* pay[2];
  uint32_t* table;     // 256 x n_wg digit counts, digit-major, scanned in place
  uint32_t* ghist;     // 8 x 256
  SortPlan* plan;
  uint32_t* cbounds;   // ordered-integer centroid bounds: min xyz, max xyz
  uint32_t* left;      // per internal node: child ids
  uint32_t* right;
  uint32_t* first;     // per internal node: covered range of sorted positions (LBVH)
  uint32_t* last;
  uint32_t* parent;    // per node id (internal i -> i, sorted position j -> n - 1 + j)
  uint32_t* arrive;    // per internal node (LBVH)
  uint32_t* ndata;     // kNodeWords per node id
};

// the slices of `scratch` for n primitives; *total (if given) receives the bytes they take
BvhArena carve_bvh(void* scratch, uint32_t n, size_t* total);

// Stages 0 to 3 on `st`: cleared links, counters and info[0..3]; A.pbox; the (key, scene index) pairs sorted
// into A.key / A.pay [A.plan->final_sel].  Returns the first launch error.
hipError_t launch_bvh_sorted(const drt_prim* d_prims, uint32_t n, const BvhArena& A, uint32_t* d_info, hipStream_t st);

__device__ inline float smin(float a, float b) { return (b < a) ? b : a; }  // std::min, as drt_accel.cpp
__device__ inline float smax(float a, float b) { return (a < b) ? b : a; }  // std::max

}  // namespace drt
