// drt_bvh_build.hpp — the device LBVH builder (drt_bvh_build.hip) as drt_capi.hip calls it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../../include/drt.h"

namespace drt {

// bytes of device scratch a build of n_prims primitives needs
size_t bvh_build_scratch_bytes(uint32_t n_prims);

// Enqueue the build on `st`: d_prims are the scene-order drt_prim records (n of them, 1 <= n <= 2^26),
// d_nodes receives up to 2n - 1 records and d_order n scene indices in the drt_upload_bvh format, d_info
// {n_nodes, n_leaves, depth, 0}.  Returns the first launch error.
hipError_t launch_bvh_build(const drt_prim* d_prims, uint32_t n, void* d_scratch, drt_bvh_node* d_nodes,
                            uint32_t* d_order, uint32_t* d_info, hipStream_t st);

}  // namespace drt
