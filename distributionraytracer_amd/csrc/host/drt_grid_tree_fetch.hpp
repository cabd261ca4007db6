// drt_grid_tree_fetch.hpp — what the host scene library (drt_host_capi.cpp) asks of the device half of the
// same shared library without a C entry point: not exported, no part of include/drt.h.
#pragma once
#include <cstdint>

#include "../../../include/drt.h"

namespace drt {

// The binary tree behind the resident device-built shadow tree of a Grid scene (drt_build_grid_device with
// DRT_GRID_SHADOW_LBVH / DRT_GRID_SHADOW_PLOC): its nodes (room for 2 * n_objects - 1) and its object order
// (n_objects), as drt_upload_grid_shadow_bvh takes them.  DRT_E_STATE unless such a tree is resident.
__attribute__((visibility("hidden"))) int fetch_grid_shadow_tree(drt_ctx* ctx, drt_bvh_node* nodes, uint32_t* order,
                                                                 uint32_t* n_nodes);

}  // namespace drt
