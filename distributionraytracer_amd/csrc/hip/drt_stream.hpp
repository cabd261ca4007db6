// drt_stream.hpp — device pieces the streaming kernels of drt_kernels.hip and drt_cell_tree.hip share.
#pragma once
#include "drt_device.hpp"
#include "drt_kernels.hpp"

namespace drt {

constexpr uint32_t kNoItem = 0xFFFFFFFFu;
constexpr uint32_t kTraceChunk = 256;  // queries claimed per wave per atomic

// LDS traversal-stack entries per thread for a given occupancy target (5 blocks of 256 threads
// fit 16 entries in 160 KiB; 6-8 blocks need a shorter LDS stack, the rest spills to scratch).
__host__ __device__ constexpr int lds_cap(int waves) {
  // per thread: 160 KiB over waves * 4 SIMDs * 64 lanes, 8 B per entry, whatever the block size
  return (160 * 1024 / (waves * 256 * 8) - 1) < 16 ? (160 * 1024 / (waves * 256 * 8) - 1) : 16;
}

__device__ __forceinline__ bool ray_finite(const RayP& r) {
  return inv_finite(r) && fabsf(r.o.x) < __builtin_inff() && fabsf(r.o.y) < __builtin_inff() &&
         fabsf(r.o.z) < __builtin_inff();
}

// Grid::Traverse(Ray&)'s first step (grid.cpp:318-324): a shadow ray whose slab test misses the grid box
// counts as shadowed.  The same float arithmetic as grid_traverse / grid_init.
__device__ __forceinline__ bool grid_box_missed(const SceneArgs& S, const RayP& r) {
  const float x0 = S.gmin[0], y0 = S.gmin[1], z0 = S.gmin[2], x1 = S.gmax[0], y1 = S.gmax[1], z1 = S.gmax[2];
  float txmin, tymin, tzmin, txmax, tymax, tzmax;
  if (r.sx()) { txmin = (x0 - r.o.x) * r.ix; txmax = (x1 - r.o.x) * r.ix; } else { txmin = (x1 - r.o.x) * r.ix; txmax = (x0 - r.o.x) * r.ix; }
  if (r.sy()) { tymin = (y0 - r.o.y) * r.iy; tymax = (y1 - r.o.y) * r.iy; } else { tymin = (y1 - r.o.y) * r.iy; tymax = (y0 - r.o.y) * r.iy; }
  if (r.sz()) { tzmin = (z0 - r.o.z) * r.iz; tzmax = (z1 - r.o.z) * r.iz; } else { tzmin = (z1 - r.o.z) * r.iz; tzmax = (z0 - r.o.z) * r.iz; }
  float t0 = (txmin > tymin) ? txmin : tymin;
  if (tzmin > t0) t0 = tzmin;
  float t1 = (txmax < tymax) ? txmax : tymax;
  if (tzmax < t1) t1 = tzmax;
  return t0 > t1 || t1 < 0.0f;  // grid.cpp:170 (NaN compares false: not missed, as there)
}

}  // namespace drt
