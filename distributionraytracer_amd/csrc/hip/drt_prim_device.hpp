// drt_prim_device.hpp — what the device builders (drt_bvh_build.hip, drt_grid_build.hip) and the device
// commits (drt_bvh_commit.hip, drt_grid_build.hip) derive from a scene-order drt_prim: its box, bit-identical
// to the host's GetBoundingBox(), the order-preserving words its bounds are reduced in, and its 48-B primitive
// record, as pack_prim (drt_capi.hip) packs it.  What they share that does not know a primitive (scans, the
// sort tile, launch and scratch plumbing) is in drt_scan_sort.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../../include/drt.h"

namespace drt {

// GetBoundingBox() (include/drt_scene.hpp, drt_scene.cpp:18-33) of one primitive
__device__ inline void prim_bounds(const drt_prim& p, float lo[3], float hi[3]) {
  if (p.type == DRT_PRIM_TRIANGLE) {  // Triangle::Triangle, drt_scene.cpp:18-33
#pragma unroll
    for (int a = 0; a < 3; a++) {
      float mn = 3.402823466e+38f, mx = -3.402823466e+38f;
      const float v[3] = {p.a[a], p.b[a], p.c[a]};
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if (v[k] < mn) mn = v[k];
        if (v[k] > mx) mx = v[k];
      }
      lo[a] = mn - 0.001f;
      hi[a] = mx + 0.001f;
    }
  } else if (p.type == DRT_PRIM_SPHERE) {
#pragma unroll
    for (int a = 0; a < 3; a++) { lo[a] = p.a[a] - p.r; hi[a] = p.a[a] + p.r; }
  } else if (p.type == DRT_PRIM_BOX) {
#pragma unroll
    for (int a = 0; a < 3; a++) { lo[a] = p.a[a]; hi[a] = p.b[a]; }
  } else {  // a plane keeps the default box (scene.h:116)
#pragma unroll
    for (int a = 0; a < 3; a++) { lo[a] = -1.f; hi[a] = 1.f; }
  }
}

// float -> unsigned whose order is the float's (negative floats below positive ones)
__device__ inline uint32_t ordered(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ inline float unordered(uint32_t o) {
  return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
__device__ inline bool finite(float f) { return (__float_as_uint(f) & 0x7F800000u) != 0x7F800000u; }

// The 48-B record of scene-order primitive o, read from the drt_prim array as three 16-B words:
// (type, material, a.x, a.y), (a.z, b.x, b.y, b.z), (c.x, c.y, c.z, r).
__device__ inline void pack_prim_record(const float4* __restrict__ raw, uint32_t o, uint32_t default_material,
                                        float4& q0, float4& q1, float4& q2) {
  const float4 w0 = raw[3 * (size_t)o], w1 = raw[3 * (size_t)o + 1], w2 = raw[3 * (size_t)o + 2];
  const uint32_t type = __float_as_uint(w0.x);
  const int32_t material = (int32_t)__float_as_uint(w0.y);
  const uint32_t mat = material < 0 ? default_material : (uint32_t)material;
  const float ax = w0.z, ay = w0.w, az = w1.x;
  q0 = make_float4(ax, ay, az, __uint_as_float((type & 3u) | (mat << 2)));
  q1 = make_float4(0.f, 0.f, 0.f, __uint_as_float(o));
  q2 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (type == (uint32_t)DRT_PRIM_TRIANGLE) {  // the edges, as pack_prim subtracts them
    q1.x = w1.y - ax; q1.y = w1.z - ay; q1.z = w1.w - az;
    q2.x = w2.x - ax; q2.y = w2.y - ay; q2.z = w2.z - az;
  } else if (type == (uint32_t)DRT_PRIM_SPHERE || type == (uint32_t)DRT_PRIM_PLANE) {
    q1.x = w2.w;
  } else {
    q1.x = w1.y; q1.y = w1.z; q1.z = w1.w;
  }
}

}  // namespace drt
