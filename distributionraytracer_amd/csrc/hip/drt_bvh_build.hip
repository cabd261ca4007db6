// drt_bvh_build.hip — a linear BVH of the resident primitives, built on the device (drt_build_bvh_device).
//
// After Karras 2012, "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees":
//   bvh_prim_bounds   one lane per primitive: its box (bit-identical to the host's GetBoundingBox(),
//                     include/drt_scene.hpp, drt_scene.cpp:18-33) and the scene's centroid bounds
//   bvh_morton        63-bit Morton keys of the centroids, and the histogram of all eight key bytes
//   bvh_sort_*        stable LSD radix sort of (key, scene index), 8-bit digits (the tile of
//                     drt_scan_sort.hpp), passes whose digit is the same for every key skipped
//   bvh_radix_tree    one lane per internal node of the binary radix tree over the sorted keys
//   bvh_refit         one lane per sorted position climbs the parent links: boxes, depths, inner counts
//   bvh_emit          renumbers into the drt_upload_bvh format (children adjacent, index > own index)
// The slices of the scratch and the launch of the stages up to the sort (launch_bvh_sorted) are declared in
// drt_bvh_arena.hpp: the PLOC builder (drt_bvh_ploc.hip) begins with the same stages.
// The tree differs from the host's binned-SAH tree; it is a tree of the same shape rules (leaves of one or
// two objects, children side by side), so the commit path of drt_upload_bvh takes it unchanged.
//
// No lane waits for another lane, wave or workgroup: the stages are ordered by kernel boundaries on one
// stream, the only cross-workgroup traffic inside a kernel is atomic adds / mins / maxes whose results no
// one polls, and bvh_refit's arrival counter lets the first arrival leave.  Workgroup barriers
// (__syncthreads) order the LDS staging of one workgroup.  The scans, the wave reduction and the sort tile are
// drt_scan_sort.hpp's, shared with drt_bvh_commit.hip and drt_grid_build.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../../include/drt.h"
#include "drt_bvh_arena.hpp"
#include "drt_bvh_build.hpp"
#include "drt_prim_device.hpp"
#include "drt_scan_sort.hpp"

namespace drt {

BvhArena carve_bvh(void* scratch, uint32_t n, size_t* total) {
  const size_t nwg = div_up(n, kBvhSortTile);
  const size_t ids = 2 * (size_t)n;  // 2n - 1 used
  ScratchSlicer s{scratch};
  BvhArena a;
  a.pbox = s.take<float4>(2 * (size_t)n);
  a.key[0] = s.take<uint64_t>(n);
  a.key[1] = s.take<uint64_t>(n);
  a.pay[0] = s.take<uint32_t>(n);
  a.pay[1] = s.take<uint32_t>(n);
  a.table = s.take<uint32_t>(256 * nwg);
  a.ghist = s.take<uint32_t>(8 * 256);
  a.plan = s.take<SortPlan>(1);
  a.cbounds = s.take<uint32_t>(8);
  a.left = s.take<uint32_t>(n);
  a.right = s.take<uint32_t>(n);
  a.first = s.take<uint32_t>(n);
  a.last = s.take<uint32_t>(n);
  a.parent = s.take<uint32_t>(ids);
  a.arrive = s.take<uint32_t>(n);
  a.ndata = s.take<uint32_t>(kNodeWords * ids);
  if (total) *total = s.used;
  return a;
}

namespace {

// ---- stage 0: clear ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void bvh_clear(BvhArena A, uint32_t n, uint32_t* info) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < 2 * n - 1) A.parent[i] = kNone;
  if (i < n) A.arrive[i] = 0u;
  if (i < 8 * 256) A.ghist[i] = 0u;
  if (i < 3) A.cbounds[i] = 0xFFFFFFFFu;      // min: above every float
  if (i >= 3 && i < 6) A.cbounds[i] = 0u;     // max: below every float
  if (i < 4) info[i] = 0u;
}

// ---- stage 1: primitive boxes, centroid bounds ---------------------------------------------------
// AABB::centroid() (include/drt_scene.hpp): (min + max) / 2.0f per axis
__device__ inline float centroid1(float lo, float hi) { return (lo + hi) / 2.0f; }

__global__ __launch_bounds__(kThreads) void bvh_prim_bounds(const drt_prim* __restrict__ prims, uint32_t n, BvhArena A) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
  const bool valid = i < n;
  if (valid) {
    const drt_prim p = prims[i];
    prim_bounds(p, lo, hi);
    A.pbox[2 * (size_t)i] = make_float4(lo[0], lo[1], lo[2], 0.f);
    A.pbox[2 * (size_t)i + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
  }
  // centroid bounds: across the wave with cross-lane shuffles, then one atomic per wave and axis.
  // Non-finite centroids take no part (bvh_morton clamps them).
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float c = centroid1(lo[a], hi[a]);
    const bool use = valid && finite(c);
    uint32_t mn = use ? ordered(c) : 0xFFFFFFFFu, mx = use ? ordered(c) : 0u;
    wave_min_max(mn, mx);
    if ((threadIdx.x & 63) == 0 && mn <= mx) {
      atomicMin(&A.cbounds[a], mn);
      atomicMax(&A.cbounds[3 + a], mx);
    }
  }
}

// ---- stage 2: Morton keys ------------------------------------------------------------------------
// 21 bits -> every third bit of a 63-bit word
__device__ inline uint64_t spread21(uint32_t v) {
  uint64_t x = v & 0x1FFFFFu;
  x = (x | (x << 32)) & 0x001F00000000FFFFull;
  x = (x | (x << 16)) & 0x001F0000FF0000FFull;
  x = (x | (x << 8)) & 0x100F00F00F00F00Full;
  x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}

// the centroid's cell on one axis, 0 .. 2^21 - 1: zero extent (or no finite centroid at all) -> 0 without
// a division; NaN -> 0; values outside the bounds (infinities) clamp
__device__ inline uint32_t quant21(float c, uint32_t omin, uint32_t omax) {
  if (!(omin < omax)) return 0u;
  const float lo = unordered(omin), ext = unordered(omax) - lo;
  if (!(ext > 0.f)) return 0u;
  const float x = ((c - lo) / ext) * 2097152.0f;
  if (!(x >= 0.f)) return 0u;
  return x >= 2097151.0f ? 2097151u : (uint32_t)x;
}

__global__ __launch_bounds__(kThreads) void bvh_morton(uint32_t n, BvhArena A) {
  __shared__ uint32_t h[8 * 256];
  for (int k = threadIdx.x; k < 8 * 256; k += kThreads) h[k] = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) {
    const float4 lo = A.pbox[2 * (size_t)i], hi = A.pbox[2 * (size_t)i + 1];
    const uint32_t qx = quant21(centroid1(lo.x, hi.x), A.cbounds[0], A.cbounds[3]);
    const uint32_t qy = quant21(centroid1(lo.y, hi.y), A.cbounds[1], A.cbounds[4]);
    const uint32_t qz = quant21(centroid1(lo.z, hi.z), A.cbounds[2], A.cbounds[5]);
    const uint64_t key = (spread21(qx) << 2) | (spread21(qy) << 1) | spread21(qz);
    A.key[0][i] = key;
    A.pay[0][i] = i;
#pragma unroll
    for (int p = 0; p < 8; p++) atomicAdd(&h[p * 256 + (uint32_t)((key >> (8 * p)) & 255u)], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 8 * 256; k += kThreads)
    if (h[k]) atomicAdd(&A.ghist[k], h[k]);
}

// ---- stage 3: stable LSD radix sort (why it is stable: radix_scatter_tile, drt_scan_sort.hpp) ------
// One workgroup: which passes run, which buffer each reads, and each pass's digit bases.
__global__ __launch_bounds__(kThreads) void bvh_sort_plan(uint32_t n, BvhArena A) {
  __shared__ uint32_t wave_tot[4];
  __shared__ uint32_t skip[8];
  const int t = threadIdx.x;
  if (t < 8) skip[t] = 0u;
  __syncthreads();
  for (int p = 0; p < 8; p++) {
    const uint32_t v = A.ghist[p * 256 + t];
    if (v == n) skip[p] = 1u;  // one digit holds every key
    uint32_t total;
    A.plan->gbase[p][t] = block_scan_excl<uint32_t>(v, wave_tot, total);
  }
  __syncthreads();
  if (t == 0) {
    uint32_t sel = 0u;
    for (int p = 0; p < 8; p++) {
      A.plan->skip[p] = skip[p];
      A.plan->src[p] = sel;
      if (!skip[p]) sel ^= 1u;
    }
    A.plan->final_sel = sel;
  }
}

// per-workgroup digit histogram of the tile -> table[digit * n_wg + wg]
__global__ __launch_bounds__(kThreads) void bvh_sort_count(uint32_t n, uint32_t n_wg, int pass, BvhArena A) {
  if (A.plan->skip[pass]) return;
  radix_count_tile<uint64_t>(A.key[A.plan->src[pass]], n, n_wg, pass, A.table);
}

// one workgroup per digit: exclusive scan of the digit's row of n_wg counts, offset by the digit's base
__global__ __launch_bounds__(kThreads) void bvh_sort_scan(uint32_t n_wg, int pass, BvhArena A) {
  if (A.plan->skip[pass]) return;
  (void)block_scan_array<uint32_t>(A.table + (size_t)blockIdx.x * n_wg, n_wg, A.plan->gbase[pass][blockIdx.x]);
}

// the tile's keys and payloads, ranked by digit, from the pass's source buffer to the other one
__global__ __launch_bounds__(kThreads) void bvh_sort_scatter(uint32_t n, uint32_t n_wg, int pass, BvhArena A) {
  if (A.plan->skip[pass]) return;
  const uint32_t sel = A.plan->src[pass];
  radix_scatter_tile<uint64_t>(A.key[sel], A.pay[sel], A.key[sel ^ 1u], A.pay[sel ^ 1u], n, n_wg, pass, A.table);
}

// ---- stage 4: binary radix tree ------------------------------------------------------------------
// length of the common prefix of the keys at sorted positions i and j; the position breaks ties, so every
// (key, position) pair is distinct and the depth is at most 63 + ceil(log2 n)
__device__ inline int delta(const uint64_t* __restrict__ k, uint64_t ki, int64_t i, int64_t j, int64_t n) {
  if (j < 0 || j >= n) return -1;
  const uint64_t x = ki ^ k[j];
  return x ? __clzll((long long)x) : 64 + __clz((int)((uint32_t)i ^ (uint32_t)j));
}

__global__ __launch_bounds__(kThreads) void bvh_radix_tree(uint32_t n_u, BvhArena A) {
  const int64_t n = n_u, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n - 1) return;
  const uint64_t* __restrict__ k = A.key[A.plan->final_sel];
  const uint64_t ki = k[i];
  const int d = delta(k, ki, i, i + 1, n) > delta(k, ki, i, i - 1, n) ? 1 : -1;
  const int dmin = delta(k, ki, i, i - d, n);
  int64_t lmax = 2;
  while (delta(k, ki, i, i + lmax * d, n) > dmin) lmax <<= 1;
  int64_t l = 0;
  for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
    if (delta(k, ki, i, i + (l + t) * d, n) > dmin) l += t;
  const int64_t j = i + l * d;
  const int dnode = delta(k, ki, i, j, n);
  int64_t s = 0;
  for (int64_t t = (l + 1) >> 1;; t = (t + 1) >> 1) {
    if (delta(k, ki, i, i + (s + t) * d, n) > dnode) s += t;
    if (t <= 1) break;
  }
  const int64_t g = i + s * d + (d < 0 ? -1 : 0);
  const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
  const uint32_t lc = lo == g ? (uint32_t)(n - 1 + g) : (uint32_t)g;
  const uint32_t rc = hi == g + 1 ? (uint32_t)(n - 1 + g + 1) : (uint32_t)(g + 1);
  A.left[i] = lc;
  A.right[i] = rc;
  A.first[i] = (uint32_t)lo;
  A.last[i] = (uint32_t)hi;
  A.parent[lc] = (uint32_t)i;
  A.parent[rc] = (uint32_t)i;
}

// ---- stage 5: refit ------------------------------------------------------------------------------
// Node data cross XCDs: the MI355X has one L2 per XCD, and the two children of a node may have been
// written by workgroups on different XCDs.  They are written with device-scope stores before a
// device-scope release fence, the arrival counter is a device-scope atomic, and the second arrival reads
// them, after an acquire fence, with the device-scope atomic loads of node_load (global_load ... sc1, which
// do not take a line from this XCD's L2 that another XCD has since rewritten).
__device__ inline void node_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline uint32_t node_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void bvh_refit(uint32_t n, BvhArena A) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;  // a sorted position
  if (j >= n) return;
  const uint32_t* __restrict__ pay = A.pay[A.plan->final_sel];
  uint32_t cur = n - 1 + j;
  const uint32_t p0 = A.parent[cur];
  float lo[3], hi[3];
  {
    const uint32_t o = pay[j];
    const float4 a = A.pbox[2 * (size_t)o], b = A.pbox[2 * (size_t)o + 1];
    lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
  }
  if (p0 != kNone && A.last[p0] - A.first[p0] == 1u) {
    // a node of two primitives is a leaf (the reference's n_objects <= 2): its first position builds it
    if (j != A.first[p0]) return;
    const uint32_t o = pay[j + 1];
    const float4 a = A.pbox[2 * (size_t)o], b = A.pbox[2 * (size_t)o + 1];
    lo[0] = smin(lo[0], a.x); lo[1] = smin(lo[1], a.y); lo[2] = smin(lo[2], a.z);
    hi[0] = smax(hi[0], b.x); hi[1] = smax(hi[1], b.y); hi[2] = smax(hi[2], b.z);
    cur = p0;
  }
  uint32_t depth = 1u, inner = 0u;
  // at most 63 + ceil(log2 n) < 96 levels; the bound also ends the loop on a malformed parent chain
  for (int level = 0; level < 128; level++) {
    uint32_t* nd = A.ndata + (size_t)cur * kNodeWords;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      node_store(nd + a, __float_as_uint(lo[a]));
      node_store(nd + 3 + a, __float_as_uint(hi[a]));
    }
    node_store(nd + 6, depth);
    node_store(nd + 7, inner);
    const uint32_t par = A.parent[cur];
    if (par == kNone) return;  // the root
    __threadfence();  // release: this node's data before the arrival
    const uint32_t old = __hip_atomic_fetch_add(&A.arrive[par], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == 0u) return;  // the first arrival leaves; the second one continues
    __threadfence();  // acquire: the sibling's data after the arrival
    const uint32_t* l = A.ndata + (size_t)A.left[par] * kNodeWords;
    const uint32_t* r = A.ndata + (size_t)A.right[par] * kNodeWords;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      lo[a] = smin(__uint_as_float(node_load(l + a)), __uint_as_float(node_load(r + a)));
      hi[a] = smax(__uint_as_float(node_load(l + 3 + a)), __uint_as_float(node_load(r + 3 + a)));
    }
    const uint32_t dl = node_load(l + 6), dr = node_load(r + 6);
    depth = 1u + (dl > dr ? dl : dr);
    inner = 1u + node_load(l + 7) + node_load(r + 7);
    cur = par;
  }
}

// ---- stage 6: emit -------------------------------------------------------------------------------
// An inner node of preorder rank r among the inner nodes keeps its children at 1 + 2r and 2 + 2r (the root
// at 0).  rank(x) = rank(parent) + 1 + (x is the right child ? inner count of the left sibling : 0), summed
// on a walk to the root: no lane needs another lane's result.
__global__ __launch_bounds__(kThreads) void bvh_emit(uint32_t n, BvhArena A, drt_bvh_node* __restrict__ nodes,
                                                     uint32_t* __restrict__ order, uint32_t* __restrict__ info) {
  const uint32_t id = blockIdx.x * kThreads + threadIdx.x;
  if (id < n) order[id] = A.pay[A.plan->final_sel][id];
  if (id >= 2 * n - 1) return;
  const bool prim = id >= n - 1;  // a sorted position (else an internal node of the radix tree)
  const uint32_t par = A.parent[id];
  uint32_t first, count;
  if (prim) {
    if (par != kNone && A.last[par] - A.first[par] == 1u) return;  // folded into its parent's leaf
    first = id - (n - 1);
    count = 1u;
  } else {
    first = A.first[id];
    count = A.last[id] - first + 1u;
  }
  const bool leaf = count <= 2u;
  // rank of the parent among the inner nodes, then this node's slot
  uint32_t slot = 0u, rank_self = 0u;
  if (par != kNone) {
    uint32_t rank_par = 0u;
    uint32_t x = par;
    for (int level = 0; level < 128; level++) {
      const uint32_t px = A.parent[x];
      if (px == kNone) break;
      rank_par += 1u;
      const uint32_t lx = A.left[px];
      if (lx != x) rank_par += A.ndata[(size_t)lx * kNodeWords + 7];
      x = px;
    }
    const uint32_t lp = A.left[par];
    const bool is_right = lp != id;
    slot = 1u + 2u * rank_par + (is_right ? 1u : 0u);
    rank_self = rank_par + 1u + (is_right ? A.ndata[(size_t)lp * kNodeWords + 7] : 0u);
  }
  if (slot >= 2 * n - 1) return;  // (cannot happen on a well-formed tree; keeps the store in bounds)
  const uint32_t* nd = A.ndata + (size_t)id * kNodeWords;
  drt_bvh_node out;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    out.bmin[a] = __uint_as_float(nd[a]);
    out.bmax[a] = __uint_as_float(nd[3 + a]);
  }
  out.leaf = leaf ? 1u : 0u;
  out.index = leaf ? first : 1u + 2u * rank_self;
  out.n_objs = leaf ? count : 0u;
  nodes[slot] = out;
  if (par == kNone) {
    info[0] = 1u + 2u * nd[7];  // nodes
    info[1] = 1u + nd[7];       // leaves
    info[2] = nd[6];            // depth
  }
}

}  // namespace

size_t bvh_build_scratch_bytes(uint32_t n_prims) {
  size_t total = 0;
  (void)carve_bvh(nullptr, n_prims ? n_prims : 1u, &total);
  return total;
}

hipError_t launch_bvh_sorted(const drt_prim* d_prims, uint32_t n, const BvhArena& A, uint32_t* d_info, hipStream_t st) {
  const uint32_t per_prim = div_up(n, kThreads), per_id = div_up(2 * n - 1, kThreads);
  const uint32_t n_wg = div_up(n, kBvhSortTile);
  const uint32_t clear_grid = per_id > 8u ? per_id : 8u;  // also covers the 8 x 256 histogram
  DRT_LAUNCH(bvh_clear, clear_grid, A, n, d_info);
  DRT_LAUNCH(bvh_prim_bounds, per_prim, d_prims, n, A);
  DRT_LAUNCH(bvh_morton, per_prim, n, A);
  DRT_LAUNCH(bvh_sort_plan, 1, n, A);
  for (int pass = 0; pass < 8; pass++) {
    DRT_LAUNCH(bvh_sort_count, n_wg, n, n_wg, pass, A);
    DRT_LAUNCH(bvh_sort_scan, 256, n_wg, pass, A);
    DRT_LAUNCH(bvh_sort_scatter, n_wg, n, n_wg, pass, A);
  }
  return hipSuccess;
}

hipError_t launch_bvh_build(const drt_prim* d_prims, uint32_t n, void* d_scratch, drt_bvh_node* d_nodes,
                            uint32_t* d_order, uint32_t* d_info, hipStream_t st) {
  if (!d_prims || !d_scratch || !d_nodes || !d_order || !d_info || n == 0 || n > (1u << 26)) return hipErrorInvalidValue;
  const BvhArena A = carve_bvh(d_scratch, n, nullptr);
  if (const hipError_t e = launch_bvh_sorted(d_prims, n, A, d_info, st)) return e;
  if (n > 1) DRT_LAUNCH(bvh_radix_tree, div_up(n - 1, kThreads), n, A);
  DRT_LAUNCH(bvh_refit, div_up(n, kThreads), n, A);
  DRT_LAUNCH(bvh_emit, div_up(2 * n - 1, kThreads), n, A, d_nodes, d_order, d_info);
  return hipSuccess;
}

}  // namespace drt
