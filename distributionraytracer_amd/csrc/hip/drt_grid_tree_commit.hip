// drt_grid_tree_commit.hip — commit a device-built tree (drt_bvh_build.hip, drt_bvh_ploc.hip) as a Grid scene's
// shadow tree on the device: the 4-ary records with grown child boxes, the primitive records in tree order, per
// such primitive its cell range for the certificate.  What drt_upload_grid_shadow_bvh decides on the host for a
// triangle scene, these kernels decide the same way (build_wide with its `widen`, drt_bvh_wide.hpp); a record's
// place in memory is the device commit's own, as in drt_bvh_commit.hip.  The Grid tree has no binary records
// and no leaf boxes: the slot the BVH's tree keeps leaf boxes in holds the cell ranges.
//
//   grid_tree_seed      one lane per node slot: cleared marks and level counts, the root in the frontier; the
//                       status words, with the boxes' growth 2^widen_log2 * M from the root box (M its largest
//                       absolute coordinate, in double as on the host)
//   launch_wide_marks   the 4-ary tree's roots and their record indices (drt_bvh_wide.hpp)
//   grid_tree_prims     one lane per tree-order slot: the 48-B primitive record of order[i] and the 32-B range
//                       record from its six cell indices, whole records per lane; the zero tails of both
//                       arrays; one lane per node slot: a leaf too large for a descriptor raises a status flag
//   grid_tree_write     one lane per 4-ary record: the record of the grown boxes; a record that does not
//                       quantise raises a status flag
//
// Stages are kernel boundaries on one stream; no lane waits for another and nothing is read back here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "drt_bvh_wide.hpp"
#include "drt_grid_tree_commit.hpp"
#include "drt_prim_device.hpp"
#include "drt_scan_sort.hpp"

namespace drt {

namespace {

constexpr uint32_t kPadWords = 4;  // kPrimPadBytes (drt_kernels.hpp) as 16-B words

__global__ __launch_bounds__(kThreads) void grid_tree_seed(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                           WideArena A, int widen_log2, GridTreeStatus* status) {
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  const bool root_inner = !nodes[0].leaf;
  if (s < (uint32_t)kMaxLevels) A.level_cnt[s] = (s == 0 && root_inner) ? 1u : 0u;
  if (s == 0) {
    const drt_bvh_node r = nodes[0];
    double m = 0.0;
    for (int a = 0; a < 3; a++) {
      const double lo = fabs((double)r.bmin[a]), hi = fabs((double)r.bmax[a]);
      const double c = lo < hi ? hi : lo;  // std::max(fabs(min), fabs(max))
      m = m < c ? c : m;
    }
    GridTreeStatus st{};
    st.flags = root_inner ? 0u : (uint32_t)kGridTreeLeafRoot;
    st.widen = ldexp(m, widen_log2);
    *status = st;
    if (root_inner) A.frontier[0][0] = 0u;
  }
  if (s < n_nodes) A.wmark[s] = (s == 0 && root_inner) ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void grid_tree_write(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                            WideArena A, GridTreeStatus* status,
                                                            uint4* __restrict__ wide) {
  const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t n_inner = (n_nodes - 1) / 2;
  uint32_t n_wide = status->n_wide;
  if (n_wide > n_inner) n_wide = n_inner;
  if (w >= n_wide) return;
  uint4 s0, s1, s2, s3;
  if (!wide_record(nodes, n_nodes, A.wlist[w], A.widx, status->widen, s0, s1, s2, s3))
    atomicOr(&status->flags, (uint32_t)kGridTreeNoQuant);
  uint4* out = wide + 4 * (size_t)w;
  out[0] = s0;
  out[1] = s1;
  out[2] = s2;
  out[3] = s3;
}

__global__ __launch_bounds__(kThreads) void grid_tree_prims(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                            GridTreeStatus* status, const uint32_t* __restrict__ order,
                                                            const float4* __restrict__ raw,
                                                            const int2* __restrict__ ranges, uint32_t n,
                                                            uint32_t default_material, int nocert,
                                                            float4* __restrict__ prims, float4* __restrict__ rng) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < kPadWords) prims[3 * (size_t)n + i] = zero;  // the node step's slot reads past the last record
  if (i < 2u) {                                        // ... and past the last range
    rng[2 * ((size_t)n + i)] = zero;
    rng[2 * ((size_t)n + i) + 1] = zero;
  }
  // a leaf of kBigLeaf objects or more has no descriptor of its own (the host keeps a table of them)
  if (i < n_nodes && nodes[i].leaf && nodes[i].n_objs >= kBigLeaf) atomicOr(&status->flags, (uint32_t)kGridTreeBigLeaf);
  if (i >= n) return;
  const uint32_t o = order[i];
  if (o >= n) return;
  float4 q0, q1, q2;
  pack_prim_record(raw, o, default_material, q0, q1, q2);
  prims[3 * (size_t)i] = q0;
  prims[3 * (size_t)i + 1] = q1;
  prims[3 * (size_t)i + 2] = q2;
  // (ix, iy), (iz, jx), (jy, jz): the object's first and last cell per axis
  const int2 a = ranges[3 * (size_t)o], b = ranges[3 * (size_t)o + 1], c = ranges[3 * (size_t)o + 2];
  // listed in no cell (an inverted range): an inverted box, never certified
  const bool none = nocert || b.y < a.x || c.x < a.y || c.y < b.x || b.y < 0;
  rng[2 * (size_t)i] = none ? make_float4(1.f, 1.f, 1.f, 0.f) : make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
  rng[2 * (size_t)i + 1] = none ? zero : make_float4((float)c.x, (float)c.y, 0.f, 0.f);
}

WideArena carve(void* scratch, uint32_t n, size_t* total) {
  ScratchSlicer s{scratch};
  const WideArena a = carve_wide(s, n);
  if (total) *total = s.used;
  return a;
}

}  // namespace

size_t grid_tree_commit_scratch_bytes(uint32_t n_prims) {
  size_t total = 0;
  (void)carve(nullptr, n_prims ? n_prims : 1u, &total);
  return total;
}

hipError_t launch_grid_tree_commit(const GridTreeCommitArgs& a, hipStream_t st) {
  if (!a.nodes || !a.order || !a.prims_raw || !a.ranges || !a.scratch || !a.wide_recs || !a.prims || !a.range_recs ||
      !a.status || a.n_prims == 0 || a.n_prims > (1u << 26) || a.n_nodes == 0 || !(a.n_nodes & 1u) ||
      a.n_nodes > 2 * a.n_prims - 1)
    return hipErrorInvalidValue;
  const WideArena A = carve(a.scratch, a.n_prims, nullptr);
  const uint32_t n = a.n_prims, n_nodes = a.n_nodes, n_inner = (n_nodes - 1) / 2;
  DRT_LAUNCH(grid_tree_seed, div_up(n_nodes, kThreads), a.nodes, n_nodes, A, a.widen_log2, a.status);
  const uint32_t slots = n_nodes > n ? n_nodes : (n > kPadWords ? n : kPadWords);  // nodes, primitives, pad words
  DRT_LAUNCH(grid_tree_prims, div_up(slots, kThreads), a.nodes, n_nodes, a.status, a.order, (const float4*)a.prims_raw,
             (const int2*)a.ranges, n, a.default_material, a.nocert, (float4*)a.prims, (float4*)a.range_recs);
  if (n_inner == 0) return hipSuccess;  // a leaf root: the status says so
  const hipError_t e = launch_wide_marks(a.nodes, n_nodes, a.depth, a.max_wide_levels, A, &a.status->wide_depth,
                                         &a.status->n_wide, st);
  if (e != hipSuccess) return e;
  DRT_LAUNCH(grid_tree_write, div_up(n_inner, kThreads), a.nodes, n_nodes, A, a.status, (uint4*)a.wide_recs);
  return hipSuccess;
}

}  // namespace drt
