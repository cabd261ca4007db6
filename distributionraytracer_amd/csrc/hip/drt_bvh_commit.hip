// drt_bvh_commit.hip — commit a device-built tree (drt_bvh_build.hip) on the device: the 64-B inner records
// and their placement, the leaf boxes, the primitive records in tree order, the 4-ary shadow tree.  What the
// host commit of drt_upload_bvh (DRT_NODE_LAYOUT=1, DRT_WIDE_ORDER=2) decides, these kernels decide the same
// way: the same double-precision box surfaces and comparisons, the same collapse, the same quantisation.  A
// record's place in memory is this file's own.
//
// The builder emits sibling pairs side by side: the inner node of preorder rank r has its children in node
// slots 1 + 2r and 2 + 2r, so node x > 0 has its sibling at x ^ 1 (after the root's offset) and its parent at
// rank_slot[(x - 1) / 2].
//
//   commit_index        rank -> node slot, the root's descriptor and box, cleared counters
//   commit_heads        one lane per node: does its record start a 128-B line ("head") or sit second in its
//                       parent's line ("paired": the inner child of larger surface of a head)?  The lane walks
//                       up its chain of larger-surface links; per-workgroup head counts
//   commit_scan         one workgroup: exclusive scan of the per-workgroup counts, the total
//                       (block_scan_array of drt_scan_sort.hpp, whose flag and wave scans the others use)
//   commit_place        a head's line = the exclusive prefix sum of head flags in node-slot order; the head
//                       places itself at 2 * line and its larger inner child at 2 * line + 1
//   commit_records      one lane per record slot: the 64-B record (or zeros for a padding slot), four 16-B
//                       stores; two neighbouring lanes cover one line
//   commit_leaf_prims   one lane per node / primitive: leaf boxes; 48-B records packed from the raw
//                       primitives as pack_prim does, gathered into tree order
//   launch_wide_marks   the 4-ary tree's roots and their record indices (drt_bvh_wide.hpp, shared with the
//                       Grid scene's shadow tree, drt_grid_tree_commit.hip)
//   commit_wide_write   one lane per wide record: collapse again, order, quantise in double, 64-B record
//
// Stages are kernel boundaries on one stream; no lane waits for another.  The frontier kernels size their
// work from a device-side count; the host bounds their number by the tree depth it read after the build.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "drt_bvh_commit.hpp"
#include "drt_bvh_wide.hpp"
#include "drt_prim_device.hpp"
#include "drt_scan_sort.hpp"

namespace drt {

namespace {

struct Arena {
  uint32_t* rank_slot;  // per inner rank: its node slot
  uint32_t* head;       // per node slot: 1 = an inner node whose record starts a line
  uint32_t* pos;        // per node slot (inner): its record slot
  uint32_t* slot_node;  // per record slot: its node slot, kNone for padding
  WideArena w;          // the 4-ary tree's marks, indices, frontiers and counts (drt_bvh_wide.hpp)
};

Arena carve(void* scratch, uint32_t n, size_t* total) {
  const size_t nodes = 2 * (size_t)n, inner = n;  // 2n - 1 and n - 1 used
  ScratchSlicer s{scratch};
  Arena a;
  a.rank_slot = s.take<uint32_t>(inner);
  a.head = s.take<uint32_t>(nodes);
  a.pos = s.take<uint32_t>(nodes);
  a.slot_node = s.take<uint32_t>(2 * inner);
  a.w = carve_wide(s, n);
  if (total) *total = s.used;
  return a;
}

// ---- helpers ---------------------------------------------------------------------------------------
// the inner child of larger surface of the node whose children are l and l + 1 (the left one on a tie),
// kNone if both are leaves
__device__ inline uint32_t larger_child(const drt_bvh_node* __restrict__ nodes, uint32_t l) {
  const bool li = !nodes[l].leaf, ri = !nodes[l + 1].leaf;
  if (li && ri) return surface(nodes, l) >= surface(nodes, l + 1) ? l : l + 1;
  return li ? l : (ri ? l + 1 : kNone);
}


// ---- stage 1: binary records and their placement ---------------------------------------------------
__global__ __launch_bounds__(kThreads) void commit_index(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                         Arena A, BvhCommitStatus* status) {
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t n_inner = (n_nodes - 1) / 2;
  const bool root_inner = !nodes[0].leaf;
  if (s < (uint32_t)kMaxLevels) A.w.level_cnt[s] = (s == 0 && root_inner) ? 1u : 0u;
  if (s == 0) {
    const drt_bvh_node r = nodes[0];
    BvhCommitStatus st{};
    st.flags = root_inner ? 0u : (uint32_t)kCommitLeafRoot;
    st.root_desc = root_inner ? 0u : leaf_desc(r.index, r.n_objs);  // an inner root: the first head, slot 0
    for (int a = 0; a < 3; a++) {
      st.root_box[a] = r.bmin[a];
      st.root_box[3 + a] = r.bmax[a];
    }
    *status = st;
    if (root_inner) A.w.frontier[0][0] = 0u;
  }
  if (s >= n_nodes) return;
  A.w.wmark[s] = (s == 0 && root_inner) ? 1u : 0u;
  const drt_bvh_node& nd = nodes[s];
  if (!nd.leaf) {
    const uint32_t rank = (nd.index - 1u) >> 1;
    if (rank < n_inner) A.rank_slot[rank] = s;
  }
}

__global__ __launch_bounds__(kThreads) void commit_heads(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                         Arena A) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  bool head = false;
  if (s < n_nodes && !nodes[s].leaf) {
    // links of "is its parent's larger-surface inner child" above this node, up to the first node that is not
    // (a head) or the root (a head): an even number of them makes this node a head
    uint32_t x = s, links = 0u;
    for (int level = 0; level < kMaxLevels && x != 0u; level++) {
      const uint32_t l = ((x - 1u) & ~1u) + 1u;  // the left one of x and its sibling
      if (larger_child(nodes, l) != x) break;
      links++;
      x = A.rank_slot[(x - 1u) >> 1];
      if (x >= n_nodes) break;  // (cannot happen on a well-formed tree; keeps the loads in bounds)
    }
    head = (links & 1u) == 0u;
  }
  if (s < n_nodes) A.head[s] = head ? 1u : 0u;
  uint32_t total;
  (void)block_flag_scan(head, wave_tot, total);
  if (threadIdx.x == 0) A.w.wg_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void commit_place(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                         Arena A) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t n_inner = (n_nodes - 1) / 2;
  const bool head = s < n_nodes && A.head[s] != 0u;
  uint32_t total;
  const uint32_t line = A.w.wg_counts[blockIdx.x] + block_flag_scan(head, wave_tot, total);
  if (!head || line >= n_inner) return;
  const uint32_t l = nodes[s].index;
  if (l + 1u >= n_nodes) return;
  const uint32_t a = larger_child(nodes, l);
  A.pos[s] = 2u * line;
  A.slot_node[2u * line] = s;
  A.slot_node[2u * line + 1u] = a;  // kNone: a padding slot
  if (a != kNone) A.pos[a] = 2u * line + 1u;
}

__global__ __launch_bounds__(kThreads) void commit_records(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                           Arena A, const BvhCommitStatus* __restrict__ status,
                                                           float4* __restrict__ recs) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t n_inner = (n_nodes - 1) / 2;
  uint32_t n_slots = 2u * status->n_lines;
  if (n_slots > 2u * n_inner) n_slots = 2u * n_inner;
  if (t >= n_slots) return;
  const uint32_t s = A.slot_node[t];
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a, d = a;
  if (s < n_nodes) {
    const uint32_t l = nodes[s].index;
    if (l + 1u < n_nodes) {
      const drt_bvh_node L = nodes[l], R = nodes[l + 1];
      a = make_float4(L.bmin[0], L.bmin[1], L.bmin[2], L.bmax[0]);
      b = make_float4(L.bmax[1], L.bmax[2], R.bmin[0], R.bmin[1]);
      c = make_float4(R.bmin[2], R.bmax[0], R.bmax[1], R.bmax[2]);
      d = make_float4(__uint_as_float(node_desc(L, A.pos, l)), __uint_as_float(node_desc(R, A.pos, l + 1u)), 0.f, 0.f);
    }
  }
  float4* out = recs + 4 * (size_t)t;
  out[0] = a;
  out[1] = b;
  out[2] = c;
  out[3] = d;
}

// ---- stage 2: leaf boxes, primitive records in tree order ------------------------------------------
__global__ __launch_bounds__(kThreads) void commit_leaf_prims(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                              const uint32_t* __restrict__ order,
                                                              const float4* __restrict__ raw, uint32_t n,
                                                              uint32_t default_material, int leaf_boxes,
                                                              float4* __restrict__ wleaf, float4* __restrict__ prims) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (leaf_boxes) {
    if (i < 2u) {  // the node step's tail slot reads
      wleaf[2 * ((size_t)n + i)] = zero;
      wleaf[2 * ((size_t)n + i) + 1] = zero;
    }
    if (i < n_nodes) {
      const drt_bvh_node nd = nodes[i];
      if (nd.leaf) {
        const float4 lo = make_float4(nd.bmin[0], nd.bmin[1], nd.bmin[2], nd.bmax[0]);
        const float4 hi = make_float4(nd.bmax[1], nd.bmax[2], 0.f, 0.f);
        for (uint32_t k = 0; k < nd.n_objs && nd.index + k < n; k++) {
          wleaf[2 * ((size_t)nd.index + k)] = lo;
          wleaf[2 * ((size_t)nd.index + k) + 1] = hi;
        }
      }
    }
  }
  if (i >= n) return;
  const uint32_t o = order[i];
  if (o >= n) return;
  float4 q0, q1, q2;
  pack_prim_record(raw, o, default_material, q0, q1, q2);
  prims[3 * (size_t)i] = q0;
  prims[3 * (size_t)i + 1] = q1;
  prims[3 * (size_t)i + 2] = q2;
}

// ---- stage 3: the 4-ary shadow tree (drt_bvh_wide.hpp) ---------------------------------------------
__global__ __launch_bounds__(kThreads) void commit_wide_write(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                              Arena A, BvhCommitStatus* status,
                                                              uint4* __restrict__ wide) {
  const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t n_inner = (n_nodes - 1) / 2;
  uint32_t n_wide = status->n_wide;
  if (n_wide > n_inner) n_wide = n_inner;
  if (w >= n_wide) return;
  uint4 s0, s1, s2, s3;
  if (!wide_record(nodes, n_nodes, A.w.wlist[w], A.w.widx, 0.0, s0, s1, s2, s3))
    atomicOr(&status->flags, (uint32_t)kCommitNoQuant);  // the host keeps the binary tree for shadow queries
  uint4* out = wide + 4 * (size_t)w;
  out[0] = s0;
  out[1] = s1;
  out[2] = s2;
  out[3] = s3;
}

}  // namespace

size_t bvh_commit_scratch_bytes(uint32_t n_prims) {
  size_t total = 0;
  (void)carve(nullptr, n_prims ? n_prims : 1u, &total);
  return total;
}

hipError_t launch_bvh_commit(const BvhCommitArgs& a, hipStream_t st) {
  if (!a.nodes || !a.order || !a.prims_raw || !a.scratch || !a.recs || !a.wide_recs || !a.leaf_boxes || !a.prims ||
      !a.status || a.n_prims == 0 || a.n_prims > (1u << 26) || a.n_nodes == 0 || !(a.n_nodes & 1u) ||
      a.n_nodes > 2 * a.n_prims - 1)
    return hipErrorInvalidValue;
  const Arena A = carve(a.scratch, a.n_prims, nullptr);
  const uint32_t n = a.n_prims, n_nodes = a.n_nodes, n_inner = (n_nodes - 1) / 2;
  const uint32_t per_node = (n_nodes + kThreads - 1) / kThreads;
  const uint32_t per_inner = (n_inner + kThreads - 1) / kThreads;
  const uint32_t per_both = ((n_nodes > n ? n_nodes : n) + kThreads - 1) / kThreads;
  const int wide = a.wide && n_inner > 0;
  DRT_LAUNCH(commit_index, per_node, a.nodes, n_nodes, A, a.status);
  if (n_inner > 0) {
    DRT_LAUNCH(commit_heads, per_node, a.nodes, n_nodes, A);
    DRT_LAUNCH(commit_scan, 1, A.w.wg_counts, per_node, &a.status->n_lines);
    DRT_LAUNCH(commit_place, per_node, a.nodes, n_nodes, A);
    DRT_LAUNCH(commit_records, (2 * n_inner + kThreads - 1) / kThreads, a.nodes, n_nodes, A, a.status,
                  (float4*)a.recs);
  }
  DRT_LAUNCH(commit_leaf_prims, per_both, a.nodes, n_nodes, a.order, (const float4*)a.prims_raw, n,
                a.default_material, wide, (float4*)a.leaf_boxes, (float4*)a.prims);
  if (!wide) return hipSuccess;
  const hipError_t e = launch_wide_marks(a.nodes, n_nodes, a.depth, a.max_wide_levels, A.w, &a.status->wide_depth,
                                         &a.status->n_wide, st);
  if (e != hipSuccess) return e;
  DRT_LAUNCH(commit_wide_write, per_inner, a.nodes, n_nodes, A, a.status, (uint4*)a.wide_recs);
  return hipSuccess;
}

}  // namespace drt
