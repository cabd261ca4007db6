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
//   commit_wide_level   once per level of the 4-ary tree: a lane per wide root of the frontier collapses its
//                       node and appends the inner children to the next frontier, one atomic per wave
//   commit_wide_count / commit_scan / commit_wide_place
//                       a wide root's record index = the exclusive prefix sum of the marks in node-slot order
//                       (only the set of marks depends on arrival order, the placement does not)
//   commit_wide_write   one lane per wide record: collapse again, order, quantise in double, 64-B record
//
// Stages are kernel boundaries on one stream; no lane waits for another.  The frontier kernels size their
// work from a device-side count; the host bounds their number by the tree depth it read after the build.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "drt_bvh_commit.hpp"
#include "drt_prim_device.hpp"
#include "drt_scan_sort.hpp"

namespace drt {

namespace {

constexpr int kMaxLevels = 128;         // level counters (the host launches far fewer levels)
constexpr uint32_t kLevelGridMax = 1024;  // workgroups of a frontier launch (grid-stride beyond)

struct Arena {
  uint32_t* rank_slot;  // per inner rank: its node slot
  uint32_t* head;       // per node slot: 1 = an inner node whose record starts a line
  uint32_t* pos;        // per node slot (inner): its record slot
  uint32_t* slot_node;  // per record slot: its node slot, kNone for padding
  uint32_t* wmark;      // per node slot: 1 = root of a 4-ary node
  uint32_t* widx;       // per node slot (wide root): its 4-ary record index
  uint32_t* wlist;      // per 4-ary record: its node slot
  uint32_t* frontier[2];
  uint32_t* wg_counts;  // per workgroup of a node-slot launch
  uint32_t* level_cnt;  // kMaxLevels frontier sizes
};

Arena carve(void* scratch, uint32_t n, size_t* total) {
  const size_t nodes = 2 * (size_t)n, inner = n;  // 2n - 1 and n - 1 used
  ScratchSlicer s{scratch};
  Arena a;
  a.rank_slot = s.take<uint32_t>(inner);
  a.head = s.take<uint32_t>(nodes);
  a.pos = s.take<uint32_t>(nodes);
  a.slot_node = s.take<uint32_t>(2 * inner);
  a.wmark = s.take<uint32_t>(nodes);
  a.widx = s.take<uint32_t>(nodes);
  a.wlist = s.take<uint32_t>(inner);
  a.frontier[0] = s.take<uint32_t>(inner);
  a.frontier[1] = s.take<uint32_t>(inner);
  a.wg_counts = s.take<uint32_t>((nodes + kThreads - 1) / kThreads + 1);
  a.level_cnt = s.take<uint32_t>(kMaxLevels);
  if (total) *total = s.used;
  return a;
}

// ---- helpers ---------------------------------------------------------------------------------------
// box surface as drt_upload_bvh's area(): double, x*y + y*z + z*x, unfused
__device__ inline double surface(const drt_bvh_node* __restrict__ nodes, uint32_t i) {
  const drt_bvh_node& nd = nodes[i];
  const double x = (double)nd.bmax[0] - nd.bmin[0], y = (double)nd.bmax[1] - nd.bmin[1],
               z = (double)nd.bmax[2] - nd.bmin[2];
  return x * y + y * z + z * x;
}

// the inner child of larger surface of the node whose children are l and l + 1 (the left one on a tie),
// kNone if both are leaves
__device__ inline uint32_t larger_child(const drt_bvh_node* __restrict__ nodes, uint32_t l) {
  const bool li = !nodes[l].leaf, ri = !nodes[l + 1].leaf;
  if (li && ri) return surface(nodes, l) >= surface(nodes, l + 1) ? l : l + 1;
  return li ? l : (ri ? l + 1 : kNone);
}

__device__ inline uint32_t node_desc(const drt_bvh_node& nd, const uint32_t* __restrict__ inner_index, uint32_t i) {
  return nd.leaf ? leaf_desc(nd.index, nd.n_objs) : inner_index[i];
}

// ---- stage 1: binary records and their placement ---------------------------------------------------
__global__ __launch_bounds__(kThreads) void commit_index(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                         Arena A, BvhCommitStatus* status) {
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t n_inner = (n_nodes - 1) / 2;
  const bool root_inner = !nodes[0].leaf;
  if (s < (uint32_t)kMaxLevels) A.level_cnt[s] = (s == 0 && root_inner) ? 1u : 0u;
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
    if (root_inner) A.frontier[0][0] = 0u;
  }
  if (s >= n_nodes) return;
  A.wmark[s] = (s == 0 && root_inner) ? 1u : 0u;
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
  if (threadIdx.x == 0) A.wg_counts[blockIdx.x] = total;
}

// One workgroup: counts[0 .. n) -> their exclusive scan in place, the total to *total_out.
__global__ __launch_bounds__(kThreads) void commit_scan(uint32_t* counts, uint32_t n, uint32_t* total_out) {
  const uint32_t total = block_scan_array<uint32_t>(counts, n, 0u);
  if (threadIdx.x == 0) *total_out = total;
}

__global__ __launch_bounds__(kThreads) void commit_place(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                         Arena A) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t n_inner = (n_nodes - 1) / 2;
  const bool head = s < n_nodes && A.head[s] != 0u;
  uint32_t total;
  const uint32_t line = A.wg_counts[blockIdx.x] + block_flag_scan(head, wave_tot, total);
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

// ---- stage 3: the 4-ary shadow tree ----------------------------------------------------------------
// build_wide's collapse at its defaults: the two children of node s, the inner one of largest surface
// replaced by its two until there are four or only leaves; then ascending surface, stable.
struct Collapse {
  uint32_t ch[4];
  double area[4];
  bool leaf[4];
  int n;
};

__device__ inline void collapse_set(Collapse& C, int k, const drt_bvh_node* __restrict__ nodes, uint32_t c) {
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (j == k) {
      C.ch[j] = c;
      C.leaf[j] = nodes[c].leaf != 0u;
      C.area[j] = surface(nodes, c);
    }
}

__device__ inline void collapse(Collapse& C, const drt_bvh_node* __restrict__ nodes, uint32_t s, uint32_t n_nodes) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    C.ch[j] = 0u;
    C.area[j] = 0.0;
    C.leaf[j] = true;
  }
  const uint32_t l = nodes[s].index;
  C.n = 0;
  if (l + 1u >= n_nodes) return;
  collapse_set(C, 0, nodes, l);
  collapse_set(C, 1, nodes, l + 1u);
  C.n = 2;
#pragma unroll
  for (int round = 0; round < 2; round++) {
    int best = -1;
    double ba = -1.0;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < C.n && !C.leaf[k] && C.area[k] > ba) {
        ba = C.area[k];
        best = k;
      }
    if (best < 0) break;
    uint32_t c = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k == best) c = C.ch[k];
    const uint32_t cl = nodes[c].index;
    if (cl + 1u >= n_nodes) break;
    collapse_set(C, best, nodes, cl);
    collapse_set(C, C.n, nodes, cl + 1u);
    C.n++;
  }
}

// stable insertion sort by ascending surface (std::stable_sort's result for this comparison)
__device__ inline void collapse_sort(Collapse& C) {
#pragma unroll
  for (int i = 1; i < 4; i++) {
#pragma unroll
    for (int j = i; j > 0; j--) {
      if (i < C.n && C.area[j] < C.area[j - 1]) {
        const uint32_t c = C.ch[j]; C.ch[j] = C.ch[j - 1]; C.ch[j - 1] = c;
        const double a = C.area[j]; C.area[j] = C.area[j - 1]; C.area[j - 1] = a;
        const bool f = C.leaf[j]; C.leaf[j] = C.leaf[j - 1]; C.leaf[j - 1] = f;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void commit_wide_level(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                              Arena A, int level, BvhCommitStatus* status) {
  const uint32_t cnt = A.level_cnt[level];
  const uint32_t n_inner = (n_nodes - 1) / 2;
  const uint32_t* __restrict__ in = A.frontier[level & 1];
  uint32_t* __restrict__ out = A.frontier[(level + 1) & 1];
  const int lane = threadIdx.x & 63;
  if (cnt && blockIdx.x == 0 && threadIdx.x == 0) status->wide_depth = (uint32_t)level + 1u;
  // the trip count is the same for every lane of a workgroup
  for (uint32_t base = blockIdx.x * kThreads; base < cnt && base < n_inner; base += gridDim.x * kThreads) {
    const uint32_t i = base + threadIdx.x;
    Collapse C;
    C.n = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      C.ch[j] = 0u;
      C.leaf[j] = true;
    }
    if (i < cnt && i < n_inner) {
      const uint32_t s = in[i];
      if (s < n_nodes) collapse(C, nodes, s, n_nodes);
    }
    uint32_t mine = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) mine += (k < C.n && !C.leaf[k]) ? 1u : 0u;
    // one atomic per wave: the wave's inner children take a contiguous run of the next frontier
    const uint32_t inc = wave_scan_incl(mine);
    const uint32_t wave_total = __shfl(inc, 63, 64);
    uint32_t run = 0u;
    if (lane == 63 && wave_total) run = atomicAdd(&A.level_cnt[level + 1], wave_total);
    run = __shfl(run, 63, 64);
    uint32_t at = run + inc - mine;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < C.n && !C.leaf[k]) {
        if (at < n_inner) out[at] = C.ch[k];
        at++;
        A.wmark[C.ch[k]] = 1u;
      }
  }
}

__global__ __launch_bounds__(kThreads) void commit_wide_count(uint32_t n_nodes, Arena A) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  uint32_t total;
  (void)block_flag_scan(s < n_nodes && A.wmark[s] != 0u, wave_tot, total);
  if (threadIdx.x == 0) A.wg_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void commit_wide_place(uint32_t n_nodes, Arena A) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t n_inner = (n_nodes - 1) / 2;
  const bool mark = s < n_nodes && A.wmark[s] != 0u;
  uint32_t total;
  const uint32_t w = A.wg_counts[blockIdx.x] + block_flag_scan(mark, wave_tot, total);
  if (!mark || w >= n_inner) return;
  A.widx[s] = w;
  A.wlist[w] = s;
}

// quantize_axis of drt_capi.hip for four children, in the same double arithmetic.  A function of its own (not
// inlined three times into the record kernel), its results by value.
struct AxisPlanes {
  float p;
  uint32_t ebits, qlo, qhi;
  bool ok;
};

__device__ __noinline__ AxisPlanes quantize_axis(double l0, double l1, double l2, double l3, double h0, double h1,
                                                 double h2, double h3, int n) {
  const double lo[4] = {l0, l1, l2, l3}, hi[4] = {h0, h1, h2, h3};
  AxisPlanes R;
  R.p = 0.f;
  R.ebits = R.qlo = R.qhi = 0u;
  R.ok = false;
  double nlo = lo[0], nhi = hi[0];
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (k < n) {
      nlo = lo[k] < nlo ? lo[k] : nlo;  // std::min / std::max
      nhi = nhi < hi[k] ? hi[k] : nhi;
    }
  if (!isfinite(nlo) || !isfinite(nhi) || nhi < nlo) return R;
  if (fabs(nlo) > 0x1p59 || fabs(nhi) > 0x1p59) return R;
  int e0 = -126;
  if (nhi > nlo) {
    const int e = ilogb((nhi - nlo) / 255.0) - 1;
    e0 = e > -126 ? e : -126;
  }
  for (int E = e0; E <= 120; E++) {
    const double s = ldexp(1.0, E);
    const double k0 = floor(nlo / s);
    if (fabs(k0) + 256.0 >= 16777216.0) continue;
    const float pf = (float)(k0 * s), sf = (float)s;
    if ((double)pf != k0 * s) continue;
    if (E > 50) return R;
    uint32_t L = 0u, H = 0u;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (k >= n) {  // unused slot: an inverted box
        L |= 255u << (8 * k);
      } else {
        const double ql = floor(lo[k] / s) - k0, qh = ceil(hi[k] / s) - k0;
        const bool in = ql >= 0.0 && qh <= 255.0;
        // the device decodes with one FMA; every value here is exact, so check it as the device does
        const float dl = fmaf((float)ql, sf, pf), dh = fmaf((float)qh, sf, pf);
        const bool covers = (double)dl <= lo[k] && (double)dh >= hi[k] && isfinite(dl) && isfinite(dh);
        ok = ok && in && covers;
        if (in) {
          L |= (uint32_t)ql << (8 * k);
          H |= (uint32_t)qh << (8 * k);
        }
      }
    }
    if (!ok) continue;
    R.p = pf;
    R.ebits = (uint32_t)(E + 127);
    R.qlo = L;
    R.qhi = H;
    R.ok = true;
    return R;
  }
  return R;
}

__global__ __launch_bounds__(kThreads) void commit_wide_write(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes,
                                                              Arena A, BvhCommitStatus* status,
                                                              uint4* __restrict__ wide) {
  const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t n_inner = (n_nodes - 1) / 2;
  uint32_t n_wide = status->n_wide;
  if (n_wide > n_inner) n_wide = n_inner;
  if (w >= n_wide) return;
  const uint32_t s = A.wlist[w];
  uint4 s0 = make_uint4(0u, 0u, 0u, 0u), s1 = s0, s2 = s0, s3 = s0;
  bool ok = s < n_nodes;
  if (ok) {
    Collapse C;
    collapse(C, nodes, s, n_nodes);
    collapse_sort(C);
    float p[3] = {0.f, 0.f, 0.f};
    uint32_t q[6] = {0u, 0u, 0u, 0u, 0u, 0u}, ebits = 0u;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      double lo[4] = {0.0, 0.0, 0.0, 0.0}, hi[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (k < C.n) {
          lo[k] = (double)nodes[C.ch[k]].bmin[a];
          hi[k] = (double)nodes[C.ch[k]].bmax[a];
        }
      const AxisPlanes R = quantize_axis(lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3], C.n);
      ok = ok && R.ok;
      p[a] = R.p;
      q[2 * a] = R.qlo;
      q[2 * a + 1] = R.qhi;
      ebits |= R.ebits << (8 * a);
    }
    uint32_t desc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < C.n) desc[k] = node_desc(nodes[C.ch[k]], A.widx, C.ch[k]);
    if (ok && C.n >= 2) {
      s0 = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]), ebits);
      s1 = make_uint4(q[0], q[1], q[2], q[3]);
      s2 = make_uint4(q[4], q[5], 0u, 0u);
      s3 = make_uint4(desc[0], desc[1], desc[2], desc[3]);
    } else {
      ok = false;
    }
  }
  if (!ok) atomicOr(&status->flags, (uint32_t)kCommitNoQuant);  // the host keeps the binary tree for shadow queries
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
    DRT_LAUNCH(commit_scan, 1, A.wg_counts, per_node, &a.status->n_lines);
    DRT_LAUNCH(commit_place, per_node, a.nodes, n_nodes, A);
    DRT_LAUNCH(commit_records, (2 * n_inner + kThreads - 1) / kThreads, a.nodes, n_nodes, A, a.status,
                  (float4*)a.recs);
  }
  DRT_LAUNCH(commit_leaf_prims, per_both, a.nodes, n_nodes, a.order, (const float4*)a.prims_raw, n,
                a.default_material, wide, (float4*)a.leaf_boxes, (float4*)a.prims);
  if (!wide) return hipSuccess;
  // wide roots sit above the leaves, so there are at most depth - 1 levels of them
  int levels = (int)a.depth - 1;
  if (levels > a.max_wide_levels) levels = a.max_wide_levels;
  if (levels > kMaxLevels - 1) levels = kMaxLevels - 1;
  const uint32_t level_grid = per_inner < kLevelGridMax ? per_inner : kLevelGridMax;
  for (int level = 0; level < levels; level++)
    DRT_LAUNCH(commit_wide_level, level_grid, a.nodes, n_nodes, A, level, a.status);
  DRT_LAUNCH(commit_wide_count, per_node, n_nodes, A);
  DRT_LAUNCH(commit_scan, 1, A.wg_counts, per_node, &a.status->n_wide);
  DRT_LAUNCH(commit_wide_place, per_node, n_nodes, A);
  DRT_LAUNCH(commit_wide_write, per_inner, a.nodes, n_nodes, A, a.status, (uint4*)a.wide_recs);
  return hipSuccess;
}

}  // namespace drt
