// drt_bvh_wide.hpp — the 4-ary collapse of a device-built binary tree, shared by the two device commits that
// write 4-ary shadow records: the BVH's (drt_bvh_commit.hip) and the Grid scene's shadow tree
// (drt_grid_tree_commit.hip).  What build_wide of drt_capi.hip decides at its defaults (DRT_WIDE_ORDER=2), this
// code decides the same way: the same double-precision box surfaces and comparisons, the same collapse, the
// same quantisation; build_wide's `widen` is wide_record's.
//
//   commit_wide_level   once per level of the 4-ary tree: a lane per wide root of the frontier collapses its
//                       node and appends the inner children to the next frontier, one atomic per wave
//   commit_wide_count / commit_scan / commit_wide_place
//                       a wide root's record index = the exclusive prefix sum of the marks in node-slot order
//                       (only the set of marks depends on arrival order, the placement does not)
//   wide_record         one lane per wide record: collapse again, order, quantise in double, 64-B record
//
// The caller's first kernel clears the marks and the level counts and seeds the frontier with the root
// (wmark[0] = 1, level_cnt[0] = 1, frontier[0][0] = 0 for an inner root).  Header-only, as drt_scan_sort.hpp:
// every translation unit instantiates its own code under its own flags.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../../include/drt.h"
#include "drt_layout.hpp"
#include "drt_scan_sort.hpp"

namespace drt {

constexpr int kMaxLevels = 128;           // level counters (the host launches far fewer levels)
constexpr uint32_t kLevelGridMax = 1024;  // workgroups of a frontier launch (grid-stride beyond)

struct WideArena {
  uint32_t* wmark;      // per node slot: 1 = root of a 4-ary node
  uint32_t* widx;       // per node slot (wide root): its 4-ary record index
  uint32_t* wlist;      // per 4-ary record: its node slot
  uint32_t* frontier[2];
  uint32_t* wg_counts;  // per workgroup of a node-slot launch
  uint32_t* level_cnt;  // kMaxLevels frontier sizes
};

inline WideArena carve_wide(ScratchSlicer& s, uint32_t n) {
  const size_t nodes = 2 * (size_t)n, inner = n;  // 2n - 1 and n - 1 used
  WideArena a;
  a.wmark = s.take<uint32_t>(nodes);
  a.widx = s.take<uint32_t>(nodes);
  a.wlist = s.take<uint32_t>(inner);
  a.frontier[0] = s.take<uint32_t>(inner);
  a.frontier[1] = s.take<uint32_t>(inner);
  a.wg_counts = s.take<uint32_t>((nodes + kThreads - 1) / kThreads + 1);
  a.level_cnt = s.take<uint32_t>(kMaxLevels);
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

__device__ inline uint32_t node_desc(const drt_bvh_node& nd, const uint32_t* __restrict__ inner_index, uint32_t i) {
  return nd.leaf ? leaf_desc(nd.index, nd.n_objs) : inner_index[i];
}

// One workgroup: counts[0 .. n) -> their exclusive scan in place, the total to *total_out.
static __global__ __launch_bounds__(kThreads) void commit_scan(uint32_t* counts, uint32_t n, uint32_t* total_out) {
  const uint32_t total = block_scan_array<uint32_t>(counts, n, 0u);
  if (threadIdx.x == 0) *total_out = total;
}

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

// *wide_depth: the levels of the 4-ary tree reached (at most the launched ones)
static __global__ __launch_bounds__(kThreads) void commit_wide_level(const drt_bvh_node* __restrict__ nodes,
                                                                     uint32_t n_nodes, WideArena A, int level,
                                                                     uint32_t* wide_depth) {
  const uint32_t cnt = A.level_cnt[level];
  const uint32_t n_inner = (n_nodes - 1) / 2;
  const uint32_t* __restrict__ in = A.frontier[level & 1];
  uint32_t* __restrict__ out = A.frontier[(level + 1) & 1];
  const int lane = threadIdx.x & 63;
  if (cnt && blockIdx.x == 0 && threadIdx.x == 0) *wide_depth = (uint32_t)level + 1u;
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

static __global__ __launch_bounds__(kThreads) void commit_wide_count(uint32_t n_nodes, WideArena A) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  uint32_t total;
  (void)block_flag_scan(s < n_nodes && A.wmark[s] != 0u, wave_tot, total);
  if (threadIdx.x == 0) A.wg_counts[blockIdx.x] = total;
}

static __global__ __launch_bounds__(kThreads) void commit_wide_place(uint32_t n_nodes, WideArena A) {
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

// Enqueue the marking and the placement on `st` for a tree of n_nodes nodes and `depth` levels whose first
// kernel has seeded A: *wide_depth and *n_wide (device words) get the levels reached and the record count.
// A 4-ary tree deeper than max_wide_levels is refused anyway: no more frontier launches than that.
inline hipError_t launch_wide_marks(const drt_bvh_node* nodes, uint32_t n_nodes, uint32_t depth, int max_wide_levels,
                                    const WideArena& A, uint32_t* wide_depth, uint32_t* n_wide, hipStream_t st) {
  const uint32_t per_node = (n_nodes + kThreads - 1) / kThreads;
  const uint32_t per_inner = ((n_nodes - 1) / 2 + kThreads - 1) / kThreads;
  // wide roots sit above the leaves, so there are at most depth - 1 levels of them
  int levels = (int)depth - 1;
  if (levels > max_wide_levels) levels = max_wide_levels;
  if (levels > kMaxLevels - 1) levels = kMaxLevels - 1;
  const uint32_t level_grid = per_inner < kLevelGridMax ? per_inner : kLevelGridMax;
  for (int level = 0; level < levels; level++)
    DRT_LAUNCH(commit_wide_level, level_grid, nodes, n_nodes, A, level, wide_depth);
  DRT_LAUNCH(commit_wide_count, per_node, n_nodes, A);
  DRT_LAUNCH(commit_scan, 1, A.wg_counts, per_node, n_wide);
  DRT_LAUNCH(commit_wide_place, per_node, n_nodes, A);
  return hipSuccess;
}

// quantize_axis of drt_capi.hip for four children, in the same double arithmetic.  A function of its own (not
// inlined three times into the record kernel), its results by value.
struct AxisPlanes {
  float p;
  uint32_t ebits, qlo, qhi;
  bool ok;
};

static __device__ __noinline__ AxisPlanes quantize_axis(double l0, double l1, double l2, double l3, double h0,
                                                        double h1, double h2, double h3, int n) {
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

// The 64-B record of the wide root at node slot s, its child boxes grown by `widen` on each side as
// build_wide grows them (0 for the BVH's own shadow tree).  False, and a record of zeros, when it does not
// quantise.
__device__ inline bool wide_record(const drt_bvh_node* __restrict__ nodes, uint32_t n_nodes, uint32_t s,
                                   const uint32_t* __restrict__ widx, double widen, uint4& s0, uint4& s1, uint4& s2,
                                   uint4& s3) {
  s0 = s1 = s2 = s3 = make_uint4(0u, 0u, 0u, 0u);
  if (s >= n_nodes) return false;
  bool ok = true;
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
        lo[k] = (double)nodes[C.ch[k]].bmin[a] - widen;
        hi[k] = (double)nodes[C.ch[k]].bmax[a] + widen;
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
    if (k < C.n) desc[k] = node_desc(nodes[C.ch[k]], widx, C.ch[k]);
  if (!ok || C.n < 2) return false;
  s0 = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]), ebits);
  s1 = make_uint4(q[0], q[1], q[2], q[3]);
  s2 = make_uint4(q[4], q[5], 0u, 0u);
  s3 = make_uint4(desc[0], desc[1], desc[2], desc[3]);
  return true;
}

}  // namespace drt
