// drt_bvh_ploc.hip — a second device builder (drt_build_bvh_device_ex, DRT_BVH_BUILDER_PLOC): bottom-up
// clustering over the Morton order, after Meister and Bittner 2018, "Parallel Locally-Ordered Clustering for
// Bounding Volume Hierarchy Construction".
//
// Stages 0 to 3 are the LBVH builder's (launch_bvh_sorted, drt_bvh_arena.hpp).  Then the sorted primitives
// are the first clusters (ploc_init), and a round is four kernels over workgroups of 256 live clusters:
//   ploc_nearest   a workgroup stages its 256 boxes and a halo of R on each side in LDS; every pair (i, i + k),
//                  k = 1 .. R, is evaluated once, by the lane of i, always as (lower, upper), and its union
//                  surface xy + yz + zx is published to both ends with a 64-bit LDS minimum of (surface bits,
//                  index of the other end): R evaluations per lane, and both ends see the same bits.  nn[i] is
//                  the least (surface, index): a non-finite surface counts as +inf, ties go to the pair partner
//                  (slot i ^ 1, see nn_key) and then to the lower index, so no result depends on lane order
//   ploc_merge     i and nn[i] merge if nn[nn[i]] == i; the lower slot keeps the cluster (flag 3), the upper
//                  one dies (flag 0), every other cluster lives on (flag 1).  Per-workgroup counts of live
//                  clusters and of merges, packed in one 64-bit word.  A forced round (below) pairs slot 2k
//                  with 2k + 1 instead and reads no nn
//   ploc_scan      one workgroup: exclusive scan of those counts (block_scan_array of drt_scan_sort.hpp); the
//                  next round's live count, and the round counts when one cluster is left
//   ploc_compact   live rank and merge rank of every cluster from the scanned counts and a workgroup scan.  A
//                  merged cluster becomes node (n - live count) + merge rank — merges so far plus its rank, no
//                  atomic counter decides an id — and writes child ids, parent links, the union box, primitive
//                  count, inner count and depth; every live cluster goes to slot `live rank` of the other
//                  cluster buffer, so the order is kept.  (Ids come through the scan, so the node is written
//                  here and not in ploc_merge.)  A merge of round 0 joins two primitives: a leaf of two (the
//                  reference's n_objects <= 2 rule, which the LBVH follows); later merges make inner nodes
//   ploc_emit      numbering as bvh_emit (the inner node of preorder rank r keeps its children at 1 + 2r and
//                  2 + 2r).  A PLOC subtree is no run of the Morton order, so a leaf's `first` is the primitive
//                  count to its left in depth-first order: on the walk to the root, the sum of the left
//                  siblings' primitive counts, next to the sum of their inner counts; order[first ..] gets the
//                  leaf's scene indices
//
// Termination and depth.  Every search round merges at least one pair: the globally least (surface, partner
// bit, lower index, upper index) pair is mutual under the tie rule.  A sorted geometric progression merges only
// about two pairs a round, so after kPlocSearchRounds search rounds the rounds are forced, which halves the
// count each time.  A merge adds at most one level: depth <= 64 + ceil(log2 n) + 1 <= 91 for n <= 2^26, below the
// traversal stack's 96.  The loop that climbs parent links is bounded by 128, as bvh_refit's and bvh_emit's.
//
// No lane waits for or polls another lane, wave or workgroup.  Rounds and the kernels of a round are kernel
// boundaries on one stream; everything a kernel reads of another workgroup's (cluster buffers, nn, flags,
// counts, node data) was written by an earlier launch and is written by no one in this one, so no cross-XCD
// fences or device-scope loads are needed, unlike bvh_refit.  The host enqueues kPlocBatch rounds on a grid
// sized by an upper bound of the live count (surplus workgroups read the count and return), then reads the
// 4-byte count back, and stops at 1.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../../include/drt.h"
#include "drt_bvh_arena.hpp"
#include "drt_bvh_ploc.hpp"
#include "drt_scan_sort.hpp"

namespace drt {

namespace {

constexpr int kR = kPlocRadius;
constexpr int kStaged = kThreads + 2 * kR;   // boxes a workgroup of ploc_nearest holds in LDS
constexpr int kPlocMaxRounds = kPlocSearchRounds + 27;  // + ceil(log2 2^26) forced ones, and one to spare
static_assert(kR >= 1 && kR <= kThreads, "the halo's evaluators are the first R lanes");

struct PlocArena {
  uint4* cluster[2];   // 2 per live cluster: (min xyz bits, node id), (max xyz bits, primitive count)
  uint32_t* nn;        // per cluster slot: the slot of its nearest neighbour
  uint32_t* flag;      // per cluster slot: 0 dead, 1 live, 3 live and merged with its partner
  uint64_t* tile;      // per workgroup: live count | merges << 32, scanned in place
  uint32_t* nprim;     // per internal node id: primitives below it
  uint32_t* counts;    // kPlocMaxRounds + 1: the live count at the start of each round
};

PlocArena carve_ploc(void* scratch, uint32_t n, BvhArena* bvh, size_t* total) {
  size_t front = 0;
  const BvhArena A = carve_bvh(scratch, n, &front);
  if (bvh) *bvh = A;
  ScratchSlicer s{scratch, front};
  PlocArena P;
  P.cluster[0] = s.take<uint4>(2 * (size_t)n);
  P.cluster[1] = s.take<uint4>(2 * (size_t)n);
  P.nn = s.take<uint32_t>(n);
  P.flag = s.take<uint32_t>(n);
  P.tile = s.take<uint64_t>(div_up(n, kThreads) + 1);
  P.nprim = s.take<uint32_t>(n);
  P.counts = s.take<uint32_t>(kPlocMaxRounds + 1);
  if (total) *total = s.used;
  return P;
}

// ---- the first clusters ----------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ploc_init(uint32_t n, BvhArena A, PlocArena P, uint32_t* info) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;  // a sorted position
  if (j == 0) P.counts[0] = n;
  if (j >= 4 && j < (uint32_t)kPlocInfoWords) info[j] = 0u;
  if (j >= n) return;
  const uint32_t o = A.pay[A.plan->final_sel][j], id = n - 1 + j;
  const float4 lo = A.pbox[2 * (size_t)o], hi = A.pbox[2 * (size_t)o + 1];
  const uint4 c0 = make_uint4(__float_as_uint(lo.x), __float_as_uint(lo.y), __float_as_uint(lo.z), id);
  const uint4 c1 = make_uint4(__float_as_uint(hi.x), __float_as_uint(hi.y), __float_as_uint(hi.z), 1u);
  P.cluster[0][2 * (size_t)j] = c0;
  P.cluster[0][2 * (size_t)j + 1] = c1;
  uint4* nd = (uint4*)(A.ndata + (size_t)id * kNodeWords);
  nd[0] = make_uint4(c0.x, c0.y, c0.z, c1.x);
  nd[1] = make_uint4(c1.y, c1.z, 1u, 0u);  // depth 1, no inner node
}

// ---- a round: nearest neighbours ---------------------------------------------------------------------
// (surface bits, not the pair partner, index): positive float bits order as integers; anything else than a
// finite surface >= 0 (NaN or infinite boxes) is +inf.  Bit 31 is clear for the pair (2k, 2k + 1): among equal
// surfaces a cluster prefers its pair partner, then the lower index.  Without it a run of equal boxes
// (coincident or instanced primitives: every surface ties) would merge one pair a round, its first two; with
// it the run halves.  The bit is the same from both ends of a pair, so the least (surface, bit, lower index,
// upper index) pair of all is still mutual.  Indices are below 2^26.
__device__ inline unsigned long long nn_key(float area, bool partner, uint32_t other) {
  const uint32_t b = (area >= 0.f && area < __uint_as_float(0x7F800000u)) ? (__float_as_uint(area) & 0x7FFFFFFFu)
                                                                          : 0x7F800000u;
  return ((unsigned long long)b << 32) | (partner ? 0u : 0x80000000u) | other;
}

__global__ __launch_bounds__(kThreads) void ploc_nearest(PlocArena P, int round) {
  __shared__ float sb[6][kStaged];  // min xyz, max xyz of staged slot s = cluster base - R + s
  __shared__ unsigned long long best[kThreads];
  const uint32_t count = P.counts[round];
  const uint32_t base = blockIdx.x * kThreads;
  if (base >= count) return;  // a surplus workgroup (the same for every lane)
  const uint4* __restrict__ cl = P.cluster[round & 1];
  const int t = threadIdx.x;
  best[t] = ~0ull;
  for (int s = t; s < kStaged; s += kThreads) {
    const int64_t g = (int64_t)base - kR + s;
    if (g >= 0 && g < (int64_t)count) {  // both ends of the array: slots outside it are never read below
      const uint4 c0 = cl[2 * (size_t)g], c1 = cl[2 * (size_t)g + 1];
      sb[0][s] = __uint_as_float(c0.x); sb[1][s] = __uint_as_float(c0.y); sb[2][s] = __uint_as_float(c0.z);
      sb[3][s] = __uint_as_float(c1.x); sb[4][s] = __uint_as_float(c1.y); sb[5][s] = __uint_as_float(c1.z);
    }
  }
  __syncthreads();
  // evaluators: staged slots 0 .. 255 + R (the left halo's too, for their pairs that reach into this
  // workgroup's clusters); the first R lanes take a second one
  for (int e = t; e < kThreads + kR; e += kThreads) {
    const int64_t g = (int64_t)base - kR + e;
    if (g < 0 || g >= (int64_t)count) continue;
    const float lx = sb[0][e], ly = sb[1][e], lz = sb[2][e], hx = sb[3][e], hy = sb[4][e], hz = sb[5][e];
#pragma unroll
    for (int k = 1; k <= kR; k++) {
      const int64_t gj = g + k;
      const int own = e - kR, other = e + k - kR;  // their slots among this workgroup's 256
      if (gj >= (int64_t)count || other < 0) continue;  // past the end / both in the left halo
      const int s = e + k;
      const float ex = smax(hx, sb[3][s]) - smin(lx, sb[0][s]);
      const float ey = smax(hy, sb[4][s]) - smin(ly, sb[1][s]);
      const float ez = smax(hz, sb[5][s]) - smin(lz, sb[2][s]);
      const float area = ex * ey + ey * ez + ez * ex;
      const bool partner = k == 1 && !(g & 1);
      if (own >= 0) atomicMin(&best[own], nn_key(area, partner, (uint32_t)gj));
      if (other < kThreads) atomicMin(&best[other], nn_key(area, partner, (uint32_t)g));
    }
  }
  __syncthreads();
  const uint32_t i = base + t;
  if (i < count) P.nn[i] = (uint32_t)best[t] & 0x7FFFFFFFu;  // 2^31 - 1, no slot, if the cluster is alone
}

// ---- a round: who merges -----------------------------------------------------------------------------
__device__ inline uint64_t flag_counts(uint32_t f) { return (uint64_t)(f & 1u) | ((uint64_t)(f >> 1) << 32); }

__global__ __launch_bounds__(kThreads) void ploc_merge(PlocArena P, int round, int forced) {
  __shared__ uint64_t wave_tot[4];
  const uint32_t count = P.counts[round];
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (blockIdx.x * kThreads >= count) return;
  uint32_t f = 0u;
  if (i < count) {
    const uint32_t j = forced ? (i ^ 1u) : P.nn[i];
    const bool mutual = j < count && (forced || P.nn[j] == i);
    f = !mutual ? 1u : (i < j ? 3u : 0u);
    P.flag[i] = f;
  }
  const uint64_t live = __ballot(f & 1u), merged = __ballot(f >> 1);
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = (uint64_t)__popcll(live) | ((uint64_t)__popcll(merged) << 32);
  __syncthreads();
  if (threadIdx.x == 0) P.tile[blockIdx.x] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
}

__global__ __launch_bounds__(kThreads) void ploc_scan(PlocArena P, int round, uint32_t* info) {
  const uint32_t count = P.counts[round];
  const uint32_t tiles = (count + kThreads - 1) / kThreads;
  const uint64_t total = block_scan_array<uint64_t>(P.tile, tiles, 0ull);
  if (threadIdx.x != 0) return;
  const uint32_t left = (uint32_t)total;
  P.counts[round + 1] = left;
  if (count > 1u && left == 1u) {  // the root was made in this round
    const uint32_t rounds = (uint32_t)round + 1u;
    info[4] = rounds < (uint32_t)kPlocSearchRounds ? rounds : (uint32_t)kPlocSearchRounds;
    info[5] = rounds - info[4];
  }
}

// ---- a round: new nodes, compaction --------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ploc_compact(uint32_t n, BvhArena A, PlocArena P, int round, int forced) {
  __shared__ uint64_t wave_tot[4];
  const uint32_t count = P.counts[round];
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (blockIdx.x * kThreads >= count) return;
  const uint4* __restrict__ in = P.cluster[round & 1];
  uint4* __restrict__ out = P.cluster[(round & 1) ^ 1];
  const uint32_t f = i < count ? P.flag[i] : 0u;
  uint64_t total;
  const uint64_t ex = P.tile[blockIdx.x] + block_scan_excl<uint64_t>(flag_counts(f), wave_tot, total);
  if (!(f & 1u)) return;
  const uint32_t slot = (uint32_t)ex, mrank = (uint32_t)(ex >> 32);
  uint4 c0 = in[2 * (size_t)i], c1 = in[2 * (size_t)i + 1];
  const uint32_t j = forced ? (i ^ 1u) : P.nn[i];
  const uint32_t id = (n - count) + mrank;  // merges of the rounds before + this one's rank
  if (f == 3u && j < count && id < n - 1) {
    const uint4 d0 = in[2 * (size_t)j], d1 = in[2 * (size_t)j + 1];
    const uint32_t lc = c0.w, rc = d0.w;
    c0.x = __float_as_uint(smin(__uint_as_float(c0.x), __uint_as_float(d0.x)));
    c0.y = __float_as_uint(smin(__uint_as_float(c0.y), __uint_as_float(d0.y)));
    c0.z = __float_as_uint(smin(__uint_as_float(c0.z), __uint_as_float(d0.z)));
    c1.x = __float_as_uint(smax(__uint_as_float(c1.x), __uint_as_float(d1.x)));
    c1.y = __float_as_uint(smax(__uint_as_float(c1.y), __uint_as_float(d1.y)));
    c1.z = __float_as_uint(smax(__uint_as_float(c1.z), __uint_as_float(d1.z)));
    c0.w = id;
    c1.w += d1.w;
    uint32_t depth = 1u, inner = 0u;  // round 0: two primitives, a leaf of two
    if (round > 0) {
      const uint2 l = *(const uint2*)(A.ndata + (size_t)lc * kNodeWords + 6);
      const uint2 r = *(const uint2*)(A.ndata + (size_t)rc * kNodeWords + 6);
      depth = 1u + (l.x > r.x ? l.x : r.x);
      inner = 1u + l.y + r.y;
    }
    A.left[id] = lc;
    A.right[id] = rc;
    A.parent[lc] = id;
    A.parent[rc] = id;
    P.nprim[id] = c1.w;
    uint4* nd = (uint4*)(A.ndata + (size_t)id * kNodeWords);
    nd[0] = make_uint4(c0.x, c0.y, c0.z, c1.x);
    nd[1] = make_uint4(c1.y, c1.z, depth, inner);
  }
  if (slot < count) {
    out[2 * (size_t)slot] = c0;
    out[2 * (size_t)slot + 1] = c1;
  }
}

// ---- emit ------------------------------------------------------------------------------------------
// A node is a leaf if its depth is 1: a primitive, or a leaf of two (whose primitives are then not emitted).
__device__ inline uint32_t node_depth(const BvhArena& A, uint32_t id) { return A.ndata[(size_t)id * kNodeWords + 6]; }
__device__ inline uint32_t node_inner(const BvhArena& A, uint32_t id) { return A.ndata[(size_t)id * kNodeWords + 7]; }

__global__ __launch_bounds__(kThreads) void ploc_emit(uint32_t n, BvhArena A, PlocArena P, drt_bvh_node* __restrict__ nodes,
                                                      uint32_t* __restrict__ order, uint32_t* __restrict__ info) {
  const uint32_t id = blockIdx.x * kThreads + threadIdx.x;
  if (id >= 2 * n - 1) return;
  const bool prim = id >= n - 1;
  const uint32_t par = A.parent[id];
  if (prim && par != kNone && node_depth(A, par) == 1u) return;  // folded into its parent's leaf
  const uint32_t* nd = A.ndata + (size_t)id * kNodeWords;
  const bool leaf = nd[6] == 1u;
  // preorder rank among the inner nodes and primitives to the left, summed on the walk to the root
  uint32_t rank = 0u, first = 0u, slot = 0u;
  uint32_t x = id;
  for (int level = 0; level < 128; level++) {
    const uint32_t px = A.parent[x];
    if (px == kNone) break;
    const uint32_t lx = A.left[px];
    const bool is_right = lx != x;
    if (x == id) slot = is_right ? 2u : 1u;  // + 2 rank(parent), below
    else rank += 1u;                         // px's child x is an inner node above id
    if (is_right) {
      rank += node_inner(A, lx);
      first += lx >= n - 1 ? 1u : P.nprim[lx];
    }
    x = px;
  }
  // here rank = rank(parent) + (id is a right child ? inner count of its left sibling : 0) for par != kNone
  uint32_t rank_self = 0u;
  if (par != kNone) {
    const uint32_t lp = A.left[par];
    const uint32_t sib = lp != id ? node_inner(A, lp) : 0u;
    slot += 2u * (rank - sib);
    rank_self = rank + 1u;
  }
  if (slot >= 2 * n - 1) return;  // (cannot happen on a well-formed tree; keeps the store in bounds)
  const uint32_t count = prim ? 1u : P.nprim[id];
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
  if (leaf && first + count <= n) {
    const uint32_t* __restrict__ pay = A.pay[A.plan->final_sel];
    if (prim) {
      order[first] = pay[id - (n - 1)];
    } else {  // the lower sorted position first
      const uint32_t a = A.left[id] - (n - 1), b = A.right[id] - (n - 1);
      if (a < n && b < n) {  // (always, on a well-formed tree; keeps the loads in bounds)
        order[first] = pay[a];
        order[first + 1] = pay[b];
      }
    }
  }
  if (par == kNone) {
    info[0] = 1u + 2u * nd[7];  // nodes
    info[1] = 1u + nd[7];       // leaves
    info[2] = nd[6];            // depth
  }
}

}  // namespace

size_t ploc_build_scratch_bytes(uint32_t n_prims) {
  size_t total = 0;
  (void)carve_ploc(nullptr, n_prims ? n_prims : 1u, nullptr, &total);
  return total;
}

hipError_t launch_ploc_build(const drt_prim* d_prims, uint32_t n, void* d_scratch, drt_bvh_node* d_nodes,
                             uint32_t* d_order, uint32_t* d_info, uint32_t* h_count, hipStream_t st) {
  if (!d_prims || !d_scratch || !d_nodes || !d_order || !d_info || !h_count || n == 0 || n > (1u << 26))
    return hipErrorInvalidValue;
  BvhArena A;
  const PlocArena P = carve_ploc(d_scratch, n, &A, nullptr);
  if (const hipError_t e = launch_bvh_sorted(d_prims, n, A, d_info, st)) return e;
  DRT_LAUNCH(ploc_init, div_up(n, kThreads), n, A, P, d_info);
  uint32_t bound = n;  // never below the live count
  for (int round = 0; bound > 1u && round < kPlocMaxRounds;) {
    for (int b = 0; b < kPlocBatch && bound > 1u && round < kPlocMaxRounds; b++, round++) {
      const int forced = round >= kPlocSearchRounds;
      const uint32_t grid = div_up(bound, kThreads);
      if (!forced) DRT_LAUNCH(ploc_nearest, grid, P, round);
      DRT_LAUNCH(ploc_merge, grid, P, round, forced);
      DRT_LAUNCH(ploc_scan, 1, P, round, d_info);
      DRT_LAUNCH(ploc_compact, grid, n, A, P, round, forced);
      bound = forced ? (bound + 1u) / 2u : bound - 1u;  // a forced round halves, a search round merges a pair
    }
    if (const hipError_t e = hipMemcpyAsync(h_count, P.counts + round, sizeof(uint32_t), hipMemcpyDeviceToHost, st)) return e;
    if (const hipError_t e = hipStreamSynchronize(st)) return e;
    if (*h_count == 0u || *h_count > bound) return hipErrorUnknown;  // (a live count the rounds cannot give)
    bound = *h_count;
  }
  if (bound != 1u) return hipErrorUnknown;
  DRT_LAUNCH(ploc_emit, div_up(2 * n - 1, kThreads), n, A, P, d_nodes, d_order, d_info);
  return hipSuccess;
}

}  // namespace drt
