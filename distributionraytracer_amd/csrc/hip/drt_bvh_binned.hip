// drt_bvh_binned.hip — a third device builder (drt_build_bvh_device_ex, DRT_BVH_BUILDER_BINNED): the reference's
// binned-SAH tree (BVH::Build, csrc/host/drt_accel.cpp, restating bvh.cpp:62-227), node for node.
//
// Why a sort-free build gives the host's tree.  The host sorts a node's objects by centroid on each axis, but
// reads the sorted order for two things only: the split position (the first lc objects of the sorted range are
// those of buckets < i, because the bucket index is monotone in the centroid), and the order of objects inside
// a leaf.  So the two sides of a split are sets defined by bucket indices; bucket boxes, child boxes (min / max
// unions), counts, the 33 candidate costs and the fallback-leaf rule depend on those sets alone, and are
// computed here with the host's float operations, one for one.  Inside a leaf the objects go in ascending
// centroid on the leaf's sort axis (its parent's best axis; axis 2, the last one tried, for a fallback leaf),
// equal keys in scene order: the host's sequence whenever the keys are distinct.  A root leaf keeps scene order.
// (One thing the sets do not fix: where a bucket holds both a +0 and a -0 bound, the host keeps whichever its
// sort met first; here -0 is the lesser word.)
//
// Large nodes, level by level.  Every live node owns a contiguous segment of the working order; node ids are
// given out level by level and, within a level, in segment order.  A round is five kernels:
//   binned_bin      a workgroup takes a tile of 2 048 positions; a lane computes its object's three bucket
//                   indices from its node's box and accumulates into LDS bins (a count and six order-preserving
//                   words, 36 bins a node) for the first kLdsNodes live nodes the tile touches, straight into
//                   the global bins for any further one; the LDS bins are flushed with one atomic per
//                   non-empty word.  Only integer adds and min / max of ordered() words are atomic: no result
//                   depends on the order they land in
//   binned_split    one wave per node of the level: lanes 0 .. 32 each evaluate one (axis, i) candidate from
//                   the 36 bins, a wave reduction keeps the least cost and then the lowest candidate (the
//                   host's strict < in axis-major order); a fallback leaf, or the axis, bucket, left count and
//                   both child boxes
//   binned_flags    per tile, the number of objects that go left
//   binned_scan     one workgroup: the tiles' left counts; over the level's nodes, the child ids (two per
//                   split, in segment order), the left counts before each node, the list of nodes a wave
//                   finishes; the children's records; the next level's id range
//   binned_scatter  stable partition of every split segment into the other order buffer: an object's rank among
//                   the lefts is the device-wide exclusive scan of the flags minus the left counts of the nodes
//                   before its own, and its node's start and left count place it
// Small nodes, in one wave (binned_wave).  A node of at most kBinnedWave objects: each lane keeps one object's
// box and centroid in registers, a node is a lane mask, bins are filled in LDS and evaluated by the same code
// as binned_split, and a small LDS stack walks the subtree in the host's recursion order.  It writes the
// subtree's nodes under subtree-local preorder ranks and its objects in final leaf order (a lane-rank sort by
// (key, scene index)).  The same kernel orders every other leaf of at most 64 objects.
// Numbering.  binned_inner_counts sums inner counts bottom-up, one launch per level of level-wise nodes (a
// wave-built subtree brings its own count); binned_emit gives each level-wise node its preorder inner rank on a
// walk to the root (rank of a left child: its parent's + 1; of a right child: + the left subtree's inner count)
// and writes the child pair of rank r at slots 1 + 2r and 2 + 2r; binned_emit_wave shifts each wave-built subtree by its root's rank.
// Leaves of more than 64 objects (degenerate input only) are ordered by one stable radix sort of all objects on
// a 64-bit key (leaf start or final position, ordered centroid), the tile of drt_scan_sort.hpp.
//
// No lane waits for or polls another lane, wave or workgroup: rounds and the kernels of a round are kernel
// boundaries on one stream, and what a kernel reads of another workgroup's was written by an earlier launch.
// LDS traffic inside one wave (binned_split, binned_wave) is ordered by wave_sync.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>

#include "../../../include/drt.h"
#include "drt_bvh_arena.hpp"
#include "drt_bvh_binned.hpp"
#include "drt_prim_device.hpp"
#include "drt_scan_sort.hpp"

namespace drt {

namespace {

constexpr int kBuckets = 12;                 // BUCKET_COUNT
constexpr int kBinWords = 7;                 // a bin: count, min xyz, max xyz (ordered words)
constexpr int kNodeBinWords = 3 * kBuckets * kBinWords;  // 252
constexpr int kLdsNodes = 8;                 // nodes of a tile that get LDS bins
constexpr int kLaneSort = 64;                // leaves up to this size are ordered by lane ranks
constexpr uint32_t kLiveMin = kBinnedWave > 2 ? kBinnedWave : 2;  // a node above this is split level-wise
constexpr uint32_t kDone = 0x80000000u;      // in onode: the object's node takes no part in further rounds
constexpr uint32_t kEmptyMin = 0xFFFFFFFFu, kEmptyMax = 0u;  // (no finite float has these ordered words)

enum : uint32_t { kLive = 0, kInner = 1, kLeaf = 2, kWaveRoot = 3 };
// nmeta.y: kind | sort axis << 4 | depth << 8 (the root's depth is 1)
__host__ __device__ inline uint32_t meta_y(uint32_t kind, uint32_t axis, uint32_t depth) { return kind | (axis << 4) | (depth << 8); }

// ctl words
enum { kCtlRootBox = 0, kCtlWaveCount = 7, kCtlBigCount = 8, kCtlLive = 9, kCtlDepth = 10, kCtlMaxLeaf = 11,
       kCtlLevel = 16, kCtlWords = kCtlLevel + kBinnedMaxRounds + 2 };

struct BinnedArena {
  float4* pbox;        // 2 per primitive, scene order: (min, 0), (max, 0)
  uint32_t* ord[2];    // the working order: scene indices
  uint32_t* onode[2];  // per position: its node id, | kDone
  float4* nbox;        // 2 per node id: (box min, segment start), (box max, object count)
  uint4* nmeta;        // per node id: parent, meta_y, first child (wave root: its subtree's inner count), preorder rank
  uint32_t* ninner;    // per node id: inner nodes in its subtree
  uint32_t* bins;      // level_cap x 252, clear between rounds
  uint4* dec;          // per level slot: (1 split | 2 fallback | axis << 2 | bucket << 4, left count, first child, lefts before)
  float4* cbox;        // 3 per level slot: left min, left max, right min, right max
  uint32_t* tilecnt;   // per tile: objects going left, scanned in place
  uint32_t* wlist;     // node ids binned_wave finishes
  drt_bvh_node* wnodes;  // 2 per position: a wave-built subtree's nodes below its root, local numbering
  uint32_t* ctl;
  uint64_t* key[2];    // the sort of leaves above kLaneSort objects
  uint32_t* pay[2];
  uint32_t* table;
  uint32_t level_cap;
};

inline uint32_t level_capacity(uint32_t n) { return 2u * (n / (kLiveMin + 1u)) + 2u; }

BinnedArena carve_binned(void* scratch, uint32_t n, size_t* total) {
  ScratchSlicer s{scratch};
  BinnedArena B;
  B.level_cap = level_capacity(n);
  B.pbox = s.take<float4>(2 * (size_t)n);
  for (int k = 0; k < 2; k++) B.ord[k] = s.take<uint32_t>(n);
  for (int k = 0; k < 2; k++) B.onode[k] = s.take<uint32_t>(n);
  B.nbox = s.take<float4>(4 * (size_t)n);
  B.nmeta = s.take<uint4>(2 * (size_t)n);
  B.ninner = s.take<uint32_t>(2 * (size_t)n);
  B.bins = s.take<uint32_t>((size_t)B.level_cap * kNodeBinWords);
  B.dec = s.take<uint4>(B.level_cap);
  B.cbox = s.take<float4>(3 * (size_t)B.level_cap);
  B.tilecnt = s.take<uint32_t>(div_up(n, kTile) + 1);
  B.wlist = s.take<uint32_t>(n);
  B.wnodes = s.take<drt_bvh_node>(2 * (size_t)n);
  B.ctl = s.take<uint32_t>(kCtlWords);
  for (int k = 0; k < 2; k++) B.key[k] = s.take<uint64_t>(n);
  for (int k = 0; k < 2; k++) B.pay[k] = s.take<uint32_t>(n);
  B.table = s.take<uint32_t>(256 * (size_t)div_up(n, kTile));
  if (total) *total = s.used;
  return B;
}

// ---- what the kernels share ------------------------------------------------------------------------
// orders the LDS traffic of one wave: its DS operations complete in issue order, the fence keeps the compiler
// from moving them
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ inline float centroid1(float lo, float hi) { return (lo + hi) / 2.0f; }  // AABB::centroid()

// min(BUCKET_COUNT - 1, (int)((c - min_bound) * scale)) with scale = BUCKET_COUNT / extent, 0 for a flat axis;
// a NaN product (non-finite input, where the host's cast is undefined) counts as bucket 0
__device__ inline int bucket_of(float c, float mn, float mx) {
  const float ext = mx - mn;
  const float scale = ext > 0.0f ? (float)kBuckets / ext : 0.0f;
  const float x = (c - mn) * scale;
  if (!(x >= 0.0f)) return 0;
  return x >= (float)(kBuckets - 1) ? kBuckets - 1 : (int)x;
}

__device__ inline float axis_of(const float4& v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }

// one object into the 36 bins `b` (LDS or global) of its node; non-finite bounds take no part, as in the LBVH
// builder's centroid bounds
__device__ inline void bin_add(uint32_t* b, const float4& lo, const float4& hi, const float4& nlo, const float4& nhi) {
  const uint32_t w[6] = {ordered(lo.x), ordered(lo.y), ordered(lo.z), ordered(hi.x), ordered(hi.y), ordered(hi.z)};
  const bool f[6] = {finite(lo.x), finite(lo.y), finite(lo.z), finite(hi.x), finite(hi.y), finite(hi.z)};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int bi = bucket_of(centroid1(axis_of(lo, a), axis_of(hi, a)), axis_of(nlo, a), axis_of(nhi, a));
    uint32_t* p = b + (a * kBuckets + bi) * kBinWords;
    atomicAdd(p, 1u);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (f[k]) atomicMin(p + 1 + k, w[k]);
      if (f[3 + k]) atomicMax(p + 4 + k, w[3 + k]);
    }
  }
}

__device__ inline float bin_min(uint32_t w) { return w == kEmptyMin ? FLT_MAX : unordered(w); }
__device__ inline float bin_max(uint32_t w) { return w == kEmptyMax ? -FLT_MAX : unordered(w); }

struct Split {
  bool split;          // else a fallback leaf
  int axis, bucket;
  uint32_t lc;
  float lmn[3], lmx[3], rmn[3], rmx[3];
};

// The host's candidate loop over one node's 36 bins `sb` (LDS, complete and visible to the wave): lane
// L < 33 evaluates axis L / 11, i = 1 + L % 11; every lane gets the result.  Whole wave, converged.
__device__ inline Split eval_split(const uint32_t* sb, const float nlo[3], const float nhi[3], uint32_t n_objects) {
  const int lane = threadIdx.x & 63;
  const int cand = lane < 33 ? lane : 0, axis = cand / 11, i = 1 + cand % 11;
  const float ex = nhi[0] - nlo[0], ey = nhi[1] - nlo[1], ez = nhi[2] - nlo[2];
  const float psa = 2.0f * (ex * ey + ex * ez + ey * ez);
  float lmn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, lmx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float rmn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, rmx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  int lc = 0, rc = 0;
  for (int j = 0; j < kBuckets; j++) {
    const uint32_t* p = sb + (axis * kBuckets + j) * kBinWords;
    const int cnt = (int)p[0];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float mn = bin_min(p[1 + k]), mx = bin_max(p[4 + k]);
      if (j < i) { lmn[k] = smin(lmn[k], mn); lmx[k] = smax(lmx[k], mx); }
      else       { rmn[k] = smin(rmn[k], mn); rmx[k] = smax(rmx[k], mx); }
    }
    if (j < i) lc += cnt; else rc += cnt;
  }
  const float lx = lmx[0] - lmn[0], ly = lmx[1] - lmn[1], lz = lmx[2] - lmn[2];
  const float rx = rmx[0] - rmn[0], ry = rmx[1] - rmn[1], rz = rmx[2] - rmn[2];
  const float la = 2.0f * (lx * ly + lx * lz + ly * lz);
  const float ra = 2.0f * (rx * ry + rx * rz + ry * rz);
  const float cost = 1.0f + ((float)lc * la + (float)rc * ra) * 1.0f / psa;
  // `cost < best_cost` from FLT_MAX on, in candidate order: the least cost below FLT_MAX, the lowest candidate
  float bc = (lane < 33 && cost < FLT_MAX) ? cost : FLT_MAX;
  int bi = (lane < 33 && cost < FLT_MAX) ? lane : 99;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float oc = __shfl_xor(bc, d, 64);
    const int oi = __shfl_xor(bi, d, 64);
    if (oi < 99 && (bi == 99 || oc < bc || (oc == bc && oi < bi))) { bc = oc; bi = oi; }
  }
  Split s;
  const int src = bi < 33 ? bi : 0;
  s.lc = (uint32_t)__shfl(lc, src, 64);
  s.axis = src / 11;
  s.bucket = 1 + src % 11;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    s.lmn[k] = __shfl(lmn[k], src, 64); s.lmx[k] = __shfl(lmx[k], src, 64);
    s.rmn[k] = __shfl(rmn[k], src, 64); s.rmx[k] = __shfl(rmx[k], src, 64);
  }
  // best_split <= left_index || best_split >= right_index || best_cost >= n_objects * INTERSECTION_COST
  s.split = bi < 33 && s.lc > 0u && s.lc < n_objects && !(bc >= (float)(int)n_objects * 1.0f);
  return s;
}

// ---- stage 0: clear, boxes, the root ----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void binned_clear(uint32_t n, BinnedArena B, uint32_t* info) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < (size_t)B.level_cap * kNodeBinWords) {
    const uint32_t f = (uint32_t)(i % kBinWords);
    B.bins[i] = f == 0u ? 0u : (f < 4u ? kEmptyMin : kEmptyMax);
  }
  if (i < (size_t)kCtlWords) B.ctl[i] = i < 3 ? kEmptyMin : 0u;
  if (i < (size_t)kBinnedInfoWords) info[i] = 0u;
  if (i < 2 * (size_t)n) B.ninner[i] = 0u;
}

__global__ __launch_bounds__(kThreads) void binned_bounds(const drt_prim* __restrict__ prims, uint32_t n, BinnedArena B) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
  const bool valid = i < n;
  if (valid) {
    const drt_prim p = prims[i];
    prim_bounds(p, lo, hi);
    B.pbox[2 * (size_t)i] = make_float4(lo[0], lo[1], lo[2], 0.f);
    B.pbox[2 * (size_t)i + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    B.ord[0][i] = i;
    B.onode[0][i] = 0u;
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {  // the world box: across the wave, then one atomic per wave and word
    uint32_t mn = valid && finite(lo[a]) ? ordered(lo[a]) : kEmptyMin;
    uint32_t mx = valid && finite(hi[a]) ? ordered(hi[a]) : kEmptyMax;
    wave_min_max(mn, mx);
    if ((threadIdx.x & 63) == 0) {
      if (mn != kEmptyMin) atomicMin(&B.ctl[kCtlRootBox + a], mn);
      if (mx != kEmptyMax) atomicMax(&B.ctl[kCtlRootBox + 3 + a], mx);
    }
  }
}

// BVH::Build's world box, grown in double by 0.001 and rounded to float; the root's record
__global__ __launch_bounds__(kThreads) void binned_root(uint32_t n, BinnedArena B) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float lo[3], hi[3];
  for (int a = 0; a < 3; a++) {
    lo[a] = (float)((double)bin_min(B.ctl[kCtlRootBox + a]) - 0.001);
    hi[a] = (float)((double)bin_max(B.ctl[kCtlRootBox + 3 + a]) + 0.001);
  }
  B.nbox[0] = make_float4(lo[0], lo[1], lo[2], __uint_as_float(0u));
  B.nbox[1] = make_float4(hi[0], hi[1], hi[2], __uint_as_float(n));
  const uint32_t kind = n <= 2u ? kLeaf : (n <= (uint32_t)kBinnedWave ? kWaveRoot : kLive);
  B.nmeta[0] = make_uint4(kNone, meta_y(kind, 3u, 1u), 0u, 0u);  // axis 3: a root leaf keeps scene order
  B.ctl[kCtlLevel] = 0u;
  B.ctl[kCtlLevel + 1] = 1u;
  B.ctl[kCtlDepth] = 1u;
  if (kind == kLive) {
    B.ctl[kCtlLive] = 1u;
  } else {
    B.wlist[0] = 0u;
    B.ctl[kCtlWaveCount] = 1u;
  }
}

// ---- a round ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void binned_bin(uint32_t n, BinnedArena B, int round) {
  __shared__ uint32_t sb[kLdsNodes * kNodeBinWords];
  __shared__ uint32_t s_first;
  const uint32_t lb = B.ctl[kCtlLevel + round], le = B.ctl[kCtlLevel + round + 1];
  const uint32_t* __restrict__ onode = B.onode[round & 1];
  const uint32_t* __restrict__ ord = B.ord[round & 1];
  const int t = threadIdx.x;
  for (int k = t; k < kLdsNodes * kNodeBinWords; k += kThreads) {
    const int f = k % kBinWords;
    sb[k] = f == 0 ? 0u : (f < 4 ? kEmptyMin : kEmptyMax);
  }
  if (t == 0) s_first = kNone;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)kTile;
  uint32_t slot[kPer];
  uint32_t lowest = kNone;
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t pos = base + j * kThreads + t;
    const uint32_t id = pos < n ? onode[pos] : kNone;  // a finished object's id carries kDone: above `le`
    slot[j] = (id >= lb && id < le && id - lb < B.level_cap) ? id - lb : kNone;
    lowest = slot[j] < lowest ? slot[j] : lowest;
  }
  if (lowest != kNone) atomicMin(&s_first, lowest);
  __syncthreads();
  const uint32_t first = s_first;
  if (first == kNone) return;  // no live object in this tile (the same for every lane)
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    if (slot[j] == kNone) continue;
    const uint32_t pos = base + j * kThreads + t;
    const uint32_t id = lb + slot[j];
    if ((B.nmeta[id].y & 15u) != kLive) continue;
    const uint32_t o = ord[pos];
    if (o >= n) continue;  // (cannot happen; keeps the loads in bounds)
    const float4 lo = B.pbox[2 * (size_t)o], hi = B.pbox[2 * (size_t)o + 1];
    const float4 nlo = B.nbox[2 * (size_t)id], nhi = B.nbox[2 * (size_t)id + 1];
    const uint32_t rel = slot[j] - first;
    uint32_t* b = rel < (uint32_t)kLdsNodes ? sb + rel * kNodeBinWords : B.bins + (size_t)slot[j] * kNodeBinWords;
    bin_add(b, lo, hi, nlo, nhi);
  }
  __syncthreads();
  for (int k = t; k < kLdsNodes * kNodeBinWords; k += kThreads) {
    const uint32_t s = first + (uint32_t)(k / kNodeBinWords);
    if (s >= le - lb || s >= B.level_cap) continue;
    const int f = k % kBinWords;
    const uint32_t v = sb[k];
    uint32_t* g = B.bins + (size_t)s * kNodeBinWords + (k % kNodeBinWords);
    if (f == 0) { if (v != 0u) atomicAdd(g, v); }
    else if (f < 4) { if (v != kEmptyMin) atomicMin(g, v); }
    else if (v != kEmptyMax) atomicMax(g, v);
  }
}

__global__ __launch_bounds__(kThreads) void binned_split(BinnedArena B, int round) {
  __shared__ uint32_t sbins[4][kNodeBinWords];
  const uint32_t lb = B.ctl[kCtlLevel + round], le = B.ctl[kCtlLevel + round + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t slot = blockIdx.x * 4u + (uint32_t)w;
  if (slot >= le - lb || slot >= B.level_cap) return;  // (the same for every lane of the wave)
  const uint32_t id = lb + slot;
  const uint4 m = B.nmeta[id];
  if ((m.y & 15u) != kLive) {
    if (lane == 0) B.dec[slot] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  uint32_t* g = B.bins + (size_t)slot * kNodeBinWords;
  uint32_t* sb = sbins[w];
  for (int k = lane; k < kNodeBinWords; k += 64) {  // take the bins and leave them clear for the next round
    sb[k] = g[k];
    const int f = k % kBinWords;
    g[k] = f == 0 ? 0u : (f < 4 ? kEmptyMin : kEmptyMax);
  }
  wave_sync();
  const float4 nlo4 = B.nbox[2 * (size_t)id], nhi4 = B.nbox[2 * (size_t)id + 1];
  const float nlo[3] = {nlo4.x, nlo4.y, nlo4.z}, nhi[3] = {nhi4.x, nhi4.y, nhi4.z};
  const uint32_t count = __float_as_uint(nhi4.w);
  const Split s = eval_split(sb, nlo, nhi, count);
  if (lane != 0) return;
  if (!s.split) {
    B.dec[slot] = make_uint4(2u, 0u, 0u, 0u);
    B.nmeta[id].y = meta_y(kLeaf, 2u, m.y >> 8);
    return;
  }
  B.dec[slot] = make_uint4(1u | ((uint32_t)s.axis << 2) | ((uint32_t)s.bucket << 4), s.lc, 0u, 0u);
  B.cbox[3 * (size_t)slot] = make_float4(s.lmn[0], s.lmn[1], s.lmn[2], s.lmx[0]);
  B.cbox[3 * (size_t)slot + 1] = make_float4(s.lmx[1], s.lmx[2], s.rmn[0], s.rmn[1]);
  B.cbox[3 * (size_t)slot + 2] = make_float4(s.rmn[2], s.rmx[0], s.rmx[1], s.rmx[2]);
}

// Position `pos` in this round: does its node split, and does the object go left?  *dout: the node's decision.
__device__ inline bool goes_left(const BinnedArena& B, const uint32_t* __restrict__ ord, uint32_t n, uint32_t id,
                                 uint32_t lb, uint32_t le, uint32_t pos, bool& splits, uint4& dout) {
  splits = false;
  if (!(id >= lb && id < le && id - lb < B.level_cap)) return false;
  dout = B.dec[id - lb];
  if (!(dout.x & 1u)) return false;
  splits = true;
  const int axis = (int)((dout.x >> 2) & 3u), bucket = (int)(dout.x >> 4);
  const uint32_t o = ord[pos];
  if (o >= n) return false;  // (cannot happen; keeps the loads in bounds)
  const float c = centroid1(axis_of(B.pbox[2 * (size_t)o], axis), axis_of(B.pbox[2 * (size_t)o + 1], axis));
  return bucket_of(c, axis_of(B.nbox[2 * (size_t)id], axis), axis_of(B.nbox[2 * (size_t)id + 1], axis)) < bucket;
}

__global__ __launch_bounds__(kThreads) void binned_flags(uint32_t n, BinnedArena B, int round) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t lb = B.ctl[kCtlLevel + round], le = B.ctl[kCtlLevel + round + 1];
  const uint32_t* __restrict__ onode = B.onode[round & 1];
  const uint32_t* __restrict__ ord = B.ord[round & 1];
  const uint32_t first = blockIdx.x * (uint32_t)kTile + kPer * threadIdx.x;  // thread t: eight neighbours
  uint32_t cnt = 0u;
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t pos = first + j;
    if (pos >= n) continue;
    bool splits;
    uint4 d;
    cnt += goes_left(B, ord, n, onode[pos], lb, le, pos, splits, d) ? 1u : 0u;
  }
  uint32_t total;
  (void)block_scan_excl<uint32_t>(cnt, wave_tot, total);
  if (threadIdx.x == 0) B.tilecnt[blockIdx.x] = total;
}

// what becomes of a child of `count` objects
__device__ inline uint32_t child_kind(uint32_t count) {
  return count <= 2u ? kLeaf : (count <= (uint32_t)kBinnedWave ? kWaveRoot : kLive);
}

__global__ __launch_bounds__(kThreads) void binned_scan(uint32_t n, uint32_t n_tiles, BinnedArena B, int round, uint32_t* info) {
  __shared__ uint64_t wt64[4], wt64b[4];
  __shared__ uint32_t s_big, s_maxleaf;
  (void)block_scan_array<uint32_t>(B.tilecnt, n_tiles, 0u);
  const uint32_t lb = B.ctl[kCtlLevel + round], le = B.ctl[kCtlLevel + round + 1];
  uint32_t slots = le - lb;
  if (slots > B.level_cap) slots = B.level_cap;
  const uint32_t wbase = B.ctl[kCtlWaveCount];
  if (threadIdx.x == 0) { s_big = 0u; s_maxleaf = 0u; }
  __syncthreads();
  uint64_t carry_a = 0ull, carry_b = 0ull;  // (splits, lefts of the splits), (wave-list entries, live children)
  for (uint32_t c0 = 0; c0 < slots; c0 += kThreads) {
    const uint32_t slot = c0 + threadIdx.x;
    const bool valid = slot < slots;
    const uint32_t id = lb + slot;
    uint4 d = make_uint4(0u, 0u, 0u, 0u);
    uint32_t start = 0u, count = 0u, kl = kLeaf, kr = kLeaf;
    if (valid) {
      d = B.dec[slot];
      start = __float_as_uint(B.nbox[2 * (size_t)id].w);
      count = __float_as_uint(B.nbox[2 * (size_t)id + 1].w);
    }
    const bool split = (d.x & 1u) != 0u, fallback = (d.x & 2u) != 0u;
    uint32_t wl = 0u, live = 0u;
    if (split) {
      kl = child_kind(d.y);
      kr = child_kind(count - d.y);
      wl = (kl != kLive ? 1u : 0u) + (kr != kLive ? 1u : 0u);
      live = 2u - wl;
    } else if (fallback) {
      if (count <= (uint32_t)kLaneSort) wl = 1u; else atomicAdd(&s_big, 1u);
      atomicMax(&s_maxleaf, count);
    }
    uint64_t tot_a, tot_b;
    const uint64_t ea = carry_a + block_scan_excl<uint64_t>((split ? 1ull : 0ull) | ((uint64_t)(split ? d.y : 0u) << 32), wt64, tot_a);
    const uint64_t eb = carry_b + block_scan_excl<uint64_t>((uint64_t)wl | ((uint64_t)live << 32), wt64b, tot_b);
    carry_a += tot_a;
    carry_b += tot_b;
    uint32_t wpos = wbase + (uint32_t)eb;
    if (split) {
      const uint32_t cid = le + 2u * (uint32_t)ea;
      if (cid + 1u < 2u * n) {  // (always: a tree of n objects has at most 2n - 1 nodes)
        const uint4 pm = B.nmeta[id];
        const uint32_t axis = (d.x >> 2) & 3u, depth = pm.y >> 8;
        const float4 c0 = B.cbox[3 * (size_t)slot], c1 = B.cbox[3 * (size_t)slot + 1], c2 = B.cbox[3 * (size_t)slot + 2];
        B.nbox[2 * (size_t)cid] = make_float4(c0.x, c0.y, c0.z, __uint_as_float(start));
        B.nbox[2 * (size_t)cid + 1] = make_float4(c0.w, c1.x, c1.y, __uint_as_float(d.y));
        B.nbox[2 * (size_t)cid + 2] = make_float4(c1.z, c1.w, c2.x, __uint_as_float(start + d.y));
        B.nbox[2 * (size_t)cid + 3] = make_float4(c2.y, c2.z, c2.w, __uint_as_float(count - d.y));
        B.nmeta[cid] = make_uint4(id, meta_y(kl, axis, depth + 1u), 0u, 0u);
        B.nmeta[cid + 1u] = make_uint4(id, meta_y(kr, axis, depth + 1u), 0u, 0u);
        B.nmeta[id] = make_uint4(pm.x, meta_y(kInner, axis, depth), cid, 0u);
        B.dec[slot] = make_uint4(d.x, d.y, cid, (uint32_t)(ea >> 32));
        if (kl != kLive && wpos < n) B.wlist[wpos++] = cid;
        if (kr != kLive && wpos < n) B.wlist[wpos++] = cid + 1u;
        if (kl == kLeaf) atomicMax(&s_maxleaf, d.y);
        if (kr == kLeaf) atomicMax(&s_maxleaf, count - d.y);
      }
    } else if (fallback && wl && wpos < n) {
      B.wlist[wpos] = id;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint32_t splits = (uint32_t)carry_a;
  B.ctl[kCtlLevel + round + 2] = le + 2u * splits;
  B.ctl[kCtlWaveCount] = wbase + (uint32_t)carry_b;
  B.ctl[kCtlLive] = (uint32_t)(carry_b >> 32);
  B.ctl[kCtlBigCount] += s_big;
  if (s_maxleaf > B.ctl[kCtlMaxLeaf]) B.ctl[kCtlMaxLeaf] = s_maxleaf;
  if (splits) B.ctl[kCtlDepth] = (uint32_t)round + 2u;
  if (splits || round == 0) info[4] = (uint32_t)round + 1u;
}

__global__ __launch_bounds__(kThreads) void binned_scatter(uint32_t n, BinnedArena B, int round) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t lb = B.ctl[kCtlLevel + round], le = B.ctl[kCtlLevel + round + 1];
  const uint32_t* __restrict__ onode = B.onode[round & 1];
  const uint32_t* __restrict__ ord = B.ord[round & 1];
  uint32_t* __restrict__ onode_out = B.onode[(round & 1) ^ 1];
  uint32_t* __restrict__ ord_out = B.ord[(round & 1) ^ 1];
  const uint32_t first = blockIdx.x * (uint32_t)kTile + kPer * threadIdx.x;
  uint32_t id[kPer], cnt = 0u;
  uint4 d[kPer];
  uint32_t state[kPer];  // 0 past the end, 1 stays, 2 goes right, 3 goes left
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t pos = first + j;
    state[j] = 0u;
    id[j] = kNone;
    d[j] = make_uint4(0u, 0u, 0u, 0u);
    if (pos >= n) continue;
    id[j] = onode[pos];
    bool splits;
    const bool left = goes_left(B, ord, n, id[j], lb, le, pos, splits, d[j]);
    state[j] = splits ? (left ? 3u : 2u) : 1u;
    cnt += left ? 1u : 0u;
  }
  uint32_t total;
  uint32_t lefts = B.tilecnt[blockIdx.x] + block_scan_excl<uint32_t>(cnt, wave_tot, total);  // lefts before `pos`, device-wide
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t pos = first + j;
    if (state[j] == 0u) continue;
    uint32_t to = pos, tag = id[j];
    if (state[j] == 1u) {
      // a node that became a leaf in this round takes no part in later ones
      if (id[j] >= lb && id[j] < le && id[j] - lb < B.level_cap && (d[j].x & 2u)) tag |= kDone;
    } else {
      const uint32_t start = __float_as_uint(B.nbox[2 * (size_t)id[j]].w);
      const uint32_t count = __float_as_uint(B.nbox[2 * (size_t)id[j] + 1].w);
      const uint32_t lc = d[j].y, before = lefts - d[j].w;  // lefts of this segment before `pos`
      const bool left = state[j] == 3u;
      to = left ? start + before : start + lc + (pos - start - before);
      const uint32_t ccount = left ? lc : count - lc;
      tag = (d[j].z + (left ? 0u : 1u)) | (child_kind(ccount) == kLive ? 0u : kDone);
      lefts += left ? 1u : 0u;
    }
    if (to < n) {
      ord_out[to] = ord[pos];
      onode_out[to] = tag;
    }
  }
}

// ---- small nodes: one wave each ---------------------------------------------------------------------
// ascending (centroid on `axis`, scene index) among the lanes of `mask`: this lane's rank.  Axis 3: scene order.
__device__ inline uint32_t lane_rank(uint64_t mask, float key, uint32_t o) {
  uint32_t rank = 0u;
  for (uint64_t mm = mask; mm; mm &= mm - 1ull) {
    const int src = __ffsll((unsigned long long)mm) - 1;
    const float k2 = __shfl(key, src, 64);
    const uint32_t o2 = __shfl(o, src, 64);
    rank += (k2 < key || (!(key < k2) && o2 < o)) ? 1u : 0u;
  }
  return rank;
}

// The stack holds disjoint, non-empty lane masks: at most one entry per object.  A split pops one and pushes
// two, and a subtree of c <= 64 objects has at most c - 1 <= 63 inner nodes, so the two guards on a split in
// binned_wave (next_rank < count, sp + 2 <= kStack) never turn one down; they keep the stores in bounds.
constexpr int kStack = 64;
static_assert(kStack >= 64 && kBinnedWave <= kStack, "one stack entry per object of a wave");
struct WaveLds {
  uint32_t bins[kNodeBinWords];
  uint64_t mask[kStack];
  float box[kStack][6];
  uint32_t slot[kStack];   // local node slot: 0 the subtree's root, k >= 1 -> wnodes[2 start + k - 1]
  uint32_t meta[kStack];   // sort axis | local depth << 4
};

__global__ __launch_bounds__(kThreads) void binned_wave(uint32_t n, uint32_t n_list, BinnedArena B, int sel,
                                                        uint32_t* __restrict__ order) {
  __shared__ WaveLds lds[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t item = blockIdx.x * 4u + (uint32_t)w;
  if (item >= n_list || item >= n) return;  // (the same for every lane of the wave)
  WaveLds& L = lds[w];
  const uint32_t id = B.wlist[item];
  if (id >= 2u * n) return;
  const uint4 m = B.nmeta[id];
  const float4 nlo4 = B.nbox[2 * (size_t)id], nhi4 = B.nbox[2 * (size_t)id + 1];
  const uint32_t start = __float_as_uint(nlo4.w), count = __float_as_uint(nhi4.w);
  if (count == 0u || count > 64u || start + count > n) return;
  const bool in = (uint32_t)lane < count;
  uint32_t o = in ? B.ord[sel][start + lane] : 0u;
  if (o >= n) o = 0u;  // (cannot happen; keeps the loads in bounds)
  const float4 lo = B.pbox[2 * (size_t)o], hi = B.pbox[2 * (size_t)o + 1];
  const float cen[3] = {centroid1(lo.x, hi.x), centroid1(lo.y, hi.y), centroid1(lo.z, hi.z)};
  const uint64_t all = count == 64u ? ~0ull : ((1ull << count) - 1ull);
  const uint32_t axis0 = (m.y >> 4) & 15u, depth0 = m.y >> 8;
  if ((m.y & 15u) == kLeaf) {
    const float key = axis0 == 0u ? cen[0] : (axis0 == 1u ? cen[1] : (axis0 == 2u ? cen[2] : 0.f));
    const uint32_t rank = lane_rank(all, key, o);
    if (in && rank < count) order[start + rank] = o;
    return;
  }
  if (lane == 0) {
    L.mask[0] = all;
    L.box[0][0] = nlo4.x; L.box[0][1] = nlo4.y; L.box[0][2] = nlo4.z;
    L.box[0][3] = nhi4.x; L.box[0][4] = nhi4.y; L.box[0][5] = nhi4.z;
    L.slot[0] = 0u;
    L.meta[0] = axis0;
  }
  int sp = 1;
  uint32_t next_rank = 0u, next_pos = start, max_depth = 0u;
  const uint32_t max_slots = 2u * count;
  for (int guard = 0; guard < 4 * 64 && sp > 0; guard++) {
    wave_sync();
    sp--;
    const uint64_t mask = L.mask[sp];
    float nlo[3], nhi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { nlo[k] = L.box[sp][k]; nhi[k] = L.box[sp][3 + k]; }
    const uint32_t slot = L.slot[sp], meta = L.meta[sp];
    wave_sync();  // the entry is read before a push overwrites it
    const uint32_t cnt = (uint32_t)__popcll(mask), ldepth = meta >> 4;
    const bool mine = (mask >> lane) & 1ull;
    max_depth = ldepth > max_depth ? ldepth : max_depth;
    Split s;
    s.split = false;
    uint32_t leaf_axis = meta & 15u;
    if (cnt > 2u) {
      for (int k = lane; k < kNodeBinWords; k += 64) {
        const int f = k % kBinWords;
        L.bins[k] = f == 0 ? 0u : (f < 4 ? kEmptyMin : kEmptyMax);
      }
      wave_sync();
      if (mine)
        bin_add(L.bins, lo, hi, make_float4(nlo[0], nlo[1], nlo[2], 0.f), make_float4(nhi[0], nhi[1], nhi[2], 0.f));
      wave_sync();
      s = eval_split(L.bins, nlo, nhi, cnt);
      leaf_axis = 2u;  // a fallback leaf keeps the sort on the last axis tried
    }
    drt_bvh_node rec;
#pragma unroll
    for (int k = 0; k < 3; k++) { rec.bmin[k] = nlo[k]; rec.bmax[k] = nhi[k]; }
    if (s.split && next_rank < count && sp + 2 <= kStack) {
      const uint32_t r = next_rank++;
      rec.leaf = 0u;
      rec.index = 1u + 2u * r;  // subtree-local; binned_emit_wave adds twice the root's rank
      rec.n_objs = 0u;
      const float c = s.axis == 0 ? cen[0] : (s.axis == 1 ? cen[1] : cen[2]);
      const bool left = mine && bucket_of(c, nlo[s.axis], nhi[s.axis]) < s.bucket;
      const uint64_t lmask = __ballot(left), rmask = mask & ~lmask;
      if (lane == 0) {  // the right child below the left one: the left subtree comes first
        L.mask[sp] = rmask; L.mask[sp + 1] = lmask;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          L.box[sp][k] = s.rmn[k]; L.box[sp][3 + k] = s.rmx[k];
          L.box[sp + 1][k] = s.lmn[k]; L.box[sp + 1][3 + k] = s.lmx[k];
        }
        L.slot[sp] = 2u + 2u * r; L.slot[sp + 1] = 1u + 2u * r;
        L.meta[sp] = L.meta[sp + 1] = (uint32_t)s.axis | ((ldepth + 1u) << 4);
      }
      sp += 2;
    } else {
      const float key = leaf_axis == 0u ? cen[0] : (leaf_axis == 1u ? cen[1] : (leaf_axis == 2u ? cen[2] : 0.f));
      const uint32_t rank = lane_rank(mask, key, o);
      if (mine && next_pos + rank < start + count) order[next_pos + rank] = o;
      rec.leaf = 1u;
      rec.index = next_pos;
      rec.n_objs = cnt;
      next_pos += cnt;
      if (lane == 0) atomicMax(&B.ctl[kCtlMaxLeaf], cnt);
    }
    if (lane == 0) {
      if (slot == 0u) {
        if (rec.leaf) B.nmeta[id].y = meta_y(kLeaf, 2u, depth0);
      } else if (slot - 1u < max_slots) {
        B.wnodes[2 * (size_t)start + slot - 1u] = rec;
      }
    }
  }
  if (lane == 0) {
    B.nmeta[id].z = next_rank;  // the subtree's inner nodes, its root included
    atomicMax(&B.ctl[kCtlDepth], depth0 + max_depth);
  }
}

// ---- numbering --------------------------------------------------------------------------------------
// one level of the level-wise nodes, the deepest first: a node's inner count from its children's
__global__ __launch_bounds__(kThreads) void binned_inner_counts(uint32_t n_ids, BinnedArena B, int level) {
  const uint32_t lb = B.ctl[kCtlLevel + level], le = B.ctl[kCtlLevel + level + 1];
  const uint32_t id = lb + blockIdx.x * kThreads + threadIdx.x;
  if (id >= le || id >= n_ids) return;
  const uint4 m = B.nmeta[id];
  const uint32_t kind = m.y & 15u;
  uint32_t inner = kind == kWaveRoot ? m.z : 0u;
  if (kind == kInner && m.z + 1u < n_ids) inner = 1u + B.ninner[m.z] + B.ninner[m.z + 1u];
  B.ninner[id] = inner;
}

__global__ __launch_bounds__(kThreads) void binned_emit(uint32_t n, uint32_t n_ids, BinnedArena B,
                                                        drt_bvh_node* __restrict__ nodes, uint32_t* __restrict__ info) {
  const uint32_t id = blockIdx.x * kThreads + threadIdx.x;
  if (id >= n_ids) return;
  const uint4 m = B.nmeta[id];
  // rank(x) = rank(parent) + 1 + (x is the right child ? inner count of its left sibling, x - 1 : 0)
  uint32_t rank = 0u, own = 0u;
  bool is_right = false;
  uint32_t x = id;
  for (int level = 0; level < 128; level++) {
    const uint32_t px = B.nmeta[x].x;
    if (px >= n_ids) break;
    const bool right = B.nmeta[px].z != x;
    const uint32_t step = 1u + (right && x > 0u ? B.ninner[x - 1u] : 0u);
    if (x == id) { own = step; is_right = right; }
    rank += step;
    x = px;
  }
  const uint32_t slot = m.x >= n_ids ? 0u : 1u + 2u * (rank - own) + (is_right ? 1u : 0u);
  if (slot >= 2u * n - 1u) return;  // (cannot happen on a well-formed tree; keeps the store in bounds)
  const float4 lo = B.nbox[2 * (size_t)id], hi = B.nbox[2 * (size_t)id + 1];
  const bool leaf = (m.y & 15u) == kLeaf;
  drt_bvh_node out;
  out.bmin[0] = lo.x; out.bmin[1] = lo.y; out.bmin[2] = lo.z;
  out.bmax[0] = hi.x; out.bmax[1] = hi.y; out.bmax[2] = hi.z;
  out.leaf = leaf ? 1u : 0u;
  out.index = leaf ? __float_as_uint(lo.w) : 1u + 2u * rank;
  out.n_objs = leaf ? __float_as_uint(hi.w) : 0u;
  nodes[slot] = out;
  B.nmeta[id].w = rank;
  if (id == 0u) {
    const uint32_t inner = B.ninner[0];
    info[0] = 1u + 2u * inner;
    info[1] = 1u + inner;
    info[2] = B.ctl[kCtlDepth];
    info[6] = B.ctl[kCtlMaxLeaf];
  }
}

// one lane per local node slot of the wave-built subtrees: wnodes[2 start + k - 1] -> nodes[2 R + k]
__global__ __launch_bounds__(kThreads) void binned_emit_wave(uint32_t n, uint32_t n_ids, BinnedArena B, int sel,
                                                             drt_bvh_node* __restrict__ nodes) {
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= 2u * n) return;
  const uint32_t id = B.onode[sel][p >> 1] & ~kDone;
  if (id >= n_ids) return;
  const uint4 m = B.nmeta[id];
  if ((m.y & 15u) != kWaveRoot) return;
  const uint32_t start = __float_as_uint(B.nbox[2 * (size_t)id].w);
  if (p < 2u * start) return;
  const uint32_t k1 = p - 2u * start;  // local slot - 1
  if (k1 >= 2u * m.z) return;
  drt_bvh_node rec = B.wnodes[p];
  if (!rec.leaf) rec.index += 2u * m.w;
  const uint32_t slot = 2u * m.w + k1 + 1u;
  if (slot < 2u * n - 1u) nodes[slot] = rec;
}

// ---- leaves above kLaneSort objects -----------------------------------------------------------------
// Keys in scene order, so that the stable sort breaks ties by scene index: (leaf start, ordered centroid on
// axis 2) for an object of such a leaf, (final position, 0) for every other one, whose place is known.
__global__ __launch_bounds__(kThreads) void binned_big_keys(uint32_t n, uint32_t n_ids, BinnedArena B, int sel,
                                                            const uint32_t* __restrict__ order) {
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= n) return;
  const uint32_t id = B.onode[sel][p] & ~kDone;
  bool big = false;
  uint32_t start = 0u, axis = 2u;
  if (id < n_ids) {
    const uint4 m = B.nmeta[id];
    start = __float_as_uint(B.nbox[2 * (size_t)id].w);
    axis = (m.y >> 4) & 15u;
    big = (m.y & 15u) == kLeaf && __float_as_uint(B.nbox[2 * (size_t)id + 1].w) > (uint32_t)kLaneSort;
  }
  const uint32_t o = big ? B.ord[sel][p] : order[p];
  if (o >= n) return;  // (cannot happen; keeps the stores in bounds)
  uint64_t key = (uint64_t)p << 32;
  if (big) {
    const int a = axis < 3u ? (int)axis : 2;
    const float c = centroid1(axis_of(B.pbox[2 * (size_t)o], a), axis_of(B.pbox[2 * (size_t)o + 1], a)) + 0.0f;  // -0 -> +0
    key = ((uint64_t)start << 32) | ordered(c);
  }
  B.key[0][o] = key;
  B.pay[0][o] = o;
}

__global__ __launch_bounds__(kThreads) void binned_sort_count(uint32_t n, uint32_t n_wg, int pass, BinnedArena B) {
  radix_count_tile<uint64_t>(B.key[pass & 1], n, n_wg, pass, B.table);
}
__global__ __launch_bounds__(kThreads) void binned_sort_scan(uint32_t n_wg, BinnedArena B) {
  (void)block_scan_array<uint32_t>(B.table, 256u * n_wg, 0u);  // digit-major: the scan gives global positions
}
__global__ __launch_bounds__(kThreads) void binned_sort_scatter(uint32_t n, uint32_t n_wg, int pass, BinnedArena B,
                                                                uint32_t* pay_dst) {
  radix_scatter_tile<uint64_t>(B.key[pass & 1], B.pay[pass & 1], B.key[(pass & 1) ^ 1], pay_dst, n, n_wg, pass, B.table);
}

}  // namespace

size_t binned_build_scratch_bytes(uint32_t n_prims) {
  size_t total = 0;
  (void)carve_binned(nullptr, n_prims ? n_prims : 1u, &total);
  return total;
}

hipError_t launch_binned_build(const drt_prim* d_prims, uint32_t n, void* d_scratch, drt_bvh_node* d_nodes,
                               uint32_t* d_order, uint32_t* d_info, uint32_t* h_count, hipStream_t st) {
  if (!d_prims || !d_scratch || !d_nodes || !d_order || !d_info || !h_count || n == 0 || n > (1u << 26))
    return hipErrorInvalidValue;
  const BinnedArena B = carve_binned(d_scratch, n, nullptr);
  const uint32_t per_prim = div_up(n, kThreads), n_tiles = div_up(n, kTile);
  const size_t clear = std::max<size_t>((size_t)B.level_cap * kNodeBinWords, std::max<size_t>(2 * (size_t)n, kCtlWords));
  DRT_LAUNCH(binned_clear, div_up(clear, kThreads), n, B, d_info);
  DRT_LAUNCH(binned_bounds, per_prim, d_prims, n, B);
  DRT_LAUNCH(binned_root, 1, n, B);
  // level-wise rounds; the level's node count is bounded by 2^round and by the arena's level capacity
  int round = 0;
  h_count[0] = n > kLiveMin ? 1u : 0u;
  while (h_count[0] != 0u && round < kBinnedMaxRounds) {
    for (int b = 0; b < kBinnedBatch && round < kBinnedMaxRounds; b++, round++) {
      const uint32_t level = round < 26 ? std::min(B.level_cap, 1u << round) : B.level_cap;
      DRT_LAUNCH(binned_bin, n_tiles, n, B, round);
      DRT_LAUNCH(binned_split, div_up(level, 4), B, round);
      DRT_LAUNCH(binned_flags, n_tiles, n, B, round);
      DRT_LAUNCH(binned_scan, 1, n, n_tiles, B, round, d_info);
      DRT_LAUNCH(binned_scatter, n_tiles, n, B, round);
    }
    if (const hipError_t e = hipMemcpyAsync(h_count, B.ctl + kCtlLive, sizeof(uint32_t), hipMemcpyDeviceToHost, st)) return e;
    if (const hipError_t e = hipStreamSynchronize(st)) return e;
  }
  if (h_count[0] != 0u) return hipSuccess;  // deeper than kBinnedMaxRounds levels: the caller refuses the tree
  const int sel = round & 1;
  // {wave-finished nodes, big leaves, -, -} and the node ids given out
  if (const hipError_t e = hipMemcpyAsync(h_count + 1, B.ctl + kCtlWaveCount, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st)) return e;
  if (const hipError_t e = hipMemcpyAsync(h_count + 3, B.ctl + kCtlLevel + round + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st)) return e;
  if (const hipError_t e = hipStreamSynchronize(st)) return e;
  const uint32_t n_list = h_count[1], n_big = h_count[2], n_ids = h_count[3];
  if (n_list > n || n_ids == 0u || n_ids > 2 * n - 1) return hipErrorUnknown;  // (counts the rounds cannot give)
  if (n_list) DRT_LAUNCH(binned_wave, div_up(n_list, 4), n, n_list, B, sel, d_order);
  for (int level = round; level >= 0; level--) {  // level `round`: the children the last round made
    const uint32_t width = level < 26 ? std::min(B.level_cap, 1u << level) : B.level_cap;
    DRT_LAUNCH(binned_inner_counts, div_up(width, kThreads), n_ids, B, level);
  }
  DRT_LAUNCH(binned_emit, div_up(n_ids, kThreads), n, n_ids, B, d_nodes, d_info);
  DRT_LAUNCH(binned_emit_wave, div_up(2 * (uint64_t)n, kThreads), n, n_ids, B, sel, d_nodes);
  if (n_big) {
    DRT_LAUNCH(binned_big_keys, per_prim, n, n_ids, B, sel, d_order);
    for (int pass = 0; pass < 8; pass++) {
      DRT_LAUNCH(binned_sort_count, n_tiles, n, n_tiles, pass, B);
      DRT_LAUNCH(binned_sort_scan, 1, n_tiles, B);
      DRT_LAUNCH(binned_sort_scatter, n_tiles, n, n_tiles, pass, B, pass == 7 ? d_order : B.pay[(pass & 1) ^ 1]);
    }
  }
  return hipSuccess;
}

}  // namespace drt
