// drt_cell_tree.hip — the Grid scene's shadow queries on a tree of cell boxes (cell_tree_stream).
//
// Grid::Traverse(Ray&) (grid.cpp:309-358) answers: occluded <=> some object listed in a cell the DDA
// visits between the ray's start and the grid's exit reports a hit with t < |L|.  There is no range
// cut per cell, and Grid::Build lists each object in a whole box of cells (grid.cpp:78-92), so the walk
// tests object P exactly when the ray crosses P's cell box.  The kernel walks a 4-ary tree over those
// cell boxes (drt_layout.hpp CellNodeRecord; built by drt_upload_grid_shadow_bvh) with the ray moved
// into cell space once per query, tests each primitive with the walk's own arithmetic, and classifies
// a reported hit by how the ray crosses that primitive's cell box:
//   decisive   the ray passes [lo + m, hi + 1 - m] at some t >= 0: the DDA enters a listing cell, so
//              the walk tests P and finds this same hit — occluded;
//   outside    the ray fails [lo - m, hi + 1 + m]: the walk cannot test P — the hit is ignored;
//   undecided  otherwise: the query goes to the Grid walk (A.fb_rays, grid_stream) unless another
//              primitive decides it.
// Inner boxes are unions of their primitives' boxes and are tested grown by m, so a subtree is skipped
// only when every primitive in it would be classified outside.
//
// Error bound.  u = 2^-24, n = the largest grid dimension, m = S.gmargin = 256 u K n (scene_args; K >= 1
// the grid's coordinates over its width).  A lane walks the tree only if its cell-space origin o' lies
// in [-n_a, 2 n_a] on every axis (R = 2 n bounds |o'|) and its direction is finite; the others (NaNs,
// infinities, far origins) go to the Grid walk.
//   o'  = fl(fl(o - gmin) * g), g = fl(n / w): within 3.01 u R of the real cell coordinate;
//   1/d'= fl(1 / fl(d * g)): relative error 3.01 u;
//   a slab value fl(fl(P - fl(o' +- m')) * 1/d'), P an integer <= 1024 and m' = m or 1 + m: the shifted
//   origin adds u (R + 2), the difference and the product 2 u relative to |P - o'| <= n + R + 2.
// So each slab value is the exact parameter at which the real ray crosses a plane displaced by at most
// s = 4.02 u R + 5.02 u (n + R + 2) < 24 u n = 12 * 2^-23 n cells, and the comparisons among the six
// values of a box are exact: a computed test is the real ray's test against a box whose planes moved by
// less than s.  grid_certificate bounds the DDA's own deviation by 16 * 2^-23 K n cells for origins inside
// the grid; an origin up to one grid width outside doubles the magnitudes it rounds: 32 * 2^-23 K n.
// Together under 44 * 2^-23 K n against m = 128 * 2^-23 K n.
#include <algorithm>

#include "drt_stream.hpp"

namespace drt {

namespace {

typedef __attribute__((address_space(3))) uint8_t LdsByte;
typedef __attribute__((address_space(3))) uint32_t LdsU32;

enum CellFlag : uint32_t {
  CF_TRAV = 1u,   // still walking the tree
  CF_HIT = 2u,    // occluded: a decisive hit, or the ray misses the grid box (grid.cpp:323)
  CF_UNDEC = 4u,  // an undecided hit, or a ray the tree does not take: the Grid walk answers
  CF_POP = 8u     // the visit gave no next node
};

struct CellLane {
  uint32_t item, fl, cur, spa;
  V3 o, d;    // the query as Grid::Traverse(Ray&) takes it (unit d)
  V3 co, ci;  // cell space: origin, reciprocal direction
  float thr;
};

// per-lane counters of a stats build, and the drt_frame_stats slots they add to
enum { CS_SHADOW, CS_RAYS, CS_INNER, CS_LEAF, CS_PRIMS, CS_VERIFY, CS_GRIDFB, CS_ITERS, CS_COUNT };
__device__ const int kCellStatSlot[CS_COUNT] = {ST_SHADOW, ST_W_RAYS,   ST_W_INNER,  ST_W_LEAF,
                                                ST_W_PRIMS, ST_W_VERIFY, ST_W_GRIDFB, ST_WAVE_NODE_ITERS};

// The ray against the cell box [lo - g, hi + 1 + g] (lo / hi packed, drt_layout.hpp), from the origin
// shifted once per step: olo = o' + g, ohi = o' - (1 + g).  Crossed at some t >= 0.  A zero direction
// component has an infinite reciprocal: both slab values are then infinite, of opposite signs (no
// constraint) when the origin lies strictly between the planes and of one sign (no crossing) when outside;
// an origin exactly on a plane gives 0 * inf = NaN, which fminf / fmaxf drop, leaving the other plane's
// infinity on both sides: no crossing.  That is the safe answer for both uses — not decisive on the box
// shrunk by m, and outside on the box grown by m, whose planes lie m from the cells that list the object.
__device__ __forceinline__ bool cell_slab(const CellLane& L, V3 olo, V3 ohi, uint32_t lo, uint32_t hi) {
  const float ax = ((float)(lo & 1023u) - olo.x) * L.ci.x, bx = ((float)(hi & 1023u) - ohi.x) * L.ci.x;
  const float ay = ((float)((lo >> 10) & 1023u) - olo.y) * L.ci.y, by = ((float)((hi >> 10) & 1023u) - ohi.y) * L.ci.y;
  const float az = ((float)(lo >> 20) - olo.z) * L.ci.z, bz = ((float)(hi >> 20) - ohi.z) * L.ci.z;
  const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
  const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
  return t0 <= t1 && t1 >= 0.0f;
}

// One Object::hit of a leaf with the walk's arithmetic (grid.cpp:338-342), and the crossing of a hit's
// cell box.  Returns the lane's flags.
template <bool TRI_ONLY, bool STATS>
__device__ __forceinline__ uint32_t cell_leaf_test(const CellLane& L, float m, const float4& q0, const float4& q1,
                                                   const float4& q2, uint32_t fl, uint32_t* cs) {
  if (STATS) cs[CS_PRIMS]++;
  RayP r;
  r.o = L.o;
  r.d = L.d;
  r.ix = r.iy = r.iz = 0.0f;  // (no primitive test reads the slab constants)
  float t;
  if (!hit_prim_rec<TRI_ONLY>(q0, q1, q2, r, t) || !(t < L.thr)) return fl;
  if (STATS) cs[CS_VERIFY]++;
  const uint32_t lo = __float_as_uint(q1.w), hi = __float_as_uint(q2.w);
  const float in = 1.0f - m, out = 1.0f + m;
  if (cell_slab(L, mk(L.co.x - m, L.co.y - m, L.co.z - m), mk(L.co.x - in, L.co.y - in, L.co.z - in), lo, hi))
    return (fl | CF_HIT) & ~CF_TRAV;  // decisive
  if (!cell_slab(L, mk(L.co.x + m, L.co.y + m, L.co.z + m), mk(L.co.x - out, L.co.y - out, L.co.z - out), lo, hi))
    return fl;  // outside
  return fl | CF_UNDEC;
}

}  // namespace

// One shadow query per lane, wave64; lanes refilled as trace_stream refills them (a 256-query claim per
// wave and atomic, XCD partitions, TraceArgs::sparse 0 and 2), the answer to the query's own slot.
// S carries the Grid and, in prims / wnodes / wroot / big_leaves, the cell tree.  A step loads three
// 16-B slots: an inner node's four boxes and descriptors, or one primitive record of a leaf (the rest
// of the leaf is itself a leaf descriptor).  Any-hit: no order, 4-B stack entries, the stack in LDS as
// [entry][thread] rows with the overflow in scratch.
template <bool TRI_ONLY, int WAVES, bool STATS>
__global__ void __launch_bounds__(kPBlock, WAVES) cell_tree_stream(SceneArgs S, TraceArgs A) {
  constexpr int CAP = 2 * lds_cap(WAVES);  // 4-B entries in the rows of lds_cap(WAVES) 8-B ones
  constexpr uint32_t kLds = (uint32_t)CAP * kRowBytes;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_bytes[];
  LdsByte* lds = (LdsByte*)lds_bytes;
  uint32_t ov[kWideMaxStack - CAP];
  uint32_t cs[CS_COUNT];
  for (int s = 0; s < CS_COUNT; s++) cs[s] = 0;
  CellLane L;
  L.item = kNoItem;
  L.fl = 0u;
  L.spa = threadIdx.x * 4u;
  const uint32_t lane = threadIdx.x & 63u;
  const float m = S.gmargin;
  const float4* __restrict__ nodes = S.wnodes;
  const float4* __restrict__ prims = S.prims;
  uint32_t chunk_next = 0, chunk_end = 0, chunk_base = 0, chunk_cnt = 0;  // wave-uniform (as trace_stream)
  bool exhausted = false;
  uint32_t part = A.parts > 1 ? (__builtin_amdgcn_s_getreg(GETREG_IMMED(3, 0, 20)) & 7u) % (uint32_t)A.parts : 0u;
  uint32_t parts_done = 0;
  while (true) {
    const uint64_t idle = __ballot(L.item == kNoItem);
    const int n_idle = __popcll(idle);
    if (n_idle >= A.refill_min || n_idle == 64) {
      while (chunk_next >= chunk_end && !exhausted) {  // claim 256 query slots of the wave's partition
        const uint32_t pbeg = part * A.part_len, pend = min(pbeg + A.part_len, A.n);
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(A.counter + 16u * part, kTraceChunk);
        base = __shfl(base, 0, 64) + pbeg;
        chunk_base = base;
        chunk_next = chunk_end = 0;
        if (A.sparse != 2) {  // dense queries
          chunk_end = base < pend ? min(base + kTraceChunk, pend) - base : 0u;
        } else if (base < pend) {  // compact queries: the chunk's four group counts (one row of the array)
          const uint32_t row = base / A.band, o0 = base - row * A.band, bl = row / (uint32_t)A.pairs;
          chunk_cnt = *(const uint32_t*)(A.cnt + (size_t)bl * (A.band >> 6) + (o0 >> 6));
          chunk_end = (chunk_cnt & 0xffu) + ((chunk_cnt >> 8) & 0xffu) + ((chunk_cnt >> 16) & 0xffu) + (chunk_cnt >> 24);
        }
        if (base + kTraceChunk >= pend) {
          part = part + 1u == (uint32_t)A.parts ? 0u : part + 1u;
          if (++parts_done == (uint32_t)A.parts) exhausted = true;
        }
      }
      if (L.item == kNoItem) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        const uint32_t it = chunk_next + rank;
        if (it < chunk_end) {
          uint32_t qs = chunk_base + it;
          if (A.sparse == 2) {  // the it-th query of the chunk: group j's (it - its first query)-th slot
            const uint32_t p1 = chunk_cnt & 0xffu, p2 = p1 + ((chunk_cnt >> 8) & 0xffu), p3 = p2 + ((chunk_cnt >> 16) & 0xffu);
            const uint32_t j = (it >= p1 ? 1u : 0u) + (it >= p2 ? 1u : 0u) + (it >= p3 ? 1u : 0u);
            const uint32_t pre = j == 0u ? 0u : (j == 1u ? p1 : (j == 2u ? p2 : p3));
            qs = chunk_base + 64u * j + (it - pre);
          }
          const size_t at = (size_t)qs * (uint32_t)A.stride;
          const float4 a = A.rays[at], b = A.rays_b[at];
          L.item = A.sparse == 2 ? __float_as_uint(b.w) : qs;
          const RayP q = make_ray(mk(a.x, a.y, a.z), mk(b.x, b.y, b.z));
          L.o = q.o;
          L.d = q.d;
          L.thr = a.w;
          // the ray in cell space
          L.co = mk((q.o.x - S.gmin[0]) * S.gscale[0], (q.o.y - S.gmin[1]) * S.gscale[1], (q.o.z - S.gmin[2]) * S.gscale[2]);
          L.ci = mk(1.0f / (q.d.x * S.gscale[0]), 1.0f / (q.d.y * S.gscale[1]), 1.0f / (q.d.z * S.gscale[2]));
          const float nx = (float)S.gdim[0], ny = (float)S.gdim[1], nz = (float)S.gdim[2];
          // (every comparison is false for a NaN; a zero direction component has an infinite reciprocal, which
          // cell_slab takes)
          const bool ok = fabsf(q.d.x) < __builtin_inff() && fabsf(q.d.y) < __builtin_inff() && fabsf(q.d.z) < __builtin_inff() &&
                          L.co.x >= -nx && L.co.x <= 2.0f * nx && L.co.y >= -ny && L.co.y <= 2.0f * ny && L.co.z >= -nz &&
                          L.co.z <= 2.0f * nz;
          // An origin on the grid's boundary is not inside it (grid.cpp:172, a strict test), so the walk starts
          // at the box's entry point, which then lies BEHIND the origin, and tests the objects of the cells
          // back there too.  Origins within m of the boundary go to the walk.
          const bool in_grown = L.co.x >= -m && L.co.x <= nx + m && L.co.y >= -m && L.co.y <= ny + m && L.co.z >= -m &&
                                L.co.z <= nz + m;
          const bool in_shrunk = L.co.x >= m && L.co.x <= nx - m && L.co.y >= m && L.co.y <= ny - m && L.co.z >= m &&
                                 L.co.z <= nz - m;
          const bool missed = grid_box_missed(S, q);
          L.fl = missed ? CF_HIT : ((ok && (in_shrunk || !in_grown)) ? CF_TRAV : CF_UNDEC);
          L.cur = S.wroot;
          L.spa &= kRowBytes - 1u;
          if (STATS) {
            cs[CS_SHADOW]++;
            if (L.fl & CF_TRAV) cs[CS_RAYS]++;
            if ((L.fl & CF_TRAV) && desc_is_leaf(S.wroot)) cs[CS_LEAF]++;  // (leaf visits are counted where one is entered)
          }
        }
      }
      chunk_next = min(chunk_next + (uint32_t)n_idle, chunk_end);
    }
    const bool in_trav = L.item != kNoItem && (L.fl & CF_TRAV);
    const uint64_t trav = __ballot(in_trav);
    if (STATS && trav && lane == 0) cs[CS_ITERS]++;
    if (in_trav) {
      uint32_t fl = L.fl;
      const uint32_t cur = L.cur;
      const bool leaf = desc_is_leaf(cur);
      const uint32_t first = desc_first(cur), cnt = desc_count(cur);
      if (leaf && cnt == kBigLeaf) {  // an oversized leaf (big-leaf table): all of it in this step
        if (STATS) cs[CS_LEAF]++;
        const uint2 bl = S.big_leaves[first];
        for (uint32_t i = 0; i < bl.y && (fl & CF_TRAV); i++) {
          const float4* rec = prims + 3 * (size_t)(bl.x + i);
          fl = cell_leaf_test<TRI_ONLY, STATS>(L, m, rec[0], rec[1], rec[2], fl, cs);
        }
        fl |= CF_POP;
      } else {
        const float4* rec = leaf ? prims + 3 * (size_t)first : nodes + 3 * (size_t)cur;
        const float4 s0 = rec[0], s1 = rec[1], s2 = rec[2];
        if (leaf) {
          fl = cell_leaf_test<TRI_ONLY, STATS>(L, m, s0, s1, s2, fl, cs);
          if (cnt > 1) L.cur = leaf_desc(first + 1, cnt - 1);
          else fl |= CF_POP;
        } else {
          if (STATS) cs[CS_INNER]++;
          const float out = 1.0f + m;
          const V3 olo = mk(L.co.x + m, L.co.y + m, L.co.z + m), ohi = mk(L.co.x - out, L.co.y - out, L.co.z - out);
          const uint32_t bx[8] = {__float_as_uint(s0.x), __float_as_uint(s0.y), __float_as_uint(s0.z), __float_as_uint(s0.w),
                                  __float_as_uint(s1.x), __float_as_uint(s1.y), __float_as_uint(s1.z), __float_as_uint(s1.w)};
          const uint32_t d[4] = {__float_as_uint(s2.x), __float_as_uint(s2.y), __float_as_uint(s2.z), __float_as_uint(s2.w)};
          bool hk[4];
          int ci = -1;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            hk[k] = cell_slab(L, olo, ohi, bx[2 * k], bx[2 * k + 1]) && d[k] != kCellNoChild;
            ci = (hk[k] && ci < 0) ? k : ci;
          }
          // go on with the first crossed child, push the others in reverse so that pops come in slot order
          uint32_t spa = L.spa;
#pragma unroll
          for (int k = 3; k >= 1; k--) {
            if (hk[k] && k != ci) {
              if (spa < kLds) *(LdsU32*)(lds + spa) = d[k];
              else ov[(spa - kLds) >> kRowShift] = d[k];
              spa += kRowBytes;
            }
          }
          L.spa = spa;
          L.cur = ci <= 0 ? d[0] : (ci == 1 ? d[1] : (ci == 2 ? d[2] : d[3]));
          if (STATS && ci >= 0 && desc_is_leaf(L.cur)) cs[CS_LEAF]++;
          fl |= ci < 0 ? CF_POP : 0u;
        }
      }
      if ((fl & (CF_POP | CF_TRAV)) == (CF_POP | CF_TRAV)) {
        fl &= ~CF_POP;
        if (L.spa < kRowBytes) {
          fl &= ~CF_TRAV;
        } else {
          const uint32_t spa = L.spa - kRowBytes;
          L.spa = spa;
          L.cur = spa < kLds ? *(LdsU32*)(lds + spa) : ov[(spa - kLds) >> kRowShift];
          if (STATS && desc_is_leaf(L.cur)) cs[CS_LEAF]++;
        }
      }
      L.fl = fl & ~CF_POP;
    }
    if (L.item != kNoItem && !(L.fl & CF_TRAV)) {  // query done
      if (!(L.fl & CF_HIT) && (L.fl & CF_UNDEC)) {  // the Grid walk answers it (grid_stream over A.fb_rays)
        const uint32_t k = atomicAdd(A.fb_count, 1u);
        A.fb_rays[2 * (size_t)k] = make_float4(L.o.x, L.o.y, L.o.z, L.thr);
        A.fb_rays[2 * (size_t)k + 1] = make_float4(L.d.x, L.d.y, L.d.z, __uint_as_float(L.item));
        if (STATS) cs[CS_GRIDFB]++;
      } else {
        A.occ_out[L.item] = (uint8_t)((L.fl & CF_HIT) ? 1 : 0);
      }
      L.item = kNoItem;
    } else if (!trav && exhausted && chunk_next >= chunk_end) {
      break;
    }
  }
  if (STATS) {
    for (int s = 0; s < CS_COUNT; s++) {
      unsigned long long v = cs[s];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0 && v) atomicAdd(&A.stats[kCellStatSlot[s]], v);
    }
  }
}

// Batched-query front end of the cell tree: rays n x {ox,oy,oz,dx,dy,dz} -> the records of a Grid shadow
// query, unit direction and range |d| (grid.cpp:313-316, as trace_kernel's).
__global__ void __launch_bounds__(256) cell_prep_kernel(const float* __restrict__ rays, int n, float4* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* rr = rays + 6 * (size_t)i;
  const V3 o = mk(rr[0], rr[1], rr[2]), d = mk(rr[3], rr[4], rr[5]);
  const float len = length(d);
  const V3 u = normalize(d);
  out[2 * (size_t)i] = make_float4(o.x, o.y, o.z, len);
  out[2 * (size_t)i + 1] = make_float4(u.x, u.y, u.z, 0.0f);
}

template <bool T, int W, bool ST>
static void launch_cell_w(const SceneArgs& S, const TraceArgs& A, hipStream_t st) {
  const size_t lds = (size_t)lds_cap(W) * kPBlock * 8;
  static int grid = 0;  // resident blocks across the device (per instantiation)
  if (!grid) {
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)cell_tree_stream<T, W, ST>, kPBlock, lds);
    grid = std::max(1, cus) * std::max(1, per_cu);
  }
  const uint64_t need = ((uint64_t)A.n + kPBlock - 1) / kPBlock;
  const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(need, (uint64_t)grid));
  hipLaunchKernelGGL((cell_tree_stream<T, W, ST>), dim3(blocks), dim3(kPBlock), lds, st, S, A);
}

// S: the Grid's SceneArgs with the cell tree in prims / wnodes / wroot / big_leaves; waves per SIMD 6 or 7
void launch_cell_tree_stream(const SceneArgs& S, const TraceArgs& A, bool tri_only, bool stats, int waves, hipStream_t st) {
  if (tri_only) {
    if (stats) launch_cell_w<true, 7, true>(S, A, st);
    else if (waves <= 6) launch_cell_w<true, 6, false>(S, A, st);
    else launch_cell_w<true, 7, false>(S, A, st);
  } else {
    if (stats) launch_cell_w<false, 7, true>(S, A, st);
    else if (waves <= 6) launch_cell_w<false, 6, false>(S, A, st);
    else launch_cell_w<false, 7, false>(S, A, st);
  }
}
void launch_cell_prep(const float* rays, int n, float4* out, hipStream_t st) {
  hipLaunchKernelGGL(cell_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, st, rays, n, out);
}

}  // namespace drt
