// drt_grid_build.hip — the uniform grid of the resident primitives, built and committed on the device
// (drt_build_grid_device).  The lists are Grid::Build's (drt_accel.cpp, grid.cpp:30-97) bit for bit: the same
// object boxes, the same float arithmetic for the cell ranges, each cell's objects in insertion order.
//
//   grid_bounds        one lane per object: its box (prim_bounds, as the BVH builder) and the world box — min /
//                      max across the wave (wave_min_max), then one ordered-uint atomic per wave and axis
//   (host)             the grown box and nx, ny, nz with glibc's pow (grid_dims, include/drt_scene.hpp)
//   grid_ranges        one lane per object: its six cell indices (24 B) and its 64-bit cell count; the
//                      workgroup's exclusive scan of the counts and its total
//   grid_scan_blocks   one workgroup: exclusive scan of the workgroup totals, the number of references
//   grid_offsets       every object's first reference slot
//   grid_expand        balanced by reference: a workgroup owns kGridTile reference slots.  It finds the tile's
//                      first and last object by binary search in the offsets, the objects that start inside the
//                      tile mark their first slot in LDS, a max-scan over the slots gives every slot its object,
//                      and each lane decodes its slot into (object, ix, iy, iz): a (cell, object) pair in object
//                      order, and the cell's count
//   grid_sort_*        stable LSD radix sort of the pairs by cell, 8-bit digits, only the passes n_cells needs:
//                      the tile of drt_scan_sort.hpp that bvh_sort_* runs on 64-bit keys (rank in LDS, each
//                      digit's run written contiguously).  Stable, and an object lists a cell once: every
//                      cell's run comes out in ascending object index, Grid::Build's insertion order
//   grid_scan_*        device-wide exclusive scan (tile sums, scan of the sums, write): the cell counts ->
//                      cell_start, every cell written; a pass's digit table -> its scatter bases; the commit's
//                      padded cell counts -> tpos
//   grid_commit_prims  the scene-order 48-B records, packed as pack_prim does
//   grid_commit_refs   one lane per reference: its inline record (40 B in pairs for triangle scenes, 48 B
//                      otherwise); a cell's first reference sets the cell's macro-cell bit
//
// No lane waits for another lane, wave or workgroup: stages are kernel boundaries on one stream, the only
// cross-workgroup traffic inside a kernel is atomic adds / ors / mins / maxes of integers whose results no one
// polls (so the outcome does not depend on their order).  __syncthreads orders one workgroup's LDS staging.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "drt_grid_build.hpp"
#include "drt_prim_device.hpp"
#include "drt_scan_sort.hpp"

namespace drt {

namespace {

// reference slots one expansion workgroup owns, pairs one sort workgroup ranks (8 KB of keys + 8 KB of values
// + 6 KB of counters in LDS), values one scan workgroup scans
constexpr int kGridTile = kTile;

struct ObjArena {
  float4* pbox;        // 2 per object, scene order: (min, 0), (max, 0)
  uint64_t* local;     // per object: exclusive scan of the cell counts within its workgroup
  uint64_t* blocks;    // per workgroup of grid_ranges: its total, then its exclusive prefix
  uint32_t* off;       // n + 1: every object's first reference slot, the number of references
};

struct RefArena {
  uint32_t* key[2];    // cell index per reference slot
  uint32_t* val[2];    // object per reference slot
  uint32_t* table;     // 256 x n_wg digit counts, digit-major, + 1: scanned in place
  uint32_t* sums;      // tile sums of a device-wide scan
};

ObjArena carve_obj(void* scratch, uint32_t n, size_t* total) {
  ScratchSlicer s{scratch};
  ObjArena a;
  a.pbox = s.take<float4>(2 * (size_t)n);
  a.local = s.take<uint64_t>(n);
  a.blocks = s.take<uint64_t>(div_up(n, kThreads) + 1);
  a.off = s.take<uint32_t>((size_t)n + 1);
  if (total) *total = s.used;
  return a;
}

RefArena carve_refs(void* scratch, uint32_t n_refs, size_t* total) {
  const size_t r = n_refs ? n_refs : 1u, n_wg = div_up(r, kGridTile);
  ScratchSlicer s{scratch};
  RefArena a;
  a.key[0] = s.take<uint32_t>(r);
  a.key[1] = s.take<uint32_t>(r);
  a.val[0] = s.take<uint32_t>(r);
  a.val[1] = s.take<uint32_t>(r);
  a.table = s.take<uint32_t>(256 * n_wg + 1);
  a.sums = s.take<uint32_t>((size_t)(1u << 20) + 2);  // a scan of up to 2^31 values has up to 2^20 tiles
  if (total) *total = s.used;
  return a;
}

// radix passes of 8 bits that order cell indices below n_cells; the sorted pairs end in buffer passes & 1
inline int sort_passes(uint64_t n_cells) {
  int p = 0;
  while (p < 4 && ((n_cells - 1) >> (8 * p)) != 0) p++;
  return p;
}

// ---- stage 1: object boxes, world box ---------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void grid_clear_status(GridBuildStatus* status) {
  const int t = threadIdx.x;
  uint32_t* w = (uint32_t*)status;
  if (t < 16) w[t] = t < 3 ? 0xFFFFFFFFu : 0u;  // min: above every float; max: below every float
}

__global__ __launch_bounds__(kThreads) void grid_bounds(const drt_prim* __restrict__ prims, uint32_t n, ObjArena A,
                                                        GridBuildStatus* status) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
  const bool valid = i < n;
  bool bad = false;
  if (valid) {
    prim_bounds(prims[i], lo, hi);
    A.pbox[2 * (size_t)i] = make_float4(lo[0], lo[1], lo[2], 0.f);
    A.pbox[2 * (size_t)i + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
#pragma unroll
    for (int a = 0; a < 3; a++) bad = bad || !finite(lo[a]) || !finite(hi[a]);
  }
  // AABB::extend keeps the least min and the greatest max: exact, whatever the order
#pragma unroll
  for (int a = 0; a < 3; a++) {
    uint32_t mn = valid ? ordered(lo[a]) : 0xFFFFFFFFu, mx = valid ? ordered(hi[a]) : 0u;
    wave_min_max(mn, mx);
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&status->wbox[a], mn);
      atomicMax(&status->wbox[3 + a], mx);
    }
  }
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&status->flags, (uint32_t)kGridNonFinite);
}

// ---- stage 2: cell ranges, reference offsets --------------------------------------------------------
// Grid::Build's range lambda on one coordinate: float subtract, float multiply by (float)nd, float divide
// (correctly rounded), then double: clamp to [0, nd - 1], truncate
__device__ inline int32_t cell_of(float v, float mn, float mx, int32_t nd) {
  const float q = (v - mn) * (float)nd / (mx - mn);
  const double x = (double)q, top = (double)(nd - 1);
  if (x != x) return 0;  // (the host's cast of a NaN is undefined)
  return (int32_t)(x < 0.0 ? 0.0 : (x > top ? top : x));
}

__global__ __launch_bounds__(kThreads) void grid_ranges(uint32_t n, GridDims g, ObjArena A, int32_t* __restrict__ ranges) {
  __shared__ uint64_t wave_tot[4];
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  uint64_t cnt = 0ull;
  if (i < n) {
    const float4 lo = A.pbox[2 * (size_t)i], hi = A.pbox[2 * (size_t)i + 1];
    int32_t r[6];
    r[0] = cell_of(lo.x, g.bmin[0], g.bmax[0], g.n[0]);
    r[1] = cell_of(lo.y, g.bmin[1], g.bmax[1], g.n[1]);
    r[2] = cell_of(lo.z, g.bmin[2], g.bmax[2], g.n[2]);
    r[3] = cell_of(hi.x, g.bmin[0], g.bmax[0], g.n[0]);
    r[4] = cell_of(hi.y, g.bmin[1], g.bmax[1], g.n[1]);
    r[5] = cell_of(hi.z, g.bmin[2], g.bmax[2], g.n[2]);
#pragma unroll
    for (int k = 0; k < 6; k++) ranges[6 * (size_t)i + k] = r[k];
    if (r[3] >= r[0] && r[4] >= r[1] && r[5] >= r[2])  // (an inverted box is listed nowhere, as on the host)
      cnt = (uint64_t)(r[3] - r[0] + 1) * (uint64_t)(r[4] - r[1] + 1) * (uint64_t)(r[5] - r[2] + 1);
  }
  uint64_t total;
  const uint64_t ex = block_scan_excl<uint64_t>(cnt, wave_tot, total);
  if (i < n) A.local[i] = ex;
  if (threadIdx.x == 0) A.blocks[blockIdx.x] = total;
}

// one workgroup: the workgroup totals -> their exclusive scan in place, the grand total
__global__ __launch_bounds__(kThreads) void grid_scan_blocks(uint32_t n_blocks, ObjArena A, GridBuildStatus* status) {
  const uint64_t total = block_scan_array<uint64_t>(A.blocks, n_blocks, 0ull);
  if (threadIdx.x == 0) status->n_refs = total;
}

// (the words are meaningful once the host has seen n_refs < 2^31)
__global__ __launch_bounds__(kThreads) void grid_offsets(uint32_t n, ObjArena A, const GridBuildStatus* status) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) A.off[i] = (uint32_t)(A.blocks[blockIdx.x] + A.local[i]);
  if (i == n) A.off[n] = (uint32_t)status->n_refs;
}

// ---- stage 3: reference expansion -------------------------------------------------------------------
// the last object whose first slot is <= slot (it holds the slot: its successor starts beyond it)
__device__ inline uint32_t object_of_slot(const uint32_t* __restrict__ off, uint32_t n, uint32_t slot) {
  uint32_t lo = 0u, hi = n;  // off[lo] <= slot < off[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= slot) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void grid_expand(uint32_t n, uint32_t n_refs, GridDims g, ObjArena A,
                                                        const int32_t* __restrict__ ranges, uint32_t* __restrict__ key,
                                                        uint32_t* __restrict__ val, uint32_t* __restrict__ cell_cnt) {
  __shared__ uint32_t obj[kGridTile];  // per slot of the tile: the object that starts there, then its object
  __shared__ uint32_t ends[2];
  __shared__ uint32_t wave_tot[4];
  const int t = threadIdx.x;
  const uint32_t base = blockIdx.x * (uint32_t)kGridTile;
  const uint32_t count = n_refs - base < (uint32_t)kGridTile ? n_refs - base : (uint32_t)kGridTile;
  if (t < 2) ends[t] = object_of_slot(A.off, n, t == 0 ? base : base + count - 1u);
  __syncthreads();
  const uint32_t first = ends[0], last = ends[1];
#pragma unroll
  for (int j = 0; j < kPer; j++) obj[j * kThreads + t] = first;
  __syncthreads();
  // objects that start inside the tile mark their first slot (one without cells owns no slot)
  for (uint32_t o = first + 1u + t; o <= last; o += kThreads) {
    const uint32_t s = A.off[o] - base;
    if (s < count && A.off[o + 1] != A.off[o]) obj[s] = o;
  }
  __syncthreads();
  {  // thread t owns slots 8t .. 8t + 7: running max, then the max of the threads before it
    uint32_t m[kPer];
    uint32_t run = first;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      const uint32_t v = obj[kPer * t + k];
      run = v > run ? v : run;
      m[k] = run;
    }
    const uint32_t ex = block_max_excl(run, first, wave_tot);
#pragma unroll
    for (int k = 0; k < kPer; k++) obj[kPer * t + k] = m[k] > ex ? m[k] : ex;
  }
  __syncthreads();
  const int64_t nx = g.n[0], nxy = (int64_t)g.n[0] * g.n[1];
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t s = j * kThreads + t;
    if (s >= count) continue;
    const uint32_t o = obj[s];
    if (o >= n) continue;  // (cannot happen; keeps the loads in bounds)
    const int32_t* r = ranges + 6 * (size_t)o;
    const uint32_t w = (uint32_t)(r[3] - r[0] + 1), h = (uint32_t)(r[4] - r[1] + 1);
    const uint32_t local = base + s - A.off[o];  // ix fastest, then iy, then iz: Grid::Build's loop order
    const uint32_t row = local / w;
    const int64_t ix = r[0] + (int64_t)(local - row * w), iy = r[1] + (int64_t)(row % h), iz = r[2] + (int64_t)(row / h);
    const int64_t cell = ix + nx * iy + nxy * iz;
    if (cell < 0 || cell >= nxy * g.n[2]) continue;  // (cannot happen; keeps the atomic in bounds)
    key[base + s] = (uint32_t)cell;
    val[base + s] = o;
    atomicAdd(&cell_cnt[cell], 1u);
  }
}

// ---- device-wide exclusive scan ---------------------------------------------------------------------
// kCounts: the values are in[i].  kPadded (the commit's tpos): in is cell_start, the value of cell i is its
// count rounded up to even, and the written word carries in bit 31 whether cell i - 1 ended on a padding slot.
enum ScanMode { kCounts = 0, kPadded = 1 };

template <int MODE>
__device__ inline uint32_t scan_value(const uint32_t* in, uint32_t i) {
  if (MODE == kCounts) return in[i];
  const uint32_t cnt = in[i + 1] - in[i];
  return cnt + (cnt & 1u);
}
template <int MODE>
__device__ inline uint32_t scan_word(const uint32_t* in, uint32_t i, uint32_t ex) {
  if (MODE == kCounts) return ex;
  return ex | (i ? ((in[i] - in[i - 1]) & 1u) << 31 : 0u);
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void grid_scan_reduce(const uint32_t* __restrict__ in, uint32_t n,
                                                             uint32_t* __restrict__ sums) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t base = blockIdx.x * (uint32_t)kGridTile;
  uint32_t s = 0u;
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t i = base + j * kThreads + threadIdx.x;
    if (i < n) s += scan_value<MODE>(in, i);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
}

// one workgroup: the tile sums -> their exclusive scan in place, the total after them and, if asked, in *total_out
__global__ __launch_bounds__(kThreads) void grid_scan_sums(uint32_t* sums, uint32_t n_tiles, uint32_t* total_out) {
  const uint32_t total = block_scan_array<uint32_t>(sums, n_tiles, 0u);
  if (threadIdx.x == 0) {
    sums[n_tiles] = total;
    if (total_out) *total_out = total;
  }
}

// out[i] for every i < n and out[n] = the total.  in == out is allowed for kCounts: a thread reads its eight
// values before the workgroup's barriers and writes the same eight slots after them.
template <int MODE>
__global__ __launch_bounds__(kThreads) void grid_scan_write(const uint32_t* in, uint32_t n, const uint32_t* __restrict__ sums,
                                                            uint32_t n_tiles, uint32_t* out) {
  __shared__ uint32_t wave_tot[4];
  const uint32_t first = blockIdx.x * (uint32_t)kGridTile + kPer * threadIdx.x;  // thread t: eight neighbours
  uint32_t v[kPer], s = 0u;
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    v[k] = first + k < n ? scan_value<MODE>(in, first + k) : 0u;
    s += v[k];
  }
  uint32_t total;
  uint32_t ex = sums[blockIdx.x] + block_scan_excl<uint32_t>(s, wave_tot, total);
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    if (first + k < n) out[first + k] = scan_word<MODE>(in, first + k, ex);
    ex += v[k];
  }
  if (blockIdx.x == n_tiles - 1u && threadIdx.x == 0) out[n] = scan_word<MODE>(in, n, sums[n_tiles]);
}

template <int MODE>
hipError_t device_scan(const uint32_t* in, uint32_t n, uint32_t* sums, uint32_t* out, uint32_t* total_out, hipStream_t st) {
  const uint32_t n_tiles = div_up(n ? n : 1u, kGridTile);
  DRT_LAUNCH(grid_scan_reduce<MODE>, n_tiles, in, n, sums);
  DRT_LAUNCH(grid_scan_sums, 1, sums, n_tiles, total_out);
  DRT_LAUNCH(grid_scan_write<MODE>, n_tiles, in, n, sums, n_tiles, out);
  return hipSuccess;
}

// ---- stable LSD radix sort of (cell, object): the tile of drt_scan_sort.hpp ------------------------
// per-workgroup digit histogram of the tile -> table[digit * n_wg + wg]
__global__ __launch_bounds__(kThreads) void grid_sort_count(const uint32_t* __restrict__ src, uint32_t n, uint32_t n_wg,
                                                            int pass, uint32_t* __restrict__ table) {
  radix_count_tile<uint32_t>(src, n, n_wg, pass, table);
}

// table holds the exclusive scan of the digit-major counts; stable (radix_scatter_tile), so a cell's run
// keeps the expansion's object order
__global__ __launch_bounds__(kThreads) void grid_sort_scatter(const uint32_t* __restrict__ ksrc, const uint32_t* __restrict__ vsrc,
                                                              uint32_t* __restrict__ kdst, uint32_t* __restrict__ vdst, uint32_t n,
                                                              uint32_t n_wg, int pass, const uint32_t* __restrict__ table) {
  radix_scatter_tile<uint32_t>(ksrc, vsrc, kdst, vdst, n, n_wg, pass, table);
}

__global__ __launch_bounds__(kThreads) void grid_copy(const uint32_t* __restrict__ src, uint32_t n, uint32_t* __restrict__ dst) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// ---- commit -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void grid_commit_prims(const float4* __restrict__ raw, uint32_t n, uint32_t default_material,
                                                              float4* __restrict__ prims) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float4 q0, q1, q2;
  pack_prim_record(raw, i, default_material, q0, q1, q2);
  prims[3 * (size_t)i] = q0;
  prims[3 * (size_t)i + 1] = q1;
  prims[3 * (size_t)i + 2] = q2;
}

// One lane per reference, in cell order.  Triangle scenes: the 40-B record (v0, e1, e2, scene index) at slot
// tpos[cell] + (position in the cell), two slots per 80-B pair; the padding slots stay as cleared.  Other
// scenes: the 48-B record with the scene index in q2.w.  A cell's first reference sets its macro-cell's bit.
__global__ __launch_bounds__(kThreads) void grid_commit_refs(GridCommitArgs a, const uint32_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n_refs) return;
  const uint32_t o = a.cell_objs[i], cell = keys[i];
  if (o >= a.n_prims) return;  // (cannot happen; keeps the loads in bounds)
  const uint32_t start = a.cell_start[cell];
  const float4* p = (const float4*)a.prims + 3 * (size_t)o;
  const float4 q0 = p[0], q1 = p[1], q2 = p[2];
  if (a.tris) {
    const uint32_t at = (a.tpos[cell] & 0x7FFFFFFFu) + (i - start);
    float2* f = (float2*)(a.tris + (size_t)(at >> 1) * 20 + (at & 1u) * 10);  // 40 B apart: 8-B aligned
    f[0] = make_float2(q0.x, q0.y);
    f[1] = make_float2(q0.z, q1.x);
    f[2] = make_float2(q1.y, q1.z);
    f[3] = make_float2(q2.x, q2.y);
    f[4] = make_float2(q2.z, __uint_as_float(o));
  } else {
    float4* r = (float4*)a.recs + 3 * (size_t)i;
    r[0] = q0;
    r[1] = q1;
    r[2] = make_float4(q2.x, q2.y, q2.z, __uint_as_float(o));
  }
  if (i == start) {
    const uint32_t nx = (uint32_t)a.g.n[0], ny = (uint32_t)a.g.n[1];
    const uint32_t x = cell % nx, y = (cell / nx) % ny, z = cell / (nx * ny);
    const size_t mi = (size_t)(x >> a.macro_shift) + (size_t)a.macro_dim[0] * (y >> a.macro_shift) +
                      (size_t)a.macro_dim[0] * a.macro_dim[1] * (z >> a.macro_shift);
    atomicOr(&a.macro[mi >> 5], 1u << (mi & 31));
  }
}

}  // namespace

size_t grid_object_scratch_bytes(uint32_t n_prims) {
  size_t total = 0;
  (void)carve_obj(nullptr, n_prims ? n_prims : 1u, &total);
  return total;
}

size_t grid_refs_scratch_bytes(uint32_t n_refs) {
  size_t total = 0;
  (void)carve_refs(nullptr, n_refs, &total);
  return total;
}

hipError_t launch_grid_bounds(const drt_prim* d_prims, uint32_t n, void* obj_scratch, GridBuildStatus* status,
                              hipStream_t st) {
  if (!d_prims || !obj_scratch || !status || n == 0 || n > (1u << 26)) return hipErrorInvalidValue;
  const ObjArena A = carve_obj(obj_scratch, n, nullptr);
  DRT_LAUNCH(grid_clear_status, 1, status);
  DRT_LAUNCH(grid_bounds, div_up(n, kThreads), d_prims, n, A, status);
  return hipSuccess;
}

hipError_t launch_grid_ranges(uint32_t n, const GridDims& g, void* obj_scratch, int32_t* ranges, GridBuildStatus* status,
                              hipStream_t st) {
  if (!obj_scratch || !ranges || !status || n == 0 || n > (1u << 26)) return hipErrorInvalidValue;
  const ObjArena A = carve_obj(obj_scratch, n, nullptr);
  const uint32_t n_blocks = div_up(n, kThreads);
  DRT_LAUNCH(grid_ranges, n_blocks, n, g, A, ranges);
  DRT_LAUNCH(grid_scan_blocks, 1, n_blocks, A, status);
  DRT_LAUNCH(grid_offsets, div_up((uint64_t)n + 1, kThreads), n, A, status);
  return hipSuccess;
}

hipError_t launch_grid_lists(uint32_t n, const GridDims& g, uint32_t n_refs, const void* obj_scratch, const int32_t* ranges,
                             void* refs_scratch, uint32_t* cell_start, uint32_t* cell_objs, hipStream_t st) {
  const uint64_t n_cells = (uint64_t)g.n[0] * g.n[1] * g.n[2];
  if (!obj_scratch || !ranges || !refs_scratch || !cell_start || !cell_objs || n == 0 || n_refs >= (1u << 31) ||
      n_cells == 0 || n_cells >= (1ull << 31))
    return hipErrorInvalidValue;
  const ObjArena A = carve_obj(const_cast<void*>(obj_scratch), n, nullptr);
  const RefArena R = carve_refs(refs_scratch, n_refs, nullptr);
  hipError_t e = hipMemsetAsync(cell_start, 0, 4 * (n_cells + 1), st);
  if (e != hipSuccess) return e;
  if (n_refs > 0) {
    const uint32_t n_wg = div_up(n_refs, kGridTile);
    DRT_LAUNCH(grid_expand, n_wg, n, n_refs, g, A, ranges, R.key[0], R.val[0], cell_start);
    const int passes = sort_passes(n_cells);
    for (int pass = 0; pass < passes; pass++) {
      const int s = pass & 1;
      DRT_LAUNCH(grid_sort_count, n_wg, R.key[s], n_refs, n_wg, pass, R.table);
      e = device_scan<kCounts>(R.table, 256u * n_wg, R.sums, R.table, nullptr, st);
      if (e != hipSuccess) return e;
      DRT_LAUNCH(grid_sort_scatter, n_wg, R.key[s], R.val[s], R.key[s ^ 1], R.val[s ^ 1], n_refs, n_wg, pass, R.table);
    }
    DRT_LAUNCH(grid_copy, div_up(n_refs, kThreads), R.val[passes & 1], n_refs, cell_objs);
  }
  return device_scan<kCounts>(cell_start, (uint32_t)n_cells, R.sums, cell_start, nullptr, st);
}

hipError_t launch_grid_commit_tpos(const GridCommitArgs& a, hipStream_t st) {
  const uint64_t n_cells = (uint64_t)a.g.n[0] * a.g.n[1] * a.g.n[2];
  if (!a.cell_start || !a.tpos || !a.refs_scratch || !a.status || n_cells == 0 || n_cells >= (1ull << 31))
    return hipErrorInvalidValue;
  const RefArena R = carve_refs(a.refs_scratch, a.n_refs, nullptr);
  return device_scan<kPadded>(a.cell_start, (uint32_t)n_cells, R.sums, a.tpos, &a.status->scan_total, st);
}

hipError_t launch_grid_commit(const GridCommitArgs& a, hipStream_t st) {
  const uint64_t n_cells = (uint64_t)a.g.n[0] * a.g.n[1] * a.g.n[2];
  if (!a.prims_raw || !a.prims || !a.cell_start || !a.cell_objs || !a.refs_scratch || !a.macro || a.n_prims == 0 ||
      (a.tris ? !a.tpos : !a.recs) || n_cells == 0 || n_cells >= (1ull << 31))
    return hipErrorInvalidValue;
  const RefArena R = carve_refs(a.refs_scratch, a.n_refs, nullptr);
  DRT_LAUNCH(grid_commit_prims, div_up(a.n_prims, kThreads), (const float4*)a.prims_raw, a.n_prims, a.default_material,
              (float4*)a.prims);
  if (a.n_refs > 0)
    DRT_LAUNCH(grid_commit_refs, div_up(a.n_refs, kThreads), a, (const uint32_t*)R.key[sort_passes(n_cells) & 1]);
  return hipSuccess;
}

}  // namespace drt
