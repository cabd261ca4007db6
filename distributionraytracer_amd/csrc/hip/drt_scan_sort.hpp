// drt_scan_sort.hpp — the building blocks the device builders and commits (drt_bvh_build.hip,
// drt_bvh_commit.hip, drt_grid_build.hip) share: the workgroup shape and the launch macro, the scratch
// slicer, wave and workgroup scans, the wave min / max reduction, and one tile of a stable LSD radix sort.
// Header-only: every translation unit instantiates its own code under its own flags.
//
// No lane waits for another lane, wave or workgroup in any of these: __syncthreads orders one workgroup's LDS
// staging, and nothing here touches global memory another workgroup writes in the same kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace drt {

constexpr int kThreads = 256;  // every kernel's workgroup: four waves of 64
constexpr uint32_t kNone = 0xFFFFFFFFu;
// what one workgroup of a sort, an expansion or a device-wide scan owns: 256 threads x 8
constexpr int kTile = 2048;
constexpr int kPer = kTile / kThreads;
static_assert(kThreads == 4 * 64 && kPer * kThreads == kTile && kPer == 8, "the tile is 4 waves x 8 rounds x 64 lanes");

__host__ __device__ inline size_t align256(size_t x) { return (x + 255u) & ~(size_t)255u; }
inline uint32_t div_up(uint64_t a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }

// Launch on the caller's stream `st` with kThreads per workgroup; the caller returns the launch error.
#define DRT_LAUNCH(kernel, grid, ...)                                           \
  do {                                                                          \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, st, __VA_ARGS__); \
    const hipError_t _e = hipGetLastError();                                    \
    if (_e != hipSuccess) return _e;                                            \
  } while (0)

// Slices one scratch allocation into 256-B aligned arrays; `used` is the bytes taken so far (a null base
// sizes the allocation).
struct ScratchSlicer {
  void* base;
  size_t used = 0;
  template <class T>
  T* take(size_t count) {
    T* p = (T*)((char*)base + used);
    used += align256(sizeof(T) * count);
    return p;
  }
};

// ---- wave and workgroup scans -----------------------------------------------------------------------
// inclusive scan of one value per lane across the wave (cross-lane shifts)
template <class T>
__device__ inline T wave_scan_incl(T v) {
  const int lane = threadIdx.x & 63;
  T inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  return inc;
}

// Exclusive scan of one value per thread over the 256 threads of the workgroup (wave scans, the four wave
// totals through LDS); every thread gets the workgroup's total.
template <class T>
__device__ inline T block_scan_excl(T v, T* wave_tot /* LDS, 4 */, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T inc = wave_scan_incl(v);
  __syncthreads();  // the previous use of wave_tot is over
  if (lane == 63) wave_tot[w] = inc;
  __syncthreads();
  const T t0 = wave_tot[0], t1 = wave_tot[1], t2 = wave_tot[2], t3 = wave_tot[3];
  total = t0 + t1 + t2 + t3;
  const T before = (w > 0 ? t0 : (T)0) + (w > 1 ? t1 : (T)0) + (w > 2 ? t2 : (T)0);
  return before + inc - v;
}

// Exclusive prefix count of one flag per thread over the workgroup: a ballot per wave, the four wave totals
// through LDS (one exchange); every thread gets the workgroup's total.
__device__ inline uint32_t block_flag_scan(bool f, uint32_t* wave_tot /* LDS, 4 words */, uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t m = __ballot(f);
  if (lane == 0) wave_tot[w] = (uint32_t)__popcll(m);
  __syncthreads();
  const uint32_t t0 = wave_tot[0], t1 = wave_tot[1], t2 = wave_tot[2], t3 = wave_tot[3];
  total = t0 + t1 + t2 + t3;
  const uint32_t before = (w > 0 ? t0 : 0u) + (w > 1 ? t1 : 0u) + (w > 2 ? t2 : 0u);
  return before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// block_scan_excl with max in place of +: the largest value of the threads before this one (floor if none)
__device__ inline uint32_t block_max_excl(uint32_t v, uint32_t floor, uint32_t* wave_tot /* LDS, 4 */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if (lane >= d) inc = up > inc ? up : inc;
  }
  uint32_t ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = floor;
  __syncthreads();
  if (lane == 63) wave_tot[w] = inc;
  __syncthreads();
  for (int k = 0; k < w; k++) ex = wave_tot[k] > ex ? wave_tot[k] : ex;
  return ex;
}

// One workgroup: ptr[0 .. n) -> carry + their exclusive scan, in place, 256 at a time; every thread gets
// carry + the sum of all n.
template <class T>
__device__ inline T block_scan_array(T* ptr, uint32_t n, T carry) {
  __shared__ T wave_tot[4];
  for (uint32_t c = 0; c < n; c += kThreads) {
    const uint32_t k = c + threadIdx.x;
    const T v = k < n ? ptr[k] : (T)0;
    T total;
    const T ex = block_scan_excl<T>(v, wave_tot, total);
    if (k < n) ptr[k] = carry + ex;
    carry += total;
  }
  return carry;
}

// the least mn and the greatest mx of the wave, to every lane (cross-lane shuffles)
__device__ inline void wave_min_max(uint32_t& mn, uint32_t& mx) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t omn = __shfl_xor(mn, d, 64), omx = __shfl_xor(mx, d, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
  }
}

// ---- one tile of a stable LSD radix sort, 8-bit digits ----------------------------------------------
// A pass is three kernels over n (key, payload) pairs in n_wg tiles of kTile: count (radix_count_tile), an
// exclusive scan of the digit-major table that the caller chooses, scatter (radix_scatter_tile).
template <class Key>
__device__ inline uint32_t radix_digit(Key key, int pass) { return (uint32_t)((key >> (8 * pass)) & 255u); }

// the digit histogram of workgroup blockIdx.x's tile -> table[digit * n_wg + blockIdx.x]
template <class Key>
__device__ inline void radix_count_tile(const Key* __restrict__ src, uint32_t n, uint32_t n_wg, int pass,
                                        uint32_t* __restrict__ table) {
  __shared__ uint32_t h[256];
  const int t = threadIdx.x;
  h[t] = 0u;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)kTile;
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t i = base + j * kThreads + t;
    if (i < n) atomicAdd(&h[radix_digit(src[i], pass)], 1u);
  }
  __syncthreads();
  table[(size_t)t * n_wg + blockIdx.x] = h[t];
}

// Rank the tile's pairs by digit, stage them in LDS in digit order, write each digit's run contiguously.
// table holds the exclusive scan of the digit-major counts: the first global position of this tile's run of
// each digit.  Stable: wave w owns positions [512 w, 512 w + 512) of the tile and takes them 64 at a time, so
// (wave, round, lane) is ascending position, and ranking in that order keeps equal digits in input order.
// Positions past n hold the key ~Key(0), which takes part in no rank.
template <class Key>
__device__ inline void radix_scatter_tile(const Key* __restrict__ ksrc, const uint32_t* __restrict__ psrc,
                                          Key* __restrict__ kdst, uint32_t* __restrict__ pdst, uint32_t n,
                                          uint32_t n_wg, int pass, const uint32_t* __restrict__ table) {
  __shared__ Key skey[kTile];
  __shared__ uint32_t spay[kTile];
  __shared__ uint32_t wcnt[4][256];  // per wave and digit: pairs ranked so far, then the waves' exclusive prefix
  __shared__ uint32_t dstart[256];   // first staged position of each digit
  __shared__ uint32_t gbase[256];    // first global position of this tile's run of each digit
  __shared__ uint32_t wave_tot[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t base = blockIdx.x * (uint32_t)kTile;
#pragma unroll
  for (int k = 0; k < 4; k++) wcnt[k][t] = 0u;
  __syncthreads();
  Key key[kPer];
  uint32_t pay[kPer], off[kPer];
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kPer; r++) {
    const uint32_t i = base + w * (64 * kPer) + r * 64 + lane;
    const bool valid = i < n;
    key[r] = valid ? ksrc[i] : ~Key(0);
    pay[r] = valid ? psrc[i] : 0u;
    const uint32_t d = radix_digit(key[r], pass);
    uint64_t mask = __ballot(valid);  // the lanes of this wave holding the same digit as this lane
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(bit);
      mask &= bit ? m : ~m;
    }
    const uint32_t prior = wcnt[w][d];
    __syncthreads();  // every lane has read the counter before its digit's first lane advances it
    const uint32_t rank = (uint32_t)__popcll(mask & below);
    if (valid && rank == 0u) wcnt[w][d] = prior + (uint32_t)__popcll(mask);
    __syncthreads();
    off[r] = prior + rank;
  }
  {  // thread t = digit t: the waves' counts -> exclusive prefix over waves; digit starts; global bases
    const uint32_t c0 = wcnt[0][t], c1 = wcnt[1][t], c2 = wcnt[2][t], c3 = wcnt[3][t];
    uint32_t total;
    const uint32_t ex = block_scan_excl<uint32_t>(c0 + c1 + c2 + c3, wave_tot, total);
    wcnt[0][t] = 0u; wcnt[1][t] = c0; wcnt[2][t] = c0 + c1; wcnt[3][t] = c0 + c1 + c2;
    dstart[t] = ex;
    gbase[t] = table[(size_t)t * n_wg + blockIdx.x];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kPer; r++) {
    const uint32_t i = base + w * (64 * kPer) + r * 64 + lane;
    const uint32_t d = radix_digit(key[r], pass);
    const uint32_t pos = dstart[d] + wcnt[w][d] + off[r];
    if (i < n && pos < (uint32_t)kTile) { skey[pos] = key[r]; spay[pos] = pay[r]; }
  }
  __syncthreads();
  const uint32_t count = n - base < (uint32_t)kTile ? n - base : (uint32_t)kTile;
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t i = j * kThreads + t;
    if (i >= count) continue;
    const Key k = skey[i];
    const uint32_t d = radix_digit(k, pass);
    const uint32_t g = gbase[d] + (i - dstart[d]);
    if (g < n) { kdst[g] = k; pdst[g] = spay[i]; }
  }
}

}  // namespace drt
