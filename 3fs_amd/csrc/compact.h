// compact.h -- a stable compaction of the records of a table that satisfy a predicate, in index
// order: the table is cut into contiguous shares, one per workgroup of 256 threads; a count pass
// leaves the listed records of every share, one workgroup turns the counts into offsets, and a
// scatter pass writes each share's records from its offset on.  The passes are separate launches;
// no workgroup waits for another.  forward_kernels.hip builds its commit list with it.  It is the
// scheme of sync_kernels.hip's write and remove lists, which keep their own, older statement of it:
// moved onto these helpers their kernels compile to other device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hf3fs_crc {

// Workgroup b owns [b * per, min(n, (b + 1) * per)): at most max_blocks shares, each a multiple of
// 256 records.
struct Shares {
  uint32_t blocks;
  uint64_t per;
};
__host__ __device__ inline Shares shares_of(uint64_t n, uint32_t max_blocks) {
  const uint64_t tiles = (n + 255) / 256;
  Shares s;
  s.blocks = (uint32_t)(tiles < max_blocks ? (tiles ? tiles : 1) : max_blocks);
  s.per = (tiles + s.blocks - 1) / s.blocks * 256;
  return s;
}

// One workgroup of 256 threads: cnt[0, nb) (nb <= 2048, eight entries per thread) becomes its
// exclusive sums.  sums: 256 shared words.  Returns the inclusive sum up to and including the
// calling thread's entries (thread 255: the total).  The caller synchronises before sums is reused.
__device__ __forceinline__ uint32_t compact_scan_counts(uint32_t* cnt, const uint32_t nb, uint32_t* sums) {
  uint32_t v[8], total = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t at = threadIdx.x * 8 + k;
    v[k] = at < nb ? cnt[at] : 0u;
    total += v[k];
  }
  sums[threadIdx.x] = total;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {  // inclusive scan of the 256 thread totals
    const uint32_t add = threadIdx.x >= d ? sums[threadIdx.x - d] : 0u;
    __syncthreads();
    sums[threadIdx.x] += add;
    __syncthreads();
  }
  const uint32_t upto = sums[threadIdx.x];
  uint32_t run = upto - total;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t at = threadIdx.x * 8 + k;
    if (at < nb) cnt[at] = run;
    run += v[k];
  }
  return upto;
}

// One workgroup of 256 threads walks its share [lo, hi) in tiles of 256: each record i with
// take(i) lands at base + (taken records before it in the share); at < n is the list's capacity.
// wave_n: four shared words.
template <class Take>
__device__ __forceinline__ void compact_scatter_share(const Take take, const uint64_t lo, const uint64_t hi,
                                                      uint64_t base, uint32_t* __restrict__ list, const uint64_t n,
                                                      uint32_t* wave_n) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t i0 = lo; i0 < hi; i0 += 256) {  // workgroup-uniform
    const uint64_t i = i0 + threadIdx.x;
    const bool mine = i < hi && take(i);
    const unsigned long long votes = __ballot(mine);
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(votes);
    __syncthreads();
    uint32_t before = 0, tile = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t c = wave_n[w];
      before += w < wave ? c : 0u;
      tile += c;
    }
    const uint64_t at = base + before + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
    if (mine && at < n) list[at] = (uint32_t)i;
    base += tile;
    __syncthreads();
  }
}

// The same walk for a list of records of any kind: place(i, at, taken) is called for every record
// i of the share, `at` the taken records before it (from base on) and so, for a taken record, its
// place in the list.  hf3fs_crc_server_read_complete builds its RDMA write list with it and keeps
// every record's `at` for the per-request first / count.
template <class Take, class Place>
__device__ __forceinline__ void compact_place_share(const Take take, const uint64_t lo, const uint64_t hi,
                                                    uint64_t base, const Place place, uint32_t* wave_n) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t i0 = lo; i0 < hi; i0 += 256) {  // workgroup-uniform
    const uint64_t i = i0 + threadIdx.x;
    const bool mine = i < hi && take(i);
    const unsigned long long votes = __ballot(mine);
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(votes);
    __syncthreads();
    uint32_t before = 0, tile = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t c = wave_n[w];
      before += w < wave ? c : 0u;
      tile += c;
    }
    const uint64_t at = base + before + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
    if (i < hi) place(i, at, mine);
    base += tile;
    __syncthreads();
  }
}

}  // namespace hf3fs_crc
