// sync_kernels.hip -- see sync_kernels.h.  These kernels only read and write 48-byte metadata
// records, 4-byte indices and 1-byte class codes; no chunk byte is touched.
//
// Who writes what (one launch per line; a word has one writer per launch, or only atomics):
//   clear     every table slot and claim word = kSyncNone, ctl[0] = kSyncNone, ctl[1..] = 0
//   insert    table: CAS empty -> i, atomicMin on a slot whose occupant has i's id
//   claim     rfound[r]; claim[rfound[r]] by atomicMin(r)
//   classify  remote r: out_class, out_peer, rcode[r]; lcode[L] of the local record it claimed;
//             ctl[0] by atomicMin over the fatal r.  local i: out_class, out_peer; lcode[i] unless
//             the record is MATCHED (then its one claimer writes it)
//   count     lcount[b], rcount[b] (list entries of workgroup b's contiguous share); ctl[32 + c]
//             by atomicAdd: the class histogram, remote classes over r <= first fatal only
//   scan      lcount / rcount become exclusive sums; every word of d_info (sync_info)
//   scatter   d_write / d_remove, stable: workgroup b writes its share from its offset on
// Nothing is read that an earlier launch of the same call has not written (option poison).
#include "sync_kernels.h"

#include "gf2.h"
#include "sync_plan.h"

namespace hf3fs_crc {
namespace {

constexpr uint8_t kSyncMatchedForward = 31;  // lcode only: MATCHED, and the peer's class forwards

unsigned grid_of(uint64_t n) {
  const uint64_t want = (n + 255) / 256;
  return (unsigned)(want < 4096 ? (want ? want : 1) : 4096);
}

// The count and scatter passes cut a table into contiguous shares, one per workgroup, each a
// multiple of 256 records: workgroup b owns [b * per, min(n, (b + 1) * per)).
struct Shares {
  uint32_t blocks;
  uint64_t per;
};
__host__ __device__ inline Shares shares_of(uint64_t n) {
  const uint64_t tiles = (n + 255) / 256;
  Shares s;
  s.blocks = (uint32_t)(tiles < kSyncBlocksMax ? (tiles ? tiles : 1) : kSyncBlocksMax);
  s.per = (tiles + s.blocks - 1) / s.blocks * 256;
  return s;
}

__global__ __launch_bounds__(256) void k_sync_clear(uint32_t* __restrict__ table, uint32_t* __restrict__ claim,
                                                    uint32_t* __restrict__ ctl, const uint32_t slots,
                                                    const uint64_t n_local) {
  if (blockIdx.x == 0 && threadIdx.x < kSyncCtlWords) ctl[threadIdx.x] = threadIdx.x == 0 ? kSyncNone : 0u;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x) {
    table[i] = kSyncNone;
    if (i < n_local) claim[i] = kSyncNone;  // (slots >= 2 n_local)
  }
}

// Local record i takes the first empty slot of its probe sequence, or joins the slot whose
// occupant has its id: atomicMin leaves the lowest index of the id there.  Slots never empty
// again, so every record of an id ends at the same slot whatever the order of arrival; the
// table holds >= 2 n_local slots for <= n_local ids, so a probe sequence always ends.
__global__ __launch_bounds__(256) void k_sync_insert(const hf3fs_crc_sync_meta* local, const uint64_t n_local,
                                                     uint32_t* __restrict__ table, const uint32_t slots) {
  const uint32_t mask = slots - 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_local;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t hi = local[i].id_hi, lo = local[i].id_lo;
    uint32_t h = sync_hash(hi, lo, mask);
    for (uint32_t probe = 0; probe < slots; ++probe, h = (h + 1) & mask) {
      const uint32_t prev = atomicCAS(&table[h], kSyncNone, (uint32_t)i);
      if (prev == kSyncNone) break;
      if (prev < n_local && local[prev].id_hi == hi && local[prev].id_lo == lo) {
        atomicMin(&table[h], (uint32_t)i);
        break;
      }
    }
  }
}

// The lowest local index with this id, kSyncNone if the table has none.
__device__ __forceinline__ uint32_t sync_find(const hf3fs_crc_sync_meta* local, const uint64_t n_local,
                                              const uint32_t* table, const uint32_t slots, const uint64_t hi,
                                              const uint64_t lo) {
  const uint32_t mask = slots - 1;
  uint32_t h = sync_hash(hi, lo, mask);
  for (uint32_t probe = 0; probe < slots; ++probe, h = (h + 1) & mask) {
    const uint32_t j = table[h];
    if (j == kSyncNone || j >= n_local) return kSyncNone;
    if (local[j].id_hi == hi && local[j].id_lo == lo) return j;
  }
  return kSyncNone;
}

__global__ __launch_bounds__(256) void k_sync_claim(const hf3fs_crc_sync_meta* local, const uint64_t n_local,
                                                    const hf3fs_crc_sync_meta* remote, const uint64_t n_remote,
                                                    const uint32_t* __restrict__ table, const uint32_t slots,
                                                    uint32_t* __restrict__ claim, uint32_t* __restrict__ rfound) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_remote;
       r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t at = sync_find(local, n_local, table, slots, remote[r].id_hi, remote[r].id_lo);
    rfound[r] = at;
    if (at != kSyncNone) atomicMin(&claim[at], (uint32_t)r);
  }
}

// A record's class depends on its own fields, its peer's and the finished claims only: the two
// loops share no written byte (a MATCHED record's lcode belongs to its claimer, its out_class and
// out_peer to the local loop; the ladder reads neither).
__global__ __launch_bounds__(256) void k_sync_classify(hf3fs_crc_sync_meta* local, const uint64_t n_local,
                                                       hf3fs_crc_sync_meta* remote, const uint64_t n_remote,
                                                       const uint32_t chain_ver, const uint32_t flags,
                                                       const uint32_t* __restrict__ table, const uint32_t slots,
                                                       const uint32_t* __restrict__ claim,
                                                       const uint32_t* __restrict__ rfound, uint8_t* lcode,
                                                       uint8_t* __restrict__ rcode, uint32_t* __restrict__ ctl) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_remote; r += stride) {
    const uint32_t at = rfound[r];
    const bool mine = at != kSyncNone && at < n_local && claim[at] == (uint32_t)r;
    const uint8_t cls = sync_classify(mine ? &local[at] : nullptr, remote[r], chain_ver, flags);
    remote[r].out_class = cls;
    remote[r].out_peer = mine ? at : kSyncNone;
    rcode[r] = cls;
    const SyncDisposition d = sync_disposition(cls);
    if (mine) lcode[at] = d == kSyncForward ? kSyncMatchedForward : (uint8_t)HF3FS_SYNC_MATCHED;
    if (d == kSyncFatal) atomicMin(&ctl[0], (uint32_t)r);
  }
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_local; i += stride) {
    const uint32_t first = sync_find(local, n_local, table, slots, local[i].id_hi, local[i].id_lo);
    const uint32_t by = claim[i];
    uint8_t cls = HF3FS_SYNC_MATCHED;
    if (first != (uint32_t)i)
      cls = HF3FS_SYNC_DUPLICATE;
    else if (by == kSyncNone)
      cls = HF3FS_SYNC_REMOTE_MISS;
    local[i].out_class = cls;
    local[i].out_peer = cls == HF3FS_SYNC_MATCHED ? by : kSyncNone;
    if (cls != HF3FS_SYNC_MATCHED) lcode[i] = cls;
  }
}

__device__ __forceinline__ bool in_write_list(uint8_t code) {
  return code == kSyncMatchedForward || code == HF3FS_SYNC_REMOTE_MISS;
}
__device__ __forceinline__ bool in_remove_list(uint8_t code) { return code == HF3FS_SYNC_REMOTE_ONLY; }

// Workgroups [0, lb) count the local table, [lb, lb + rb) the remote one.
__global__ __launch_bounds__(256) void k_sync_count(const uint8_t* __restrict__ lcode, const uint64_t n_local,
                                                    const uint8_t* __restrict__ rcode, const uint64_t n_remote,
                                                    uint32_t* __restrict__ ctl, uint32_t* __restrict__ lcount,
                                                    uint32_t* __restrict__ rcount) {
  __shared__ uint32_t hist[32];
  __shared__ uint32_t listed;
  if (threadIdx.x < 32) hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) listed = 0;
  __syncthreads();
  const Shares ls = shares_of(n_local), rs = shares_of(n_remote);
  const bool is_local = blockIdx.x < ls.blocks;
  const uint32_t b = is_local ? blockIdx.x : blockIdx.x - ls.blocks;
  const uint64_t n = is_local ? n_local : n_remote;
  const uint64_t per = is_local ? ls.per : rs.per;
  const uint8_t* code = is_local ? lcode : rcode;
  const uint64_t lo = (uint64_t)b * per, hi = lo + per < n ? lo + per : n;
  const uint64_t last = is_local ? ~0ull : (uint64_t)ctl[0];  // (the break: remote classes up to the first fatal)
  uint32_t mine = 0;
  for (uint64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const uint8_t c = code[i] & 31;
    if (i <= last) atomicAdd(&hist[c], 1u);
    mine += (is_local ? in_write_list(c) : in_remove_list(c)) ? 1u : 0u;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&listed, mine);
  __syncthreads();
  if (threadIdx.x == 0) (is_local ? lcount : rcount)[b] = listed;
  if (threadIdx.x < 32 && hist[threadIdx.x]) atomicAdd(&ctl[32 + threadIdx.x], hist[threadIdx.x]);
}

// One workgroup: the exclusive sums of both count arrays (kSyncBlocksMax = 256 threads x 8
// entries), then d_info from the histogram.
__global__ __launch_bounds__(256) void k_sync_scan(uint32_t* __restrict__ lcount, const uint32_t lb,
                                                   uint32_t* __restrict__ rcount, const uint32_t rb,
                                                   const uint32_t* __restrict__ ctl, uint32_t* __restrict__ info) {
  static_assert(kSyncBlocksMax == 256 * 8, "k_sync_scan: eight entries per thread");
  __shared__ uint32_t sums[256];
  for (int which = 0; which < 2; ++which) {
    uint32_t* cnt = which ? rcount : lcount;
    const uint32_t nb = which ? rb : lb;
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
    uint32_t run = sums[threadIdx.x] - total;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t at = threadIdx.x * 8 + k;
      if (at < nb) cnt[at] = run;
      run += v[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    uint32_t h[32], out[HF3FS_SYNC_INFO_WORDS];
    for (int c = 0; c < 32; ++c) h[c] = ctl[32 + c];
    sync_info(h, h[kSyncMatchedForward], ctl[0], out);
    for (int w = 0; w < HF3FS_SYNC_INFO_WORDS; ++w) info[w] = out[w];
  }
}

// Stable compaction: workgroup b walks its share in tiles of 256, each listed record lands at
// (b's offset) + (listed records before it in the share).  After a fatal record the reference
// builds no list: nothing is written.
__global__ __launch_bounds__(256) void k_sync_scatter(const uint8_t* __restrict__ lcode, const uint64_t n_local,
                                                      const uint8_t* __restrict__ rcode, const uint64_t n_remote,
                                                      const uint32_t* __restrict__ ctl,
                                                      const uint32_t* __restrict__ lcount,
                                                      const uint32_t* __restrict__ rcount,
                                                      uint32_t* __restrict__ d_write, uint32_t* __restrict__ d_remove) {
  __shared__ uint32_t wave_n[4];
  if (ctl[0] != kSyncNone) return;  // (uniform over the grid)
  const Shares ls = shares_of(n_local), rs = shares_of(n_remote);
  const bool is_local = blockIdx.x < ls.blocks;
  uint32_t* list = is_local ? d_write : d_remove;
  if (!list) return;  // (uniform over the workgroup)
  const uint32_t b = is_local ? blockIdx.x : blockIdx.x - ls.blocks;
  const uint64_t n = is_local ? n_local : n_remote;
  const uint64_t per = is_local ? ls.per : rs.per;
  const uint8_t* code = is_local ? lcode : rcode;
  const uint64_t lo = (uint64_t)b * per, hi = lo + per < n ? lo + per : n;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t base = (is_local ? lcount : rcount)[b];
  for (uint64_t i0 = lo; i0 < hi; i0 += 256) {  // workgroup-uniform
    const uint64_t i = i0 + threadIdx.x;
    bool take = false;
    if (i < hi) {
      const uint8_t c = code[i] & 31;
      take = is_local ? in_write_list(c) : in_remove_list(c);
    }
    const unsigned long long votes = __ballot(take);
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
    if (take && at < n) list[at] = (uint32_t)i;  // (at < listed records <= n: the list's capacity)
    base += tile;
    __syncthreads();
  }
}

// Record k < n_write describes local record d_write[k]; every other record is an empty NONE one.
__global__ __launch_bounds__(256) void k_sync_scrub_fill(const hf3fs_crc_sync_meta* __restrict__ const local,
                                                         const uint64_t* __restrict__ const addrs,
                                                         const uint32_t* __restrict__ const d_write,
                                                         const uint32_t* __restrict__ const info,
                                                         const uint64_t n_local,
                                                         hf3fs_crc_scrub_io* __restrict__ scrub) {
  const uint32_t n_write = info[HF3FS_SYNC_INFO_N_WRITE];
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_local;
       k += (uint64_t)gridDim.x * blockDim.x) {
    hf3fs_crc_scrub_io io{};
    io.checksum_type = kTypeNone;
    if (k < n_write) {
      const uint32_t i = d_write[k];
      if (i < n_local) {
        io.data = addrs[i];
        io.length = local[i].length;
        io.checksum_type = local[i].checksum_type;
        io.checksum = local[i].checksum;
      }
    }
    scrub[k] = io;
  }
}

}  // namespace

size_t sync_scratch_bytes(uint64_t n_local, uint64_t n_remote) {
  uint64_t slots = 2;
  while (slots < 2 * n_local) slots <<= 1;
  // ctl, table, claim, rfound, two count arrays, two code arrays; 16-byte rounding of each piece
  return kSyncCtlWords * 4 + slots * 4 + n_local * 4 + n_remote * 4 + 2 * kSyncBlocksMax * 4 + n_local + n_remote +
         8 * 16;
}

void sync_scratch_carve(void* base, uint64_t n_local, uint64_t n_remote, SyncScratch* s) {
  uint64_t slots = 2;
  while (slots < 2 * n_local) slots <<= 1;
  uint8_t* p = (uint8_t*)base;
  auto take = [&](size_t bytes) {
    uint8_t* r = p;
    p += (bytes + 15) & ~size_t(15);
    return r;
  };
  s->ctl = (uint32_t*)take(kSyncCtlWords * 4);
  s->table = (uint32_t*)take(slots * 4);
  s->claim = (uint32_t*)take(n_local * 4);
  s->rfound = (uint32_t*)take(n_remote * 4);
  s->lcount = (uint32_t*)take(kSyncBlocksMax * 4);
  s->rcount = (uint32_t*)take(kSyncBlocksMax * 4);
  s->lcode = take(n_local);
  s->rcode = take(n_remote);
  s->slots = (uint32_t)slots;
}

hipError_t launch_sync_plan(hf3fs_crc_sync_meta* local, uint64_t n_local, hf3fs_crc_sync_meta* remote,
                            uint64_t n_remote, uint32_t chain_ver, uint32_t flags, uint32_t* d_write,
                            uint32_t* d_remove, uint32_t* d_info, const SyncScratch& s, hipStream_t st) {
  const uint64_t both = n_local > n_remote ? n_local : n_remote;
  const unsigned lists = shares_of(n_local).blocks + shares_of(n_remote).blocks;
  hipLaunchKernelGGL(k_sync_clear, dim3(grid_of(s.slots)), dim3(256), 0, st, s.table, s.claim, s.ctl, s.slots, n_local);
  hipLaunchKernelGGL(k_sync_insert, dim3(grid_of(n_local)), dim3(256), 0, st, local, n_local, s.table, s.slots);
  hipLaunchKernelGGL(k_sync_claim, dim3(grid_of(n_remote)), dim3(256), 0, st, local, n_local, remote, n_remote,
                     s.table, s.slots, s.claim, s.rfound);
  hipLaunchKernelGGL(k_sync_classify, dim3(grid_of(both)), dim3(256), 0, st, local, n_local, remote, n_remote,
                     chain_ver, flags, s.table, s.slots, s.claim, s.rfound, s.lcode, s.rcode, s.ctl);
  hipLaunchKernelGGL(k_sync_count, dim3(lists), dim3(256), 0, st, s.lcode, n_local, s.rcode, n_remote, s.ctl,
                     s.lcount, s.rcount);
  hipLaunchKernelGGL(k_sync_scan, dim3(1), dim3(256), 0, st, s.lcount, shares_of(n_local).blocks, s.rcount,
                     shares_of(n_remote).blocks, s.ctl, d_info);
  hipLaunchKernelGGL(k_sync_scatter, dim3(lists), dim3(256), 0, st, s.lcode, n_local, s.rcode, n_remote, s.ctl,
                     s.lcount, s.rcount, d_write, d_remove);
  return hipGetLastError();
}

hipError_t launch_sync_scrub_fill(const hf3fs_crc_sync_meta* local, const uint64_t* addrs, const uint32_t* d_write,
                                  const uint32_t* d_info, uint64_t n_local, hf3fs_crc_scrub_io* scrub, hipStream_t st) {
  hipLaunchKernelGGL(k_sync_scrub_fill, dim3(grid_of(n_local)), dim3(256), 0, st, local, addrs, d_write, d_info,
                     n_local, scrub);
  return hipGetLastError();
}

}  // namespace hf3fs_crc
