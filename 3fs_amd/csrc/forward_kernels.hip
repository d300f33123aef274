// forward_kernels.hip -- see forward_kernels.h.  The kernels read 192-byte job records and write
// their output fields, 8-byte job descriptors, 4-byte indices and eight info words; no byte of a
// chunk or payload is loaded here (the range kernels of crc_kernels.hip hash the prep's jobs) and
// none is stored anywhere.  Every decision is forward_plan.h's.
//
// Who writes what (one lane per job; a job's record is loaded and stored by its lane alone):
//   prep             addr[i], len[i] for every job, maxl[0] by atomicMax
//   prepare finish   jobs[i]: the prepare outputs, commit_ver / commit_chain_ver, and for a job
//                    that is not sent the response fields; d_info by atomicAdd (zeroed before)
//   complete settle  jobs[i]: the complete outputs; take[i]; count[b] (COMMIT jobs of workgroup
//                    b's contiguous share); d_info words 1.. by atomicAdd (zeroed before)
//   complete scan    count[] becomes its exclusive sums; d_info[HF3FS_FORWARD_DONE_COMMITS]
//   complete scatter d_commit_idx, stable: workgroup b writes its share from its offset on
// The compaction is compact.h's (count per share, one scan, scatter: the scheme of the resync
// plan's write list).  Phases are ordered by kernel boundaries only.  Nothing is read that an
// earlier launch of the same call has not written (option poison).
#include "forward_kernels.h"

#include "compact.h"
#include "forward_plan.h"
#include "loadcheck.h"

namespace hf3fs_crc {
namespace {

unsigned grid_of(uint64_t n) {
  const uint64_t want = (n + 255) / 256;
  return (unsigned)(want < 4096 ? (want ? want : 1) : 4096);
}

// Complete's finish cuts the jobs into contiguous shares (compact.h), one per workgroup.
__host__ __device__ inline Shares shares_of(uint64_t n) { return ::hf3fs_crc::shares_of(n, kForwardBlocksMax); }

// Sums each lane's eight counters over the workgroup and adds the non-zero ones into info[from..8).
__device__ __forceinline__ void add_info(uint32_t (&mine)[HF3FS_FORWARD_INFO_WORDS], uint32_t* total,
                                         uint32_t* __restrict__ info, uint32_t from) {
#pragma unroll
  for (int w = 0; w < HF3FS_FORWARD_INFO_WORDS; ++w) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine[w] += __shfl_xor(mine[w], d, 64);
    if ((threadIdx.x & 63) == 0 && mine[w]) atomicAdd(&total[w], mine[w]);
  }
  __syncthreads();
  if (threadIdx.x >= from && threadIdx.x < HF3FS_FORWARD_INFO_WORDS && total[threadIdx.x])
    atomicAdd(&info[threadIdx.x], total[threadIdx.x]);
}

template <bool COMPLETE>
__global__ __launch_bounds__(256) void k_forward_prep(const hf3fs_crc_forward_job* __restrict__ const jobs,
                                                      const uint64_t n, const uint8_t type, const uint32_t max_len,
                                                      uint64_t* __restrict__ addr, uint64_t* __restrict__ len,
                                                      uint32_t* __restrict__ maxl) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const hf3fs_crc_forward_job j = HF3FS_LC_REC(jobs, i, n);
    bool need;
    uint64_t a;
    uint32_t l;
    if (COMPLETE) {
      need = forward_rehash(j, type, max_len);
      a = j.out_data;
      l = j.out_length;
    } else {
      need = forward_route(j, type, max_len).hashes;
      a = j.chunk;
      l = j.chunk_len;
    }
    addr[i] = need ? a : 0;
    len[i] = need ? l : 0;
    if (need) atomicMax(maxl, l);
  }
}

__global__ __launch_bounds__(256) void k_forward_prepare_finish(hf3fs_crc_forward_job* __restrict__ jobs,
                                                                const uint64_t n, const uint8_t type,
                                                                const uint32_t max_len, const uint32_t max_inline_bytes,
                                                                const uint32_t* __restrict__ const v,
                                                                uint32_t* __restrict__ info) {
  __shared__ uint32_t total[HF3FS_FORWARD_INFO_WORDS];
  if (threadIdx.x < HF3FS_FORWARD_INFO_WORDS) total[threadIdx.x] = 0;
  __syncthreads();
  uint32_t mine[HF3FS_FORWARD_INFO_WORDS] = {};
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    hf3fs_crc_forward_job j = HF3FS_LC_REC(jobs, i, n);
    const ForwardRoute r = forward_route(j, type, max_len);
    const ForwardPrepCounts c = forward_prepare_settle(j, r, r.hashes ? v[i] : 0u, max_inline_bytes);
    hf3fs_crc_forward_job* o = jobs + i;
    o->out_data = j.out_data;
    o->status = j.status;
    o->res_length = j.res_length;
    o->res_update_ver = j.res_update_ver;
    o->res_commit_ver = j.res_commit_ver;
    o->out_offset = j.out_offset;
    o->out_length = j.out_length;
    o->out_checksum = j.out_checksum;
    o->out_update_ver = j.out_update_ver;
    o->out_commit_chain_ver = j.out_commit_chain_ver;
    o->computed = j.computed;
    o->action = j.action;
    o->is_syncing = j.is_syncing;
    o->out_update_type = j.out_update_type;
    o->out_checksum_type = j.out_checksum_type;
    o->out_flags = j.out_flags;
    o->commit_ver = j.commit_ver;
    o->commit_chain_ver = j.commit_chain_ver;
    if (j.action != HF3FS_FORWARD_SEND) {  // (a sent job's response is the host's to write)
      o->fwd_checksum_type = j.fwd_checksum_type;
      o->fwd_status = j.fwd_status;
      o->fwd_length = j.fwd_length;
      o->fwd_checksum = j.fwd_checksum;
      o->fwd_commit_ver = j.fwd_commit_ver;
      o->fwd_commit_chain_ver = j.fwd_commit_chain_ver;
    }
    mine[HF3FS_FORWARD_INFO_SENT] += c.sent;
    mine[HF3FS_FORWARD_INFO_RETURNED] += c.returned;
    mine[HF3FS_FORWARD_INFO_NO_SUCCESSOR] += c.no_successor;
    mine[HF3FS_FORWARD_INFO_SYNC_HASHED] += c.hashed;
    mine[HF3FS_FORWARD_INFO_SYNC_MISMATCHED] += c.mismatched;
    mine[HF3FS_FORWARD_INFO_BAD_RECORDS] += c.bad;
  }
  add_info(mine, total, info, 0);
}

__global__ __launch_bounds__(256) void k_forward_complete_settle(hf3fs_crc_forward_job* __restrict__ jobs,
                                                                 const uint64_t n, const uint8_t type,
                                                                 const uint32_t max_len,
                                                                 const uint32_t* __restrict__ const v,
                                                                 uint8_t* __restrict__ take,
                                                                 uint32_t* __restrict__ count,
                                                                 uint32_t* __restrict__ info) {
  __shared__ uint32_t total[HF3FS_FORWARD_INFO_WORDS];
  if (threadIdx.x < HF3FS_FORWARD_INFO_WORDS) total[threadIdx.x] = 0;
  __syncthreads();
  const Shares sh = shares_of(n);
  const uint64_t lo = (uint64_t)blockIdx.x * sh.per, hi = lo + sh.per < n ? lo + sh.per : n;
  uint32_t mine[HF3FS_FORWARD_INFO_WORDS] = {};
  for (uint64_t i = lo + threadIdx.x; i < hi; i += 256) {
    hf3fs_crc_forward_job j = HF3FS_LC_REC(jobs, i, n);
    const uint32_t hashed = forward_rehash(j, type, max_len) ? v[i] : 0u;
    const ForwardDoneCounts c = forward_complete_settle(j, type, max_len, hashed);
    hf3fs_crc_forward_job* o = jobs + i;
    o->final_status = j.final_status;
    o->commit_ver = j.commit_ver;
    o->commit_chain_ver = j.commit_chain_ver;
    o->fwd_update_ver = j.fwd_update_ver;
    o->buffer_computed = j.buffer_computed;
    o->final_action = j.final_action;
    o->buffer_corrupted = j.buffer_corrupted;
    take[i] = c.commit;
    mine[HF3FS_FORWARD_DONE_COMMITS] += c.commit;
    mine[HF3FS_FORWARD_DONE_RETURNED] += c.returned;
    mine[HF3FS_FORWARD_DONE_7015] += c.e7015;
    mine[HF3FS_FORWARD_DONE_4081] += c.e4081;
    mine[HF3FS_FORWARD_DONE_4082] += c.e4082;
    mine[HF3FS_FORWARD_DONE_REHASHED] += c.rehashed;
    mine[HF3FS_FORWARD_DONE_CORRUPTED] += c.corrupted;
    mine[HF3FS_FORWARD_DONE_UNHASHABLE] += c.unhashable;
  }
  add_info(mine, total, info, 1);  // (word 0, the commits, is the scan's: their sum over the shares)
  if (threadIdx.x == 0) count[blockIdx.x] = total[HF3FS_FORWARD_DONE_COMMITS];
}

// One workgroup: the exclusive sums of the count array, and the commit count.
__global__ __launch_bounds__(256) void k_forward_scan(uint32_t* __restrict__ count, const uint32_t nb,
                                                      uint32_t* __restrict__ info) {
  static_assert(kForwardBlocksMax == 256 * 8, "compact_scan_counts: eight entries per thread");
  __shared__ uint32_t sums[256];
  const uint32_t upto = compact_scan_counts(count, nb, sums);
  if (threadIdx.x == 255) info[HF3FS_FORWARD_DONE_COMMITS] = upto;
}

// Workgroup b writes the COMMIT jobs of its share from its offset on, in index order.
__global__ __launch_bounds__(256) void k_forward_scatter(const uint8_t* __restrict__ const take, const uint64_t n,
                                                         const uint32_t* __restrict__ const count,
                                                         uint32_t* __restrict__ commit_idx) {
  __shared__ uint32_t wave_n[4];
  const Shares sh = shares_of(n);
  const uint64_t lo = (uint64_t)blockIdx.x * sh.per, hi = lo + sh.per < n ? lo + sh.per : n;
  compact_scatter_share([&](uint64_t i) { return take[i] != 0; }, lo, hi, count[blockIdx.x], commit_idx, n, wave_n);
}

}  // namespace

size_t forward_scratch_bytes(uint64_t n) { return ((n + 15) & ~uint64_t(15)) + kForwardBlocksMax * 4; }

void forward_scratch_carve(void* base, uint64_t n, ForwardScratch* s) {
  s->count = (uint32_t*)base;
  s->take = (uint8_t*)base + kForwardBlocksMax * 4;
  (void)n;
}

hipError_t launch_forward_prep(const hf3fs_crc_forward_job* jobs, uint64_t n, uint8_t type, uint32_t max_len,
                               bool complete, uint64_t* addr, uint64_t* len, uint32_t* maxl, hipStream_t st) {
  if (complete)
    hipLaunchKernelGGL(k_forward_prep<true>, dim3(grid_of(n)), dim3(256), 0, st, jobs, n, type, max_len, addr, len,
                       maxl);
  else
    hipLaunchKernelGGL(k_forward_prep<false>, dim3(grid_of(n)), dim3(256), 0, st, jobs, n, type, max_len, addr, len,
                       maxl);
  return hipGetLastError();
}

hipError_t launch_forward_prepare_finish(hf3fs_crc_forward_job* jobs, uint64_t n, uint8_t type, uint32_t max_len,
                                         uint32_t max_inline_bytes, const uint32_t* v, uint32_t* info, hipStream_t st) {
  hipLaunchKernelGGL(k_forward_prepare_finish, dim3(grid_of(n)), dim3(256), 0, st, jobs, n, type, max_len,
                     max_inline_bytes, v, info);
  return hipGetLastError();
}

hipError_t launch_forward_complete_finish(hf3fs_crc_forward_job* jobs, uint64_t n, uint8_t type, uint32_t max_len,
                                          const uint32_t* v, uint32_t* commit_idx, uint32_t* info,
                                          const ForwardScratch& s, hipStream_t st) {
  const uint32_t blocks = shares_of(n).blocks;
  hipLaunchKernelGGL(k_forward_complete_settle, dim3(blocks), dim3(256), 0, st, jobs, n, type, max_len, v, s.take,
                     s.count, info);
  hipLaunchKernelGGL(k_forward_scan, dim3(1), dim3(256), 0, st, s.count, blocks, info);
  if (commit_idx)
    hipLaunchKernelGGL(k_forward_scatter, dim3(blocks), dim3(256), 0, st, s.take, n, s.count, commit_idx);
  return hipGetLastError();
}

}  // namespace hf3fs_crc
