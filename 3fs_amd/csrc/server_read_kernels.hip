// server_read_kernels.hip -- see server_read_kernels.h.  The kernels read 192-byte job records and
// 128-byte request records and write their output fields, 8-byte job descriptors, the scratch of
// ServerReadScratch, 32-byte list entries and eight info words.  No byte of a read buffer is
// loaded to be hashed here (the range kernels of crc_kernels.hip hash the prep's jobs); the pack
// kernel alone loads them, to store them into the inline arena, through copy_range.h's body.
// Every decision is server_read_plan.h's.
//
// Who writes what:
//   prepare   one lane per request: its record's prepare outputs, the prepare outputs of its jobs
//             (and an engine job's commit_ver); d_info by atomicAdd (zeroed before)
//   prep      one lane per job: addr[i], len[i], req[i]; maxl[0] by atomicMax
//   settle    one lane per job of workgroup b's contiguous share: jobs[i]'s complete outputs but
//             inline_off, done[i], count[b], bytes[b]; d_info's counters by atomicAdd (zeroed before)
//   scan      one workgroup: count[] and bytes[] become their exclusive sums; pre[n], wr_pre[n];
//             d_info's inline bytes, overflow word and list length
//   place     workgroup b walks its share from its offsets on: pre[i], wr_pre[i], jobs[i].inline_off,
//             d_wr below wr_cap (compact.h's stable placement)
//   requests  one lane per request: its record's complete outputs
//   pack      one workgroup per packing job at a time: d_inline[inline_off, +result_len)
// Phases are ordered by kernel boundaries only.  Nothing is read that an earlier launch of the same
// call has not written (option poison).
#include "server_read_kernels.h"

#include "compact.h"
#include "copy_range.h"
#include "loadcheck.h"
#include "server_read_plan.h"

namespace hf3fs_crc {
namespace {

unsigned grid_of(uint64_t n) {
  const uint64_t want = (n + 255) / 256;
  return (unsigned)(want < 4096 ? (want ? want : 1) : 4096);
}

__host__ __device__ inline Shares shares_of(uint64_t n) { return ::hf3fs_crc::shares_of(n, kServerReadBlocksMax); }

// Sums each lane's eight counters over the workgroup and adds the non-zero ones into info, but
// for word `skip` (another launch's to set; its workgroup sum stays in total[skip]).
__device__ __forceinline__ void add_info(uint32_t (&mine)[HF3FS_SERVER_READ_INFO_WORDS], uint32_t* total,
                                         uint32_t* __restrict__ info,
                                         uint32_t skip = HF3FS_SERVER_READ_INFO_WORDS) {
#pragma unroll
  for (int w = 0; w < HF3FS_SERVER_READ_INFO_WORDS; ++w) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine[w] += __shfl_xor(mine[w], d, 64);
    if ((threadIdx.x & 63) == 0 && mine[w]) atomicAdd(&total[w], mine[w]);
  }
  __syncthreads();
  if (threadIdx.x < HF3FS_SERVER_READ_INFO_WORDS && threadIdx.x != skip && total[threadIdx.x])
    atomicAdd(&info[threadIdx.x], total[threadIdx.x]);
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
  return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int d) {
  const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
  return (uint64_t)hi << 32 | lo;
}

__device__ __forceinline__ void store_prepare(hf3fs_crc_server_read_job* o, const hf3fs_crc_server_read_job& j) {
  o->read_offset = j.read_offset;
  if (j.engine) o->commit_ver = j.commit_ver;
  o->head_len = j.head_len;
  o->tail_len = j.tail_len;
  o->read_len = j.read_len;
  o->buf_ordinal = j.buf_ordinal;
  o->buf_off = j.buf_off;
  o->status = j.status;
  o->buf_kind = j.buf_kind;
}

__global__ __launch_bounds__(256) void k_server_read_prepare(hf3fs_crc_server_read_job* __restrict__ jobs,
                                                             const uint64_t n,
                                                             hf3fs_crc_server_read_req* __restrict__ reqs,
                                                             const uint64_t* __restrict__ const req_off,
                                                             const uint64_t n_reqs, const uint32_t small_buf,
                                                             const uint32_t big_buf, uint32_t* __restrict__ info) {
  __shared__ uint32_t total[HF3FS_SERVER_READ_INFO_WORDS];
  if (threadIdx.x < HF3FS_SERVER_READ_INFO_WORDS) total[threadIdx.x] = 0;
  __syncthreads();
  uint32_t mine[HF3FS_SERVER_READ_INFO_WORDS] = {};
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reqs; r += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t lo, hi;
    server_read_jobs_of(req_off, r, n, &lo, &hi);
    hf3fs_crc_server_read_req q = HF3FS_LC_REC(reqs, r, n_reqs);
    const ServerReadPrepCounts c = server_read_prepare_request(
        q, lo, hi, small_buf, big_buf, [&](uint64_t i) { return HF3FS_LC_REC(jobs, i, n); },
        [&](uint64_t i, const hf3fs_crc_server_read_job& j) { store_prepare(jobs + i, j); });
    hf3fs_crc_server_read_req* o = reqs + r;
    o->total_len = q.total_len;
    o->total_head = q.total_head;
    o->total_tail = q.total_tail;
    o->status = q.status;
    o->failed_job = q.failed_job;
    o->n_small = q.n_small;
    o->n_big = q.n_big;
    mine[HF3FS_SERVER_READ_INFO_REQS_OK] += c.reqs_ok;
    mine[HF3FS_SERVER_READ_INFO_REQS_FAILED] += c.reqs_failed;
    mine[HF3FS_SERVER_READ_INFO_JOBS_OK] += c.jobs_ok;
    mine[HF3FS_SERVER_READ_INFO_JOBS_FAILED] += c.jobs_failed;
    mine[HF3FS_SERVER_READ_INFO_SMALL] += c.n_small;
    mine[HF3FS_SERVER_READ_INFO_BIG] += c.n_big;
  }
  add_info(mine, total, info);
}

__global__ __launch_bounds__(256) void k_server_read_prep(const hf3fs_crc_server_read_job* __restrict__ const jobs,
                                                          const uint64_t n,
                                                          const hf3fs_crc_server_read_req* __restrict__ const reqs,
                                                          const uint64_t* __restrict__ const req_off,
                                                          const uint64_t n_reqs, const uint8_t type,
                                                          const uint32_t max_len, uint64_t* __restrict__ addr,
                                                          uint64_t* __restrict__ len, uint32_t* __restrict__ maxl,
                                                          uint32_t* __restrict__ req) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const hf3fs_crc_server_read_job j = HF3FS_LC_REC(jobs, i, n);
    const uint64_t r = server_read_req_of(req_off, n_reqs, i);
    const ServerReadRoute o = server_read_route(j, HF3FS_LC_REC(reqs, r, n_reqs), type, max_len);
    req[i] = (uint32_t)r;
    addr[i] = o.hashes ? j.localbuf + j.head_len : 0;
    len[i] = o.hashes ? o.len : 0;
    if (o.hashes) atomicMax(maxl, o.len);
  }
}

__global__ __launch_bounds__(256) void k_server_read_settle(hf3fs_crc_server_read_job* __restrict__ jobs,
                                                            const uint64_t n,
                                                            const hf3fs_crc_server_read_req* __restrict__ const reqs,
                                                            const uint8_t type, const uint32_t max_len,
                                                            const uint32_t* __restrict__ const v,
                                                            const uint32_t* __restrict__ const req,
                                                            uint8_t* __restrict__ done, uint32_t* __restrict__ count,
                                                            uint64_t* __restrict__ bytes, uint32_t* __restrict__ info) {
  __shared__ uint32_t total[HF3FS_SERVER_READ_INFO_WORDS];
  __shared__ unsigned long long packed;
  if (threadIdx.x < HF3FS_SERVER_READ_INFO_WORDS) total[threadIdx.x] = 0;
  if (threadIdx.x == 0) packed = 0;
  __syncthreads();
  const Shares sh = shares_of(n);
  const uint64_t lo = (uint64_t)blockIdx.x * sh.per, hi = lo + sh.per < n ? lo + sh.per : n;
  uint32_t mine[HF3FS_SERVER_READ_INFO_WORDS] = {};
  uint64_t pack = 0;
  for (uint64_t i = lo + threadIdx.x; i < hi; i += 256) {
    hf3fs_crc_server_read_job j = HF3FS_LC_REC(jobs, i, n);
    const hf3fs_crc_server_read_req q = reqs[req[i]];  // (req[i] < n_reqs: the prep's)
    const ServerReadRoute o = server_read_route(j, q, type, max_len);
    const ServerReadDone d = server_read_settle(j, q, o, o.hashes ? v[i] : 0u);
    hf3fs_crc_server_read_job* out = jobs + i;
    out->result_len = j.result_len;
    out->result_status = j.result_status;
    out->checksum = j.checksum;
    out->checksum_type = j.checksum_type;
    done[i] = server_read_done_bits(d);
    pack += d.packs ? j.result_len : 0u;
    mine[HF3FS_SERVER_READ_DONE_OK] += d.ok;
    mine[HF3FS_SERVER_READ_DONE_FAILED] += d.ok ? 0u : 1u;
    mine[HF3FS_SERVER_READ_DONE_WR] += d.listed;
    mine[HF3FS_SERVER_READ_DONE_WR_FAILS] += d.wr_failed;
    mine[HF3FS_SERVER_READ_DONE_HASHED] += d.hashed;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) pack += shfl_xor64(pack, d);
  if ((threadIdx.x & 63) == 0 && pack) atomicAdd(&packed, (unsigned long long)pack);
  add_info(mine, total, info, HF3FS_SERVER_READ_DONE_WR);  // (the list length is the scan's: the sum over the shares)
  if (threadIdx.x == 0) {
    count[blockIdx.x] = total[HF3FS_SERVER_READ_DONE_WR];
    bytes[blockIdx.x] = packed;
  }
}

// One workgroup: the exclusive sums of both share arrays, the totals.
__global__ __launch_bounds__(256) void k_server_read_scan(uint32_t* __restrict__ count, uint64_t* __restrict__ bytes,
                                                          const uint32_t nb, const uint64_t n,
                                                          const uint64_t inline_cap, uint64_t* __restrict__ pre,
                                                          uint32_t* __restrict__ wr_pre, uint32_t* __restrict__ info) {
  static_assert(kServerReadBlocksMax == 256 * 8, "compact_scan_counts: eight entries per thread");
  __shared__ uint32_t sums[256];
  __shared__ uint64_t sums64[256];
  const uint32_t upto = compact_scan_counts(count, nb, sums);
  uint64_t b[8], total = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t at = threadIdx.x * 8 + k;
    b[k] = at < nb ? bytes[at] : 0u;
    total += b[k];
  }
  sums64[threadIdx.x] = total;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint64_t add = threadIdx.x >= d ? sums64[threadIdx.x - d] : 0u;
    __syncthreads();
    sums64[threadIdx.x] += add;
    __syncthreads();
  }
  const uint64_t upto64 = sums64[threadIdx.x];
  uint64_t run = upto64 - total;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t at = threadIdx.x * 8 + k;
    if (at < nb) bytes[at] = run;
    run += b[k];
  }
  if (threadIdx.x == 255) {
    info[HF3FS_SERVER_READ_DONE_WR] = upto;
    info[HF3FS_SERVER_READ_DONE_INLINE_LO] = (uint32_t)upto64;
    info[HF3FS_SERVER_READ_DONE_INLINE_HI] = (uint32_t)(upto64 >> 32);
    info[HF3FS_SERVER_READ_DONE_INLINE_OVERFLOW] = upto64 > inline_cap ? 1u : 0u;
    pre[n] = upto64;
    wr_pre[n] = upto;
  }
}

// Workgroup b walks its share in tiles of 256, in index order, from its offsets on.
__global__ __launch_bounds__(256) void k_server_read_place(hf3fs_crc_server_read_job* __restrict__ jobs,
                                                           const uint64_t n, const uint8_t* __restrict__ const done,
                                                           const uint32_t* __restrict__ const req,
                                                           const uint32_t* __restrict__ const count,
                                                           const uint64_t* __restrict__ const bytes,
                                                           uint64_t* __restrict__ pre, uint32_t* __restrict__ wr_pre,
                                                           hf3fs_crc_server_read_wr* __restrict__ wr,
                                                           const uint64_t wr_cap) {
  __shared__ uint32_t wave_n[4];
  __shared__ uint64_t wave_b[4];
  const Shares sh = shares_of(n);
  const uint64_t lo = (uint64_t)blockIdx.x * sh.per, hi = lo + sh.per < n ? lo + sh.per : n;
  // the list: compact.h's stable placement, every job's position kept for the requests
  compact_place_share([&](uint64_t i) { return (done[i] & kSrdListed) != 0; }, lo, hi, count[blockIdx.x],
                      [&](uint64_t i, uint64_t at, bool mine) {
                        wr_pre[i] = (uint32_t)at;
                        if (mine && at < wr_cap)
                          wr[at] = server_read_wr_of(HF3FS_LC_REC(jobs, i, n), (uint32_t)i, req[i]);
                      },
                      wave_n);
  // the inline offsets: an exclusive scan of the packing jobs' lengths, 64 bits
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t base = bytes[blockIdx.x];
  for (uint64_t i0 = lo; i0 < hi; i0 += 256) {  // workgroup-uniform
    const uint64_t i = i0 + threadIdx.x;
    const bool packs = i < hi && (done[i] & kSrdPacks) != 0;
    const uint64_t len = packs ? jobs[i].result_len : 0u;
    uint64_t incl = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t up = shfl_up64(incl, d);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) wave_b[wave] = incl;
    __syncthreads();
    uint64_t before = 0, tile = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint64_t c = wave_b[w];
      before += w < wave ? c : 0u;
      tile += c;
    }
    const uint64_t at = base + before + incl - len;
    if (i < hi) {
      pre[i] = at;
      jobs[i].inline_off = packs ? at : 0u;
    }
    base += tile;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_server_read_requests(const hf3fs_crc_server_read_job* __restrict__ const jobs,
                                                              const uint64_t n,
                                                              hf3fs_crc_server_read_req* __restrict__ reqs,
                                                              const uint64_t* __restrict__ const req_off,
                                                              const uint64_t n_reqs,
                                                              const uint8_t* __restrict__ const done,
                                                              const uint64_t* __restrict__ const pre,
                                                              const uint32_t* __restrict__ const wr_pre) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reqs; r += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t lo, hi;
    server_read_jobs_of(req_off, r, n, &lo, &hi);
    uint32_t n_ok = 0, wr_fails = 0;
    uint64_t wr_bytes = 0;
    for (uint64_t i = lo; i < hi; ++i) {
      const uint8_t d = done[i];
      n_ok += d & kSrdOk ? 1u : 0u;
      wr_fails += d & kSrdWrFailed ? 1u : 0u;
      wr_bytes += d & kSrdListed ? jobs[i].result_len : 0u;
    }
    hf3fs_crc_server_read_req* o = reqs + r;
    o->n_ok = n_ok;
    o->wr_fails = wr_fails;
    o->wr_bytes = wr_bytes;
    o->inline_off = n ? pre[lo] : 0u;
    o->inline_bytes = n ? pre[hi] - pre[lo] : 0u;
    o->wr_first = n ? wr_pre[lo] : 0u;
    o->wr_count = n ? wr_pre[hi] - wr_pre[lo] : 0u;
  }
}

// The inline pack (BatchReadJob.cc:96-113): workgroup w takes jobs w, w + gridDim.x, ...; the
// bytes [localbuf + head_len, +result_len) of a packing job go to d_inline + inline_off.  Bounds
// are the scan's: the offsets are exclusive sums of the lengths and their total is at most
// inline_cap, or the overflow word is set and nothing is stored.
__global__ __launch_bounds__(256) void k_server_read_pack(const hf3fs_crc_server_read_job* __restrict__ const jobs,
                                                          const uint64_t n, const uint8_t* __restrict__ const done,
                                                          const uint64_t d_inline, const uint64_t inline_cap,
                                                          const uint32_t* __restrict__ const info) {
  if (info[HF3FS_SERVER_READ_DONE_INLINE_OVERFLOW]) return;  // workgroup-uniform
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {     // workgroup-uniform
    if (!(done[i] & kSrdPacks)) continue;
    const uint64_t src = jobs[i].localbuf + jobs[i].head_len, len = jobs[i].result_len, off = jobs[i].inline_off;
    if (len == 0 || off > inline_cap || len > inline_cap - off) continue;
    copy_range_hw<4, false, false>(d_inline + off, src, len, threadIdx.x, blockDim.x);
  }
}

}  // namespace

size_t server_read_scratch_bytes(uint64_t n) {
  // bytes[B] 8, pre[n + 1] 8, count[B] 4, wr_pre[n + 1] 4, req[n] 4, done[n] 1, up to a multiple of 16
  return (kServerReadBlocksMax * 12 + (n + 1) * 12 + n * 5 + 15) & ~size_t(15);
}

void server_read_scratch_carve(void* base, uint64_t n, ServerReadScratch* s) {
  s->bytes = (uint64_t*)base;
  s->pre = s->bytes + kServerReadBlocksMax;
  s->count = (uint32_t*)(s->pre + n + 1);
  s->wr_pre = s->count + kServerReadBlocksMax;
  s->req = s->wr_pre + n + 1;
  s->done = (uint8_t*)(s->req + n);
}

hipError_t launch_server_read_prepare(hf3fs_crc_server_read_job* jobs, uint64_t n, hf3fs_crc_server_read_req* reqs,
                                      const uint64_t* req_off, uint64_t n_reqs, uint32_t small_buf, uint32_t big_buf,
                                      uint32_t* info, hipStream_t st) {
  // one lane per request, 64-thread workgroups: few requests of many jobs spread over the CUs
  const uint64_t want = (n_reqs + 63) / 64;
  hipLaunchKernelGGL(k_server_read_prepare, dim3((unsigned)(want < 16384 ? (want ? want : 1) : 16384)), dim3(64), 0,
                     st, jobs, n, reqs, req_off, n_reqs, small_buf, big_buf, info);
  return hipGetLastError();
}

hipError_t launch_server_read_prep(const hf3fs_crc_server_read_job* jobs, uint64_t n,
                                   const hf3fs_crc_server_read_req* reqs, const uint64_t* req_off, uint64_t n_reqs,
                                   uint8_t type, uint32_t max_len, uint64_t* addr, uint64_t* len, uint32_t* maxl,
                                   const ServerReadScratch& s, hipStream_t st) {
  hipLaunchKernelGGL(k_server_read_prep, dim3(grid_of(n)), dim3(256), 0, st, jobs, n, reqs, req_off, n_reqs, type,
                     max_len, addr, len, maxl, s.req);
  return hipGetLastError();
}

hipError_t launch_server_read_finish(hf3fs_crc_server_read_job* jobs, uint64_t n,
                                     const hf3fs_crc_server_read_req* reqs, uint8_t type, uint32_t max_len,
                                     const uint32_t* v, uint64_t inline_cap, hf3fs_crc_server_read_wr* wr,
                                     uint64_t wr_cap, uint32_t* info, const ServerReadScratch& s, hipStream_t st) {
  const uint32_t blocks = shares_of(n).blocks;
  hipLaunchKernelGGL(k_server_read_settle, dim3(blocks), dim3(256), 0, st, jobs, n, reqs, type, max_len, v, s.req,
                     s.done, s.count, s.bytes, info);
  hipLaunchKernelGGL(k_server_read_scan, dim3(1), dim3(256), 0, st, s.count, s.bytes, blocks, n, inline_cap, s.pre,
                     s.wr_pre, info);
  hipLaunchKernelGGL(k_server_read_place, dim3(blocks), dim3(256), 0, st, jobs, n, s.done, s.req, s.count, s.bytes,
                     s.pre, s.wr_pre, wr, wr ? wr_cap : 0);
  return hipGetLastError();
}

hipError_t launch_server_read_requests(const hf3fs_crc_server_read_job* jobs, uint64_t n,
                                       hf3fs_crc_server_read_req* reqs, const uint64_t* req_off, uint64_t n_reqs,
                                       const ServerReadScratch& s, hipStream_t st) {
  const uint64_t want = (n_reqs + 63) / 64;
  hipLaunchKernelGGL(k_server_read_requests, dim3((unsigned)(want < 16384 ? (want ? want : 1) : 16384)), dim3(64), 0,
                     st, jobs, n, reqs, req_off, n_reqs, s.done, s.pre, s.wr_pre);
  return hipGetLastError();
}

hipError_t launch_server_read_pack(const hf3fs_crc_server_read_job* jobs, uint64_t n, void* d_inline,
                                   uint64_t inline_cap, const uint32_t* info, const ServerReadScratch& s,
                                   hipStream_t st) {
  const uint64_t want = n < 8192 ? n : 8192;
  hipLaunchKernelGGL(k_server_read_pack, dim3((unsigned)(want ? want : 1)), dim3(256), 0, st, jobs, n, s.done,
                     (uint64_t)d_inline, inline_cap, info);
  return hipGetLastError();
}

}  // namespace hf3fs_crc
