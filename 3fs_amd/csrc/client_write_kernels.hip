// client_write_kernels.hip -- see client_write_kernels.h.  The kernels read and write 64-byte IO
// records, 56-byte update records, 24-byte file records, 8-byte offsets, 4-byte indices and eight
// info words; no byte of a caller's data buffer is loaded here (the range kernels of
// crc_kernels.hip hash the prep's jobs) and none is stored anywhere.  Every decision is
// client_write_plan.h's.
//
// Who writes what:
//   prep            addr[i], len[i] for every IO, ctl[0] by atomicMax, ctl[1] (the poison word) by
//                   atomicOr
//   prepare finish  ios[i]: checksum, checksum_type, send_inline, status; updates[i]: the request
//                   fields; d_info by atomicAdd (zeroed before)
//   settle          ios[i]: the four answer fields (FROM_UPDATES, sent IOs only); take[i];
//                   count[b] (failed IOs of workgroup b's contiguous share); d_info words 1..3
//   scan            count[] becomes its exclusive sums; d_info[HF3FS_CLIENT_WRITE_DONE_FAILED]
//   scatter         d_failed, stable: workgroup b writes its share from its offset on
//   fold            d_files[f]; d_info words 4 and 5
// A record is loaded and stored by its own lane alone in prepare finish and settle, and loaded
// through inputs_of / answer_of, which leave out the words the same launch stores.  The compaction
// is compact.h's.  Phases are ordered by kernel boundaries only.  Nothing is read that an earlier
// launch of the same call has not written (option poison).
#include "client_write_kernels.h"

#include "client_write_plan.h"
#include "compact.h"
#include "gf2.h"
#include "loadcheck.h"

namespace hf3fs_crc {
namespace {

unsigned grid_of(uint64_t n, unsigned per = 256) {
  const uint64_t want = (n + per - 1) / per;
  return (unsigned)(want < 4096 ? (want ? want : 1) : 4096);
}

__host__ __device__ inline Shares shares_of(uint64_t n) { return ::hf3fs_crc::shares_of(n, kClientWriteBlocksMax); }

struct GfTables {
  const DeviceTables* tabs;
  __device__ __forceinline__ uint32_t shift(uint32_t v, uint64_t nbytes, uint8_t type) const {
    const uint32_t poly = poly_of(type);
    return gf_mul(v, xpow8_bytes((int64_t)nbytes, &tabs->poly[type == kTypeCrc32 ? 1 : 0], poly), poly);
  }
};

// The request fields of record i behind HF3FS_LC_REC's index check (an index >= n is logged and
// gives a zeroed record): what prepare decides from, none of the words it stores.
__device__ __forceinline__ hf3fs_crc_client_write_io inputs_of(const hf3fs_crc_client_write_io* ios, uint64_t i,
                                                               uint64_t n) {
  hf3fs_crc_client_write_io io{};
  if (!lc_desc_ok(i, n)) return io;
  const hf3fs_crc_client_write_io* p = ios + i;
  io.data = p->data;
  io.buf_base = p->buf_base;
  io.buf_size = p->buf_size;
  io.offset = p->offset;
  io.length = p->length;
  io.chunk_size = p->chunk_size;
  return io;
}

// What complete decides from: prepare's status, the length and the answer.
__device__ __forceinline__ hf3fs_crc_client_write_io answer_of(const hf3fs_crc_client_write_io* ios, uint64_t i,
                                                               uint64_t n) {
  hf3fs_crc_client_write_io io{};
  if (!lc_desc_ok(i, n)) return io;
  const hf3fs_crc_client_write_io* p = ios + i;
  io.length = p->length;
  io.status = p->status;
  io.status_in = p->status_in;
  io.result_len = p->result_len;
  io.result_checksum = p->result_checksum;
  io.result_checksum_type = p->result_checksum_type;
  return io;
}

// The outcome fields of update record i.
__device__ __forceinline__ hf3fs_crc_update_io outcome_of(const hf3fs_crc_update_io* updates, uint64_t i, uint64_t n) {
  hf3fs_crc_update_io u{};
  if (!lc_desc_ok(i, n)) return u;
  const hf3fs_crc_update_io* p = updates + i;
  u.length = p->length;
  u.out_checksum = p->out_checksum;
  u.out_checksum_type = p->out_checksum_type;
  u.status = p->status;
  return u;
}

// File f's IOs [lo, hi) of the batch: the caller's offsets, clamped.
__device__ __forceinline__ void ios_of(const uint64_t* file_off, uint64_t f, uint64_t n_files, uint64_t n, uint64_t* lo,
                                       uint64_t* hi) {
  uint64_t b1 = HF3FS_LC_REC(file_off, f + 1, n_files + 1);
  uint64_t b0 = HF3FS_LC_REC(file_off, f, n_files + 1);
  if (b1 > n) b1 = n;
  if (b0 > b1) b0 = b1;
  *lo = b0;
  *hi = b1;
}

// Sums each lane's counters over the workgroup into total[] (shared, zeroed, W words).
template <int W>
__device__ __forceinline__ void sum_counts(uint32_t (&mine)[W], uint32_t* total) {
#pragma unroll
  for (int w = 0; w < W; ++w) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine[w] += __shfl_xor(mine[w], d, 64);
    if ((threadIdx.x & 63) == 0 && mine[w]) atomicAdd(&total[w], mine[w]);
  }
}

// The workgroup's 64-bit sum (one thread calls) into the info words lo_w, lo_w + 1: the low word's
// carry is the wrap its own atomicAdd saw.
__device__ __forceinline__ void add_info64(uint32_t* __restrict__ info, uint32_t lo_w, uint64_t sum) {
  if (!sum) return;
  const uint32_t lo = (uint32_t)sum, hi = (uint32_t)(sum >> 32);
  const uint32_t old = lo ? atomicAdd(&info[lo_w], lo) : 0u;
  const uint32_t up = hi + ((uint32_t)(old + lo) < old ? 1u : 0u);
  if (up) atomicAdd(&info[lo_w + 1], up);
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, d, 64);
  return x;
}

__global__ __launch_bounds__(256) void k_client_write_prep(const hf3fs_crc_client_write_io* __restrict__ const ios,
                                                           const uint64_t n, const uint32_t max_len, const bool verify,
                                                           uint64_t* __restrict__ addr, uint64_t* __restrict__ len,
                                                           uint32_t* __restrict__ ctl) {
  uint32_t longest = 0, offender = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const hf3fs_crc_client_write_io io = inputs_of(ios, i, n);
    const CwClass k = client_write_class(io, max_len);
    const bool need = client_write_hashes(k, verify, io.length);
    if (addr) {
      addr[i] = need ? io.data : 0;
      len[i] = need ? io.length : 0;
    }
    if (need && io.length > longest) longest = io.length;
    offender |= k == kCwOffender ? 1u : 0u;
  }
  // one atomic per wave and word, not one per IO (the kernel's time did not move with it: 0.19 ms
  // per 1 Mi records either way, profiles/client_write.jsonl)
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t o = __shfl_xor(longest, d, 64);
    longest = o > longest ? o : longest;
    offender |= __shfl_xor(offender, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (longest) atomicMax(&ctl[0], longest);
    if (offender) atomicOr(&ctl[1], 1u);
  }
}

__global__ __launch_bounds__(256) void k_client_write_prepare_finish(
    hf3fs_crc_client_write_io* __restrict__ ios, const uint64_t n, const uint8_t type, const uint32_t max_len,
    const uint32_t max_inline_bytes, const bool verify, const uint32_t* __restrict__ const v,
    const uint32_t* __restrict__ const poison, hf3fs_crc_update_io* __restrict__ updates, uint32_t* __restrict__ info) {
  __shared__ uint32_t total[HF3FS_CLIENT_WRITE_INFO_WORDS];
  __shared__ unsigned long long bytes;
  if (threadIdx.x < HF3FS_CLIENT_WRITE_INFO_WORDS) total[threadIdx.x] = 0;
  if (threadIdx.x == 0) bytes = 0;
  __syncthreads();
  const bool poisoned = *poison != 0;
  uint32_t mine[HF3FS_CLIENT_WRITE_INFO_WORDS] = {};
  uint64_t hashed_bytes = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const hf3fs_crc_client_write_io io = inputs_of(ios, i, n);
    const CwClass k = client_write_class(io, max_len);
    const bool hashes = client_write_hashes(k, verify, io.length);
    const CwPrepared p = client_write_settle(k, poisoned, io.length, hashes ? v[i] : ~0u, type, verify, max_inline_bytes);
    hf3fs_crc_client_write_io* o = ios + i;
    o->checksum = p.checksum;
    o->checksum_type = p.checksum_type;
    o->send_inline = p.send_inline;
    o->status = p.status;
    if (updates) {
      hf3fs_crc_update_io* u = updates + i;
      if (p.sent) {
        u->payload = io.data;
        u->offset = io.offset;
        u->length = io.length;
        u->update_type = HF3FS_UPDATE_WRITE;
        u->write_checksum_type = p.checksum_type;
        u->flags = 0;
        u->write_checksum = p.checksum;
      } else {
        u->update_type = 0;
      }
    }
    mine[HF3FS_CLIENT_WRITE_INFO_SENT] += p.sent ? 1u : 0u;
    mine[HF3FS_CLIENT_WRITE_INFO_RANGE] += k == kCwRange ? 1u : 0u;
    mine[HF3FS_CLIENT_WRITE_INFO_BAD_RECORDS] += k == kCwBadRecord ? 1u : 0u;
    mine[HF3FS_CLIENT_WRITE_INFO_INLINE] += p.send_inline;
    hashed_bytes += hashes ? io.length : 0u;
  }
  sum_counts(mine, total);
  hashed_bytes = wave_sum64(hashed_bytes);
  if ((threadIdx.x & 63) == 0 && hashed_bytes) atomicAdd(&bytes, (unsigned long long)hashed_bytes);
  __syncthreads();
  if (threadIdx.x < HF3FS_CLIENT_WRITE_INFO_WORDS && total[threadIdx.x])
    atomicAdd(&info[threadIdx.x], total[threadIdx.x]);
  if (threadIdx.x == 0) add_info64(info, HF3FS_CLIENT_WRITE_INFO_HASHED_LO, bytes);
  if (threadIdx.x == 0 && blockIdx.x == 0 && poisoned) info[HF3FS_CLIENT_WRITE_INFO_POISONED] = 1;
}

__global__ __launch_bounds__(256) void k_client_write_settle(hf3fs_crc_client_write_io* __restrict__ ios,
                                                             const uint64_t n,
                                                             const hf3fs_crc_update_io* __restrict__ const updates,
                                                             uint8_t* __restrict__ take, uint32_t* __restrict__ count,
                                                             uint32_t* __restrict__ info) {
  __shared__ uint32_t total[2];
  __shared__ unsigned long long bytes;
  if (threadIdx.x < 2) total[threadIdx.x] = 0;
  if (threadIdx.x == 0) bytes = 0;
  __syncthreads();
  const Shares sh = shares_of(n);
  const uint64_t lo = (uint64_t)blockIdx.x * sh.per, hi = lo + sh.per < n ? lo + sh.per : n;
  uint32_t mine[2] = {};  // failed, ok
  uint64_t data_len = 0;
  for (uint64_t i = lo + threadIdx.x; i < hi; i += 256) {
    hf3fs_crc_client_write_io io = answer_of(ios, i, n);
    if (updates && io.status == 0) {
      client_write_take_update(io, outcome_of(updates, i, n));
      hf3fs_crc_client_write_io* o = ios + i;
      o->status_in = io.status_in;
      o->result_len = io.result_len;
      o->result_checksum = io.result_checksum;
      o->result_checksum_type = io.result_checksum_type;
    }
    const CwAnswer a = client_write_answer(io);
    const bool failed = a.status != 0;
    take[i] = failed ? 1 : 0;
    mine[0] += failed ? 1u : 0u;
    mine[1] += failed ? 0u : 1u;
    data_len += failed ? 0u : a.result_len;
  }
  sum_counts(mine, total);
  data_len = wave_sum64(data_len);
  if ((threadIdx.x & 63) == 0 && data_len) atomicAdd(&bytes, (unsigned long long)data_len);
  __syncthreads();
  if (threadIdx.x == 0) {
    count[blockIdx.x] = total[0];  // (word 0, the failed IOs, is the scan's: their sum over the shares)
    if (total[1]) atomicAdd(&info[HF3FS_CLIENT_WRITE_DONE_OK], total[1]);
    add_info64(info, HF3FS_CLIENT_WRITE_DONE_LEN_LO, bytes);
  }
}

// One workgroup: the exclusive sums of the count array, and the failed count.
__global__ __launch_bounds__(256) void k_client_write_scan(uint32_t* __restrict__ count, const uint32_t nb,
                                                           uint32_t* __restrict__ info) {
  static_assert(kClientWriteBlocksMax == 256 * 8, "compact_scan_counts: eight entries per thread");
  __shared__ uint32_t sums[256];
  const uint32_t upto = compact_scan_counts(count, nb, sums);
  if (threadIdx.x == 255) info[HF3FS_CLIENT_WRITE_DONE_FAILED] = upto;
}

// Workgroup b writes the failed IOs of its share from its offset on, in index order, below cap.
__global__ __launch_bounds__(256) void k_client_write_scatter(const uint8_t* __restrict__ const take, const uint64_t n,
                                                              const uint32_t* __restrict__ const count,
                                                              uint32_t* __restrict__ failed, const uint64_t cap) {
  __shared__ uint32_t wave_n[4];
  const Shares sh = shares_of(n);
  const uint64_t lo = (uint64_t)blockIdx.x * sh.per, hi = lo + sh.per < n ? lo + sh.per : n;
  compact_scatter_share([&](uint64_t i) { return take[i] != 0; }, lo, hi, count[blockIdx.x], failed, cap, wave_n);
}

__device__ __forceinline__ CwSum shfl_down_sum(const CwSum& s, int d) {
  CwSum r;
  r.len = __shfl_down(s.len, d, 64);
  r.length = __shfl_down(s.length, d, 64);
  r.v = __shfl_down(s.v, d, 64);
  r.nv = __shfl_down(s.nv, d, 64);
  r.end = __shfl_down(s.end, d, 64);
  r.end_code = __shfl_down(s.end_code, d, 64);
  r.adopt = __shfl_down(s.adopt, d, 64);
  r.mis = __shfl_down(s.mis, d, 64);
  r.first[0] = __shfl_down(s.first[0], d, 64);
  r.first[1] = __shfl_down(s.first[1], d, 64);
  r.first[2] = __shfl_down(s.first[2], d, 64);
  r.has_nv = __shfl_down(s.has_nv, d, 64);
  return r;
}

// WAVE = false: one lane per file, the reference's loop in registers.
// WAVE = true: one wave per file; lane l summarises its contiguous run of the file's IOs, then the
// ordered tree of client_read_kernels.hip's merge runs over the wave in registers.
template <bool WAVE>
__global__ __launch_bounds__(256) void k_client_write_fold(const hf3fs_crc_client_write_io* __restrict__ const ios,
                                                           const uint64_t n, const uint64_t* __restrict__ file_off,
                                                           const uint64_t n_files,
                                                           const uint32_t* __restrict__ const expected,
                                                           hf3fs_crc_client_write_file* __restrict__ files,
                                                           uint32_t* __restrict__ info,
                                                           const DeviceTables* __restrict__ tabs) {
  __shared__ uint32_t total[2];
  if (threadIdx.x < 2) total[threadIdx.x] = 0;
  __syncthreads();
  const GfTables gf{tabs};
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, threads = (uint64_t)gridDim.x * blockDim.x;
  uint32_t mine[2] = {};  // files with status != 0, files with 7015
  const auto emit = [&](CwFile f, uint64_t p, uint64_t lo) {
    if (expected) client_write_expect(f, HF3FS_LC_REC(expected, p, n_files));
    client_write_file_emit(f, lo, files + p);
    mine[0] += f.status != 0 ? 1u : 0u;
    mine[1] += f.status == HF3FS_CRC_CLIENT_CHECKSUM_MISMATCH && f.failed == kCwNone && expected ? 1u : 0u;
  };
  if (!WAVE) {
    for (uint64_t p = tid; p < n_files; p += threads) {
      uint64_t lo, hi;
      ios_of(file_off, p, n_files, n, &lo, &hi);
      CwFile f = client_write_file_begin();
      for (uint64_t i = lo; i < hi; ++i)
        if (!client_write_seq_step(f, client_write_answer(answer_of(ios, i, n)), (uint32_t)(i - lo), gf)) break;
      emit(f, p, lo);
    }
  } else {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t p = tid >> 6; p < n_files; p += threads >> 6) {  // wave-uniform
      uint64_t lo, hi;
      ios_of(file_off, p, n_files, n, &lo, &hi);
      const uint64_t k = hi - lo, run = (k + 63) / 64;
      CwSum acc = client_write_sum_identity();
      for (uint64_t j = lane * run, e = j + run < k ? j + run : k; j < e; ++j)
        acc = client_write_sum_join(acc, client_write_sum_of(client_write_answer(answer_of(ios, lo + j, n)), (uint32_t)j),
                                    gf);
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {  // ordered: lane l joins lane l + d's summary on its right
        const CwSum o = shfl_down_sum(acc, d);
        if ((lane & (2 * d - 1)) == 0) acc = client_write_sum_join(acc, o, gf);
      }
      if (lane == 0) emit(client_write_sum_finish(acc), p, lo);
    }
  }
  sum_counts(mine, total);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (total[0]) atomicAdd(&info[HF3FS_CLIENT_WRITE_DONE_BAD_FILES], total[0]);
    if (total[1]) atomicAdd(&info[HF3FS_CLIENT_WRITE_DONE_MISMATCHED_FILES], total[1]);
  }
}

}  // namespace

size_t client_write_scratch_bytes(uint64_t n) { return ((n + 15) & ~uint64_t(15)) + kClientWriteBlocksMax * 4; }

void client_write_scratch_carve(void* base, uint64_t n, ClientWriteScratch* s) {
  s->count = (uint32_t*)base;
  s->take = (uint8_t*)base + kClientWriteBlocksMax * 4;
  (void)n;
}

hipError_t launch_client_write_prep(const hf3fs_crc_client_write_io* ios, uint64_t n, uint32_t max_len, bool verify,
                                    uint64_t* addr, uint64_t* len, uint32_t* ctl, hipStream_t st) {
  hipLaunchKernelGGL(k_client_write_prep, dim3(grid_of(n)), dim3(256), 0, st, ios, n, max_len, verify, addr, len, ctl);
  return hipGetLastError();
}

hipError_t launch_client_write_prepare_finish(hf3fs_crc_client_write_io* ios, uint64_t n, uint8_t type,
                                              uint32_t max_len, uint32_t max_inline_bytes, bool verify,
                                              const uint32_t* v, const uint32_t* poison, hf3fs_crc_update_io* updates,
                                              uint32_t* info, hipStream_t st) {
  hipLaunchKernelGGL(k_client_write_prepare_finish, dim3(grid_of(n)), dim3(256), 0, st, ios, n, type, max_len,
                     max_inline_bytes, verify, v, poison, updates, info);
  return hipGetLastError();
}

hipError_t launch_client_write_settle(hf3fs_crc_client_write_io* ios, uint64_t n, const hf3fs_crc_update_io* updates,
                                      uint32_t* failed, uint64_t failed_cap, uint32_t* info,
                                      const ClientWriteScratch& s, hipStream_t st) {
  const uint32_t blocks = shares_of(n).blocks;
  hipLaunchKernelGGL(k_client_write_settle, dim3(blocks), dim3(256), 0, st, ios, n, updates, s.take, s.count, info);
  hipLaunchKernelGGL(k_client_write_scan, dim3(1), dim3(256), 0, st, s.count, blocks, info);
  if (failed && failed_cap)
    hipLaunchKernelGGL(k_client_write_scatter, dim3(blocks), dim3(256), 0, st, s.take, n, s.count, failed, failed_cap);
  return hipGetLastError();
}

hipError_t launch_client_write_fold(const hf3fs_crc_client_write_io* ios, uint64_t n, const uint64_t* file_off,
                                    uint64_t n_files, bool wave, const uint32_t* expected,
                                    hf3fs_crc_client_write_file* files, uint32_t* info, const DeviceTables* tabs,
                                    hipStream_t st) {
  if (wave)
    hipLaunchKernelGGL(k_client_write_fold<true>, dim3(grid_of(n_files, 4)), dim3(256), 0, st, ios, n, file_off,
                       n_files, expected, files, info, tabs);
  else
    hipLaunchKernelGGL(k_client_write_fold<false>, dim3(grid_of(n_files)), dim3(256), 0, st, ios, n, file_off, n_files,
                       expected, files, info, tabs);
  return hipGetLastError();
}

}  // namespace hf3fs_crc
