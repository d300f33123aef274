// range_kernels.hip -- see range_kernels.h.  These kernels read 48-byte metadata records, 96-byte
// op records and 64-byte file records, and write the ops' and files' output fields, 4-byte list
// entries, eight info words and the scratch of RangeScratch; no chunk byte is touched.  Every
// decision is range_plan.h's.
//
// Who writes what (one launch per line; a word has one writer per launch):
//   count      workgroup b over its contiguous share of the table: share_cnt[b], share_len[b],
//              share_bad[b]
//   scan       one workgroup: share_cnt and share_len become their exclusive sums; ctl[0]
//   apply      workgroup b walks its share from its offsets on: cnt_pre[i], len_pre[i]; the
//              workgroup whose share ends the table: cnt_pre[n_meta], len_pre[n_meta]
//   ops        one lane per op of workgroup b's share of the ops: the op's outputs but list_first,
//              op_off[i] (its list count), op_top[i]; share_list[b], share_chunks[b], share_ok[b]
//   ops scan   one workgroup: share_list becomes its exclusive sums; ctl[2..3]; every word of d_info
//   ops apply  workgroup b walks its share: op_off[i] becomes the entries before op i, the op's
//              list_first; the workgroup whose share ends the ops: op_off[n_ops]
//   list       one lane per list entry below list_cap: d_list[e]
//   file       one lane per file: its outputs; d_info by atomicAdd (zeroed before)
// Nothing is read that an earlier launch of the same call has not written (option poison).
#include "range_kernels.h"

#include "compact.h"
#include "loadcheck.h"
#include "range_plan.h"

namespace hf3fs_crc {
namespace {

unsigned grid_of(uint64_t n) {
  const uint64_t want = (n + 255) / 256;
  return (unsigned)(want < 4096 ? (want ? want : 1) : 4096);
}

__host__ __device__ inline Shares shares_of(uint64_t n) { return ::hf3fs_crc::shares_of(n, kRangeBlocksMax); }

// Workgroup b's share [lo, hi) of n records, and whether it is the one that ends them (and so
// writes the prefixes' entry n): the share that holds record n - 1, workgroup 0 of an empty table.
struct Share {
  uint64_t lo, hi;
  bool ends;
};
__device__ __forceinline__ Share share_of(const uint64_t n, const uint32_t b) {
  const Shares s = shares_of(n);
  Share r;
  r.lo = (uint64_t)b * s.per;
  r.hi = r.lo + s.per < n ? r.lo + s.per : n;
  if (r.hi < r.lo) r.hi = r.lo;  // (a share past the table: empty)
  r.ends = n ? (r.lo < n && n <= r.lo + s.per) : b == 0;
  return r;
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
  return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int d) {
  const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
  return (uint64_t)hi << 32 | lo;
}

// The sum of v over the workgroup's 256 threads, to every thread.  part: four shared words; the
// caller synchronises before part is reused.
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* part) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += shfl_xor64(v, d);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

// compact_scan_counts for 64-bit entries: cnt[0, nb) (nb <= 2048) becomes its exclusive sums, the
// return value is the inclusive sum up to the calling thread's entries.  sums: 256 shared words.
__device__ __forceinline__ uint64_t scan_counts64(uint64_t* cnt, const uint32_t nb, uint64_t* sums) {
  uint64_t v[8], total = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t at = threadIdx.x * 8 + k;
    v[k] = at < nb ? cnt[at] : 0ull;
    total += v[k];
  }
  sums[threadIdx.x] = total;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint64_t add = threadIdx.x >= d ? sums[threadIdx.x - d] : 0ull;
    __syncthreads();
    sums[threadIdx.x] += add;
    __syncthreads();
  }
  const uint64_t upto = sums[threadIdx.x];
  uint64_t run = upto - total;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t at = threadIdx.x * 8 + k;
    if (at < nb) cnt[at] = run;
    run += v[k];
  }
  return upto;
}

// The tile's exclusive sums of v in thread order: returns the sum of the threads before the
// caller, *tile the sum of all 256.  wave_v: four shared words; ends with a barrier.
__device__ __forceinline__ uint64_t tile_exclusive64(const uint64_t v, uint64_t* wave_v, uint64_t* tile) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = shfl_up64(inc, d);
    if (lane >= (uint32_t)d) inc += up;
  }
  if (lane == 63) wave_v[wave] = inc;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    const uint64_t c = wave_v[w];
    before += w < wave ? c : 0ull;
    all += c;
  }
  __syncthreads();
  *tile = all;
  return before + inc - v;
}

__global__ __launch_bounds__(256) void k_range_count(const hf3fs_crc_sync_meta* __restrict__ const meta,
                                                     const uint64_t n, uint32_t* __restrict__ share_cnt,
                                                     uint64_t* __restrict__ share_len,
                                                     uint32_t* __restrict__ share_bad) {
  __shared__ uint64_t part[4];
  const Share sh = share_of(n, blockIdx.x);
  uint64_t cnt = 0, len = 0, bad = 0;
  for (uint64_t i = sh.lo + threadIdx.x; i < sh.hi; i += 256) {
    const hf3fs_crc_sync_meta m = HF3FS_LC_REC(meta, i, n);
    if (m.recycle_state == 0) {
      ++cnt;
      len += m.length;
    }
    if (i >= 1) {
      const hf3fs_crc_sync_meta p = HF3FS_LC_REC(meta, i - 1, n);
      bad += range_id_less(p.id_hi, p.id_lo, m.id_hi, m.id_lo) ? 0u : 1u;
    }
  }
  cnt = block_sum(cnt, part);
  __syncthreads();
  len = block_sum(len, part);
  __syncthreads();
  bad = block_sum(bad, part);
  if (threadIdx.x == 0) {
    share_cnt[blockIdx.x] = (uint32_t)cnt;
    share_len[blockIdx.x] = len;
    share_bad[blockIdx.x] = (uint32_t)bad;
  }
}

__global__ __launch_bounds__(256) void k_range_scan(uint32_t* __restrict__ share_cnt, uint64_t* __restrict__ share_len,
                                                    const uint32_t* __restrict__ const share_bad, const uint32_t nb,
                                                    uint32_t* __restrict__ ctl) {
  static_assert(kRangeBlocksMax == 256 * 8, "k_range_scan: eight entries per thread");
  __shared__ uint32_t sums[256];
  __shared__ uint64_t sums64[256];
  __shared__ uint64_t part[4];
  (void)compact_scan_counts(share_cnt, nb, sums);
  (void)scan_counts64(share_len, nb, sums64);
  uint64_t bad = 0;
  for (uint32_t at = threadIdx.x; at < nb; at += 256) bad += share_bad[at];
  bad = block_sum(bad, part);
  if (threadIdx.x == 0) ctl[0] = (uint32_t)bad;  // (< n_meta <= 2^30)
}

__global__ __launch_bounds__(256) void k_range_apply(const hf3fs_crc_sync_meta* __restrict__ const meta,
                                                     const uint64_t n, const uint32_t* __restrict__ const share_cnt,
                                                     const uint64_t* __restrict__ const share_len,
                                                     uint32_t* __restrict__ cnt_pre, uint64_t* __restrict__ len_pre) {
  __shared__ uint32_t wave_n[4];
  __shared__ uint64_t wave_v[4];
  const Share sh = share_of(n, blockIdx.x);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t base_c = share_cnt[blockIdx.x];
  uint64_t base_l = share_len[blockIdx.x];
  for (uint64_t i0 = sh.lo; i0 < sh.hi; i0 += 256) {  // workgroup-uniform
    const uint64_t i = i0 + threadIdx.x;
    bool normal = false;
    uint64_t v = 0;
    if (i < sh.hi) {
      const hf3fs_crc_sync_meta m = HF3FS_LC_REC(meta, i, n);
      normal = m.recycle_state == 0;
      v = normal ? m.length : 0u;
    }
    const unsigned long long votes = __ballot(normal);
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(votes);
    uint64_t tile_l;
    const uint64_t before_l = tile_exclusive64(v, wave_v, &tile_l);  // (its first barrier covers wave_n)
    uint32_t before_c = 0, tile_c = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t c = wave_n[w];
      before_c += w < wave ? c : 0u;
      tile_c += c;
    }
    if (i < sh.hi) {
      cnt_pre[i] = base_c + before_c + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
      len_pre[i] = base_l + before_l;
    }
    base_c += tile_c;
    base_l += tile_l;
    __syncthreads();
  }
  if (sh.ends && threadIdx.x == 0) {
    cnt_pre[n] = base_c;
    len_pre[n] = base_l;
  }
}

__device__ __forceinline__ void store_outputs(hf3fs_crc_range_op* o, const hf3fs_crc_range_op& op) {
  o->last_hi = op.last_hi;
  o->last_lo = op.last_lo;
  o->total_len = op.total_len;
  o->total_chunks = op.total_chunks;
  o->last_len = op.last_len;
  o->last_index = op.last_index;
  o->status = op.status;
  o->more = op.more;
  o->reserved1[0] = o->reserved1[1] = o->reserved1[2] = 0;
}

__global__ __launch_bounds__(256) void k_range_ops(const hf3fs_crc_sync_meta* __restrict__ const meta,
                                                   const uint64_t n_meta, hf3fs_crc_range_op* __restrict__ ops,
                                                   const uint64_t n_ops, const uint32_t* __restrict__ const ctl,
                                                   const uint32_t* __restrict__ const cnt_pre,
                                                   const uint64_t* __restrict__ const len_pre,
                                                   uint64_t* __restrict__ op_off, uint32_t* __restrict__ op_top,
                                                   uint64_t* __restrict__ share_list,
                                                   uint64_t* __restrict__ share_chunks,
                                                   uint32_t* __restrict__ share_ok) {
  __shared__ uint64_t part[4];
  const Share sh = share_of(n_ops, blockIdx.x);
  const bool unsorted = ctl[0] != 0;
  uint64_t listed = 0, chunks = 0, ok = 0;
  for (uint64_t i = sh.lo + threadIdx.x; i < sh.hi; i += 256) {
    hf3fs_crc_range_op op = HF3FS_LC_REC(ops, i, n_ops);
    const RangeOpPlan p = range_op_plan(
        op, unsorted, n_meta,
        [&](uint64_t r, uint64_t hi, uint64_t lo) {
          const hf3fs_crc_sync_meta m = HF3FS_LC_REC(meta, r, n_meta);
          return range_id_less(m.id_hi, m.id_lo, hi, lo);
        },
        [&](uint64_t r) { return cnt_pre[r]; }, [&](uint64_t r) { return len_pre[r]; },
        [&](uint64_t r, uint64_t* hi, uint64_t* lo, uint32_t* length) {
          const hf3fs_crc_sync_meta m = HF3FS_LC_REC(meta, r, n_meta);
          *hi = m.id_hi;
          *lo = m.id_lo;
          *length = m.length;
        });
    store_outputs(ops + i, op);
    op_off[i] = p.list_n;
    op_top[i] = p.top;
    listed += p.list_n;
    chunks += op.total_chunks;
    ok += op.status == 0 ? 1u : 0u;
  }
  listed = block_sum(listed, part);
  __syncthreads();
  chunks = block_sum(chunks, part);
  __syncthreads();
  ok = block_sum(ok, part);
  if (threadIdx.x == 0) {
    share_list[blockIdx.x] = listed;
    share_chunks[blockIdx.x] = chunks;
    share_ok[blockIdx.x] = (uint32_t)ok;
  }
}

__global__ __launch_bounds__(256) void k_range_ops_scan(uint64_t* __restrict__ share_list,
                                                        const uint64_t* __restrict__ const share_chunks,
                                                        const uint32_t* __restrict__ const share_ok, const uint32_t nb,
                                                        const uint64_t n_ops, const uint64_t list_cap,
                                                        uint32_t* __restrict__ ctl, uint32_t* __restrict__ info) {
  __shared__ uint64_t sums64[256];
  __shared__ uint64_t part[4];
  const uint64_t upto = scan_counts64(share_list, nb, sums64);  // thread 255: every list entry
  uint64_t chunks = 0, ok = 0;
  for (uint32_t at = threadIdx.x; at < nb; at += 256) {
    chunks += share_chunks[at];
    ok += share_ok[at];
  }
  chunks = block_sum(chunks, part);
  __syncthreads();
  ok = block_sum(ok, part);
  if (threadIdx.x == 255) {
    ctl[2] = (uint32_t)upto;
    ctl[3] = (uint32_t)(upto >> 32);
    info[HF3FS_RANGE_INFO_OPS_OK] = (uint32_t)ok;
    info[HF3FS_RANGE_INFO_OPS_FAILED] = (uint32_t)(n_ops - ok);
    info[HF3FS_RANGE_INFO_CHUNKS_LO] = (uint32_t)chunks;
    info[HF3FS_RANGE_INFO_CHUNKS_HI] = (uint32_t)(chunks >> 32);
    info[HF3FS_RANGE_INFO_LIST_LO] = (uint32_t)upto;
    info[HF3FS_RANGE_INFO_LIST_HI] = (uint32_t)(upto >> 32);
    info[HF3FS_RANGE_INFO_OVERFLOW] = upto > list_cap ? 1u : 0u;
    info[HF3FS_RANGE_INFO_UNSORTED] = ctl[0];
  }
}

__global__ __launch_bounds__(256) void k_range_ops_apply(hf3fs_crc_range_op* __restrict__ ops, const uint64_t n_ops,
                                                         const uint64_t* __restrict__ const share_list,
                                                         uint64_t* __restrict__ op_off) {
  __shared__ uint64_t wave_v[4];
  const Share sh = share_of(n_ops, blockIdx.x);
  uint64_t base = share_list[blockIdx.x];
  for (uint64_t i0 = sh.lo; i0 < sh.hi; i0 += 256) {  // workgroup-uniform
    const uint64_t i = i0 + threadIdx.x;
    const uint64_t v = i < sh.hi ? op_off[i] : 0ull;
    uint64_t tile;
    const uint64_t before = tile_exclusive64(v, wave_v, &tile);
    if (i < sh.hi) {
      op_off[i] = base + before;
      ops[i].list_first = range_list_first(base + before);
    }
    base += tile;
  }
  if (sh.ends && threadIdx.x == 0) op_off[n_ops] = base;
}

__global__ __launch_bounds__(256) void k_range_list(const uint64_t n_meta, const uint64_t n_ops,
                                                    const uint32_t* __restrict__ const cnt_pre,
                                                    const uint64_t* __restrict__ const op_off,
                                                    const uint32_t* __restrict__ const op_top,
                                                    const uint32_t* __restrict__ const ctl,
                                                    uint32_t* __restrict__ list, const uint64_t list_cap) {
  const uint64_t total = (uint64_t)ctl[3] << 32 | ctl[2];
  const uint64_t m = total < list_cap ? total : list_cap;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x)
    list[e] = range_list_entry(
        e, n_ops, n_meta, [&](uint64_t j) { return op_off[j]; }, [&](uint64_t j) { return op_top[j]; },
        [&](uint64_t r) { return cnt_pre[r]; });
}

__global__ __launch_bounds__(64) void k_file_length(const hf3fs_crc_range_op* __restrict__ const ops,
                                                    const uint64_t n_ops, hf3fs_crc_file_len* __restrict__ files,
                                                    const uint64_t n_files, uint32_t* __restrict__ info) {
  uint32_t mine[6] = {};
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_files; i += (uint64_t)gridDim.x * blockDim.x) {
    hf3fs_crc_file_len f = HF3FS_LC_REC(files, i, n_files);
    const RangeFileCounts c = range_file_fold(
        f, n_ops, [&](uint64_t k) { return HF3FS_LC_REC(ops, k, n_ops); },
        [&](uint64_t k) { return HF3FS_LC_REC(ops, k, n_ops).chain_id; });
    hf3fs_crc_file_len* o = files + i;
    o->status = f.status;
    o->length = f.length;
    o->total_len = f.total_len;
    o->total_chunks = f.total_chunks;
    o->last_chunk = f.last_chunk;
    o->last_chunk_len = f.last_chunk_len;
    mine[HF3FS_FILE_LEN_INFO_OK] += f.status == 0 ? 1u : 0u;
    mine[HF3FS_FILE_LEN_INFO_FAILED] += f.status != 0 ? 1u : 0u;
    mine[HF3FS_FILE_LEN_INFO_EMPTY] += c.empty ? 1u : 0u;
    mine[HF3FS_FILE_LEN_INFO_NOT_FOUND] += c.not_found;
    mine[HF3FS_FILE_LEN_INFO_BUSY] += f.status == kRangeBusy ? 1u : 0u;
    mine[HF3FS_FILE_LEN_INFO_CORRUPT] += f.status == kRangeDataCorruption ? 1u : 0u;
  }
#pragma unroll
  for (int w = 0; w < 6; ++w) {  // (one wave per workgroup)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine[w] += __shfl_xor(mine[w], d, 64);
    if (threadIdx.x == 0 && mine[w]) atomicAdd(&info[w], mine[w]);
  }
}

}  // namespace

size_t range_scratch_bytes(uint64_t n_meta, uint64_t n_ops) {
  // len_pre[n_meta + 1] 8, op_off[n_ops + 1] 8, three share arrays of 8, cnt_pre[n_meta + 1] 4,
  // op_top[n_ops] 4, three share arrays of 4, ctl[4] 4, up to a multiple of 16
  return ((n_meta + 1) * 12 + (n_ops + 1) * 8 + n_ops * 4 + kRangeBlocksMax * 36 + 16 + 15) & ~size_t(15);
}

void range_scratch_carve(void* base, uint64_t n_meta, uint64_t n_ops, RangeScratch* s) {
  s->len_pre = (uint64_t*)base;
  s->op_off = s->len_pre + n_meta + 1;
  s->share_len = s->op_off + n_ops + 1;
  s->share_list = s->share_len + kRangeBlocksMax;
  s->share_chunks = s->share_list + kRangeBlocksMax;
  s->cnt_pre = (uint32_t*)(s->share_chunks + kRangeBlocksMax);
  s->op_top = s->cnt_pre + n_meta + 1;
  s->share_cnt = s->op_top + n_ops;
  s->share_bad = s->share_cnt + kRangeBlocksMax;
  s->share_ok = s->share_bad + kRangeBlocksMax;
  s->ctl = s->share_ok + kRangeBlocksMax;
}

hipError_t launch_range_query(const hf3fs_crc_sync_meta* meta, uint64_t n_meta, hf3fs_crc_range_op* ops,
                              uint64_t n_ops, uint32_t* list, uint64_t list_cap, uint32_t* info,
                              const RangeScratch& s, hipStream_t st) {
  const unsigned tb = shares_of(n_meta).blocks, ob = shares_of(n_ops).blocks;
  hipLaunchKernelGGL(k_range_count, dim3(tb), dim3(256), 0, st, meta, n_meta, s.share_cnt, s.share_len, s.share_bad);
  hipLaunchKernelGGL(k_range_scan, dim3(1), dim3(256), 0, st, s.share_cnt, s.share_len, s.share_bad, tb, s.ctl);
  hipLaunchKernelGGL(k_range_apply, dim3(tb), dim3(256), 0, st, meta, n_meta, s.share_cnt, s.share_len, s.cnt_pre,
                     s.len_pre);
  hipLaunchKernelGGL(k_range_ops, dim3(ob), dim3(256), 0, st, meta, n_meta, ops, n_ops, s.ctl, s.cnt_pre, s.len_pre,
                     s.op_off, s.op_top, s.share_list, s.share_chunks, s.share_ok);
  hipLaunchKernelGGL(k_range_ops_scan, dim3(1), dim3(256), 0, st, s.share_list, s.share_chunks, s.share_ok, ob, n_ops,
                     list_cap, s.ctl, info);
  hipLaunchKernelGGL(k_range_ops_apply, dim3(ob), dim3(256), 0, st, ops, n_ops, s.share_list, s.op_off);
  hipLaunchKernelGGL(k_range_list, dim3(grid_of(list_cap)), dim3(256), 0, st, n_meta, n_ops, s.cnt_pre, s.op_off,
                     s.op_top, s.ctl, list, list_cap);
  return hipGetLastError();
}

hipError_t launch_file_length(const hf3fs_crc_range_op* ops, uint64_t n_ops, hf3fs_crc_file_len* files,
                              uint64_t n_files, uint32_t* info, hipStream_t st) {
  // one lane per file, 64-thread workgroups: few files of many ops spread over the CUs
  const uint64_t want = (n_files + 63) / 64;
  hipLaunchKernelGGL(k_file_length, dim3((unsigned)(want < 16384 ? (want ? want : 1) : 16384)), dim3(64), 0, st, ops,
                     n_ops, files, n_files, info);
  return hipGetLastError();
}

}  // namespace hf3fs_crc
