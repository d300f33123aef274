// range_plan.h -- the decisions of hf3fs_crc_range_query and hf3fs_crc_file_length, plain C++ that
// both the device compiler and a host compiler take.
//
// range_query: the closed form of StorageOperator::processQueryResults (src/storage/service/
// StorageOperator.cc:653-751) over ChunkStore::queryChunks (src/storage/store/ChunkStore.cc:120-147)
// with queryLastChunk's (:875-891) and removeChunks' (:949-971) processors, on a table that is
// strictly ascending by id and carries exclusive prefixes of its normal records' count and length.
// file_length: FileOperation::queryChunksByChain / queryChunks (src/fbs/meta/FileOperation.cc:
// 45-179), stated without an order of evaluation: the first failing op in op order, else the
// maximum over the ops no later op of the same chain replaces.
// The kernels of range_kernels.hip decide nothing else; tests/cpp/fuzz_range_plan.cpp includes this
// header and holds it to restatements of the paged loop and of the std::map fold under ASan + UBSan.
#pragma once
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

#ifdef __HIPCC__
#define HF3FS_RANGE_FN __host__ __device__ __forceinline__
#else
#define HF3FS_RANGE_FN inline
#endif

namespace hf3fs_crc {

constexpr uint64_t kRangeMaxCount = 1ull << 30;    // 32-bit indices and count prefixes
constexpr uint32_t kRangeNone = 0xFFFFFFFFu;       // no last chunk; a saturated list_first
constexpr uint32_t kRangeLimitMax = 0xFFFFFFFEu;   // UINT32_MAX - 1 (:658-660)
constexpr int32_t kRangeInvalidArg = 3;            // StatusCode::kInvalidArg
constexpr int32_t kRangeDataCorruption = 2;        // StatusCode::kDataCorruption
constexpr int32_t kRangeChunkNotFound = 7007;      // StorageClientCode::kChunkNotFound
constexpr int32_t kRangeBusy = 3019;               // MetaCode::kBusy

// ChunkId's operator< over the 16 bytes of ChunkId(high, low) (Common.cc:10-18): big-endian, so
// the unsigned pair.
HF3FS_RANGE_FN bool range_id_less(uint64_t ahi, uint64_t alo, uint64_t bhi, uint64_t blo) {
  return ahi < bhi || (ahi == bhi && alo < blo);
}

// The first i of [0, n) with !before(i), n if there is none; before is true on a prefix of [0, n).
// Probes only indices below n.
template <class Before>
HF3FS_RANGE_FN uint64_t range_partition_point(uint64_t n, const Before before) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (before(mid))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

HF3FS_RANGE_FN uint32_t range_limit(uint32_t max_chunks) {
  return max_chunks ? (max_chunks < kRangeLimitMax ? max_chunks : kRangeLimitMax) : kRangeLimitMax;
}

// The table record that holds the normal record of rank r (r normal records lie before it), given
// cnt(i) = normal records of [0, i) for i in [0, n_meta]: the last i with cnt(i) <= r.  r < cnt(n_meta).
template <class Cnt>
HF3FS_RANGE_FN uint64_t range_record_of_rank(uint64_t n_meta, uint32_t r, const Cnt cnt) {
  // cnt(i + 1) <= r holds on a prefix of i in [0, n_meta); the probe cnt(i + 1) stays <= n_meta
  return range_partition_point(n_meta, [&](uint64_t i) { return cnt(i + 1) <= r; });
}

// What one op leaves behind besides its record.
struct RangeOpPlan {
  uint32_t list_n;  // entries of its list segment
  uint32_t top;     // normal records of the table below the span's end: entry k of the segment is the
                    // normal record of rank top - 1 - k
};

// One op.  op's outputs but list_first are set; list_first is the caller's (a sum over the ops
// before).  id_lt(i, hi, lo): is record i's id below (hi, lo); cnt / len: the prefixes, n_meta + 1
// entries; last(i, &hi, &lo, &length): record i's id and length.
template <class IdLt, class Cnt, class Len, class Last>
HF3FS_RANGE_FN RangeOpPlan range_op_plan(hf3fs_crc_range_op& op, const bool unsorted, const uint64_t n_meta,
                                         const IdLt id_lt, const Cnt cnt, const Len len, const Last last) {
  op.last_hi = op.last_lo = op.total_len = 0;
  op.total_chunks = op.last_len = 0;
  op.last_index = kRangeNone;
  op.more = 0;
  op.reserved1[0] = op.reserved1[1] = op.reserved1[2] = 0;
  RangeOpPlan p{0, 0};
  if (unsorted) {
    op.status = kRangeInvalidArg;
    return p;
  }
  if (op.status_in != 0) {
    op.status = op.status_in;
    return p;
  }
  if (op.kind != HF3FS_RANGE_QUERY && op.kind != HF3FS_RANGE_REMOVE) {
    op.status = kRangeInvalidArg;
    return p;
  }
  op.status = 0;
  if (!range_id_less(op.begin_hi, op.begin_lo, op.end_hi, op.end_lo)) return p;  // [begin, end) is empty
  // the span [a, b): the first record with id >= begin, the first with id >= end
  const uint64_t a = range_partition_point(n_meta, [&](uint64_t i) { return id_lt(i, op.begin_hi, op.begin_lo); });
  const uint64_t b = range_partition_point(n_meta, [&](uint64_t i) { return id_lt(i, op.end_hi, op.end_lo); });
  const uint32_t below = cnt(a), top = cnt(b);
  const uint32_t normals = top - below, limit = range_limit(op.max_chunks);
  const uint32_t total = normals < limit ? normals : limit;
  op.more = normals > limit ? 1 : 0;
  op.total_chunks = total;
  p.top = top;
  if (total == 0) return p;
  // the lowest processed record (rank top - total) and the last chunk (rank top - 1)
  const uint64_t low = total == normals ? a : range_record_of_rank(n_meta, top - total, cnt);
  const uint64_t high = range_record_of_rank(n_meta, top - 1, cnt);
  op.total_len = len(b) - len(low);
  op.last_index = (uint32_t)high;
  last(high, &op.last_hi, &op.last_lo, &op.last_len);
  p.list_n = op.kind == HF3FS_RANGE_REMOVE ? total : 0u;
  return p;
}

HF3FS_RANGE_FN uint32_t range_list_first(uint64_t running) { return running < kRangeNone ? (uint32_t)running : kRangeNone; }

// List entry e: its op is the last j with off(j) <= e (off: the n_ops + 1 exclusive sums of the list
// counts, e < off(n_ops)), its record the normal record of rank top(j) - 1 - (e - off(j)).
template <class Off, class Top, class Cnt>
HF3FS_RANGE_FN uint32_t range_list_entry(uint64_t e, uint64_t n_ops, uint64_t n_meta, const Off off, const Top top,
                                         const Cnt cnt) {
  const uint64_t j = range_partition_point(n_ops, [&](uint64_t i) { return off(i + 1) <= e; });
  const uint32_t r = top(j) - 1u - (uint32_t)(e - off(j));
  return (uint32_t)range_record_of_rank(n_meta, r, cnt);
}

// ---- hf3fs_crc_file_length ----

HF3FS_RANGE_FN uint64_t range_id_inode(uint64_t hi, uint64_t lo) { return (hi & 0xFFFFFFFFFFFFull) << 16 | lo >> 48; }
HF3FS_RANGE_FN uint64_t range_id_chunk(uint64_t lo) { return lo & 0xFFFFFFFFull; }
// meta::ChunkId(InodeId(-1), 0, 0): what ChunkId::unpack leaves when it fails (Schema.h:201-207,223).
HF3FS_RANGE_FN bool range_id_invalid(uint64_t hi, uint64_t lo) {
  return hi == 0x0000FFFFFFFFFFFFull && lo == 0xFFFF000000000000ull;
}

enum RangeFileOp : uint8_t { kRangeOpNotFound = 0, kRangeOpEmpty, kRangeOpFails, kRangeOpEnters };

// What one op of a file does to it (:127-176), by itself: `code` when it fails.
HF3FS_RANGE_FN RangeFileOp range_file_op(const hf3fs_crc_range_op& op, const hf3fs_crc_file_len& f, int32_t* code) {
  if (op.status != 0) {
    if (op.status == kRangeChunkNotFound) return kRangeOpNotFound;
    *code = op.status;
    return kRangeOpFails;
  }
  if (op.total_chunks == 0) return kRangeOpEmpty;
  *code = kRangeDataCorruption;
  if (range_id_invalid(op.last_hi, op.last_lo)) return kRangeOpFails;
  if (range_id_inode(op.last_hi, op.last_lo) != f.inode) return kRangeOpFails;
  *code = kRangeBusy;
  if ((f.flags & HF3FS_FILE_LEN_DYN) && f.n_file_ops < f.stripe_size && range_id_chunk(op.last_lo) >= f.n_file_ops)
    return kRangeOpFails;
  *code = 0;
  return kRangeOpEnters;
}

struct RangeFileCounts {
  uint32_t not_found;  // 7007 ops before the first failing op
  bool empty;          // status 0 and no entry
};

// One file.  op_at(i) is op i of the caller's array, chain_at(i) its chain_id; f's outputs are set.
// Order-free: the file's status is the code of its first failing op in op order; else an op that
// enters counts unless a later op of the file that enters has its chain_id, and among those that
// count the greatest length wins, on equal lengths the lowest chain_id.
template <class OpAt, class ChainAt>
HF3FS_RANGE_FN RangeFileCounts range_file_fold(hf3fs_crc_file_len& f, const uint64_t n_ops, const OpAt op_at,
                                               const ChainAt chain_at) {
  f.status = 0;
  f.length = f.total_len = f.total_chunks = 0;
  f.last_chunk = f.last_chunk_len = 0;
  RangeFileCounts c{0, false};
  if (f.n_file_ops > HF3FS_FILE_LEN_MAX_OPS || (uint64_t)f.first_op + f.n_file_ops > n_ops) {
    f.status = kRangeInvalidArg;
    return c;
  }
  const uint64_t lo = f.first_op, hi = lo + f.n_file_ops;
  for (uint64_t i = lo; i < hi; ++i) {
    int32_t code = 0;
    const RangeFileOp what = range_file_op(op_at(i), f, &code);
    if (what == kRangeOpNotFound) ++c.not_found;
    if (what == kRangeOpFails) {
      f.status = code;
      return c;
    }
  }
  bool any = false;
  uint32_t best_chain = 0;
  for (uint64_t i = lo; i < hi; ++i) {
    int32_t code = 0;
    const hf3fs_crc_range_op op = op_at(i);
    if (range_file_op(op, f, &code) != kRangeOpEnters) continue;
    bool replaced = false;
    for (uint64_t j = i + 1; j < hi && !replaced; ++j)
      replaced = chain_at(j) == op.chain_id && range_file_op(op_at(j), f, &code) == kRangeOpEnters;
    if (replaced) continue;
    const uint64_t chunk = range_id_chunk(op.last_lo);
    const uint64_t length = chunk * f.chunk_size + op.last_len;
    if (!any || length > f.length || (length == f.length && op.chain_id < best_chain)) {
      f.length = length;
      f.last_chunk = (uint32_t)chunk;
      f.last_chunk_len = op.last_len;
      best_chain = op.chain_id;
    }
    any = true;
    f.total_len += op.total_len;
    f.total_chunks += op.total_chunks;
  }
  c.empty = !any;
  return c;
}

}  // namespace hf3fs_crc
