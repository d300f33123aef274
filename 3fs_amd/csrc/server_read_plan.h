// server_read_plan.h -- the decisions of hf3fs_crc_server_read_prepare and
// hf3fs_crc_server_read_complete, plain C++ that both the device compiler and a host compiler
// take, on the pattern of forward_plan.h: what StorageOperator::batchRead
// (src/storage/service/StorageOperator.cc:98-226), AioReadJob (src/storage/aio/BatchReadJob.cc:16-113),
// setReadJobResult (src/storage/aio/AioStatus.cc:27-55), aioPrepareRead / aioFinishRead
// (src/storage/store/ChunkReplica.cc:38-100, ChunkEngine.h:34-73, StorageTarget.cc:299-304),
// BufferPool::Buffer (src/storage/service/BufferPool.cc:102-141) and RDMAReqBatch::add
// (src/common/net/ib/IBSocket.cc:258-275) make of one ReadIO.  Hashing and copying are not done
// here: a caller asks server_read_route whether a job hashes, hashes those bytes, and hands the
// value to server_read_settle.  The kernels of server_read_kernels.hip keep no ladder of their
// own, and tests/cpp/fuzz_server_read.cpp runs these functions against a sequential restatement of
// the reference's control flow under ASan + UBSan.
#pragma once
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

#ifdef __HIPCC__
#define HF3FS_SRD_FN __host__ __device__ __forceinline__
#else
#define HF3FS_SRD_FN inline
#endif

namespace hf3fs_crc {

constexpr uint64_t kServerReadMaxCount = 1ull << 30;
constexpr uint32_t kServerReadAlign = 4096;       // kAIOAlignSize
constexpr uint32_t kServerReadRawEmpty = ~0u;     // the raw CRC of no bytes, either polynomial

// ---------------------------------------------------------------------------------------------
// prepare

struct ServerReadAlign {
  uint32_t head, tail, read_len;
};
// AioReadJob::AioReadJob (BatchReadJob.cc:20-21) and alignedLength(), in wrapping uint32_t.
HF3FS_SRD_FN ServerReadAlign server_read_align(uint32_t offset, uint32_t length) {
  ServerReadAlign a;
  a.head = offset % kServerReadAlign;
  a.tail = (kServerReadAlign - (uint32_t)(offset + length) % kServerReadAlign) % kServerReadAlign;
  a.read_len = length + a.head + a.tail;
  return a;
}

// One job of the first loop (StorageOperator.cc:101-130): 0, or the code that ends the request.
HF3FS_SRD_FN int32_t server_read_first_check(const hf3fs_crc_server_read_job& j) {
  if (j.target_status != 0) return j.target_status;                  // :107-111
  if (!j.up_to_date) return HF3FS_CRC_TARGET_STATE_INVALID;          // :113-117
  if (j.length > j.rdmabuf_size) return HF3FS_CRC_INVALID_ARG;       // :122-128
  return 0;
}

// BufferPool::Buffer of one request: indices_.size(), and current_'s kind, size and room.
struct ServerReadCarve {
  uint32_t taken;   // buffers so far
  uint32_t cap;     // the current buffer's size
  uint32_t room;    // bytes left in it
  uint32_t n_small, n_big;
  uint8_t kind;
};
struct ServerReadPlace {
  int32_t status;
  uint32_t ordinal, off;
  uint8_t kind;
};
HF3FS_SRD_FN ServerReadCarve server_read_carve_begin() { return ServerReadCarve{0, 0, 0, 0, 0, HF3FS_SERVER_READ_BUF_NONE}; }
// tryAllocate, then allocate (BufferPool.cc:102-141): a next-fit walk.
HF3FS_SRD_FN ServerReadPlace server_read_carve_take(ServerReadCarve& c, uint32_t size, uint32_t small_buf,
                                                    uint32_t big_buf) {
  if (c.taken == 0 || c.room < size) {                                // :103,122
    if (size > big_buf) return ServerReadPlace{HF3FS_CRC_RDMA_NO_BUF, 0, 0, HF3FS_SERVER_READ_BUF_NONE};  // :123-124
    if (size > small_buf) {                                           // :125-129
      c.kind = HF3FS_SERVER_READ_BUF_BIG;
      c.cap = c.room = big_buf;
      c.n_big++;
    } else {                                                          // :107-110,130-134
      c.kind = HF3FS_SERVER_READ_BUF_SMALL;
      c.cap = c.room = small_buf;
      c.n_small++;
    }
    c.taken++;
  }
  const ServerReadPlace p{0, c.taken - 1, c.cap - c.room, c.kind};   // takeFirst (:115,137)
  c.room -= size;
  return p;
}

// The stored checksum as complete reads it (ChunkReplica.cc:59, ChunkEngine.h:65).
HF3FS_SRD_FN uint8_t server_read_stored_type(const hf3fs_crc_server_read_job& j) {
  return j.engine ? (uint8_t)HF3FS_CHECKSUM_CRC32C : j.chunk_checksum_type;
}
HF3FS_SRD_FN uint32_t server_read_stored_value(const hf3fs_crc_server_read_job& j) {
  return j.engine ? ~j.chunk_checksum : j.chunk_checksum;
}

// The prepare outputs of a job of a failed request.
HF3FS_SRD_FN void server_read_fail_job(hf3fs_crc_server_read_job& j, int32_t code) {
  const ServerReadAlign a = server_read_align(j.offset, j.length);
  j.head_len = a.head;
  j.tail_len = a.tail;
  j.read_len = 0;
  j.read_offset = 0;
  j.buf_ordinal = 0;
  j.buf_off = 0;
  j.buf_kind = HF3FS_SERVER_READ_BUF_NONE;
  j.status = code;
}

// The prepare outputs of a job of a passing request: its place, then aioPrepareRead.
HF3FS_SRD_FN void server_read_prepare_job(hf3fs_crc_server_read_job& j, const ServerReadPlace& p,
                                          bool read_uncommitted) {
  const ServerReadAlign a = server_read_align(j.offset, j.length);
  j.head_len = a.head;
  j.tail_len = a.tail;
  j.read_len = a.read_len;
  j.buf_ordinal = p.ordinal;
  j.buf_off = p.off;
  j.buf_kind = p.kind;
  j.read_offset = 0;
  if (j.meta_status != 0) {                                           // ChunkReplica.cc:46-50, ChunkEngine.h:48-54
    j.status = j.meta_status;
    return;
  }
  if (j.engine) {
    j.commit_ver = j.update_ver;                                      // ChunkEngine.h:61-62
  } else if (j.commit_ver != j.update_ver && !read_uncommitted) {     // ChunkReplica.cc:61-66
    j.status = HF3FS_CRC_CHUNK_NOT_COMMIT;
    return;
  }
  j.read_offset = j.inner_offset + (uint32_t)(j.offset - a.head);     // ChunkReplica.cc:72, ChunkEngine.h:70
  j.status = 0;
}

struct ServerReadPrepCounts {
  uint32_t reqs_ok, reqs_failed, jobs_ok, jobs_failed, n_small, n_big;
};

// One request, jobs [lo, hi) of `jobs`: steps 1-5 of prepare.  get(i) loads record i, put(i, j)
// stores its prepare outputs (and an engine job's commit_ver); the walk keeps nothing else.
template <class Get, class Put>
HF3FS_SRD_FN ServerReadPrepCounts server_read_prepare_request(hf3fs_crc_server_read_req& r, uint64_t lo, uint64_t hi,
                                                              uint32_t small_buf, uint32_t big_buf, const Get get,
                                                              const Put put) {
  ServerReadPrepCounts c{0, 0, 0, 0, 0, 0};
  int32_t code = 0;
  uint64_t failed = 0, total_len = 0, total_head = 0, total_tail = 0;
  for (uint64_t i = lo; i < hi && code == 0; ++i) {                   // StorageOperator.cc:101-130
    const hf3fs_crc_server_read_job j = get(i);
    const ServerReadAlign a = server_read_align(j.offset, j.length);
    code = server_read_first_check(j);
    failed = i;
    total_len += j.length;                                            // :119-121
    total_head += a.head;
    total_tail += a.tail;
  }
  ServerReadCarve carve = server_read_carve_begin();
  for (uint64_t i = lo; i < hi && code == 0; ++i) {                   // :141-154, before any job is enqueued
    const hf3fs_crc_server_read_job j = get(i);
    code = server_read_carve_take(carve, server_read_align(j.offset, j.length).read_len, small_buf, big_buf).status;
    failed = i;
  }
  if (code == 0) {                                                    // the same walk again, and aioPrepareRead
    carve = server_read_carve_begin();
    for (uint64_t i = lo; i < hi; ++i) {
      hf3fs_crc_server_read_job j = get(i);
      const ServerReadPlace p = server_read_carve_take(carve, server_read_align(j.offset, j.length).read_len,
                                                       small_buf, big_buf);
      server_read_prepare_job(j, p, r.read_uncommitted != 0);
      put(i, j);
      c.jobs_ok += j.status == 0 ? 1u : 0u;
      c.jobs_failed += j.status == 0 ? 0u : 1u;
    }
    r.total_len = total_len;
    r.total_head = total_head;
    r.total_tail = total_tail;
    r.n_small = carve.n_small;
    r.n_big = carve.n_big;
  } else {
    r.total_len = r.total_head = r.total_tail = 0;
  }
  r.status = code;
  r.failed_job = code ? (uint32_t)failed : HF3FS_SERVER_READ_NONE;
  if (code != 0) {                                                    // the request is answered with the code
    r.n_small = r.n_big = 0;
    c.jobs_ok = 0;
    c.jobs_failed = (uint32_t)(hi - lo);
    for (uint64_t i = lo; i < hi; ++i) {
      hf3fs_crc_server_read_job j = get(i);
      server_read_fail_job(j, code);
      put(i, j);
    }
  }
  c.reqs_ok = code == 0 ? 1u : 0u;
  c.reqs_failed = code == 0 ? 0u : 1u;
  c.n_small = r.n_small;
  c.n_big = r.n_big;
  return c;
}

// ---------------------------------------------------------------------------------------------
// complete

// Where a job stands before anything is hashed.
struct ServerReadRoute {
  bool live;       // takes part in the rungs
  bool hashes;     // [localbuf + head_len, +len) goes to the range kernels
  int32_t status;  // !live: the job's result_status
  uint32_t len;    // the clipped length L
};

// setReadJobResult's clip (AioStatus.cc:33-34), in signed 64 bits.
HF3FS_SRD_FN uint32_t server_read_clip(const hf3fs_crc_server_read_job& j) {
  int64_t a = j.res - (int64_t)j.head_len;
  if (a < 0) a = 0;
  int64_t b = (int64_t)j.chunk_len - (int64_t)j.offset;
  if (b < 0) b = 0;
  int64_t l = a < (int64_t)j.length ? a : (int64_t)j.length;
  if (b < l) l = b;
  return (uint32_t)l;
}

HF3FS_SRD_FN bool server_read_full(const hf3fs_crc_server_read_job& j, uint32_t len) {
  return j.offset == 0 && len == j.chunk_len;                         // BatchReadJob.cc:30,43
}
// aioFinishRead (StorageTarget.cc:299-304, ChunkReplica.cc:79-100): 0 or its code.
HF3FS_SRD_FN int32_t server_read_finish_check(const hf3fs_crc_server_read_job& j) {
  if (j.engine) return 0;
  if (j.meta_status_now != 0) return j.meta_status_now;
  if (j.update_ver != j.update_ver_now) return HF3FS_CRC_CHUNK_NOT_COMMIT;
  return 0;
}

HF3FS_SRD_FN ServerReadRoute server_read_route(const hf3fs_crc_server_read_job& j, const hf3fs_crc_server_read_req& r,
                                               uint8_t type, uint32_t max_len) {
  ServerReadRoute o{false, false, 0, 0};
  if (j.status != 0) return o.status = j.status, o;
  const uint8_t T = r.checksum_type, S = server_read_stored_type(j);
  if ((T != HF3FS_CHECKSUM_NONE && T != type) || (S != HF3FS_CHECKSUM_NONE && S != type))
    return o.status = HF3FS_CRC_INVALID_ARG, o;
  if (j.res < 0) return o.live = true, o;                             // AioStatus.cc:40-53
  o.len = server_read_clip(j);
  if (o.len > max_len) return o.len = 0, o.status = HF3FS_CRC_INVALID_ARG, o;
  const bool full = server_read_full(j, o.len);
  const bool create = T != HF3FS_CHECKSUM_NONE && !(T == S && full);                               // :28-35
  const bool recalc = r.recalculate && full && S != HF3FS_CHECKSUM_NONE && server_read_finish_check(j) == 0;  // :43-44
  o.hashes = (create || recalc) && o.len > 0;
  const bool packs = r.xmit == HF3FS_SERVER_READ_XMIT_INLINE && o.len > 0;
  if ((o.hashes || packs) && j.localbuf == 0) return o.hashes = false, o.len = 0, o.status = HF3FS_CRC_INVALID_ARG, o;
  o.live = true;
  return o;
}

// What the settle makes of one job, besides its record.
struct ServerReadDone {
  uint8_t ok;         // result_status == 0
  uint8_t packs;      // its bytes go to the inline arena
  uint8_t listed;     // it is an entry of the RDMA list
  uint8_t wr_failed;  // RDMAReqBatch::add refused it
  uint8_t hashed;
};
enum : uint8_t { kSrdOk = 1, kSrdPacks = 2, kSrdListed = 4, kSrdWrFailed = 8 };

// Rungs 1-4 and 6's checks: result_len, result_status, checksum, checksum_type of j.  hashed:
// the range kernels' value, read only when the route hashes.  inline_off is the scan's.
HF3FS_SRD_FN ServerReadDone server_read_settle(hf3fs_crc_server_read_job& j, const hf3fs_crc_server_read_req& r,
                                               const ServerReadRoute& o, uint32_t hashed) {
  ServerReadDone d{0, 0, 0, 0, (uint8_t)(o.hashes ? 1 : 0)};
  j.result_len = 0;
  j.checksum = 0;
  j.checksum_type = HF3FS_CHECKSUM_NONE;
  j.inline_off = 0;
  if (!o.live) return j.result_status = o.status, d;
  if (j.res < 0) return j.result_status = HF3FS_CRC_CHUNK_READ_FAILED, d;  // AioStatus.cc:52
  const uint32_t L = o.len;
  const uint8_t T = r.checksum_type, S = server_read_stored_type(j);
  const bool full = server_read_full(j, L);
  const uint32_t raw = L ? hashed : kServerReadRawEmpty;
  if (T == HF3FS_CHECKSUM_NONE) {                                     // BatchReadJob.cc:28-29
  } else if (T == S && full) {                                        // :30-31
    j.checksum_type = S;
    j.checksum = server_read_stored_value(j);
  } else {                                                            // :32-35
    j.checksum_type = T;
    j.checksum = raw;
  }
  int32_t status = server_read_finish_check(j);                       // :38-41
  if (status == 0 && r.recalculate && full) {                         // :43-54
    const uint32_t real = S == HF3FS_CHECKSUM_NONE ? 0u : raw;        // ChecksumInfo::create(NONE, ..) is {NONE, 0}
    if (real != server_read_stored_value(j)) status = HF3FS_CRC_CHECKSUM_MISMATCH;
  }
  if (status == 0 && r.xmit == HF3FS_SERVER_READ_XMIT_RDMA) {         // BatchReadJob.cc:78-85
    if (j.localbuf == 0 || !j.has_rkey || L > j.rdmabuf_size || L > r.max_msg_sz) {  // IBSocket.cc:261-262
      status = HF3FS_CRC_INVALID_ARG;
      d.wr_failed = 1;
    } else {
      d.listed = 1;
    }
  }
  j.result_status = status;
  if (status != 0) return d;
  j.result_len = L;
  d.ok = 1;
  d.packs = r.xmit == HF3FS_SERVER_READ_XMIT_INLINE ? 1 : 0;          // :99-110
  return d;
}
HF3FS_SRD_FN uint8_t server_read_done_bits(const ServerReadDone& d) {
  return (uint8_t)((d.ok ? kSrdOk : 0) | (d.packs ? kSrdPacks : 0) | (d.listed ? kSrdListed : 0) |
                   (d.wr_failed ? kSrdWrFailed : 0));
}

// The RDMA list's entry of a listed job (BatchReadJob.cc:80-81, IBSocket.cc:259-273).
HF3FS_SRD_FN hf3fs_crc_server_read_wr server_read_wr_of(const hf3fs_crc_server_read_job& j, uint32_t job,
                                                        uint32_t req) {
  return hf3fs_crc_server_read_wr{j.remote_addr, j.localbuf + j.head_len, j.result_len, j.rkey, job, req};
}

// Request r's jobs among n, from offsets that may hold anything: [lo, hi) within [0, n].
HF3FS_SRD_FN void server_read_jobs_of(const uint64_t* req_off, uint64_t r, uint64_t n, uint64_t* lo, uint64_t* hi) {
  const uint64_t a = req_off[r], b = req_off[r + 1];
  *lo = a < n ? a : n;
  *hi = b < *lo ? *lo : (b < n ? b : n);
}
// The request that owns job i: the last r of [0, n_reqs) with req_off[r] <= i (n_reqs > 0).
HF3FS_SRD_FN uint64_t server_read_req_of(const uint64_t* req_off, uint64_t n_reqs, uint64_t i) {
  uint64_t lo = 0, hi = n_reqs;  // req_off[lo] <= i (or lo == 0), req_off[hi] > i (or hi == n_reqs)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (req_off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace hf3fs_crc
