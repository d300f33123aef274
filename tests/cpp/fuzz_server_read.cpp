// fuzz_server_read.cpp -- stand-alone (own main, no GPU, no Python): random requests through the
// decisions of hf3fs_crc_server_read_prepare / _complete (3fs_amd/csrc/server_read_plan.h, the header
// the kernels include) and through a restatement of the reference's control flow, written as the
// reference's functions with their own local structures (StorageOperator::batchRead,
// src/storage/service/StorageOperator.cc:98-226; AioReadJob and BatchReadJob,
// src/storage/aio/BatchReadJob.cc:16-113; setReadJobResult, src/storage/aio/AioStatus.cc:27-55;
// BufferPool::Buffer, src/storage/service/BufferPool.cc:102-141; aioPrepareRead / aioFinishRead,
// src/storage/store/ChunkReplica.cc:38-100, ChunkEngine.h:34-73, StorageTarget.cc:289-304;
// RDMAReqBatch::add, src/common/net/ib/IBSocket.cc:258-275).  Both start from the same records with
// poisoned outputs; afterwards the records must be equal byte for byte, after prepare and again
// after complete, the inline layout and the RDMA list must be equal, and no input field may have
// changed but an engine job's commit_ver.  Built by tests/test_server_read_sanitized.py with
// -fsanitize=address,undefined.
//
// Bytes are not hashed here: "memory" is a function of (address, length, type), the same for both
// sides, so that a stored checksum can be made right or wrong at will.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../3fs_amd/csrc/server_read_plan.h"

namespace {

using Job = hf3fs_crc_server_read_job;
using Req = hf3fs_crc_server_read_req;
using Wr = hf3fs_crc_server_read_wr;
constexpr uint8_t kNone = 0, kCrc32c = 1, kCrc32 = 2;
constexpr uint32_t kMaxLen = 8192, kSmall = 8192, kBig = 65536;

std::map<std::string, uint64_t> g_branches;
void took(const char* name) { ++g_branches[name]; }

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }
bool chance(uint32_t percent) { return below(100) < percent; }

// What hashing [addr, addr + len) in `type` gives (len > 0, type != NONE).
uint32_t memory_hash(uint64_t addr, uint32_t len, uint8_t type) {
  uint64_t z = addr * 0xD6E8FEB86659FD93ull ^ ((uint64_t)len << 8) ^ type;
  z = (z ^ (z >> 32)) * 0xD6E8FEB86659FD93ull;
  return (uint32_t)(z ^ (z >> 32));
}

// ---- the reference, restated ----------------------------------------------------------------------
struct ChecksumInfo {
  uint8_t type = kNone;
  uint32_t value = 0;
  bool operator==(const ChecksumInfo& o) const { return type == o.type && value == o.value; }
  bool operator!=(const ChecksumInfo& o) const { return !(*this == o); }
  static ChecksumInfo create(uint8_t type, uint64_t addr, uint32_t len) {  // Common.h:150
    if (type == kNone) return {kNone, 0};
    return {type, len ? memory_hash(addr, len, type) : ~0u};
  }
};
struct Result {  // Result<uint32_t>
  int32_t error = 0;
  uint32_t value = 0;
  explicit operator bool() const { return error == 0; }
};
struct IOResult {
  Result lengthInfo{7003, 0};
  uint32_t commitVer = 0, updateVer = 0, commitChainVer = 0;
  ChecksumInfo checksum;
};
struct RDMABuf {  // a range of a buffer of the pool: which, its kind, where
  uint32_t index = 0, off = 0, size = 0;
  uint8_t kind = 0;
};
struct State {  // AioReadJob::State
  uint32_t headLength = 0, tailLength = 0, chunkLen = 0, readLength = 0;
  uint64_t readOffset = 0;
  bool readUncommitted = false, engineChunk = false;
  ChecksumInfo chunkChecksum;
  RDMABuf localbuf;
};
struct AioReadJob {
  const Job* readIO;  // the record's ReadIO and metadata fields
  IOResult result;
  State state;
  bool enqueued = false;
  uint32_t alignedLength() const { return readIO->length + state.headLength + state.tailLength; }
  uint32_t alignedOffset() const { return readIO->offset - state.headLength; }
};

struct Buffer {  // BufferPool::Buffer
  std::vector<uint8_t> indices_;
  uint32_t current_size = 0, current_cap = 0;
  bool allocate(uint32_t size, RDMABuf* out) {  // tryAllocate (:102-119) then allocate (:121-141)
    if (indices_.empty() || current_size < size) {
      if (size > kBig) return took("p_carve_2019"), false;
      if (size > kSmall) {
        took("p_carve_new_big");
        indices_.push_back(HF3FS_SERVER_READ_BUF_BIG);
        current_size = current_cap = kBig;
      } else {
        took(indices_.empty() ? "p_carve_first_small" : "p_carve_new_small");
        indices_.push_back(HF3FS_SERVER_READ_BUF_SMALL);
        current_size = current_cap = kSmall;
      }
    } else {
      took(indices_.back() == HF3FS_SERVER_READ_BUF_BIG ? (size <= kSmall ? "p_carve_small_from_big" : "p_carve_big_from_big")
                                                        : "p_carve_fits");
    }
    *out = RDMABuf{(uint32_t)indices_.size() - 1, current_cap - current_size, size, indices_.back()};  // takeFirst
    current_size -= size;
    return true;
  }
};

int32_t aioPrepareRead(AioReadJob& job) {  // StorageTarget.cc:289-297
  const Job& io = *job.readIO;
  if (io.meta_status != 0) return took(io.engine ? "p_meta_error_engine" : "p_meta_error_replica"), io.meta_status;
  if (io.engine) {  // ChunkEngine.h:59-70
    took("p_engine");
    job.state.engineChunk = true;
    job.result.commitVer = job.result.updateVer = io.update_ver;
    job.result.commitChainVer = io.chain_ver;
    job.state.chunkLen = io.chunk_len;
    job.state.chunkChecksum = ChecksumInfo{kCrc32c, ~io.chunk_checksum};
  } else {  // ChunkReplica.cc:55-72
    job.result.commitVer = io.commit_ver;
    job.result.updateVer = io.update_ver;
    job.result.commitChainVer = io.chain_ver;
    job.state.chunkLen = io.chunk_len;
    job.state.chunkChecksum = ChecksumInfo{io.chunk_checksum_type, io.chunk_checksum};
    if (job.result.commitVer != job.result.updateVer && !job.state.readUncommitted)
      return took("p_replica_4004"), HF3FS_CRC_CHUNK_NOT_COMMIT;
    took(job.result.commitVer != job.result.updateVer ? "p_replica_uncommitted_allowed" : "p_replica_ok");
  }
  job.state.readLength = job.alignedLength();
  job.state.readOffset = io.inner_offset + job.alignedOffset();
  return 0;
}

// batchRead up to the enqueue, and aioPrepareRead as the AIO workers run it.  Returns the request's code.
int32_t batchReadPrepare(std::vector<AioReadJob>& batch, const Req& req, uint32_t* failed, Buffer& buffer,
                         uint64_t totals[3]) {
  if (batch.empty()) took("p_empty_request");
  for (auto& job : batch) {  // AioReadJob::AioReadJob, BatchReadJob.cc:20-21
    job.state.headLength = job.readIO->offset % 4096;
    job.state.tailLength = (4096 - (uint32_t)(job.readIO->offset + job.readIO->length) % 4096) % 4096;
    if ((uint64_t)job.readIO->offset + job.readIO->length > 0xFFFFFFFFull) took("p_offset_plus_length_wraps");
  }
  size_t totalLength = 0, totalHeadLength = 0, totalTailLength = 0;
  for (size_t k = 0; k < batch.size(); ++k) {  // StorageOperator.cc:101-130
    auto& it = batch[k];
    *failed = (uint32_t)k;
    if (it.readIO->target_status != 0) return took("p_target_error"), it.readIO->target_status;
    if (!it.readIO->up_to_date) return took("p_not_up_to_date"), HF3FS_CRC_TARGET_STATE_INVALID;
    totalLength += it.readIO->length;
    totalHeadLength += it.state.headLength;
    totalTailLength += it.state.tailLength;
    if (it.readIO->length > it.readIO->rdmabuf_size) return took("p_bad_buffer_size"), HF3FS_CRC_INVALID_ARG;
    it.state.readUncommitted = req.read_uncommitted != 0;
  }
  for (size_t k = 0; k < batch.size(); ++k) {  // :141-154
    *failed = (uint32_t)k;
    if (!buffer.allocate(batch[k].alignedLength(), &batch[k].state.localbuf)) return HF3FS_CRC_RDMA_NO_BUF;
  }
  totals[0] = totalLength, totals[1] = totalHeadLength, totals[2] = totalTailLength;
  for (auto& job : batch) {  // :163-168 and the worker
    const int32_t rc = aioPrepareRead(job);
    if (rc) job.result.lengthInfo = Result{rc, 0};
    else job.enqueued = true;
  }
  return 0;
}

// The reference's side of prepare, written into a copy of the records.
void reference_prepare(std::vector<Job>& jobs, Req& req, uint64_t lo, uint64_t hi) {
  std::vector<Job> inputs(jobs.begin() + lo, jobs.begin() + hi);
  std::vector<AioReadJob> batch(hi - lo);
  for (uint64_t i = lo; i < hi; ++i) batch[i - lo].readIO = &inputs[i - lo];
  Buffer buffer;
  uint32_t failed = 0;
  uint64_t totals[3] = {0, 0, 0};
  const int32_t code = batchReadPrepare(batch, req, &failed, buffer, totals);
  req.status = code;
  req.failed_job = code ? (uint32_t)(lo + failed) : HF3FS_SERVER_READ_NONE;
  req.total_len = code ? 0 : totals[0];
  req.total_head = code ? 0 : totals[1];
  req.total_tail = code ? 0 : totals[2];
  req.n_small = req.n_big = 0;
  if (!code)
    for (uint8_t kind : buffer.indices_) (kind == HF3FS_SERVER_READ_BUF_BIG ? req.n_big : req.n_small)++;
  for (uint64_t i = lo; i < hi; ++i) {
    const AioReadJob& a = batch[i - lo];
    Job& j = jobs[i];
    j.head_len = a.state.headLength;
    j.tail_len = a.state.tailLength;
    if (code) {
      j.read_len = j.buf_ordinal = j.buf_off = 0;
      j.read_offset = 0;
      j.buf_kind = HF3FS_SERVER_READ_BUF_NONE;
      j.status = code;
      continue;
    }
    j.read_len = a.alignedLength();
    j.buf_ordinal = a.state.localbuf.index;
    j.buf_off = a.state.localbuf.off;
    j.buf_kind = a.state.localbuf.kind;
    j.status = a.enqueued ? 0 : a.result.lengthInfo.error;
    j.read_offset = a.enqueued ? a.state.readOffset : 0;
    if (a.state.engineChunk) j.commit_ver = a.result.commitVer;
  }
}

// AioReadJob::setResult (BatchReadJob.cc:24-63) on one record after prepare; localbuf is the record's.
struct Completed {
  Result lengthInfo;
  ChecksumInfo checksum;
};
Completed setResult(const Job& io, const Req& req, Result lengthInfo) {
  Completed out;
  const ChecksumInfo chunkChecksum = io.engine ? ChecksumInfo{kCrc32c, ~io.chunk_checksum}
                                               : ChecksumInfo{io.chunk_checksum_type, io.chunk_checksum};
  if (lengthInfo) {
    const uint8_t checksumType = req.checksum_type;
    if (checksumType == kNone) {
      took("c_rung1_none");
      out.checksum = {kNone, 0};
    } else if (checksumType == chunkChecksum.type && io.offset == 0 && lengthInfo.value == io.chunk_len) {
      took(io.engine ? "c_rung1_reuse_engine" : "c_rung1_reuse");
      out.checksum = chunkChecksum;
    } else {
      took(lengthInfo.value ? "c_rung1_create" : "c_rung1_create_empty");
      out.checksum = ChecksumInfo::create(checksumType, io.localbuf + io.head_len, lengthInfo.value);
    }
    const uint32_t length = lengthInfo.value;
    bool finish_failed = false;
    if (io.engine) {  // StorageTarget.cc:300-302
      took("c_finish_engine");
    } else if (io.meta_status_now != 0) {  // ChunkReplica.cc:85-88
      took("c_finish_meta_error");
      lengthInfo = Result{io.meta_status_now, 0};
      finish_failed = true;
    } else if (io.update_ver != io.update_ver_now) {  // :93-98
      took("c_finish_4004");
      lengthInfo = Result{HF3FS_CRC_CHUNK_NOT_COMMIT, 0};
      finish_failed = true;
    } else {
      took("c_finish_ok");
    }
    // :43 reads *lengthInfo even after the error above; the call skips the rung then
    if (finish_failed) {
      if (req.recalculate && io.offset == 0 && length == io.chunk_len) took("c_recalc_skipped_after_finish_error");
    } else if (req.recalculate && io.offset == 0 && length == io.chunk_len) {
      const ChecksumInfo realChecksum = ChecksumInfo::create(chunkChecksum.type, io.localbuf, length);
      if (realChecksum != chunkChecksum) {
        took(chunkChecksum.type == kNone ? "c_recalc_none_4080" : "c_recalc_4080");
        lengthInfo = Result{HF3FS_CRC_CHECKSUM_MISMATCH, 0};
      } else {
        took(chunkChecksum.type == kNone ? "c_recalc_none_ok" : "c_recalc_ok");
      }
    }
  }
  out.lengthInfo = lengthInfo;
  return out;
}

// setReadJobResult (AioStatus.cc:27-55), with the call's own limits in front.
Completed setReadJobResult(const Job& io, const Req& req, uint8_t call_type) {
  if (io.status != 0) return took("c_failed_in_prepare"), Completed{Result{io.status, 0}, {}};
  const uint8_t stored = io.engine ? kCrc32c : io.chunk_checksum_type;
  if ((req.checksum_type != kNone && req.checksum_type != call_type) || (stored != kNone && stored != call_type))
    return took("c_limit_type"), Completed{Result{HF3FS_CRC_INVALID_ARG, 0}, {}};
  const int64_t res = io.res;
  if (res >= 0) {
    const int64_t a = std::max<int64_t>(0l, res - io.head_len), b = int64_t(io.length),
                  c = std::max<int64_t>(0l, int64_t(io.chunk_len) - io.offset);
    const int64_t length = std::min(std::min(a, b), c);
    took(length == 0 ? "c_clip_zero" : length == c && c < b ? "c_clip_chunk_len" : length == a && a < b ? "c_clip_res" : "c_clip_length");
    if (a < 0 || res < io.head_len) took("c_res_below_head");
    if (length > kMaxLen) return took("c_limit_length"), Completed{Result{HF3FS_CRC_INVALID_ARG, 0}, {}};
    // the call's limit: bytes it would have to load behind a null localbuf
    const bool full = io.offset == 0 && (uint32_t)length == io.chunk_len;
    const bool finish_ok = io.engine || (io.meta_status_now == 0 && io.update_ver == io.update_ver_now);
    const bool loads = (req.checksum_type != kNone && !(req.checksum_type == stored && full)) ||
                       (finish_ok && req.recalculate && full && stored != kNone) ||
                       req.xmit == HF3FS_SERVER_READ_XMIT_INLINE;
    if (io.localbuf == 0 && length > 0 && loads) return took("c_limit_null"), Completed{Result{HF3FS_CRC_INVALID_ARG, 0}, {}};
    return setResult(io, req, Result{0, (uint32_t)length});
  }
  took("c_4010");
  return setResult(io, req, Result{HF3FS_CRC_CHUNK_READ_FAILED, 0});
}

struct Transmission {
  uint64_t inline_bytes = 0;
  std::vector<Wr> wr;
};

// The reference's side of complete for one request, written into a copy of the records.
void reference_complete(std::vector<Job>& jobs, Req& req, uint32_t r, uint64_t lo, uint64_t hi, uint8_t call_type,
                        Transmission& t) {
  std::vector<Completed> done(hi - lo);
  for (uint64_t i = lo; i < hi; ++i) done[i - lo] = setReadJobResult(jobs[i], req, call_type);
  req.inline_off = t.inline_bytes;
  req.wr_first = (uint32_t)t.wr.size();
  req.wr_fails = 0;
  req.wr_bytes = 0;
  for (uint64_t i = lo; i < hi; ++i) jobs[i].inline_off = 0;
  if (req.xmit == HF3FS_SERVER_READ_XMIT_INLINE) {  // copyToRespBuffer, BatchReadJob.cc:96-113
    for (uint64_t i = lo; i < hi; ++i)
      if (done[i - lo].lengthInfo) {
        took(done[i - lo].lengthInfo.value ? "x_inline" : "x_inline_empty");
        jobs[i].inline_off = t.inline_bytes;
        t.inline_bytes += done[i - lo].lengthInfo.value;
      }
  } else if (req.xmit == HF3FS_SERVER_READ_XMIT_RDMA) {  // addBufferToBatch, :74-94
    for (uint64_t i = lo; i < hi; ++i)
      if (done[i - lo].lengthInfo) {
        const Job& io = jobs[i];
        const uint32_t length = done[i - lo].lengthInfo.value;
        // RDMAReqBatch::add, IBSocket.cc:258-275
        if (io.localbuf == 0 || !io.has_rkey || length > io.rdmabuf_size || length > req.max_msg_sz) {
          took(io.localbuf == 0 ? "x_rdma_null" : !io.has_rkey ? "x_rdma_no_rkey"
               : length > io.rdmabuf_size ? "x_rdma_buf_size_unreachable" : "x_rdma_max_msg_sz");
          done[i - lo].lengthInfo = Result{HF3FS_CRC_INVALID_ARG, 0};
          req.wr_fails++;
        } else {
          took(length ? "x_rdma_listed" : "x_rdma_listed_empty");
          t.wr.push_back(Wr{io.remote_addr, io.localbuf + io.head_len, length, io.rkey, (uint32_t)i, r});
          req.wr_bytes += length;
        }
      }
  } else {
    took("x_none");
  }
  req.inline_bytes = t.inline_bytes - req.inline_off;
  req.wr_count = (uint32_t)t.wr.size() - req.wr_first;
  req.n_ok = 0;
  for (uint64_t i = lo; i < hi; ++i) {
    Job& j = jobs[i];
    const Completed& c = done[i - lo];
    j.result_status = c.lengthInfo.error;
    j.result_len = c.lengthInfo ? c.lengthInfo.value : 0;
    j.checksum = c.checksum.value;
    j.checksum_type = c.checksum.type;
    if (!c.lengthInfo) j.inline_off = 0;
    req.n_ok += c.lengthInfo ? 1 : 0;
  }
}

// ---- the plan's side --------------------------------------------------------------------------------
void plan_prepare(std::vector<Job>& jobs, Req& req, uint64_t lo, uint64_t hi) {
  using namespace hf3fs_crc;
  server_read_prepare_request(
      req, lo, hi, kSmall, kBig, [&](uint64_t i) { return jobs[i]; },
      [&](uint64_t i, const Job& j) {  // what the kernel stores
        Job& o = jobs[i];
        o.read_offset = j.read_offset;
        if (j.engine) o.commit_ver = j.commit_ver;
        o.head_len = j.head_len, o.tail_len = j.tail_len, o.read_len = j.read_len;
        o.buf_ordinal = j.buf_ordinal, o.buf_off = j.buf_off, o.status = j.status, o.buf_kind = j.buf_kind;
      });
}

void plan_complete(std::vector<Job>& jobs, Req& req, uint32_t r, uint64_t lo, uint64_t hi, uint8_t call_type,
                   Transmission& t) {
  using namespace hf3fs_crc;
  req.inline_off = t.inline_bytes;
  req.wr_first = (uint32_t)t.wr.size();
  req.n_ok = req.wr_fails = 0;
  req.wr_bytes = 0;
  for (uint64_t i = lo; i < hi; ++i) {
    Job j = jobs[i];
    const ServerReadRoute o = server_read_route(j, req, call_type, kMaxLen);
    const uint32_t hashed = o.hashes ? memory_hash(j.localbuf + j.head_len, o.len, call_type) : 0xDEADBEEFu;
    const uint8_t bits = server_read_done_bits(server_read_settle(j, req, o, hashed));
    Job& out = jobs[i];  // what the kernels store
    out.result_len = j.result_len, out.result_status = j.result_status;
    out.checksum = j.checksum, out.checksum_type = j.checksum_type;
    out.inline_off = bits & kSrdPacks ? t.inline_bytes : 0;  // the scan
    if (bits & kSrdPacks) t.inline_bytes += j.result_len;
    if (bits & kSrdListed) t.wr.push_back(server_read_wr_of(out, (uint32_t)i, r)), req.wr_bytes += j.result_len;
    req.n_ok += bits & kSrdOk ? 1 : 0;
    req.wr_fails += bits & kSrdWrFailed ? 1 : 0;
  }
  req.inline_bytes = t.inline_bytes - req.inline_off;
  req.wr_count = (uint32_t)t.wr.size() - req.wr_first;
}

// ---- the generator ------------------------------------------------------------------------------------
const uint32_t kLengths[] = {0, 1, 15, 16, 17, 100, 1000, 4095, 4096, 4097, 8192, 9000};

Job random_job(uint8_t call_type) {
  Job j;
  memset(&j, 0xA5, sizeof j);
  memset(j.reserved, 0, sizeof j.reserved);
  j.remote_addr = rnd() >> 16;
  j.inner_offset = (rnd() >> 24) * 4096;
  j.localbuf = chance(3) ? 0 : 0x7f0000000000ull + (rnd() & 0xFFFFFFF0ull) + (chance(50) ? below(16) : 0);
  j.offset = chance(45) ? 0 : chance(2) ? 0xFFFFFFFFu - below(5000) : below(20000);
  j.length = kLengths[below(chance(10) ? 12 : 10)];
  if (chance(1)) j.length = 70000 + below(5000);  // above the big buffer
  const uint32_t head = j.offset % 4096;
  j.rdmabuf_size = chance(30) ? j.length : chance(2) ? j.length / 2 : 1u << 30;
  j.rkey = (uint32_t)rnd();
  j.has_rkey = !chance(4);
  j.target_status = chance(1) ? HF3FS_CRC_CHAIN_VERSION_MISMATCH : 0;
  j.up_to_date = !chance(1);
  j.engine = chance(30);
  j.meta_status = chance(3) ? (chance(50) ? 4001 : 4002) : 0;
  j.update_ver = 1 + below(3);
  j.commit_ver = chance(12) ? j.update_ver + 1 : j.update_ver;
  j.chain_ver = below(5);
  j.update_ver_now = chance(6) ? j.update_ver + 1 : j.update_ver;
  j.meta_status_now = chance(4) ? 4001 : 0;
  const uint64_t end = (uint64_t)j.offset + j.length;
  switch (below(4)) {
    case 0: j.chunk_len = (uint32_t)std::min<uint64_t>(end, 0xFFFFFFFFull); break;
    case 1: j.chunk_len = (uint32_t)std::min<uint64_t>(end + 1 + below(5000), 0xFFFFFFFFull); break;
    case 2: j.chunk_len = (uint32_t)(end > 600 ? std::min<uint64_t>(end - 1 - below(600), 0xFFFFFFFFull) : 0); break;
    default: j.chunk_len = j.offset > 2 ? j.offset - below(3) : 0; break;
  }
  const uint32_t full_res = head + j.length + (4096 - (uint32_t)(j.offset + j.length) % 4096) % 4096;
  switch (below(10)) {
    case 0: j.res = -(int64_t)(1 + below(100)); break;
    case 1: j.res = head / 2; break;
    case 2: j.res = (int64_t)head + j.length / 2; break;
    case 3: j.res = (int64_t)full_res + 4096; break;
    default: j.res = full_res; break;
  }
  const uint8_t other = call_type == kCrc32c ? kCrc32 : kCrc32c;
  j.chunk_checksum_type = chance(15) ? kNone : chance(3) ? other : call_type;
  // the stored checksum, right for a whole read or not
  int64_t clip = std::min<int64_t>(std::max<int64_t>(0, j.res - head), j.length);
  clip = std::min<int64_t>(clip, std::max<int64_t>(0, (int64_t)j.chunk_len - j.offset));
  const uint8_t stored = j.engine ? kCrc32c : j.chunk_checksum_type;
  uint32_t value = stored == kNone ? 0u : clip > 0 ? memory_hash(j.localbuf, (uint32_t)clip, stored) : ~0u;
  if (chance(20)) value ^= 1u << below(32);
  j.chunk_checksum = j.engine ? ~value : value;
  return j;
}

Req random_req(uint8_t call_type) {
  Req q;
  memset(&q, 0xA5, sizeof q);
  memset(q.reserved, 0, sizeof q.reserved);
  const uint8_t other = call_type == kCrc32c ? kCrc32 : kCrc32c;
  q.checksum_type = chance(25) ? kNone : chance(3) ? other : call_type;
  q.xmit = (uint8_t)below(3);
  q.read_uncommitted = chance(40);
  q.recalculate = chance(50);
  q.max_msg_sz = chance(20) ? 1000 : 1u << 30;
  return q;
}

bool same_inputs(const Job& a, const Job& b) {
  Job x = a, y = b;
  if (x.engine) x.commit_ver = y.commit_ver = 0;
  x.read_offset = y.read_offset = 0, x.inline_off = y.inline_off = 0;
  x.head_len = y.head_len = x.tail_len = y.tail_len = x.read_len = y.read_len = 0;
  x.buf_ordinal = y.buf_ordinal = x.buf_off = y.buf_off = 0, x.status = y.status = 0;
  x.result_len = y.result_len = 0, x.result_status = y.result_status = 0, x.checksum = y.checksum = 0;
  x.buf_kind = y.buf_kind = x.checksum_type = y.checksum_type = 0;
  return memcmp(&x, &y, sizeof x) == 0;
}

int fail(const char* what, uint64_t request, uint64_t job) {
  fprintf(stderr, "fuzz_server_read: %s (request %llu, job %llu)\n", what, (unsigned long long)request,
          (unsigned long long)job);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t n_reqs = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000;
  uint64_t n_jobs = 0, ok_jobs = 0, ok_reqs = 0;
  for (uint64_t round = 0; round < n_reqs; round += 8) {  // eight requests to a call
    const uint8_t call_type = chance(80) ? kCrc32c : kCrc32;
    std::vector<Req> reqs;
    std::vector<uint64_t> off{0};
    std::vector<Job> jobs;
    for (int r = 0; r < 8; ++r) {
      reqs.push_back(random_req(call_type));
      const uint32_t count = chance(8) ? 0 : chance(50) ? 1 + below(4) : 1 + below(24);
      for (uint32_t k = 0; k < count; ++k) jobs.push_back(random_job(call_type));
      off.push_back(jobs.size());
    }
    n_jobs += jobs.size();
    const std::vector<Job> original = jobs;
    std::vector<Job> ref = jobs, plan = jobs;
    std::vector<Req> ref_q = reqs, plan_q = reqs;
    for (int r = 0; r < 8; ++r) {
      reference_prepare(ref, ref_q[r], off[r], off[r + 1]);
      plan_prepare(plan, plan_q[r], off[r], off[r + 1]);
      uint64_t lo, hi;
      hf3fs_crc::server_read_jobs_of(off.data(), r, jobs.size(), &lo, &hi);
      if (lo != off[r] || hi != off[r + 1]) return fail("server_read_jobs_of", round + r, lo);
      for (uint64_t i = lo; i < hi; ++i)
        if (hf3fs_crc::server_read_req_of(off.data(), 8, i) != (uint64_t)r) return fail("server_read_req_of", round + r, i);
    }
    // complete's outputs are still poison on both sides: compare everything
    for (size_t i = 0; i < jobs.size(); ++i) {
      if (memcmp(&ref[i], &plan[i], sizeof(Job))) return fail("prepare: job records differ", round, i);
      if (!same_inputs(plan[i], original[i])) return fail("prepare changed an input", round, i);
    }
    for (int r = 0; r < 8; ++r)
      if (memcmp(&ref_q[r], &plan_q[r], sizeof(Req))) return fail("prepare: request records differ", round + r, 0);
    for (int pass = 0; pass < 2; ++pass) {  // twice: complete reads no field it writes
      Transmission ref_t, plan_t;
      for (int r = 0; r < 8; ++r) {
        reference_complete(ref, ref_q[r], r, off[r], off[r + 1], call_type, ref_t);
        plan_complete(plan, plan_q[r], r, off[r], off[r + 1], call_type, plan_t);
      }
      for (size_t i = 0; i < jobs.size(); ++i) {
        if (memcmp(&ref[i], &plan[i], sizeof(Job))) return fail("complete: job records differ", round, i);
        if (!same_inputs(plan[i], original[i])) return fail("complete changed an input", round, i);
      }
      for (int r = 0; r < 8; ++r)
        if (memcmp(&ref_q[r], &plan_q[r], sizeof(Req))) return fail("complete: request records differ", round + r, 0);
      if (ref_t.inline_bytes != plan_t.inline_bytes || ref_t.wr.size() != plan_t.wr.size() ||
          (ref_t.wr.size() && memcmp(ref_t.wr.data(), plan_t.wr.data(), ref_t.wr.size() * sizeof(Wr))))
        return fail("complete: the transmissions differ", round, 0);
    }
    for (const Job& j : ref) ok_jobs += j.result_status == 0;
    for (const Req& q : ref_q) ok_reqs += q.status == 0;
  }
  printf("{\"fuzz_server_read\": \"ok\", \"requests\": %llu, \"jobs\": %llu, \"ok_requests\": %llu, \"ok_jobs\": %llu, \"branches\": {",
         (unsigned long long)n_reqs, (unsigned long long)n_jobs, (unsigned long long)ok_reqs, (unsigned long long)ok_jobs);
  bool first = true;
  for (const auto& b : g_branches) {
    printf("%s\"%s\": %llu", first ? "" : ", ", b.first.c_str(), (unsigned long long)b.second);
    first = false;
  }
  printf("}}\n");
  return 0;
}
