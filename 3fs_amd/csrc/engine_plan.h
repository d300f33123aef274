// engine_plan.h -- the two decisions of the chunk engine's update path, plain C++ that both the
// device compiler and a host compiler take, on the pattern of version_plan.h: what
// Engine::update_chunk (chunk_engine/src/core/engine.rs:288-468, behind ChunkEngine::update,
// ChunkEngine.cc:15-80) and Engine::commit_chunk (engine.rs:470-507, behind ChunkEngine::commit,
// ChunkEngine.cc:82-110) make of one job given the committed chunk and the writing-list entry it
// meets.  Each is a function of (state, job) -> (status, detail, where, copy-on-write, state after
// success).  The kernels of hf3fs_crc_update_engine (engine_kernels.hip) keep no version
// arithmetic of their own, and tests/cpp/fuzz_engine_ladder.cpp runs the same functions against a
// sequential restatement under ASan + UBSan.
#pragma once
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

#ifdef __HIPCC__
#define HF3FS_ENG_FN __host__ __device__ __forceinline__
#else
#define HF3FS_ENG_FN inline
#endif

namespace hf3fs_crc {

// What one job hands to the chunk's next: the committed chunk (Engine::get, engine.rs:314) and the
// chunk's writing-list entry (:430-455; w_addr == 0: none).  Checksums are raw, as at the ABI.
struct EngState {
  uint64_t addr;  // committed allocation
  uint32_t size, checksum, chain_ver, chunk_ver;
  uint8_t ctype;  // checksum type of the IO record's committed state (CRC32C once the call committed)
  uint64_t w_addr;
  uint32_t w_len, w_checksum, w_chain_ver, w_chunk_ver;
};

// Where a job left its ladder (the values of version_plan.h's enum, by name here).
enum : uint8_t {
  kEngAdmit = 0,   // an update: through the pipeline; `next` holds if the pipeline answers OK, with
                   // w_len / w_checksum taken from its outputs (eng_written)
  kEngEarly = 1,   // a malformed record: refused before the payload verify, never hashed
  kEngLate = 2,    // refused after the payload verify's place (rungs 3-6): 4080 is decided first
  kEngCommit = 3   // a commit job: decided, `status` is its result, `next` its state if OK
};

struct EngVerdict {
  int32_t status;  // kEngAdmit: HF3FS_CRC_OK so far
  uint8_t detail;  // HF3FS_ENGINE_DETAIL_*
  uint8_t where;
  uint8_t cow;     // kEngAdmit: the job writes into dst
  EngState next;   // == the state before for every refusal
};

// engine.rs:377-380.  The capacity clause (offset + length > capacity) never holds: capacity is
// taken as max_len, which no well-formed record exceeds.  A truncate / extend reaches the engine
// with length 0 (ChunkEngine.cc:49-52).
HF3FS_ENG_FN bool eng_needs_cow(uint8_t update_type, uint8_t flags, uint32_t offset, uint32_t length, uint32_t size) {
  if (flags & HF3FS_UPDATE_FLAG_SYNCING) return true;
  return update_type == HF3FS_UPDATE_WRITE && length > 0 && offset < size;
}

// Engine::update_chunk.  record_ok: the IO record passed every kInvalidArg check of the plain call
// (derive().ok).
HF3FS_ENG_FN EngVerdict engine_update(const EngState& s, uint32_t io_ver, uint32_t job_chain_ver, uint64_t dst,
                                      uint8_t update_type, uint8_t flags, uint32_t offset, uint32_t length,
                                      bool record_ok) {
  EngVerdict v{HF3FS_CRC_OK, HF3FS_ENGINE_DETAIL_NONE, kEngEarly, 0, s};
  const bool known = update_type == HF3FS_UPDATE_WRITE || update_type == HF3FS_UPDATE_TRUNCATE ||
                     update_type == HF3FS_UPDATE_EXTEND;
  if (!record_ok || !known || !(flags & HF3FS_UPDATE_FLAG_ENGINE))
    return v.status = HF3FS_CRC_INVALID_ARG, v.detail = HF3FS_ENGINE_DETAIL_RECORD, v;
  v.where = kEngLate;  // (:297-311, the payload verify, stands here)
  if (job_chain_ver < s.chain_ver) return v.status = HF3FS_CRC_CHAIN_VERSION_MISMATCH, v;            // :340
  const bool syncing = (flags & HF3FS_UPDATE_FLAG_SYNCING) != 0;
  uint32_t new_ver;
  if (syncing) {                                                                                     // :347
    new_ver = io_ver;
  } else if (io_ver > 0) {                                                                           // :349-362
    if (io_ver <= s.chunk_ver) return v.status = HF3FS_CRC_CHUNK_COMMITTED_UPDATE, v;
    if (io_ver > s.chunk_ver + 1u) return v.status = HF3FS_CRC_CHUNK_MISSING_UPDATE, v;
    new_ver = io_ver;
  } else {                                                                                           // :364
    new_ver = s.chunk_ver + 1u;
  }
  const bool cow = eng_needs_cow(update_type, flags, offset, length, s.size);
  if (cow && dst == 0) return v.status = HF3FS_CRC_INVALID_ARG, v.detail = HF3FS_ENGINE_DETAIL_NO_DST, v;
  if (s.w_addr != 0) return v.status = HF3FS_CRC_INVALID_ARG, v.detail = HF3FS_ENGINE_DETAIL_IN_WRITING, v;  // :441
  v.where = kEngAdmit;
  v.cow = cow ? 1 : 0;
  v.next.w_addr = cow ? dst : s.addr;
  v.next.w_len = 0;       // (the pipeline's out_size and out_checksum: eng_written)
  v.next.w_checksum = 0;
  v.next.w_chain_ver = job_chain_ver;                                                                // :426
  v.next.w_chunk_ver = new_ver;                                                                      // :425
  return v;
}

// The state after an admitted job the pipeline answered OK.
HF3FS_ENG_FN EngState eng_written(EngState next, uint32_t out_size, uint32_t out_checksum) {
  next.w_len = out_size;
  next.w_checksum = out_checksum;
  return next;
}

// ChunkEngine::commit + Engine::commit_chunk: the writing version, with the job's chain version
// (ChunkEngine.cc:96), becomes the committed chunk (engine.rs:493-503).  No version ladder.
HF3FS_ENG_FN EngVerdict engine_commit(const EngState& s, uint32_t job_chain_ver) {
  EngVerdict v{HF3FS_CRC_OK, HF3FS_ENGINE_DETAIL_NONE, kEngCommit, 0, s};
  if (s.w_addr == 0) return v.status = HF3FS_CRC_INVALID_ARG, v.detail = HF3FS_ENGINE_DETAIL_NO_WRITING, v;
  v.next.addr = s.w_addr;
  v.next.size = s.w_len;
  v.next.checksum = s.w_checksum;
  v.next.ctype = HF3FS_CHECKSUM_CRC32C;
  v.next.chain_ver = job_chain_ver;
  v.next.chunk_ver = s.w_chunk_ver;
  v.next.w_addr = 0;
  v.next.w_len = v.next.w_checksum = v.next.w_chain_ver = v.next.w_chunk_ver = 0;
  return v;
}

}  // namespace hf3fs_crc
