// version_plan.h -- the two version ladders of the update path, plain C++ that both the device
// compiler and a host compiler take: what ChunkReplica::update (ChunkReplica.cc:171-191,211-245)
// and ChunkReplica::commit (:397-467) make of one job given the ChunkMetadata it meets.  Each is
// a function of (state, job) -> (status, state after success).  The kernels of
// hf3fs_crc_update_versioned (version_kernels.hip) keep no version arithmetic of their own, and
// tests/cpp/fuzz_version_ladder.cpp runs the same functions against a sequential restatement
// under ASan + UBSan.
#pragma once
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

#ifdef __HIPCC__
#define HF3FS_VER_FN __host__ __device__ __forceinline__
#else
#define HF3FS_VER_FN inline
#endif

namespace hf3fs_crc {

enum : uint8_t { kChunkCommit = 0, kChunkDirty = 1, kChunkClean = 2 };  // ChunkState (Common.h)

// ChunkMetadata's version part: the six fields one job hands to the chunk's next.
struct VerState {
  uint32_t chain_ver, update_ver, commit_ver, meta_chunk_size;
  uint8_t chunk_state, recycle_state;
};

// Where a job left its ladder.
enum : uint8_t {
  kVerAdmit = 0,    // an update: through the pipeline, `next` holds if the pipeline answers OK
  kVerEarly = 1,    // refused before the payload verify (rungs 1-4): never hashed
  kVerLate = 2,     // refused by the version ladder (rung 6): the payload verify decides 4080 first
  kVerCommit = 3    // a commit job: decided, `status` is its result, `next` its state if OK
};

struct VerVerdict {
  int32_t status;  // kVerAdmit: HF3FS_CRC_OK so far
  uint8_t where;
  VerState next;   // == the state before for every refusal
};

HF3FS_VER_FN VerState ver_before(const hf3fs_crc_update_ver& v) {
  return VerState{v.chain_ver, v.update_ver, v.commit_ver, v.meta_chunk_size, v.chunk_state, v.recycle_state};
}

// ChunkReplica::update.  record_ok: the IO record passed every kInvalidArg check of the plain call
// (derive().ok; :141-146 among them).
HF3FS_VER_FN VerVerdict update_ladder(const VerState& s, uint32_t io_ver, uint32_t job_chain_ver, uint8_t flags,
                                      bool record_ok, uint32_t max_len) {
  VerVerdict v{HF3FS_CRC_OK, kVerEarly, s};
  const bool syncing = (flags & HF3FS_UPDATE_FLAG_SYNCING) != 0;
  if (!record_ok || (flags & HF3FS_UPDATE_FLAG_ENGINE)) return v.status = HF3FS_CRC_INVALID_ARG, v;
  if (s.meta_chunk_size != max_len) return v.status = HF3FS_CRC_CHUNK_SIZE_MISMATCH, v;               // :176
  if (s.chunk_state == kChunkDirty && !syncing) return v.status = HF3FS_CRC_CHUNK_NOT_CLEAN, v;      // :181
  if (job_chain_ver < s.chain_ver && s.chunk_state == kChunkCommit)
    return v.status = HF3FS_CRC_CHAIN_VERSION_MISMATCH, v;                                           // :186
  v.where = kVerLate;  // (:193-207, the payload verify, stands here)
  if (syncing) {                                                                                     // :211-215
    v.next.update_ver = io_ver;
    v.next.commit_ver = io_ver - 1u;
    v.next.recycle_state = 0;
  } else if (io_ver > 0) {                                                                           // :216-231
    if (io_ver <= s.commit_ver) return v.status = HF3FS_CRC_CHUNK_COMMITTED_UPDATE, v;
    if (io_ver <= s.update_ver) return v.status = HF3FS_CRC_CHUNK_STALE_UPDATE, v;
    if (io_ver > s.update_ver + 1u) return v.status = HF3FS_CRC_CHUNK_MISSING_UPDATE, v;
    v.next.update_ver = io_ver;
  } else {                                                                                           // :232-239
    if (s.update_ver + 1u > s.commit_ver + 1u) return v.status = HF3FS_CRC_CHUNK_ADVANCE_UPDATE, v;
    v.next.update_ver = s.update_ver + 1u;
  }
  v.where = kVerAdmit;
  v.next.chunk_state = kChunkClean;  // DIRTY during the write (:241), CLEAN after it (:304)
  v.next.chain_ver = job_chain_ver;  // :242
  return v;
}

// ChunkReplica::commit.  A chunk in recycling would be removed by this commit (store.remove, :458):
// that stays on the host, kInvalidArg here.
HF3FS_VER_FN VerVerdict commit_ladder(const VerState& s, uint32_t io_ver, uint32_t job_chain_ver, uint8_t flags,
                                      bool is_force) {
  VerVerdict v{HF3FS_CRC_OK, kVerCommit, s};
  if ((flags & HF3FS_UPDATE_FLAG_ENGINE) || s.recycle_state != 0) return v.status = HF3FS_CRC_INVALID_ARG, v;
  if (job_chain_ver < s.chain_ver) return v.status = HF3FS_CRC_CHAIN_VERSION_MISMATCH, v;            // :419
  if (io_ver > s.update_ver) return v.status = HF3FS_CRC_CHUNK_VERSION_MISMATCH, v;                  // :425
  if (is_force) {                                                                                    // :432
    v.next.chunk_state = kChunkClean;
    v.next.commit_ver = io_ver;
  } else if (s.chunk_state == kChunkDirty) {                                                         // :435
    return v.status = HF3FS_CRC_CHUNK_NOT_CLEAN, v;
  } else if (s.commit_ver < io_ver) {                                                                // :440
    v.next.commit_ver = io_ver;
  } else {                                                                                           // :442
    return v.status = HF3FS_CRC_CHUNK_STALE_COMMIT, v;
  }
  if (v.next.commit_ver == v.next.update_ver) {                                                      // :451
    v.next.chunk_state = kChunkCommit;
    v.next.chain_ver = job_chain_ver;
  }
  return v;
}

}  // namespace hf3fs_crc
