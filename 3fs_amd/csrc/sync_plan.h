// sync_plan.h -- the decisions of hf3fs_crc_sync_plan, plain C++ that both the device compiler and
// a host compiler take: the ladder of ResyncWorker::handleSync (src/storage/sync/
// ResyncWorker.cc:203-275) as one function of (local record or none, remote record, chain_ver,
// flags) -> class, and what a class means: its disposition and the d_info word it counts in.
// The kernels of sync_kernels.hip decide nothing else about a record; tests/cpp/fuzz_sync_plan.cpp
// includes this header and compares it, with lowest-index claims, against a sequential restatement
// of the reference loop under ASan + UBSan.
#pragma once
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

#ifdef __HIPCC__
#define HF3FS_SYNC_FN __host__ __device__ __forceinline__
#else
#define HF3FS_SYNC_FN inline
#endif

namespace hf3fs_crc {

constexpr uint32_t kSyncNone = ~0u;     // no record / no peer / no fatal record
constexpr uint8_t kSyncStateCommit = 0;  // ChunkState::COMMIT

enum SyncDisposition : uint8_t { kSyncNothing = 0, kSyncForward, kSyncSkip, kSyncRemove, kSyncFatal };

// Slot of the 128-bit id in a table of mask + 1 slots: both halves enter.
HF3FS_SYNC_FN uint32_t sync_hash(uint64_t hi, uint64_t lo, uint32_t mask) {
  uint64_t x = (hi ^ (lo >> 29)) * 0x9E3779B97F4A7C15ull + lo;
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32;
  return (uint32_t)x & mask;
}

// The ladder.  local == nullptr: the remote record has no local record left (none with its id, or
// an earlier remote record with the same id erased it, :205-210).
HF3FS_SYNC_FN uint8_t sync_classify(const hf3fs_crc_sync_meta* local, const hf3fs_crc_sync_meta& remote,
                                    uint32_t chain_ver, uint32_t flags) {
  if (!local) return HF3FS_SYNC_REMOTE_ONLY;
  const hf3fs_crc_sync_meta& meta = *local;
  if (meta.recycle_state != 0) return HF3FS_SYNC_LOCAL_RECYCLING;
  if (meta.chain_ver > remote.chain_ver) return HF3FS_SYNC_CHAIN_VER_LOW;
  if (remote.update_ver != remote.commit_ver || remote.chunk_state != kSyncStateCommit)
    return HF3FS_SYNC_REMOTE_UNCOMMITTED;
  if (meta.chain_ver < remote.chain_ver)
    return meta.chunk_state == kSyncStateCommit ? HF3FS_SYNC_REMOTE_CHAIN_VER_HIGH : HF3FS_SYNC_LOCAL_UNCOMMITTED;
  if (meta.update_ver != remote.commit_ver)
    return meta.chain_ver != chain_ver && meta.chunk_state == kSyncStateCommit ? HF3FS_SYNC_COMMIT_VER_MISMATCH
                                                                              : HF3FS_SYNC_CHAIN_WRITING;
  if (flags & HF3FS_SYNC_HEAVY) return HF3FS_SYNC_FULL_SYNC_HEAVY;
  if (meta.checksum_type != remote.checksum_type || meta.checksum != remote.checksum)
    return meta.chain_ver != chain_ver ? HF3FS_SYNC_CHECKSUM_MISMATCH : HF3FS_SYNC_CHAIN_WRITING_CHECKSUM;
  return HF3FS_SYNC_EQUAL;
}

HF3FS_SYNC_FN SyncDisposition sync_disposition(uint8_t cls) {
  switch (cls) {
    case HF3FS_SYNC_REMOTE_ONLY:
      return kSyncRemove;
    case HF3FS_SYNC_CHAIN_VER_LOW:
    case HF3FS_SYNC_REMOTE_UNCOMMITTED:
    case HF3FS_SYNC_FULL_SYNC_HEAVY:
    case HF3FS_SYNC_REMOTE_MISS:
      return kSyncForward;
    case HF3FS_SYNC_REMOTE_CHAIN_VER_HIGH:
    case HF3FS_SYNC_COMMIT_VER_MISMATCH:
    case HF3FS_SYNC_CHECKSUM_MISMATCH:
      return kSyncFatal;
    case HF3FS_SYNC_LOCAL_UNCOMMITTED:
    case HF3FS_SYNC_CHAIN_WRITING:
    case HF3FS_SYNC_CHAIN_WRITING_CHECKSUM:
    case HF3FS_SYNC_EQUAL:
      return kSyncSkip;
    default:  // LOCAL_RECYCLING, MATCHED, DUPLICATE
      return kSyncNothing;
  }
}

// The d_info word a class counts in, 0 for none (REMOTE_ONLY goes to the remove list, EQUAL only
// into `skip`, MATCHED nowhere).
HF3FS_SYNC_FN uint32_t sync_counter(uint8_t cls) {
  switch (cls) {
    case HF3FS_SYNC_LOCAL_RECYCLING:
      return HF3FS_SYNC_INFO_RECYCLE;
    case HF3FS_SYNC_CHAIN_VER_LOW:
      return HF3FS_SYNC_INFO_CHAIN_VER_LOW;
    case HF3FS_SYNC_REMOTE_UNCOMMITTED:
      return HF3FS_SYNC_INFO_REMOTE_UNCOMMITTED;
    case HF3FS_SYNC_REMOTE_CHAIN_VER_HIGH:
      return HF3FS_SYNC_INFO_CHAIN_VER_HIGH;
    case HF3FS_SYNC_LOCAL_UNCOMMITTED:
      return HF3FS_SYNC_INFO_LOCAL_UNCOMMITTED;
    case HF3FS_SYNC_COMMIT_VER_MISMATCH:
      return HF3FS_SYNC_INFO_COMMIT_VER_MISMATCH;
    case HF3FS_SYNC_CHAIN_WRITING:
    case HF3FS_SYNC_CHAIN_WRITING_CHECKSUM:
      return HF3FS_SYNC_INFO_CHAIN_WRITING;
    case HF3FS_SYNC_FULL_SYNC_HEAVY:
      return HF3FS_SYNC_INFO_FULL_SYNC_HEAVY;
    case HF3FS_SYNC_CHECKSUM_MISMATCH:
      return HF3FS_SYNC_INFO_FULL_SYNC_LIGHT;
    case HF3FS_SYNC_REMOTE_MISS:
      return HF3FS_SYNC_INFO_REMOTE_MISS;
    case HF3FS_SYNC_DUPLICATE:
      return HF3FS_SYNC_INFO_DUPLICATES;
    default:
      return 0;
  }
}

// d_info from a histogram of classes (hist[c] = records of class c: remote classes over the remote
// records [0, first_fatal], local classes and `forwards` -- the MATCHED records whose peer forwards
// -- over the whole local table), with the break applied: after a fatal record the reference has
// built no list and counted no remote miss.
HF3FS_SYNC_FN void sync_info(const uint32_t* hist, uint32_t forwards, uint32_t first_fatal, uint32_t* info) {
  for (int w = 0; w < HF3FS_SYNC_INFO_WORDS; ++w) info[w] = 0;
  for (int c = 1; c < 32; ++c) {
    if (const uint32_t w = sync_counter((uint8_t)c)) info[w] += hist[c];
    if (sync_disposition((uint8_t)c) == kSyncSkip) info[HF3FS_SYNC_INFO_SKIP] += hist[c];
  }
  const bool fatal = first_fatal != kSyncNone;
  info[HF3FS_SYNC_INFO_FATAL] = fatal ? 1u : 0u;
  info[HF3FS_SYNC_INFO_FIRST_FATAL] = first_fatal;
  info[HF3FS_SYNC_INFO_N_WRITE] = fatal ? 0u : forwards + hist[HF3FS_SYNC_REMOTE_MISS];
  info[HF3FS_SYNC_INFO_N_REMOVE] = fatal ? 0u : hist[HF3FS_SYNC_REMOTE_ONLY];
  if (fatal) info[HF3FS_SYNC_INFO_REMOTE_MISS] = 0;
}

}  // namespace hf3fs_crc
