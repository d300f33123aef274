// sync_kernels.h -- device side of hf3fs_crc_sync_plan: the comparison loop of
// ResyncWorker::handleSync (src/storage/sync/ResyncWorker.cc:199-303) as a hash join of the local
// and the remote table on the 128-bit chunk id plus the ladder of sync_plan.h, and of
// hf3fs_crc_sync_scrub_fill, which turns the plan's write list into scrub records.
//
// Everything is a kernel on the call's stream: nothing is read back, nothing is decided on the
// host from the tables' contents, so a captured call re-plans at every replay.  Phases are ordered
// by kernel boundaries only: no kernel waits on another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

namespace hf3fs_crc {

constexpr uint32_t kSyncBlocksMax = 2048;  // workgroups of the count / scatter passes per table
constexpr uint32_t kSyncCtlWords = 64;     // [0] first fatal index, [32 + c] records of code c
constexpr uint64_t kSyncMaxRecords = 1ull << 30;  // 32-bit indices, a table of 2 n_local slots

// Scratch of one call (device memory).  Who writes what is in sync_kernels.hip.
struct SyncScratch {
  uint32_t* ctl;     // kSyncCtlWords
  uint32_t* table;   // [slots] local index of the slot's id, kSyncNone = empty (linear probing)
  uint32_t* claim;   // [n_local] lowest remote index with the record's id, kSyncNone = none
  uint32_t* rfound;  // [n_remote] local index the remote record's id resolves to, kSyncNone = none
  uint32_t* lcount;  // [kSyncBlocksMax] write-list entries per workgroup, then their exclusive scan
  uint32_t* rcount;  // [kSyncBlocksMax] the same for the remove list
  uint8_t* lcode;    // [n_local] class of the local record (MATCHED with a forwarding peer: kSyncMatchedForward)
  uint8_t* rcode;    // [n_remote] class of the remote record
  uint32_t slots;    // power of two >= 2 n_local
};

size_t sync_scratch_bytes(uint64_t n_local, uint64_t n_remote);
void sync_scratch_carve(void* base, uint64_t n_local, uint64_t n_remote, SyncScratch* s);

// clear -> insert -> claim -> classify -> count -> scan -> scatter.
hipError_t launch_sync_plan(hf3fs_crc_sync_meta* local, uint64_t n_local, hf3fs_crc_sync_meta* remote,
                            uint64_t n_remote, uint32_t chain_ver, uint32_t flags, uint32_t* d_write,
                            uint32_t* d_remove, uint32_t* d_info, const SyncScratch& s, hipStream_t st);
hipError_t launch_sync_scrub_fill(const hf3fs_crc_sync_meta* local, const uint64_t* addrs, const uint32_t* d_write,
                                  const uint32_t* d_info, uint64_t n_local, hf3fs_crc_scrub_io* scrub, hipStream_t st);

}  // namespace hf3fs_crc
