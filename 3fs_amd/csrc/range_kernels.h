// range_kernels.h -- device side of hf3fs_crc_range_query and hf3fs_crc_file_length (see
// range_kernels.hip): chunk range walks over one target's metadata table as a prefix sum over the
// table, paid once per call, and a few binary searches per op and per list entry.
//
// Everything is a kernel on the call's stream: nothing is read back, nothing is decided on the host
// from the contents of table or ops, so a captured call re-plans at every replay.  Phases are ordered
// by kernel boundaries only: no kernel waits on another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

namespace hf3fs_crc {

constexpr uint32_t kRangeBlocksMax = 2048;  // workgroups of a share pass: one contiguous share each

// Scratch of one range_query call (device memory).  Who writes what is in range_kernels.hip.
struct RangeScratch {
  uint64_t* len_pre;    // [n_meta + 1] length of the normal records before record i
  uint64_t* op_off;     // [n_ops + 1] an op's list count, then the list entries before op i
  uint64_t* share_len;  // [kRangeBlocksMax] normal length per table share, then the exclusive scan
  uint64_t* share_list; // [kRangeBlocksMax] list entries per op share, then the exclusive scan
  uint64_t* share_chunks;  // [kRangeBlocksMax] total_chunks per op share
  uint32_t* cnt_pre;    // [n_meta + 1] normal records before record i
  uint32_t* op_top;     // [n_ops] normal records below the op's span end
  uint32_t* share_cnt;  // [kRangeBlocksMax] normal records per table share, then the exclusive scan
  uint32_t* share_bad;  // [kRangeBlocksMax] order breaks per table share
  uint32_t* share_ok;   // [kRangeBlocksMax] ops with status 0 per op share
  uint32_t* ctl;        // [4] [0] order breaks of the table, [1] padding (never written or read), [2..3] list
                        // entries (64 bits as two words)
};
size_t range_scratch_bytes(uint64_t n_meta, uint64_t n_ops);
void range_scratch_carve(void* base, uint64_t n_meta, uint64_t n_ops, RangeScratch* s);

// table count -> scan -> apply -> ops -> scan -> apply -> list.
hipError_t launch_range_query(const hf3fs_crc_sync_meta* meta, uint64_t n_meta, hf3fs_crc_range_op* ops,
                              uint64_t n_ops, uint32_t* list, uint64_t list_cap, uint32_t* info,
                              const RangeScratch& s, hipStream_t st);

// One lane per file; info is zeroed before (the kernel adds into it).
hipError_t launch_file_length(const hf3fs_crc_range_op* ops, uint64_t n_ops, hf3fs_crc_file_len* files,
                              uint64_t n_files, uint32_t* info, hipStream_t st);

}  // namespace hf3fs_crc
