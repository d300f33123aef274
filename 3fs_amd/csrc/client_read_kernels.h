// client_read_kernels.h -- hf3fs_crc_client_read_batch on the device (see client_read_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hf3fs_crc.h"
#include "crc_kernels.h"

namespace hf3fs_crc {

// Parents of at most this many children (the call's max_children) take one lane each, the
// sequential loop in registers; above it one wave per parent folds them.  The switch-over of the
// A/B in profiles/client_read_threshold.jsonl, record threshold_chosen (scripts/
// bench_client_read.py: 2^22 children per call, one lane per parent 0.34 ms against 0.43 ms at
// 128 children, 0.61 ms against 0.31 ms at 256; measured without VERIFY, the merge kernel alone:
// with VERIFY every child also loads its hashed value, which the A/B does not cover).  Either schedule merges any parent: a caller
// (or a test) that passes another max_children only moves the choice.
constexpr uint32_t kClientLaneMaxChildren = 128;

// The (addr, len) jobs of the children that are hashed (len 0 for the others), the longest in maxl[0].
hipError_t launch_client_read_prep(const hf3fs_crc_client_read_io* ios, uint64_t n_ios, uint8_t type, uint32_t max_len,
                                   uint64_t* addr, uint64_t* len, uint32_t* maxl, hipStream_t st);

// Verdicts, parents, block records and d_info (zeroed before: the kernel adds into it).  v: the
// hashed values of the prep's jobs, null without VERIFY.  wave: one wave per parent.
hipError_t launch_client_read_merge(hf3fs_crc_client_read_io* ios, uint64_t n_ios, const uint64_t* parent_off,
                                    uint64_t n_parents, uint8_t type, uint32_t max_len, bool verify, bool wave,
                                    const uint32_t* v, hf3fs_crc_client_read_result* parents,
                                    hf3fs_crc_block_digest* blocks, uint32_t* info, const DeviceTables* tabs,
                                    hipStream_t st);

}  // namespace hf3fs_crc
