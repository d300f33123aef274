// forward_kernels.h -- hf3fs_crc_forward_prepare / _complete on the device (see forward_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

namespace hf3fs_crc {

constexpr uint32_t kForwardBlocksMax = 2048;  // workgroups of complete's finish: one contiguous share each

// Complete's scratch behind the record jobs' own: who commits, and the shares' counts.
struct ForwardScratch {
  uint8_t* take;    // [n] 1: job i commits
  uint32_t* count;  // [kForwardBlocksMax] COMMIT jobs per share, then their exclusive scan
};
size_t forward_scratch_bytes(uint64_t n);
void forward_scratch_carve(void* base, uint64_t n, ForwardScratch* s);

// The (addr, len) jobs of the chunks (prepare) or outgoing buffers (complete) that are hashed,
// len 0 for the others, the longest in maxl[0].
hipError_t launch_forward_prep(const hf3fs_crc_forward_job* jobs, uint64_t n, uint8_t type, uint32_t max_len,
                               bool complete, uint64_t* addr, uint64_t* len, uint32_t* maxl, hipStream_t st);

// Prepare's outputs and d_info (zeroed before: the kernel adds into it).  v: the prep's hashed values.
hipError_t launch_forward_prepare_finish(hf3fs_crc_forward_job* jobs, uint64_t n, uint8_t type, uint32_t max_len,
                                         uint32_t max_inline_bytes, const uint32_t* v, uint32_t* info, hipStream_t st);

// Complete's outputs, d_info (zeroed before) and d_commit_idx (may be null): settle -> scan -> scatter.
hipError_t launch_forward_complete_finish(hf3fs_crc_forward_job* jobs, uint64_t n, uint8_t type, uint32_t max_len,
                                          const uint32_t* v, uint32_t* commit_idx, uint32_t* info,
                                          const ForwardScratch& s, hipStream_t st);

}  // namespace hf3fs_crc
