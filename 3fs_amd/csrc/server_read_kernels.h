// server_read_kernels.h -- hf3fs_crc_server_read_prepare / _complete on the device (see
// server_read_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

namespace hf3fs_crc {

constexpr uint32_t kServerReadBlocksMax = 2048;  // workgroups of complete's finish: one contiguous share each

// Complete's scratch behind the record jobs' own.
struct ServerReadScratch {
  uint64_t* bytes;    // [kServerReadBlocksMax] inline bytes per share, then their exclusive scan
  uint64_t* pre;      // [n + 1] inline bytes before job i, [n]: all of them
  uint32_t* count;    // [kServerReadBlocksMax] listed jobs per share, then their exclusive scan
  uint32_t* wr_pre;   // [n + 1] listed jobs before job i, [n]: all of them
  uint32_t* req;      // [n] the request that owns job i
  uint8_t* done;      // [n] server_read_plan.h's kSrd* bits of job i
};
size_t server_read_scratch_bytes(uint64_t n);
void server_read_scratch_carve(void* base, uint64_t n, ServerReadScratch* s);

// Prepare: one lane per request; d_info is zeroed before (the kernel adds into it).
hipError_t launch_server_read_prepare(hf3fs_crc_server_read_job* jobs, uint64_t n, hf3fs_crc_server_read_req* reqs,
                                      const uint64_t* req_off, uint64_t n_reqs, uint32_t small_buf, uint32_t big_buf,
                                      uint32_t* info, hipStream_t st);

// The (addr, len) jobs of the reads that are hashed, len 0 for the others, the longest in maxl[0];
// s.req for every job.
hipError_t launch_server_read_prep(const hf3fs_crc_server_read_job* jobs, uint64_t n,
                                   const hf3fs_crc_server_read_req* reqs, const uint64_t* req_off, uint64_t n_reqs,
                                   uint8_t type, uint32_t max_len, uint64_t* addr, uint64_t* len, uint32_t* maxl,
                                   const ServerReadScratch& s, hipStream_t st);

// Complete's job outputs, d_info (zeroed before), the offsets and d_wr: settle -> scan -> place.
// v: the prep's hashed values.
hipError_t launch_server_read_finish(hf3fs_crc_server_read_job* jobs, uint64_t n,
                                     const hf3fs_crc_server_read_req* reqs, uint8_t type, uint32_t max_len,
                                     const uint32_t* v, uint64_t inline_cap, hf3fs_crc_server_read_wr* wr,
                                     uint64_t wr_cap, uint32_t* info, const ServerReadScratch& s, hipStream_t st);

// Complete's request outputs, one lane per request.  s: null scratch arrays when n == 0.
hipError_t launch_server_read_requests(const hf3fs_crc_server_read_job* jobs, uint64_t n,
                                       hf3fs_crc_server_read_req* reqs, const uint64_t* req_off, uint64_t n_reqs,
                                       const ServerReadScratch& s, hipStream_t st);

// The inline pack, a launch of its own: the bytes of the jobs that pack, unless info says overflow.
hipError_t launch_server_read_pack(const hf3fs_crc_server_read_job* jobs, uint64_t n, void* d_inline,
                                   uint64_t inline_cap, const uint32_t* info, const ServerReadScratch& s,
                                   hipStream_t st);

}  // namespace hf3fs_crc
