// client_write_kernels.h -- hf3fs_crc_client_write_prepare / _complete on the device (see
// client_write_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hf3fs_crc.h"
#include "crc_kernels.h"

namespace hf3fs_crc {

// Files of at most this many IOs (the call's max_ios_per_file) take one lane each, the sequential
// loop in registers; above it one wave per file folds them.  The figure is hf3fs_crc_client_read_
// batch's (client_read_kernels.h, profiles/client_read_threshold.jsonl); it was not measured for
// this fold.  Either schedule folds any file to the same record.
constexpr uint32_t kClientWriteLaneMaxIos = 128;
constexpr uint32_t kClientWriteBlocksMax = 2048;  // workgroups of complete's settle: one contiguous share each
constexpr uint32_t kClientWriteRunsMinLen = 1u << 20;  // prepare hashes as byte runs from this max_len on

// Complete's scratch: who failed, and the shares' counts.
struct ClientWriteScratch {
  uint8_t* take;    // [n] 1: IO i's final status is not 0
  uint32_t* count;  // [kClientWriteBlocksMax] failed IOs per share, then their exclusive scan
};
size_t client_write_scratch_bytes(uint64_t n);
void client_write_scratch_carve(void* base, uint64_t n, ClientWriteScratch* s);

// The (addr, len) jobs of the payloads that are hashed (len 0 for the others; addr and len may be
// null without VERIFY), the longest in ctl[0], ctl[1] raised when an IO fails the buffer check.
hipError_t launch_client_write_prep(const hf3fs_crc_client_write_io* ios, uint64_t n, uint32_t max_len, bool verify,
                                    uint64_t* addr, uint64_t* len, uint32_t* ctl, hipStream_t st);

// Prepare's outputs, d_updates (may be null) and d_info (zeroed before: the kernel adds into it).
// v: the prep's hashed values (null without VERIFY); poison: the prep's ctl + 1.
hipError_t launch_client_write_prepare_finish(hf3fs_crc_client_write_io* ios, uint64_t n, uint8_t type,
                                              uint32_t max_len, uint32_t max_inline_bytes, bool verify,
                                              const uint32_t* v, const uint32_t* poison, hf3fs_crc_update_io* updates,
                                              uint32_t* info, hipStream_t st);

// Complete's answers (updates: FROM_UPDATES, else null), the failed list (may be null) and the IO
// words of d_info (zeroed before): settle -> scan -> scatter.
hipError_t launch_client_write_settle(hf3fs_crc_client_write_io* ios, uint64_t n, const hf3fs_crc_update_io* updates,
                                      uint32_t* failed, uint64_t failed_cap, uint32_t* info,
                                      const ClientWriteScratch& s, hipStream_t st);

// The file records and the file words of d_info, from the answers d_ios holds.  wave: one wave per file.
hipError_t launch_client_write_fold(const hf3fs_crc_client_write_io* ios, uint64_t n, const uint64_t* file_off,
                                    uint64_t n_files, bool wave, const uint32_t* expected,
                                    hf3fs_crc_client_write_file* files, uint32_t* info, const DeviceTables* tabs,
                                    hipStream_t st);

}  // namespace hf3fs_crc
