// md5_kernels.h -- device side of hf3fs_crc_md5_batch: the MD5 leg of the admin `checksum`
// command (src/client/cli/admin/Checksum.cc:50-83, FileWrapper.cc:172-177) for many files at once,
// one lane per file.  What a lane does with its file's bytes is md5_core.h; this is the mapping of
// files to lanes and the two ways a lane gets its 64 bytes.
//
// Everything is a kernel on the call's stream: nothing is read back and nothing is decided on the
// host from what the arrays hold, so a captured call re-plans at every replay.  Phases are ordered
// by kernel boundaries only: no kernel waits on another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

namespace hf3fs_crc {

constexpr uint64_t kMd5MaxCount = 1ull << 30;  // files or segments of one call (32-bit permutation)
constexpr uint32_t kMd5SharesMax = 256;        // waves of the bucket count / scatter passes

// Scratch of one call (device memory).  Who writes what is in md5_kernels.hip.
struct Md5Scratch {
  uint64_t* blocks;  // [n_files] 64-byte blocks the call compresses for the file
  uint32_t* perm;    // [n_files] file of lane i: files by bucket, ties by ascending file index
  uint32_t* count;   // [kMd5Buckets][shares] files per bucket and share, then their exclusive scan
  uint32_t shares;   // contiguous shares of the files, one wave each
};

size_t md5_scratch_bytes(uint64_t n_files);
void md5_scratch_carve(void* base, uint64_t n_files, Md5Scratch* s);

// prep -> (sort: count -> scan -> scatter) -> hash.  stage: 0 every lane loads its own block,
// 1 the wave stages the lanes' next pieces through LDS.
hipError_t launch_md5_batch(const hf3fs_crc_md5_seg* segs, const uint64_t* file_off, uint64_t n_files,
                            uint64_t n_segs, hf3fs_crc_md5_state* state, uint8_t* out, uint32_t flags, bool sort,
                            bool stage, const Md5Scratch& s, hipStream_t st);

}  // namespace hf3fs_crc
