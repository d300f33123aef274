// engine_kernels.h -- the kernels hf3fs_crc_update_engine adds to the ordered call: the step
// between rounds with the chunk engine's state machine (engine_plan.h) in it, and the kernel that
// settles the jobs refused after the payload verify's place once their payloads are hashed.
// Siblings of launch_version_step / launch_version_settle (version_kernels.h), whose scratch
// arrays, dec[] encoding and control words they share.
//
// The call runs the order planner unchanged (order_kernels.h: rank / pred / succ over the `chunk`
// keys) and one pass of the copy-on-write pipeline per rank over an array of n records of which
// the others are no-ops.  The step before round r
//   - finishes the jobs of round r - 1: a job that went through the pipeline takes its outputs
//     from the round array; when the pipeline answered OK its writing version takes out_size and
//     out_checksum, otherwise out_* of its job record fall back to the before-state;
//   - hands the committed state {size, checksum type, checksum value, addr, chain_ver, chunk_ver}
//     and the writing version to the chunk's next job (rank r) and runs that job's decision there
//     and then, in the same thread;
//   - a job the engine admits enters round r with chunk = addr, and dst (copy on write) or 0 (in
//     place) in the per-round destination array; every other job is decided on the spot and
//     enters as a no-op record with destination 0: a malformed record, a commit (either way), or
//     a refusal at the version, destination or writing-list rungs (kEngLate).
// A kEngLate job may still owe 4080: the engine verifies the payload before everything else
// (engine.rs:297-311).  Both answers leave the chunk as it was, so the successor does not wait:
// the deferred hashing pass of update_versioned settles them after the last round.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "order_kernels.h"
#include "version_kernels.h"

namespace hf3fs_crc {

struct EngineScratch {
  VersionScratch v;  // dec / vaddr / vlen / vout, as in update_versioned
  uint64_t* rdst;    // [n] the round's destinations: dst of an admitted copy-on-write job, else 0
};

size_t engine_scratch_bytes(uint64_t n);
void engine_scratch_carve(void* base, uint64_t n, EngineScratch* s);

// The step before round r (r = 0 .. max_rounds).  r == 0 also zeroes info (may be null), which
// the settle kernel counts into.  r == max_rounds finishes the last round and gives the jobs never
// reached NOT_APPLIED with the state after their chunk's last applied job in both records.
hipError_t launch_engine_step(hf3fs_crc_update_io* ios, hf3fs_crc_engine_job* jobs, uint64_t n, uint32_t r,
                              uint32_t max_rounds, uint32_t max_len, int mode, const OrderScratch& os,
                              const EngineScratch& es, uint32_t* info, hipStream_t st);
// After the hashing pass over (vaddr, vlen) -> vout: a kEngLate job gets 4080 (detail 0) if its
// payload failed, else the decision's code; then every job is counted into info[2..7] (may be
// null; step 0 zeroed it) and info[0..1] take the planner's two words.
hipError_t launch_engine_settle(hf3fs_crc_update_io* ios, hf3fs_crc_engine_job* jobs, uint64_t n,
                                uint32_t max_rounds, const OrderScratch& os, const EngineScratch& es, uint32_t* info,
                                hipStream_t st);

}  // namespace hf3fs_crc
