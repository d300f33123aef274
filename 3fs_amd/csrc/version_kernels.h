// version_kernels.h -- the kernels hf3fs_crc_update_versioned adds to the ordered call: the step
// between rounds with the version ladders of version_plan.h in it, and the kernel that settles
// the jobs the update ladder refused once their payloads are hashed.
//
// The call runs the order planner and the update pipeline unchanged (order_kernels.h: rank / pred
// / succ, one pipeline pass per rank over an array of n records of which the others are no-ops).
// What changes is who may enter a round.  The step before round r
//   - finishes the jobs of round r - 1: a job that went through the pipeline takes its outputs
//     from the round array, and out_* of its version record fall back to the before-state when
//     the pipeline answered anything but OK;
//   - hands {size, checksum type, checksum value} and the six version fields to the chunk's next
//     job (rank r) and runs that job's ladder there and then, in the same thread;
//   - a job the ladder admits enters round r as it would in update_ordered; every other job is
//     decided on the spot and enters as a no-op record: refused at rungs 1-4, a commit (either
//     way), or refused by the version rungs (kVerLate).
// A kVerLate job may still owe 4080: the reference verifies the payload BEFORE the version rungs
// (ChunkReplica.cc:193-207 vs :211-239).  Both answers leave the chunk and its metadata as they
// were, so its successor does not wait for the verdict: the step records payload address and
// length per job (length 0 for every other job), and after the last round one pass of the range
// hasher over that list and one settle kernel choose between 4080 and the ladder's code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "order_kernels.h"

namespace hf3fs_crc {

// Control words of the versioned part: the two spare words of the ordered call's four
// (order_kernels.h), so the planner's clear kernel zeroes them before step 0 and the call needs
// no zeroing launch of its own.
enum {
  kOrdVerMaxLen = 2,  // longest payload among the kVerLate jobs that verify: the hashing pass's length bound
  kOrdVerQueue = 3    // the hashing pass's ticket counter
};
static_assert(kOrdVerMaxLen > kOrdNotApplied && kOrdVerQueue < kOrdWords, "the ordered call's spare control words");

// dec[i]: 0 = job i entered its round; else status | where << 16 | verify << 24.
constexpr uint32_t kDecWhereShift = 16, kDecVerifyBit = 1u << 24, kDecStatusMask = 0xffffu;

struct VersionScratch {
  uint32_t* dec;    // [n]
  uint64_t* vaddr;  // [n] payload of a kVerLate job that verifies, else 0
  uint64_t* vlen;   // [n] its length, else 0
  uint32_t* vout;   // [n] the hashing pass's output (zeroed by step 0)
};

size_t version_scratch_bytes(uint64_t n);
void version_scratch_carve(void* base, uint64_t n, VersionScratch* s);

// The step before round r (r = 0 .. max_rounds), launch_order_step's sibling.  r == 0 also zeroes
// info (may be null), which the settle kernel counts into.  r == max_rounds finishes the last round
// and gives the jobs never reached NOT_APPLIED with the state after their chunk's last applied job
// in both records.
hipError_t launch_version_step(hf3fs_crc_update_io* ios, hf3fs_crc_update_ver* ver, uint64_t n, uint32_t r,
                               uint32_t max_rounds, uint32_t max_len, uint8_t type, int mode, const OrderScratch& os,
                               const VersionScratch& vs, uint32_t* info, hipStream_t st);
// After the hashing pass over (vaddr, vlen) -> vout: a kVerLate job gets 4080 if its payload
// failed, else the ladder's code; then every job is counted into info[2..7] (may be null;
// step 0 zeroed it) and info[0..1] take the planner's two words.
hipError_t launch_version_settle(hf3fs_crc_update_io* ios, uint64_t n, uint32_t max_rounds, const OrderScratch& os,
                                 const VersionScratch& vs, uint32_t* info, hipStream_t st);

}  // namespace hf3fs_crc
