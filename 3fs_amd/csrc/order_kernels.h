// order_kernels.h -- device-side planner of hf3fs_crc_update_ordered: a batch of update IOs in
// arrival order whose IOs may share a chunk (the reference serialises them under the chunk lock,
// one UpdateWorker job per IO, each starting from the ChunkMetadata its predecessor left).
//
// The planner ranks every IO among the IOs of its chunk (rank = earlier IOs on the same chunk)
// and the call then runs the update pipeline once per rank ("round") on an array of n records in
// which every IO of another rank is a no-op record (update_type 0: derive() marks it !ok, so it
// gets no jobs, no writes and no verdict).  Within a round every active IO is on a distinct
// chunk: the pipeline's precondition.  Between rounds one kernel copies the round's outputs back
// and hands each chunk's new {size, checksumType, checksumValue} to the chunk's next IO.
//
// Everything is a kernel on the call's stream: nothing is read back, nothing is decided on the
// host from the records' contents, so a captured call re-plans at every replay.
//
// Cost: the rank kernel walks, per IO, the list of its chunk's IOs -- O(multiplicity) steps per
// IO, so ONE chunk taking all n IOs costs n^2 dependent list steps (n = 4096: 16 M).  Batches of
// that shape belong in several calls; the depth bound (max_rounds <= 64) caps what one call
// applies per chunk anyway.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

namespace hf3fs_crc {

constexpr uint32_t kOrderNone = ~0u;  // no slot / no predecessor / no successor

// Control words of one ordered call (zeroed by the clear kernel).
enum {
  kOrdChainMax = 0,    // longest chain of the batch (uncapped): d_info[0]
  kOrdNotApplied = 1,  // IOs of rank >= max_rounds: d_info[1]
  kOrdWords = 4
};

// Planner scratch of one call (device memory, carved behind the pipeline's own scratch).
struct OrderScratch {
  uint32_t* ctl;                // kOrdWords
  unsigned long long* keys;     // [table] chunk addresses, 0 = empty (open addressing, linear probing)
  uint32_t* head;               // [table] last inserted IO of the slot's chunk
  uint32_t* next;               // [n] the slot list (unordered: atomicExch order)
  uint32_t* slot;               // [n] IO i's table slot, kOrderNone for chunk == 0
  uint32_t* rank;               // [n] earlier IOs on the same chunk
  uint32_t* pred;               // [n] the latest earlier IO on the same chunk
  uint32_t* succ;               // [n] the earliest later IO on the same chunk
  hf3fs_crc_update_io* round;   // [n] the round array the pipeline runs on
  uint32_t table;               // power of two >= 2 n
};

size_t order_scratch_bytes(uint64_t n);
void order_scratch_carve(void* base, uint64_t n, OrderScratch* s);

// clear -> insert -> rank: fills slot / next / rank / pred / succ and the two control words.
hipError_t launch_order_plan(const hf3fs_crc_update_io* ios, uint64_t n, uint32_t max_rounds, const OrderScratch& s,
                             hipStream_t st);
// The step before round r (r = 0 .. max_rounds): copies round r - 1's outputs back into ios, hands
// the state they left to each chunk's next IO (in ios and in the round array) and turns every
// other record of the round array into a no-op.  r == max_rounds is the call's last launch: the
// IOs never reached get HF3FS_CRC_NOT_APPLIED and info (may be null) the two control words.
hipError_t launch_order_step(hf3fs_crc_update_io* ios, uint64_t n, uint32_t r, uint32_t max_rounds,
                             const OrderScratch& s, uint32_t* info, hipStream_t st);

}  // namespace hf3fs_crc
