// forward_plan.h -- the decisions of hf3fs_crc_forward_prepare and hf3fs_crc_forward_complete,
// plain C++ that both the device compiler and a host compiler take, on the pattern of
// engine_plan.h and client_read_plan.h: what StorageOperator::handleUpdate
// (src/storage/service/StorageOperator.cc:401-485) and ReliableForwarding::forward / doForward
// (src/storage/service/ReliableForwarding.cc:113-134,145-278) make of one update between the local
// update and the commit.  Hashing is not done here: a caller asks forward_route / forward_rehash
// whether a job hashes, hashes those bytes, and hands the value back.  The kernels of
// forward_kernels.hip keep no ladder of their own, and tests/cpp/fuzz_forward.cpp runs these
// functions against a sequential restatement of the reference's control flow under ASan + UBSan.
#pragma once
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

#ifdef __HIPCC__
#define HF3FS_FWD_FN __host__ __device__ __forceinline__
#else
#define HF3FS_FWD_FN inline
#endif

namespace hf3fs_crc {

constexpr uint64_t kForwardMaxJobs = 1ull << 30;
constexpr uint32_t kForwardRawEmpty = ~0u;  // the raw CRC of no bytes, either polynomial

// Where rungs A and B leave a job before anything is hashed.
enum : uint8_t {
  kFwdReturn = 0,       // decided: `status` answers
  kFwdNoSuccessor = 1,  // ReliableForwarding.cc:113-117
  kFwdSyncRead = 2,     // :160-214, the chunk is compared with its stored checksum first
  kFwdPlain = 3         // :215-222, the request goes out as it is
};

struct ForwardRoute {
  uint8_t where;
  uint8_t is_syncing;
  bool bad;     // a record the call refuses (status 3)
  bool hashes;  // kFwdSyncRead: the chunk bytes are hashed (typed, chunk_len > 0)
  int32_t status;
  uint32_t res_length, res_update_ver, res_commit_ver;  // updateResult after rung A
  uint32_t req_update_ver;                              // req.payload.updateVer after :404-405
};

// What the two calls count into d_info (one bit each, per job).
struct ForwardPrepCounts {
  uint8_t sent, returned, no_successor, hashed, mismatched, bad;
};
struct ForwardDoneCounts {
  uint8_t commit, returned, e7015, e4081, e4082, rehashed, corrupted, unhashable;
};

HF3FS_FWD_FN bool forward_is_wte(uint8_t t) {  // UpdateIO::isWriteTruncateExtend (Common.h:343)
  return t == HF3FS_UPDATE_WRITE || t == HF3FS_UPDATE_TRUNCATE || t == HF3FS_UPDATE_EXTEND;
}

// req.payload.updateVer as handleUpdate leaves it at :404-405 (only a successful update sets it).
HF3FS_FWD_FN uint32_t forward_req_update_ver(const hf3fs_crc_forward_job& j) {
  return j.upd_status == 0 && j.req_update_ver == 0 ? j.upd_update_ver : j.req_update_ver;
}

// May [addr, len) be hashed in `ctype` by a call that hashes in `type`?
HF3FS_FWD_FN bool forward_hashable(uint8_t ctype, uint64_t addr, uint32_t len, uint8_t type, uint32_t max_len) {
  if (ctype != HF3FS_CHECKSUM_NONE && ctype != type) return false;
  if (len > max_len) return false;
  return addr != 0 || len == 0;
}

// ChecksumInfo::create(ctype, bytes, len).value given the range kernels' value for len > 0.
HF3FS_FWD_FN uint32_t forward_created(uint8_t ctype, uint32_t len, uint32_t hashed) {
  if (ctype == HF3FS_CHECKSUM_NONE) return 0u;  // {NONE, 0} before the first byte (Common.h:150)
  return len ? hashed : kForwardRawEmpty;
}

// Rungs A and B up to the point where the syncing read's bytes are needed.
HF3FS_FWD_FN ForwardRoute forward_route(const hf3fs_crc_forward_job& j, uint8_t type, uint32_t max_len) {
  ForwardRoute r{kFwdReturn, 0, false, false, 0, 0, 0, 0, forward_req_update_ver(j)};
  const auto refuse = [&](int32_t code) { return r.status = code, r; };
  if (!forward_is_wte(j.update_type) && j.update_type != HF3FS_UPDATE_REMOVE)
    return r.bad = true, refuse(HF3FS_CRC_INVALID_ARG);
  // A. StorageOperator.cc:401-434
  r.res_length = j.upd_length;
  r.res_update_ver = j.upd_update_ver;
  r.res_commit_ver = j.upd_commit_ver;
  if (j.upd_status == 0) {
    if (r.req_update_ver != j.upd_update_ver) {                                         // :406-409
      r.res_length = r.res_update_ver = r.res_commit_ver = 0;                           // makeError
      return refuse(HF3FS_CRC_CHUNK_VERSION_MISMATCH);
    }
  } else if (j.upd_status == HF3FS_CRC_CHUNK_COMMITTED_UPDATE) {                        // :415-421
    r.res_length = j.length;
    r.res_update_ver = r.res_commit_ver = r.req_update_ver;
    return refuse(0);
  } else if (j.upd_status == HF3FS_CRC_CHUNK_STALE_UPDATE) {                            // :422-426
    r.res_length = j.length;
    r.res_update_ver = r.req_update_ver;
  } else {                                                                              // :411-414,427-434
    return refuse(j.upd_status);
  }
  // B. ReliableForwarding.cc:113-222
  if (!j.has_successor) return r.where = kFwdNoSuccessor, r;                            // :113-117
  r.is_syncing = j.successor_syncing ? 1 : 0;                                           // :152
  const bool read_for_syncing = forward_is_wte(j.update_type) && r.is_syncing &&
                                ((j.req_flags & HF3FS_FORWARD_REQ_SYNCING) || j.length != j.chunk_size);  // :158-159
  if (read_for_syncing) {
    if (j.chunk_status_in != 0) return refuse(j.chunk_status_in);                       // :190
    if (!forward_hashable(j.chunk_checksum_type, j.chunk, j.chunk_len, type, max_len))
      return r.bad = true, refuse(HF3FS_CRC_INVALID_ARG);
    r.where = kFwdSyncRead;
    r.hashes = j.chunk_checksum_type != HF3FS_CHECKSUM_NONE && j.chunk_len > 0;
    return r;
  }
  if (r.is_syncing && j.update_type != HF3FS_UPDATE_REMOVE && !j.engine_job && j.chunk_status_in != 0)
    return refuse(j.chunk_status_in);                                                   // :216-220
  r.where = kFwdPlain;
  return r;
}

// The rest of prepare: every output field of j (and the response presets of a job that is not
// sent).  hashed: the range kernels' value for the chunk, read only when r.hashes.
HF3FS_FWD_FN ForwardPrepCounts forward_prepare_settle(hf3fs_crc_forward_job& j, ForwardRoute r, uint32_t hashed,
                                                      uint32_t max_inline_bytes) {
  ForwardPrepCounts c{0, 0, 0, 0, 0, 0};
  uint32_t computed = 0;
  if (r.where == kFwdSyncRead) {                                      // BatchReadJob.cc:43-54
    computed = forward_created(j.chunk_checksum_type, j.chunk_len, r.hashes ? hashed : 0u);
    c.hashed = r.hashes ? 1 : 0;
    if (computed != j.chunk_checksum) {
      r.where = kFwdReturn;
      r.status = HF3FS_CRC_CHECKSUM_MISMATCH;
      c.mismatched = 1;
    }
  }
  j.status = r.status;
  j.res_length = r.res_length;
  j.res_update_ver = r.res_update_ver;
  j.res_commit_ver = r.res_commit_ver;
  j.computed = computed;
  j.is_syncing = r.where == kFwdReturn ? 0 : r.is_syncing;
  j.out_data = 0;
  j.out_offset = j.out_length = j.out_checksum = j.out_update_ver = j.out_commit_chain_ver = 0;
  j.out_update_type = j.out_checksum_type = j.out_flags = 0;
  j.commit_ver = r.where == kFwdReturn ? 0u : r.res_update_ver;      // StorageOperator.cc:441
  j.commit_chain_ver = 0;
  if (r.where != kFwdSyncRead && r.where != kFwdPlain) {             // the response a send would have filled
    j.fwd_status = r.where == kFwdNoSuccessor ? HF3FS_CRC_NO_SUCCESSOR_TARGET : 0;
    j.fwd_length = j.fwd_checksum = j.fwd_commit_ver = j.fwd_commit_chain_ver = 0;
    j.fwd_checksum_type = 0;
  }
  if (r.where == kFwdReturn) {
    j.action = HF3FS_FORWARD_RETURN;
    c.returned = 1;
    c.bad = r.bad ? 1 : 0;
    return c;
  }
  if (r.where == kFwdNoSuccessor) {
    j.action = HF3FS_FORWARD_NO_SUCCESSOR;
    j.commit_chain_ver = j.chain_ver;                                 // ReliableForwarding.cc:115
    c.no_successor = 1;
    return c;
  }
  j.action = HF3FS_FORWARD_SEND;
  c.sent = 1;
  uint8_t flags = (j.req_flags & HF3FS_FORWARD_REQ_SYNCING ? HF3FS_FORWARD_OUT_SYNCING : 0) |
                  (j.req_flags & HF3FS_FORWARD_REQ_INLINE ? HF3FS_FORWARD_OUT_INLINE : 0);
  if (r.is_syncing) {                                                 // :153-156
    flags |= HF3FS_FORWARD_OUT_SYNCING | HF3FS_FORWARD_OUT_COMMIT_CHAIN_VER;
    j.out_commit_chain_ver = j.chain_ver;
  }
  if (r.where == kFwdSyncRead) {                                      // :193-212
    flags &= (uint8_t)~HF3FS_FORWARD_OUT_INLINE;
    j.out_update_ver = j.chunk_update_ver;
    if (j.req_flags & HF3FS_FORWARD_REQ_SYNCING) j.out_commit_chain_ver = j.chunk_commit_chain_ver;
    j.out_offset = 0;
    j.out_length = j.chunk_len;
    j.out_data = j.chunk;
    j.out_checksum = j.chunk_checksum;
    j.out_checksum_type = j.chunk_checksum_type;
    j.out_update_type = HF3FS_UPDATE_WRITE;
    if (j.chunk_len <= max_inline_bytes) flags |= HF3FS_FORWARD_OUT_INLINE;
  } else {
    j.out_update_type = j.update_type;
    j.out_offset = j.offset;
    j.out_length = j.length;
    j.out_data = j.payload;
    j.out_checksum = j.req_checksum;
    j.out_checksum_type = j.req_checksum_type;
    j.out_update_ver = r.req_update_ver;
    if (r.is_syncing && j.update_type != HF3FS_UPDATE_REMOVE && !j.engine_job)
      j.out_update_ver = j.chunk_update_ver;                          // :215-221
  }
  j.out_flags = flags;
  return c;
}

// Does complete meet the job at all?
HF3FS_FWD_FN bool forward_completes(const hf3fs_crc_forward_job& j) {
  return j.action == HF3FS_FORWARD_SEND || j.action == HF3FS_FORWARD_NO_SUCCESSOR;
}
// ReliableForwarding.cc:263: is the outgoing buffer looked at again, and are its bytes hashed?
HF3FS_FWD_FN bool forward_rechecks(const hf3fs_crc_forward_job& j) {
  return forward_completes(j) && j.fwd_status == HF3FS_CRC_CHECKSUM_MISMATCH;
}
HF3FS_FWD_FN bool forward_rehash(const hf3fs_crc_forward_job& j, uint8_t type, uint32_t max_len) {
  return forward_rechecks(j) && forward_hashable(j.out_checksum_type, j.out_data, j.out_length, type, max_len) &&
         j.out_checksum_type != HF3FS_CHECKSUM_NONE && j.out_length > 0;
}

// Rungs C and D: every complete output of j.  hashed: the range kernels' value for the outgoing
// buffer, read only when forward_rehash(j).  Reads none of the fields it writes.
HF3FS_FWD_FN ForwardDoneCounts forward_complete_settle(hf3fs_crc_forward_job& j, uint8_t type, uint32_t max_len,
                                                       uint32_t hashed) {
  ForwardDoneCounts c{0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t commit_ver = 0, commit_chain_ver = 0, fwd_update_ver = 0, computed = 0;
  uint8_t corrupted = 0, action = HF3FS_FORWARD_RETURN;
  int32_t final_status = j.status;
  if (forward_completes(j)) {
    commit_ver = j.res_update_ver;                                                      // StorageOperator.cc:441
    if (j.action == HF3FS_FORWARD_NO_SUCCESSOR) commit_chain_ver = j.chain_ver;         // ReliableForwarding.cc:115
    // C. doForward's tail (:237-277), then forward's (:120-134)
    int32_t fwd = j.fwd_status;
    if (fwd == 0) {
      if (j.chain_ver < j.fwd_commit_chain_ver) {                                       // :238-245
        fwd = HF3FS_CRC_CHAIN_VERSION_MISMATCH;
        c.e4081 = 1;
      } else {
        if (j.is_syncing) fwd_update_ver = forward_req_update_ver(j);                   // :251
        commit_ver = j.fwd_commit_ver;                                                  // :121
        commit_chain_ver = j.fwd_commit_chain_ver;                                      // :123
        if (j.fwd_commit_chain_ver > j.chain_ver) {                                     // :125, never after :238
          fwd = HF3FS_CRC_CHAIN_VERSION_MISMATCH;
          c.e4081 = 1;
        }
      }
    } else if (forward_rechecks(j)) {                                                   // :263-276
      if (!forward_hashable(j.out_checksum_type, j.out_data, j.out_length, type, max_len)) {
        c.unhashable = 1;
      } else {
        const bool hashes = forward_rehash(j, type, max_len);
        computed = forward_created(j.out_checksum_type, j.out_length, hashes ? hashed : 0u);
        c.rehashed = hashes ? 1 : 0;
        corrupted = computed != j.out_checksum ? 1 : 0;                                 // :268 (the types are equal)
        c.corrupted = corrupted;
      }
    }
    // D. StorageOperator.cc:446-485
    if (commit_ver != j.res_update_ver) {                                               // :446-453
      final_status = HF3FS_CRC_CHUNK_VERSION_MISMATCH;
      c.e4082 = 1;
    } else if (fwd == 0) {
      const bool exempt = j.update_type == HF3FS_UPDATE_REMOVE &&
                          (j.fwd_checksum_type == HF3FS_CHECKSUM_NONE || j.upd_checksum_type == HF3FS_CHECKSUM_NONE ||
                           j.is_syncing);                                               // :465-466
      if (!exempt && (j.fwd_checksum_type != j.upd_checksum_type || j.fwd_checksum != j.upd_checksum)) {  // :475
        final_status = HF3FS_CRC_CLIENT_CHECKSUM_MISMATCH;
        c.e7015 = 1;
      } else {
        action = HF3FS_FORWARD_COMMIT;
      }
    } else if (fwd != HF3FS_CRC_NO_SUCCESSOR_TARGET) {                                  // :483-485
      final_status = fwd;
    } else {
      action = HF3FS_FORWARD_COMMIT;
    }
    if (action == HF3FS_FORWARD_COMMIT) final_status = 0;
  }
  j.final_action = action;
  j.final_status = final_status;
  j.commit_ver = commit_ver;
  j.commit_chain_ver = commit_chain_ver;
  j.fwd_update_ver = fwd_update_ver;
  j.buffer_computed = computed;
  j.buffer_corrupted = corrupted;
  c.commit = action == HF3FS_FORWARD_COMMIT ? 1 : 0;
  c.returned = c.commit ? 0 : 1;
  return c;
}

}  // namespace hf3fs_crc
