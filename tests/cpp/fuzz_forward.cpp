// fuzz_forward.cpp -- stand-alone (own main, no GPU, no Python): random jobs through the decisions of
// hf3fs_crc_forward_prepare / _complete (3fs_amd/csrc/forward_plan.h, the header the kernels include)
// and through a restatement of the reference's control flow, written as the reference's three
// functions with their own local structures (StorageOperator::handleUpdate,
// src/storage/service/StorageOperator.cc:401-485; ReliableForwarding::forward and doForward,
// src/storage/service/ReliableForwarding.cc:113-278; AioReadJob::setResult,
// src/storage/aio/BatchReadJob.cc:43-54).  Both start from the same record with poisoned outputs;
// afterwards the two records must be equal byte for byte, after prepare and again after complete.
// Built by tests/test_forward_sanitized.py with -fsanitize=address,undefined.
//
// Bytes are not hashed here: "memory" is a function of (address, length, type), the same for both
// sides, so that a stored checksum can be made right or wrong at will.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <optional>
#include <string>

#include "../../3fs_amd/csrc/forward_plan.h"

namespace {

using Job = hf3fs_crc_forward_job;
constexpr uint8_t kNone = 0, kCrc32c = 1, kCrc32 = 2;
constexpr uint32_t kMaxLen = 4096;

std::map<std::string, uint64_t> g_branches;
void took(const char* name) { ++g_branches[name]; }

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }
bool chance(uint32_t percent) { return below(100) < percent; }

// What hashing [addr, addr + len) in `type` gives (len > 0, type != NONE).
uint32_t memory_hash(uint64_t addr, uint32_t len, uint8_t type) {
  uint64_t z = addr * 0xD6E8FEB86659FD93ull ^ ((uint64_t)len << 8) ^ type;
  z = (z ^ (z >> 32)) * 0xD6E8FEB86659FD93ull;
  return (uint32_t)(z ^ (z >> 32));
}

// ---- the reference, restated ----------------------------------------------------------------------
struct ChecksumInfo {
  uint8_t type = kNone;
  uint32_t value = 0;
  bool operator==(const ChecksumInfo& o) const { return type == o.type && value == o.value; }
  bool operator!=(const ChecksumInfo& o) const { return !(*this == o); }
  static ChecksumInfo create(uint8_t type, uint64_t addr, uint32_t len) {  // Common.h:150
    if (type == kNone) return {kNone, 0};
    return {type, len ? memory_hash(addr, len, type) : ~0u};
  }
};
struct IOResult {
  int32_t code = 0;  // 0: lengthInfo holds a value
  uint32_t length = 0, updateVer = 0, commitVer = 0, commitChainVer = 0;
  ChecksumInfo checksum;
};
struct CommitIO {
  uint32_t commitVer = 0, commitChainVer = 0;
  bool isSyncing = false, isRemove = false;
};
struct UpdateReq {
  uint8_t updateType;
  uint32_t offset, length, updateVer;
  uint64_t rdmabuf;
  ChecksumInfo checksum;
  bool isSyncing, inlineData;
  std::optional<uint32_t> commitChainVer;  // set by doForward only
};

bool can_hash(uint8_t ctype, uint64_t addr, uint32_t len, uint8_t call_type) {  // the library's own limits
  return (ctype == kNone || ctype == call_type) && len <= kMaxLen && (addr != 0 || len == 0);
}

// A job that is not sent gets the response fields a send would have filled.
void preset_response(Job& j, int32_t fwd_status) {
  j.fwd_status = fwd_status;
  j.fwd_length = j.fwd_checksum = j.fwd_commit_ver = j.fwd_commit_chain_ver = 0;
  j.fwd_checksum_type = 0;
}

void write_outputs(Job& j, int32_t status, const IOResult& res, uint32_t computed) {
  j.action = HF3FS_FORWARD_RETURN;
  j.status = status;
  j.res_length = res.length;
  j.res_update_ver = res.updateVer;
  j.res_commit_ver = res.commitVer;
  j.computed = computed;
  j.is_syncing = 0;
  j.out_data = 0;
  j.out_offset = j.out_length = j.out_checksum = j.out_update_ver = j.out_commit_chain_ver = 0;
  j.out_update_type = j.out_checksum_type = j.out_flags = 0;
  j.commit_ver = j.commit_chain_ver = 0;
}

void write_returned(Job& j, int32_t status, const IOResult& res, uint32_t computed) {
  write_outputs(j, status, res, computed);
  preset_response(j, 0);
}

// handleUpdate up to the send.
void reference_prepare(Job& j, uint8_t call_type, uint32_t max_inline) {
  const IOResult nothing;
  if (j.update_type != 1 && j.update_type != 2 && j.update_type != 4 && j.update_type != 8) {
    took("bad_update_type");
    return write_returned(j, 3, nothing, 0);
  }
  uint32_t reqUpdateVer = j.req_update_ver;
  IOResult updateResult;
  updateResult.code = j.upd_status;
  updateResult.length = j.upd_length;
  updateResult.updateVer = j.upd_update_ver;
  updateResult.commitVer = j.upd_commit_ver;
  const uint32_t code = (uint32_t)updateResult.code;
  if (code == 0) {
    if (reqUpdateVer == 0) {
      took("a_version_adopted");
      reqUpdateVer = updateResult.updateVer;
    } else if (reqUpdateVer != updateResult.updateVer) {
      took("a_4082");
      return write_returned(j, 4082, nothing, 0);
    } else {
      took("a_version_equal");
    }
  } else if (code == 4007) {
    took("a_missing");
    return write_returned(j, 4007, updateResult, 0);
  } else if (code == 4008) {
    took("a_committed");
    updateResult.length = j.length;
    updateResult.updateVer = reqUpdateVer;
    updateResult.commitVer = reqUpdateVer;
    return write_returned(j, 0, updateResult, 0);
  } else if (code == 4006) {
    took("a_stale");
    updateResult.length = j.length;
    updateResult.updateVer = reqUpdateVer;
  } else if (code == 4012) {
    took("a_advance");
    return write_returned(j, 4012, updateResult, 0);
  } else {
    took("a_other_error");
    return write_returned(j, (int32_t)code, updateResult, 0);
  }
  CommitIO commitIO;
  commitIO.commitVer = updateResult.updateVer;
  commitIO.isRemove = j.update_type == 2;

  // forward()
  if (!j.has_successor) {
    took("b_no_successor");
    commitIO.commitChainVer = j.chain_ver;
    write_outputs(j, 0, updateResult, 0);
    preset_response(j, 4033);
    j.action = HF3FS_FORWARD_NO_SUCCESSOR;
    j.commit_ver = commitIO.commitVer;
    j.commit_chain_ver = commitIO.commitChainVer;
    return;
  }
  // doForward()
  UpdateReq updateReq{j.update_type, j.offset, j.length, reqUpdateVer, j.payload,
                      ChecksumInfo{j.req_checksum_type, j.req_checksum}, (j.req_flags & 1) != 0,
                      (j.req_flags & 2) != 0, std::nullopt};
  const bool reqIsSyncing = (j.req_flags & 1) != 0;
  bool& isSyncing = commitIO.isSyncing;
  isSyncing = j.successor_syncing != 0;
  if (isSyncing) {
    updateReq.isSyncing = true;
    updateReq.commitChainVer = j.chain_ver;
  }
  const bool isWriteTruncateExtend = j.update_type == 1 || j.update_type == 4 || j.update_type == 8;
  const bool readForSyncing = isWriteTruncateExtend && isSyncing && (reqIsSyncing || j.length != j.chunk_size);
  uint32_t computed = 0;
  if (readForSyncing) {
    took(reqIsSyncing ? "b_read_syncing_request" : "b_read_partial_write");
    if (j.chunk_status_in != 0) {
      took("b_read_failed");
      return write_returned(j, j.chunk_status_in, updateResult, 0);
    }
    if (!can_hash(j.chunk_checksum_type, j.chunk, j.chunk_len, call_type)) {
      took(j.chunk_checksum_type != kNone && j.chunk_checksum_type != call_type ? "b_read_bad_type"
           : j.chunk_len > kMaxLen                                              ? "b_read_bad_length"
                                                                                : "b_read_bad_null");
      return write_returned(j, 3, updateResult, 0);
    }
    const ChecksumInfo chunkChecksum{j.chunk_checksum_type, j.chunk_checksum};
    const ChecksumInfo realChecksum = ChecksumInfo::create(chunkChecksum.type, j.chunk, j.chunk_len);
    computed = realChecksum.value;
    if (realChecksum != chunkChecksum) {
      took(chunkChecksum.type == kNone ? "b_read_none_mismatch" : "b_read_mismatch");
      return write_returned(j, 4080, updateResult, computed);
    }
    took(chunkChecksum.type == kNone ? "b_read_none_ok" : j.chunk_len == 0 ? "b_read_empty_ok" : "b_read_ok");
    if (updateReq.inlineData) updateReq.inlineData = false;
    const uint32_t length = j.chunk_len;
    updateReq.updateVer = j.chunk_update_ver;
    if (reqIsSyncing) updateReq.commitChainVer = j.chunk_commit_chain_ver;
    updateReq.offset = 0;
    updateReq.length = length;
    updateReq.rdmabuf = j.chunk;
    updateReq.checksum = chunkChecksum;
    updateReq.updateType = 1;
    if (length <= max_inline) {
      took("b_read_inline");
      updateReq.inlineData = true;
    } else {
      took("b_read_not_inline");
    }
  } else if (isSyncing && !commitIO.isRemove && !j.engine_job) {
    if (j.chunk_status_in != 0) {
      took("b_query_failed");
      return write_returned(j, j.chunk_status_in, updateResult, 0);
    }
    took("b_query");
    updateReq.updateVer = j.chunk_update_ver;
  } else {
    took(!isSyncing ? "b_plain" : commitIO.isRemove ? "b_syncing_remove" : "b_syncing_engine_job");
  }
  write_outputs(j, 0, updateResult, computed);  // (the response is the host's to write)
  j.action = HF3FS_FORWARD_SEND;
  j.is_syncing = isSyncing;
  j.commit_ver = commitIO.commitVer;
  j.out_update_type = updateReq.updateType;
  j.out_offset = updateReq.offset;
  j.out_length = updateReq.length;
  j.out_data = updateReq.rdmabuf;
  j.out_checksum_type = updateReq.checksum.type;
  j.out_checksum = updateReq.checksum.value;
  j.out_update_ver = updateReq.updateVer;
  j.out_commit_chain_ver = updateReq.commitChainVer.value_or(0);
  j.out_flags = (uint8_t)((updateReq.isSyncing ? 1 : 0) | (updateReq.inlineData ? 2 : 0) |
                          (updateReq.commitChainVer ? 4 : 0));
}

// From the answer on.
void reference_complete(Job& j, uint8_t call_type) {
  j.buffer_computed = 0;
  j.buffer_corrupted = 0;
  j.fwd_update_ver = 0;
  if (j.action != HF3FS_FORWARD_SEND && j.action != HF3FS_FORWARD_NO_SUCCESSOR) {
    took("d_returned_in_prepare");
    j.final_action = HF3FS_FORWARD_RETURN;
    j.final_status = j.status;
    j.commit_ver = j.commit_chain_ver = 0;
    return;
  }
  uint32_t reqUpdateVer = j.req_update_ver;
  if (j.upd_status == 0 && reqUpdateVer == 0) reqUpdateVer = j.upd_update_ver;
  const uint32_t localUpdateVer = j.res_update_ver;
  CommitIO commitIO;
  commitIO.commitVer = localUpdateVer;
  commitIO.isSyncing = j.is_syncing != 0;
  commitIO.isRemove = j.update_type == 2;
  IOResult forwardResult;
  if (j.action == HF3FS_FORWARD_NO_SUCCESSOR) commitIO.commitChainVer = j.chain_ver;
  {  // doForward's tail
    IOResult result;
    result.code = j.fwd_status;
    result.length = j.fwd_length;
    result.commitVer = j.fwd_commit_ver;
    result.commitChainVer = j.fwd_commit_chain_ver;
    result.checksum = {j.fwd_checksum_type, j.fwd_checksum};
    if (result.code == 0) {
      if (j.chain_ver < result.commitChainVer) {
        took("c_4081");
        result = IOResult{};
        result.code = 4081;
      } else if (commitIO.isSyncing) {
        took("c_ok_syncing");
        j.fwd_update_ver = reqUpdateVer;
      } else {
        took("c_ok");
      }
    } else if (result.code == 4080) {
      const ChecksumInfo reqChecksum{j.out_checksum_type, j.out_checksum};
      if (!can_hash(reqChecksum.type, j.out_data, j.out_length, call_type)) {
        took("c_4080_unhashable");
      } else {
        const ChecksumInfo realChecksum = ChecksumInfo::create(reqChecksum.type, j.out_data, j.out_length);
        j.buffer_computed = realChecksum.value;
        if (reqChecksum != realChecksum) {
          took(reqChecksum.type == kNone ? "c_4080_none_corrupted" : "c_4080_corrupted");
          j.buffer_corrupted = 1;
        } else {
          took(reqChecksum.type == kNone ? "c_4080_none_intact" : "c_4080_intact");
        }
      }
    }
    forwardResult = result;
  }
  if (forwardResult.code == 0) {  // forward()'s tail
    commitIO.commitVer = forwardResult.commitVer;
    commitIO.commitChainVer = forwardResult.commitChainVer;
    if (forwardResult.commitChainVer > j.chain_ver) {
      took("c_forward_4081_unreachable");
      forwardResult.code = 4081;
    }
  }
  j.commit_ver = commitIO.commitVer;
  j.commit_chain_ver = commitIO.commitChainVer;
  // handleUpdate's tail
  if (commitIO.commitVer != localUpdateVer) {
    took("d_4082");
    j.final_action = HF3FS_FORWARD_RETURN;
    j.final_status = 4082;
    return;
  }
  if (forwardResult.code == 0) {
    const ChecksumInfo local{j.upd_checksum_type, j.upd_checksum};
    if (commitIO.isRemove && (forwardResult.checksum.type == kNone || local.type == kNone || commitIO.isSyncing)) {
      took(commitIO.isSyncing ? "d_remove_exempt_syncing" : "d_remove_exempt_none");
    } else if (forwardResult.checksum != local) {
      took(forwardResult.checksum.type != local.type ? "d_7015_type" : "d_7015_value");
      j.final_action = HF3FS_FORWARD_RETURN;
      j.final_status = 7015;
      return;
    } else {
      took("d_checksums_equal");
    }
  } else if (forwardResult.code != 4033) {
    took("d_forward_error");
    j.final_action = HF3FS_FORWARD_RETURN;
    j.final_status = forwardResult.code;
    return;
  } else {
    took(j.action == HF3FS_FORWARD_NO_SUCCESSOR ? "d_4033_no_successor" : "d_4033_answered");
  }
  j.final_action = HF3FS_FORWARD_COMMIT;
  j.final_status = 0;
}

// ---- the generator --------------------------------------------------------------------------------
Job random_job(uint8_t call_type) {
  Job j;
  memset(&j, 0xA5, sizeof(j));  // every output poisoned
  memset(j.reserved0, 0, sizeof(j.reserved0));
  memset(j.reserved1, 0, sizeof(j.reserved1));
  const uint8_t other = call_type == kCrc32c ? kCrc32 : kCrc32c;
  static const uint8_t types[] = {1, 1, 1, 1, 1, 1, 2, 2, 4, 8, 16, 0};
  j.update_type = types[below(12)];
  j.payload = chance(95) ? 0x10000 + below(1 << 20) : 0;
  j.chunk = chance(94) ? 0x4000000 + below(1 << 20) : 0;
  j.offset = below(64);
  j.length = chance(5) ? kMaxLen + 1 + below(8) : below(kMaxLen + 1);
  j.chunk_size = chance(35) ? j.length : kMaxLen;
  j.upd_update_ver = 1 + below(5);
  j.req_update_ver = chance(30) ? 0 : chance(88) ? j.upd_update_ver : j.upd_update_ver + 1;
  j.req_checksum_type = chance(15) ? kNone : chance(92) ? call_type : other;
  j.req_flags = (uint8_t)below(4);
  static const int32_t codes[] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4006, 4006, 4007, 4008, 4012, 4010};
  j.upd_status = codes[below(20)];
  j.upd_length = j.length;
  j.upd_commit_ver = j.upd_update_ver - 1;
  j.upd_checksum_type = chance(15) ? kNone : chance(90) ? call_type : other;
  j.upd_checksum = (uint32_t)rnd();
  j.chain_ver = 1 + below(4);
  j.has_successor = chance(88);
  j.successor_syncing = chance(60);
  j.engine_job = chance(30);
  j.chunk_len = chance(4) ? kMaxLen + 1 : chance(6) ? 0 : below(kMaxLen + 1);
  j.chunk_checksum_type = chance(12) ? kNone : chance(94) ? call_type : other;
  j.chunk_checksum = ChecksumInfo::create(j.chunk_checksum_type, j.chunk, j.chunk_len).value;
  if (chance(12)) j.chunk_checksum ^= 1u << below(32);
  j.chunk_update_ver = 1 + below(9);
  j.chunk_commit_chain_ver = 1 + below(4);
  j.chunk_status_in = chance(8) ? 4010 : 0;
  // the request checksum describes the payload, mostly
  j.req_checksum = ChecksumInfo::create(j.req_checksum_type, j.payload, j.length).value;
  if (chance(30)) j.req_checksum ^= 1u << below(32);
  return j;
}

void random_answer(Job& j) {
  const uint32_t kind = chance(40) ? 0 : 1 + below(8);
  j.fwd_status = kind == 1 || kind == 2 ? 4080 : kind == 3 ? 4010 : kind == 4 ? 4033 : 0;
  j.fwd_length = j.upd_length;
  j.fwd_checksum_type = kind == 5 ? (uint8_t)((j.upd_checksum_type + 1) % 3) : j.upd_checksum_type;
  j.fwd_checksum = kind == 6 ? j.upd_checksum ^ (1u << below(32)) : j.upd_checksum;
  j.fwd_commit_ver = kind == 7 ? j.res_update_ver + 1 : j.res_update_ver;
  j.fwd_commit_chain_ver = kind == 8 ? j.chain_ver + 1 + below(3) : j.chain_ver - below(2);
}

uint32_t hashed_for(uint64_t addr, uint32_t len, uint8_t type) { return memory_hash(addr, len, type); }

[[noreturn]] void differ(const char* phase, uint64_t i, const Job& a, const Job& b) {
  const uint8_t *pa = (const uint8_t*)&a, *pb = (const uint8_t*)&b;
  for (size_t k = 0; k < sizeof(Job); ++k)
    if (pa[k] != pb[k]) {
      fprintf(stderr, "job %llu: %s differs at byte %zu: plan %02x, reference %02x\n", (unsigned long long)i, phase, k,
              pa[k], pb[k]);
      break;
    }
  exit(1);
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 200000;
  using namespace hf3fs_crc;
  uint64_t prep_info[2][8] = {}, done_info[2][8] = {};
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t call_type = chance(50) ? kCrc32c : kCrc32;
    const uint32_t max_inline = chance(50) ? 0 : below(kMaxLen + 2);
    const Job start = random_job(call_type);
    Job a = start, b = start;
    // the plan, driven as the kernels drive it
    const ForwardRoute r = forward_route(a, call_type, kMaxLen);
    const uint32_t v = r.hashes ? hashed_for(a.chunk, a.chunk_len, a.chunk_checksum_type) : 0xDEADBEEFu;
    const ForwardPrepCounts pc = forward_prepare_settle(a, r, r.hashes ? v : 0u, max_inline);
    reference_prepare(b, call_type, max_inline);
    if (memcmp(&a, &b, sizeof(Job)) != 0) differ("prepare", i, a, b);
    if (memcmp(&a, &start, offsetof(Job, out_data)) != 0) differ("prepare wrote an input", i, a, start);
    const uint8_t pbits[8] = {pc.sent, pc.returned, pc.no_successor, pc.hashed, pc.mismatched, pc.bad, 0, 0};
    for (int w = 0; w < 8; ++w) prep_info[0][w] += pbits[w];
    prep_info[1][0] += b.action == HF3FS_FORWARD_SEND;
    prep_info[1][1] += b.action == HF3FS_FORWARD_RETURN;
    prep_info[1][2] += b.action == HF3FS_FORWARD_NO_SUCCESSOR;
    prep_info[1][4] += b.action == HF3FS_FORWARD_RETURN && b.status == 4080;
    prep_info[1][5] += b.action == HF3FS_FORWARD_RETURN && b.status == 3;
    // the successor's answer, the same on both sides; twice, as a resent job's would be
    for (int round = 0; round < 2; ++round) {
      if (a.action == HF3FS_FORWARD_SEND) {
        random_answer(a);
        memcpy(&b, &a, sizeof(Job));
      }
      const Job before = a;
      const bool hashes = forward_rehash(a, call_type, kMaxLen);
      const uint32_t hv = hashes ? hashed_for(a.out_data, a.out_length, a.out_checksum_type) : 0xDEADBEEFu;
      const ForwardDoneCounts dc = forward_complete_settle(a, call_type, kMaxLen, hashes ? hv : 0u);
      reference_complete(b, call_type);
      if (memcmp(&a, &b, sizeof(Job)) != 0) differ("complete", i, a, b);
      if (memcmp(&a, &before, offsetof(Job, final_status)) != 0) differ("complete wrote an input", i, a, before);
      if (round) continue;
      const uint8_t dbits[8] = {dc.commit, dc.returned, dc.e7015, dc.e4081, dc.e4082, dc.rehashed, dc.corrupted,
                                dc.unhashable};
      for (int w = 0; w < 8; ++w) done_info[0][w] += dbits[w];
      done_info[1][0] += b.final_action == HF3FS_FORWARD_COMMIT;
      done_info[1][1] += b.final_action == HF3FS_FORWARD_RETURN;
      done_info[1][2] += b.final_status == 7015;
      done_info[1][4] += b.final_status == 4082 && b.action != HF3FS_FORWARD_RETURN;
      done_info[1][6] += b.buffer_corrupted;
    }
  }
  for (int w : {0, 1, 2, 4, 5})
    if (prep_info[0][w] != prep_info[1][w]) return fprintf(stderr, "prepare info word %d\n", w), 1;
  for (int w : {0, 1, 2, 4, 6})
    if (done_info[0][w] != done_info[1][w]) return fprintf(stderr, "complete info word %d\n", w), 1;
  if (done_info[0][0] + done_info[0][1] != n) return fprintf(stderr, "commits + returned != n\n"), 1;
  printf("{\"fuzz_forward\": \"ok\", \"jobs\": %llu, \"sent\": %llu, \"commits\": %llu, \"branches\": {",
         (unsigned long long)n, (unsigned long long)prep_info[0][0], (unsigned long long)done_info[0][0]);
  bool first = true;
  for (const auto& kv : g_branches) {
    printf("%s\"%s\": %llu", first ? "" : ", ", kv.first.c_str(), (unsigned long long)kv.second);
    first = false;
  }
  printf("}}\n");
  return 0;
}
