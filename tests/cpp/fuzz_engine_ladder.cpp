// fuzz_engine_ladder.cpp -- 3fs_amd/csrc/engine_plan.h (the two decisions the kernels of
// hf3fs_crc_update_engine run) against an independent sequential restatement: a map of chunk
// states and the reference's control flow (engine.rs:288-507 behind ChunkEngine.cc:15-110), one
// job at a time.  Stand-alone (its own main), built with -fsanitize=address,undefined by
// tests/test_update_engine_sanitized.py; no GPU, nothing loaded into Python.
//
// The driver hands state down each chunk's chain the way the step kernel does: the job's before-
// state is what the previous job of the chunk left; a job engine_update admits "runs" with a drawn
// pipeline verdict (OK with a drawn size and checksum, or a payload mismatch), one it refuses
// after the verify's place is settled as 4080 when its payload is bad and as its own code otherwise.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../../3fs_amd/csrc/engine_plan.h"

using namespace hf3fs_crc;

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  uint32_t below(uint32_t n) { return next() % n; }
};

struct Job {
  uint32_t chunk, update_ver, chain_ver, offset, length;
  uint64_t dst;
  uint8_t update_type, flags;
  bool record_ok, verify, payload_bad;
  uint32_t new_len, new_checksum;  // what the write would leave
};

// ---- the restatement: committed ChunkMeta and the writing list in maps ---------------------------
struct RefMeta {
  uint64_t pos;
  uint32_t len, checksum, chain_ver, chunk_ver;
};
struct RefEngine {
  std::map<uint32_t, RefMeta> committed;
  std::map<uint32_t, RefMeta> writing_list;
};

// -> status (detail through *detail)
int ref_update(RefEngine& eng, const Job& j, int* detail, bool* cow_out) {
  *detail = 0;
  *cow_out = false;
  const bool is_write = j.update_type == HF3FS_UPDATE_WRITE;
  const bool known = is_write || j.update_type == HF3FS_UPDATE_TRUNCATE || j.update_type == HF3FS_UPDATE_EXTEND;
  if (!j.record_ok || !known || !(j.flags & 1)) return *detail = 1, 3;
  if (j.verify && j.payload_bad) return 4080;  // 1. prepare update info
  const RefMeta old = eng.committed[j.chunk];  // 2. get old chunk (described by the caller when unknown)
  uint32_t out_commit_ver = old.chunk_ver, out_chain_ver = old.chain_ver;
  if (j.chain_ver < out_chain_ver) return 4081;  // 3. check version
  const bool is_syncing = (j.flags & 2) != 0;
  uint32_t new_chunk_ver;
  if (is_syncing) {
    new_chunk_ver = j.update_ver;
  } else if (j.update_ver > 0) {
    if (j.update_ver <= out_commit_ver) {
      return 4008;
    } else if (j.update_ver > out_commit_ver + 1) {
      return 4007;
    }
    new_chunk_ver = j.update_ver;
  } else {
    new_chunk_ver = out_commit_ver + 1;
  }
  // 4. do update: req.length is 0 for a truncate / extend (ChunkEngine.cc:49-52)
  const uint32_t req_length = is_write ? j.length : 0;
  const bool cow = is_syncing || (req_length > 0 && j.offset < old.len);
  if (cow && j.dst == 0) return *detail = 3, 3;
  if (eng.writing_list.count(j.chunk)) return *detail = 2, 3;
  RefMeta now{cow ? j.dst : old.pos, j.new_len, j.new_checksum, j.chain_ver, new_chunk_ver};
  eng.writing_list[j.chunk] = now;
  *cow_out = cow;
  return 0;
}

int ref_commit(RefEngine& eng, const Job& j, int* detail) {
  *detail = 0;
  auto it = eng.writing_list.find(j.chunk);
  if (it == eng.writing_list.end()) return *detail = 4, 3;
  RefMeta m = it->second;
  m.chain_ver = j.chain_ver;  // chunk->set_chain_ver(job.commitChainVer())
  eng.committed[j.chunk] = m;
  eng.writing_list.erase(it);
  return 0;
}

bool same(const EngState& s, const RefEngine& eng, uint32_t c) {
  const RefMeta& m = eng.committed.at(c);
  if (s.addr != m.pos || s.size != m.len || s.checksum != m.checksum || s.chain_ver != m.chain_ver ||
      s.chunk_ver != m.chunk_ver)
    return false;
  auto it = eng.writing_list.find(c);
  if (it == eng.writing_list.end())
    return s.w_addr == 0 && s.w_len == 0 && s.w_checksum == 0 && s.w_chain_ver == 0 && s.w_chunk_ver == 0;
  const RefMeta& w = it->second;
  return s.w_addr == w.pos && s.w_len == w.len && s.w_checksum == w.checksum && s.w_chain_ver == w.chain_ver &&
         s.w_chunk_ver == w.chunk_ver;
}

bool equal(const EngState& a, const EngState& b) {
  return a.addr == b.addr && a.size == b.size && a.checksum == b.checksum && a.chain_ver == b.chain_ver &&
         a.chunk_ver == b.chunk_ver && a.ctype == b.ctype && a.w_addr == b.w_addr && a.w_len == b.w_len &&
         a.w_checksum == b.w_checksum && a.w_chain_ver == b.w_chain_ver && a.w_chunk_ver == b.w_chunk_ver;
}

#define CHECK(c)                                                                   \
  do {                                                                             \
    if (!(c)) {                                                                    \
      fprintf(stderr, "queue %d job %zu: %s (line %d)\n", q, i, #c, __LINE__);     \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

}  // namespace

int main(int argc, char** argv) {
  const int queues = argc > 1 ? atoi(argv[1]) : 2000;
  Rng rng{0xE61E5EEDull};
  uint64_t jobs_run = 0, deferred = 0, wraps = 0, cows = 0, in_place = 0;
  std::set<int> statuses, details;
  for (int q = 0; q < queues; ++q) {
    const uint32_t max_len = rng.below(2) ? 512u : 128u << 10;
    const uint32_t n_chunks = 1 + rng.below(12);
    const size_t n = 1 + rng.below(96);
    // versions near 0 and near 2^32 so that the uint32 wrap of chunk_ver + 1 is walked too
    const uint32_t origin = rng.below(4) == 0 ? 0xFFFFFFFCu : rng.below(3);
    RefEngine eng;
    std::vector<EngState> now(n_chunks);
    uint64_t next_alloc = 0x10000;
    for (uint32_t c = 0; c < n_chunks; ++c) {
      const uint32_t len0 = rng.below(3) ? rng.below(max_len) : 0u;
      RefMeta m{next_alloc, len0, rng.next(), 1 + rng.below(4), origin + rng.below(4)};
      next_alloc += max_len;
      eng.committed[c] = m;
      EngState s{m.pos, m.len, m.checksum, m.chain_ver, m.chunk_ver, HF3FS_CHECKSUM_CRC32C, 0, 0, 0, 0, 0};
      if (rng.below(6) == 0) {  // a live holder the caller supplies
        RefMeta w{next_alloc, rng.below(max_len), rng.next(), m.chain_ver, m.chunk_ver + 1u};
        next_alloc += max_len;
        eng.writing_list[c] = w;
        s.w_addr = w.pos, s.w_len = w.len, s.w_checksum = w.checksum, s.w_chain_ver = w.chain_ver,
        s.w_chunk_ver = w.chunk_ver;
      }
      now[c] = s;
    }
    for (size_t i = 0; i < n; ++i) {
      Job j{};
      j.chunk = rng.below(n_chunks);
      const EngState before = now[j.chunk];
      const uint32_t kind = rng.below(16);
      static const uint8_t kTypes[6] = {HF3FS_UPDATE_WRITE, HF3FS_UPDATE_TRUNCATE, HF3FS_UPDATE_EXTEND,
                                        HF3FS_UPDATE_COMMIT, 2 /* REMOVE */, 0};
      j.update_type = kTypes[kind < 7 ? 0 : kind < 8 ? 1 : kind < 9 ? 2 : kind < 14 ? 3 : kind < 15 ? 4 : 5];
      j.flags = (uint8_t)((rng.below(16) == 0 ? 0 : HF3FS_UPDATE_FLAG_ENGINE) |
                          (rng.below(8) == 0 ? HF3FS_UPDATE_FLAG_SYNCING : 0));
      j.chain_ver = 1 + rng.below(5);
      j.update_ver = rng.below(5) == 0 ? 0u : before.chunk_ver + rng.below(4) - 1u;
      j.length = rng.below(4) ? 1 + rng.below(max_len / 2) : 0;
      j.offset = rng.below(3) == 0 ? before.size : rng.below(max_len / 2);
      j.dst = rng.below(5) ? next_alloc : 0;
      next_alloc += max_len;
      j.record_ok = rng.below(16) != 0;
      j.verify = j.update_type == HF3FS_UPDATE_WRITE && j.length != 0 && rng.below(8) != 0;
      j.payload_bad = rng.below(5) == 0;
      j.new_len = rng.below(max_len + 1);
      j.new_checksum = rng.next();
      if (before.chunk_ver + 1u == 0u || j.update_ver == 0xFFFFFFFFu) ++wraps;

      const bool commit = j.update_type == HF3FS_UPDATE_COMMIT;
      int want_detail = 0;
      bool want_cow = false;
      const int want = commit ? ref_commit(eng, j, &want_detail) : ref_update(eng, j, &want_detail, &want_cow);

      const EngVerdict v = commit ? engine_commit(before, j.chain_ver)
                                  : engine_update(before, j.update_ver, j.chain_ver, j.dst, j.update_type, j.flags,
                                                  j.offset, j.length, j.record_ok);
      int got = v.status, got_detail = v.detail;
      EngState after = before;
      if (commit) {
        CHECK(v.where == kEngCommit);
        if (got == HF3FS_CRC_OK) after = v.next;
      } else if (v.where == kEngAdmit) {
        CHECK(got == HF3FS_CRC_OK && got_detail == 0);
        got = j.verify && j.payload_bad ? HF3FS_CRC_CHECKSUM_MISMATCH : HF3FS_CRC_OK;  // the pipeline's verdict
        if (got == HF3FS_CRC_OK) {
          after = eng_written(v.next, j.new_len, j.new_checksum);
          CHECK((v.cow != 0) == want_cow);
          CHECK(after.w_addr == (v.cow ? j.dst : before.addr));
          ++(v.cow ? cows : in_place);
        }
      } else if (v.where == kEngLate) {
        CHECK(got != HF3FS_CRC_OK);
        ++deferred;
        if (j.verify && j.payload_bad) got = HF3FS_CRC_CHECKSUM_MISMATCH, got_detail = 0;  // the settle kernel's choice
      } else {
        CHECK(v.where == kEngEarly && got == HF3FS_CRC_INVALID_ARG && got_detail == HF3FS_ENGINE_DETAIL_RECORD);
      }
      if (v.status != HF3FS_CRC_OK) CHECK(equal(v.next, before));  // every refusal hands the before-state on
      CHECK(got == want);
      CHECK(got_detail == want_detail);
      CHECK((got_detail != 0) == (got == HF3FS_CRC_INVALID_ARG));
      // the committed {len, checksum} travel in the IO record; the type is CRC32C throughout here
      CHECK(same(after, eng, j.chunk));
      now[j.chunk] = after;
      statuses.insert(got);
      details.insert(got_detail);
      ++jobs_run;
    }
  }
  printf("{\"fuzz_engine_ladder\": \"ok\", \"queues\": %d, \"jobs\": %llu, \"deferred\": %llu, \"wraps\": %llu, "
         "\"cows\": %llu, \"in_place\": %llu, \"statuses\": %zu, \"details\": %zu}\n",
         queues, (unsigned long long)jobs_run, (unsigned long long)deferred, (unsigned long long)wraps,
         (unsigned long long)cows, (unsigned long long)in_place, statuses.size(), details.size());
  return 0;
}
