// fuzz_version_ladder.cpp -- 3fs_amd/csrc/version_plan.h (the two ladders the kernels of
// hf3fs_crc_update_versioned run) against an independent sequential restatement: a map of chunk
// states and the reference's if-chains (ChunkReplica.cc:171-245, :397-467), one job at a time.
// Stand-alone (its own main), built with -fsanitize=address,undefined by
// tests/test_update_versioned_sanitized.py; no GPU, nothing loaded into Python.
//
// The driver hands state down each chunk's chain the way the step kernel does: the job's before-
// state is what the previous job of the chunk left; a job the update ladder admits "runs" with a
// drawn pipeline verdict (OK or a payload mismatch), one it refuses at the version rungs is
// settled as 4080 when its payload is bad and as the ladder's code otherwise.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <set>
#include <vector>

#include "../../3fs_amd/csrc/version_plan.h"

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
  uint32_t chunk, io_ver, job_chain_ver;
  uint8_t update_type, flags;
  bool is_force, record_ok, verify, payload_bad;
};

// ---- the restatement: ChunkMetadata in a map, the reference's control flow ------------------------
struct RefMeta {
  uint32_t chainVer, updateVer, commitVer, chunkSize;
  int chunkState;    // 0 COMMIT, 1 DIRTY, 2 CLEAN
  int recycleState;  // 0 NORMAL
};

int ref_update(RefMeta& meta, const Job& j, uint32_t chunkSize) {
  if (!j.record_ok || (j.flags & 1)) return 3;
  if (meta.chunkSize != chunkSize) return 4015;
  const bool isSyncing = (j.flags & 2) != 0;
  if (meta.chunkState == 1 && !isSyncing) return 4005;
  if (j.job_chain_ver < meta.chainVer && meta.chunkState == 0) return 4081;
  if (j.verify && j.payload_bad) return 4080;
  RefMeta m = meta;  // (the reference mutates a copy and returns before store.set on every refusal)
  if (isSyncing) {
    m.updateVer = j.io_ver;
    m.commitVer = j.io_ver - 1;
    m.recycleState = 0;
  } else if (j.io_ver > 0) {
    if (j.io_ver <= m.commitVer) {
      return 4008;
    } else if (j.io_ver <= m.updateVer) {
      return 4006;
    } else if (j.io_ver > m.updateVer + 1) {
      return 4007;
    }
    m.updateVer = j.io_ver;
  } else {
    m.updateVer += 1;
    if (m.updateVer > m.commitVer + 1) return 4012;
  }
  m.chunkState = 1;
  m.chainVer = j.job_chain_ver;
  m.chunkState = 2;
  meta = m;
  return 0;
}

int ref_commit(RefMeta& meta, const Job& j) {
  if ((j.flags & 1) || meta.recycleState != 0) return 3;
  if (j.job_chain_ver < meta.chainVer) return 4081;
  if (j.io_ver > meta.updateVer) return 4082;
  if (j.is_force) {
    meta.chunkState = 2;
    meta.commitVer = j.io_ver;
  } else if (meta.chunkState == 1) {
    return 4005;
  } else if (meta.commitVer < j.io_ver) {
    meta.commitVer = j.io_ver;
  } else {
    return 4023;
  }
  if (meta.commitVer == meta.updateVer) {
    meta.chunkState = 0;
    meta.chainVer = j.job_chain_ver;
  }
  return 0;
}

bool same(const VerState& s, const RefMeta& m) {
  return s.chain_ver == m.chainVer && s.update_ver == m.updateVer && s.commit_ver == m.commitVer &&
         s.meta_chunk_size == m.chunkSize && s.chunk_state == m.chunkState && s.recycle_state == m.recycleState;
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
  Rng rng{0x5EEDull};
  uint64_t jobs_run = 0, deferred = 0, wraps = 0;
  std::set<int> update_codes, commit_codes;
  for (int q = 0; q < queues; ++q) {
    const uint32_t max_len = rng.below(2) ? 512u : 128u << 10;
    const uint32_t n_chunks = 1 + rng.below(12);
    const size_t n = 1 + rng.below(96);
    // versions near 0 and near 2^32 so that the uint32 wrap of ChunkVer is walked too
    const uint32_t origin = rng.below(4) == 0 ? 0xFFFFFFFCu : rng.below(3);
    std::map<uint32_t, RefMeta> ref;
    std::vector<VerState> now(n_chunks);
    for (uint32_t c = 0; c < n_chunks; ++c) {
      RefMeta m{};
      m.chainVer = 1 + rng.below(4);
      m.updateVer = origin + rng.below(4);
      m.commitVer = m.updateVer - rng.below(3);
      m.chunkSize = rng.below(12) ? max_len : max_len / 2;
      m.chunkState = (int)rng.below(3);
      m.recycleState = rng.below(8) ? 0 : 1 + (int)rng.below(2);
      ref[c] = m;
      now[c] = VerState{m.chainVer, m.updateVer, m.commitVer, m.chunkSize, (uint8_t)m.chunkState,
                        (uint8_t)m.recycleState};
    }
    for (size_t i = 0; i < n; ++i) {
      Job j{};
      j.chunk = rng.below(n_chunks);
      const VerState before = now[j.chunk];
      const uint32_t kind = rng.below(16);
      static const uint8_t kTypes[4] = {HF3FS_UPDATE_WRITE, HF3FS_UPDATE_TRUNCATE, HF3FS_UPDATE_EXTEND,
                                        HF3FS_UPDATE_COMMIT};
      j.update_type = kTypes[kind < 9 ? 0 : kind < 10 ? 1 : kind < 11 ? 2 : 3];
      j.flags = (uint8_t)((rng.below(16) == 0 ? HF3FS_UPDATE_FLAG_ENGINE : 0) |
                          (rng.below(8) == 0 ? HF3FS_UPDATE_FLAG_SYNCING : 0));
      j.job_chain_ver = 1 + rng.below(5);
      j.io_ver = rng.below(5) == 0 ? 0u : before.update_ver + rng.below(4) - 1u;
      if (j.update_type == HF3FS_UPDATE_COMMIT) j.io_ver = before.update_ver + rng.below(3) - 1u;
      j.is_force = rng.below(6) == 0;
      j.record_ok = rng.below(16) != 0;
      j.verify = j.update_type == HF3FS_UPDATE_WRITE && rng.below(8) != 0;
      j.payload_bad = rng.below(5) == 0;
      if (before.update_ver + 1u == 0u || j.io_ver - 1u == 0xFFFFFFFFu) ++wraps;

      RefMeta& meta = ref[j.chunk];
      const bool commit = j.update_type == HF3FS_UPDATE_COMMIT;
      const int want = commit ? ref_commit(meta, j) : ref_update(meta, j, max_len);

      const VerVerdict v = commit ? commit_ladder(before, j.io_ver, j.job_chain_ver, j.flags, j.is_force)
                                  : update_ladder(before, j.io_ver, j.job_chain_ver, j.flags, j.record_ok, max_len);
      int got = v.status;
      VerState after = before;
      if (commit) {
        CHECK(v.where == kVerCommit);
        if (got == HF3FS_CRC_OK) after = v.next;
      } else if (v.where == kVerAdmit) {
        CHECK(got == HF3FS_CRC_OK);
        got = j.verify && j.payload_bad ? HF3FS_CRC_CHECKSUM_MISMATCH : HF3FS_CRC_OK;  // the pipeline's verdict
        if (got == HF3FS_CRC_OK) after = v.next;
      } else if (v.where == kVerLate) {
        CHECK(got != HF3FS_CRC_OK);
        ++deferred;
        if (j.verify && j.payload_bad) got = HF3FS_CRC_CHECKSUM_MISMATCH;  // the settle kernel's choice
      } else {
        CHECK(v.where == kVerEarly && got != HF3FS_CRC_OK);
      }
      if (v.status != HF3FS_CRC_OK) {  // every refusal hands the before-state on
        const VerState& x = v.next;
        CHECK(x.chain_ver == before.chain_ver && x.update_ver == before.update_ver &&
              x.commit_ver == before.commit_ver && x.meta_chunk_size == before.meta_chunk_size &&
              x.chunk_state == before.chunk_state && x.recycle_state == before.recycle_state);
      }
      CHECK(got == want);
      CHECK(same(after, meta));
      now[j.chunk] = after;
      (commit ? commit_codes : update_codes).insert(got);
      ++jobs_run;
    }
  }
  printf("{\"fuzz_version_ladder\": \"ok\", \"queues\": %d, \"jobs\": %llu, \"deferred\": %llu, \"wraps\": %llu, "
         "\"update_codes\": %zu, \"commit_codes\": %zu}\n",
         queues, (unsigned long long)jobs_run, (unsigned long long)deferred, (unsigned long long)wraps,
         update_codes.size(), commit_codes.size());
  return 0;
}
