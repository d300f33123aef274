// fuzz_sync_plan.cpp -- 3fs_amd/csrc/sync_plan.h against the reference's loop, on the CPU.
//
// For random pairs of tables (duplicate ids in both, ids equal in one half only, every rung of the
// ladder, fatal rows) two computations must agree in every class, peer, d_info word and list:
//   (a) a sequential restatement shaped like ResyncWorker::handleSync (src/storage/sync/
//       ResyncWorker.cc:199-303): an unordered_map of the local records, a walk over the remote
//       records that erases what it visits, nested ifs, break.  It uses nothing of sync_plan.h
//       but the constants.
//   (b) the order-free form the kernels of sync_kernels.hip use: a linear-probing table on
//       sync_hash where equal ids resolve to the lowest index, claims by minimum remote index,
//       sync_classify per record, a histogram of classes, sync_info, lists by ascending scan.
//       Inserts and claims run in a shuffled order: the result may not depend on it.
// Usage:  fuzz_sync_plan [rounds]                      the fuzz; prints one JSON line
//         fuzz_sync_plan --time local remote cv flags   times (a) on two files of raw 48-byte records
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../3fs_amd/csrc/sync_plan.h"

using namespace hf3fs_crc;
using Meta = hf3fs_crc_sync_meta;
static_assert(sizeof(Meta) == 48, "hf3fs_crc_sync_meta layout");

struct Id {
  uint64_t hi, lo;
  bool operator==(const Id& o) const { return hi == o.hi && lo == o.lo; }
};
struct IdHash {
  size_t operator()(const Id& k) const { return std::hash<uint64_t>()(k.hi * 0x100000001B3ull ^ k.lo); }
};

struct Result {
  std::vector<uint8_t> lclass, rclass;
  std::vector<uint32_t> lpeer, rpeer, write, remove;
  uint32_t info[HF3FS_SYNC_INFO_WORDS] = {};
};

// ---- (a) the reference's shape -------------------------------------------------------------------
struct Walk {
  uint32_t cnt[HF3FS_SYNC_INFO_WORDS] = {};
  std::vector<uint32_t> write, remove;
  std::unordered_map<Id, uint32_t, IdHash> left;
  uint32_t first_fatal = kSyncNone;
};

static Walk walk(const std::vector<Meta>& local, const std::vector<Meta>& remote, uint32_t chain_ver, bool heavy,
                 bool stop, std::vector<uint8_t>* rclass, std::vector<uint32_t>* rpeer) {
  Walk w;
  w.left.reserve(local.size());
  for (uint32_t i = 0; i < local.size(); ++i) w.left.emplace(Id{local[i].id_hi, local[i].id_lo}, i);  // first wins
  for (uint32_t r = 0; r < remote.size(); ++r) {
    const Meta& remoteMeta = remote[r];
    auto it = w.left.find(Id{remoteMeta.id_hi, remoteMeta.id_lo});
    if (it == w.left.end()) {
      w.remove.push_back(r);
      if (rclass) (*rclass)[r] = HF3FS_SYNC_REMOTE_ONLY;
      continue;
    }
    const uint32_t i = it->second;
    const Meta& meta = local[i];
    w.left.erase(it);
    if (rpeer) (*rpeer)[r] = i;
    uint8_t cls;
    if (meta.recycle_state != 0) {
      ++w.cnt[HF3FS_SYNC_INFO_RECYCLE];
      if (rclass) (*rclass)[r] = HF3FS_SYNC_LOCAL_RECYCLING;
      continue;
    }
    bool needForward = true, fatal = false;
    if (meta.chain_ver > remoteMeta.chain_ver) {
      ++w.cnt[HF3FS_SYNC_INFO_CHAIN_VER_LOW];
      cls = HF3FS_SYNC_CHAIN_VER_LOW;
    } else if (remoteMeta.update_ver != remoteMeta.commit_ver || remoteMeta.chunk_state != 0) {
      ++w.cnt[HF3FS_SYNC_INFO_REMOTE_UNCOMMITTED];
      cls = HF3FS_SYNC_REMOTE_UNCOMMITTED;
    } else if (meta.chain_ver < remoteMeta.chain_ver) {
      if (meta.chunk_state == 0) {
        ++w.cnt[HF3FS_SYNC_INFO_CHAIN_VER_HIGH];
        cls = HF3FS_SYNC_REMOTE_CHAIN_VER_HIGH;
        fatal = true;
      } else {
        needForward = false;
        ++w.cnt[HF3FS_SYNC_INFO_LOCAL_UNCOMMITTED];
        cls = HF3FS_SYNC_LOCAL_UNCOMMITTED;
      }
    } else if (meta.update_ver != remoteMeta.commit_ver) {
      if (meta.chain_ver != chain_ver && meta.chunk_state == 0) {
        ++w.cnt[HF3FS_SYNC_INFO_COMMIT_VER_MISMATCH];
        cls = HF3FS_SYNC_COMMIT_VER_MISMATCH;
        fatal = true;
      } else {
        needForward = false;
        ++w.cnt[HF3FS_SYNC_INFO_CHAIN_WRITING];
        cls = HF3FS_SYNC_CHAIN_WRITING;
      }
    } else if (heavy) {
      ++w.cnt[HF3FS_SYNC_INFO_FULL_SYNC_HEAVY];
      cls = HF3FS_SYNC_FULL_SYNC_HEAVY;
    } else if (!(meta.checksum_type == remoteMeta.checksum_type && meta.checksum == remoteMeta.checksum)) {
      if (meta.chain_ver != chain_ver) {
        ++w.cnt[HF3FS_SYNC_INFO_FULL_SYNC_LIGHT];
        cls = HF3FS_SYNC_CHECKSUM_MISMATCH;
        fatal = true;
      } else {
        needForward = false;
        ++w.cnt[HF3FS_SYNC_INFO_CHAIN_WRITING];
        cls = HF3FS_SYNC_CHAIN_WRITING_CHECKSUM;
      }
    } else {
      needForward = false;
      cls = HF3FS_SYNC_EQUAL;
    }
    if (rclass) (*rclass)[r] = cls;
    if (fatal) {
      if (w.first_fatal == kSyncNone) w.first_fatal = r;
      if (stop) break;
      continue;
    }
    if (needForward)
      w.write.push_back(i);
    else
      ++w.cnt[HF3FS_SYNC_INFO_SKIP];
  }
  return w;
}

// What the reference's loop leaves: counters and lists with the break; with `classes`, also every
// record's own class from a second walk that does not stop.
static Result sequential(const std::vector<Meta>& local, const std::vector<Meta>& remote, uint32_t chain_ver,
                         uint32_t flags, bool classes) {
  const bool heavy = (flags & HF3FS_SYNC_HEAVY) != 0;
  Result out;
  Walk w = walk(local, remote, chain_ver, heavy, true, nullptr, nullptr);
  memcpy(out.info, w.cnt, sizeof(out.info));
  out.info[HF3FS_SYNC_INFO_FIRST_FATAL] = w.first_fatal;
  if (w.first_fatal != kSyncNone) {
    out.info[HF3FS_SYNC_INFO_FATAL] = 1;
  } else {
    for (const auto& kv : w.left) {
      w.write.push_back(kv.second);
      ++out.info[HF3FS_SYNC_INFO_REMOTE_MISS];
    }
    std::sort(w.write.begin(), w.write.end());
    out.info[HF3FS_SYNC_INFO_N_WRITE] = (uint32_t)w.write.size();
    out.info[HF3FS_SYNC_INFO_N_REMOVE] = (uint32_t)w.remove.size();
    out.write = std::move(w.write);
    out.remove = std::move(w.remove);
  }
  if (classes) {
    out.rclass.assign(remote.size(), 0);
    out.rpeer.assign(remote.size(), kSyncNone);
    const Walk all = walk(local, remote, chain_ver, heavy, false, &out.rclass, &out.rpeer);
    out.lclass.assign(local.size(), HF3FS_SYNC_DUPLICATE);
    out.lpeer.assign(local.size(), kSyncNone);
    for (uint32_t r = 0; r < remote.size(); ++r)
      if (out.rpeer[r] != kSyncNone) {
        out.lclass[out.rpeer[r]] = HF3FS_SYNC_MATCHED;
        out.lpeer[out.rpeer[r]] = r;
      }
    for (const auto& kv : all.left) out.lclass[kv.second] = HF3FS_SYNC_REMOTE_MISS;
    for (uint8_t c : out.lclass) out.info[HF3FS_SYNC_INFO_DUPLICATES] += c == HF3FS_SYNC_DUPLICATE;
  }
  return out;
}

// ---- (b) the kernels' shape ----------------------------------------------------------------------
static uint32_t find(const std::vector<Meta>& local, const std::vector<uint32_t>& table, uint64_t hi, uint64_t lo) {
  const uint32_t slots = (uint32_t)table.size(), mask = slots - 1;
  uint32_t h = sync_hash(hi, lo, mask);
  for (uint32_t probe = 0; probe < slots; ++probe, h = (h + 1) & mask) {
    const uint32_t j = table[h];
    if (j == kSyncNone) return kSyncNone;
    if (local[j].id_hi == hi && local[j].id_lo == lo) return j;
  }
  return kSyncNone;
}

static Result order_free(const std::vector<Meta>& local, const std::vector<Meta>& remote, uint32_t chain_ver,
                         uint32_t flags, std::mt19937_64& rng) {
  const uint32_t nl = (uint32_t)local.size(), nr = (uint32_t)remote.size();
  uint32_t slots = 2;
  while (slots < 2 * (uint64_t)nl) slots <<= 1;
  const uint32_t mask = slots - 1;
  std::vector<uint32_t> table(slots, kSyncNone), claim(nl, kSyncNone), rfound(nr), order(nl);
  for (uint32_t i = 0; i < nl; ++i) order[i] = i;
  std::shuffle(order.begin(), order.end(), rng);
  for (uint32_t i : order) {  // k_sync_insert
    uint32_t h = sync_hash(local[i].id_hi, local[i].id_lo, mask);
    bool placed = false;
    for (uint32_t probe = 0; probe < slots && !placed; ++probe, h = (h + 1) & mask) {
      if (table[h] == kSyncNone) {
        table[h] = i;
        placed = true;
      } else if (local[table[h]].id_hi == local[i].id_hi && local[table[h]].id_lo == local[i].id_lo) {
        table[h] = std::min(table[h], i);
        placed = true;
      }
    }
    if (!placed) {
      fprintf(stderr, "insert: probe sequence of record %u did not end\n", i);
      exit(1);
    }
  }
  order.resize(nr);
  for (uint32_t r = 0; r < nr; ++r) order[r] = r;
  std::shuffle(order.begin(), order.end(), rng);
  for (uint32_t r : order) {  // k_sync_claim
    rfound[r] = find(local, table, remote[r].id_hi, remote[r].id_lo);
    if (rfound[r] != kSyncNone) claim[rfound[r]] = std::min(claim[rfound[r]], r);
  }
  Result out;
  out.lclass.assign(nl, 0);
  out.rclass.assign(nr, 0);
  out.lpeer.assign(nl, kSyncNone);
  out.rpeer.assign(nr, kSyncNone);
  std::vector<uint8_t> forwards(nl, 0);
  uint32_t first_fatal = kSyncNone;
  for (uint32_t r = 0; r < nr; ++r) {  // k_sync_classify, remote loop
    const uint32_t at = rfound[r];
    const bool mine = at != kSyncNone && claim[at] == r;
    const uint8_t cls = sync_classify(mine ? &local[at] : nullptr, remote[r], chain_ver, flags);
    out.rclass[r] = cls;
    out.rpeer[r] = mine ? at : kSyncNone;
    if (mine) forwards[at] = sync_disposition(cls) == kSyncForward;
    if (sync_disposition(cls) == kSyncFatal) first_fatal = std::min(first_fatal, r);
  }
  for (uint32_t i = 0; i < nl; ++i) {  // local loop
    const uint32_t first = find(local, table, local[i].id_hi, local[i].id_lo);
    out.lclass[i] = first != i ? HF3FS_SYNC_DUPLICATE : claim[i] == kSyncNone ? HF3FS_SYNC_REMOTE_MISS : HF3FS_SYNC_MATCHED;
    if (out.lclass[i] == HF3FS_SYNC_MATCHED) out.lpeer[i] = claim[i];
  }
  uint32_t hist[32] = {}, fwd = 0;  // k_sync_count
  for (uint32_t r = 0; r < nr; ++r)
    if (r <= first_fatal) ++hist[out.rclass[r] & 31];
  for (uint32_t i = 0; i < nl; ++i) {
    ++hist[out.lclass[i] & 31];
    fwd += out.lclass[i] == HF3FS_SYNC_MATCHED && forwards[i];
  }
  sync_info(hist, fwd, first_fatal, out.info);  // k_sync_scan
  if (first_fatal == kSyncNone) {                // k_sync_scatter
    for (uint32_t i = 0; i < nl; ++i)
      if (out.lclass[i] == HF3FS_SYNC_REMOTE_MISS || (out.lclass[i] == HF3FS_SYNC_MATCHED && forwards[i]))
        out.write.push_back(i);
    for (uint32_t r = 0; r < nr; ++r)
      if (sync_disposition(out.rclass[r]) == kSyncRemove) out.remove.push_back(r);
  }
  return out;
}

// ---- tables --------------------------------------------------------------------------------------
static Meta random_meta(std::mt19937_64& rng, uint32_t pool) {
  Meta m{};
  // few distinct halves: ids repeat inside a table and agree in one half only across records
  m.id_hi = rng() % 4 == 0 ? rng() % 3 : 0x5000 + rng() % 3;
  m.id_lo = rng() % pool;
  if (rng() % 16 == 0) m.id_lo <<= 40;  // (high bits only)
  m.chain_ver = 2 + rng() % 3;
  m.commit_ver = 1 + rng() % 2;
  m.update_ver = m.commit_ver + (rng() % 5 == 0);
  m.checksum = rng() % 3;
  m.checksum_type = 1 + (rng() % 4 == 0);
  m.chunk_state = rng() % 5 < 3 ? 0 : 1 + rng() % 2;
  m.length = (uint32_t)rng();
  m.out_class = 0xA5;
  m.out_peer = 0xA5A5A5A5u;
  return m;
}

static bool same(const Result& a, const Result& b, std::string* why) {
  auto fail = [&](const char* what) {
    *why = what;
    return false;
  };
  if (a.lclass != b.lclass) return fail("local classes");
  if (a.rclass != b.rclass) return fail("remote classes");
  if (a.lpeer != b.lpeer) return fail("local peers");
  if (a.rpeer != b.rpeer) return fail("remote peers");
  if (memcmp(a.info, b.info, sizeof(a.info))) return fail("info words");
  if (a.write != b.write) return fail("write lists");
  if (a.remove != b.remove) return fail("remove lists");
  return true;
}

static std::vector<Meta> read_table(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<Meta> t((size_t)bytes / sizeof(Meta));
  if (!t.empty() && fread(t.data(), sizeof(Meta), t.size(), f) != t.size()) {
    perror(path);
    exit(2);
  }
  fclose(f);
  return t;
}

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "--time")) {
    const std::vector<Meta> local = read_table(argv[2]), remote = read_table(argv[3]);
    const uint32_t cv = (uint32_t)strtoul(argv[4], nullptr, 0), flags = (uint32_t)strtoul(argv[5], nullptr, 0);
    double best = 1e30;
    Result res;
    for (int rep = 0; rep < 3; ++rep) {
      const auto t0 = std::chrono::steady_clock::now();
      res = sequential(local, remote, cv, flags, false);
      best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    printf("{\"host_loop_ms\": %.3f, \"n_local\": %zu, \"n_remote\": %zu, \"fatal\": %u, \"n_write\": %u, "
           "\"n_remove\": %u}\n",
           best, local.size(), remote.size(), res.info[HF3FS_SYNC_INFO_FATAL], res.info[HF3FS_SYNC_INFO_N_WRITE],
           res.info[HF3FS_SYNC_INFO_N_REMOVE]);
    return 0;
  }
  const uint64_t rounds = argc > 1 ? strtoull(argv[1], nullptr, 0) : 2000;
  std::mt19937_64 rng(0x53594E43);
  uint64_t records = 0, fatal_tables = 0, calm_tables = 0, dups = 0, seen_class[32] = {};
  for (uint64_t round = 0; round < rounds; ++round) {
    const uint32_t nl = round % 7 == 0 ? 0 : (uint32_t)(rng() % 300), nr = round % 11 == 0 ? 0 : (uint32_t)(rng() % 300);
    const uint32_t pool = 1 + (uint32_t)(rng() % 400);
    const uint32_t cv = 2 + (uint32_t)(rng() % 3), flags = round % 3 == 0 ? HF3FS_SYNC_HEAVY : 0;
    std::vector<Meta> local(nl), remote(nr);
    for (Meta& m : local) {
      m = random_meta(rng, pool);
      m.recycle_state = rng() % 12 == 0 ? 1 + rng() % 2 : 0;
      m.chunk_size = 1u << 20;
    }
    for (Meta& m : remote) m = random_meta(rng, pool);
    if (round % 2) {  // a calm table: nothing fatal, so that the lists are compared too
      const Result probe = sequential(local, remote, cv, flags, true);
      for (uint32_t r = 0; r < nr; ++r)
        if (sync_disposition(probe.rclass[r]) == kSyncFatal) remote[r].chain_ver = 0;
    }
    const Result a = sequential(local, remote, cv, flags, true);
    const Result b = order_free(local, remote, cv, flags, rng);
    std::string why;
    if (!same(a, b, &why)) {
      fprintf(stderr, "round %llu (%u local, %u remote, chain_ver %u, flags %u): %s differ\n",
              (unsigned long long)round, nl, nr, cv, flags, why.c_str());
      return 1;
    }
    for (uint32_t w = 0; w < HF3FS_SYNC_INFO_WORDS; ++w)
      if (a.info[HF3FS_SYNC_INFO_FATAL] && (w == HF3FS_SYNC_INFO_N_WRITE || w == HF3FS_SYNC_INFO_N_REMOVE) && a.info[w]) {
        fprintf(stderr, "round %llu: a list count after a fatal record\n", (unsigned long long)round);
        return 1;
      }
    records += nl + nr;
    (a.info[HF3FS_SYNC_INFO_FATAL] ? fatal_tables : calm_tables) += 1;
    dups += a.info[HF3FS_SYNC_INFO_DUPLICATES];
    for (uint8_t c : a.rclass) ++seen_class[c & 31];
    for (uint8_t c : a.lclass) ++seen_class[c & 31];
  }
  uint32_t classes = 0;
  for (int c = 1; c < 32; ++c) classes += seen_class[c] != 0;
  printf("{\"fuzz_sync_plan\": \"ok\", \"tables\": %llu, \"records\": %llu, \"fatal_tables\": %llu, "
         "\"calm_tables\": %llu, \"duplicates\": %llu, \"classes_seen\": %u}\n",
         (unsigned long long)rounds, (unsigned long long)records, (unsigned long long)fatal_tables,
         (unsigned long long)calm_tables, (unsigned long long)dups, classes);
  return 0;
}
