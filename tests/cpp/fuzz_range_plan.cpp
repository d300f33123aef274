// fuzz_range_plan.cpp -- 3fs_amd/csrc/range_plan.h, the header the kernels of range_kernels.hip
// include, against restatements of the reference's loops.  A stand-alone program: g++ with
// -fsanitize=address,undefined, no GPU, no Python.
//
// range_query: random tables (strictly ascending ids over a few id_hi values, recycle states 0-2,
// lengths up to 2^32 - 1), random ranges at ids, their neighbours and gaps, limits around the span's
// size, page sizes 1..1000.  The restatement is the paged loop itself: queryChunks
// (ChunkStore.cc:120-147) as a descending walk with its three tests, processQueryResults
// (StorageOperator.cc:653-751) with its page arithmetic, queryLastChunk's processor (:875-891) and
// removeChunks' (:949-971).  Every op is run at two page sizes; op outputs, the list segments (through
// range_list_entry, entry by entry) and list_first must be equal.
// file_length: random files over random finished ops with duplicate chain ids and length ties; the
// restatement is queryChunksByChain (FileOperation.cc:127-176) with a std::map and queryChunks' fold
// (:45-76).
// Prints one JSON line with the branches reached; the test fails if one stays at zero.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../3fs_amd/csrc/range_plan.h"

using namespace hf3fs_crc;

static std::map<std::string, uint64_t> g_branch;
#define HIT(name) (++g_branch[name])

struct Id {
  uint64_t hi, lo;
  bool operator<(const Id& o) const { return hi < o.hi || (hi == o.hi && lo < o.lo); }
  bool operator==(const Id& o) const { return hi == o.hi && lo == o.lo; }
};

static int die(const char* what, uint64_t a, uint64_t b) {
  fprintf(stderr, "MISMATCH %s: %llu vs %llu\n", what, (unsigned long long)a, (unsigned long long)b);
  exit(1);
}
#define SAME(what, a, b) ((uint64_t)(a) == (uint64_t)(b) ? 0 : die(what, (uint64_t)(a), (uint64_t)(b)))

// ---- the reference's storage side, restated ----
using Table = std::vector<hf3fs_crc_sync_meta>;

// ChunkStore::queryChunks: the iterator seeks to `end` and descends.
static std::vector<uint32_t> query_chunks(const Table& t, Id begin, Id end, uint32_t max_num) {
  std::vector<uint32_t> out;
  int64_t it = (int64_t)t.size() - 1;
  while (it >= 0 && end < Id{t[it].id_hi, t[it].id_lo}) --it;  // metaStore_.iterator(end)
  for (; it >= 0 && out.size() < max_num; --it) {              // :128
    const Id id{t[it].id_hi, t[it].id_lo};
    if (id == end) continue;  // :132
    if (id < begin) break;    // :136
    out.push_back((uint32_t)it);
  }
  return out;
}

struct Walk {
  std::vector<uint32_t> processed;  // table indices, in processing order
  bool more = false;
  uint32_t pages = 0;
};

static Walk process_query_results(const Table& t, Id begin, Id end, uint32_t max_chunks, uint32_t page) {
  Walk w;
  const uint32_t num_to_process = max_chunks ? std::min(max_chunks, UINT32_MAX - 1) : (UINT32_MAX - 1);  // :658
  Id current_end = end;
  uint32_t num_results = 0;
  while (true) {
    const uint32_t current_max = std::min(num_to_process - num_results + 1, page);  // :667
    const std::vector<uint32_t> result = query_chunks(t, begin, current_end, current_max);
    ++w.pages;
    bool done = false;
    for (uint32_t index : result) {
      if (t[index].recycle_state != 0) continue;                           // :677-696
      if (num_results < num_to_process) w.processed.push_back(index);     // :698
      num_results++;
      if (num_results >= num_to_process + 1) {                             // :709
        done = true;
        break;
      }
    }
    if (done || result.size() < current_max) break;                        // :719
    current_end = Id{t[result.back()].id_hi, t[result.back()].id_lo};      // :728
  }
  w.more = num_results > num_to_process;                                    // :743
  SAME("processed count", w.processed.size(), std::min(num_results, num_to_process));
  return w;
}

struct Prefix {
  std::vector<uint32_t> cnt;
  std::vector<uint64_t> len;
};
static Prefix prefixes(const Table& t) {
  Prefix p;
  p.cnt.assign(t.size() + 1, 0);
  p.len.assign(t.size() + 1, 0);
  for (size_t i = 0; i < t.size(); ++i) {
    const bool normal = t[i].recycle_state == 0;
    p.cnt[i + 1] = p.cnt[i] + (normal ? 1u : 0u);
    p.len[i + 1] = p.len[i] + (normal ? t[i].length : 0u);
  }
  return p;
}

static void fuzz_range(std::mt19937_64& rng, uint64_t rounds) {
  for (uint64_t round = 0; round < rounds; ++round) {
    const uint32_t n = round % 13 == 0 ? (uint32_t)(rng() % 3) : (uint32_t)(1 + rng() % 60);
    Table t(n);
    Id id{rng() % 2, rng() % 3};
    const bool big_len = rng() % 4 == 0;
    for (uint32_t i = 0; i < n; ++i) {
      memset(&t[i], 0, sizeof(t[i]));
      t[i].id_hi = id.hi;
      t[i].id_lo = id.lo;
      t[i].length = big_len ? (uint32_t)(0xFFFFFF00u + rng() % 256) : (uint32_t)(rng() % 5000);
      t[i].recycle_state = rng() % 4 == 0 ? (uint8_t)(1 + rng() % 2) : 0;
      if (rng() % 9 == 0) {  // the next id differs in id_hi, id_lo anywhere (also 0 and 2^64 - 1)
        id.hi += 1 + rng() % 2;
        id.lo = rng() % 3 == 0 ? 0 : (rng() % 3 == 0 ? ~0ull : rng());
      } else {
        const uint64_t step = 1 + rng() % 3;
        if (id.lo > ~0ull - step) {
          ++id.hi;
          id.lo = rng() % 2;
        } else {
          id.lo += step;
        }
      }
    }
    bool unsorted = false;
    if (n >= 2 && round % 11 == 3) {  // one duplicate or one inversion
      const uint32_t k = 1 + (uint32_t)(rng() % (n - 1));
      if (rng() % 2) {
        t[k].id_hi = t[k - 1].id_hi;
        t[k].id_lo = t[k - 1].id_lo;
      } else {
        std::swap(t[k], t[k - 1]);
      }
      unsorted = true;
    }
    uint32_t breaks = 0;
    for (uint32_t i = 1; i < n; ++i)
      breaks += range_id_less(t[i - 1].id_hi, t[i - 1].id_lo, t[i].id_hi, t[i].id_lo) ? 0 : 1;
    SAME("unsorted", breaks != 0, unsorted);
    const Prefix p = prefixes(t);

    const uint32_t n_ops = 1 + (uint32_t)(rng() % 12);
    std::vector<hf3fs_crc_range_op> ops(n_ops);
    std::vector<RangeOpPlan> plans(n_ops);
    std::vector<uint64_t> off(n_ops + 1, 0);
    std::vector<uint32_t> want_list;
    for (uint32_t k = 0; k < n_ops; ++k) {
      hf3fs_crc_range_op& op = ops[k];
      memset(&op, 0xA5, sizeof(op));
      auto pick = [&]() {
        Id x{rng() % 4, rng()};
        if (n && rng() % 8) {
          const hf3fs_crc_sync_meta& m = t[rng() % n];
          x = Id{m.id_hi, m.id_lo};
          const uint64_t nudge = rng() % 3;  // the id, its upper neighbour, its lower neighbour
          if (nudge == 1) {
            if (++x.lo == 0) ++x.hi;
          } else if (nudge == 2) {
            if (x.lo)
              --x.lo;
            else if (x.hi)
              --x.hi, x.lo = ~0ull;
          }
        }
        return x;
      };
      Id begin = pick(), end = pick();
      if (end < begin && rng() % 4) std::swap(begin, end);
      op.begin_hi = begin.hi, op.begin_lo = begin.lo, op.end_hi = end.hi, op.end_lo = end.lo;
      op.kind = rng() % 2 ? HF3FS_RANGE_QUERY : HF3FS_RANGE_REMOVE;
      if (rng() % 23 == 0) op.kind = (uint8_t)(rng() % 2 ? 0 : 3 + rng() % 250);
      op.status_in = rng() % 19 == 0 ? (int32_t)(rng() % 2 ? 4032 : -7) : 0;
      op.chain_id = (uint32_t)rng();
      // the span's normal records, to aim the limit
      uint32_t normals = 0;
      bool end_is_record = false, begin_is_record = false;
      for (uint32_t i = 0; i < n; ++i) {
        const Id x{t[i].id_hi, t[i].id_lo};
        if (!(x < begin) && x < end && t[i].recycle_state == 0) ++normals;
        end_is_record |= x == end;
        begin_is_record |= x == begin;
      }
      switch (rng() % 7) {
        case 0: op.max_chunks = 0; break;
        case 1: op.max_chunks = 1; break;
        case 2: op.max_chunks = normals > 1 ? normals - 1 : 1; break;
        case 3: op.max_chunks = normals ? normals : 1; break;
        case 4: op.max_chunks = normals + 1; break;
        case 5: op.max_chunks = UINT32_MAX; break;
        default: op.max_chunks = (uint32_t)(1 + rng() % 8); break;
      }
      const hf3fs_crc_range_op in = op;
      plans[k] = range_op_plan(
          op, unsorted, n,
          [&](uint64_t r, uint64_t hi, uint64_t lo) {
            if (r >= n) die("id probe past the table", r, n);
            return range_id_less(t[r].id_hi, t[r].id_lo, hi, lo);
          },
          [&](uint64_t r) { return r <= n ? p.cnt[r] : (uint32_t)die("cnt probe", r, n); },
          [&](uint64_t r) { return r <= n ? p.len[r] : (uint64_t)die("len probe", r, n); },
          [&](uint64_t r, uint64_t* hi, uint64_t* lo, uint32_t* length) {
            if (r >= n) die("last past the table", r, n);
            *hi = t[r].id_hi, *lo = t[r].id_lo, *length = t[r].length;
          });
      op.list_first = range_list_first(off[k]);
      off[k + 1] = off[k] + plans[k].list_n;
      if (memcmp(&in, &op, offsetof(hf3fs_crc_range_op, last_hi)) != 0) die("an input field changed", k, 0);

      // the reference
      hf3fs_crc_range_op want = in;
      want.last_hi = want.last_lo = want.total_len = 0;
      want.total_chunks = want.last_len = 0;
      want.last_index = kRangeNone;
      want.more = 0;
      memset(want.reserved1, 0, 3);
      want.list_first = range_list_first(want_list.size());
      if (unsorted) {
        want.status = 3;
        HIT("r_unsorted");
      } else if (in.status_in) {
        want.status = in.status_in;
        HIT("r_status_in");
      } else if (in.kind != HF3FS_RANGE_QUERY && in.kind != HF3FS_RANGE_REMOVE) {
        want.status = 3;
        HIT("r_bad_kind");
      } else {
        want.status = 0;
        const uint32_t pages[2] = {(uint32_t)(1 + rng() % 4), (uint32_t)(rng() % 2 ? 1000 : 1 + rng() % 40)};
        Walk w[2] = {process_query_results(t, begin, end, in.max_chunks, pages[0]),
                     process_query_results(t, begin, end, in.max_chunks, pages[1])};
        if (w[0].processed != w[1].processed || w[0].more != w[1].more) die("the page size changed the walk", k, 0);
        if (w[0].pages > 2) HIT("r_several_pages");
        if (pages[0] == 1) HIT("r_page_of_one");
        // queryLastChunk's processor
        bool have = false;
        Id last{0, 0};
        for (uint32_t index : w[0].processed) {
          const Id x{t[index].id_hi, t[index].id_lo};
          if (!have || last < x) {
            last = x, want.last_len = t[index].length, want.last_index = index;
            have = true;
          }
          want.total_len += t[index].length;
          want.total_chunks++;
        }
        want.last_hi = last.hi, want.last_lo = last.lo;
        want.more = w[0].more;
        if (in.kind == HF3FS_RANGE_REMOVE) {
          want_list.insert(want_list.end(), w[0].processed.begin(), w[0].processed.end());
          HIT("r_remove");
        } else {
          HIT("r_query");
        }
        if (!(begin < end)) HIT(begin == end ? "r_begin_equals_end" : "r_begin_above_end");
        else if (normals == 0) HIT("r_no_normal_record");
        if (begin < end && end_is_record) HIT("r_end_is_a_record");
        if (begin < end && begin_is_record) HIT("r_begin_is_a_record");
        if (in.max_chunks == 0) HIT("r_unlimited");
        if (want.more) HIT("r_more");
        if (in.max_chunks && normals == in.max_chunks && normals) HIT("r_limit_equals_normals");
        if (in.max_chunks == UINT32_MAX) HIT("r_limit_clamped");
        if (want.total_len >> 32) HIT("r_total_len_past_32_bits");
        if (want.total_chunks && want.total_chunks < normals && want.total_chunks > 1) HIT("r_lowest_processed_by_rank");
      }
      if (memcmp(&want, &op, sizeof(op)) != 0) {
        fprintf(stderr, "op %u: status %d/%d chunks %u/%u len %llu/%llu last %u/%u more %u/%u first %u/%u\n", k,
                op.status, want.status, op.total_chunks, want.total_chunks, (unsigned long long)op.total_len,
                (unsigned long long)want.total_len, op.last_index, want.last_index, op.more, want.more, op.list_first,
                want.list_first);
        die("op record", k, round);
      }
    }
    SAME("list length", off[n_ops], want_list.size());
    for (uint64_t e = 0; e < want_list.size(); ++e) {
      const uint32_t got = range_list_entry(
          e, n_ops, n, [&](uint64_t j) { return j <= n_ops ? off[j] : (uint64_t)die("off probe", j, n_ops); },
          [&](uint64_t j) { return j < n_ops ? plans[j].top : (uint32_t)die("top probe", j, n_ops); },
          [&](uint64_t r) { return r <= n ? p.cnt[r] : (uint32_t)die("cnt probe", r, n); });
      SAME("list entry", got, want_list[e]);
    }
    if (want_list.size() > 1) HIT("r_list");
  }
  if (range_list_first(0xFFFFFFFFull) != kRangeNone || range_list_first(0xFFFFFFFEull) != 0xFFFFFFFEu ||
      range_list_first(1ull << 40) != kRangeNone)
    die("list_first saturation", 0, 0);
  HIT("r_list_first_saturates");
}

// ---- the reference's meta side, restated ----
struct QueryResult {
  uint64_t length = 0, lastChunk = 0, lastChunkLen = 0, totalChunkLen = 0, totalNumChunks = 0;
};

static void fuzz_files(std::mt19937_64& rng, uint64_t rounds) {
  for (uint64_t round = 0; round < rounds; ++round) {
    const uint32_t n_ops = (uint32_t)(rng() % 24);
    const uint64_t inode = rng() % 3 ? 0x123456789ABCull + rng() % 2 : rng();
    const uint32_t chunk_size = rng() % 3 ? 4096 : (uint32_t)rng();
    std::vector<hf3fs_crc_range_op> ops(n_ops);
    for (auto& op : ops) {
      memset(&op, 0, sizeof(op));
      op.chain_id = (uint32_t)(rng() % 6);  // duplicates
      const uint64_t ino = rng() % 15 ? inode : inode ^ (1ull << (rng() % 64));
      const uint32_t chunk = (uint32_t)(rng() % 5);
      op.last_hi = ino >> 16;
      op.last_lo = (ino & 0xFFFF) << 48 | chunk;
      if (rng() % 40 == 0) op.last_hi = 0x0000FFFFFFFFFFFFull, op.last_lo = 0xFFFF000000000000ull;
      // lengths that tie: (c, chunk_size) against (c + 1, 0)
      op.last_len = rng() % 3 == 0 ? chunk_size : (rng() % 2 ? 0 : (uint32_t)(rng() % 100));
      op.total_chunks = rng() % 6 ? (uint32_t)(1 + rng() % 9) : 0;
      op.total_len = rng();
      op.status = rng() % 7 == 0 ? kRangeChunkNotFound : (rng() % 25 == 0 ? (int32_t)(rng() % 2 ? 4032 : -3) : 0);
    }
    hf3fs_crc_file_len f;
    memset(&f, 0x5A, sizeof(f));
    f.inode = inode;
    f.first_op = n_ops ? (uint32_t)(rng() % n_ops) : 0;
    f.n_file_ops = (uint32_t)(rng() % (n_ops - f.first_op + 1));
    if (rng() % 30 == 0) f.n_file_ops = n_ops - f.first_op + 1 + (uint32_t)(rng() % 3);
    if (rng() % 40 == 0) f.n_file_ops = 1025 + (uint32_t)(rng() % 5);
    f.chunk_size = chunk_size;
    f.stripe_size = rng() % 2 ? f.n_file_ops : f.n_file_ops + 1 + (uint32_t)(rng() % 4);
    f.flags = (uint8_t)(rng() % 2);
    const hf3fs_crc_file_len in = f;
    const RangeFileCounts c = range_file_fold(
        f, n_ops, [&](uint64_t i) { return i < n_ops ? ops[i] : (die("op probe", i, n_ops), ops[0]); },
        [&](uint64_t i) { return i < n_ops ? ops[i].chain_id : (uint32_t)die("chain probe", i, n_ops); });
    if (memcmp(&in, &f, offsetof(hf3fs_crc_file_len, status)) != 0) die("a file input changed", round, 0);

    hf3fs_crc_file_len want = in;
    want.status = 0;
    want.length = want.total_len = want.total_chunks = 0;
    want.last_chunk = want.last_chunk_len = 0;
    uint32_t not_found = 0;
    bool empty = false;
    if (in.n_file_ops > 1024) {
      want.status = 3;
      HIT("f_too_many_ops");
    } else if ((uint64_t)in.first_op + in.n_file_ops > n_ops) {
      want.status = 3;
      HIT("f_segment_past_the_ops");
    } else {
      // queryChunksByChain :127-176
      std::map<uint32_t, QueryResult> chunks;
      const uint32_t maxStripe = in.n_file_ops;
      for (uint32_t q = in.first_op; q < in.first_op + maxStripe && want.status == 0; ++q) {
        const hf3fs_crc_range_op& result = ops[q];
        if (result.status != 0) {
          if (result.status == 7007) {
            ++not_found;
            HIT("f_not_found_skipped");
            continue;
          }
          want.status = result.status;
          HIT("f_op_status");
          break;
        }
        if (result.total_chunks == 0) {
          HIT("f_no_chunks_skipped");
          continue;
        }
        const bool invalid = result.last_hi == 0x0000FFFFFFFFFFFFull && result.last_lo == 0xFFFF000000000000ull;
        const uint64_t ino = (result.last_hi & 0xFFFFFFFFFFFFull) << 16 | result.last_lo >> 48;
        const uint64_t chunk = result.last_lo & 0xFFFFFFFFull;
        if (invalid) {
          want.status = 2;
          HIT("f_invalid_id");
          break;
        }
        if (ino != in.inode) {
          want.status = 2;
          HIT("f_inode_mismatch");
          break;
        }
        if ((in.flags & HF3FS_FILE_LEN_DYN) && maxStripe < in.stripe_size && chunk >= maxStripe) {
          want.status = 3019;
          HIT("f_busy");
          break;
        }
        if ((in.flags & HF3FS_FILE_LEN_DYN) && maxStripe < in.stripe_size) HIT("f_dyn_below_stripe");
        if (chunks.count(result.chain_id)) HIT("f_chain_replaced");
        chunks[result.chain_id] = QueryResult{chunk * in.chunk_size + result.last_len, chunk, result.last_len,
                                              result.total_len, result.total_chunks};
      }
      if (want.status == 0) {
        // queryChunks :45-76
        QueryResult r;
        for (auto iter = chunks.begin(); iter != chunks.end(); iter++) {
          const QueryResult& cr = iter->second;
          if (iter != chunks.begin() && r.length == cr.length) HIT("f_length_tie");
          if (iter == chunks.begin() || r.length < cr.length) {
            if (iter != chunks.begin()) HIT("f_later_chain_wins");
            r.length = cr.length, r.lastChunk = cr.lastChunk, r.lastChunkLen = cr.lastChunkLen;
          }
          r.totalChunkLen += cr.totalChunkLen;
          r.totalNumChunks += cr.totalNumChunks;
        }
        if (r.lastChunk * in.chunk_size + r.lastChunkLen != r.length) die("kFoundBug", round, 0);
        want.length = r.length, want.total_len = r.totalChunkLen, want.total_chunks = r.totalNumChunks;
        want.last_chunk = (uint32_t)r.lastChunk, want.last_chunk_len = (uint32_t)r.lastChunkLen;
        empty = chunks.empty();
        HIT(empty ? "f_no_entry" : "f_ok");
      }
    }
    if (memcmp(&want, &f, sizeof(f)) != 0) {
      fprintf(stderr, "file: status %d/%d length %llu/%llu chunks %llu/%llu last %u/%u\n", f.status, want.status,
              (unsigned long long)f.length, (unsigned long long)want.length, (unsigned long long)f.total_chunks,
              (unsigned long long)want.total_chunks, f.last_chunk, want.last_chunk);
      die("file record", round, 0);
    }
    SAME("not found", c.not_found, not_found);
    SAME("empty", c.empty, empty);
  }
}

int main(int argc, char** argv) {
  const uint64_t rounds = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000;
  std::mt19937_64 rng(0x52414E4745ull);
  fuzz_range(rng, rounds);
  fuzz_files(rng, rounds * 4);
  printf("{\"fuzz_range_plan\": \"ok\", \"rounds\": %llu, \"branches\": {", (unsigned long long)rounds);
  bool first = true;
  for (const auto& [name, count] : g_branch) {
    printf("%s\"%s\": %llu", first ? "" : ", ", name.c_str(), (unsigned long long)count);
    first = false;
  }
  printf("}}\n");
  return 0;
}
