// fuzz_client_write.cpp -- 3fs_amd/csrc/client_write_plan.h on the CPU: the per-IO ladder of
// prepare and the order-free summary of writeFile's fold against restatements of the reference's
// loops.
//
// Prepare: for random batches (bad records, own-range failures with wrapping sums, null and
// uncontained buffers with wrapping sums, with and without VERIFY) client_write_class /
// client_write_hashes / client_write_settle, used as the two kernels use them (classes and the
// poison word first, the settle behind it), must give what a restatement of the two loops of
// StorageClientImpl.cc:994-1015 and :889-951 and of :1878-1901 gives.
// Complete: for random files of 0 to 2,000 IOs (every mix of the three types, zero lengths,
// failing statuses, short writes, unknown types, lengths up to 2^32 - 1) four computations must
// agree in every field of the file record:
//   (a) a restatement written here in the shape of FileWrapper.cc:218-248 over
//       ChecksumInfo::combine (Common.h:179-198), counting the branches a file took;
//   (b) client_write_seq_step, the loop of the lane schedule;
//   (c) client_write_sum_of / _join / _finish bracketed as the wave schedule does it: 64
//       contiguous runs summarised left to right, then the ordered tree over the 64 partials;
//   (d) the same summary under a random bracketing, and for files of at most 12 IOs cut in two at
//       every position.
// Usage:  fuzz_client_write [files]     prints one JSON line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../3fs_amd/csrc/client_write_plan.h"

using namespace hf3fs_crc;
using Io = hf3fs_crc_client_write_io;
static_assert(sizeof(Io) == 64, "hf3fs_crc_client_write_io layout");
static_assert(sizeof(hf3fs_crc_client_write_file) == 24, "hf3fs_crc_client_write_file layout");

// x^(8 n) from the squares of x^8: the same value as gf2.h's xpow_bytes (checked in main) at a
// multiply per set bit of n.
struct GfFast {
  uint32_t sq[2][64];
  GfFast() {
    for (int t = 0; t < 2; ++t) {
      const uint32_t poly = t ? kPolyCrc32 : kPolyCrc32c;
      uint32_t b = xpow_bits(8, poly);
      for (int k = 0; k < 64; ++k, b = gf_mul(b, b, poly)) sq[t][k] = b;
    }
  }
  uint32_t shift(uint32_t v, uint64_t nbytes, uint8_t type) const {
    const int t = type == kTypeCrc32 ? 1 : 0;
    const uint32_t poly = poly_of(type);
    for (int k = 0; nbytes; ++k, nbytes >>= 1)
      if (nbytes & 1) v = gf_mul(v, sq[t][k], poly);
    return v;
  }
};

enum Branch {
  kNoIos, kEndStatus, kEndUnknownType, kEndShort, kEndTypeBytes, kEndTypeZeroLength, kEndTypeNone, kZeroLengthPass,
  kForeignZeroInFront, kAdoptTyped, kAdoptNone, kCombineCrc32c, kCombineCrc32, kEndFirst, kEndLast, kClean, kBranches
};
const char* const kBranchName[kBranches] = {
    "no_ios", "end_status", "end_unknown_type", "end_short", "end_type_bytes", "end_type_zero_length", "end_type_none",
    "zero_length_pass", "foreign_zero_in_front", "adopt_typed", "adopt_none", "combine_crc32c", "combine_crc32",
    "end_first", "end_last", "clean"};

// (a)
CwFile reference_loop(const std::vector<CwAnswer>& ios, bool* took) {
  uint8_t type = 0;  // storage::ChecksumInfo checksum;
  uint32_t value = 0;
  uint64_t total = 0;
  if (ios.empty()) took[kNoIos] = true;
  auto ended = [&](int32_t code, size_t k) {
    took[k == 0 ? kEndFirst : kEndLast] |= k == 0 || k + 1 == ios.size();
    CwFile f;
    f.length = 0;
    f.value = 0;
    f.type = 0;
    f.status = code;
    f.failed = (uint32_t)k;
    return f;
  };
  for (size_t k = 0; k < ios.size(); ++k) {
    const CwAnswer& io = ios[k];
    if (io.status != 0) return took[kEndStatus] = true, ended(io.status, k);  // CO_RETURN_AND_LOG_ON_ERROR(lengthInfo)
    if (io.type > 2) return took[kEndUnknownType] = true, ended(3, k);
    const uint32_t succ = io.result_len;
    if (succ != io.length) return took[kEndShort] = true, ended(33, k);
    // checksum.combine(writeIO.result.checksum, succLength)
    if (type != 0 && type != io.type) {
      took[io.type == 0 ? kEndTypeNone : succ == 0 ? kEndTypeZeroLength : kEndTypeBytes] = true;
      return ended(4080, k);
    }
    if (succ == 0) {
      took[kZeroLengthPass] = true;
      if (type == 0 && io.type != 0) took[kForeignZeroInFront] = true;
      continue;
    }
    switch (type) {
      case 0:
        took[io.type == 0 ? kAdoptNone : kAdoptTyped] = true;
        type = io.type;
        value = io.value;
        break;
      case 1:
        took[kCombineCrc32c] = true;
        value = combine_raw(~value, io.value, succ, kPolyCrc32c);
        break;
      case 2:
        took[kCombineCrc32] = true;
        value = combine_raw(~value, io.value, succ, kPolyCrc32);
        break;
    }
    total += succ;
  }
  if (!ios.empty()) took[kClean] = true;
  CwFile f;
  f.length = total;
  f.value = value;
  f.type = type;
  f.status = 0;
  f.failed = ~0u;
  return f;
}

// (b)
template <class Gf>
CwFile plan_loop(const std::vector<CwAnswer>& ios, const Gf& gf) {
  CwFile f = client_write_file_begin();
  for (size_t k = 0; k < ios.size(); ++k)
    if (!client_write_seq_step(f, ios[k], (uint32_t)k, gf)) break;
  return f;
}

template <class Gf>
CwSum run_sum(const std::vector<CwAnswer>& ios, size_t lo, size_t hi, const Gf& gf) {
  CwSum acc = client_write_sum_identity();
  for (size_t j = lo; j < hi; ++j) acc = client_write_sum_join(acc, client_write_sum_of(ios[j], (uint32_t)j), gf);
  return acc;
}

// (c)
template <class Gf>
CwFile wave_fold(const std::vector<CwAnswer>& ios, const Gf& gf) {
  const size_t k = ios.size(), run = (k + 63) / 64;
  CwSum lane[64];
  for (size_t l = 0; l < 64; ++l) {
    const size_t j = l * run, e = j + run < k ? j + run : k;
    lane[l] = run_sum(ios, j < k ? j : k, e > j ? e : (j < k ? j : k), gf);
  }
  for (int d = 1; d < 64; d <<= 1)
    for (int l = 0; l + d < 64; l += 2 * d) lane[l] = client_write_sum_join(lane[l], lane[l + d], gf);
  return client_write_sum_finish(lane[0]);
}

// (d)
template <class Gf>
CwSum random_fold(const std::vector<CwAnswer>& ios, size_t lo, size_t hi, std::mt19937_64& rng, const Gf& gf) {
  if (hi == lo) return client_write_sum_identity();
  if (hi - lo == 1) return client_write_sum_of(ios[lo], (uint32_t)lo);
  size_t mid = lo + (size_t)(rng() % (hi - lo + 1));  // an empty side joins the identity
  if (mid == lo || mid == hi) {
    const CwSum none = client_write_sum_identity();
    const size_t half = lo + (hi - lo) / 2;
    const CwSum all = client_write_sum_join(random_fold(ios, lo, half, rng, gf), random_fold(ios, half, hi, rng, gf), gf);
    return mid == lo ? client_write_sum_join(none, all, gf) : client_write_sum_join(all, none, gf);
  }
  const CwSum a = random_fold(ios, lo, mid, rng, gf);
  return client_write_sum_join(a, random_fold(ios, mid, hi, rng, gf), gf);
}

bool same(const CwFile& a, const CwFile& b) {
  return a.status == b.status && a.length == b.length && a.value == b.value && a.type == b.type && a.failed == b.failed;
}

void show(const char* name, const CwFile& f) {
  fprintf(stderr, "  %s: status %d length %llu checksum {%u, %08x} failed %u\n", name, f.status,
          (unsigned long long)f.length, f.type, f.value, f.failed);
}

// ---- prepare ------------------------------------------------------------------------------------
struct Out {
  int32_t status;
  uint32_t checksum;
  uint8_t type, send_inline;
  bool hashed;
};

// The reference's order: one loop that drops, one over the survivors that is all or nothing, the send.
std::vector<Out> reference_prepare(const std::vector<Io>& ios, const std::vector<uint32_t>& crc, uint8_t type,
                                   uint32_t max_len, uint32_t max_inline, bool verify, bool* poisoned) {
  std::vector<Out> out(ios.size());
  std::vector<size_t> valid;
  for (size_t i = 0; i < ios.size(); ++i) {
    out[i] = Out{0, 0, 0, 0, false};
    if (ios[i].length > max_len) {
      out[i].status = 3;
      continue;
    }
    const uint32_t end = ios[i].offset + ios[i].length;  // uint32_t: wraps
    if (ios[i].chunk_size == 0 || end > ios[i].chunk_size) {
      out[i].status = 7002;
      continue;
    }
    valid.push_back(i);
  }
  *poisoned = false;
  for (size_t i : valid) {
    const Io& io = ios[i];
    bool ok = io.buf_base != 0 && io.data != 0;
    if (ok) {
      const unsigned __int128 end = (unsigned __int128)io.data + io.length, cap = (unsigned __int128)io.buf_base + io.buf_size;
      ok = end <= UINT64_MAX && cap <= UINT64_MAX && io.buf_base <= io.data && end <= cap;
    }
    out[i].hashed = ok && verify && io.length > 0;  // valid by itself: its bytes may be read
    if (!ok) *poisoned = true;
  }
  for (size_t i : valid) {
    if (*poisoned) {
      out[i].status = 7002;
      continue;
    }
    if (verify) {
      out[i].type = type;
      out[i].checksum = ios[i].length ? crc[i] : ~0u;
    }
    out[i].send_inline = ios[i].length <= max_inline;
  }
  return out;
}

int main(int argc, char** argv) {
  const uint64_t files = argc > 1 ? strtoull(argv[1], nullptr, 0) : 20000;
  std::mt19937_64 rng(0x43575254);
  const GfFast fast;
  const CwGfPlain plain;
  for (int k = 0; k < 200; ++k) {  // the fuzz's arithmetic is gf2.h's
    const uint32_t v = (uint32_t)rng();
    const uint64_t n = k < 64 ? 1ull << k : rng() >> (rng() % 64);
    const uint8_t t = 1 + k % 2;
    if (fast.shift(v, n, t) != plain.shift(v, n, t)) return fprintf(stderr, "shift differs\n"), 1;
  }

  // ---- prepare
  uint64_t batches = 0, prep_ios = 0, seen_prep[6] = {};  // sent, range, bad, poisoned IOs, hashed, poisoned batches
  for (uint64_t round = 0; round < files / 10 + 100; ++round) {
    const uint32_t n = (uint32_t)(rng() % 40);
    const bool verify = rng() % 2;
    const uint8_t type = 1 + rng() % 2;
    const uint32_t max_len = rng() % 3 ? 1u << 20 : ~0u, max_inline = rng() % 3 ? (uint32_t)(rng() % 4096) : 0;
    const uint32_t offender_odds = rng() % 2 ? 0 : 1 + (uint32_t)(rng() % (2 * n + 1));
    std::vector<Io> ios(n);
    std::vector<uint32_t> crc(n);
    for (uint32_t i = 0; i < n; ++i) {
      Io& io = ios[i];
      memset(&io, 0xA5, sizeof(io));
      io.buf_base = 0x10000 + (rng() % 16) * 4096;
      io.buf_size = 1 << 16;
      io.length = rng() % 8 == 0 ? 0 : (uint32_t)(rng() % 4097);
      io.data = io.buf_base + rng() % (io.buf_size - io.length + 1);
      io.chunk_size = 1u << (12 + rng() % 10);
      io.offset = (uint32_t)(rng() % (io.chunk_size - (io.length < io.chunk_size ? io.length : io.chunk_size) + 1));
      switch (rng() % 24) {  // the droppable shapes
        case 0: io.length = max_len == ~0u ? io.length : max_len + 1 + (uint32_t)(rng() % 9); break;
        case 1: io.chunk_size = 0; break;
        case 2: io.offset = io.chunk_size - io.length + 1; break;
        case 3: io.offset = io.chunk_size - io.length; break;                      // the last byte of the chunk
        case 4: io.offset = 0xFFFFFFF0u, io.length = 0x20, io.chunk_size = 0x100; break;  // wraps and passes
        case 5: io.offset = (uint32_t)rng(), io.length = (uint32_t)rng() >> (rng() % 32); break;
      }
      if (offender_odds && rng() % offender_odds == 0) {
        switch (rng() % 9) {
          case 0: io.data = 0; break;
          case 1: io.buf_base = 0; break;
          case 2: io.data = io.buf_base + io.buf_size - io.length + 1; break;   // one past the end
          case 3: io.data = io.buf_base - 1; break;
          case 4: io.data = io.buf_base + io.buf_size - io.length; break;       // ends with the buffer: contained
          case 5: io.data = io.buf_base; break;                                  // starts with it: contained
          case 6: io.data = ~0ull - io.length / 2, io.buf_base = 1, io.buf_size = ~0ull - 1; break;  // data + length wraps
          case 7: io.buf_base = ~0ull - 100, io.buf_size = 4096, io.data = io.buf_base + 8; break;   // base + size wraps
          case 8: io.buf_size = 0; break;
        }
      }
      crc[i] = (uint32_t)rng();
    }
    bool want_poison = false;
    const std::vector<Out> want = reference_prepare(ios, crc, type, max_len, max_inline, verify, &want_poison);
    // as the kernels run it: every IO's class and the poison word, then every IO's settle
    bool poison = false;
    for (uint32_t i = 0; i < n; ++i) poison |= client_write_class(ios[i], max_len) == kCwOffender;
    if (poison != want_poison) return fprintf(stderr, "prepare round %llu: poison %d\n", (unsigned long long)round, poison), 1;
    for (uint32_t i = 0; i < n; ++i) {
      const CwClass k = client_write_class(ios[i], max_len);
      const bool hashes = client_write_hashes(k, verify, ios[i].length);
      const CwPrepared p = client_write_settle(k, poison, ios[i].length, hashes ? crc[i] : ~0u, type, verify, max_inline);
      if (p.status != want[i].status || p.checksum != want[i].checksum || p.checksum_type != want[i].type ||
          p.send_inline != want[i].send_inline || hashes != want[i].hashed || p.sent != (want[i].status == 0)) {
        fprintf(stderr, "prepare round %llu IO %u: status %d checksum {%u, %08x} inline %u hashed %d, expected %d {%u, %08x} %u %d\n",
                (unsigned long long)round, i, p.status, p.checksum_type, p.checksum, p.send_inline, (int)hashes,
                want[i].status, want[i].type, want[i].checksum, want[i].send_inline, (int)want[i].hashed);
        return 1;
      }
      ++seen_prep[p.status == 0 ? 0 : k == kCwRange ? 1 : k == kCwBadRecord ? 2 : 3];
      seen_prep[4] += hashes;
    }
    seen_prep[5] += poison;
    ++batches;
    prep_ios += n;
  }

  // ---- complete
  uint64_t total_ios = 0, cuts = 0, seen[kBranches] = {};
  for (uint64_t round = 0; round < files; ++round) {
    const uint32_t shape = (uint32_t)(rng() % 100);
    const uint32_t n = round % 29 == 0 ? 0 : shape < 80 ? (uint32_t)(rng() % 13) : shape < 98 ? (uint32_t)(rng() % 200)
                                                                                           : (uint32_t)(rng() % 2001);
    const uint8_t type = 1 + rng() % 2;
    // the odds of an IO that ends the fold by itself, and of a deviant (another type, often without bytes)
    const uint32_t end_odds = rng() % 3 == 0 ? 0 : 1 + (uint32_t)(rng() % (3 * (n + 1)));
    const uint32_t deviant_odds = rng() % 3 == 0 ? 0 : 1 + (uint32_t)(rng() % (2 * (n + 1)));
    const uint32_t mix = (uint32_t)(rng() % 5);  // 0-1: all `type`, 2: type + NONE, 3: all three, 4: all NONE
    const uint32_t zero_odds = 2 + (uint32_t)(rng() % 8);
    const bool big = rng() % 2;
    std::vector<CwAnswer> ios(n);
    for (uint32_t k = 0; k < n; ++k) {
      Io io;
      memset(&io, 0, sizeof(io));
      io.length = rng() % zero_odds == 0 ? 0 : big ? (uint32_t)rng() : 1 + (uint32_t)(rng() % (1u << 20));
      if (rng() % 64 == 0) io.length = ~0u;
      io.result_len = io.length;
      io.result_checksum = (uint32_t)rng();
      const uint32_t pick = (uint32_t)(rng() % 8);
      io.result_checksum_type = mix < 2 ? type : mix == 2 ? (pick < 6 ? type : 0) : mix == 3 ? (uint8_t)(pick % 3) : 0;
      if (deviant_odds && rng() % deviant_odds == 0) {
        io.result_checksum_type = (uint8_t)((io.result_checksum_type + 1 + rng() % 2) % 3);
        if (rng() % 2) io.length = io.result_len = 0;
      }
      if (end_odds && rng() % end_odds == 0) {
        switch (rng() % 5) {
          case 0: io.status = rng() % 2 ? 7002 : 3; break;                 // prepare's status
          case 1: io.status_in = rng() % 2 ? 7003 : 4080; break;           // the answer's
          case 2: io.result_len = io.length - 1; break;                    // a short write (wraps for 0)
          case 3: io.result_checksum_type = 3 + rng() % 200; break;
          case 4: io.status = 7002, io.status_in = 4010; break;            // prepare's wins
        }
      }
      const CwAnswer a = client_write_answer(io);
      const int32_t final_status = io.status != 0 ? io.status : io.status_in;
      if (a.status != final_status || a.result_len != io.result_len || a.length != io.length ||
          a.value != io.result_checksum || a.type != io.result_checksum_type)
        return fprintf(stderr, "round %llu IO %u: the answer view differs\n", (unsigned long long)round, k), 1;
      ios[k] = a;
    }
    bool took[kBranches] = {};
    const CwFile a = reference_loop(ios, took);
    const CwFile b = plan_loop(ios, fast);
    const CwFile c = wave_fold(ios, fast);
    const CwFile d = client_write_sum_finish(random_fold(ios, 0, ios.size(), rng, fast));
    bool ok = same(a, b) && same(a, c) && same(a, d);
    CwFile e = a;
    if (ok && n <= 12)
      for (size_t cut = 0; cut <= n && ok; ++cut, ++cuts) {
        e = client_write_sum_finish(client_write_sum_join(run_sum(ios, 0, cut, fast), run_sum(ios, cut, n, fast), fast));
        ok = same(a, e);
      }
    if (!ok) {
      fprintf(stderr, "round %llu (%u IOs, type %u): the forms differ\n", (unsigned long long)round, n, type);
      for (uint32_t k = 0; k < n && n <= 16; ++k)
        fprintf(stderr, "    IO %u: status %d type %u result_len %u length %u value %08x\n", k, ios[k].status, ios[k].type,
                ios[k].result_len, ios[k].length, ios[k].value);
      show("reference loop", a);
      show("plan loop", b);
      show("wave fold", c);
      show("random fold", d);
      show("two runs", e);
      return 1;
    }
    if (round % 50 == 0 && n <= 200 && !same(a, plan_loop(ios, plain)))  // and with gf2.h's own shift
      return fprintf(stderr, "round %llu: the plan loop differs under gf2.h's shift\n", (unsigned long long)round), 1;
    // Bench.cc:41-48 on top
    CwFile hit = a, miss = a;
    client_write_expect(hit, a.value);
    client_write_expect(miss, a.value ^ 1u);
    if (!same(hit, a) || (a.status == 0 ? miss.status != 7015 || miss.failed != ~0u || miss.value != a.value : !same(miss, a)))
      return fprintf(stderr, "round %llu: the expected-value check differs\n", (unsigned long long)round), 1;
    total_ios += n;
    for (int k = 0; k < kBranches; ++k) seen[k] += took[k];
  }
  printf("{\"fuzz_client_write\": \"ok\", \"files\": %llu, \"ios\": %llu, \"cuts\": %llu, \"batches\": %llu, "
         "\"prepare_ios\": %llu, \"prepare_sent\": %llu, \"prepare_range\": %llu, \"prepare_bad_record\": %llu, "
         "\"prepare_poisoned\": %llu, \"prepare_hashed\": %llu, \"prepare_poisoned_batches\": %llu, \"branches\": {",
         (unsigned long long)files, (unsigned long long)total_ios, (unsigned long long)cuts,
         (unsigned long long)batches, (unsigned long long)prep_ios, (unsigned long long)seen_prep[0],
         (unsigned long long)seen_prep[1], (unsigned long long)seen_prep[2], (unsigned long long)seen_prep[3],
         (unsigned long long)seen_prep[4], (unsigned long long)seen_prep[5]);
  for (int k = 0; k < kBranches; ++k)
    printf("%s\"%s\": %llu", k ? ", " : "", kBranchName[k], (unsigned long long)seen[k]);
  printf("}}\n");
  return 0;
}
