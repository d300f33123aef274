// fuzz_client_read.cpp -- 3fs_amd/csrc/client_read_plan.h on the CPU: the order-free fold of the
// split-read merge against the reference's loop.
//
// For random parents of 0 to 2,000 children (every mix of the three types, zero lengths, failing
// statuses, verify mismatches, bad records, lengths up to 2^32 - 1) four computations must agree in
// every field of the parent:
//   (a) a restatement written here in the shape of StorageClientImpl.cc:1607-1633 over
//       ChecksumInfo::combine (Common.h:179-198): for, if / else if / else, break, a switch on the
//       parent's type.  It uses gf2.h's combine_raw and nothing of the plan but the child view,
//       and it counts which branches a parent took.
//   (b) client_seq_begin / client_seq_step, the loop of the lane schedule;
//   (c) client_sum_of / client_sum_join / client_sum_finish bracketed as the wave schedule does it:
//       64 contiguous runs folded left to right, then the ordered tree over the 64 partials;
//   (d) the same fold under a random bracketing (associativity).
// The children come out of client_read_verdict over random records, so the hash decision and the
// verdict are exercised on the way; they are checked against rules restated here.
// Usage:  fuzz_client_read [parents]     prints one JSON line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../3fs_amd/csrc/client_read_plan.h"

using namespace hf3fs_crc;
using Io = hf3fs_crc_client_read_io;
static_assert(sizeof(Io) == 40, "hf3fs_crc_client_read_io layout");
static_assert(sizeof(hf3fs_crc_client_read_result) == 24, "hf3fs_crc_client_read_result layout");

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
  kNoChildren, kTakeFirst, kTakeMiddle, kTakeLast, kTakeMismatch, kTakeBadRecord, kAdoptTyped, kAdoptNone,
  kTypeIgnored, kZeroLength, kCombineCrc32c, kCombineCrc32, kLengthWrap, kClean, kBranches
};
const char* const kBranchName[kBranches] = {"no_children", "take_first", "take_middle", "take_last", "take_mismatch",
                                            "take_bad_record", "adopt_typed", "adopt_none", "type_ignored",
                                            "zero_length", "combine_crc32c", "combine_crc32", "length_wrap", "clean"};

// (a)
ClientParent reference_loop(const std::vector<ClientChild>& kids, bool* took) {
  ClientParent p;
  p.status = 7003;  // IOResult(): lengthInfo = makeError(kNotInitialized)
  p.length = 0;
  p.value = 0;
  p.type = 0;
  p.failed = ~0u;
  p.block_len = 0;
  if (kids.empty()) took[kNoChildren] = true;
  for (const ClientChild& c : kids) p.block_len += c.length;
  bool clean = !kids.empty();
  for (size_t ioIndex = 0; ioIndex < kids.size(); ioIndex++) {
    const ClientChild& io = kids[ioIndex];
    if (io.status != 0) {  // !bool(splittedIO.result.lengthInfo)
      p.status = io.status;
      p.length = 0;
      p.value = io.value;
      p.type = io.type;
      p.failed = (uint32_t)ioIndex;
      took[ioIndex == 0 ? kTakeFirst : ioIndex + 1 == kids.size() ? kTakeLast : kTakeMiddle] = true;
      if (io.status == 7015) took[kTakeMismatch] = true;
      if (io.status == 3) took[kTakeBadRecord] = true;
      clean = false;
      break;
    } else if (ioIndex == 0) {
      p.status = 0;
      p.length = io.read_len;
      p.value = io.value;
      p.type = io.type;
    } else {
      const uint64_t wide = (uint64_t)p.length + io.read_len;
      if (wide >> 32) took[kLengthWrap] = true;
      p.length = (uint32_t)wide;
      // ChecksumInfo::combine(o, length), the Result dropped
      if (p.type != 0 && p.type != io.type) {
        took[kTypeIgnored] = true;
        continue;
      }
      if (io.read_len == 0) {
        took[kZeroLength] = true;
        continue;
      }
      switch (p.type) {
        case 0:
          p.type = io.type;
          p.value = io.value;
          took[io.type == 0 ? kAdoptNone : kAdoptTyped] = true;
          break;
        case 1:
          p.value = combine_raw(~p.value, io.value, io.read_len, kPolyCrc32c);
          took[kCombineCrc32c] = true;
          break;
        case 2:
          p.value = combine_raw(~p.value, io.value, io.read_len, kPolyCrc32);
          took[kCombineCrc32] = true;
          break;
      }
    }
  }
  if (clean) took[kClean] = true;
  return p;
}

// (b)
template <class Gf>
ClientParent plan_loop(const std::vector<ClientChild>& kids, const Gf& gf) {
  ClientSeq s = client_seq_begin();
  for (size_t k = 0; k < kids.size(); ++k) client_seq_step(s, kids[k], (uint32_t)k, gf);
  return s.p;
}

template <class Gf>
ClientParent finish(const ClientSum& s, const std::vector<ClientChild>& kids, const Gf& gf) {
  return client_sum_finish(s, kids.size(), [&](uint32_t j) { return kids.at(j); }, gf);
}

// (c)
template <class Gf>
ClientParent wave_fold(const std::vector<ClientChild>& kids, const Gf& gf) {
  const uint64_t k = kids.size(), run = (k + 63) / 64;
  ClientSum lane[64];
  for (uint64_t l = 0; l < 64; ++l) {
    lane[l] = client_sum_identity();
    for (uint64_t j = l * run, e = j + run < k ? j + run : k; j < e; ++j)
      lane[l] = client_sum_join(lane[l], client_sum_of(kids[j], (uint32_t)j), gf);
  }
  for (int d = 1; d < 64; d <<= 1)
    for (int l = 0; l + d < 64; l += 2 * d) lane[l] = client_sum_join(lane[l], lane[l + d], gf);
  return finish(lane[0], kids, gf);
}

// (d)
template <class Gf>
ClientSum random_fold(const std::vector<ClientChild>& kids, size_t lo, size_t hi, std::mt19937_64& rng, const Gf& gf) {
  if (hi == lo) return client_sum_identity();
  if (hi - lo == 1) return client_sum_of(kids[lo], (uint32_t)lo);
  const size_t mid = lo + (size_t)(rng() % (hi - lo + 1));  // an empty side joins the identity
  if (mid == lo || mid == hi) {
    const ClientSum all = random_fold(kids, lo, lo + (hi - lo) / 2, rng, gf);
    return client_sum_join(all, random_fold(kids, lo + (hi - lo) / 2, hi, rng, gf), gf);
  }
  const ClientSum a = random_fold(kids, lo, mid, rng, gf);
  return client_sum_join(a, random_fold(kids, mid, hi, rng, gf), gf);
}

bool same(const ClientParent& a, const ClientParent& b) {
  return a.status == b.status && a.length == b.length && a.value == b.value && a.type == b.type &&
         a.failed == b.failed && a.block_len == b.block_len;
}

void show(const char* name, const ClientParent& p) {
  fprintf(stderr, "  %s: status %d length %u checksum {%u, %08x} failed %u block_len %u\n", name, p.status, p.length,
          p.type, p.value, p.failed, p.block_len);
}

int main(int argc, char** argv) {
  const uint64_t parents = argc > 1 ? strtoull(argv[1], nullptr, 0) : 1500;
  std::mt19937_64 rng(0x434C5244);
  const GfFast fast;
  const ClientGfPlain plain;
  for (int k = 0; k < 200; ++k) {  // the fuzz's arithmetic is gf2.h's
    const uint32_t v = (uint32_t)rng();
    const uint64_t n = k < 64 ? 1ull << k : rng() >> (rng() % 64);
    const uint8_t t = 1 + k % 2;
    if (fast.shift(v, n, t) != plain.shift(v, n, t)) {
      fprintf(stderr, "shift(%08x, %llu, %u) differs\n", v, (unsigned long long)n, t);
      return 1;
    }
  }
  uint64_t children = 0, seen[kBranches] = {}, verdicts[4] = {};
  for (uint64_t round = 0; round < parents; ++round) {
    const uint32_t shape = (uint32_t)(rng() % 10);
    const uint32_t n = round % 23 == 0 ? 0 : shape < 6 ? (uint32_t)(rng() % 8) : shape < 9 ? (uint32_t)(rng() % 200)
                                                                                           : (uint32_t)(rng() % 2001);
    const bool verify = rng() % 2;
    const uint8_t type = 1 + rng() % 2;
    const uint32_t max_len = rng() % 4 ? ~0u : 1u << 20;
    // what the parent is made of: the odds of a failing child, of a zero length, of each type
    const uint32_t fail_odds = rng() % 3 == 0 ? 0 : 1 + (uint32_t)(rng() % (4 * (n + 1)));
    const uint32_t mix = (uint32_t)(rng() % 4);  // 0: all `type`, 1: type + NONE, 2: all three, 3: mostly NONE
    const bool big = rng() % 2;
    std::vector<ClientChild> kids(n);
    for (uint32_t k = 0; k < n; ++k) {
      Io io;
      memset(&io, 0, sizeof(io));
      io.data = rng() % 16 == 0 ? 0 : 0x1000 + rng() % 4096;
      io.read_len = rng() % 6 == 0 ? 0 : big ? (uint32_t)rng() : (uint32_t)(rng() % (1u << 20));
      if (rng() % 64 == 0) io.read_len = ~0u;
      io.length = rng() % 16 == 0 ? (uint32_t)rng() : io.read_len + (uint32_t)(rng() % 3 == 0);
      if (io.length < io.read_len && rng() % 4) io.length = io.read_len;
      io.status_in = fail_odds && rng() % fail_odds == 0 ? (rng() % 2 ? 7007 : 4010) : 0;
      io.checksum = (uint32_t)rng();
      const uint32_t pick = (uint32_t)(rng() % 8);
      io.checksum_type = mix == 0 ? type : mix == 1 ? (pick < 5 ? type : 0) : mix == 2 ? (uint8_t)(pick % 3)
                                                                                       : (pick < 6 ? 0 : type);
      if (rng() % 512 == 0) io.checksum_type = 3 + rng() % 200;
      if (io.checksum_type == 0 && rng() % 2) io.checksum = 0;  // what a NONE-typed answer really carries
      // the hashed value: mostly the server's (a verify that passes)
      const uint32_t hashed = fail_odds && rng() % fail_odds == 0 ? (uint32_t)rng() : io.checksum;
      const ClientChild c = client_read_verdict(io, hashed, type, max_len, verify);
      // the rules, restated
      const bool known = io.checksum_type <= 2;
      const bool bad = io.status_in == 0 &&
                       (!known || (verify && ((io.checksum_type != 0 && io.checksum_type != type) ||
                                              io.read_len > max_len || io.read_len > io.length ||
                                              (io.read_len > 0 && io.data == 0))));
      const bool compared = verify && io.status_in == 0 && io.read_len > 0 && !bad;
      const uint32_t local = io.checksum_type == 0 ? 0u : hashed;
      const int32_t want = bad ? 3 : compared && local != io.checksum ? 7015 : io.status_in;
      const bool hashes = client_read_hashes(io, type, max_len, verify);
      if (c.status != want || c.computed != (compared ? local : 0u) || hashes != (compared && io.checksum_type != 0) ||
          c.read_len != io.read_len || c.length != io.length ||
          c.type != (want == 7015 ? 0 : io.checksum_type) || c.value != (want == 7015 ? 0u : io.checksum)) {
        fprintf(stderr, "round %llu child %u: verdict %d (computed %08x), expected %d\n", (unsigned long long)round, k,
                c.status, c.computed, want);
        return 1;
      }
      ++verdicts[want == 0 ? 0 : want == 3 ? 1 : want == 7015 ? 2 : 3];
      kids[k] = c;
    }
    bool took[kBranches] = {};
    const ClientParent a = reference_loop(kids, took);
    const ClientParent b = plan_loop(kids, fast);
    const ClientParent c = wave_fold(kids, fast);
    const ClientParent d = finish(random_fold(kids, 0, kids.size(), rng, fast), kids, fast);
    if (!same(a, b) || !same(a, c) || !same(a, d)) {
      fprintf(stderr, "round %llu (%u children, verify %d, type %u): the forms differ\n", (unsigned long long)round, n,
              (int)verify, type);
      show("reference loop", a);
      show("plan loop", b);
      show("wave fold", c);
      show("random fold", d);
      return 1;
    }
    if (round % 50 == 0 && n <= 200 && !same(a, plan_loop(kids, plain))) {  // and with gf2.h's own shift
      fprintf(stderr, "round %llu: the plan loop differs under gf2.h's shift\n", (unsigned long long)round);
      return 1;
    }
    children += n;
    for (int k = 0; k < kBranches; ++k) seen[k] += took[k];
  }
  printf("{\"fuzz_client_read\": \"ok\", \"parents\": %llu, \"children\": %llu, \"verdict_ok\": %llu, "
         "\"verdict_bad_record\": %llu, \"verdict_mismatch\": %llu, \"verdict_failed\": %llu, \"branches\": {",
         (unsigned long long)parents, (unsigned long long)children, (unsigned long long)verdicts[0],
         (unsigned long long)verdicts[1], (unsigned long long)verdicts[2], (unsigned long long)verdicts[3]);
  for (int k = 0; k < kBranches; ++k)
    printf("%s\"%s\": %llu", k ? ", " : "", kBranchName[k], (unsigned long long)seen[k]);
  printf("}}\n");
  return 0;
}
