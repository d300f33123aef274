// fuzz_md5.cpp -- 3fs_amd/csrc/md5_core.h against hashlib's digests, on the CPU.
//
// tests/test_md5_sanitized.py writes a case file: per case a content, its cut into segments (empty
// ones and holes among them; the content is zero where a hole lies), the residue mod 16 of the first
// segment's address, the split of the segments over 1-4 calls, and hashlib's hex digest.  Every case
// is replayed the way k_md5_hash of md5_kernels.hip walks a file -- stream open from the carried
// state, md5_call_blocks blocks, a block inside one segment through the aligned 16-byte granules and
// md5_words_from_granules (zeros for a hole), every other block through the byte cursor, then the
// digest or md5_state_out -- and once more through the byte cursor alone.  Both must give the
// digest, and every state between two calls must be the same 96 bytes in both, its tail zero beyond
// total % 64.
// Usage:  fuzz_md5 <case file>       prints one JSON line with what the cases covered
//
// A line of the case file:  residue digest content-hex|- ncalls { nsegs { kind length } }
// or, a file that is one hole:  H length digest
// The second kind takes totals past 2^29 bytes (a bit length that needs its upper word) through the
// core where bytes cost nothing: an INIT call over the hole leaves the state just before the
// padding, which is printed as its own JSON line {"hole", "h", "total"} (tests/md5_queue.py keeps
// these as seeds for the GPU), a FINAL call without segments from that state gives the digest, and
// below 2^30 bytes the one-shot call must give it too.  Only the block path of the kernel is walked:
// the byte cursor over 2^32 zeros is the same 64 bytes 2^26 times.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../../3fs_amd/csrc/md5_core.h"

using namespace hf3fs_crc;
static_assert(sizeof(hf3fs_crc_md5_seg) == 16 && sizeof(hf3fs_crc_md5_state) == 96, "ABI layout");

struct Counts {
  uint64_t cases = 0, calls = 0, granule_blocks = 0, hole_blocks = 0, cursor_blocks = 0, pad_one = 0, pad_two = 0,
           holes = 0, empty_segs = 0, empty_calls = 0, long_holes = 0;
  uint64_t tails = 0;     // bit t: a call began with t carried bytes
  uint32_t residues = 0;  // bit r: a granule block began r bytes into a granule
};

struct Call {
  std::vector<hf3fs_crc_md5_seg> segs;
};

static void fail(size_t line, const char* what) {
  fprintf(stderr, "fuzz_md5: case %zu: %s\n", line, what);
  exit(1);
}

static std::string hex(const uint8_t* p, size_t n) {
  static const char d[] = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) s += d[p[i] >> 4], s += d[p[i] & 15];
  return s;
}

// One call, as the hash kernel runs one lane.  fast: take blocks inside one segment through the
// granules.  Returns the digest (FINAL) or leaves the next state in *state.
static void run_call(const Call& c, uint32_t flags, hf3fs_crc_md5_state* state, uint8_t digest[16], bool fast,
                     Counts* n) {
  const bool init = flags & HF3FS_MD5_INIT, final = flags & HF3FS_MD5_FINAL;
  Md5Stream s;
  md5_stream_open(s, c.segs.data(), 0, c.segs.size(), init ? nullptr : state);
  uint32_t h[4];
  md5_init(h);
  if (!init) memcpy(h, state->h, sizeof(h));
  uint64_t bytes = 0;
  for (const auto& g : c.segs) bytes += g.length;
  const uint64_t blocks = md5_call_blocks(s.tail_len, bytes, final);
  if (n) {
    n->tails |= 1ull << s.tail_len;
    if (final) ++(((s.tail_len + bytes) % 64) < 56 ? n->pad_one : n->pad_two);
  }
  for (uint64_t b = 0; b < blocks; ++b) {
    uint32_t w[16];
    if (fast && md5_stream_run64(s)) {
      if (s.addr == 0) {
        memset(w, 0, sizeof(w));
        if (n) ++n->hole_blocks;
      } else {
        const uint32_t r = (uint32_t)(s.addr & 15);
        uint32_t g[20] = {};
        memcpy(g, (const void*)(uintptr_t)(s.addr - r), r ? 80 : 64);  // whole aligned granules only
        md5_words_from_granules(g, r, w);
        if (n) ++n->granule_blocks, n->residues |= 1u << r;
      }
      md5_stream_skip64(s);
    } else {
      md5_stream_block(s, final, w);
      if (n && fast) ++n->cursor_blocks;
    }
    md5_block(h, w);
  }
  if (final) {
    md5_digest_bytes(h, digest);
  } else {
    uint32_t tail[16];
    hf3fs_crc_md5_state out;
    md5_state_out(s, h, out.h, &out.total, tail);
    memcpy(out.tail, tail, 64);
    out.reserved = 0;
    *state = out;
  }
}

static void run_long_hole(size_t lineno, uint64_t length, const std::string& want, Counts* n) {
  Call hole, none;
  hole.segs.push_back({0, length});
  hf3fs_crc_md5_state state;
  memset(&state, 0xA5, sizeof(state));
  uint8_t digest[16] = {};
  run_call(hole, HF3FS_MD5_INIT, &state, digest, true, n);
  if (state.total != length || state.reserved) fail(lineno, "state total of a hole");
  for (unsigned i = 0; i < 64; ++i)
    if (state.tail[i]) fail(lineno, "state tail of a hole");
  printf("{\"hole\": %llu, \"h\": [%u, %u, %u, %u], \"total\": %llu}\n", (unsigned long long)length, state.h[0],
         state.h[1], state.h[2], state.h[3], (unsigned long long)state.total);
  const hf3fs_crc_md5_state before = state;
  run_call(none, HF3FS_MD5_FINAL, &state, digest, true, n);
  if (memcmp(&before, &state, sizeof(before))) fail(lineno, "FINAL changed the state");
  if (hex(digest, 16) != want) fail(lineno, ("digest of a hole " + hex(digest, 16) + " != " + want).c_str());
  if (length < (1ull << 30)) {
    run_call(hole, HF3FS_MD5_INIT | HF3FS_MD5_FINAL, nullptr, digest, true, n);
    if (hex(digest, 16) != want) fail(lineno, "one-shot digest of a hole");
  }
  ++n->long_holes;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: fuzz_md5 <case file>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    fprintf(stderr, "fuzz_md5: cannot read %s\n", argv[1]);
    return 2;
  }
  Counts n;
  std::mt19937_64 rng(0x3d5);
  std::string line;
  size_t lineno = 0;
  while (std::getline(in, line)) {
    ++lineno;
    if (line.empty()) continue;
    if (line[0] == 'H') {
      std::istringstream hs(line.substr(1));
      uint64_t length = 0;
      std::string want;
      hs >> length >> want;
      if (!hs || want.size() != 32) fail(lineno, "bad hole line");
      run_long_hole(lineno, length, want, &n);
      ++n.cases;
      continue;
    }
    std::istringstream ls(line);
    unsigned residue = 0, ncalls = 0;
    std::string want, content_hex;
    ls >> residue >> want >> content_hex >> ncalls;
    if (!ls || residue > 15 || ncalls < 1 || ncalls > 4 || want.size() != 32) fail(lineno, "bad header");
    std::vector<uint8_t> content;
    if (content_hex != "-")
      for (size_t i = 0; i + 1 < content_hex.size(); i += 2)
        content.push_back((uint8_t)strtoul(content_hex.substr(i, 2).c_str(), nullptr, 16));
    // The arena: every data segment a copy of its bytes, the first at `residue` mod 16, the others
    // wherever a junk gap of 0-20 bytes leaves them; 32 junk bytes at both ends.
    struct Piece {
      bool hole;
      uint64_t at, len, arena_off;
    };
    std::vector<std::vector<Piece>> pieces(ncalls);
    uint64_t pos = 0, arena_size = 32 + residue;
    for (unsigned c = 0; c < ncalls; ++c) {
      unsigned nsegs = 0;
      ls >> nsegs;
      for (unsigned k = 0; k < nsegs; ++k) {
        unsigned kind = 0;
        uint64_t len = 0;
        ls >> kind >> len;
        if (!ls || kind > 1) fail(lineno, "bad segment");
        Piece p{kind == 1, pos, len, 0};
        if (!p.hole) {
          p.arena_off = arena_size;
          arena_size += len + rng() % 21;
        }
        pos += len;
        pieces[c].push_back(p);
      }
    }
    if (!ls || pos != content.size()) fail(lineno, "segments do not cover the content");
    arena_size += 32;
    uint8_t* arena = (uint8_t*)aligned_alloc(16, (arena_size + 15) / 16 * 16);
    if (!arena) fail(lineno, "no memory");
    for (uint64_t i = 0; i < arena_size; ++i) arena[i] = (uint8_t)(1 + rng() % 255);
    std::vector<Call> calls(ncalls);
    for (unsigned c = 0; c < ncalls; ++c)
      for (const Piece& p : pieces[c]) {
        if (p.hole) {
          for (uint64_t i = 0; i < p.len; ++i)
            if (content[p.at + i]) fail(lineno, "content is not zero in a hole");
          ++n.holes;
        } else if (p.len) {
          memcpy(arena + p.arena_off, content.data() + p.at, p.len);
        }
        if (!p.len) ++n.empty_segs;
        calls[c].segs.push_back({p.hole ? 0 : (uint64_t)(uintptr_t)(arena + p.arena_off), p.len});
      }
    hf3fs_crc_md5_state state[2];
    memset(state, 0xA5, sizeof(state));
    uint8_t digest[2][16] = {};
    uint64_t seen = 0;
    for (unsigned c = 0; c < ncalls; ++c) {
      const uint32_t flags = (c == 0 ? HF3FS_MD5_INIT : 0) | (c + 1 == ncalls ? HF3FS_MD5_FINAL : 0);
      const hf3fs_crc_md5_state before = state[0];
      run_call(calls[c], flags, &state[0], digest[0], true, &n);
      run_call(calls[c], flags, &state[1], digest[1], false, nullptr);
      ++n.calls;
      uint64_t bytes = 0;
      for (const auto& g : calls[c].segs) bytes += g.length;
      if (!bytes) ++n.empty_calls;
      seen += bytes;
      if (flags & HF3FS_MD5_FINAL) {
        if (c && memcmp(&before, &state[0], sizeof(before))) fail(lineno, "FINAL changed the state");
        continue;
      }
      if (memcmp(&state[0], &state[1], sizeof(state[0]))) fail(lineno, "granule path and byte cursor leave different states");
      if (state[0].total != seen || state[0].reserved) fail(lineno, "state total");
      for (unsigned i = 0; i < 64; ++i) {
        const uint8_t want_byte = i < seen % 64 ? content[seen - seen % 64 + i] : 0;
        if (state[0].tail[i] != want_byte) fail(lineno, "state tail");
      }
    }
    if (hex(digest[0], 16) != want) fail(lineno, ("digest " + hex(digest[0], 16) + " != " + want).c_str());
    if (hex(digest[1], 16) != want) fail(lineno, "byte-cursor digest");
    free(arena);
    ++n.cases;
  }
  printf("{\"fuzz_md5\": \"ok\", \"cases\": %llu, \"calls\": %llu, \"granule_blocks\": %llu, \"hole_blocks\": %llu, "
         "\"cursor_blocks\": %llu, \"pad_one\": %llu, \"pad_two\": %llu, \"holes\": %llu, \"empty_segs\": %llu, "
         "\"empty_calls\": %llu, \"long_holes\": %llu, \"tail_lengths\": %d, \"residues\": %d}\n",
         (unsigned long long)n.cases, (unsigned long long)n.calls, (unsigned long long)n.granule_blocks,
         (unsigned long long)n.hole_blocks, (unsigned long long)n.cursor_blocks, (unsigned long long)n.pad_one,
         (unsigned long long)n.pad_two, (unsigned long long)n.holes, (unsigned long long)n.empty_segs,
         (unsigned long long)n.empty_calls, (unsigned long long)n.long_holes, __builtin_popcountll(n.tails), __builtin_popcount(n.residues));
  return 0;
}
