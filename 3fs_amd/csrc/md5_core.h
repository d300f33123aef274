// md5_core.h -- everything hf3fs_crc_md5_batch decides about bytes, plain C++ that both the device
// compiler and a host compiler take: the RFC 1321 block function, and the stream of one file in
// one call -- the incoming tail of hf3fs_crc_md5_state, then the file's segments in order (any
// address, any length, zero-length ones, holes), then with FINAL the padding and the bit length.
// The kernels of md5_kernels.hip call exactly these functions; tests/cpp/fuzz_md5.cpp includes this
// header and replays random cases against hashlib's digests under ASan + UBSan.
//
// The reference (src/client/cli/admin/Checksum.cc:50-83, FileWrapper.cc:172-177) is MD5_Init, one
// MD5_Update per buffer fill in file order, MD5_Final: a stream's bytes are what those updates saw.
#pragma once
#include <stdint.h>

#include "../../include/hf3fs_crc.h"

#ifdef __HIPCC__
#define HF3FS_MD5_FN __host__ __device__ __forceinline__
#define HF3FS_MD5_UNROLL _Pragma("unroll")
#define HF3FS_MD5_ROLLED _Pragma("unroll 1")
#else
#define HF3FS_MD5_FN inline
#define HF3FS_MD5_UNROLL
#define HF3FS_MD5_ROLLED
#endif

// The load-checked build (loadcheck.h) routes the cursor's segment bytes through its check.
#if defined(HF3FS_CRC_LOAD_CHECK) && defined(__HIP_DEVICE_COMPILE__)
#define HF3FS_MD5_BYTE_OK(a) lc_ok((a), 1, kSiteMd5Byte)
#else
#define HF3FS_MD5_BYTE_OK(a) true
#endif

namespace hf3fs_crc {

HF3FS_MD5_FN void md5_init(uint32_t h[4]) {
  h[0] = 0x67452301u;
  h[1] = 0xefcdab89u;
  h[2] = 0x98badcfeu;
  h[3] = 0x10325476u;
}

#define HF3FS_MD5_F(b, c, d) ((d) ^ ((b) & ((c) ^ (d))))
#define HF3FS_MD5_G(b, c, d) ((c) ^ ((d) & ((b) ^ (c))))
#define HF3FS_MD5_H(b, c, d) ((b) ^ (c) ^ (d))
#define HF3FS_MD5_I(b, c, d) ((c) ^ ((b) | ~(d)))
#define HF3FS_MD5_STEP(f, a, b, c, d, x, t, s)      \
  do {                                              \
    (a) += f((b), (c), (d)) + (x) + (uint32_t)(t);  \
    (a) = (((a) << (s)) | ((a) >> (32 - (s)))) + (b); \
  } while (0)

// One 64-byte block: w[j] is bytes 4j .. 4j+3 of the block, little-endian.
HF3FS_MD5_FN void md5_block(uint32_t h[4], const uint32_t w[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
  HF3FS_MD5_STEP(HF3FS_MD5_F, a, b, c, d, w[0], 0xd76aa478u, 7);
  HF3FS_MD5_STEP(HF3FS_MD5_F, d, a, b, c, w[1], 0xe8c7b756u, 12);
  HF3FS_MD5_STEP(HF3FS_MD5_F, c, d, a, b, w[2], 0x242070dbu, 17);
  HF3FS_MD5_STEP(HF3FS_MD5_F, b, c, d, a, w[3], 0xc1bdceeeu, 22);
  HF3FS_MD5_STEP(HF3FS_MD5_F, a, b, c, d, w[4], 0xf57c0fafu, 7);
  HF3FS_MD5_STEP(HF3FS_MD5_F, d, a, b, c, w[5], 0x4787c62au, 12);
  HF3FS_MD5_STEP(HF3FS_MD5_F, c, d, a, b, w[6], 0xa8304613u, 17);
  HF3FS_MD5_STEP(HF3FS_MD5_F, b, c, d, a, w[7], 0xfd469501u, 22);
  HF3FS_MD5_STEP(HF3FS_MD5_F, a, b, c, d, w[8], 0x698098d8u, 7);
  HF3FS_MD5_STEP(HF3FS_MD5_F, d, a, b, c, w[9], 0x8b44f7afu, 12);
  HF3FS_MD5_STEP(HF3FS_MD5_F, c, d, a, b, w[10], 0xffff5bb1u, 17);
  HF3FS_MD5_STEP(HF3FS_MD5_F, b, c, d, a, w[11], 0x895cd7beu, 22);
  HF3FS_MD5_STEP(HF3FS_MD5_F, a, b, c, d, w[12], 0x6b901122u, 7);
  HF3FS_MD5_STEP(HF3FS_MD5_F, d, a, b, c, w[13], 0xfd987193u, 12);
  HF3FS_MD5_STEP(HF3FS_MD5_F, c, d, a, b, w[14], 0xa679438eu, 17);
  HF3FS_MD5_STEP(HF3FS_MD5_F, b, c, d, a, w[15], 0x49b40821u, 22);

  HF3FS_MD5_STEP(HF3FS_MD5_G, a, b, c, d, w[1], 0xf61e2562u, 5);
  HF3FS_MD5_STEP(HF3FS_MD5_G, d, a, b, c, w[6], 0xc040b340u, 9);
  HF3FS_MD5_STEP(HF3FS_MD5_G, c, d, a, b, w[11], 0x265e5a51u, 14);
  HF3FS_MD5_STEP(HF3FS_MD5_G, b, c, d, a, w[0], 0xe9b6c7aau, 20);
  HF3FS_MD5_STEP(HF3FS_MD5_G, a, b, c, d, w[5], 0xd62f105du, 5);
  HF3FS_MD5_STEP(HF3FS_MD5_G, d, a, b, c, w[10], 0x02441453u, 9);
  HF3FS_MD5_STEP(HF3FS_MD5_G, c, d, a, b, w[15], 0xd8a1e681u, 14);
  HF3FS_MD5_STEP(HF3FS_MD5_G, b, c, d, a, w[4], 0xe7d3fbc8u, 20);
  HF3FS_MD5_STEP(HF3FS_MD5_G, a, b, c, d, w[9], 0x21e1cde6u, 5);
  HF3FS_MD5_STEP(HF3FS_MD5_G, d, a, b, c, w[14], 0xc33707d6u, 9);
  HF3FS_MD5_STEP(HF3FS_MD5_G, c, d, a, b, w[3], 0xf4d50d87u, 14);
  HF3FS_MD5_STEP(HF3FS_MD5_G, b, c, d, a, w[8], 0x455a14edu, 20);
  HF3FS_MD5_STEP(HF3FS_MD5_G, a, b, c, d, w[13], 0xa9e3e905u, 5);
  HF3FS_MD5_STEP(HF3FS_MD5_G, d, a, b, c, w[2], 0xfcefa3f8u, 9);
  HF3FS_MD5_STEP(HF3FS_MD5_G, c, d, a, b, w[7], 0x676f02d9u, 14);
  HF3FS_MD5_STEP(HF3FS_MD5_G, b, c, d, a, w[12], 0x8d2a4c8au, 20);

  HF3FS_MD5_STEP(HF3FS_MD5_H, a, b, c, d, w[5], 0xfffa3942u, 4);
  HF3FS_MD5_STEP(HF3FS_MD5_H, d, a, b, c, w[8], 0x8771f681u, 11);
  HF3FS_MD5_STEP(HF3FS_MD5_H, c, d, a, b, w[11], 0x6d9d6122u, 16);
  HF3FS_MD5_STEP(HF3FS_MD5_H, b, c, d, a, w[14], 0xfde5380cu, 23);
  HF3FS_MD5_STEP(HF3FS_MD5_H, a, b, c, d, w[1], 0xa4beea44u, 4);
  HF3FS_MD5_STEP(HF3FS_MD5_H, d, a, b, c, w[4], 0x4bdecfa9u, 11);
  HF3FS_MD5_STEP(HF3FS_MD5_H, c, d, a, b, w[7], 0xf6bb4b60u, 16);
  HF3FS_MD5_STEP(HF3FS_MD5_H, b, c, d, a, w[10], 0xbebfbc70u, 23);
  HF3FS_MD5_STEP(HF3FS_MD5_H, a, b, c, d, w[13], 0x289b7ec6u, 4);
  HF3FS_MD5_STEP(HF3FS_MD5_H, d, a, b, c, w[0], 0xeaa127fau, 11);
  HF3FS_MD5_STEP(HF3FS_MD5_H, c, d, a, b, w[3], 0xd4ef3085u, 16);
  HF3FS_MD5_STEP(HF3FS_MD5_H, b, c, d, a, w[6], 0x04881d05u, 23);
  HF3FS_MD5_STEP(HF3FS_MD5_H, a, b, c, d, w[9], 0xd9d4d039u, 4);
  HF3FS_MD5_STEP(HF3FS_MD5_H, d, a, b, c, w[12], 0xe6db99e5u, 11);
  HF3FS_MD5_STEP(HF3FS_MD5_H, c, d, a, b, w[15], 0x1fa27cf8u, 16);
  HF3FS_MD5_STEP(HF3FS_MD5_H, b, c, d, a, w[2], 0xc4ac5665u, 23);

  HF3FS_MD5_STEP(HF3FS_MD5_I, a, b, c, d, w[0], 0xf4292244u, 6);
  HF3FS_MD5_STEP(HF3FS_MD5_I, d, a, b, c, w[7], 0x432aff97u, 10);
  HF3FS_MD5_STEP(HF3FS_MD5_I, c, d, a, b, w[14], 0xab9423a7u, 15);
  HF3FS_MD5_STEP(HF3FS_MD5_I, b, c, d, a, w[5], 0xfc93a039u, 21);
  HF3FS_MD5_STEP(HF3FS_MD5_I, a, b, c, d, w[12], 0x655b59c3u, 6);
  HF3FS_MD5_STEP(HF3FS_MD5_I, d, a, b, c, w[3], 0x8f0ccc92u, 10);
  HF3FS_MD5_STEP(HF3FS_MD5_I, c, d, a, b, w[10], 0xffeff47du, 15);
  HF3FS_MD5_STEP(HF3FS_MD5_I, b, c, d, a, w[1], 0x85845dd1u, 21);
  HF3FS_MD5_STEP(HF3FS_MD5_I, a, b, c, d, w[8], 0x6fa87e4fu, 6);
  HF3FS_MD5_STEP(HF3FS_MD5_I, d, a, b, c, w[15], 0xfe2ce6e0u, 10);
  HF3FS_MD5_STEP(HF3FS_MD5_I, c, d, a, b, w[6], 0xa3014314u, 15);
  HF3FS_MD5_STEP(HF3FS_MD5_I, b, c, d, a, w[13], 0x4e0811a1u, 21);
  HF3FS_MD5_STEP(HF3FS_MD5_I, a, b, c, d, w[4], 0xf7537e82u, 6);
  HF3FS_MD5_STEP(HF3FS_MD5_I, d, a, b, c, w[11], 0xbd3af235u, 10);
  HF3FS_MD5_STEP(HF3FS_MD5_I, c, d, a, b, w[2], 0x2ad7d2bbu, 15);
  HF3FS_MD5_STEP(HF3FS_MD5_I, b, c, d, a, w[9], 0xeb86d391u, 21);
  h[0] += a;
  h[1] += b;
  h[2] += c;
  h[3] += d;
}

#undef HF3FS_MD5_STEP
#undef HF3FS_MD5_F
#undef HF3FS_MD5_G
#undef HF3FS_MD5_H
#undef HF3FS_MD5_I

// ---- the work of one file in one call ----------------------------------------------------------------
// Blocks the call compresses for a file that enters with tail_len unhashed bytes and brings
// new_bytes more: the whole blocks of both, and with FINAL the one or two blocks of the padding
// (0x80, zeros up to 56 mod 64, the 64-bit bit length: two blocks when 56 or more bytes are left).
HF3FS_MD5_FN uint64_t md5_call_blocks(uint32_t tail_len, uint64_t new_bytes, bool final) {
  const uint64_t m = (uint64_t)tail_len + new_bytes;
  return m / 64 + (final ? ((m % 64) < 56 ? 1u : 2u) : 0u);
}

// Files are bucketed by block count, a few sub-buckets per octave, the longest first: bucket 0
// holds the largest counts, kMd5Buckets - 1 the files with no block at all.
constexpr uint32_t kMd5Buckets = 256;
HF3FS_MD5_FN uint32_t md5_bucket(uint64_t blocks) {
  if (blocks == 0) return kMd5Buckets - 1;
  uint32_t o = 0;
  for (uint64_t v = blocks; v >>= 1;) ++o;                                         // floor(log2), 0..63
  const uint32_t sub = o >= 2 ? (uint32_t)(blocks >> (o - 2)) & 3u : (uint32_t)(blocks << (2 - o)) & 3u;
  const uint32_t at = 4 * o + sub;  // a call's count is below 2^58 + 2: at <= 235
  return kMd5Buckets - 2 - (at < kMd5Buckets - 2 ? at : kMd5Buckets - 2);
}

// ---- the cursor ----------------------------------------------------------------------------------------
// Position in one file's stream of one call.  Between calls of md5_stream_* the cursor is settled:
// either every segment is consumed (seg == seg_end) or the current one has rem > 0 bytes left.
struct Md5Stream {
  const hf3fs_crc_md5_seg* segs;  // the batch's segment records
  uint64_t seg, seg_end;          // current segment, end of the file's segments
  uint64_t addr;                  // address of the current segment's next byte, 0 = a hole
  uint64_t rem;                   // bytes left in the current segment
  const uint8_t* tail;            // incoming tail (hf3fs_crc_md5_state.tail), read while tail_pos < tail_len
  uint32_t tail_len, tail_pos;
  uint32_t pad_pos;               // padding bytes produced so far
  uint64_t total;                 // message bytes before the position, earlier calls' included
};

HF3FS_MD5_FN void md5_stream_settle(Md5Stream& s) {
  s.rem = 0;
  s.addr = 0;
  while (s.seg < s.seg_end) {
    const uint64_t len = s.segs[s.seg].length;
    if (len) {
      s.rem = len;
      s.addr = s.segs[s.seg].data;
      return;
    }
    ++s.seg;
  }
}

// state == nullptr (INIT): an empty message so far.  Else the state's total and tail.
HF3FS_MD5_FN void md5_stream_open(Md5Stream& s, const hf3fs_crc_md5_seg* segs, uint64_t seg, uint64_t seg_end,
                                  const hf3fs_crc_md5_state* state) {
  s.segs = segs;
  s.seg = seg;
  s.seg_end = seg_end < seg ? seg : seg_end;
  s.tail = state ? state->tail : nullptr;
  s.tail_len = state ? (uint32_t)(state->total % 64) : 0u;
  s.tail_pos = 0;
  s.pad_pos = 0;
  s.total = state ? state->total - s.tail_len : 0u;
  md5_stream_settle(s);
}

// The next byte of the stream.  Past the message: with pad the padding (the caller stops at the
// block count of md5_call_blocks), without it zeros (the rest of an outgoing tail).
HF3FS_MD5_FN uint32_t md5_stream_byte(Md5Stream& s, bool pad) {
  if (s.tail_pos < s.tail_len) {
    ++s.total;
    return s.tail[s.tail_pos++];
  }
  if (s.seg < s.seg_end) {
    uint32_t b = 0;
    if (s.addr) {
      if (HF3FS_MD5_BYTE_OK(s.addr)) b = *(const uint8_t*)(uintptr_t)s.addr;
      ++s.addr;
    }
    ++s.total;
    if (--s.rem == 0) {
      ++s.seg;
      md5_stream_settle(s);
    }
    return b;
  }
  if (!pad) return 0;
  const uint32_t k = s.pad_pos++;
  const uint32_t m = (uint32_t)(s.total % 64);
  const uint32_t zeros_end = (m < 56 ? 56u : 120u) - m;  // 0x80 and zeros fill [0, zeros_end)
  if (k == 0) return 0x80;
  if (k < zeros_end) return 0;
  return (uint32_t)((s.total * 8) >> (8 * ((k - zeros_end) & 7))) & 0xFF;
}

// The next 64 bytes, byte by byte: any position (tail, segment boundaries, holes, padding).
// Each new word enters at w[15] while the others move down one place: every index is a constant,
// so on the device the block stays in registers without the loop being unrolled 64 times.
HF3FS_MD5_FN void md5_stream_block(Md5Stream& s, bool pad, uint32_t w[16]) {
HF3FS_MD5_UNROLL
  for (int i = 0; i < 16; ++i) w[i] = 0;
HF3FS_MD5_ROLLED
  for (int j = 0; j < 16; ++j) {
    uint32_t word = 0;
HF3FS_MD5_ROLLED
    for (int b = 0; b < 32; b += 8) word |= md5_stream_byte(s, pad) << b;
HF3FS_MD5_UNROLL
    for (int i = 0; i < 15; ++i) w[i] = w[i + 1];
    w[15] = word;
  }
}

// Do the next 64 bytes lie in one segment (no tail byte left, none of the padding)?
HF3FS_MD5_FN bool md5_stream_run64(const Md5Stream& s) {
  return s.tail_pos >= s.tail_len && s.seg < s.seg_end && s.rem >= 64;
}

// Step over 64 bytes of the current segment that the caller took itself (md5_stream_run64 held).
HF3FS_MD5_FN void md5_stream_skip64(Md5Stream& s) {
  if (s.addr) s.addr += 64;
  s.total += 64;
  s.rem -= 64;
  if (s.rem == 0) {
    ++s.seg;
    md5_stream_settle(s);
  }
}

// A block that starts r = addr % 16 bytes into g: the five 16-byte granules from addr - r on, as
// 20 little-endian words (g[16..19] are not looked at for r == 0).  Every granule holds at least
// one byte of the block, so loading them never leaves the pages the block lies in.
HF3FS_MD5_FN void md5_words_from_granules(const uint32_t g[20], uint32_t r, uint32_t w[16]) {
  // Whole words move by two bitwise selects (masks, so that no index depends on r), bytes by a
  // funnel shift.
  const uint32_t by2 = (r & 8) ? ~0u : 0u, by1 = (r & 4) ? ~0u : 0u;
  const uint32_t sh = (r & 3) * 8;
  uint32_t t[18], u[17];
HF3FS_MD5_UNROLL
  for (int i = 0; i < 18; ++i) t[i] = (g[i + 2] & by2) | (g[i] & ~by2);
HF3FS_MD5_UNROLL
  for (int i = 0; i < 17; ++i) u[i] = (t[i + 1] & by1) | (t[i] & ~by1);
HF3FS_MD5_UNROLL
  for (int i = 0; i < 16; ++i) w[i] = (uint32_t)((((uint64_t)u[i + 1] << 32) | u[i]) >> sh);
}

// ---- the ends of a call ----------------------------------------------------------------------------------
// MD5_Final's byte order: h[0] first, each word little-endian.
HF3FS_MD5_FN void md5_digest_bytes(const uint32_t h[4], uint8_t out[16]) {
  for (int i = 0; i < 16; ++i) out[i] = (uint8_t)(h[i >> 2] >> (8 * (i & 3)));
}

// The state a call without FINAL leaves: s stands behind the call's last whole block; the bytes
// left (fewer than 64) become the tail, the rest of the tail is zero.
HF3FS_MD5_FN void md5_state_out(Md5Stream& s, const uint32_t h[4], uint32_t h_out[4], uint64_t* total_out,
                                uint32_t tail_words[16]) {
  md5_stream_block(s, false, tail_words);
  for (int i = 0; i < 4; ++i) h_out[i] = h[i];
  *total_out = s.total;
}

}  // namespace hf3fs_crc
