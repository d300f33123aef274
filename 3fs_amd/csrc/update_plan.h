// update_plan.h -- the planner arithmetic of the update path, plain C++ that both the device
// compiler and a host compiler take.  Every address and every count of the path is decided here:
// what ChunkReplica::update / the chunk engine make of one IO (derive), the hash jobs before and
// after the write (pre_lens, plan_jobs), which byte ranges the apply moves and where (plan_ranges),
// where the one-shot apply cuts a range (pieces_of, piece_span) and where the ticketed apply does
// (piece_bytes, piece_count, piece_bounds).  Who calls what:
//   derive, pre_lens       prep (prep_one and the runs workgroup), finalize, the fused kernel;
//   plan_jobs              prep_one, which only stores the four jobs;
//   plan_ranges, pieces_of k_update_prep<RPI>, in place (RPI = 2: image == chunk, the payload and
//                          gap records) and with destinations (RPI = kPlanRanges);
//   piece_count / _bounds  k_update_prep<2>'s ticketed emission;
//   piece_span             the one-shot apply (one_shot_piece).
// The kernels keep no address arithmetic of their own, so the rules "every piece lies inside
// [dst, dst + out_size), the pieces of an IO tile its image exactly once, every job reads inside
// its buffer" are checked on the CPU for every entry point (tests/cpp/fuzz_cow_planner.cpp, under
// ASan + UBSan).
#pragma once
#include <stdint.h>

#include "../../include/hf3fs_crc.h"
#include "gf2.h"

#ifdef __HIPCC__
#define HF3FS_PLAN_FN __host__ __device__ __forceinline__
#else
#define HF3FS_PLAN_FN inline
#endif

namespace hf3fs_crc {

struct Eff {
  uint32_t s0, s1;          // chunk size before / after
  uint32_t off, len;        // the UpdateIO as updateChecksum sees it (truncate: off = size, len = 0)
  uint32_t wval, cval;      // write / chunk checksum values
  uint32_t zero_from, zero_to;
  uint8_t wtype, ctype;
  uint8_t kase;             // 1 none/empty, 2 reuse, 3 append-combine, 4 recompute
  bool delta;               // case 4 via the delta identity
  bool verify;              // payload checksum must be verified
  bool te;                  // truncate / extend
  bool ok;                  // IO is well formed
  bool engine;              // chunk-engine semantics (HF3FS_UPDATE_FLAG_ENGINE)
  bool hash_payload;        // the payload job must run (verify, or engine without_checksum)
  bool sync;                // a resync write (HF3FS_UPDATE_FLAG_SYNCING): size = length, nothing old is kept
};

HF3FS_PLAN_FN Eff derive(const hf3fs_crc_update_io& io, uint32_t max_len, uint8_t type, int mode) {
  Eff e{};
  e.s0 = io.chunk_size;
  e.ctype = io.chunk_checksum_type;
  e.cval = io.chunk_checksum;
  e.ok = true;
  e.zero_from = e.zero_to = 0;
  e.sync = (io.flags & HF3FS_UPDATE_FLAG_SYNCING) != 0;
  // The batch hashes bytes in `type`: a write's payload and (when the types differ)
  // its prefix / suffix recompute, ChunkReplica.cc:340,356-392 -- the chunk's stored
  // type may differ for a write; a truncate / extend hashes in the chunk's type.
  if (io.chunk_size > max_len || e.ctype > kTypeCrc32) e.ok = false;
  if (io.update_type != HF3FS_UPDATE_WRITE && e.ctype != kTypeNone && e.ctype != type) e.ok = false;
  // isSyncing is the whole-chunk write of resync (ReliableForwarding.cc:179-206): offset 0 only
  if (e.sync && (io.update_type != HF3FS_UPDATE_WRITE || io.offset != 0)) e.ok = false;
  if (io.update_type == HF3FS_UPDATE_WRITE) {
    // ChunkReplica.cc:139-145: offset >= chunkSize || offset + length > chunkSize -> kInvalidArg
    if (io.offset >= max_len || (uint64_t)io.offset + io.length > max_len) e.ok = false;
    if (io.length && !io.payload) e.ok = false;
    if (io.write_checksum_type != kTypeNone && io.write_checksum_type != type) e.ok = false;
    e.off = io.offset;
    e.len = io.length;
    e.s1 = e.s0 > io.offset + io.length ? e.s0 : io.offset + io.length;
    if (e.sync) e.s1 = io.offset + io.length;  // meta.size = writeIO.length (ChunkReplica.cc:289; chunk.rs:112)
    if (io.offset > e.s0) {
      e.zero_from = e.s0;
      e.zero_to = io.offset;
    }
    e.wtype = io.write_checksum_type;
    e.wval = io.write_checksum;
    e.verify = e.wtype != kTypeNone && e.len != 0;
  } else if (io.update_type == HF3FS_UPDATE_TRUNCATE || io.update_type == HF3FS_UPDATE_EXTEND) {
    const uint32_t target = io.length;  // ChunkReplica.cc:255-269
    if (target > max_len) e.ok = false;
    if (target <= e.s0) {
      e.s1 = io.update_type == HF3FS_UPDATE_TRUNCATE ? target : e.s0;
    } else {
      e.s1 = target;
      e.zero_from = e.s0;
      e.zero_to = target;
    }
    e.te = true;
    e.wtype = e.ctype;  // create(meta.checksumType, nullptr, 0) (:328-332)
    e.wval = e.ctype == kTypeNone ? 0u : ~0u;
    e.off = e.s1;
    e.len = 0;
  } else {
    e.ok = false;
  }
  e.hash_payload = e.verify;
  const bool is_append = io.offset == e.s0;  // :243, before the write
  if (io.flags & HF3FS_UPDATE_FLAG_ENGINE) {
    // ChunkEngine.cc:41-45: a CRC32C write checksum is verified (engine.rs:297-311), anything else
    // is "without_checksum" -- hashed and used.  The stored checksum is always the CRC32C of the
    // chunk bytes (chunk.rs:89-281), an empty chunk included (~0 raw).
    e.engine = true;
    if (type != kTypeCrc32c) e.ok = false;
    e.ctype = kTypeCrc32c;
    if (e.s0 == 0) e.cval = ~0u;
    if (!e.te) {
      e.verify = io.write_checksum_type == kTypeCrc32c && e.len != 0;
      e.hash_payload = e.len != 0;
      if (e.wtype != kTypeCrc32c) e.ok = e.ok && io.write_checksum_type == kTypeNone;
    }
    e.wtype = kTypeCrc32c;
    if (e.te) e.wval = ~0u;
    if (e.s1 == 0)
      e.kase = 1;
    else if (e.off == 0 && e.len == e.s1)
      e.kase = 2;  // copy_on_write skip_read: reuse (chunk.rs:110,150-155); every syncing write
    else if (e.s0 > 0 && is_append)
      e.kase = 3;  // direct / indirect append: combine (chunk.rs:229,266)
    else
      e.kase = 4;
    e.delta = e.kase == 4 && mode == HF3FS_UPDATE_MODE_DELTA;
    return e;
  }
  const bool combine = e.s0 > 0 && is_append;
  if (e.wtype == kTypeNone || e.s1 == 0)
    e.kase = 1;
  else if (e.off == 0 && e.len == e.s1)
    e.kase = 2;  // (every syncing write with a typed checksum: ChunkReplica.cc:337-339 with size = length)
  else if (e.wtype == e.ctype && combine)
    e.kase = 3;
  else
    e.kase = 4;
  e.delta = e.kase == 4 && mode == HF3FS_UPDATE_MODE_DELTA && (e.s0 == 0 || e.ctype == e.wtype);
  return e;
}

// The address IO i's new image is written at: its chunk (in place) unless the caller gave a
// destination of its own (hf3fs_crc_update_cow_batch: d_dst[i], 0 = none).
HF3FS_PLAN_FN uint64_t plan_image(uint64_t chunk, uint64_t dst) { return dst ? dst : chunk; }

// Lengths of an IO's two pre jobs: the payload (verify) and, for the delta method, the old
// bytes under the write or the truncated tail.  Only the IO's input fields and Eff.
HF3FS_PLAN_FN void pre_lens(const Eff& e, uint64_t& l0, uint64_t& l1) {
  l0 = l1 = 0;
  if (!e.ok) return;
  if (e.hash_payload) l0 = e.len;
  if (e.kase == 4 && e.delta) {
    if (!e.te && e.off < e.s0)
      l1 = (e.off + e.len < e.s0 ? e.off + e.len : e.s0) - e.off;
    else if (e.te && e.s1 < e.s0)
      l1 = e.s0 - e.s1;
  }
}

// The hash jobs of one IO whose image is written at `image`.  Before the write ("pre"):
//   [0] payload    payload[0, len)
//   [1] old bytes  chunk[off, min(off + len, s0)), a truncate's chunk[s1, s0)   (delta method)
// After it ("post", the reference method's recompute, ChunkReplica.cc:356-389):
//   [2] prefix     image[0, off)       (holds the zero-filled gap of a write past the size)
//   [3] suffix     image[min(off + len, s1), s1)
// The pre jobs read the committed chunk whatever the image; a job of length 0 has address 0, and
// an IO that is not ok has none.
struct PlanJob {
  uint64_t addr, len;
};
enum { kJobPayload = 0, kJobOld = 1, kJobPrefix = 2, kJobSuffix = 3, kPlanJobs = 4 };
struct PlanJobs {
  PlanJob job[kPlanJobs];
};

HF3FS_PLAN_FN PlanJobs plan_jobs(const hf3fs_crc_update_io& io, const Eff& e, uint64_t image) {
  PlanJobs J{};
  pre_lens(e, J.job[kJobPayload].len, J.job[kJobOld].len);
  if (J.job[kJobPayload].len) J.job[kJobPayload].addr = io.payload;
  if (J.job[kJobOld].len) J.job[kJobOld].addr = io.chunk + (e.te ? e.s1 : e.off);
  if (e.ok && e.kase == 4 && !e.delta) {
    const uint32_t suffix_start = e.off + e.len < e.s1 ? e.off + e.len : e.s1;
    J.job[kJobPrefix] = PlanJob{image, e.off};
    J.job[kJobSuffix] = PlanJob{image + suffix_start, e.s1 - suffix_start};
  }
  return J;
}

// The byte ranges the apply moves for one IO whose image is written at `image`:
//   [0] payload  image[off, off + len)            <- payload
//   [1] gap      image[zero_from, zero_to)        <- 0   (write past the size; an extend's extension)
//   [2] prefix   image[0, min(off, s0))           <- chunk   (truncate / extend: [0, min(s0, s1)))
//   [3] suffix   image[min(off + len, s0), s0)    <- chunk
// [2] and [3] only out of place (image != chunk) and never for a syncing write, which keeps no
// old byte.  The four are disjoint and tile [0, s1) of an out-of-place image exactly (for a
// syncing write [0, length)); an IO that is not ok has none.  A range of length 0 has no piece.
struct PlanRange {
  uint64_t dst, src;
  uint32_t len;
};
enum { kPlanPayload = 0, kPlanGap = 1, kPlanPrefix = 2, kPlanSuffix = 3, kPlanRanges = 4 };

HF3FS_PLAN_FN void plan_ranges(const hf3fs_crc_update_io& io, const Eff& e, uint64_t image, PlanRange* r) {
  for (int k = 0; k < kPlanRanges; ++k) r[k] = PlanRange{0, 0, 0};
  if (!e.ok) return;
  if (!e.te && e.len) r[kPlanPayload] = PlanRange{image + e.off, io.payload, e.len};
  if (e.zero_to > e.zero_from) r[kPlanGap] = PlanRange{image + e.zero_from, 0, e.zero_to - e.zero_from};
  if (image == io.chunk || e.sync) return;
  if (e.te) {
    const uint32_t keep = e.s0 < e.s1 ? e.s0 : e.s1;
    if (keep) r[kPlanPrefix] = PlanRange{image, io.chunk, keep};
    return;
  }
  const uint32_t pre = e.off < e.s0 ? e.off : e.s0;
  const uint32_t end = e.off + e.len;  // (<= max_len: no wrap)
  const uint32_t suf = end < e.s0 ? end : e.s0;
  if (pre) r[kPlanPrefix] = PlanRange{image, io.chunk, pre};
  if (e.s0 > suf) r[kPlanSuffix] = PlanRange{image + suf, io.chunk + suf, e.s0 - suf};
}

// One-shot apply pieces of a range: cut at every 2^shift-aligned destination address.
HF3FS_PLAN_FN uint32_t pieces_of(uint64_t dst, uint64_t len, uint32_t shift) {
  if (!len) return 0;
  const uint64_t m = (uint64_t(1) << shift) - 1;
  return (uint32_t)(((dst & m) + len + m) >> shift);
}

// Piece j (< pieces_of) of the range: destination bytes [a, e).
HF3FS_PLAN_FN void piece_span(uint64_t dst, uint64_t len, uint32_t shift, uint64_t j, uint64_t& a, uint64_t& e) {
  const uint64_t P = uint64_t(1) << shift;
  const uint64_t cut = (dst & ~(P - 1)) + (j << shift);
  a = cut > dst ? cut : dst;
  e = cut + P < dst + len ? cut + P : dst + len;
}

// Ticketed apply pieces of a range of len bytes at dst: at most `pieces` even shares of at least
// piece_min bytes, cut at 16-byte aligned destination addresses.  With h = dst & 15 and ps =
// piece_bytes, piece j = [max(0, j ps - h), min(len, (j + 1) ps - h)).  len <= pieces * ps and
// ps > 15, so a range has at most pieces + 1 of them (the + 1 is the alignment of the cuts).
HF3FS_PLAN_FN uint64_t piece_bytes(uint64_t len, uint32_t pieces, uint32_t piece_min) {
  const uint64_t even = ((len + pieces - 1) / pieces + 15) & ~uint64_t(15);
  return even > piece_min ? even : piece_min;
}
HF3FS_PLAN_FN uint32_t piece_count(uint64_t dst, uint64_t len, uint32_t pieces, uint32_t piece_min) {
  if (!len) return 0;
  const uint64_t ps = piece_bytes(len, pieces, piece_min);
  return (uint32_t)(((dst & 15) + len + ps - 1) / ps);
}
// Piece j (< piece_count) of the range: bytes [a, b) of it.
HF3FS_PLAN_FN void piece_bounds(uint64_t dst, uint64_t len, uint32_t j, uint32_t pieces, uint32_t piece_min,
                                uint64_t& a, uint64_t& b) {
  const uint64_t ps = piece_bytes(len, pieces, piece_min), h = dst & 15;
  a = j ? (uint64_t)j * ps - h : 0;
  const uint64_t b0 = (uint64_t)(j + 1) * ps - h;
  b = b0 < len ? b0 : len;
}

// Piece-table entries one IO can need, in place (payload + gap) and with a destination (all four
// ranges).  A range of L bytes has at most floor((L + 2 P - 2) / P) <= L / P + 2 pieces, and the
// ranges of an IO are disjoint inside [0, max_len), so k ranges take at most max_len / P + 2 k.
HF3FS_PLAN_FN uint64_t plan_piece_bound(uint32_t max_len, uint32_t shift, uint32_t ranges) {
  return ((uint64_t)max_len >> shift) + 2 * (uint64_t)ranges;
}

}  // namespace hf3fs_crc
