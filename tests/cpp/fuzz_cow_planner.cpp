// fuzz_cow_planner.cpp -- the update path's planner (3fs_amd/csrc/update_plan.h) on the CPU, built
// with -fsanitize=address,undefined (tests/test_cow_planner_sanitized.py).  For a few hundred
// thousand random IOs it enumerates every range record and every one-shot piece exactly as the
// kernels do (derive -> plan_ranges -> pieces_of -> piece_span), plays each piece into a byte map of
// the image's neighbourhood and compares the map with a model written from the specification:
//   out of place, status OK: image[0, out_size) = old bytes outside the write, gap zero-fill, payload,
//                            zero extension; nothing at or beyond out_size, nothing before the image;
//   in place:                only the payload and the zero-filled gap are written;
//   invalid IOs:             nothing (a failed payload verify is the apply kernel's business: every
//                            record of the IO must carry the verify bit's condition, checked here).
// Every byte is written at most once, and the piece counts stay inside plan_piece_bound.
// The in-place records of hf3fs_crc_update_batch are literally plan_ranges(..., image == chunk)
// -- k_update_prep<2> has no lines of its own for them -- so the in-place model check covers
// that kernel's addresses too.  Beside the records, for every IO:
//   jobs      plan_jobs, the four hash jobs prep stores: the payload job is [payload, payload +
//             length), the old-byte job lies inside [chunk, chunk + s0), both post jobs inside
//             [image, image + s1), and an IO that is not ok has none;
//   tickets   the ticketed apply's cuts (piece_count / piece_bounds) for pieces in [1, 64] and
//             piece_min a multiple of 1 KiB (the ranges options.cc admits), every destination
//             residue mod 16, lengths around 0, 16, piece_min and pieces * piece_min: the pieces
//             tile [0, len) exactly once and in order, every cut but the first lies on a 16-byte
//             aligned destination address, and piece_count <= pieces + 1 -- the bound the record
//             array's size rests on (update_record_cap).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../3fs_amd/csrc/update_plan.h"

using namespace hf3fs_crc;

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1Dull;
}
uint32_t below(uint32_t n) { return n ? (uint32_t)(rnd() % n) : 0; }

[[noreturn]] void die(const char* what, uint64_t it, const hf3fs_crc_update_io& io, uint64_t image, uint32_t shift,
                      long long x) {
  std::printf("{\"fuzz_cow_planner\":\"FAIL\",\"what\":\"%s\",\"iteration\":%llu,\"type\":%u,\"flags\":%u,"
              "\"chunk\":%llu,\"image\":%llu,\"payload\":%llu,\"offset\":%u,\"length\":%u,\"chunk_size\":%u,"
              "\"shift\":%u,\"x\":%lld}\n",
              what, (unsigned long long)it, io.update_type, io.flags, (unsigned long long)io.chunk,
              (unsigned long long)image, (unsigned long long)io.payload, io.offset, io.length, io.chunk_size, shift, x);
  std::exit(1);
}

// byte tags: where a written byte came from
constexpr uint32_t kNone = 0, kZero = 1u << 30, kOld = 2u << 30, kPay = 3u << 30;
constexpr uint32_t kGuard = 64;  // bytes of the map before the image and after max_len

// a length near 0, near a cut line of the destination, or anywhere
uint32_t pick_len(uint32_t limit, uint32_t P, uint64_t at) {
  if (!limit) return 0;
  uint32_t v;
  switch (below(8)) {
    case 0: v = below(3); break;
    case 1: v = below(40); break;
    case 2: v = 15 + below(4); break;
    case 3: {  // ends within +-2 of a destination cut line
      const uint64_t to_line = (P - (at & (P - 1))) & (P - 1);
      v = (uint32_t)to_line + P * below(3) + below(5) - 2;
      break;
    }
    case 4: v = P * (1 + below(2)) + below(5) - 2; break;
    case 5: v = limit - below(3 < limit ? 3 : limit); break;
    default: v = below(600);
  }
  if ((int32_t)v < 0) v = 0;
  return v > limit ? limit : v;
}

[[noreturn]] void die_ticket(const char* what, uint64_t it, uint64_t dst, uint64_t len, uint32_t pieces,
                             uint32_t piece_min, long long x) {
  std::printf("{\"fuzz_cow_planner\":\"FAIL\",\"what\":\"%s\",\"iteration\":%llu,\"dst\":%llu,\"len\":%llu,"
              "\"pieces\":%u,\"piece_min\":%u,\"x\":%lld}\n",
              what, (unsigned long long)it, (unsigned long long)dst, (unsigned long long)len, pieces, piece_min, x);
  std::exit(1);
}

// The ticketed apply's cuts of one range, as k_update_prep<2> emits them; returns the piece count.
uint32_t check_tickets(uint64_t it, uint64_t dst, uint64_t len, uint32_t pieces, uint32_t piece_min) {
  const uint32_t np = piece_count(dst, len, pieces, piece_min);
  if ((len == 0) != (np == 0)) die_ticket("empty range with tickets", it, dst, len, pieces, piece_min, np);
  if (np > pieces + 1) die_ticket("ticket bound", it, dst, len, pieces, piece_min, np);
  uint64_t prev = 0;
  for (uint32_t j = 0; j < np; ++j) {
    uint64_t a, b;
    piece_bounds(dst, len, j, pieces, piece_min, a, b);
    if (a != prev || b <= a || b > len) die_ticket("tickets do not tile the range", it, dst, len, pieces, piece_min, j);
    if (j && ((dst + a) & 15)) die_ticket("ticket cut off a 16-byte line", it, dst, len, pieces, piece_min, j);
    prev = b;
  }
  if (prev != len) die_ticket("tickets short of the range", it, dst, len, pieces, piece_min, (long long)prev);
  return np;
}

// a length around 0, 16, piece_min or pieces * piece_min, or anywhere below 2^32
uint64_t pick_ticket_len(uint32_t pieces, uint32_t piece_min) {
  uint64_t v;
  switch (below(6)) {
    case 0: v = below(3); break;
    case 1: v = 14 + below(20); break;
    case 2: v = (uint64_t)piece_min * (1 + below(2)) + below(35) - 17; break;
    case 3: v = (uint64_t)pieces * piece_min + below(35) - 17; break;
    case 4: v = (uint64_t)pieces * piece_min * (1 + below(3)) + below(1u << 20); break;
    default: v = rnd() >> (32 + below(32));
  }
  return v > 0xffffffffull ? 0xffffffffull : v;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t iterations = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 300000;
  uint64_t n_ok = 0, n_bad = 0, n_pieces = 0, n_oop = 0, n_sync = 0, n_big = 0;
  uint64_t n_pre_jobs = 0, n_post_jobs = 0, n_tickets = 0, n_ticket_full = 0;  // (full: a range of pieces + 1 tickets)
  uint64_t residues[3] = {0, 0, 0};  // bit r set: residue r mod 16 seen for chunk / image / payload
  std::vector<uint32_t> map, model;
  for (uint64_t it = 0; it < iterations; ++it) {
    const uint32_t shift = 12 + below(3);  // 4 / 8 / 16 KiB pieces
    const uint32_t P = 1u << shift;
    const bool big = it % 64 == 0;  // most IOs are short and sit around a cut line; some span pieces
    const uint32_t max_len = big ? P * (1 + below(3)) + below(200) + 1 : 700 + below(800);
    n_big += big;
    hf3fs_crc_update_io io{};
    // addresses: any residue mod 16, the chunk / image placed a few bytes either side of a cut line
    const uint64_t near = below(2) ? P - below(40) : below(P);
    io.chunk = (uint64_t(1) << 40) + (uint64_t)below(1000) * (4u << 20) + near;
    uint64_t dst = 0;  // d_dst[i]
    switch (below(8)) {
      case 0: dst = 0; break;
      case 1: dst = io.chunk; break;
      default: dst = (uint64_t(1) << 41) + (uint64_t)below(1000) * (4u << 20) + (below(2) ? P - below(40) : below(P));
    }
    io.payload = (uint64_t(1) << 42) + below(1u << 20);
    const uint8_t type = below(2) ? kTypeCrc32c : kTypeCrc32;
    const int mode = (int)below(2);
    io.chunk_checksum_type = below(16) ? type : (uint8_t)below(4);
    io.chunk_checksum = (uint32_t)rnd();
    io.write_checksum_type = below(4) ? type : (uint8_t)below(4);
    io.write_checksum = (uint32_t)rnd();
    if (below(3) == 0) io.flags |= HF3FS_UPDATE_FLAG_ENGINE;
    if (below(6) == 0) io.flags |= HF3FS_UPDATE_FLAG_SYNCING;
    const uint64_t image = plan_image(io.chunk, dst);
    io.chunk_size = pick_len(max_len, P, image);
    const uint32_t kind = below(16);
    if (kind < 11) {
      io.update_type = HF3FS_UPDATE_WRITE;
      io.offset = (io.flags & HF3FS_UPDATE_FLAG_SYNCING) && below(8) ? 0 : below(4) == 0 ? io.chunk_size : pick_len(max_len - 1, P, image);
      io.length = pick_len(max_len - io.offset, P, image + io.offset);
      if (below(40) == 0) io.offset = max_len + below(3);                    // ChunkReplica.cc:139-145
      if (below(40) == 0) io.length = max_len - (io.offset < max_len ? io.offset : 0) + 1 + below(3);
      if (below(60) == 0) io.payload = 0;
    } else if (kind < 15) {
      io.update_type = kind < 13 ? HF3FS_UPDATE_TRUNCATE : HF3FS_UPDATE_EXTEND;
      io.length = pick_len(max_len, P, image);
      if (below(40) == 0) io.length = max_len + 1 + below(3);
      io.payload = 0;
    } else {
      io.update_type = (uint8_t)below(16);  // mostly unknown types
    }
    if (below(50) == 0) io.chunk_size = max_len + 1 + below(5);
    residues[0] |= 1ull << (io.chunk & 15);
    residues[1] |= 1ull << (image & 15);
    residues[2] |= 1ull << (io.payload & 15);

    // ---- the model, from the specification -----------------------------------------------------
    const bool engine = io.flags & HF3FS_UPDATE_FLAG_ENGINE, sync = io.flags & HF3FS_UPDATE_FLAG_SYNCING;
    const bool write = io.update_type == HF3FS_UPDATE_WRITE;
    const bool te = io.update_type == HF3FS_UPDATE_TRUNCATE || io.update_type == HF3FS_UPDATE_EXTEND;
    bool ok = write || te;
    if (io.chunk_size > max_len || io.chunk_checksum_type > kTypeCrc32) ok = false;
    if (write) {
      if (io.offset >= max_len || (uint64_t)io.offset + io.length > max_len) ok = false;
      if (io.length && !io.payload) ok = false;
      if (io.write_checksum_type != kTypeNone && io.write_checksum_type != type) ok = false;
      if (sync && io.offset != 0) ok = false;
    } else {
      if (io.length > max_len) ok = false;
      if (io.chunk_checksum_type != kTypeNone && io.chunk_checksum_type != type) ok = false;
      if (sync) ok = false;
    }
    if (engine && type != kTypeCrc32c) ok = false;
    const bool oop = image != io.chunk;
    const uint32_t s0 = io.chunk_size;
    uint32_t out_size = s0;
    model.assign(max_len + 2 * kGuard, kNone);
    if (ok) {
      if (write) {
        const uint32_t end = io.offset + io.length;
        out_size = sync ? io.length : (s0 > end ? s0 : end);
        for (uint32_t x = 0; x < out_size; ++x) {
          uint32_t tag;
          if (x >= io.offset && x < end) tag = kPay | (x - io.offset);
          else if (x >= s0) tag = kZero;   // the gap between the old size and the write
          else tag = oop ? (kOld | x) : kNone;  // an old byte: copied out of place, left alone in place
          model[kGuard + x] = tag;
        }
      } else {
        const uint32_t target = io.length;
        out_size = target > s0 ? target : (io.update_type == HF3FS_UPDATE_TRUNCATE ? target : s0);
        for (uint32_t x = 0; x < out_size; ++x) model[kGuard + x] = x >= s0 ? kZero : (oop ? (kOld | x) : kNone);
      }
    }
    (ok ? n_ok : n_bad)++;
    n_oop += ok && oop;
    n_sync += ok && sync;

    // ---- the planner, as the kernels run it ---------------------------------------------------
    const Eff e = derive(io, max_len, type, mode);
    if (e.ok != ok) die("derive.ok", it, io, image, shift, e.ok);
    if (ok && e.s1 != out_size) die("derive.s1", it, io, image, shift, e.s1);
    if (ok && write) {
      const bool want_verify = io.length != 0 && (engine ? io.write_checksum_type == kTypeCrc32c
                                                         : io.write_checksum_type != kTypeNone);
      if (e.verify != want_verify) die("derive.verify", it, io, image, shift, e.verify);
    }
    PlanRange R[kPlanRanges];
    plan_ranges(io, e, image, R);
    map.assign(max_len + 2 * kGuard, kNone);
    uint64_t pieces_io = 0;
    const uint32_t nranges = oop ? kPlanRanges : 2;
    for (int k = 0; k < kPlanRanges; ++k) {
      const uint32_t np = pieces_of(R[k].dst, R[k].len, shift);
      if ((R[k].len == 0) != (np == 0)) die("empty range with pieces", it, io, image, shift, k);
      if (!oop && k >= 2 && R[k].len) die("old-byte record of an in-place IO", it, io, image, shift, k);
      pieces_io += np;
      uint64_t prev_end = R[k].dst;
      for (uint32_t j = 0; j < np; ++j) {
        uint64_t a, b;
        piece_span(R[k].dst, R[k].len, shift, j, a, b);
        if (a != prev_end || b <= a) die("pieces not consecutive", it, io, image, shift, j);
        if (b - a > P || (j + 1 < np && (b & (P - 1)))) die("piece crosses a cut line", it, io, image, shift, j);
        prev_end = b;
        for (uint64_t x = a; x < b; ++x) {
          const int64_t rel = (int64_t)(x - image) + kGuard;
          if (rel < 0 || rel >= (int64_t)map.size()) die("piece outside the image's neighbourhood", it, io, image, shift, rel);
          if (map[rel] != kNone) die("byte written twice", it, io, image, shift, rel - kGuard);
          uint32_t tag = kZero;
          if (R[k].src) {
            const uint64_t s = R[k].src + (x - R[k].dst);
            if (k == kPlanPayload) {
              if (s < io.payload || s >= io.payload + io.length) die("payload read out of bounds", it, io, image, shift, k);
              tag = kPay | (uint32_t)(s - io.payload);
            } else {
              if (s < io.chunk || s >= io.chunk + s0) die("old bytes read out of bounds", it, io, image, shift, k);
              tag = kOld | (uint32_t)(s - io.chunk);
            }
          }
          map[rel] = tag;
        }
      }
      if (np && prev_end != R[k].dst + R[k].len) die("pieces short of the range", it, io, image, shift, k);
    }
    if (pieces_io > plan_piece_bound(max_len, shift, nranges)) die("piece bound", it, io, image, shift, (long long)pieces_io);
    n_pieces += pieces_io;
    for (size_t x = 0; x < map.size(); ++x)
      if (map[x] != model[x]) die("image differs from the model", it, io, image, shift, (long long)x - kGuard);

    // ---- the hash jobs prep stores ------------------------------------------------------------
    const PlanJobs J = plan_jobs(io, e, image);
    uint64_t l0, l1;
    pre_lens(e, l0, l1);  // (the runs workgroup takes the lengths from here)
    if (l0 != J.job[kJobPayload].len || l1 != J.job[kJobOld].len) die("pre_lens differs from plan_jobs", it, io, image, shift, 0);
    for (int k = 0; k < kPlanJobs; ++k) {
      const PlanJob& j = J.job[k];
      if (!j.len) {
        if (j.addr && k < kJobPrefix) die("empty pre job with an address", it, io, image, shift, k);
        continue;
      }
      if (!ok) die("job of an invalid IO", it, io, image, shift, k);
      const uint64_t lo = k == kJobPayload ? io.payload : k == kJobOld ? io.chunk : image;
      const uint64_t hi = lo + (k == kJobPayload ? io.length : k == kJobOld ? s0 : out_size);
      if (j.addr < lo || j.addr + j.len > hi) die("job outside its buffer", it, io, image, shift, k);
      if (k == kJobPayload && (j.addr != io.payload || j.len != io.length)) die("payload job is not the payload", it, io, image, shift, k);
      (k < kJobPrefix ? n_pre_jobs : n_post_jobs)++;
    }
    if (J.job[kJobPrefix].len + J.job[kJobSuffix].len) {  // the recompute: prefix, payload and suffix tile [0, s1)
      if (J.job[kJobPrefix].addr != image || J.job[kJobPrefix].len != e.off) die("prefix job", it, io, image, shift, 0);
      if (J.job[kJobSuffix].len && J.job[kJobSuffix].addr + J.job[kJobSuffix].len != image + out_size) die("suffix job", it, io, image, shift, 0);
      if (J.job[kJobPrefix].len + e.len + J.job[kJobSuffix].len != out_size) die("post jobs do not tile the image", it, io, image, shift, 0);
    }

    // ---- the ticketed apply's cuts: of this IO's in-place records, and of a drawn range --------
    const uint32_t tpieces = 1 + below(64);
    const uint32_t tmin = (below(4) ? 1 + below(64) : 1 + below(1u << 20)) << 10;
    if (!oop) n_tickets += check_tickets(it, R[0].dst, R[0].len, tpieces, tmin) + check_tickets(it, R[1].dst, R[1].len, tpieces, tmin);
    const uint64_t tdst = (uint64_t(1) << 40) + (rnd() & 0xffffff0) + it % 16;
    const uint32_t tn = check_tickets(it, tdst, pick_ticket_len(tpieces, tmin), tpieces, tmin);
    n_tickets += tn;
    n_ticket_full += tn == tpieces + 1;
  }
  const bool all_res = residues[0] == 0xffff && residues[1] == 0xffff && residues[2] == 0xffff;
  if (!all_res || !n_ok || !n_bad || !n_oop || !n_sync || !n_big || !n_pre_jobs || !n_post_jobs || !n_ticket_full) {
    std::printf("{\"fuzz_cow_planner\":\"FAIL\",\"what\":\"coverage\"}\n");
    return 1;
  }
  std::printf("{\"fuzz_cow_planner\":\"ok\",\"ios\":%llu,\"valid\":%llu,\"invalid\":%llu,\"out_of_place\":%llu,"
              "\"syncing\":%llu,\"pieces\":%llu,\"pre_jobs\":%llu,\"post_jobs\":%llu,\"tickets\":%llu,"
              "\"ranges_of_pieces_plus_1_tickets\":%llu}\n",
              (unsigned long long)iterations, (unsigned long long)n_ok, (unsigned long long)n_bad,
              (unsigned long long)n_oop, (unsigned long long)n_sync, (unsigned long long)n_pieces,
              (unsigned long long)n_pre_jobs, (unsigned long long)n_post_jobs, (unsigned long long)n_tickets,
              (unsigned long long)n_ticket_full);
  return 0;
}
