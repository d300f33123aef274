// client_write_plan.h -- the decisions of hf3fs_crc_client_write_prepare / _complete, plain C++
// that both the device compiler and a host compiler take: what StorageClientImpl::batchWrite
// makes of a WriteIO before the send (validateWriteDataRange, src/client/storage/
// StorageClientImpl.cc:994-1015; validateDataRange, :889-951; sendWriteRequest, :1878-1901) and
// FileWrapper::writeFile's fold of the answers (src/client/cli/admin/FileWrapper.cc:218-248 over
// ChecksumInfo::combine, src/fbs/storage/Common.h:179-198) in two forms: the reference's
// sequential loop, and the order-free summary the wave schedule of client_write_kernels.hip uses.
// tests/cpp/fuzz_client_write.cpp includes this header and holds both to a restatement of the
// reference's loops under ASan + UBSan.
//
// The fold.  A file's IOs a_0 .. a_{k-1}, each an answer (final status s, type t, result_len r,
// requested length l, value v).  Three ends depend on the IO alone: s != 0 (code s), t > CRC32
// (code 3), r != l (code 33); call the lowest such index e.  The fourth, combine's type check,
// depends on the accumulator, whose type is NONE until the first IO with t typed and r > 0, the
// adopter at index a of type T, and T from then on (a NONE answer with r > 0 is adopted too, but
// leaves the type NONE: only its value stays).  So the check fires at the lowest m > a with
// t_m != T, whatever r_m is -- the check stands before the zero-length return -- and the fold ends
// at min(e, m), at e when they are equal (the IO's own checks come first).  Without an end every
// typed answer with r > 0 has type T and none lies before a, so the value is the raw
// concatenation of those answers, (V_a, L_a).(V_b, L_b) = ((~V_a) X^L_b ^ V_b, L_a + L_b), which is
// associative; without an adopter it is the last NONE answer's value with r > 0, else 0.
// The summary of a run is therefore {e and its code, the adopter a and T, the run's own m, the
// concatenation (V, L), the first index of each answer type (so that a typed run on the left finds
// its m in the run on the right), the last NONE value, the sum of r}.
#pragma once
#include <stdint.h>

#include "../../include/hf3fs_crc.h"
#include "gf2.h"

#ifdef __HIPCC__
#define HF3FS_CW_FN __host__ __device__ __forceinline__
#else
#define HF3FS_CW_FN inline
#endif

namespace hf3fs_crc {

constexpr uint32_t kCwNone = ~0u;                    // no index
constexpr uint64_t kClientWriteMaxCount = 1ull << 30;  // IOs and files of one call
constexpr int32_t kCwInvalidArg = HF3FS_CRC_CLIENT_INVALID_ARG;

// ---- prepare ----------------------------------------------------------------------------------
enum CwClass : uint8_t {
  kCwBadRecord = 0,  // rule 1: status 3
  kCwRange = 1,      // rule 2: 7002, this IO alone
  kCwOffender = 2,   // passed 1 and 2, fails the buffer check: poisons the batch
  kCwValid = 3,      // valid by itself: sent unless the batch is poisoned
};

// RDMABuf::contains (RDMABuf.h:162) in 64-bit unsigned sums; a sum that wraps is not contained.
HF3FS_CW_FN bool client_write_contained(uint64_t data, uint32_t length, uint64_t base, uint64_t size) {
  const uint64_t end = data + length, cap = base + size;
  if (end < data || cap < base) return false;
  return base <= data && end <= cap;
}

HF3FS_CW_FN CwClass client_write_class(const hf3fs_crc_client_write_io& io, uint32_t max_len) {
  if (io.length > max_len) return kCwBadRecord;
  if (io.chunk_size == 0 || (uint32_t)(io.offset + io.length) > io.chunk_size) return kCwRange;  // :1000, uint32_t
  if (io.buf_base == 0 || io.data == 0 || !client_write_contained(io.data, io.length, io.buf_base, io.buf_size))
    return kCwOffender;
  return kCwValid;
}

// Is the payload hashed?  (The prep cannot know yet whether the batch is poisoned; length 0 is
// ChecksumInfo::create's starting value, ~0u, and no job.)
HF3FS_CW_FN bool client_write_hashes(CwClass k, bool verify, uint32_t length) {
  return verify && k == kCwValid && length > 0;
}

struct CwPrepared {
  int32_t status;
  uint32_t checksum;
  uint8_t checksum_type, send_inline;
  bool sent;
};

// hashed: the range kernels' raw CRC of the payload when client_write_hashes, else ~0u.
HF3FS_CW_FN CwPrepared client_write_settle(CwClass k, bool poisoned, uint32_t length, uint32_t hashed, uint8_t type,
                                           bool verify, uint32_t max_inline_bytes) {
  CwPrepared p;
  p.status = k == kCwBadRecord ? HF3FS_CRC_INVALID_ARG : k == kCwRange || poisoned ? kCwInvalidArg : 0;
  p.sent = p.status == 0;
  p.checksum = p.sent && verify ? hashed : 0u;
  p.checksum_type = p.sent && verify ? type : kTypeNone;
  p.send_inline = p.sent && length <= max_inline_bytes ? 1 : 0;
  return p;
}

// ---- complete ---------------------------------------------------------------------------------
// An IO as the fold sees it.
struct CwAnswer {
  int32_t status;  // the final status
  uint32_t result_len, length, value;
  uint8_t type;
};

HF3FS_CW_FN CwAnswer client_write_answer(const hf3fs_crc_client_write_io& io) {
  CwAnswer a;
  a.status = io.status != 0 ? io.status : io.status_in;
  a.result_len = io.result_len;
  a.length = io.length;
  a.value = io.result_checksum;
  a.type = io.result_checksum_type;
  return a;
}

// FROM_UPDATES: the answer of an IO that was sent is its update record's outcome.
HF3FS_CW_FN void client_write_take_update(hf3fs_crc_client_write_io& io, const hf3fs_crc_update_io& u) {
  if (io.status != 0) return;
  io.status_in = u.status;
  io.result_len = u.length;
  io.result_checksum = u.out_checksum;
  io.result_checksum_type = u.out_checksum_type;
}

// The code an answer ends the fold with by itself, 0 if none.
HF3FS_CW_FN int32_t client_write_own_end(const CwAnswer& a) {
  if (a.status != 0) return a.status;                          // FileWrapper.cc:236
  if (a.type > kTypeCrc32) return HF3FS_CRC_INVALID_ARG;       // (no such ChecksumType)
  if (a.result_len != a.length) return HF3FS_CRC_INVALID_FORMAT;  // :238-246
  return 0;
}

struct CwFile {
  uint64_t length;
  uint32_t value;
  uint8_t type;
  int32_t status;
  uint32_t failed;  // index among the file's IOs, kCwNone if none
};

HF3FS_CW_FN CwFile client_write_file_begin() {
  CwFile f;
  f.length = 0;
  f.value = 0;
  f.type = kTypeNone;  // ChecksumInfo{}: {NONE, 0}
  f.status = 0;
  f.failed = kCwNone;
  return f;
}

HF3FS_CW_FN CwFile client_write_file_ended(int32_t code, uint32_t index) {
  CwFile f = client_write_file_begin();
  f.status = code;
  f.failed = index;
  return f;
}

// Bench.cc:41-48: .value alone is compared.
HF3FS_CW_FN void client_write_expect(CwFile& f, uint32_t expected) {
  if (f.status == 0 && f.value != expected) {
    f.status = HF3FS_CRC_CLIENT_CHECKSUM_MISMATCH;
    f.failed = kCwNone;
  }
}

HF3FS_CW_FN void client_write_file_emit(const CwFile& f, uint64_t first_io, hf3fs_crc_client_write_file* out) {
  hf3fs_crc_client_write_file r{};
  r.length = f.length;
  r.value = f.value;
  r.type = f.type;
  r.status = f.status;
  r.failed_io = f.failed == kCwNone ? kCwNone : (uint32_t)(first_io + f.failed);
  *out = r;
}

// ---- the reference's loop -----------------------------------------------------------------------
// IO number `index` of the file, in order; false: the fold has ended.
template <class Gf>
HF3FS_CW_FN bool client_write_seq_step(CwFile& f, const CwAnswer& a, uint32_t index, const Gf& gf) {
  if (f.status != 0) return false;
  int32_t end = client_write_own_end(a);
  if (!end && f.type != kTypeNone && f.type != a.type) end = HF3FS_CRC_CHECKSUM_MISMATCH;  // Common.h:180-183
  if (end) {
    f = client_write_file_ended(end, index);
    return false;
  }
  if (a.result_len != 0) {        // :184
    if (f.type == kTypeNone) {    // :186-188
      f.type = a.type;
      f.value = a.value;
    } else {                      // :190-196
      f.value = gf.shift(~f.value, a.result_len, f.type) ^ a.value;
    }
  }
  f.length += a.result_len;
  return true;
}

// ---- the order-free summary ---------------------------------------------------------------------
struct CwSum {
  uint64_t len;       // bytes of the concatenation
  uint64_t length;    // sum of result_len
  uint32_t v;         // the raw concatenation of the typed answers with result_len > 0
  uint32_t nv;        // the last NONE answer's value with result_len > 0
  uint32_t end;       // lowest index that ends the fold by itself
  int32_t end_code;
  uint32_t adopt;     // (index << 2 | type) of the run's adopter
  uint32_t mis;       // lowest index behind the run's adopter whose type is not the adopter's
  uint32_t first[3];  // lowest index of an answer of each type
  uint32_t has_nv;
};

HF3FS_CW_FN CwSum client_write_sum_identity() {
  CwSum s;
  s.len = s.length = 0;
  s.v = s.nv = 0;
  s.end = kCwNone;
  s.end_code = 0;
  s.adopt = s.mis = kCwNone;
  s.first[0] = s.first[1] = s.first[2] = kCwNone;
  s.has_nv = 0;
  return s;
}

HF3FS_CW_FN CwSum client_write_sum_of(const CwAnswer& a, uint32_t index) {
  CwSum s = client_write_sum_identity();
  const int32_t end = client_write_own_end(a);
  if (end) {  // nothing at or behind an end counts: the other fields stay empty
    s.end = index;
    s.end_code = end;
    return s;
  }
  s.first[a.type] = index;
  s.length = a.result_len;
  if (a.result_len == 0) return s;
  if (a.type == kTypeNone) {
    s.has_nv = 1;
    s.nv = a.value;
  } else {
    s.adopt = index << 2 | a.type;  // (index < 2^30)
    s.v = a.value;
    s.len = a.result_len;
  }
  return s;
}

HF3FS_CW_FN uint32_t cw_min(uint32_t a, uint32_t b) { return b < a ? b : a; }

// a's IOs lie before b's.
template <class Gf>
HF3FS_CW_FN CwSum client_write_sum_join(const CwSum& a, const CwSum& b, const Gf& gf) {
  CwSum r = a;
  if (a.adopt != kCwNone) {
    const uint8_t t = (uint8_t)(a.adopt & 3);
    uint32_t other = kCwNone;
    for (int k = 0; k < 3; ++k)
      if (k != t) other = cw_min(other, b.first[k]);
    r.mis = cw_min(a.mis, other);
    if (b.adopt != kCwNone) {  // (of another type: r.mis says so, the value is then unused)
      r.v = gf.shift(~a.v, b.len, t) ^ b.v;
      r.len = a.len + b.len;
    }
  } else {
    r.adopt = b.adopt;
    r.mis = b.mis;
    r.v = b.v;
    r.len = b.len;
  }
  if (b.has_nv) {
    r.nv = b.nv;
    r.has_nv = 1;
  }
  if (b.end < a.end) {
    r.end = b.end;
    r.end_code = b.end_code;
  }
  for (int k = 0; k < 3; ++k) r.first[k] = cw_min(a.first[k], b.first[k]);
  r.length = a.length + b.length;
  return r;
}

HF3FS_CW_FN CwFile client_write_sum_finish(const CwSum& s) {
  if (s.end != kCwNone && s.end <= s.mis) return client_write_file_ended(s.end_code, s.end);
  if (s.mis != kCwNone) return client_write_file_ended(HF3FS_CRC_CHECKSUM_MISMATCH, s.mis);
  CwFile f = client_write_file_begin();
  f.length = s.length;
  if (s.adopt != kCwNone) {
    f.type = (uint8_t)(s.adopt & 3);
    f.value = s.v;
  } else if (s.has_nv) {
    f.value = s.nv;
  }
  return f;
}

// gf2.h's arithmetic as a Gf (the host's; the kernels have the device tables).
struct CwGfPlain {
  HF3FS_CW_FN uint32_t shift(uint32_t v, uint64_t nbytes, uint8_t type) const {
    return shift_bytes(v, nbytes, poly_of(type));
  }
};

}  // namespace hf3fs_crc
