// client_read_plan.h -- the decisions of hf3fs_crc_client_read_batch, plain C++ that both the device
// compiler and a host compiler take: which children of a completed batchRead are hashed and what
// the comparison makes of them (src/client/storage/StorageClientImpl.cc:1720-1737), and the
// split-read merge (:1607-1633 over ChecksumInfo::combine, src/fbs/storage/Common.h:179-198) in
// two forms: the reference's sequential loop, and the order-free fold the wave schedule of
// client_read_kernels.hip uses.  tests/cpp/fuzz_client_read.cpp includes this header and holds
// the fold to the loop under ASan + UBSan.
//
// The GF(2) arithmetic is a parameter: `Gf` has shift(v, nbytes, type) = v * x^(8 nbytes) under
// the type's polynomial (gf2.h on the host, the device tables in the kernels).
//
// The fold.  A parent's children c_0 .. c_{k-1}, each after the verify (status, type t, value v,
// read_len r).  If any status is non-zero the lowest such index takes over: a minimum.  Else
// child 0 is assigned whatever its r, and for i >= 1 the loop's state S moves as
//     S.t != NONE and S.t != t_i : nothing         r_i == 0 : nothing
//     S.t == NONE : S = (t_i, v_i)                 else : S.v = (~S.v) x^(8 r_i) ^ v_i
// so (1) S stays NONE until the first i >= 1 with t_i != NONE and r_i > 0, the child that fixes
// the type (a minimum again), unless t_0 fixed it; while NONE it holds the value of the last NONE
// child with r_i > 0, else v_0; (2) once typed T, only the children of type T with r_i > 0 act,
// each by the affine map x -> (~x) X^r_i ^ v_i.  A run of such maps composes to
// x -> (~x) X^L ^ V with (V, L) the raw concatenation (V_a, L_a).(V_b, L_b) =
// ((~V_a) X^L_b ^ V_b, L_a + L_b), which is associative, and V alone is what a state that adopts
// the run's first child ends with.  No typed child of type T with r > 0 lies before the child
// that fixes T, so one concatenation per CRC type over the children i >= 1 serves both cases:
//     t_0 = T typed     : value = (~v_0) X^(L_T) ^ V_T  (v_0 if no such child)
//     fixed by i >= 1   : value = V_T
//     never fixed       : {NONE, last NONE value, else v_0}
// The state of a run is therefore {fail = min index, fix = min (index << 2 | type), (V, L) for
// CRC32C and for CRC32, the last NONE value, the uint32 sums of read_len and length}.
#pragma once
#include <stdint.h>

#include "../../include/hf3fs_crc.h"
#include "gf2.h"

#ifdef __HIPCC__
#define HF3FS_CR_FN __host__ __device__ __forceinline__
#else
#define HF3FS_CR_FN inline
#endif

namespace hf3fs_crc {

constexpr uint32_t kClientNone = ~0u;               // no failing child / no child fixes the type
constexpr uint64_t kClientMaxCount = 1ull << 30;    // IOs and parents of one call
constexpr int32_t kClientMismatch = HF3FS_CRC_CLIENT_CHECKSUM_MISMATCH;
constexpr int32_t kClientNotInitialized = HF3FS_CRC_CLIENT_NOT_INITIALIZED;
constexpr int32_t kClientChunkNotFound = HF3FS_CRC_CHUNK_NOT_FOUND;

// A record the call refuses (status 3); see the header's comment for the rules.
HF3FS_CR_FN bool client_read_bad(const hf3fs_crc_client_read_io& io, uint8_t type, uint32_t max_len, bool verify) {
  if (io.status_in != 0) return false;  // no lengthInfo: nothing of the record is used but its status and checksum
  if (io.checksum_type > kTypeCrc32) return true;
  if (!verify) return false;
  if (io.checksum_type != kTypeNone && io.checksum_type != type) return true;
  if (io.read_len > max_len || io.read_len > io.length) return true;
  return io.read_len > 0 && io.data == 0;
}

// :1722 -- is the child compared at all?
HF3FS_CR_FN bool client_read_verifies(const hf3fs_crc_client_read_io& io, uint8_t type, uint32_t max_len, bool verify) {
  return verify && io.status_in == 0 && io.read_len > 0 && !client_read_bad(io, type, max_len, verify);
}

// Are its bytes hashed?  ChecksumInfo::create(NONE, ...) returns {NONE, 0} before the first byte.
HF3FS_CR_FN bool client_read_hashes(const hf3fs_crc_client_read_io& io, uint8_t type, uint32_t max_len, bool verify) {
  return client_read_verifies(io, type, max_len, verify) && io.checksum_type != kTypeNone;
}

// A child as the merge sees it: its result after the verify.
struct ClientChild {
  int32_t status;
  uint32_t computed;  // what the verdict stores beside the status
  uint32_t value;     // result.checksum
  uint8_t type;
  uint32_t read_len;  // *lengthInfo (status == 0)
  uint32_t length;    // ReadIO.length
};

// :1723-1733.  hashed: the range kernels' value for the child (read only if the child is hashed).
HF3FS_CR_FN ClientChild client_read_verdict(const hf3fs_crc_client_read_io& io, uint32_t hashed, uint8_t type,
                                            uint32_t max_len, bool verify) {
  ClientChild c;
  c.status = io.status_in;
  c.computed = 0;
  c.value = io.checksum;
  c.type = io.checksum_type;
  c.read_len = io.read_len;
  c.length = io.length;
  if (client_read_bad(io, type, max_len, verify)) {
    c.status = HF3FS_CRC_INVALID_ARG;
  } else if (client_read_verifies(io, type, max_len, verify)) {
    c.computed = io.checksum_type == kTypeNone ? 0u : hashed;
    if (c.computed != io.checksum) {  // (the types are equal by construction, :1723)
      c.status = kClientMismatch;     // setErrorCodeOfOp: result = IOResult(7015)
      c.value = 0;
      c.type = kTypeNone;
    }
  }
  return c;
}

// parentIO->result.
struct ClientParent {
  int32_t status;
  uint32_t length, value;
  uint8_t type;
  uint32_t failed;  // index among the parent's children, kClientNone if none
  uint32_t block_len;
};

HF3FS_CR_FN void client_parent_emit(const ClientParent& p, uint64_t first_child, hf3fs_crc_client_read_result* out,
                                    hf3fs_crc_block_digest* block) {
  if (out) {
    hf3fs_crc_client_read_result r{};
    r.length = p.length;
    r.checksum = p.value;
    r.checksum_type = p.type;
    r.status = p.status;
    r.failed_child = p.failed == kClientNone ? kClientNone : (uint32_t)(first_child + p.failed);
    r.block_len = p.block_len;
    *out = r;
  }
  if (block) {  // FileWrapper.cc:132-163
    hf3fs_crc_block_digest b{};
    b.read_len = p.length;
    b.block_len = p.block_len;
    b.checksum = p.value;
    b.checksum_type = p.type;
    b.missing = p.status == kClientChunkNotFound ? 1 : 0;
    *block = b;
  }
}

// ---- the reference's loop -------------------------------------------------------------------
struct ClientSeq {
  ClientParent p;
  bool done;
};

HF3FS_CR_FN ClientSeq client_seq_begin() {
  ClientSeq s;
  s.p.status = kClientNotInitialized;  // IOResult(): lengthInfo = makeError(kNotInitialized)
  s.p.length = 0;
  s.p.value = 0;
  s.p.type = kTypeNone;
  s.p.failed = kClientNone;
  s.p.block_len = 0;
  s.done = false;
  return s;
}

// Child number `index` of the parent, in order.  After the break only block_len moves on.
template <class Gf>
HF3FS_CR_FN void client_seq_step(ClientSeq& s, const ClientChild& c, uint32_t index, const Gf& gf) {
  s.p.block_len += c.length;
  if (s.done) return;
  if (c.status != 0) {  // :1621-1623
    s.p.status = c.status;
    s.p.length = 0;
    s.p.value = c.value;
    s.p.type = c.type;
    s.p.failed = index;
    s.done = true;
  } else if (index == 0) {  // :1624-1627
    s.p.status = 0;
    s.p.length = c.read_len;
    s.p.value = c.value;
    s.p.type = c.type;
  } else {
    s.p.length += c.read_len;                               // :1629
    if (s.p.type != kTypeNone && s.p.type != c.type) return;  // Common.h:180-183, result dropped
    if (c.read_len == 0) return;                            // :184
    if (s.p.type == kTypeNone) {                            // :186-188
      s.p.type = c.type;
      s.p.value = c.value;
    } else {                                                // :190-196
      s.p.value = gf.shift(~s.p.value, c.read_len, s.p.type) ^ c.value;
    }
  }
}

// ---- the order-free fold --------------------------------------------------------------------
constexpr uint8_t kClientHasNone = 4;  // has bits: 1 << (type - 1) for the two CRC types, 4 for a NONE value

struct ClientSum {
  uint64_t len[2];  // [0] CRC32C, [1] CRC32: bytes of the typed children, index >= 1, read_len > 0
  uint32_t v[2];    // their raw concatenation
  uint32_t nv;      // the last NONE child's value (index >= 1, read_len > 0)
  uint32_t fix;     // min (index << 2 | type) over the typed children, index >= 1, read_len > 0
  uint32_t fail;    // min index with a non-zero status
  uint32_t length, block_len;
  uint32_t has;
};

HF3FS_CR_FN ClientSum client_sum_identity() {
  ClientSum s;
  s.len[0] = s.len[1] = 0;
  s.v[0] = s.v[1] = 0;
  s.nv = 0;
  s.fix = kClientNone;
  s.fail = kClientNone;
  s.length = s.block_len = 0;
  s.has = 0;
  return s;
}

HF3FS_CR_FN ClientSum client_sum_of(const ClientChild& c, uint32_t index) {
  ClientSum s = client_sum_identity();
  s.block_len = c.length;
  if (c.status != 0) {
    s.fail = index;
    return s;
  }
  s.length = c.read_len;
  if (index == 0 || c.read_len == 0) return s;  // child 0 enters at the end (client_sum_finish)
  if (c.type == kTypeNone) {
    s.has = kClientHasNone;
    s.nv = c.value;
  } else if (c.type <= kTypeCrc32) {
    const int k = c.type - 1;
    s.has = 1u << k;
    s.v[k] = c.value;
    s.len[k] = c.read_len;
    s.fix = index << 2 | c.type;  // (index < 2^30)
  }
  return s;
}

// a's children lie before b's.
template <class Gf>
HF3FS_CR_FN ClientSum client_sum_join(const ClientSum& a, const ClientSum& b, const Gf& gf) {
  ClientSum r = a;
  for (int k = 0; k < 2; ++k) {
    if (!(b.has & (1u << k))) continue;
    r.v[k] = (a.has & (1u << k)) ? gf.shift(~a.v[k], b.len[k], (uint8_t)(k + 1)) ^ b.v[k] : b.v[k];
    r.len[k] = a.len[k] + b.len[k];
  }
  if (b.has & kClientHasNone) r.nv = b.nv;
  r.has = a.has | b.has;
  r.fix = b.fix < a.fix ? b.fix : a.fix;
  r.fail = b.fail < a.fail ? b.fail : a.fail;
  r.length = a.length + b.length;
  r.block_len = a.block_len + b.block_len;
  return r;
}

// The parent from the fold over its n children; child(i) gives child i (asked for child 0 and
// for the failing child only).
template <class Gf, class ChildAt>
HF3FS_CR_FN ClientParent client_sum_finish(const ClientSum& s, uint64_t n, const ChildAt& child, const Gf& gf) {
  ClientParent p = client_seq_begin().p;
  p.block_len = s.block_len;
  if (n == 0) return p;
  if (s.fail != kClientNone) {
    const ClientChild c = child(s.fail);
    p.status = c.status;
    p.value = c.value;
    p.type = c.type;
    p.failed = s.fail;
    return p;
  }
  const ClientChild c0 = child(0u);
  p.status = 0;
  p.length = s.length;
  if (c0.type != kTypeNone) {
    const int k = c0.type - 1;  // (a good child's type is <= CRC32)
    p.type = c0.type;
    p.value = (s.has & (1u << k)) ? gf.shift(~c0.value, s.len[k], c0.type) ^ s.v[k] : c0.value;
  } else if (s.fix != kClientNone) {
    p.type = (uint8_t)(s.fix & 3);
    p.value = s.v[p.type - 1];
  } else {
    p.type = kTypeNone;
    p.value = (s.has & kClientHasNone) ? s.nv : c0.value;
  }
  return p;
}

// gf2.h's arithmetic as a Gf (the host's; the kernels have the device tables).
struct ClientGfPlain {
  HF3FS_CR_FN uint32_t shift(uint32_t v, uint64_t nbytes, uint8_t type) const {
    return shift_bytes(v, nbytes, poly_of(type));
  }
};

}  // namespace hf3fs_crc
