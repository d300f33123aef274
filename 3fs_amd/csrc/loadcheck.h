// loadcheck.h -- the load-checked build (-DHF3FS_CRC_LOAD_CHECK, libhf3fs_crc_loadcheck.so;
// DESIGN.md §5).  Plain HIP: every kernel load of caller bytes goes through lc_ok(), which
// records the 16-byte granules it touches in a bitmap the test owns, and refuses (the caller then
// uses zeros) a load outside the one allocation, the "yard", the test laid its buffers out in.
// So the read set of a call is observable, and a wrong address is logged, not dereferenced.
//
// Without the macro this header defines the site ids and an lc_ok() that is the constant true:
// the default library's device code does not change.
#pragma once
#include <stdint.h>
#if defined(HF3FS_CRC_LOAD_CHECK) && defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace hf3fs_crc {

// One id per load primitive or, where one primitive serves schedules that compute their
// addresses differently, per call site.  tests/load_footprint.py names them (SITES).
enum LoadSite : uint32_t {
  kSiteNone = 0,
  kSiteGload16 = 1,        // gload16: aligned granule
  kSiteGload16s = 2,       // gload16s: the streamed body of hash_grid
  kSiteGloadMasked = 3,    // gload16_masked: an edge granule
  kSiteDirectPre = 4,      // direct_pipe: the head blocks of this / the next task
  kSiteStreamProduce = 5,  // k_crc_range_stream: produce()
  kSiteFrameStream = 6,    // frame_kernels: the block stream and its clamped loads
  kSiteFramePair = 7,      // frame_kernels lin_t: at most two granules of a short range
  kSiteLd16 = 8,           // ld16: copy_rows_shfl's aligned source rows
  kSiteLd16Unaligned = 9,  // ld16_unaligned: two aligned granules of an unaligned 16 bytes
  kSiteLdu16 = 10,         // ldu16: the hardware's unaligned 16-byte load
  kSiteCopyByte = 11,      // head / tail bytes of copy_range, copy_range_hw, wg_write_hash_old
  kSiteApplyByte = 12,     // one_shot_piece: a piece's edge byte
  kSiteAuditBytes = 13,    // lin_serial: the payload re-hash of a verify mismatch
  kSiteMd5Granules = 14,   // load_granules
  kSiteMd5StageRow = 15,   // k_md5_hash<true>: the staged row load
  kSiteMd5Byte = 16,       // md5_stream_byte: the byte-granular cursor
  kSiteDesc = 17,          // a descriptor index >= n (never a load)
  kSiteCount = 18,
};

constexpr uint32_t kLoadCheckLogEntries = 64;
struct LoadCheckEntry {
  uint64_t address;
  uint32_t bytes, site, block, thread;
};
// The log the test hands in (device memory, zeroed): counters, then the first refused loads.
struct LoadCheckLog {
  uint32_t site_count[32];  // checked loads per site (armed only)
  uint32_t outside;         // loads outside the yard: refused, zeros returned
  uint32_t desc;            // descriptor indices >= n: refused, 0 returned
  uint32_t logged;          // entries used (counts on past kLoadCheckLogEntries)
  uint32_t reserved;
  LoadCheckEntry entry[kLoadCheckLogEntries];
};
struct LoadCheckState {
  uint64_t base, bytes;  // the yard
  uint32_t* bitmap;      // one bit per 16-byte granule of the yard; nullptr = disarmed
  uint8_t* site_map;     // one byte per granule: a site that touched it
  LoadCheckLog* log;
};

#ifdef HF3FS_CRC_LOAD_CHECK
#ifdef __HIPCC__
// The library is built without relocatable device code: every translation unit has its own copy,
// and hf3fs_crc_loadcheck_arm sets them all through the setters registered below.
static __device__ LoadCheckState g_loadcheck;
#define HF3FS_LC_FN __attribute__((unused)) static __device__ __noinline__

void loadcheck_register(int (*set)(const LoadCheckState*));
namespace {
int loadcheck_set_this_unit(const LoadCheckState* s) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_loadcheck), s, sizeof(*s));
}
struct LoadCheckRegistrar {
  LoadCheckRegistrar() { loadcheck_register(&loadcheck_set_this_unit); }
};
static LoadCheckRegistrar g_loadcheck_registrar;
}  // namespace

HF3FS_LC_FN void lc_log(const LoadCheckState& s, uint64_t addr, uint32_t nbytes, uint32_t site) {
  const uint32_t k = atomicAdd(&s.log->logged, 1u);
  if (k < kLoadCheckLogEntries) {
    LoadCheckEntry* e = &s.log->entry[k];
    e->address = addr;
    e->bytes = nbytes;
    e->site = site;
    e->block = blockIdx.x;
    e->thread = threadIdx.x;
  }
}
// May the load of [addr, addr + nbytes) go out?  Armed: counts it, marks its granules, or logs
// and refuses it.  Disarmed (the child's own fills and set-up): every load goes out.
HF3FS_LC_FN bool lc_ok(uint64_t addr, uint32_t nbytes, uint32_t site) {
  const LoadCheckState s = g_loadcheck;
  if (!s.bitmap) return true;
  atomicAdd(&s.log->site_count[site], 1u);
  if (addr < s.base || addr + nbytes > s.base + s.bytes || addr + nbytes < addr) {
    atomicAdd(&s.log->outside, 1u);
    lc_log(s, addr, nbytes, site);
    return false;
  }
  const uint64_t g0 = (addr - s.base) >> 4, g1 = (addr + nbytes - 1 - s.base) >> 4;
  for (uint64_t g = g0; g <= g1; ++g) {
    atomicOr(&s.bitmap[g >> 5], 1u << (g & 31));
    s.site_map[g] = (uint8_t)site;
  }
  return true;
}
// Is descriptor index i of an n-element caller array in range?  Armed or not.
HF3FS_LC_FN bool lc_desc_ok(uint64_t i, uint64_t n) {
  if (i < n) return true;
  const LoadCheckState s = g_loadcheck;
  if (s.bitmap) {
    atomicAdd(&s.log->site_count[kSiteDesc], 1u);
    atomicAdd(&s.log->desc, 1u);
    lc_log(s, i, 0, kSiteDesc);
  }
  return false;
}
// Record i of a caller's n-element record array (update, read, scrub and frame records): an
// index >= n is logged under kSiteDesc and gives a zeroed record without a load.
template <class T>
__device__ __forceinline__ T lc_rec(const T* recs, uint64_t i, uint64_t n) {
  return lc_desc_ok(i, n) ? recs[i] : T{};
}
#define HF3FS_LC_REC(recs, i, n) ::hf3fs_crc::lc_rec((recs), (uint64_t)(i), (uint64_t)(n))
// The element count as one more parameter / argument of a device function that takes a record index
// (behind the index; nothing in the default build).
#define HF3FS_LC_N(n) , uint64_t n
#define HF3FS_LC_PASS(n) , (n)
#else  // a host-only unit of the check build: no kernels, no loads
inline constexpr bool lc_desc_ok(uint64_t, uint64_t) { return true; }
#endif  // __HIPCC__
#else
#ifdef __HIPCC__
__host__ __device__ __forceinline__ constexpr bool lc_ok(uint64_t, uint32_t, uint32_t) { return true; }
__host__ __device__ __forceinline__ constexpr bool lc_desc_ok(uint64_t, uint64_t) { return true; }
#define HF3FS_LC_REC(recs, i, n) ((recs)[i])
#define HF3FS_LC_N(n)
#define HF3FS_LC_PASS(n)
#else
inline constexpr bool lc_desc_ok(uint64_t, uint64_t) { return true; }
#endif
#endif

}  // namespace hf3fs_crc
