// loadcheck.hip -- the host side of the load-checked build (loadcheck.h): the list of the
// translation units' state setters, and the three functions a test calls.  Only
// libhf3fs_crc_loadcheck.so has them; include/hf3fs_crc.h does not declare them.
#ifndef HF3FS_CRC_LOAD_CHECK
#error "loadcheck.hip belongs to the load-checked build only"
#endif
#include "loadcheck.h"

namespace hf3fs_crc {
namespace {
constexpr int kMaxUnits = 32;
int (*g_setters[kMaxUnits])(const LoadCheckState*);  // zero-initialised before any registrar runs
int g_units;

int set_all(const LoadCheckState& s) {
  for (int k = 0; k < g_units; ++k) {
    const int e = g_setters[k](&s);
    if (e) return e;
  }
  return 0;
}
}  // namespace

void loadcheck_register(int (*set)(const LoadCheckState*)) {
  if (g_units < kMaxUnits) g_setters[g_units++] = set;
}
}  // namespace hf3fs_crc

extern "C" {
// The yard [base, base + bytes), base 16-byte aligned; d_bitmap: one bit per granule, rounded up
// to whole 32-bit words; d_site_map: one byte per granule; d_log: a zeroed LoadCheckLog.  All
// device memory of the caller's, which reads them back itself after the synchronize.
// Returns 0, or a hipError_t / -1 for bad arguments.
__attribute__((visibility("default"))) int hf3fs_crc_loadcheck_arm(uint64_t base, uint64_t bytes, void* d_bitmap,
                                                                   void* d_site_map, void* d_log) {
  if (!base || (base & 15) || !bytes || !d_bitmap || !d_site_map || !d_log) return -1;
  const hf3fs_crc::LoadCheckState s{base, bytes, (uint32_t*)d_bitmap, (uint8_t*)d_site_map,
                                    (hf3fs_crc::LoadCheckLog*)d_log};
  return hf3fs_crc::set_all(s);
}
__attribute__((visibility("default"))) int hf3fs_crc_loadcheck_disarm(void) {
  return hf3fs_crc::set_all(hf3fs_crc::LoadCheckState{0, 0, nullptr, nullptr, nullptr});
}
// Translation units that carry a copy of the state (a test checks that none was lost).
__attribute__((visibility("default"))) int hf3fs_crc_loadcheck_units(void) { return hf3fs_crc::g_units; }
}
