// check_client_write_scratch.cpp -- the scratch carve of hf3fs_crc_client_write_complete fits its
// byte count, and the public sizing function covers both calls.  Needs no GPU: only sizing and
// carving functions of libhf3fs_crc.so are called, on a fake base.  A program of its own beside
// check_scratch_layout.cpp, whose golden sizes stay as they are.
//
// Fit: the layout is carved at a 16-byte aligned base; every member must be 16-byte aligned,
// disjoint from the other and inside [base, base + client_write_scratch_bytes(n)).
// Cover: hf3fs_crc_client_write_scratch_bytes(n, f) is at least complete's carve plus the slack
// the entry point adds to align it, and at least run_record_jobs' carve {ctl[4], addr[n], len[n],
// v[n]} with the byte-run tables of a 256-CU device, which is what prepare takes.
#include <cstdio>
#include <initializer_list>

#include "../../include/hf3fs_crc.h"
#include "../../3fs_amd/csrc/client_write_kernels.h"
#include "../../3fs_amd/csrc/update_kernels.h"  // kRunBlocksMax

using namespace hf3fs_crc;

int main() {
  int failures = 0;
  uint8_t* const base = (uint8_t*)0x7f0000000010ull;  // 16-byte aligned, not 64
  for (uint64_t n : {1ull, 2ull, 15ull, 16ull, 17ull, 255ull, 256ull, 257ull, 4096ull, 65537ull, 1000003ull, 1ull << 30}) {
    const size_t total = client_write_scratch_bytes(n);
    ClientWriteScratch s;
    client_write_scratch_carve(base, n, &s);
    const uintptr_t lo = (uintptr_t)base, hi = lo + total;
    const uintptr_t count = (uintptr_t)s.count, take = (uintptr_t)s.take;
    const size_t count_bytes = kClientWriteBlocksMax * 4;
    if (count % 16 || take % 16) ++failures, fprintf(stderr, "n %llu: a member is not 16-byte aligned\n", (unsigned long long)n);
    if (count < lo || count + count_bytes > hi || take < lo || take + n > hi)
      ++failures, fprintf(stderr, "n %llu: a member leaves the %zu bytes\n", (unsigned long long)n, total);
    if (count < take ? count + count_bytes > take : take + n > count)
      ++failures, fprintf(stderr, "n %llu: count and take overlap\n", (unsigned long long)n);
    const size_t pub = hf3fs_crc_client_write_scratch_bytes(n, n);
    const size_t nw = 256 * kWaves;
    const size_t prepare = (16 + n * (8 + 8 + 4) + 63) / 64 * 64 + (kRunBlocksMax + 2 * (nw + 1)) * 8 + (nw + 1) * 4 + 64;
    if (pub < total + 16 || pub < prepare || pub % 4)
      ++failures, fprintf(stderr, "n %llu: the public size %zu does not cover %zu / %zu\n", (unsigned long long)n, pub,
                          total + 16, prepare);
    printf("size client_write_scratch_bytes/%llu %zu\n", (unsigned long long)n, total);
    printf("size hf3fs_crc_client_write_scratch_bytes/%llu %zu\n", (unsigned long long)n, pub);
  }
  if (hf3fs_crc_client_write_scratch_bytes((1ull << 30) + 1, 0) || hf3fs_crc_client_write_scratch_bytes(1, (1ull << 30) + 1))
    ++failures, fprintf(stderr, "a rejected count has a size\n");
  if (failures) return fprintf(stderr, "%d layout failures\n", failures), 1;
  printf("ALL OK\n");
  return 0;
}
