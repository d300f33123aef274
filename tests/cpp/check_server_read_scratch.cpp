// check_server_read_scratch.cpp -- the scratch carve of hf3fs_crc_server_read_complete fits its byte
// count, and the public sizing function covers the call.  Needs no GPU: only sizing and carving
// functions of libhf3fs_crc.so are called, on a fake base.  A program of its own beside
// check_scratch_layout.cpp and check_client_write_scratch.cpp, whose golden sizes stay as they are.
//
// Fit: the layout is carved at a 16-byte aligned base; every member must be aligned to its element,
// disjoint from the others and inside [base, base + server_read_scratch_bytes(n)).
// Cover: hf3fs_crc_server_read_scratch_bytes(n, r) is at least run_record_jobs' carve {ctl[4],
// addr[n], len[n], v[n]} up to a multiple of 64, its 64 spare bytes, complete's tail and the 16 bytes
// the entry point adds to align it.
#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../include/hf3fs_crc.h"
#include "../../3fs_amd/csrc/server_read_kernels.h"

using namespace hf3fs_crc;

int main() {
  int failures = 0;
  uint8_t* const base = (uint8_t*)0x7f0000000010ull;  // 16-byte aligned, not 64
  for (uint64_t n : {1ull, 2ull, 15ull, 16ull, 17ull, 255ull, 256ull, 257ull, 4096ull, 65537ull, 1000003ull, 1ull << 30}) {
    const size_t total = server_read_scratch_bytes(n);
    ServerReadScratch s;
    server_read_scratch_carve(base, n, &s);
    struct Member {
      const char* name;
      uintptr_t at;
      size_t bytes, align;
    };
    std::vector<Member> m = {{"bytes", (uintptr_t)s.bytes, kServerReadBlocksMax * 8, 8},
                             {"pre", (uintptr_t)s.pre, (n + 1) * 8, 8},
                             {"count", (uintptr_t)s.count, kServerReadBlocksMax * 4, 4},
                             {"wr_pre", (uintptr_t)s.wr_pre, (n + 1) * 4, 4},
                             {"req", (uintptr_t)s.req, n * 4, 4},
                             {"done", (uintptr_t)s.done, n, 1}};
    const uintptr_t lo = (uintptr_t)base, hi = lo + total;
    for (const Member& a : m) {
      if (a.at % a.align) ++failures, fprintf(stderr, "n %llu: %s is not aligned\n", (unsigned long long)n, a.name);
      if (a.at < lo || a.at + a.bytes > hi)
        ++failures, fprintf(stderr, "n %llu: %s leaves the %zu bytes\n", (unsigned long long)n, a.name, total);
    }
    std::sort(m.begin(), m.end(), [](const Member& a, const Member& b) { return a.at < b.at; });
    for (size_t k = 0; k + 1 < m.size(); ++k)
      if (m[k].at + m[k].bytes > m[k + 1].at)
        ++failures, fprintf(stderr, "n %llu: %s and %s overlap\n", (unsigned long long)n, m[k].name, m[k + 1].name);
    const size_t pub = hf3fs_crc_server_read_scratch_bytes(n, n);
    const size_t own = (16 + n * (8 + 8 + 4) + 63) / 64 * 64 + 64;
    if (pub < own + total + 16 || pub % 4)
      ++failures, fprintf(stderr, "n %llu: the public size %zu does not cover %zu\n", (unsigned long long)n, pub,
                          own + total + 16);
    printf("size server_read_scratch_bytes/%llu %zu\n", (unsigned long long)n, total);
    printf("size hf3fs_crc_server_read_scratch_bytes/%llu %zu\n", (unsigned long long)n, pub);
  }
  if (hf3fs_crc_server_read_scratch_bytes((1ull << 30) + 1, 0) || hf3fs_crc_server_read_scratch_bytes(1, (1ull << 30) + 1))
    ++failures, fprintf(stderr, "a rejected count has a size\n");
  if (failures) return fprintf(stderr, "%d layout failures\n", failures), 1;
  printf("ALL OK\n");
  return 0;
}
