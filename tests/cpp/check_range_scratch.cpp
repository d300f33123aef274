// check_range_scratch.cpp -- the scratch carve of hf3fs_crc_range_query fits its byte count, and the
// public sizing function is that count.  Needs no GPU: only sizing and carving functions of
// libhf3fs_crc.so are called, on a fake base.  A program of its own beside check_scratch_layout.cpp
// and check_server_read_scratch.cpp, whose golden sizes stay as they are.
//
// Fit: the layout is carved at a 16-byte aligned base; every member must be aligned to its element,
// disjoint from the others and inside [base, base + range_scratch_bytes(n_meta, n_ops)).
#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../include/hf3fs_crc.h"
#include "../../3fs_amd/csrc/range_kernels.h"

using namespace hf3fs_crc;

int main() {
  int failures = 0;
  uint8_t* const base = (uint8_t*)0x7f0000000010ull;  // 16-byte aligned, not 64
  const uint64_t counts[] = {0, 1, 2, 15, 16, 17, 255, 256, 257, 4096, 65537, 1000003, 1ull << 30};
  for (uint64_t n : counts)
    for (uint64_t q : {0ull, 1ull, 3ull, 256ull, 70001ull, 1ull << 30}) {
      const size_t total = range_scratch_bytes(n, q);
      RangeScratch s;
      range_scratch_carve(base, n, q, &s);
      struct Member {
        const char* name;
        uintptr_t at;
        size_t bytes, align;
      };
      std::vector<Member> m = {{"len_pre", (uintptr_t)s.len_pre, (n + 1) * 8, 8},
                               {"op_off", (uintptr_t)s.op_off, (q + 1) * 8, 8},
                               {"share_len", (uintptr_t)s.share_len, kRangeBlocksMax * 8, 8},
                               {"share_list", (uintptr_t)s.share_list, kRangeBlocksMax * 8, 8},
                               {"share_chunks", (uintptr_t)s.share_chunks, kRangeBlocksMax * 8, 8},
                               {"cnt_pre", (uintptr_t)s.cnt_pre, (n + 1) * 4, 4},
                               {"op_top", (uintptr_t)s.op_top, q * 4, 4},
                               {"share_cnt", (uintptr_t)s.share_cnt, kRangeBlocksMax * 4, 4},
                               {"share_bad", (uintptr_t)s.share_bad, kRangeBlocksMax * 4, 4},
                               {"share_ok", (uintptr_t)s.share_ok, kRangeBlocksMax * 4, 4},
                               {"ctl", (uintptr_t)s.ctl, 16, 4}};
      const uintptr_t lo = (uintptr_t)base, hi = lo + total;
      for (const Member& a : m) {
        if (a.at % a.align)
          ++failures, fprintf(stderr, "n %llu q %llu: %s is not aligned\n", (unsigned long long)n, (unsigned long long)q, a.name);
        if (a.at < lo || a.at + a.bytes > hi)
          ++failures, fprintf(stderr, "n %llu q %llu: %s leaves the %zu bytes\n", (unsigned long long)n,
                              (unsigned long long)q, a.name, total);
      }
      std::stable_sort(m.begin(), m.end(), [](const Member& a, const Member& b) { return a.at < b.at; });
      for (size_t k = 0; k + 1 < m.size(); ++k)
        if (m[k].at + m[k].bytes > m[k + 1].at)
          ++failures, fprintf(stderr, "n %llu q %llu: %s and %s overlap\n", (unsigned long long)n, (unsigned long long)q,
                              m[k].name, m[k + 1].name);
      const size_t pub = hf3fs_crc_range_query_scratch_bytes(n, q);
      if (pub != total || pub % 16)
        ++failures, fprintf(stderr, "n %llu q %llu: the public size %zu is not %zu\n", (unsigned long long)n,
                            (unsigned long long)q, pub, total);
      printf("size range_scratch_bytes/%llu/%llu %zu\n", (unsigned long long)n, (unsigned long long)q, total);
    }
  if (hf3fs_crc_range_query_scratch_bytes((1ull << 30) + 1, 0) || hf3fs_crc_range_query_scratch_bytes(1, (1ull << 30) + 1))
    ++failures, fprintf(stderr, "a rejected count has a size\n");
  if (failures) return fprintf(stderr, "%d layout failures\n", failures), 1;
  printf("ALL OK\n");
  return 0;
}
