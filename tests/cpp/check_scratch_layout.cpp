// check_scratch_layout.cpp -- every scratch carve fits its byte count, and no byte count moves.
// Needs no GPU: only sizing and carving functions of libhf3fs_crc.so are called, on a fake base.
//
// Fit: each layout (update, order, version, engine, sync, md5, forward) is carved at a 16-byte
// aligned base and every member must be 16-byte aligned, disjoint from the others and inside
// [base, base + *_scratch_bytes).  A member that outgrows the slack term of its size fails here
// instead of becoming a kernel that writes past the pair's buffer.
// Cover: the public sizes of the record batches (client read, client write, forward) are at least
// what a call takes on a device of 256 CUs, restated here.
// Sizes: "size <key> <value>" lines, compared by tests/test_scratch_layout.py with
// tests/golden/scratch_sizes.json.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/hf3fs_crc.h"
#include "../../3fs_amd/csrc/client_write_kernels.h"
#include "../../3fs_amd/csrc/digest_kernels.h"
#include "../../3fs_amd/csrc/engine_kernels.h"
#include "../../3fs_amd/csrc/forward_kernels.h"
#include "../../3fs_amd/csrc/md5_kernels.h"
#include "../../3fs_amd/csrc/order_kernels.h"
#include "../../3fs_amd/csrc/sync_kernels.h"
#include "../../3fs_amd/csrc/update_kernels.h"
#include "../../3fs_amd/csrc/version_kernels.h"

using namespace hf3fs_crc;

namespace {

int g_failures = 0;
uint8_t* const kBase = (uint8_t*)0x7f0000000010ull;  // 16-byte aligned, not 64

struct Member {
  const char* name;
  const void* ptr;
  size_t bytes, align;
};

void check_fit(const std::string& what, size_t total, std::vector<Member> m) {
  const uintptr_t lo = (uintptr_t)kBase, hi = lo + total;
  for (const Member& x : m) {
    const uintptr_t p = (uintptr_t)x.ptr;
    if (p % x.align) ++g_failures, fprintf(stderr, "%s: %s is not %zu-byte aligned\n", what.c_str(), x.name, x.align);
    if (p < lo || p > hi || x.bytes > hi - p)
      ++g_failures, fprintf(stderr, "%s: %s [+%zu, %zu bytes) leaves the %zu bytes\n", what.c_str(), x.name,
                            (size_t)(p - lo), x.bytes, total);
  }
  m.erase(std::remove_if(m.begin(), m.end(), [](const Member& x) { return x.bytes == 0; }), m.end());
  std::sort(m.begin(), m.end(), [](const Member& a, const Member& b) { return a.ptr < b.ptr; });
  for (size_t i = 1; i < m.size(); ++i)
    if ((uintptr_t)m[i - 1].ptr + m[i - 1].bytes > (uintptr_t)m[i].ptr)
      ++g_failures, fprintf(stderr, "%s: %s overlaps %s\n", what.c_str(), m[i - 1].name, m[i].name);
}

template <class... A>
std::string key(const char* name, A... a) {
  std::string k = name;
  for (unsigned long long v : {(unsigned long long)a...}) k += "/" + std::to_string(v);
  return k;
}
void size_line(const std::string& k, unsigned long long v) { printf("size %s %llu\n", k.c_str(), v); }

std::vector<Member> version_members(const VersionScratch& v, uint64_t n) {
  return {{"vaddr", v.vaddr, n * 8, 16}, {"vlen", v.vlen, n * 8, 16}, {"dec", v.dec, n * 4, 16}, {"vout", v.vout, n * 4, 16}};
}
std::vector<Member> forward_members(const ForwardScratch& f, uint64_t n) {
  return {{"count", f.count, kForwardBlocksMax * 4, 16}, {"take", f.take, n, 16}};
}
void check_n(uint64_t n) {
  // update: every nw, piece table, records per IO and ticketed pieces
  for (uint32_t rpi : {2u, 4u})
    for (uint32_t pieces : {0u, 8u}) {
      const uint64_t records = update_record_cap(n, rpi, pieces);
      size_line(key("update_record_cap", n, rpi, pieces), records);
      for (uint32_t nw : {1u, 7u, 1024u, 8192u})
        for (uint64_t ptab : {(uint64_t)0, (uint64_t)5, 516 * n}) {
          const size_t total = update_scratch_bytes(n, records, nw, ptab);
          size_line(key("update_scratch_bytes", n, rpi, pieces, nw, ptab), total);
          UpdateScratch s;
          update_scratch_carve(kBase, n, records, pieces, 64 << 10, nw, ptab, &s);
          check_fit(key("update", n, rpi, pieces, nw, ptab), total,
                    {{"ctl", s.ctl, kCtlWords * 4, 16},
                     {"pre_addr", s.pre_addr, 2 * n * 8, 16},
                     {"pre_len", s.pre_len, 2 * n * 8, 16},
                     {"pre_start", s.pre_start, 2 * n * 4, 16},
                     {"pre_out", s.pre_out, 2 * n * 4, 16},
                     {"post_addr", s.post_addr, 2 * n * 8, 16},
                     {"post_len", s.post_len, 2 * n * 8, 16},
                     {"post_start", s.post_start, 2 * n * 4, 16},
                     {"post_out", s.post_out, 2 * n * 4, 16},
                     {"tasks", s.tasks, records * sizeof(ApplyTask), 16},
                     {"ptab", s.ptab, ptab * 4, 16},
                     {"run_partial", s.run_partial, kRunBlocksMax * 8, 16},
                     {"run_bal", s.run_bal, (nw + 1) * 4ull, 16},
                     {"run_boff", s.run_boff, (nw + 1) * 8ull, 16}});
        }
    }
  {
    const size_t total = order_scratch_bytes(n);
    size_line(key("order_scratch_bytes", n), total);
    OrderScratch s;
    order_scratch_carve(kBase, n, &s);
    const uint64_t t = s.table;
    check_fit(key("order", n), total,
              {{"ctl", s.ctl, 64, 16},         {"keys", s.keys, t * 8, 16},     {"head", s.head, t * 4, 16},
               {"next", s.next, n * 4, 16},    {"slot", s.slot, n * 4, 16},     {"rank", s.rank, n * 4, 16},
               {"pred", s.pred, n * 4, 16},    {"succ", s.succ, n * 4, 16},
               {"round", s.round, n * sizeof(hf3fs_crc_update_io), 16}});
  }
  {
    const size_t total = version_scratch_bytes(n);
    size_line(key("version_scratch_bytes", n), total);
    VersionScratch s;
    version_scratch_carve(kBase, n, &s);
    check_fit(key("version", n), total, version_members(s, n));
  }
  {
    const size_t total = engine_scratch_bytes(n);
    size_line(key("engine_scratch_bytes", n), total);
    EngineScratch s;
    engine_scratch_carve(kBase, n, &s);
    std::vector<Member> m = version_members(s.v, n);
    m.push_back({"rdst", s.rdst, n * 8, 16});
    check_fit(key("engine", n), total, m);
  }
  for (uint64_t nr : {(uint64_t)0, (uint64_t)1, (uint64_t)17, (uint64_t)4097}) {
    const size_t total = sync_scratch_bytes(n, nr);
    size_line(key("sync_scratch_bytes", n, nr), total);
    size_line(key("hf3fs_crc_sync_plan_scratch_bytes", n, nr), hf3fs_crc_sync_plan_scratch_bytes(n, nr));
    SyncScratch s;
    sync_scratch_carve(kBase, n, nr, &s);
    check_fit(key("sync", n, nr), total,
              {{"ctl", s.ctl, kSyncCtlWords * 4, 16},
               {"table", s.table, s.slots * 4ull, 16},
               {"claim", s.claim, n * 4, 16},
               {"rfound", s.rfound, nr * 4, 16},
               {"lcount", s.lcount, kSyncBlocksMax * 4, 16},
               {"rcount", s.rcount, kSyncBlocksMax * 4, 16},
               {"lcode", s.lcode, n, 16},
               {"rcode", s.rcode, nr, 16}});
  }
  {
    const size_t total = md5_scratch_bytes(n);
    size_line(key("md5_scratch_bytes", n), total);
    size_line(key("hf3fs_crc_md5_scratch_bytes", n), hf3fs_crc_md5_scratch_bytes(n));
    Md5Scratch s;
    md5_scratch_carve(kBase, n, &s);
    check_fit(key("md5", n), total,
              {{"blocks", s.blocks, n * 8, 16}, {"perm", s.perm, n * 4, 16}, {"count", s.count, 256ull * s.shares * 4, 16}});
  }
  const size_t forward_bytes = forward_scratch_bytes(n);
  {
    size_line(key("forward_scratch_bytes", n), forward_bytes);
    size_line(key("hf3fs_crc_forward_scratch_bytes", n), hf3fs_crc_forward_scratch_bytes(n));
    ForwardScratch s;
    forward_scratch_carve(kBase, n, &s);
    check_fit(key("forward", n), forward_bytes, forward_members(s, n));
  }
  size_line(key("hf3fs_crc_client_read_scratch_bytes", n), hf3fs_crc_client_read_scratch_bytes(n, n));
  for (uint32_t splits : {1u, 4u})
    for (uint32_t fill : {0u, 1u})
      size_line(key("digest_scratch_bytes", n, splits, fill), digest_scratch_bytes(n, splits, fill != 0));
}

// The public sizes of the record batches cover what a call of n records takes on a device of 256
// CUs.  The need is restated here, independently of the library: the carve {ctl[4], addr[n],
// len[n], v[n]} up to a multiple of 64, the byte-run tables of min(kRunBlocksMax, max(1, n / 256))
// blocks and nw waves where the call reserves them, 64 spare bytes, and the caller's tail.
void check_record_cover(uint64_t n) {
  const size_t nw = 256 * kWaves, blocks = std::min<uint64_t>(kRunBlocksMax, std::max<uint64_t>(1, n / 256));
  const size_t plain = (16 + n * (8 + 8 + 4) + 63) / 64 * 64 + 64;
  const size_t with_runs = plain + (blocks + 2 * (nw + 1)) * 8 + (nw + 1) * 4;
  const struct {
    const char* name;
    size_t pub, need;
  } sizes[] = {{"client_read", hf3fs_crc_client_read_scratch_bytes(n, n), plain},
               {"client_write", hf3fs_crc_client_write_scratch_bytes(n, n), with_runs},
               {"forward", hf3fs_crc_forward_scratch_bytes(n), with_runs + forward_scratch_bytes(n) + 16}};
  for (const auto& x : sizes)
    if (x.pub < x.need)
      ++g_failures, fprintf(stderr, "n %llu: hf3fs_crc_%s_scratch_bytes is %zu, a call takes %zu\n",
                            (unsigned long long)n, x.name, x.pub, x.need);
  size_line(key("client_write_scratch_bytes", n), client_write_scratch_bytes(n));
  size_line(key("hf3fs_crc_client_write_scratch_bytes", n), hf3fs_crc_client_write_scratch_bytes(n, n));
}

}  // namespace

int main() {
  for (uint64_t n : {1ull, 2ull, 3ull, 15ull, 16ull, 17ull, 255ull, 256ull, 257ull, 4096ull, 65537ull, 1000003ull}) check_n(n);
  for (uint64_t n : {1ull, 2ull, 15ull, 16ull, 17ull, 255ull, 256ull, 257ull, 4096ull, 65537ull, 1000003ull, 1ull << 30})
    check_record_cover(n);
  if (g_failures) return fprintf(stderr, "%d layout failures\n", g_failures), 1;
  printf("ALL OK\n");
  return 0;
}
