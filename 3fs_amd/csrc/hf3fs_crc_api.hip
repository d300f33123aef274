// hf3fs_crc_api.hip -- C ABI of libhf3fs_crc.so (declared in include/hf3fs_crc.h).
//
// Host side of the boundary: per-device contexts (constant tables in HBM, built by
// device_tables.cc; one record per (stream, thread) pair; memory of captured calls in
// capture_scratch.hip), launch planning and argument validation.  All byte hashing happens in the
// HIP kernels of crc_kernels.hip; the host only does O(log n) scalar algebra
// (combine/shift of 32-bit values), exactly like ChecksumInfo::combine does on
// the reference's host (Common.h:179-198).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/hf3fs_crc.h"
#include "aux_kernels.h"
#include "capture_scratch.h"
#include "client_read_kernels.h"
#include "client_read_plan.h"  // kClientMaxCount
#include "client_write_kernels.h"
#include "client_write_plan.h"  // kClientWriteMaxCount
#include "frame_kernels.h"
#include "crc_kernels.h"
#include "digest_kernels.h"
#include "engine_kernels.h"
#include "forward_kernels.h"
#include "forward_plan.h"  // kForwardMaxJobs
#include "internal.h"
#include "md5_kernels.h"
#include "options.h"
#include "order_kernels.h"
#include "range_kernels.h"
#include "range_plan.h"  // kRangeMaxCount
#include "server_read_kernels.h"
#include "server_read_plan.h"  // kServerReadMaxCount
#include "sync_kernels.h"
#include "update_kernels.h"
#include "update_plan.h"  // kPlanRanges
#include "version_kernels.h"

static_assert(sizeof(hf3fs_crc_update_io) == 56, "hf3fs_crc_update_io ABI layout");
static_assert(sizeof(hf3fs_crc_read_io) == 48, "hf3fs_crc_read_io ABI layout");
static_assert(sizeof(hf3fs_crc_client_read_io) == 40 && sizeof(hf3fs_crc_client_read_result) == 24,
              "hf3fs_crc_client_read_io / _result ABI layout");
static_assert(sizeof(hf3fs_crc_client_write_io) == 64 && offsetof(hf3fs_crc_client_write_io, data) == 0 &&
                  offsetof(hf3fs_crc_client_write_io, buf_base) == 8 &&
                  offsetof(hf3fs_crc_client_write_io, buf_size) == 16 &&
                  offsetof(hf3fs_crc_client_write_io, offset) == 24 &&
                  offsetof(hf3fs_crc_client_write_io, length) == 28 &&
                  offsetof(hf3fs_crc_client_write_io, chunk_size) == 32 &&
                  offsetof(hf3fs_crc_client_write_io, checksum) == 36 &&
                  offsetof(hf3fs_crc_client_write_io, checksum_type) == 40 &&
                  offsetof(hf3fs_crc_client_write_io, send_inline) == 41 &&
                  offsetof(hf3fs_crc_client_write_io, reserved0) == 42 &&
                  offsetof(hf3fs_crc_client_write_io, status) == 44 &&
                  offsetof(hf3fs_crc_client_write_io, status_in) == 48 &&
                  offsetof(hf3fs_crc_client_write_io, result_len) == 52 &&
                  offsetof(hf3fs_crc_client_write_io, result_checksum) == 56 &&
                  offsetof(hf3fs_crc_client_write_io, result_checksum_type) == 60 &&
                  offsetof(hf3fs_crc_client_write_io, reserved1) == 61,
              "hf3fs_crc_client_write_io ABI layout");
static_assert(sizeof(hf3fs_crc_client_write_file) == 24 && offsetof(hf3fs_crc_client_write_file, length) == 0 &&
                  offsetof(hf3fs_crc_client_write_file, value) == 8 &&
                  offsetof(hf3fs_crc_client_write_file, type) == 12 &&
                  offsetof(hf3fs_crc_client_write_file, reserved) == 13 &&
                  offsetof(hf3fs_crc_client_write_file, status) == 16 &&
                  offsetof(hf3fs_crc_client_write_file, failed_io) == 20,
              "hf3fs_crc_client_write_file ABI layout");
static_assert(sizeof(hf3fs_crc_block_digest) == 24, "hf3fs_crc_block_digest ABI layout");
static_assert(sizeof(hf3fs_crc_file_digest) == 24, "hf3fs_crc_file_digest ABI layout");
static_assert(sizeof(hf3fs_crc_scrub_io) == 32, "hf3fs_crc_scrub_io ABI layout");
static_assert(sizeof(hf3fs_crc_sync_meta) == 48, "hf3fs_crc_sync_meta ABI layout");
static_assert(sizeof(hf3fs_crc_md5_seg) == 16 && sizeof(hf3fs_crc_md5_state) == 96, "hf3fs_crc_md5 ABI layout");
static_assert(sizeof(hf3fs_crc_frame) == 24, "hf3fs_crc_frame ABI layout");
static_assert(sizeof(hf3fs_crc_engine_meta) == 120, "hf3fs_crc_engine_meta ABI layout");
static_assert(sizeof(hf3fs_crc_anomaly) == 72, "hf3fs_crc_anomaly ABI layout");
static_assert(sizeof(hf3fs_crc_engine_job) == 104 && alignof(hf3fs_crc_engine_job) == 8,
              "hf3fs_crc_engine_job ABI layout");

using namespace hf3fs_crc;

namespace {

#define HIP_OR_FAIL(expr)                                                                                    \
  do {                                                                                                       \
    hipError_t _e = (expr);                                                                                  \
    if (_e != hipSuccess) return fail(HF3FS_CRC_DEVICE_ERROR, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                      __FILE__, __LINE__);                                                   \
  } while (0)

bool valid_type(uint8_t t) { return t == kTypeNone || t == kTypeCrc32c || t == kTypeCrc32; }

// Work queued by one thread on one stream is ordered, so per-(stream, thread)
// state is reused safely by that pair; no two pairs ever share it (two threads
// on the null stream, or on one stream handle, interleave their launches).
using StreamKey = std::pair<hipStream_t, std::thread::id>;
inline StreamKey stream_key(hipStream_t s) { return {s, std::this_thread::get_id()}; }

struct Scratch {
  uint32_t* ptr = nullptr;
  size_t words = 0;
};
// A side stream with a fork and a join event: the update batch's one-shot apply runs beside
// the finalize of every verdict.  Per pair, so that two threads capturing
// graphs never fork into one stream.
struct Side {
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
constexpr uint32_t kNoHint = ~0u;
// Everything the library keeps for one (stream, thread) pair, each member made on first use.
// Only uncaptured calls use the device memory here: a captured call's belongs to its graph.
struct PairState {
  Scratch verify;               // verify values of calls with d_computed == NULL
  Scratch call;                 // scratch of update / record / frame / digest batches
  Scratch balance;              // byte-balance region of whole-range launches (bal_words words)
  uint32_t* counter = nullptr;  // ticket counter: a 16 B slot of a shared slab, not owned
  uint32_t hint[4] = {kNoHint, kNoHint, kNoHint, kNoHint};  // slots of the one-shot apply's pinned hint
                                                            // words: [0] update_batch, [1] round 0 of
                                                            // update_ordered, [2] update_cow_batch,
                                                            // [3] round 0 of update_engine
  Side side;
};

// The end of a pair record that left the context (release_stream, shutdown), never with the
// context locked: waits for the side stream, destroys it and its events and frees the three
// buffers (an error of the frees is returned).  The counter and hint slots stay in their slabs.
hipError_t destroy_pair(const PairState& p) {
  if (p.side.side) {
    (void)hipStreamSynchronize(p.side.side);
    (void)hipEventDestroy(p.side.fork);
    (void)hipEventDestroy(p.side.join);
    (void)hipStreamDestroy(p.side.side);
  }
  hipError_t err = hipSuccess;
  for (const Scratch* b : {&p.verify, &p.call, &p.balance})
    if (b->ptr)
      if (const hipError_t e = hipFree(b->ptr)) err = e;
  return err;
}

struct Context {
  int device = -1;
  int cus = 0;
  DeviceTables* tables = nullptr;  // device
  hf3fs_crc_anomaly* diag = nullptr;  // device: the self-check's record (hf3fs_crc_anomalies)
  std::mutex mu;                   // guards everything below
  std::map<StreamKey, PairState> pairs;
  // Ticket counters of the dynamic task queues (16 B each, zeroed on the launch
  // stream right before the launch).  A (stream, thread) pair owns one counter
  // for all its launches (they are stream-ordered), a slot of a slab.
  static constexpr uint32_t kSlabSlots = 16384;
  std::vector<uint32_t*> slabs;
  uint32_t slab_used = kSlabSlots;
  // Byte-balance scratch of whole-range launches: partial sums + per-wave task boundaries.
  static constexpr uint32_t kBalBlocksMax = 1024;
  size_t bal_words() const { return (2 * kBalBlocksMax + (size_t)cus * kWaves + 1 + 63) / 64 * 64; }
  // One-shot apply grid hints (update_batch): a pinned word per (stream, thread) pair where the
  // apply kernel leaves (pieces << 32 | n) of its call; the pair's next call sizes its one-shot
  // grid from it.  One slab for the process's pairs (a word of a captured call's graph stays
  // valid until shutdown); more pairs than slots share words (only the grid's fit suffers).
  // hint_uses counts the live pairs of a slot: release_stream puts a slot on the free list
  // when its last pair goes.
  static constexpr uint32_t kHintSlots = 4096;
  uint64_t* hint_host = nullptr;
  uint64_t* hint_dev = nullptr;
  uint32_t hint_uses[kHintSlots] = {};
  std::vector<uint32_t> hint_free;
  uint32_t hint_next = 0;
  int hint_word(hipStream_t s, int which, uint64_t** host, uint64_t** dev) {
    std::lock_guard<std::mutex> lk(mu);
    if (!hint_host) {  // (the pair's first update call may be a captured one)
      RelaxedCapture relaxed;
      HIP_OR_FAIL(relaxed.err);
      HIP_OR_FAIL(hipHostMalloc((void**)&hint_host, kHintSlots * 8, hipHostMallocMapped | hipHostMallocCoherent));
      memset(hint_host, 0, kHintSlots * 8);
      HIP_OR_FAIL(hipHostGetDevicePointer((void**)&hint_dev, hint_host, 0));
    }
    uint32_t& slot = pairs[stream_key(s)].hint[which];
    if (slot == kNoHint) {
      if (!hint_free.empty()) {
        slot = hint_free.back();
        hint_free.pop_back();
      } else {
        slot = hint_next++ % kHintSlots;
      }
      ++hint_uses[slot];
    }
    *host = hint_host + slot;
    *dev = hint_dev + slot;
    return HF3FS_CRC_OK;
  }
  // The pair's side stream, created in relaxed capture mode (a call may be captured).
  int side_of(hipStream_t s, Side* out) {
    {
      std::lock_guard<std::mutex> lk(mu);
      *out = pairs[stream_key(s)].side;
    }
    if (out->side) return HF3FS_CRC_OK;
    Side n;
    hipError_t e;
    {
      RelaxedCapture relaxed;
      e = relaxed.err;
      if (e == hipSuccess) e = hipStreamCreateWithFlags(&n.side, hipStreamNonBlocking);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&n.fork, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&n.join, hipEventDisableTiming);
    }
    if (e != hipSuccess) {
      if (n.join) (void)hipEventDestroy(n.join);
      if (n.fork) (void)hipEventDestroy(n.fork);
      if (n.side) (void)hipStreamDestroy(n.side);
      return fail(HF3FS_CRC_DEVICE_ERROR, "side stream: %s", hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lk(mu);
    pairs[stream_key(s)].side = n;
    *out = n;
    return HF3FS_CRC_OK;
  }
  // host staging (hf3fs_crc_create_host), one caller at a time
  std::mutex stage_mu;
  static constexpr size_t kStage = 32ull << 20;
  uint8_t* pinned[2] = {nullptr, nullptr};
  uint8_t* dstage[2] = {nullptr, nullptr};
  uint64_t* pdesc[2] = {nullptr, nullptr};  // pinned descriptors (addr, len pairs) + out
  uint64_t* ddesc[2] = {nullptr, nullptr};
  hipStream_t streams[2] = {nullptr, nullptr};
};

std::mutex g_ctx_mu;
std::vector<std::unique_ptr<Context>> g_ctx;

int get_context(Context** out) {
  int dev = 0;
  HIP_OR_FAIL(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  if ((int)g_ctx.size() <= dev) g_ctx.resize(dev + 1);
  if (!g_ctx[dev]) {
    auto c = std::make_unique<Context>();
    c->device = dev;
    HIP_OR_FAIL(hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, dev));
    auto host = std::make_unique<DeviceTables>();
    build_device_tables(*host);
    // The process's first library call may sit inside a stream capture: the allocations in
    // relaxed capture mode, the uploads on a stream of their own and waited for there (nothing
    // touches the null stream or the capturing one).
    RelaxedCapture relaxed;
    HIP_OR_FAIL(relaxed.err);
    const hf3fs_crc_anomaly none{};
    hipStream_t up = nullptr;
    HIP_OR_FAIL(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
    hipError_t e = hipMalloc(&c->tables, sizeof(DeviceTables));
    if (e == hipSuccess) e = hipMalloc(&c->diag, sizeof(hf3fs_crc_anomaly));
    if (e == hipSuccess) e = hipMemcpyAsync(c->tables, host.get(), sizeof(DeviceTables), hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = hipMemcpyAsync(c->diag, &none, sizeof(none), hipMemcpyHostToDevice, up);
    const hipError_t waited = hipStreamSynchronize(up);  // (also after an error: `none` and `host` end here)
    if (e == hipSuccess) e = waited;
    (void)hipStreamDestroy(up);
    if (e != hipSuccess) {
      if (c->diag) (void)hipFree(c->diag);
      if (c->tables) (void)hipFree(c->tables);
      return fail(HF3FS_CRC_DEVICE_ERROR, "context tables: %s", hipGetErrorString(e));
    }
    (void)options();  // the environment snapshot, once per process
    g_ctx[dev] = std::move(c);
  }
  *out = g_ctx[dev].get();
  return HF3FS_CRC_OK;
}

// Is the call on s being captured into a graph?
int is_capturing(hipStream_t s, bool* capturing) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  HIP_OR_FAIL(hipStreamIsCapturing(s, &cs));
  *capturing = cs != hipStreamCaptureStatusNone;
  return HF3FS_CRC_OK;
}

// What a roomy pair buffer of `words` is sized to when it is first made.
constexpr size_t roomy_words(size_t words) { return (words + 65535) / 65536 * 65536; }

std::atomic<uint64_t> g_pair_allocs{0};  // allocations and growths of pair buffers (hf3fs_crc_pair_scratch_stats)

// The calling (stream, thread) pair's buffer `member`, at least `words` long (roomy: sized
// up to a multiple of 64 Ki words and at least doubled, else exactly `words`).  Only that
// pair ever uses the buffer and only this thread launched work on it, all of it on s, so
// growth detaches it under the lock and waits for the stream, frees and allocates with the
// lock released (other threads' calls never wait for this stream; not graph-capturable, a
// warm-up call of the largest size avoids it), then publishes the new buffer.  On a failure
// before the new buffer exists the old one goes back into the record (nothing leaks).
int pair_buffer(Context* c, Scratch PairState::*member, hipStream_t s, size_t words, bool roomy, uint32_t** out) {
  const StreamKey key = stream_key(s);
  Scratch e;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    Scratch& slot = c->pairs[key].*member;
    e = slot;
    if (slot.words < words) slot = Scratch{};
  }
  if (e.words < words) {
    g_pair_allocs.fetch_add(1, std::memory_order_relaxed);
    const size_t grow_to = roomy ? std::max<size_t>(roomy_words(words), 2 * e.words) : words;
    hipError_t err = e.ptr ? hipStreamSynchronize(s) : hipSuccess;
    if (err == hipSuccess && e.ptr) {
      err = hipFree(e.ptr);
      if (err == hipSuccess) e = Scratch{};
    }
    uint32_t* fresh = nullptr;
    if (err == hipSuccess) err = hipMalloc(&fresh, grow_to * sizeof(uint32_t));
    if (err == hipSuccess) e = Scratch{fresh, grow_to};
    std::lock_guard<std::mutex> lk(c->mu);
    c->pairs[key].*member = e;  // the new buffer, or after a failure the old one (none, if it was freed)
    if (err != hipSuccess)
      return fail(HF3FS_CRC_DEVICE_ERROR, "scratch growth to %zu words: %s", grow_to, hipGetErrorString(err));
  }
  *out = e.ptr;
  return HF3FS_CRC_OK;
}

// The pair's ticket counter: a slot carved from the context's slabs on first use.
int pair_counter(Context* c, hipStream_t s, uint32_t** out) {
  std::lock_guard<std::mutex> lk(c->mu);
  uint32_t*& q = c->pairs[stream_key(s)].counter;
  if (!q) {
    if (c->slab_used == Context::kSlabSlots) {
      uint32_t* slab = nullptr;
      HIP_OR_FAIL(hipMalloc(&slab, Context::kSlabSlots * 16));
      c->slabs.push_back(slab);
      c->slab_used = 0;
    }
    q = c->slabs.back() + 4 * c->slab_used++;
  }
  *out = q;
  return HF3FS_CRC_OK;
}

// Device memory of one call on s: library-owned hipMalloc memory, never the stream-ordered
// pool (rounds 1 and 3 saw the first DELTA update of a process -- the first call whose
// per-call hipMallocAsync scratch the pool had to grow -- verify a correct payload as
// mismatched in 2-3 of 16 fresh processes, and a retry pass).  Outside a
// stream capture it is the calling (stream, thread) pair's persistent member.  During a
// capture it is memory of the captured call alone, owned by the captured graph and freed
// after the graph is gone (capture_malloc): the graph may be replayed on any stream, and a
// replay never touches pair memory that release_stream or a later growth freed.
// Option poison (test only): the words of a verify, call or balance buffer are first filled with
// that pattern on the stream, so a call that read a word before writing it (a bal[] boundary
// k_bal_assign never placed) would see junk (tests/test_gpu_parity.py::
// test_update_batch_poisoned_scratch, tests/test_gpu_batch_contexts.py).
enum class Mem { kVerify, kCall, kBalance, kCounter };
int call_memory(Context* c, hipStream_t s, Mem what, size_t words, uint32_t** out) {
  bool capturing = false;
  if (int rc = is_capturing(s, &capturing)) return rc;
  if (capturing) {
    HIP_OR_FAIL(capture_malloc(c->device, s, words * 4, (void**)out));
  } else {
    reap_captured();
    Scratch PairState::*const buffer[] = {&PairState::verify, &PairState::call, &PairState::balance};
    const int rc = what == Mem::kCounter ? pair_counter(c, s, out)
                                         : pair_buffer(c, buffer[(int)what], s, words, what == Mem::kCall, out);
    if (rc) return rc;
  }
  if (what == Mem::kVerify || what == Mem::kCall || what == Mem::kBalance)
    if (const uint32_t pattern = options().poison.load()) HIP_OR_FAIL(launch_fill_words(*out, words, pattern, s));
  return HF3FS_CRC_OK;
}

// Scratch of one batch call (update, record jobs, frames, file digest).
int call_scratch(Context* c, hipStream_t s, size_t bytes, void** out) {
  uint32_t* p = nullptr;
  const int rc = call_memory(c, s, Mem::kCall, (bytes + 3) / 4, &p);
  *out = p;
  return rc;
}

// Cross-task head prefetch for whole-buffer tasks on a static stride (DESIGN.md
// §3.1), by default only for batches whose longest range (the kernel's bound:
// the device-side maximum of record jobs, else the task size) fits the
// prefetched head four times over (A/B profiles/r01_ab_pipe.jsonl: f4 frames <= 16 KiB
// +3.5 %, d5 KV blocks <= 64 KiB -3 %, d2 4 MiB flat).
constexpr uint64_t kPipeMaxLen = 16 << 10;  // 4 x the prefetched head (kHashPrefetch = 4 blocks of 1 KiB)

// Tasks of seg_bytes each; as large as possible while leaving >= ~4 tasks per
// resident wave for balance (or seg_hint when the caller knows better).
// Option seg_kib overrides (tuning).
Plan make_plan(const Context* c, uint64_t n, uint64_t max_len, uint64_t seg_hint = 0) {
  Plan p;
  const Options& o = options();
  const uint64_t waves = (uint64_t)c->cus * kWaves;
  const uint64_t max_seg = std::max<uint64_t>(kBlockBytes, (max_len + kBlockBytes - 1) / kBlockBytes * kBlockBytes);
  uint64_t seg = max_seg;
  const uint64_t total = n * max_len;
  if (const uint32_t kib = o.seg_kib.load()) {
    seg = (uint64_t)kib * 1024;
  } else if (seg_hint) {
    seg = seg_hint;
  } else if (total / waves < 4 * seg) {
    uint64_t target = std::max<uint64_t>(total / (4 * waves), 64 << 10);
    uint64_t pow2 = 64 << 10;
    while (pow2 < target) pow2 <<= 1;
    seg = pow2;
  }
  seg = std::min(seg, max_seg);
  p.seg_bytes = seg;
  p.segs = std::max<uint64_t>(1, (max_len + seg - 1) / seg);
  const uint64_t tasks = n * p.segs;
  const uint64_t want = (tasks + kWaves - 1) / kWaves;
  p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)c->cus));
  p.queue = nullptr;
  p.dyn_max = nullptr;
  p.skip = nullptr;
  p.bal = nullptr;
  p.boff = nullptr;
  p.nt = o.nt.load() != 0;  // non-temporal streamed loads (A/B: profiles/r01_ab_bulk.json)
  const int pipe = o.pipe.load();
  p.pipe_max = pipe < 0 ? kPipeMaxLen : pipe ? ~uint64_t(0) : 0;
  p.range_stream = o.range_stream.load() != 0;
  return p;
}

// Ticket queues for ragged task sets, unless the static stride is forced (option static).
inline bool tickets_allowed() { return options().static_stride.load() == 0; }

// Zero what the launch accumulates into and hand it a freshly zeroed ticket
// counter (the kernel decides whether tickets pay for its task count).
int launch_prepare(Context* c, Plan& p, uint64_t n, uint32_t* out, hipStream_t s) {
  const uint64_t tasks = n * p.segs;
  if (tasks >= (1ull << 32)) return fail(HF3FS_CRC_INVALID_ARG, "too many tasks (%llu)", (unsigned long long)tasks);
  if (p.segs > 1 || p.dyn_max) HIP_OR_FAIL(launch_zero_words(out, n, s));
  p.queue = nullptr;
  if ((tasks > (uint64_t)p.grid * kWaves || p.dyn_max) && tickets_allowed()) {
    if (int rc = call_memory(c, s, Mem::kCounter, 4, &p.queue)) return rc;
    HIP_OR_FAIL(launch_zero_counter(p.queue, s));
  }
  return HF3FS_CRC_OK;
}

// Whole-range tasks on a static stride (more than 16 per wave, too long for
// the cross-task prefetch) get byte-balanced contiguous task ranges per wave:
// the stride leaves the slowest waves' summed lengths several sigma above the
// mean for ragged sizes (KVCache blocks of 4-64 KiB).  Option balance = 0: off.
template <class Src>
int plan_balance(Context* c, Plan& p, const Src& src, uint64_t n, uint64_t max_len, hipStream_t s) {
  const bool on = options().balance.load() != 0;
  const uint64_t nw = (uint64_t)p.grid * kWaves;
  // (the kernel drops its ticket queue for more than 16 tasks per wave)
  if (!on || p.segs != 1 || p.dyn_max || max_len <= p.pipe_max || n <= 16 * nw) return HF3FS_CRC_OK;
  uint32_t* sc = nullptr;
  if (int rc = call_memory(c, s, Mem::kBalance, c->bal_words(), &sc)) return rc;
  const uint32_t nblocks = (uint32_t)std::min<uint64_t>(Context::kBalBlocksMax, std::max<uint64_t>(1, n / 1024));
  uint64_t* partial = (uint64_t*)sc;
  uint32_t* bal = sc + 2 * Context::kBalBlocksMax;
  HIP_OR_FAIL(launch_balance(src, n, (uint32_t)nw, partial, nblocks, bal, s));
  p.bal = bal;
  // The kernel drops its ticket queue here (n > 16 nw), so the plan carries none: launch_poly takes
  // the range-stream kernel (option range_stream) only for a plan without a queue, and with the
  // counter launch_prepare handed over the option never reached it.
  p.queue = nullptr;
  return HF3FS_CRC_OK;
}

// Byte runs (launch_balance with boff): scratch for a ragged list of long
// ranges that every wave should split at exact byte shares of the batch.
struct ByteRuns {
  uint64_t* partial;
  uint32_t* bal;
  uint64_t* boff;
  uint32_t blocks;
  bool placed;  // bal / boff already placed on the stream (update prep's runs workgroup)
  uint32_t rep = 1;  // runs per wave (Plan::run_rep): bal / boff hold rep x W + 1 entries
};
// The tables of nw runs, not placed yet: partial[blocks], boff[nw + 1] in room for twice as many, bal[nw + 1].
constexpr size_t byte_runs_bytes(size_t blocks, size_t nw) { return (blocks + 2 * (nw + 1)) * 8 + (nw + 1) * 4; }
ByteRuns byte_runs_carve(void* base, uint32_t blocks, uint32_t nw, uint32_t rep) {
  uint64_t* partial = (uint64_t*)base;
  return {partial, (uint32_t*)(partial + blocks + 2 * (nw + 1)), partial + blocks, blocks, false, rep};
}

// zeroed_queue: the caller zeroed `out` and hands over a zeroed ticket counter
// (update_batch: one zeroing launch per call instead of two per hash pass).
// runs: hash as byte runs (out must be zeroed: the parts are xor-ed).
int run_ranges_list(Context* c, uint8_t type, const ListSource& src, uint64_t max_len, uint32_t* out,
                    hipStream_t s, uint64_t seg_hint = 0, const uint32_t* dyn_max = nullptr,
                    const uint32_t* skip = nullptr, uint32_t* zeroed_queue = nullptr,
                    const ByteRuns* runs = nullptr) {
  if (src.n == 0) return HF3FS_CRC_OK;
  Plan p = make_plan(c, src.n, max_len, seg_hint);
  p.dyn_max = dyn_max;
  p.skip = skip;
  if (dyn_max) p.grid = (uint32_t)c->cus;  // task count unknown on the host: full persistent grid
  if (runs) {
    p.grid = (uint32_t)c->cus;
    p.queue = nullptr;
    if (!runs->placed)
      HIP_OR_FAIL(launch_balance(src, src.n, p.grid * kWaves * runs->rep, runs->partial, runs->blocks, runs->bal, s,
                                 runs->boff));
    p.bal = runs->bal;
    p.boff = runs->boff;
    p.run_rep = runs->rep;
    HIP_OR_FAIL(launch_ranges_list(type, src, p, out, c->tables, s));
    return HF3FS_CRC_OK;
  }
  if (zeroed_queue) {
    const bool tickets = (src.n * p.segs > (uint64_t)p.grid * kWaves || dyn_max) && tickets_allowed();
    p.queue = tickets ? zeroed_queue : nullptr;
  } else if (int rc = launch_prepare(c, p, src.n, out, s)) {
    return rc;
  }
  if (int rc = plan_balance(c, p, src, src.n, max_len, s)) return rc;
  HIP_OR_FAIL(launch_ranges_list(type, src, p, out, c->tables, s));
  return HF3FS_CRC_OK;
}

// prep -> k_crc_ranges -> finalize over per-record jobs, with stream-ordered
// scratch {maxl[4], addr[n], len[n], v[n]}: the shape shared by the record
// batches (read results, scrub, frames).
// Scrub batches (whole stored chunks: their lengths are close to the bound) of
// n * max_len >= kRecordRunsBytes with max_len >= kRecordRunsMinLen hash as byte runs (every
// wave the same byte share, the balance placed on the device from the prep's lengths):
// 4096 x 4 MiB scrub records ran 3.5 % slower as 1 MiB ticketed segments (the planner's
// choice for a device-side length bound).  Read results keep the planner: their partial
// reads are far below the bound (the chunk size), and two balance launches would cost more
// than they save on a reaped batch of small reads.
constexpr uint64_t kRecordRunsBytes = 1ull << 30;
constexpr uint32_t kRecordRunsMinLen = 64 << 10;
constexpr uint64_t kRunWindowBytes = 4ull << 20;  // most bytes of one byte run (create_strided)

// What the carve takes without the caller's tail: {ctl[4], addr[n], len[n], v[n]} up to a multiple
// of 64 (the head), the byte-run tables of rblocks blocks and nw runs (with_runs), 64 spare bytes.
constexpr size_t record_head_bytes(uint64_t n) { return (16 + n * (8 + 8 + 4) + 63) / 64 * 64; }
constexpr size_t record_own_bytes(uint64_t n, size_t rblocks, size_t nw, bool with_runs) {
  return record_head_bytes(n) + (with_runs ? byte_runs_bytes(rblocks, nw) : 0) + 64;
}
// The public *_scratch_bytes functions size the tables for any device: kRunBlocksMax blocks and the
// 16,384 waves of 1024 CUs.
constexpr size_t kSizingWaves = 1024 * kWaves;

struct RecordOptions {
  const char* what;           // the call's name in an error
  bool runs_ok = false;       // a large batch hashes as byte runs
  bool reserve_runs = false;  // the byte-run tables are part of the size whatever max_len is, so that
                              // the pair's buffer depends on n alone
  size_t tail_bytes = 0;      // the caller's bytes behind the carve, for its fin (own is a multiple of 4),
  void** tail = nullptr;      // and where they start
};
template <class Prep, class Fin>
int run_record_jobs(Context* c, uint8_t type, uint64_t n, uint32_t max_len, hipStream_t s, Prep prep, Fin fin,
                    const RecordOptions& o) {
  const bool use_runs = o.runs_ok && max_len >= kRecordRunsMinLen && n * (uint64_t)max_len >= kRecordRunsBytes;
  const uint32_t nw = (uint32_t)c->cus * kWaves;
  const uint32_t rblocks = (uint32_t)std::min<uint64_t>(kRunBlocksMax, std::max<uint64_t>(1, n / 256));
  const size_t own = record_own_bytes(n, rblocks, nw, use_runs || o.reserve_runs);
  void* scratch = nullptr;
  if (int rc = call_scratch(c, s, own + o.tail_bytes, &scratch)) return rc;
  uint8_t* base = (uint8_t*)scratch;
  if (o.tail) *o.tail = base + (own + 15) / 16 * 16;
  uint32_t* maxl = (uint32_t*)base;
  uint64_t* addr = (uint64_t*)(base + 16);
  uint64_t* len = addr + n;
  uint32_t* v = (uint32_t*)(len + n);
  hipError_t e = launch_zero_words(maxl, 4, s);
  if (e == hipSuccess) e = prep(addr, len, maxl);
  if (e == hipSuccess && use_runs) e = launch_zero_words(v, n, s);  // the runs xor their parts in
  if (e != hipSuccess) return fail(HF3FS_CRC_DEVICE_ERROR, "%s prep: %s", o.what, hipGetErrorString(e));
  const ListSource src{addr, len, nullptr, n, ~0u};
  const ByteRuns runs = use_runs ? byte_runs_carve(base + record_head_bytes(n), rblocks, nw, 1) : ByteRuns{};
  if (int rc = run_ranges_list(c, type, src, max_len, v, s, 0, maxl, nullptr, nullptr, use_runs ? &runs : nullptr))
    return rc;
  if ((e = fin(v)) != hipSuccess) return fail(HF3FS_CRC_DEVICE_ERROR, "%s finalize: %s", o.what, hipGetErrorString(e));
  return HF3FS_CRC_OK;
}
int record_type(uint8_t type) {  // the record batches hash with one of the two CRCs
  if (type != kTypeCrc32c && type != kTypeCrc32) return fail(HF3FS_CRC_INVALID_ARG, "type must be CRC32C or CRC32");
  return HF3FS_CRC_OK;
}

int create_host_staged(Context* c, uint8_t type, const void* const* h_bufs, const uint64_t* h_lens,
                       const uint32_t* h_starts, uint32_t* h_out, uint64_t n);  // (below hf3fs_crc_create_host)

}  // namespace

int hf3fs_crc::current_tables(const DeviceTables** out) {
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  *out = c->tables;
  return HF3FS_CRC_OK;
}

// ===========================================================================
extern "C" {

const char* hf3fs_crc_version(void) { return "hf3fs_crc 0.1 gfx950"; }

int hf3fs_crc_init(int device) {
  int prev = 0;
  HIP_OR_FAIL(hipGetDevice(&prev));
  HIP_OR_FAIL(hipSetDevice(device));
  Context* c = nullptr;
  int rc = get_context(&c);
  (void)hipSetDevice(prev);
  return rc;
}

void hf3fs_crc_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  for (auto& c : g_ctx) {
    if (!c) continue;
    (void)hipSetDevice(c->device);
    std::map<StreamKey, PairState> gone;
    {
      std::lock_guard<std::mutex> lk2(c->mu);
      gone.swap(c->pairs);
    }
    for (auto& kv : gone) (void)destroy_pair(kv.second);
    (void)hipFree(c->tables);
    for (uint32_t* slab : c->slabs) (void)hipFree(slab);
    (void)hipFree(c->diag);
    if (c->hint_host) (void)hipHostFree(c->hint_host);
    for (int k = 0; k < 2; ++k) {
      if (c->pinned[k]) (void)hipHostFree(c->pinned[k]);
      if (c->pdesc[k]) (void)hipHostFree(c->pdesc[k]);
      if (c->dstage[k]) (void)hipFree(c->dstage[k]);
      if (c->ddesc[k]) (void)hipFree(c->ddesc[k]);
      if (c->streams[k]) (void)hipStreamDestroy(c->streams[k]);
    }
  }
  g_ctx.clear();
  free_all_captured();
}

int hf3fs_crc_release_stream(void* stream) {
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_OR_FAIL(hipStreamSynchronize(s));
  reap_captured(true);
  std::vector<PairState> gone;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    for (auto it = c->pairs.begin(); it != c->pairs.end();) {
      if (it->first.first != s) {
        ++it;
        continue;
      }
      // the pair's one-shot hint word: cleared (the slot's next call starts with the ticketed
      // apply that counts its pieces), the slot back on the free list with its last pair
      for (const uint32_t slot : it->second.hint)
        if (slot != kNoHint) {
          __atomic_store_n(c->hint_host + slot, 0ull, __ATOMIC_RELEASE);
          if (--c->hint_uses[slot] == 0) c->hint_free.push_back(slot);
        }
      gone.push_back(it->second);
      it = c->pairs.erase(it);
    }
  }
  hipError_t err = hipSuccess;
  for (const PairState& p : gone)
    if (const hipError_t e = destroy_pair(p)) err = e;
  HIP_OR_FAIL(err);
  return HF3FS_CRC_OK;
}

int hf3fs_crc_stream_wait(void* stream, uint32_t poll_us) {
  hipStream_t s = (hipStream_t)stream;
  if (poll_us == 0) {
    HIP_OR_FAIL(hipStreamSynchronize(s));
    return HF3FS_CRC_OK;
  }
  hipError_t e;
  while ((e = hipStreamQuery(s)) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(poll_us));
  HIP_OR_FAIL(e);
  return HF3FS_CRC_OK;
}

int hf3fs_crc_anomalies(int device, hf3fs_crc_anomaly* out, int reset) {
  if (!out) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
  int prev = 0;
  HIP_OR_FAIL(hipGetDevice(&prev));
  HIP_OR_FAIL(hipSetDevice(device));
  Context* c = nullptr;
  int rc = get_context(&c);
  if (!rc) {
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, c->diag, sizeof(*out), hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) {
      const hf3fs_crc_anomaly none{};
      e = hipMemcpy(c->diag, &none, sizeof(none), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) rc = fail(HF3FS_CRC_DEVICE_ERROR, "anomalies: %s", hipGetErrorString(e));
  }
  (void)hipSetDevice(prev);
  return rc;
}

int hf3fs_crc_serialize_batch(uint8_t type, const uint32_t* d_values, uint64_t n, uint8_t* d_out, void* stream) {
  if (!valid_type(type)) return fail(HF3FS_CRC_INVALID_ARG, "unknown checksum type %u", type);
  if (n == 0) return HF3FS_CRC_OK;
  if (!d_values || !d_out) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
  HIP_OR_FAIL(launch_serialize(type, d_values, n, d_out, (hipStream_t)stream));
  return HF3FS_CRC_OK;
}

int hf3fs_crc_finalize_batch(uint32_t* d_values, uint64_t n, void* stream) {
  if (n == 0) return HF3FS_CRC_OK;
  if (!d_values) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
  HIP_OR_FAIL(launch_finalize_values(d_values, n, (hipStream_t)stream));
  return HF3FS_CRC_OK;
}

int hf3fs_crc_create_batch(uint8_t type, const void* const* d_bufs, const uint64_t* d_lens,
                           const uint32_t* d_starts, uint32_t* d_out, uint64_t n, uint64_t max_len, void* stream) {
  if (!valid_type(type)) return fail(HF3FS_CRC_INVALID_ARG, "unknown checksum type %u", type);
  if (n == 0) return HF3FS_CRC_OK;
  if (!d_bufs || !d_lens || !d_out) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
  hipStream_t s = (hipStream_t)stream;
  if (type == kTypeNone) {
    HIP_OR_FAIL(launch_zero_words(d_out, n, s));
    return HF3FS_CRC_OK;
  }
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  ListSource src{reinterpret_cast<const uint64_t*>(d_bufs), d_lens, d_starts, n, ~0u};
  if (options().list_runs.load()) {  // byte runs (option list_runs; the update pre hash's schedule)
    const uint32_t rep = std::max<uint32_t>(1, options().prehash_rep.load());  // runs per wave, as the pre hash
    const uint32_t nw = (uint32_t)c->cus * kWaves * rep;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kRunBlocksMax, std::max<uint64_t>(1, n / 256));
    void* scr = nullptr;
    if (int rc = call_scratch(c, s, byte_runs_bytes(blocks, nw), &scr)) return rc;
    const ByteRuns runs = byte_runs_carve(scr, blocks, nw, rep);
    HIP_OR_FAIL(launch_zero_words(d_out, n, s));
    return run_ranges_list(c, type, src, max_len, d_out, s, 0, nullptr, nullptr, nullptr, &runs);
  }
  return run_ranges_list(c, type, src, max_len, d_out, s);
}

int hf3fs_crc_create_strided(uint8_t type, const void* d_base, uint64_t stride, uint64_t len, uint64_t n,
                             uint32_t start, uint32_t* d_out, void* stream) {
  if (!valid_type(type)) return fail(HF3FS_CRC_INVALID_ARG, "unknown checksum type %u", type);
  if (n == 0) return HF3FS_CRC_OK;
  if ((!d_base && len) || !d_out) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
  hipStream_t s = (hipStream_t)stream;
  if (type == kTypeNone) {
    HIP_OR_FAIL(launch_zero_words(d_out, n, s));
    return HF3FS_CRC_OK;
  }
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  // Equal-length buffers: whole buffers per wave (no shift, no memset) when
  // they divide evenly over the resident waves, else segments; never tickets
  // (uniform tasks balance statically; tickets cost ~1.3% here, A/B in
  // profiles/r01_ab_bulk.json).
  const uint64_t waves = (uint64_t)c->cus * kWaves;
  const bool whole = n % waves == 0 || n >= 8 * waves;
  Plan p = make_plan(c, n, len, whole ? std::max<uint64_t>(len, 1) : 0);
  StridedSource src{(uint64_t)d_base, stride, len, n, start};
  // Otherwise, for a large batch of long buffers: byte runs, every wave one exact share
  // (placed in closed form), instead of segments on a static stride: 1024 x 64 MiB (d4)
  // 10.43 -> 10.25 ms in one process (profiles/r05_d4_runs_probe.log).  More than
  // kRunWindowBytes per wave (batches past 16 GiB, whole buffers included): run_rep runs of
  // <= 4 MiB per wave, so the chip's reads sweep the batch in 16 GiB windows -- one 16 MiB run
  // per wave over a 64 GiB batch read at 6.68 TB/s against 6.95 for four 4 MiB tasks per wave
  // on the same bytes, and 4096 x 16 MiB whole buffers (the same wave -> address map as the
  // 64 MiB runs) at 6.72 (profiles/r06_d4_geometry.log).
  const uint64_t per_wave = n * len / waves;
  const uint32_t rep = per_wave > kRunWindowBytes ? (uint32_t)((per_wave + kRunWindowBytes - 1) / kRunWindowBytes) : 1u;
  const bool big = n < (1ull << 31) && n * len >= kRecordRunsBytes && len >= kRecordRunsMinLen;
  // (whole buffers of <= 4 MiB on their static stride sweep the batch in such windows already)
  const bool window = rep > 1 && !(whole && len <= kRunWindowBytes);
  if (big && ((!whole && p.segs > 1) || window) && (uint64_t)rep * waves < (1ull << 31)) {
    const uint32_t nv = (uint32_t)(rep * waves);  // runs
    void* scr = nullptr;
    if (int rc = call_scratch(c, s, (size_t)(nv + 1) * 12 + 64, &scr)) return rc;
    uint64_t* boff = (uint64_t*)scr;
    uint32_t* bal = (uint32_t*)(boff + nv + 1);
    HIP_OR_FAIL(launch_zero_words(d_out, n, s));  // the parts are xor-ed in
    HIP_OR_FAIL(launch_runs_uniform(n, len, nv, bal, boff, s));
    p.grid = (uint32_t)c->cus;
    p.queue = nullptr;
    p.bal = bal;
    p.boff = boff;
    p.run_rep = rep;
    HIP_OR_FAIL(launch_ranges_strided(type, src, p, d_out, c->tables, s));
    return HF3FS_CRC_OK;
  }
  if (int rc = launch_prepare(c, p, n, d_out, s)) return rc;
  p.queue = nullptr;
  HIP_OR_FAIL(launch_ranges_strided(type, src, p, d_out, c->tables, s));
  return HF3FS_CRC_OK;
}

// The opening of the three verify entry points: validation, the context, and where the
// computed values go (d_computed, else library memory of the call).  *comp stays null for
// n == 0 (the count is zeroed: nothing more to do).
static int verify_begin(uint8_t type, bool args_ok, uint32_t* d_count, uint32_t* d_computed, uint64_t n, hipStream_t s,
                        Context** c, uint32_t** comp) {
  *comp = nullptr;
  if (!valid_type(type)) return fail(HF3FS_CRC_INVALID_ARG, "unknown checksum type %u", type);
  if (!d_count) return fail(HF3FS_CRC_INVALID_ARG, "null mismatch count");
  if (n == 0) {
    HIP_OR_FAIL(launch_zero_words(d_count, 1, s));
    return HF3FS_CRC_OK;
  }
  if (!args_ok) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
  if (int rc = get_context(c)) return rc;
  *comp = d_computed;
  return d_computed ? HF3FS_CRC_OK : call_memory(*c, s, Mem::kVerify, n, comp);
}

static int verify_tail(const uint32_t* computed, const uint32_t* d_expected, uint8_t* d_mismatch, uint32_t* d_count,
                       uint64_t n, hipStream_t s) {
  HIP_OR_FAIL(launch_zero_words(d_count, 1, s));
  HIP_OR_FAIL(launch_compare(computed, d_expected, d_mismatch, d_count, n, s));
  return HF3FS_CRC_OK;
}

int hf3fs_crc_verify_batch(uint8_t type, const void* const* d_bufs, const uint64_t* d_lens,
                           const uint32_t* d_expected, uint8_t* d_mismatch, uint32_t* d_mismatch_count,
                           uint32_t* d_computed, uint64_t n, uint64_t max_len, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  Context* c = nullptr;
  uint32_t* comp = nullptr;
  if (const int rc = verify_begin(type, d_expected && d_mismatch, d_mismatch_count, d_computed, n, s, &c, &comp);
      rc || !comp)
    return rc;
  if (int rc = hf3fs_crc_create_batch(type, d_bufs, d_lens, nullptr, comp, n, max_len, stream)) return rc;
  return verify_tail(comp, d_expected, d_mismatch, d_mismatch_count, n, s);
}

int hf3fs_crc_verify_strided(uint8_t type, const void* d_base, uint64_t stride, uint64_t len, uint64_t n,
                             const uint32_t* d_expected, uint8_t* d_mismatch, uint32_t* d_mismatch_count,
                             uint32_t* d_computed, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  Context* c = nullptr;
  uint32_t* comp = nullptr;
  if (const int rc = verify_begin(type, d_expected && d_mismatch, d_mismatch_count, d_computed, n, s, &c, &comp);
      rc || !comp)
    return rc;
  if (int rc = hf3fs_crc_create_strided(type, d_base, stride, len, n, ~0u, comp, stream)) return rc;
  return verify_tail(comp, d_expected, d_mismatch, d_mismatch_count, n, s);
}

int hf3fs_crc_verify_blocks(uint8_t type, const void* d_arena, const uint64_t* d_offsets, const uint32_t* d_lens,
                            const uint32_t* d_expected, uint8_t* d_mismatch, uint32_t* d_mismatch_count,
                            uint32_t* d_computed, uint64_t n, uint32_t max_len, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  Context* c = nullptr;
  uint32_t* comp = nullptr;
  const bool args_ok = d_arena && d_offsets && d_lens && d_expected && d_mismatch;
  if (const int rc = verify_begin(type, args_ok, d_mismatch_count, d_computed, n, s, &c, &comp); rc || !comp) return rc;
  if (type == kTypeNone) {
    HIP_OR_FAIL(launch_zero_words(comp, n, s));
  } else {
    Plan p = make_plan(c, n, max_len);
    if (int rc = launch_prepare(c, p, n, comp, s)) return rc;
    ArenaSource src{(uint64_t)d_arena, d_offsets, d_lens, n};
    if (int rc = plan_balance(c, p, src, n, max_len, s)) return rc;
    HIP_OR_FAIL(launch_ranges_arena(type, src, p, comp, c->tables, s));
  }
  return verify_tail(comp, d_expected, d_mismatch, d_mismatch_count, n, s);
}

int hf3fs_crc_combine_batch(uint8_t type, uint32_t* d_acc, const uint32_t* d_crc2, const uint64_t* d_len2,
                            uint64_t n, void* stream) {
  if (!valid_type(type)) return fail(HF3FS_CRC_INVALID_ARG, "unknown checksum type %u", type);
  if (n == 0 || type == kTypeNone) return HF3FS_CRC_OK;
  if (!d_acc || !d_crc2 || !d_len2) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  HIP_OR_FAIL(launch_combine(type, d_acc, d_crc2, d_len2, n, c->tables, (hipStream_t)stream));
  return HF3FS_CRC_OK;
}

int hf3fs_crc_fill_synth(void* d_dst, uint64_t stride, uint64_t chunk_len, uint64_t n_chunks, uint64_t seed,
                         uint64_t first_chunk_id, void* stream) {
  if (!d_dst && n_chunks && chunk_len) return fail(HF3FS_CRC_INVALID_ARG, "null destination");
  if (((uint64_t)d_dst | stride) & 7) return fail(HF3FS_CRC_INVALID_ARG, "fill_synth needs 8-byte alignment");
  HIP_OR_FAIL(
      launch_fill_synth((uint8_t*)d_dst, stride, chunk_len, n_chunks, seed, first_chunk_id, (hipStream_t)stream));
  return HF3FS_CRC_OK;
}

// Pipeline per mode: DELTA runs the three streaming passes (pre hash, apply:
// the payload is read twice); REFERENCE the fused per-IO kernel (its prefix/suffix pass follows
// either way).  Option update_pipeline = unfused | fused forces one (A/B and the parity tests,
// which run both on every mode).  Apply pieces (three-pass pipeline): up to apply_pieces (8) per
// range, at least apply_min_kib (64 KiB) each (the tests cut finer).
void update_pipeline(int mode, bool* unfused, uint32_t* pieces, uint32_t* piece_min) {
  const Options& o = options();
  const int forced = o.update_pipeline.load();
  *unfused = forced < 0 ? mode == HF3FS_UPDATE_MODE_DELTA : forced == 0;
  *pieces = *unfused ? o.apply_pieces.load() : 0;  // only the three-pass pipeline has an apply pass
  *piece_min = o.apply_min_kib.load() << 10;
}

size_t hf3fs_crc_update_scratch_bytes(uint64_t n, int mode) {
  Context* c = nullptr;
  if (get_context(&c)) return 0;
  bool unfused = false;
  uint32_t pieces = 0, piece_min = 0;
  update_pipeline(mode, &unfused, &pieces, &piece_min);
  return update_scratch_bytes(n, update_record_cap(n, 2, pieces), (uint32_t)c->cus * kWaves, 0);
}

// The plan of one update call: what the options make of it in `mode` -- the pipeline, the
// ticketed apply's pieces, the waves of its hash launches (pre-hash byte runs: prehash_rep runs
// per wave, Plan::run_rep) -- and its apply: one-shot (a workgroup per piece of
// 2^shift destination bytes) on a grid sized from the pair's previous call, or the ticketed tasks
// when no call has counted pieces yet (option apply_grid) or the piece table would be too large.
// The entry point is also the index of the pair's hint word: what one entry point counts never
// sizes the grid of another on the same pair.
enum UpdateEntry { kEntryBatch = 0, kEntryOrdered = 1, kEntryCow = 2, kEntryEngine = 3 };  // ordered, engine: round 0
struct UpdatePlan {
  bool unfused = false;
  uint32_t pieces = 0, piece_min = 0, rep = 1, nw = 0;
  uint32_t rpi = 2;               // range records per IO: kPlanRanges for a call with destinations
  const uint64_t* dst = nullptr;  // its destinations (device, may be null)
  uint64_t records = 0;           // entries of the record array (update_record_cap)
  bool one_shot = false;
  uint32_t shift = 13;
  uint32_t grid = 0;
  uint64_t cap = 0;       // piece-table entries a one-shot apply of this shape takes, 0: always ticketed
  uint64_t ptab_cap = 0;  // those of this call (0: it is ticketed)
  uint64_t* hint = nullptr;  // device view of the pair's pinned hint word
};
uint32_t apply_piece_shift() {
  const uint32_t kib = options().apply_piece_kib.load();
  return kib <= 4 ? 12 : kib <= 8 ? 13 : 14;
}
// The one-shot grid for n IOs from a hint word (pieces << 32 | n of the pair's previous call):
// that call's pieces per IO with 3 % + 64 workgroups of headroom, at most cap; 0 = no call yet.
static uint32_t hinted_grid(uint64_t h, uint64_t n, uint64_t cap) {
  const uint64_t prev_pieces = h >> 32, prev_n = h & 0xffffffffull;
  if (!prev_n) return 0;
  const uint64_t want = prev_pieces * n / prev_n;
  return (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(1, want + want / 32 + 64));
}
// s null: the shape only (what the *_scratch_bytes functions need), no hint is read.
// hf3fs_crc_update_cow_batch differs in this: it pins the three-pass pipeline with the one-shot
// apply in both modes -- its range records (payload, gap, old prefix, old suffix: 4 per IO) are
// the one-shot apply's, and that kernel loops when the grid is short of the piece count, so no
// call needs the ticketed tasks and the pair's first call takes their grid instead; its piece
// table has its own bound, and a table over 1 GiB rejects the call where the others fall back
// to tickets.
static int plan_update(Context* c, UpdateEntry entry, uint64_t n, uint32_t max_len, int mode, const uint64_t* d_dst,
                       const hipStream_t* s, UpdatePlan* p) {
  const bool cow = entry == kEntryCow || entry == kEntryEngine;  // (every round of update_engine is a COW batch)
  const int apply_grid = options().apply_grid.load();
  update_pipeline(mode, &p->unfused, &p->pieces, &p->piece_min);
  if (cow) {
    p->unfused = true;
    p->pieces = 0;  // no ticketed apply
  }
  p->rpi = cow ? kPlanRanges : 2;
  p->dst = d_dst;
  p->records = update_record_cap(n, p->rpi, p->pieces);
  p->rep = std::max<uint32_t>(1, options().prehash_rep.load());
  p->nw = (uint32_t)c->cus * kWaves * p->rep;
  if (!p->unfused) return HF3FS_CRC_OK;
  p->shift = apply_piece_shift();
  p->grid = (uint32_t)c->cus * 8;  // the ticketed apply's
  uint64_t cap = cow ? update_cow_piece_cap(n, max_len, p->shift) : update_piece_cap(n, max_len, p->shift);
  if (cap >= (1ull << 31) || cap * 4 > (1ull << 30) || (cow && n >= (1ull << 28))) cap = 0;
  if (cow && !cap)
    return fail(HF3FS_CRC_INVALID_ARG, "piece table of %llu IOs of %u bytes exceeds 1 GiB: split the batch",
                (unsigned long long)n, max_len);
  if (!cow && apply_grid == 0) cap = 0;
  p->cap = cap;
  if (cow) p->ptab_cap = cap;
  if (!s) return HF3FS_CRC_OK;
  uint64_t* host = nullptr;
  if (int rc = c->hint_word(*s, entry, &host, &p->hint)) return rc;
  if (!cap) return HF3FS_CRC_OK;  // tickets
  const uint32_t hinted = hinted_grid(__atomic_load_n(host, __ATOMIC_ACQUIRE), n, cap);
  if (apply_grid == 2) {  // test: a small grid, every workgroup loops over several pieces
    p->grid = (uint32_t)c->cus;
  } else if (hinted) {
    p->grid = hinted;
  } else if (!cow && apply_grid < 0) {
    return HF3FS_CRC_OK;  // auto, first call of the pair: tickets (they count the pieces)
  }
  p->one_shot = true;
  p->ptab_cap = cap;
  return HF3FS_CRC_OK;
}
static int update_args(uint8_t type, int mode) {
  if (!valid_type(type)) return fail(HF3FS_CRC_INVALID_ARG, "unknown checksum type %u", type);
  if (mode != HF3FS_UPDATE_MODE_REFERENCE && mode != HF3FS_UPDATE_MODE_DELTA)
    return fail(HF3FS_CRC_INVALID_ARG, "unknown update mode %d", mode);
  return HF3FS_CRC_OK;
}

// The side stream of a one-shot update call from its fork on.  Whichever way the call
// leaves, side.join is recorded on the side stream (once) and s waits for it: a side stream
// left forked would fail the end of a capture and stay in the invalidated capture.
struct SideJoin {
  Side side;
  hipStream_t s = nullptr;
  bool forked = false, recorded = false;
  hipError_t record() { return recorded = true, hipEventRecord(side.join, side.side); }
  hipError_t wait() {
    forked = false;
    const hipError_t e = recorded ? hipSuccess : record();
    const hipError_t w = hipStreamWaitEvent(s, side.join, 0);
    return e != hipSuccess ? e : w;
  }
  ~SideJoin() { if (forked) (void)wait(); }
};

static int update_run(Context* c, uint8_t type, hf3fs_crc_update_io* d_ios, uint64_t n, uint32_t max_len, int mode,
                      const UpdatePlan& p, void* base, hipStream_t s);

int hf3fs_crc_update_batch(uint8_t type, hf3fs_crc_update_io* d_ios, uint64_t n, uint32_t max_len, int mode,
                           void* stream) {
  if (int rc = update_args(type, mode)) return rc;
  if (n == 0) return HF3FS_CRC_OK;
  if (!d_ios) return fail(HF3FS_CRC_INVALID_ARG, "null ios");
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  UpdatePlan p;
  if (int rc = plan_update(c, kEntryBatch, n, max_len, mode, nullptr, &s, &p)) return rc;
  void* base = nullptr;
  if (int rc = call_scratch(c, s, update_scratch_bytes(n, p.records, p.nw, p.ptab_cap), &base)) return rc;
  return update_run(c, type, d_ios, n, max_len, mode, p, base, s);
}

// One pass of the update pipeline over n IOs on DISTINCT chunks, on scratch the caller got for it
// (update_scratch_bytes(n, p.records, p.nw, p.ptab_cap) at base): hf3fs_crc_update_batch,
// hf3fs_crc_update_cow_batch, and every round of hf3fs_crc_update_ordered.
static int update_run(Context* c, uint8_t type, hf3fs_crc_update_io* d_ios, uint64_t n, uint32_t max_len, int mode,
                      const UpdatePlan& p, void* base, hipStream_t s) {
  const uint8_t ktype = type == kTypeNone ? kTypeCrc32c : type;
  const bool unfused = p.unfused;
  // Pre-hash task size: 512 KiB segments of the payload / old-byte jobs (A/B on d3 DELTA:
  // 1.766-1.772 ms per batch vs 1.788-1.797 at 256 KiB, 1.85 at 1 MiB; gpurun_out r03 seg sweep).
  constexpr uint64_t kPreSeg = 512 << 10;
  UpdateScratch sc;
  update_scratch_carve(base, n, p.records, p.pieces, p.piece_min, p.nw, p.ptab_cap, &sc);
  sc.piece_shift = p.shift;
  sc.one_shot = p.one_shot ? 1u : 0u;
  sc.diag = c->diag;
  sc.runs_used = unfused;
  sc.fault_io = options().fault_io.load();
  // Pre hash as byte runs: every wave the same share of payload + old bytes, ranges split
  // anywhere (A/B vs 512 KiB tickets: 1.721-1.732 vs 1.726-1.738 ms per d3 DELTA batch).
  const bool prep_runs = 2 * n <= kPrepRunJobs;  // prep's runs workgroup places them (else launch_balance)
  const ByteRuns runs{sc.run_partial, sc.run_bal, sc.run_boff, sc.run_blocks, prep_runs, p.rep};
  // ONE zeroing launch: the job maxima, the task count and every ticket counter of this
  // call live in sc.ctl; prep zeroes the per-IO hash outputs itself.
  HIP_OR_FAIL(launch_zero_words(sc.ctl, kCtlWords, s));
  SideJoin join;
  if (!unfused) {  // one kernel: prep + payload verify + write (+ delta old-byte hash)
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n, (uint64_t)c->cus);
    const int nt = (int)options().apply_nt.load();
    HIP_OR_FAIL(launch_update_fused(d_ios, n, max_len, type, mode, sc, c->tables, grid, nt, s));
  } else {  // three passes: prep, the pre jobs through k_crc_ranges, apply (+ finalize of most IOs)
    HIP_OR_FAIL(launch_update_prep(d_ios, p.dst, n, max_len, type, mode, sc, p.rpi, prep_runs, s));
    ListSource pre{sc.pre_addr, sc.pre_len, sc.pre_start, 2 * n, 0u};
    if (int rc = run_ranges_list(c, ktype, pre, max_len, sc.pre_out, s, kPreSeg, sc.ctl + kCtlPreMax, nullptr,
                                 sc.ctl + kCtlQueuePre, &runs))
      return rc;
    if (p.one_shot) {  // every verdict and every IO without a post job, beside the apply
      if (int rc = c->side_of(s, &join.side)) return rc;
      join.s = s;
      HIP_OR_FAIL(hipEventRecord(join.side.fork, s));
      join.forked = true;  // from here on every return joins the side stream again
      HIP_OR_FAIL(hipStreamWaitEvent(join.side.side, join.side.fork, 0));
      HIP_OR_FAIL(launch_update_finalize(d_ios, n, type, mode, sc, c->tables, max_len, 1, false, join.side.side));
      HIP_OR_FAIL(join.record());
    }
    HIP_OR_FAIL(launch_update_apply(d_ios, n, max_len, type, mode, sc, c->tables, p.rpi, true, p.grid,
                                    (int)options().apply_nt.load(), p.ptab_cap, p.hint, s));
  }
  ListSource post{sc.post_addr, sc.post_len, sc.post_start, 2 * n, 0u};
  if (int rc = run_ranges_list(c, ktype, post, max_len, sc.post_out, s, 256 << 10, sc.ctl + kCtlPostMax, nullptr,
                               sc.ctl + kCtlQueuePost))
    return rc;
  // the last launch also re-checks every payload it reports as mismatched (option audit)
  // the three-pass pipeline's verdicts came from the apply (ticketed) or the side stream
  // (one-shot): only the post-job IOs and the audit are left
  if (p.one_shot) HIP_OR_FAIL(join.wait());
  HIP_OR_FAIL(launch_update_finalize(d_ios, n, type, mode, sc, c->tables, max_len, unfused ? 2 : 0,
                                     options().audit.load() != 0, s));
  if (options().debug.load()) {  // diagnostics: job maxima and the first pre/post hashes
    uint32_t mx[2] = {0, 0}, pre[4] = {0, 0, 0, 0}, post[4] = {0, 0, 0, 0};
    uint64_t plen[4] = {0, 0, 0, 0};
    const size_t k = std::min<uint64_t>(4, 2 * n);
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(mx, sc.ctl, 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(pre, sc.pre_out, 4 * k, hipMemcpyDeviceToHost);
    (void)hipMemcpy(post, sc.post_out, 4 * k, hipMemcpyDeviceToHost);
    (void)hipMemcpy(plen, sc.pre_len, 8 * k, hipMemcpyDeviceToHost);
    fprintf(stderr, "[hf3fs_crc debug] update n=%llu mode=%d max=%u/%u pre=%08x,%08x len=%llu,%llu post=%08x,%08x\n",
            (unsigned long long)n, mode, mx[0], mx[1], pre[0], pre[1], (unsigned long long)plen[0],
            (unsigned long long)plen[1], post[0], post[1]);
  }
  return HF3FS_CRC_OK;
}

// The one scratch request of an ordered call: the pipeline's part first -- with the piece table
// of a one-shot apply whenever the options allow one, whether or not this call's first round
// takes it (the pair's hint decides that from call to call, and no later call may need more than
// the first of a shape got) -- and the planner's arrays behind it.
static size_t ordered_pipeline_bytes(const UpdatePlan& p, uint64_t n) {
  return (update_scratch_bytes(n, p.records, p.nw, p.cap) + 63) & ~size_t(63);
}
static int ordered_args(uint8_t type, int mode, uint32_t max_rounds) {
  if (int rc = update_args(type, mode)) return rc;
  if (max_rounds < 1 || max_rounds > 64)
    return fail(HF3FS_CRC_INVALID_ARG, "max_rounds %u is not in 1..64", max_rounds);
  return HF3FS_CRC_OK;
}
constexpr uint64_t kOrderedMaxIos = 1ull << 30;  // 32-bit IO indices, a table of 2 n slots
// The gate of the round calls (ordered, versioned, engine) behind their argument check: an empty
// queue zeroes the call's info words and leaves *c null.
static int rounds_gate(const void* d_ios, uint64_t n, uint32_t* d_info, uint32_t info_words, hipStream_t s, Context** c) {
  *c = nullptr;
  if (n == 0) {
    if (d_info) HIP_OR_FAIL(launch_zero_words(d_info, info_words, s));
    return HF3FS_CRC_OK;
  }
  if (!d_ios) return fail(HF3FS_CRC_INVALID_ARG, "null ios");
  if (n > kOrderedMaxIos) return fail(HF3FS_CRC_INVALID_ARG, "too many IOs (%llu)", (unsigned long long)n);
  return get_context(c);
}
// Round 0 is planned like an update_batch of the n records (with every chunk distinct it IS that
// call), on a hint word of its own: what an ordered call counts never sizes the grid of a plain
// update_batch on the same pair.  Later rounds shrink fast and are padded to n records, so a
// pieces-per-IO figure says nothing about them: they take the ticketed apply, which needs none.
static UpdatePlan later_rounds(UpdatePlan p, const Context* c) {
  p.one_shot = false;
  p.ptab_cap = 0;
  p.hint = nullptr;
  p.grid = (uint32_t)c->cus * 8;
  return p;
}
// The planner, then rounds 0 .. max_rounds - 1 -- the entry point's step(r), then one pass of the
// pipeline over the round's records (os.round) on the scratch at base -- and step(max_rounds).
extern "C++" template <class Step>
int run_rounds(Context* c, uint8_t type, hf3fs_crc_update_io* d_ios, uint64_t n, uint32_t max_len, int mode,
               uint32_t max_rounds, const UpdatePlan& first, const UpdatePlan& later, const OrderScratch& os, void* base,
               hipStream_t s, Step step) {
  HIP_OR_FAIL(launch_order_plan(d_ios, n, max_rounds, os, s));
  for (uint32_t r = 0; r < max_rounds; ++r) {
    HIP_OR_FAIL(step(r));
    if (int rc = update_run(c, type, os.round, n, max_len, mode, r ? later : first, base, s)) return rc;
  }
  HIP_OR_FAIL(step(max_rounds));
  return HF3FS_CRC_OK;
}
// The payloads of the jobs a versioned or engine call refused behind the verify's place (4080 goes
// first).  Every other entry of the list is empty; with no such job the pass finds a length bound of 0.
static int hash_refused(Context* c, uint8_t type, const VersionScratch& v, uint64_t n, uint32_t max_len,
                        const OrderScratch& os, hipStream_t s) {
  const ListSource late{v.vaddr, v.vlen, nullptr, n, ~0u};
  return run_ranges_list(c, type == kTypeNone ? kTypeCrc32c : type, late, max_len, v.vout, s, 0, os.ctl + kOrdVerMaxLen,
                         nullptr, os.ctl + kOrdVerQueue);
}

size_t hf3fs_crc_update_ordered_scratch_bytes(uint64_t n, uint32_t max_len, int mode, uint32_t max_rounds) {
  if (ordered_args(kTypeCrc32c, mode, max_rounds) || n == 0 || n > kOrderedMaxIos) return 0;
  Context* c = nullptr;
  if (get_context(&c)) return 0;
  UpdatePlan p;
  if (plan_update(c, kEntryOrdered, n, max_len, mode, nullptr, nullptr, &p)) return 0;
  return ordered_pipeline_bytes(p, n) + order_scratch_bytes(n);
}

int hf3fs_crc_update_ordered(uint8_t type, hf3fs_crc_update_io* d_ios, uint64_t n, uint32_t max_len, int mode,
                             uint32_t max_rounds, uint32_t* d_info, void* stream) {
  if (int rc = ordered_args(type, mode, max_rounds)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Context* c = nullptr;
  if (const int rc = rounds_gate(d_ios, n, d_info, 2, s, &c); rc || !c) return rc;
  UpdatePlan first;
  if (int rc = plan_update(c, kEntryOrdered, n, max_len, mode, nullptr, &s, &first)) return rc;
  const size_t pipe_bytes = ordered_pipeline_bytes(first, n);
  void* base = nullptr;
  if (int rc = call_scratch(c, s, pipe_bytes + order_scratch_bytes(n), &base)) return rc;
  OrderScratch os;
  order_scratch_carve((uint8_t*)base + pipe_bytes, n, &os);
  const auto step = [&](uint32_t r) {
    return launch_order_step(d_ios, n, r, max_rounds, os, r < max_rounds ? nullptr : d_info, s);
  };
  return run_rounds(c, type, d_ios, n, max_len, mode, max_rounds, first, later_rounds(first, c), os, base, s, step);
}

// update_ordered with the version ladders (version_kernels.h).  Round 0 plans on the ordered
// call's hint word: for a queue the ladders admit whole it IS that call's round 0.
static size_t versioned_order_bytes(uint64_t n) { return (order_scratch_bytes(n) + 63) & ~size_t(63); }

size_t hf3fs_crc_update_versioned_scratch_bytes(uint64_t n, uint32_t max_len, int mode, uint32_t max_rounds) {
  const size_t ordered = hf3fs_crc_update_ordered_scratch_bytes(n, max_len, mode, max_rounds);
  if (!ordered) return 0;
  return ordered - order_scratch_bytes(n) + versioned_order_bytes(n) + version_scratch_bytes(n);
}

int hf3fs_crc_update_versioned(uint8_t type, hf3fs_crc_update_io* d_ios, hf3fs_crc_update_ver* d_ver, uint64_t n,
                               uint32_t max_len, int mode, uint32_t max_rounds, uint32_t* d_info, void* stream) {
  if (!d_ver) return hf3fs_crc_update_ordered(type, d_ios, n, max_len, mode, max_rounds, d_info, stream);
  if (int rc = ordered_args(type, mode, max_rounds)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Context* c = nullptr;
  if (const int rc = rounds_gate(d_ios, n, d_info, HF3FS_VER_INFO_WORDS, s, &c); rc || !c) return rc;
  UpdatePlan first;
  if (int rc = plan_update(c, kEntryOrdered, n, max_len, mode, nullptr, &s, &first)) return rc;
  const size_t pipe_bytes = ordered_pipeline_bytes(first, n), order_bytes = versioned_order_bytes(n);
  void* base = nullptr;
  if (int rc = call_scratch(c, s, pipe_bytes + order_bytes + version_scratch_bytes(n), &base)) return rc;
  OrderScratch os;
  VersionScratch vs;
  order_scratch_carve((uint8_t*)base + pipe_bytes, n, &os);
  version_scratch_carve((uint8_t*)base + pipe_bytes + order_bytes, n, &vs);
  const auto step = [&](uint32_t r) {
    return launch_version_step(d_ios, d_ver, n, r, max_rounds, max_len, type, mode, os, vs, d_info, s);
  };
  if (int rc = run_rounds(c, type, d_ios, n, max_len, mode, max_rounds, first, later_rounds(first, c), os, base, s, step))
    return rc;
  if (int rc = hash_refused(c, type, vs, n, max_len, os, s)) return rc;  // (ChunkReplica.cc:193-207)
  HIP_OR_FAIL(launch_version_settle(d_ios, n, max_rounds, os, vs, d_info, s));
  return HF3FS_CRC_OK;
}

// The chunk engine's queue (engine_kernels.h): the ordered call's planner, the engine's state
// machine between rounds, and every round a copy-on-write batch over the step's destination array.
// Every round takes the one-shot apply -- the copy-on-write pipeline has no ticketed form, and its
// kernel loops when the grid is short; round 0 plans on the call's own hint word and leaves its
// piece count there, the later rounds (which shrink fast) run on round 0's grid and leave none.
static int engine_args(uint8_t type, int mode, uint32_t max_rounds) {
  if (int rc = ordered_args(type, mode, max_rounds)) return rc;
  if (type != kTypeCrc32c)
    return fail(HF3FS_CRC_INVALID_ARG, "the chunk engine's checksum type is CRC32C, not %u", type);
  return HF3FS_CRC_OK;
}
static size_t engine_pipeline_bytes(const UpdatePlan& p, uint64_t n) {
  return (update_scratch_bytes(n, p.records, p.nw, p.ptab_cap) + 63) & ~size_t(63);
}

size_t hf3fs_crc_update_engine_scratch_bytes(uint64_t n, uint32_t max_len, int mode, uint32_t max_rounds) {
  if (engine_args(kTypeCrc32c, mode, max_rounds) || n == 0 || n > kOrderedMaxIos) return 0;
  Context* c = nullptr;
  if (get_context(&c)) return 0;
  UpdatePlan p;
  if (plan_update(c, kEntryEngine, n, max_len, mode, nullptr, nullptr, &p)) return 0;
  return engine_pipeline_bytes(p, n) + versioned_order_bytes(n) + engine_scratch_bytes(n);
}

int hf3fs_crc_update_engine(uint8_t type, hf3fs_crc_update_io* d_ios, hf3fs_crc_engine_job* d_jobs, uint64_t n,
                            uint32_t max_len, int mode, uint32_t max_rounds, uint32_t* d_info, void* stream) {
  if (int rc = engine_args(type, mode, max_rounds)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (n && d_ios && !d_jobs) return fail(HF3FS_CRC_INVALID_ARG, "null jobs");
  Context* c = nullptr;
  if (const int rc = rounds_gate(d_ios, n, d_info, HF3FS_ENGINE_INFO_WORDS, s, &c); rc || !c) return rc;
  const size_t order_bytes = versioned_order_bytes(n);
  UpdatePlan first;
  if (int rc = plan_update(c, kEntryEngine, n, max_len, mode, nullptr, &s, &first)) return rc;
  const size_t pipe_bytes = engine_pipeline_bytes(first, n);
  void* base = nullptr;
  if (int rc = call_scratch(c, s, pipe_bytes + order_bytes + engine_scratch_bytes(n), &base)) return rc;
  OrderScratch os;
  EngineScratch es;
  order_scratch_carve((uint8_t*)base + pipe_bytes, n, &os);
  engine_scratch_carve((uint8_t*)base + pipe_bytes + order_bytes, n, &es);
  first.dst = es.rdst;
  UpdatePlan later = first;
  later.hint = nullptr;
  const auto step = [&](uint32_t r) {
    return launch_engine_step(d_ios, d_jobs, n, r, max_rounds, max_len, mode, os, es, d_info, s);
  };
  if (int rc = run_rounds(c, type, d_ios, n, max_len, mode, max_rounds, first, later, os, base, s, step)) return rc;
  if (int rc = hash_refused(c, type, es.v, n, max_len, os, s)) return rc;  // (engine.rs:297-311)
  HIP_OR_FAIL(launch_engine_settle(d_ios, d_jobs, n, max_rounds, os, es, d_info, s));
  return HF3FS_CRC_OK;
}

size_t hf3fs_crc_update_cow_scratch_bytes(uint64_t n, uint32_t max_len, int mode) {
  if (update_args(kTypeCrc32c, mode) || n == 0) return 0;
  Context* c = nullptr;
  if (get_context(&c)) return 0;
  UpdatePlan p;
  if (plan_update(c, kEntryCow, n, max_len, mode, nullptr, nullptr, &p)) return 0;
  return update_scratch_bytes(n, p.records, p.nw, p.ptab_cap);
}

int hf3fs_crc_update_cow_batch(uint8_t type, hf3fs_crc_update_io* d_ios, const uint64_t* d_dst, uint64_t n,
                               uint32_t max_len, int mode, void* stream) {
  if (int rc = update_args(type, mode)) return rc;
  if (n == 0) return HF3FS_CRC_OK;
  if (!d_ios) return fail(HF3FS_CRC_INVALID_ARG, "null ios");
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  UpdatePlan p;
  if (int rc = plan_update(c, kEntryCow, n, max_len, mode, d_dst, &s, &p)) return rc;
  void* base = nullptr;
  if (int rc = call_scratch(c, s, update_scratch_bytes(n, p.records, p.nw, p.ptab_cap), &base)) return rc;
  return update_run(c, type, d_ios, n, max_len, mode, p, base, s);
}

int hf3fs_crc_pair_scratch_stats(void* stream, uint64_t* call_bytes, uint64_t* allocations) {
  if (call_bytes) {
    Context* c = nullptr;
    if (int rc = get_context(&c)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    const auto it = c->pairs.find(stream_key((hipStream_t)stream));
    *call_bytes = it == c->pairs.end() ? 0 : (uint64_t)it->second.call.words * 4;
  }
  if (allocations) *allocations = g_pair_allocs.load(std::memory_order_relaxed);
  return HF3FS_CRC_OK;
}

int hf3fs_crc_read_result_batch(uint8_t type, hf3fs_crc_read_io* d_ios, uint64_t n, uint32_t max_len,
                                void* stream) {
  if (int rc = record_type(type)) return rc;
  if (n == 0) return HF3FS_CRC_OK;
  if (!d_ios) return fail(HF3FS_CRC_INVALID_ARG, "null ios");
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  return run_record_jobs(
      c, type, n, max_len, s,
      [&](uint64_t* addr, uint64_t* len, uint32_t* maxl) {
        return launch_read_prep(d_ios, n, type, max_len, addr, len, maxl, s);
      },
      [&](const uint32_t* v) { return launch_read_finalize(d_ios, n, v, s); }, {.what = "read"});
}

size_t hf3fs_crc_client_read_scratch_bytes(uint64_t n_ios, uint64_t n_parents) {
  if (n_ios > kClientMaxCount || n_parents > kClientMaxCount) return 0;
  // run_record_jobs' carve without byte runs, as the pair's buffer is sized by a first call (a
  // captured call's own memory is the exact bytes); the parents take no scratch.
  return roomy_words((record_own_bytes(n_ios, 0, 0, false) + 3) / 4) * 4;
}

int hf3fs_crc_client_read_batch(uint8_t type, hf3fs_crc_client_read_io* d_ios, uint64_t n_ios,
                                const uint64_t* d_parent_off, uint64_t n_parents, uint64_t max_children,
                                uint32_t max_len, uint32_t flags, hf3fs_crc_client_read_result* d_parents,
                                hf3fs_crc_block_digest* d_blocks, uint32_t* d_info, void* stream) {
  if (int rc = record_type(type)) return rc;
  if (flags & ~(uint32_t)HF3FS_CLIENT_READ_VERIFY) return fail(HF3FS_CRC_INVALID_ARG, "unknown flags %#x", flags);
  if (!d_ios && n_ios) return fail(HF3FS_CRC_INVALID_ARG, "null ios");
  if (!d_info) return fail(HF3FS_CRC_INVALID_ARG, "null info");
  if (!d_parent_off && n_parents != n_ios)
    return fail(HF3FS_CRC_INVALID_ARG, "null parent offsets need n_parents == n_ios (%llu != %llu)",
                (unsigned long long)n_parents, (unsigned long long)n_ios);
  const bool verify = (flags & HF3FS_CLIENT_READ_VERIFY) != 0;
  if (!d_parents && !d_blocks && !verify) return fail(HF3FS_CRC_INVALID_ARG, "nothing to do: no output and no VERIFY");
  if (n_ios > kClientMaxCount || n_parents > kClientMaxCount)
    return fail(HF3FS_CRC_INVALID_ARG, "too many IOs or parents (%llu, %llu)", (unsigned long long)n_ios,
                (unsigned long long)n_parents);
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_OR_FAIL(launch_zero_words(d_info, HF3FS_CLIENT_READ_INFO_WORDS, s));  // the merge adds into it
  if (n_ios == 0 && n_parents == 0) return HF3FS_CRC_OK;
  const bool wave = max_children > kClientLaneMaxChildren;
  const auto merge = [&](const uint32_t* v) {
    return launch_client_read_merge(d_ios, n_ios, d_parent_off, n_parents, type, max_len, v != nullptr, wave, v,
                                    d_parents, d_blocks, d_info, c->tables, s);
  };
  if (!verify || n_ios == 0) {  // no child is compared: no byte is read, no scratch taken
    HIP_OR_FAIL(merge(nullptr));
    return HF3FS_CRC_OK;
  }
  return run_record_jobs(
      c, type, n_ios, max_len, s,
      [&](uint64_t* addr, uint64_t* len, uint32_t* maxl) {
        return launch_client_read_prep(d_ios, n_ios, type, max_len, addr, len, maxl, s);
      },
      merge, {.what = "client read"});
}

// Prepare takes run_record_jobs' carve with the byte-run tables reserved, complete
// client_write_scratch_bytes; a caller sizes for the larger.  The files take no scratch.
size_t hf3fs_crc_client_write_scratch_bytes(uint64_t n, uint64_t n_files) {
  if (n > kClientWriteMaxCount || n_files > kClientWriteMaxCount) return 0;
  const size_t prepare = record_own_bytes(n, kRunBlocksMax, kSizingWaves, true);
  return roomy_words((std::max(prepare, client_write_scratch_bytes(n) + 16) + 3) / 4) * 4;
}

int hf3fs_crc_client_write_prepare(uint8_t type, hf3fs_crc_client_write_io* d_ios, uint64_t n, uint32_t max_len,
                                   uint32_t max_inline_bytes, uint32_t flags, hf3fs_crc_update_io* d_updates,
                                   uint32_t* d_info, void* stream) {
  if (int rc = record_type(type)) return rc;
  if (flags & ~(uint32_t)HF3FS_CLIENT_WRITE_VERIFY) return fail(HF3FS_CRC_INVALID_ARG, "unknown flags %#x", flags);
  if (!d_ios && n) return fail(HF3FS_CRC_INVALID_ARG, "null ios");
  if (!d_info) return fail(HF3FS_CRC_INVALID_ARG, "null info");
  if (n > kClientWriteMaxCount) return fail(HF3FS_CRC_INVALID_ARG, "too many IOs (%llu)", (unsigned long long)n);
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_OR_FAIL(launch_zero_words(d_info, HF3FS_CLIENT_WRITE_INFO_WORDS, s));  // the finish adds into it
  if (n == 0) return HF3FS_CRC_OK;
  const bool verify = (flags & HF3FS_CLIENT_WRITE_VERIFY) != 0;
  const uint32_t* poison = nullptr;  // the prep's ctl + 1
  const auto finish = [&](const uint32_t* v) {
    return launch_client_write_prepare_finish(d_ios, n, type, max_len, max_inline_bytes, verify, v, poison, d_updates,
                                              d_info, s);
  };
  if (!verify) {  // no payload is hashed: the checks alone, behind the poison word
    void* scratch = nullptr;
    if (int rc = call_scratch(c, s, 16, &scratch)) return rc;
    uint32_t* ctl = (uint32_t*)scratch;
    poison = ctl + 1;
    HIP_OR_FAIL(launch_zero_words(ctl, 4, s));
    HIP_OR_FAIL(launch_client_write_prep(d_ios, n, max_len, false, nullptr, nullptr, ctl, s));
    HIP_OR_FAIL(finish(nullptr));
    return HF3FS_CRC_OK;
  }
  // Batches of chunk-sized payloads hash as byte runs, like a scrub batch (4096 x 4 MiB: 2.54 ms
  // against 2.59 ms for create_batch).  A batch of small IOs does not: 1 Mi IOs of 4-64 KiB ran
  // 38 % slower as byte runs than create_batch's planner over the same bytes (profiles/
  // client_write.jsonl, record prepare_mix_runs), so the runs start at a bound of 1 MiB, the
  // planner's segment.  The run tables are reserved whatever max_len is.
  const bool runs_ok = max_len >= kClientWriteRunsMinLen;
  return run_record_jobs(
      c, type, n, max_len, s,
      [&](uint64_t* addr, uint64_t* len, uint32_t* ctl) {
        poison = ctl + 1;  // (run_record_jobs zeroes the four words; the range kernels read ctl[0] only)
        return launch_client_write_prep(d_ios, n, max_len, true, addr, len, ctl, s);
      },
      finish, {.what = "client write prepare", .runs_ok = runs_ok, .reserve_runs = true});
}

int hf3fs_crc_client_write_complete(hf3fs_crc_client_write_io* d_ios, uint64_t n, const uint64_t* d_file_off,
                                    uint64_t n_files, uint64_t max_ios_per_file, uint32_t flags,
                                    const hf3fs_crc_update_io* d_updates, const uint32_t* d_expected,
                                    hf3fs_crc_client_write_file* d_files, uint32_t* d_failed, uint64_t failed_cap,
                                    uint32_t* d_info, void* stream) {
  if (flags & ~(uint32_t)HF3FS_CLIENT_WRITE_FROM_UPDATES) return fail(HF3FS_CRC_INVALID_ARG, "unknown flags %#x", flags);
  if (!d_ios && n) return fail(HF3FS_CRC_INVALID_ARG, "null ios");
  if (!d_info) return fail(HF3FS_CRC_INVALID_ARG, "null info");
  if (n > kClientWriteMaxCount || n_files > kClientWriteMaxCount)
    return fail(HF3FS_CRC_INVALID_ARG, "too many IOs or files (%llu, %llu)", (unsigned long long)n,
                (unsigned long long)n_files);
  const bool from_updates = (flags & HF3FS_CLIENT_WRITE_FROM_UPDATES) != 0;
  if (from_updates && !d_updates) return fail(HF3FS_CRC_INVALID_ARG, "FROM_UPDATES needs update records");
  if (n_files && (!d_file_off || !d_files)) return fail(HF3FS_CRC_INVALID_ARG, "files need offsets and records");
  if (failed_cap && !d_failed) return fail(HF3FS_CRC_INVALID_ARG, "null failed list");
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_OR_FAIL(launch_zero_words(d_info, HF3FS_CLIENT_WRITE_DONE_WORDS, s));  // the kernels add into it
  if (n) {
    void* scratch = nullptr;
    if (int rc = call_scratch(c, s, client_write_scratch_bytes(n) + 16, &scratch)) return rc;
    ClientWriteScratch cs;
    client_write_scratch_carve((void*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15), n, &cs);
    HIP_OR_FAIL(launch_client_write_settle(d_ios, n, from_updates ? d_updates : nullptr, d_failed, failed_cap, d_info,
                                           cs, s));
  }
  if (n_files)
    HIP_OR_FAIL(launch_client_write_fold(d_ios, n, d_file_off, n_files, max_ios_per_file > kClientWriteLaneMaxIos,
                                         d_expected, d_files, d_info, c->tables, s));
  return HF3FS_CRC_OK;
}

// run_record_jobs' carve with the byte-run tables a large prepare adds, and complete's tail.
size_t hf3fs_crc_forward_scratch_bytes(uint64_t n) {
  if (n > kForwardMaxJobs) return 0;
  const size_t bytes = record_own_bytes(n, kRunBlocksMax, kSizingWaves, true) + forward_scratch_bytes(n) + 16;
  return roomy_words((bytes + 3) / 4) * 4;
}

static int forward_args(uint8_t type, const hf3fs_crc_forward_job* d_jobs, uint64_t n, const uint32_t* d_info) {
  if (int rc = record_type(type)) return rc;
  if (!d_jobs && n) return fail(HF3FS_CRC_INVALID_ARG, "null jobs");
  if (!d_info) return fail(HF3FS_CRC_INVALID_ARG, "null info");
  if (n > kForwardMaxJobs) return fail(HF3FS_CRC_INVALID_ARG, "too many jobs (%llu)", (unsigned long long)n);
  return HF3FS_CRC_OK;
}

int hf3fs_crc_forward_prepare(uint8_t type, hf3fs_crc_forward_job* d_jobs, uint64_t n, uint32_t max_len,
                              uint32_t max_inline_bytes, uint32_t* d_info, void* stream) {
  if (int rc = forward_args(type, d_jobs, n, d_info)) return rc;
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_OR_FAIL(launch_zero_words(d_info, HF3FS_FORWARD_INFO_WORDS, s));  // the finish adds into it
  if (n == 0) return HF3FS_CRC_OK;
  // Whole stored chunks, like a scrub batch: large batches hash as byte runs (runs_ok).  The tail
  // is complete's and the run tables are reserved in both calls, so that either call takes the same
  // bytes for n jobs whatever max_len is: the pair's buffer never grows between the two.
  return run_record_jobs(
      c, type, n, max_len, s,
      [&](uint64_t* addr, uint64_t* len, uint32_t* maxl) {
        return launch_forward_prep(d_jobs, n, type, max_len, false, addr, len, maxl, s);
      },
      [&](const uint32_t* v) {
        return launch_forward_prepare_finish(d_jobs, n, type, max_len, max_inline_bytes, v, d_info, s);
      },
      {.what = "forward prepare", .runs_ok = true, .reserve_runs = true, .tail_bytes = forward_scratch_bytes(n) + 16});
}

int hf3fs_crc_forward_complete(uint8_t type, hf3fs_crc_forward_job* d_jobs, uint64_t n, uint32_t max_len,
                               uint32_t* d_commit_idx, uint32_t* d_info, void* stream) {
  if (int rc = forward_args(type, d_jobs, n, d_info)) return rc;
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_OR_FAIL(launch_zero_words(d_info, HF3FS_FORWARD_INFO_WORDS, s));  // the finish adds into it
  if (n == 0) return HF3FS_CRC_OK;
  void* tail = nullptr;
  return run_record_jobs(
      c, type, n, max_len, s,
      [&](uint64_t* addr, uint64_t* len, uint32_t* maxl) {
        return launch_forward_prep(d_jobs, n, type, max_len, true, addr, len, maxl, s);
      },
      [&](const uint32_t* v) {
        ForwardScratch fs;
        forward_scratch_carve(tail, n, &fs);
        return launch_forward_complete_finish(d_jobs, n, type, max_len, v, d_commit_idx, d_info, fs, s);
      },
      {.what = "forward complete", .reserve_runs = true, .tail_bytes = forward_scratch_bytes(n) + 16, .tail = &tail});
}

// Complete takes run_record_jobs' carve without byte runs (reaped reads keep the planner, as read
// results do) and its own tail; prepare takes no scratch.
size_t hf3fs_crc_server_read_scratch_bytes(uint64_t n, uint64_t n_reqs) {
  if (n > kServerReadMaxCount || n_reqs > kServerReadMaxCount) return 0;
  const size_t bytes = record_own_bytes(n, 0, 0, false) + server_read_scratch_bytes(n) + 16;
  return roomy_words((bytes + 3) / 4) * 4;
}

static int server_read_args(const hf3fs_crc_server_read_job* d_jobs, uint64_t n, const hf3fs_crc_server_read_req* d_reqs,
                            const uint64_t* d_req_off, uint64_t n_reqs, const uint32_t* d_info) {
  if (!d_jobs && n) return fail(HF3FS_CRC_INVALID_ARG, "null jobs");
  if ((!d_reqs || !d_req_off) && n_reqs) return fail(HF3FS_CRC_INVALID_ARG, "requests need records and offsets");
  if (n && !n_reqs) return fail(HF3FS_CRC_INVALID_ARG, "%llu jobs of no request", (unsigned long long)n);
  if (!d_info) return fail(HF3FS_CRC_INVALID_ARG, "null info");
  if (n > kServerReadMaxCount || n_reqs > kServerReadMaxCount)
    return fail(HF3FS_CRC_INVALID_ARG, "too many jobs or requests (%llu, %llu)", (unsigned long long)n,
                (unsigned long long)n_reqs);
  return HF3FS_CRC_OK;
}

int hf3fs_crc_server_read_prepare(hf3fs_crc_server_read_job* d_jobs, uint64_t n, hf3fs_crc_server_read_req* d_reqs,
                                  const uint64_t* d_req_off, uint64_t n_reqs, uint64_t max_jobs_per_req,
                                  uint32_t small_buf, uint32_t big_buf, uint32_t* d_info, void* stream) {
  if (int rc = server_read_args(d_jobs, n, d_reqs, d_req_off, n_reqs, d_info)) return rc;
  (void)max_jobs_per_req;  // no effect at present: one lane walks one request whatever its length
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_OR_FAIL(launch_zero_words(d_info, HF3FS_SERVER_READ_INFO_WORDS, s));  // the kernel adds into it
  if (n_reqs == 0) return HF3FS_CRC_OK;
  HIP_OR_FAIL(launch_server_read_prepare(d_jobs, n, d_reqs, d_req_off, n_reqs, small_buf, big_buf, d_info, s));
  return HF3FS_CRC_OK;
}

int hf3fs_crc_server_read_complete(uint8_t type, hf3fs_crc_server_read_job* d_jobs, uint64_t n,
                                   hf3fs_crc_server_read_req* d_reqs, const uint64_t* d_req_off, uint64_t n_reqs,
                                   uint32_t max_len, void* d_inline, uint64_t inline_cap,
                                   hf3fs_crc_server_read_wr* d_wr, uint64_t wr_cap, uint32_t* d_info, void* stream) {
  if (int rc = record_type(type)) return rc;
  if (int rc = server_read_args(d_jobs, n, d_reqs, d_req_off, n_reqs, d_info)) return rc;
  if (inline_cap && !d_inline) return fail(HF3FS_CRC_INVALID_ARG, "null inline arena");
  if (wr_cap && !d_wr) return fail(HF3FS_CRC_INVALID_ARG, "null write list");
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_OR_FAIL(launch_zero_words(d_info, HF3FS_SERVER_READ_INFO_WORDS, s));  // the kernels add into it
  if (n_reqs == 0) return HF3FS_CRC_OK;
  if (n == 0) {  // requests of no job: their outputs alone
    HIP_OR_FAIL(launch_server_read_requests(d_jobs, 0, d_reqs, d_req_off, n_reqs, ServerReadScratch{}, s));
    return HF3FS_CRC_OK;
  }
  void* tail = nullptr;
  ServerReadScratch ss;
  return run_record_jobs(
      c, type, n, max_len, s,
      [&](uint64_t* addr, uint64_t* len, uint32_t* maxl) {
        server_read_scratch_carve(tail, n, &ss);
        return launch_server_read_prep(d_jobs, n, d_reqs, d_req_off, n_reqs, type, max_len, addr, len, maxl, ss, s);
      },
      [&](const uint32_t* v) {
        hipError_t e = launch_server_read_finish(d_jobs, n, d_reqs, type, max_len, v, inline_cap, d_wr, wr_cap, d_info,
                                                 ss, s);
        if (e == hipSuccess) e = launch_server_read_requests(d_jobs, n, d_reqs, d_req_off, n_reqs, ss, s);
        // The inline pack: a launch of its own behind the hash and the offsets, never fused with either.
        if (e == hipSuccess && d_inline && inline_cap) e = launch_server_read_pack(d_jobs, n, d_inline, inline_cap, d_info, ss, s);
        return e;
      },
      {.what = "server read complete", .tail_bytes = server_read_scratch_bytes(n) + 16, .tail = &tail});
}

int hf3fs_crc_scrub_batch(uint8_t type, hf3fs_crc_scrub_io* d_ios, uint64_t n, uint32_t max_len,
                          uint32_t* d_mismatch_count, void* stream) {
  if (int rc = record_type(type)) return rc;
  if (!d_mismatch_count) return fail(HF3FS_CRC_INVALID_ARG, "null mismatch count");
  hipStream_t s = (hipStream_t)stream;
  HIP_OR_FAIL(launch_zero_words(d_mismatch_count, 1, s));
  if (n == 0) return HF3FS_CRC_OK;
  if (!d_ios) return fail(HF3FS_CRC_INVALID_ARG, "null ios");
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  return run_record_jobs(
      c, type, n, max_len, s, [&](uint64_t* addr, uint64_t* len, uint32_t* maxl) {
        return launch_scrub_prep(d_ios, n, type, max_len, addr, len, maxl, s);
      },
      [&](const uint32_t* v) { return launch_scrub_finalize(d_ios, n, v, d_mismatch_count, s); },
      {.what = "scrub", .runs_ok = true});
}

size_t hf3fs_crc_sync_plan_scratch_bytes(uint64_t n_local, uint64_t n_remote) {
  if (n_local > kSyncMaxRecords || n_remote > kSyncMaxRecords) return 0;
  return sync_scratch_bytes(n_local, n_remote);
}

int hf3fs_crc_sync_plan(hf3fs_crc_sync_meta* d_local, uint64_t n_local, hf3fs_crc_sync_meta* d_remote,
                        uint64_t n_remote, uint32_t chain_ver, uint32_t flags, uint32_t* d_write, uint32_t* d_remove,
                        uint32_t* d_info, void* stream) {
  if (!d_info) return fail(HF3FS_CRC_INVALID_ARG, "null info");
  if ((!d_local && n_local) || (!d_remote && n_remote)) return fail(HF3FS_CRC_INVALID_ARG, "null table");
  if (flags & ~(uint32_t)HF3FS_SYNC_HEAVY) return fail(HF3FS_CRC_INVALID_ARG, "unknown flags %#x", flags);
  if (n_local > kSyncMaxRecords || n_remote > kSyncMaxRecords)
    return fail(HF3FS_CRC_INVALID_ARG, "too many records (%llu local, %llu remote)", (unsigned long long)n_local,
                (unsigned long long)n_remote);
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  // Empty tables take the same launches (every loop is empty): d_info becomes the empty plan.
  void* base = nullptr;
  if (int rc = call_scratch(c, s, sync_scratch_bytes(n_local, n_remote), &base)) return rc;
  SyncScratch ss;
  sync_scratch_carve(base, n_local, n_remote, &ss);
  HIP_OR_FAIL(launch_sync_plan(d_local, n_local, d_remote, n_remote, chain_ver, flags, d_write, d_remove, d_info, ss, s));
  return HF3FS_CRC_OK;
}

size_t hf3fs_crc_range_query_scratch_bytes(uint64_t n_meta, uint64_t n_ops) {
  if (n_meta > kRangeMaxCount || n_ops > kRangeMaxCount) return 0;
  return range_scratch_bytes(n_meta, n_ops);
}

int hf3fs_crc_range_query(const hf3fs_crc_sync_meta* d_meta, uint64_t n_meta, hf3fs_crc_range_op* d_ops, uint64_t n_ops,
                          uint32_t* d_list, uint64_t list_cap, uint32_t* d_info, void* stream) {
  if (!d_info) return fail(HF3FS_CRC_INVALID_ARG, "null info");
  if ((!d_meta && n_meta) || (!d_ops && n_ops)) return fail(HF3FS_CRC_INVALID_ARG, "null table or ops");
  if (n_meta > kRangeMaxCount || n_ops > kRangeMaxCount)
    return fail(HF3FS_CRC_INVALID_ARG, "too many records or ops (%llu, %llu)", (unsigned long long)n_meta,
                (unsigned long long)n_ops);
  if (!d_list && list_cap) return fail(HF3FS_CRC_INVALID_ARG, "null list");
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  // Empty arrays take the same launches (every loop is empty): d_info becomes the empty result.
  void* base = nullptr;
  if (int rc = call_scratch(c, s, range_scratch_bytes(n_meta, n_ops), &base)) return rc;
  RangeScratch rs;
  range_scratch_carve(base, n_meta, n_ops, &rs);
  HIP_OR_FAIL(launch_range_query(d_meta, n_meta, d_ops, n_ops, d_list, list_cap, d_info, rs, s));
  return HF3FS_CRC_OK;
}

int hf3fs_crc_file_length(const hf3fs_crc_range_op* d_ops, uint64_t n_ops, hf3fs_crc_file_len* d_files,
                          uint64_t n_files, uint32_t* d_info, void* stream) {
  if (!d_info) return fail(HF3FS_CRC_INVALID_ARG, "null info");
  if ((!d_ops && n_ops) || (!d_files && n_files)) return fail(HF3FS_CRC_INVALID_ARG, "null ops or files");
  if (n_ops > kRangeMaxCount || n_files > kRangeMaxCount)
    return fail(HF3FS_CRC_INVALID_ARG, "too many ops or files (%llu, %llu)", (unsigned long long)n_ops,
                (unsigned long long)n_files);
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_OR_FAIL(launch_zero_words(d_info, HF3FS_FILE_LEN_INFO_WORDS, s));  // the kernel adds into it
  if (n_files == 0) return HF3FS_CRC_OK;
  HIP_OR_FAIL(launch_file_length(d_ops, n_ops, d_files, n_files, d_info, s));
  return HF3FS_CRC_OK;
}

size_t hf3fs_crc_md5_scratch_bytes(uint64_t n_files) {
  if (n_files > kMd5MaxCount) return 0;
  // What the pair's buffer is sized to by a first call of n_files (a captured call's own memory is
  // the carve's exact bytes, which are fewer).
  return roomy_words((md5_scratch_bytes(n_files) + 3) / 4) * 4;
}

int hf3fs_crc_md5_batch(const hf3fs_crc_md5_seg* d_segs, const uint64_t* d_file_off, uint64_t n_files, uint64_t n_segs,
                        hf3fs_crc_md5_state* d_state, uint8_t* d_out, uint32_t flags, void* stream) {
  if (n_files == 0) return HF3FS_CRC_OK;
  if (!d_file_off) return fail(HF3FS_CRC_INVALID_ARG, "null file offsets");
  if (n_segs && !d_segs) return fail(HF3FS_CRC_INVALID_ARG, "null segments");
  constexpr uint32_t kBoth = HF3FS_MD5_INIT | HF3FS_MD5_FINAL;
  if (flags & ~kBoth) return fail(HF3FS_CRC_INVALID_ARG, "unknown flags %#x", flags);
  if (!d_state && flags != kBoth) return fail(HF3FS_CRC_INVALID_ARG, "null state needs INIT | FINAL");
  if ((flags & HF3FS_MD5_FINAL) && !d_out) return fail(HF3FS_CRC_INVALID_ARG, "FINAL with null output");
  if (n_files > kMd5MaxCount || n_segs > kMd5MaxCount)
    return fail(HF3FS_CRC_INVALID_ARG, "too many files or segments (%llu, %llu)", (unsigned long long)n_files,
                (unsigned long long)n_segs);
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  void* base = nullptr;
  if (int rc = call_scratch(c, s, md5_scratch_bytes(n_files), &base)) return rc;
  Md5Scratch ms;
  md5_scratch_carve(base, n_files, &ms);
  const Options& o = options();
  HIP_OR_FAIL(launch_md5_batch(d_segs, d_file_off, n_files, n_segs, d_state, d_out, flags, o.md5_sort.load() != 0,
                               o.md5_stage.load() != 0, ms, s));
  return HF3FS_CRC_OK;
}

uint32_t hf3fs_crc_md5_hex(const uint8_t* digest16, char* out32) {
  static const char kHex[] = "0123456789abcdef";
  for (int i = 0; i < 16; ++i) {
    out32[2 * i] = kHex[digest16[i] >> 4];
    out32[2 * i + 1] = kHex[digest16[i] & 15];
  }
  return 32;
}

int hf3fs_crc_sync_scrub_fill(const hf3fs_crc_sync_meta* d_local, const uint64_t* d_addrs, const uint32_t* d_write,
                              const uint32_t* d_info, uint64_t n_local, hf3fs_crc_scrub_io* d_scrub, void* stream) {
  if (n_local == 0) return HF3FS_CRC_OK;
  if (!d_local || !d_addrs || !d_write || !d_info || !d_scrub) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
  if (n_local > kSyncMaxRecords)
    return fail(HF3FS_CRC_INVALID_ARG, "too many records (%llu)", (unsigned long long)n_local);
  HIP_OR_FAIL(launch_sync_scrub_fill(d_local, d_addrs, d_write, d_info, n_local, d_scrub, (hipStream_t)stream));
  return HF3FS_CRC_OK;
}

int hf3fs_crc_frame_verify_batch(const void* d_buf, hf3fs_crc_frame* d_frames, uint64_t n, uint32_t max_size,
                                 uint32_t* d_mismatch_count, void* stream) {
  if (!d_mismatch_count) return fail(HF3FS_CRC_INVALID_ARG, "null mismatch count");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0 || !d_frames || !d_buf || n >= (1ull << 31)) {  // (the map launch zeroes the count otherwise)
    HIP_OR_FAIL(launch_zero_words(d_mismatch_count, 1, s));
    if (n == 0) return HF3FS_CRC_OK;
    if (!d_frames || !d_buf) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
    return fail(HF3FS_CRC_INVALID_ARG, "too many frames (%llu)", (unsigned long long)n);
  }
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  const uint8_t* buf = (const uint8_t*)d_buf;
  // The stream path (frame_kernels.h) is tried for batches of walked frames;
  // the device falls back to one record job per frame when they are not sorted
  // and disjoint.  Option frame_stream = 0 / 1 forces it off / on (A/B).
  const Options& o = options();
  const int fs = o.frame_stream.load();
  const bool try_stream = fs < 0 ? n >= kFrameStreamMinFrames : fs != 0;
  const uint64_t waves = (uint64_t)c->cus * kWaves;
  const uint64_t segw = o.frame_segw.load();
  const uint64_t cap = try_stream ? frame_stream_cap(waves, segw) : 0;
  // scratch {flags[4], sums[2] (u64: payload bytes, gap bytes), ticket counter, (pad to 64 B),
  // addr[n], len[n], v[n], params, seg_first[cap], seg_lin[cap], seg_pre[cap]}; the stream path's
  // boundary values ev[2n] reuse addr (the record path's, idle then).  ONE zeroing launch: the
  // flags; the map launch zeroes the mismatch count and, on the record path, v.
  const size_t head = (4 * kFrameFlagWords + n * (8 + 8 + 4) + 63) / 64 * 64;
  const size_t bytes = head + sizeof(FrameStreamParams) + 12 * cap + 64;
  void* scratch = nullptr;
  if (int rc = call_scratch(c, s, bytes, &scratch)) return rc;
  uint8_t* base = (uint8_t*)scratch;
  uint32_t* flags = (uint32_t*)base;
  uint64_t* addr = (uint64_t*)(base + 4 * kFrameFlagWords);
  uint64_t* len = addr + n;
  uint32_t* v = (uint32_t*)(len + n);
  FrameStreamParams* prm = (FrameStreamParams*)(base + head);
  uint32_t* seg_first = (uint32_t*)(prm + 1);
  uint32_t* seg_lin = seg_first + cap;
  uint32_t* seg_pre = seg_lin + cap;
  uint32_t* ev = (uint32_t*)addr;
  int rc = HF3FS_CRC_OK;
  hipError_t e = launch_zero_words(flags, kFrameFlagWords, s);
  if (e == hipSuccess && try_stream) e = launch_frame_check(d_frames, n, max_size, flags, s);
  if (e == hipSuccess)
    e = launch_frame_map(buf, d_frames, n, segw * waves ? segw * waves : 1, waves, flags, prm, seg_first, max_size, addr,
                         len, v, d_mismatch_count, try_stream, s);
  if (e != hipSuccess) rc = fail(HF3FS_CRC_DEVICE_ERROR, "frame map: %s", hipGetErrorString(e));
  if (!rc) {  // record path (returns at once when the stream path took the batch); v and the
              // ticket counter (flags[8]) are zeroed already
    ListSource src{addr, len, nullptr, n, 0u};  // calcSerde hashes with init 0 (MessageHeader.h:35)
    rc = run_ranges_list(c, kTypeCrc32c, src, max_size, v, s, 0, flags, flags + 1, flags + 8);
  }
  if (!rc && try_stream) {
    e = launch_frame_stream(buf, d_frames, n, flags, prm, seg_first, seg_lin, ev, (uint32_t)c->cus, c->tables, s);
    if (e == hipSuccess) e = launch_frame_seg_scan(flags, prm, seg_lin, seg_pre, c->tables, s);
    if (e != hipSuccess) rc = fail(HF3FS_CRC_DEVICE_ERROR, "frame stream: %s", hipGetErrorString(e));
  }
  if (!rc) {
    e = launch_frame_finalize(buf, d_frames, n, v, flags, prm, ev, seg_lin, seg_pre, d_mismatch_count, c->tables, s);
    if (e != hipSuccess) rc = fail(HF3FS_CRC_DEVICE_ERROR, "frame finalize: %s", hipGetErrorString(e));
  }
  return rc;
}

int hf3fs_crc_file_digest_batch_ex(const hf3fs_crc_block_digest* d_blocks, const uint64_t* d_file_off,
                                   hf3fs_crc_file_digest* d_out, uint64_t n_files, uint64_t max_blocks, uint32_t flags,
                                   void* stream) {
  if (n_files == 0) return HF3FS_CRC_OK;
  if (!d_file_off || !d_out || (!d_blocks && max_blocks)) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
  if (flags & ~uint32_t(HF3FS_DIGEST_FILL_ZERO)) return fail(HF3FS_CRC_INVALID_ARG, "unknown flags %#x", flags);
  const bool fill_zero = flags & HF3FS_DIGEST_FILL_ZERO;
  const uint32_t splits = digest_splits(max_blocks);
  if (n_files * splits >= (1ull << 24)) return fail(HF3FS_CRC_INVALID_ARG, "too many files (%llu)",
                                                    (unsigned long long)n_files);
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = digest_scratch_bytes(n_files, splits, fill_zero);
  void* scratch = nullptr;
  if (bytes)
    if (int rc = call_scratch(c, s, bytes, &scratch)) return rc;
  hipError_t e =
      launch_file_digest(d_blocks, d_file_off, n_files, max_blocks, splits, fill_zero, scratch, d_out, c->tables, s);
  if (e != hipSuccess) return fail(HF3FS_CRC_DEVICE_ERROR, "file digest: %s", hipGetErrorString(e));
  return HF3FS_CRC_OK;
}

int hf3fs_crc_file_digest_batch(const hf3fs_crc_block_digest* d_blocks, const uint64_t* d_file_off,
                                hf3fs_crc_file_digest* d_out, uint64_t n_files, uint64_t max_blocks, void* stream) {
  return hf3fs_crc_file_digest_batch_ex(d_blocks, d_file_off, d_out, n_files, max_blocks, HF3FS_DIGEST_FILL_ZERO,
                                        stream);
}

// ---------------------------------------------------------------------------
// Host buffers: pieces of <= kStage bytes are packed into a pinned stage,
// copied H2D and hashed (start 0 -> linear CRC of the piece) on one of two
// streams while the next stage is packed; the pieces of each buffer are then
// stitched on the host with the combine algebra:
//   raw(buf, start) = start * x^(8 len) ^ sum_j lin(piece_j) * x^(8 * bytes after piece j).
int hf3fs_crc_create_host(uint8_t type, const void* const* h_bufs, const uint64_t* h_lens, const uint32_t* h_starts,
                          uint32_t* h_out, uint64_t n) {
  if (!valid_type(type)) return fail(HF3FS_CRC_INVALID_ARG, "unknown checksum type %u", type);
  if (n == 0) return HF3FS_CRC_OK;
  if (!h_bufs || !h_lens || !h_out) return fail(HF3FS_CRC_INVALID_ARG, "null argument");
  if (type == kTypeNone) {
    for (uint64_t i = 0; i < n; ++i) h_out[i] = 0;
    return HF3FS_CRC_OK;
  }
  Context* c = nullptr;
  if (int rc = get_context(&c)) return rc;
  std::lock_guard<std::mutex> lk(c->stage_mu);
  // An error return must not leave copies in flight into the pinned stages the
  // next call refills: drain both staging streams first.
  const int rc = create_host_staged(c, type, h_bufs, h_lens, h_starts, h_out, n);
  if (rc != HF3FS_CRC_OK)
    for (int k = 0; k < 2; ++k)
      if (c->streams[k]) (void)hipStreamSynchronize(c->streams[k]);
  return rc;
}

}  // extern "C"

namespace {
int create_host_staged(Context* c, uint8_t type, const void* const* h_bufs, const uint64_t* h_lens,
                       const uint32_t* h_starts, uint32_t* h_out, uint64_t n) {
  constexpr size_t kStage = Context::kStage;
  constexpr size_t kMaxPieces = 4096;
  if (!c->pinned[0]) {
    for (int k = 0; k < 2; ++k) {
      HIP_OR_FAIL(hipHostMalloc((void**)&c->pinned[k], kStage, hipHostMallocDefault));
      HIP_OR_FAIL(hipHostMalloc((void**)&c->pdesc[k], kMaxPieces * 5 * sizeof(uint64_t), hipHostMallocDefault));
      HIP_OR_FAIL(hipMalloc(&c->dstage[k], kStage));
      HIP_OR_FAIL(hipMalloc(&c->ddesc[k], kMaxPieces * 5 * sizeof(uint64_t)));
      HIP_OR_FAIL(hipStreamCreateWithFlags(&c->streams[k], hipStreamNonBlocking));
    }
  }
  const uint32_t poly = poly_of(type);
  for (uint64_t i = 0; i < n; ++i) h_out[i] = gf_mul(h_starts ? h_starts[i] : ~0u, xpow_bits(8 * h_lens[i], poly), poly);

  struct Piece {
    uint64_t buf, tail;  // buffer index, bytes after the piece in its buffer
  };
  std::vector<Piece> pieces[2];
  uint64_t npieces[2] = {0, 0};
  bool busy[2] = {false, false};
  int k = 0;
  uint64_t bi = 0, boff = 0;
  auto drain = [&](int slot) -> int {
    if (!busy[slot]) return HF3FS_CRC_OK;
    HIP_OR_FAIL(hipStreamSynchronize(c->streams[slot]));
    const uint32_t* res = reinterpret_cast<const uint32_t*>(c->pdesc[slot] + 4 * kMaxPieces);
    for (uint64_t j = 0; j < npieces[slot]; ++j) {
      const Piece& pc = pieces[slot][j];
      h_out[pc.buf] ^= gf_mul(res[j], xpow_bits(8 * pc.tail, poly), poly);
    }
    busy[slot] = false;
    return HF3FS_CRC_OK;
  };
  while (bi < n) {
    if (int rc = drain(k)) return rc;
    pieces[k].clear();
    uint64_t used = 0, np = 0;
    uint64_t* addrs = c->pdesc[k];
    uint64_t* lens = c->pdesc[k] + kMaxPieces;
    while (bi < n && np < kMaxPieces && used < kStage) {
      const uint64_t len = h_lens[bi];
      if (boff >= len) {
        ++bi;
        boff = 0;
        continue;
      }
      const uint64_t take = std::min<uint64_t>(len - boff, kStage - used);
      memcpy(c->pinned[k] + used, (const uint8_t*)h_bufs[bi] + boff, take);
      addrs[np] = (uint64_t)(c->dstage[k] + used);
      lens[np] = take;
      pieces[k].push_back({bi, len - boff - take});
      ++np;
      used = (used + take + 15) & ~uint64_t(15);
      boff += take;
    }
    if (np == 0) break;
    npieces[k] = np;
    hipStream_t s = c->streams[k];
    HIP_OR_FAIL(hipMemcpyAsync(c->dstage[k], c->pinned[k], std::min<uint64_t>(used, kStage), hipMemcpyHostToDevice, s));
    HIP_OR_FAIL(hipMemcpyAsync(c->ddesc[k], c->pdesc[k], 2 * kMaxPieces * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    uint32_t* dout = reinterpret_cast<uint32_t*>(c->ddesc[k] + 4 * kMaxPieces);
    ListSource src{c->ddesc[k], c->ddesc[k] + kMaxPieces, nullptr, np, 0u};
    if (int rc = run_ranges_list(c, type, src, kStage, dout, s)) return rc;
    HIP_OR_FAIL(hipMemcpyAsync(c->pdesc[k] + 4 * kMaxPieces, dout, np * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    busy[k] = true;
    k ^= 1;
  }
  if (int rc = drain(0)) return rc;
  if (int rc = drain(1)) return rc;
  return HF3FS_CRC_OK;
}
}  // namespace
