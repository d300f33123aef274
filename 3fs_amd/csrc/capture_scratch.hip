// capture_scratch.hip -- scratch of calls captured into graphs (capture_scratch.h).
//
// Every captured call gets device memory of its own (ticket counter, balance region,
// verify values, batch scratch), owned by the graph it was captured into.  One owner
// record per capture sequence (keyed by the capture id): one hipUserObject whose
// reference the graph holds -- and every executable graph instantiated from it -- and
// the capture's buffers: requests of <= kCapSmall bytes are carved from kCapSlab-byte
// slabs of the capture, larger ones get buffers of their own.  When the last reference
// goes, the destructor moves the buffers to the dead list.  A destructor may not call
// HIP, so dead buffers are freed by hf3fs_crc_release_graph_scratch, release_stream,
// shutdown, or by an uncaptured call once the dead list holds >= kCapReapBytes (never
// in every call: hipFree waits for the whole device).  That device-wide wait of hipFree
// is also what makes the free safe for an executable graph destroyed while a replay
// is still in flight (HIP may release user objects at hipGraphExecDestroy without
// waiting for pending launches).  A capture whose graph could not take the reference
// (orphan) keeps its buffers until release_graph_scratch or shutdown.  The registry is
// process-wide (a graph may outlive hf3fs_crc_shutdown) and a heap object that is never
// destroyed, so a late destructor callback from the HIP runtime's own teardown after
// this library's static destructors still finds a live mutex and map.  Owners are keyed
// by a never-reused id (the user object's payload), not by address.
#include "capture_scratch.h"

#include <atomic>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/hf3fs_crc.h"

namespace hf3fs_crc {
namespace {

struct CapturedBuf {
  void* ptr;
  int device;
  size_t bytes;
};
struct CaptureOwner {
  std::vector<CapturedBuf> bufs;
  unsigned long long cap_id = 0;  // the capture sequence (by_capture key), 0 = none
  bool orphan = true;
  uint8_t* slab = nullptr;  // the current slab and its fill
  size_t slab_used = 0;
};
constexpr size_t kCapSmall = 64 << 10, kCapSlab = 256 << 10, kCapReapBytes = 64ull << 20;
struct CapRegistry {
  std::mutex mu;
  std::map<uint64_t, CaptureOwner> live;                  // owner id -> owner
  std::map<unsigned long long, uint64_t> by_capture;      // capture id -> owner id (capture in progress)
  std::vector<CapturedBuf> dead;
  std::atomic<size_t> dead_n{0}, dead_bytes{0};
  uint64_t next_id = 1;
};
CapRegistry& cap_reg() {
  static CapRegistry* r = new CapRegistry;  // intentionally leaked (late destructor callbacks)
  return *r;
}

// A buffer of owner o, from hipMalloc while the calling thread's stream is being captured:
// in relaxed capture mode the allocation is no graph node and invalidates no capture.
// Library scratch never comes from the stream-ordered pool.
hipError_t owner_malloc(CaptureOwner& o, int device, size_t bytes, void** p) {
  RelaxedCapture relaxed;
  const hipError_t e = relaxed.err != hipSuccess ? relaxed.err : hipMalloc(p, bytes);
  if (e == hipSuccess) o.bufs.push_back(CapturedBuf{*p, device, bytes});
  return e;
}

void captured_graph_gone(void* id) {
  CapRegistry& R = cap_reg();
  std::lock_guard<std::mutex> lk(R.mu);
  auto it = R.live.find((uint64_t)(uintptr_t)id);
  if (it == R.live.end() || it->second.orphan) return;  // freed already (shutdown), or no graph owns it
  for (const CapturedBuf& b : it->second.bufs) {
    R.dead.push_back(b);
    R.dead_bytes.fetch_add(b.bytes);
  }
  auto bc = R.by_capture.find(it->second.cap_id);
  if (bc != R.by_capture.end() && bc->second == it->first) R.by_capture.erase(bc);
  R.live.erase(it);
  R.dead_n.store(R.dead.size());
}

// hipFree the buffers of destroyed graphs.  Relaxed capture mode for the frees, so that
// another thread's global-mode capture neither fails this call nor is invalidated by it.
void free_captured(std::vector<CapturedBuf>& dead) {
  if (dead.empty()) return;
  int prev = 0;
  (void)hipGetDevice(&prev);
  RelaxedCapture relaxed;
  for (const CapturedBuf& b : dead) {
    (void)hipSetDevice(b.device);
    (void)hipFree(b.ptr);
  }
  (void)hipSetDevice(prev);
}

}  // namespace

void reap_captured(bool force) {
  CapRegistry& R = cap_reg();
  if (R.dead_n.load(std::memory_order_relaxed) == 0) return;
  if (!force && R.dead_bytes.load(std::memory_order_relaxed) < kCapReapBytes) return;
  std::vector<CapturedBuf> dead;
  {
    std::lock_guard<std::mutex> lk(R.mu);
    dead.swap(R.dead);
    R.dead_n.store(0);
    R.dead_bytes.store(0);
  }
  free_captured(dead);
}

void free_all_captured() {
  std::vector<CapturedBuf> all;
  {
    CapRegistry& R = cap_reg();
    std::lock_guard<std::mutex> lk(R.mu);
    all.swap(R.dead);
    for (auto& kv : R.live) all.insert(all.end(), kv.second.bufs.begin(), kv.second.bufs.end());
    R.live.clear();
    R.by_capture.clear();
    R.dead_n.store(0);
    R.dead_bytes.store(0);
  }
  free_captured(all);
}

hipError_t capture_malloc(int device, hipStream_t s, size_t bytes, void** out) {
  CapRegistry& R = cap_reg();
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long cap_id = 0;
  hipGraph_t graph = nullptr;
  const bool info = hipStreamGetCaptureInfo_v2(s, &st, &cap_id, &graph, nullptr, nullptr) == hipSuccess && graph &&
                    st == hipStreamCaptureStatusActive;
  uint64_t id = 0;
  bool fresh = false;
  {
    std::lock_guard<std::mutex> lk(R.mu);
    auto bc = info ? R.by_capture.find(cap_id) : R.by_capture.end();
    auto ow = bc != R.by_capture.end() ? R.live.find(bc->second) : R.live.end();
    if (ow == R.live.end() || ow->second.bufs.empty() || ow->second.bufs.front().device != device) {
      id = R.next_id++;
      R.live[id].cap_id = info ? cap_id : 0;  // an orphan until its graph holds the reference
      if (info) R.by_capture[cap_id] = id;
      fresh = true;
    } else {
      id = ow->first;
    }
  }
  if (fresh && info) {  // the owner's user object, retained by the graph
    hipUserObject_t obj = nullptr;
    if (hipUserObjectCreate(&obj, (void*)(uintptr_t)id, captured_graph_gone, 1, hipUserObjectNoDestructorSync) ==
        hipSuccess) {
      {  // owned before the graph holds the reference: the destructor may run as soon as it does
        std::lock_guard<std::mutex> lk(R.mu);
        R.live[id].orphan = false;
      }
      if (hipGraphRetainUserObject(graph, obj, 1, hipGraphUserObjectMove) != hipSuccess) {
        {
          std::lock_guard<std::mutex> lk(R.mu);
          R.live[id].orphan = true;  // the release below then frees nothing
        }
        (void)hipUserObjectRelease(obj, 1);
      }
    }
  }
  std::lock_guard<std::mutex> lk(R.mu);
  auto it = R.live.find(id);
  if (it == R.live.end()) return hipErrorInvalidValue;  // (the graph died during this call)
  CaptureOwner& o = it->second;
  const size_t need = (bytes + 255) & ~size_t(255);
  if (need <= kCapSmall) {
    if (!o.slab || o.slab_used + need > kCapSlab) {
      void* p = nullptr;
      if (const hipError_t e = owner_malloc(o, device, kCapSlab, &p)) return e;
      o.slab = (uint8_t*)p;
      o.slab_used = 0;
    }
    *out = o.slab + o.slab_used;
    o.slab_used += need;
    return hipSuccess;
  }
  return owner_malloc(o, device, bytes, out);
}

}  // namespace hf3fs_crc

using namespace hf3fs_crc;

extern "C" {

int hf3fs_crc_release_graph_scratch(void) {
  reap_captured(true);  // buffers of graphs already destroyed
  std::vector<CapturedBuf> orphans;
  {
    CapRegistry& R = cap_reg();
    std::lock_guard<std::mutex> lk(R.mu);
    for (auto it = R.live.begin(); it != R.live.end();) {
      if (it->second.orphan) {
        orphans.insert(orphans.end(), it->second.bufs.begin(), it->second.bufs.end());
        it = R.live.erase(it);
      } else {
        ++it;
      }
    }
    // finished captures: no later allocation joins them
    for (auto it = R.by_capture.begin(); it != R.by_capture.end();)
      it = R.live.count(it->second) ? ++it : R.by_capture.erase(it);
  }
  free_captured(orphans);
  return HF3FS_CRC_OK;
}

int hf3fs_crc_graph_scratch_stats(uint64_t* live_buffers, uint64_t* live_bytes, uint64_t* dead_buffers) {
  CapRegistry& R = cap_reg();
  std::lock_guard<std::mutex> lk(R.mu);
  uint64_t bytes = 0, n = 0;
  for (auto& kv : R.live)
    for (const CapturedBuf& b : kv.second.bufs) {
      bytes += b.bytes;
      ++n;
    }
  if (live_buffers) *live_buffers = n;
  if (live_bytes) *live_bytes = bytes;
  if (dead_buffers) *dead_buffers = R.dead.size();
  return HF3FS_CRC_OK;
}

}  // extern "C"
