// capture_scratch.h -- device memory of calls captured into graphs (capture_scratch.hip), and
// the relaxed capture mode in which the library allocates for itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace hf3fs_crc {

// The calling thread in relaxed capture mode for a scope (back to the caller's mode at its
// end): what the library allocates, frees or creates for itself inside -- never a graph node --
// is neither rejected as capture-unsupported nor invalidates a capture when the call sits
// inside one, or beside another thread's (torch.cuda.graph's default mode is global).
struct RelaxedCapture {
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  hipError_t err;
  RelaxedCapture() : err(hipThreadExchangeStreamCaptureMode(&mode)) {}
  ~RelaxedCapture() {
    if (err == hipSuccess) (void)hipThreadExchangeStreamCaptureMode(&mode);
  }
  RelaxedCapture(const RelaxedCapture&) = delete;
  RelaxedCapture& operator=(const RelaxedCapture&) = delete;
};

// `bytes` of device memory for the call being captured on s, owned by the capture's graph.
hipError_t capture_malloc(int device, hipStream_t s, size_t bytes, void** out);

// Free the buffers of destroyed graphs (force), or from an uncaptured call only once they
// hold kCapReapBytes.
void reap_captured(bool force = false);

// Free every captured call's buffers (hf3fs_crc_shutdown): graphs still alive must not be replayed.
void free_all_captured();

}  // namespace hf3fs_crc
