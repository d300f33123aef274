// copy_range.h -- the update apply's byte copy (doRealWrite on HBM): copy_range and copy_range_hw,
// with any source and destination alignment.  update_kernels.hip applies payloads with it and
// server_read_kernels.hip packs the inline response; each unit instantiates its own copies.
#pragma once
#include "crc_device.h"

namespace hf3fs_crc {
namespace {

// ---------------------------------------------------------------------------
// byte copy with arbitrary source/destination alignment (doRealWrite on HBM)
// dst[0, len) = src ? src[0, len) : 0, executed by `nthreads` cooperating
// threads (tid = 0..nthreads-1: a workgroup or one wave): full 16-byte
// destination granules are written with aligned dwordx4 stores, four in flight
// per thread; the (at most two) partial granules at the ends byte by byte.
// 16 bytes at byte offset sh (1..15) into the 32-byte window A:B.
__device__ __forceinline__ u32x4 funnel16(const u32x4& A, const u32x4& B, uint32_t sh) {
  const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
  const uint32_t q = sh >> 2, r = sh & 3;
  uint32_t t[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) t[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
  u32x4 o;
  o.x = __builtin_amdgcn_alignbyte(t[1], t[0], r);
  o.y = __builtin_amdgcn_alignbyte(t[2], t[1], r);
  o.z = __builtin_amdgcn_alignbyte(t[3], t[2], r);
  o.w = __builtin_amdgcn_alignbyte(t[4], t[3], r);
  return o;
}

// Copy rows of full destination granules from a source misaligned by sh != 0
// with ONE aligned source load per granule: a wave's 64 lanes cover 64
// consecutive granules, lane l takes the upper neighbour granule from lane
// l + 1 (ds_bpermute) and lane 63 loads it.  Returns the first granule index
// (per thread) not yet copied; only wave-uniform rows are taken here.
template <int U, bool NT, bool NTS = NT>
__device__ __forceinline__ uint64_t copy_rows_shfl(uint64_t gdst, uint64_t sg0, uint32_t sh, uint64_t ng,
                                                   uint64_t g, uint64_t stride) {
  const uint32_t lane = (uint32_t)(g & 63);  // stride and the thread's start are multiples of 64 apart
  uint64_t gw = g - lane;                    // the wave's first granule of the row
  for (; gw + 63 + (U - 1) * stride < ng; gw += U * stride) {  // wave-uniform
    u32x4 a[U], b[U];
#pragma unroll
    for (int k = 0; k < U; ++k) a[k] = ld16<NT>(sg0 + (gw + lane + k * stride) * 16);
#pragma unroll
    for (int k = 0; k < U; ++k) b[k] = lane == 63 ? ld16<NT>(sg0 + (gw + 64 + k * stride) * 16) : a[k];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const u32x4 nb{(uint32_t)__shfl_down((int)a[k].x, 1, 64), (uint32_t)__shfl_down((int)a[k].y, 1, 64),
                     (uint32_t)__shfl_down((int)a[k].z, 1, 64), (uint32_t)__shfl_down((int)a[k].w, 1, 64)};
      st16<NTS>(gdst + (gw + lane + k * stride) * 16, funnel16(a[k], lane == 63 ? b[k] : nb, sh));
    }
  }
  return gw + lane;
}

template <int U = 4, bool NT = false, bool SHFL = false, int ALIGN = 0, bool NTS = NT>
__device__ void copy_range(uint64_t dst, uint64_t src, uint64_t len, uint32_t tid, uint32_t nthreads) {
  const uint64_t d0 = dst, d1 = dst + len;
  const uint64_t gfirst = (d0 + 15) & ~uint64_t(15);  // first full granule
  const uint64_t glast = d1 & ~uint64_t(15);          // end of full granules
  {  // partial head [d0, hend) and tail [tstart, d1): at most 30 bytes, one per thread
    const uint64_t hend = gfirst < d1 ? gfirst : d1;
    const uint64_t tstart = glast >= gfirst ? glast : d1;
    const uint64_t nh = hend - d0, nt = d1 - tstart;
    if (tid < nh + nt) {
      const uint64_t b = tid < nh ? d0 + tid : tstart + (tid - nh);
      *reinterpret_cast<uint8_t*>(b) = src ? load_byte(src + (b - d0), kSiteCopyByte) : 0;
    }
  }
  if (glast <= gfirst) return;
  uint64_t gfirst_rows = gfirst;
  if (ALIGN) {  // granules up to the first ALIGN-byte boundary one per thread (ALIGN <= 16 nthreads):
                // every wave row below is 8 whole 128 B lines
    const uint64_t ga0 = (gfirst + ALIGN - 1) & ~uint64_t(ALIGN - 1);
    const uint64_t ga = ga0 < glast ? ga0 : glast;
    if (tid < (ga - gfirst) / 16) {
      const uint64_t gd = gfirst + 16 * (uint64_t)tid;
      st16<NTS>(gd, src ? ld16_unaligned<NT>(src + (gd - d0)) : u32x4{0, 0, 0, 0});
    }
    gfirst_rows = ga;
    if (glast <= ga) return;
  }
  const uint64_t ng = (glast - gfirst_rows) / 16;
  const uint64_t soff = gfirst_rows - d0;  // source offset of the first full granule
  const uint64_t stride = nthreads;
  uint64_t g = tid;
  if (SHFL && src && ((src + soff) & 15)) {  // nthreads is a multiple of 64
    const uint64_t s0 = src + soff;
    g = copy_rows_shfl<U, NT, NTS>(gfirst_rows, s0 & ~uint64_t(15), (uint32_t)(s0 & 15), ng, g, stride);
  }
  for (; g + (U - 1) * stride < ng; g += U * stride) {
    u32x4 v[U];
#pragma unroll
    for (int k = 0; k < U; ++k)
      v[k] = src ? ld16_unaligned<NT>(src + soff + (g + k * stride) * 16) : u32x4{0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < U; ++k) st16<NTS>(gfirst_rows + (g + k * stride) * 16, v[k]);
  }
  for (; g < ng; g += stride)
    st16<NTS>(gfirst_rows + g * 16, src ? ld16_unaligned<NT>(src + soff + g * 16) : u32x4{0, 0, 0, 0});
}

// The same copy with the source read by unaligned dwordx4 loads (the hardware
// splits a load that crosses a line): one load per destination granule, no lane
// shuffle.  Rows start at a 1 KiB destination boundary as in copy_range; the
// per-wave step count is wave-uniform (a counted loop, no vmcnt(0) at a join).
// In scripts/probe_copy.hip this body moved exactly the algorithmic bytes
// (WRITE_SIZE 1.000x, FETCH_SIZE 1.02-1.03x) where copy_range's lane-shuffle
// rows wrote 1.10x and read 1.11x (profiles/r04_copy_pmc.json).
typedef unsigned int u32x4u __attribute__((ext_vector_type(4), aligned(1)));
typedef __attribute__((address_space(1))) const u32x4u g_cu32x4u;
template <bool NT>
__device__ __forceinline__ u32x4 ldu16(uint64_t a) {
  if (!lc_ok(a, 16, kSiteLdu16)) return u32x4{0, 0, 0, 0};
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<g_cu32x4u*>(a));
  return *reinterpret_cast<g_cu32x4u*>(a);
}

template <int U, bool NTL, bool NTS>
__device__ void copy_range_hw(uint64_t dst, uint64_t src, uint64_t len, uint32_t tid, uint32_t nthreads) {
  const uint64_t d0 = dst, d1 = dst + len;
  const uint64_t gfirst = (d0 + 15) & ~uint64_t(15);
  const uint64_t glast = d1 & ~uint64_t(15);
  {  // partial head and tail granules: at most 30 bytes, one per thread
    const uint64_t hend = gfirst < d1 ? gfirst : d1;
    const uint64_t tstart = glast >= gfirst ? glast : d1;
    const uint64_t nh = hend - d0, nt = d1 - tstart;
    if (tid < nh + nt) {
      const uint64_t b = tid < nh ? d0 + tid : tstart + (tid - nh);
      *reinterpret_cast<uint8_t*>(b) = src ? load_byte(src + (b - d0), kSiteCopyByte) : 0;
    }
  }
  if (glast <= gfirst) return;
  const uint64_t ga0 = (gfirst + 1023) & ~uint64_t(1023);
  const uint64_t ga = ga0 < glast ? ga0 : glast;
  if (tid < (ga - gfirst) / 16) {  // granules up to the first 1 KiB boundary, one per thread
    const uint64_t gd = gfirst + 16 * (uint64_t)tid;
    st16<NTS>(gd, src ? ldu16<NTL>(src + (gd - d0)) : u32x4{0, 0, 0, 0});
  }
  if (glast <= ga) return;
  const uint64_t ng = (glast - ga) / 16;
  const uint64_t stride = nthreads;
  const uint64_t wlast = tid | 63;                 // this wave's last thread
  const uint64_t span = wlast + (U - 1) * stride;  // its highest granule of a step
  const uint64_t steps = ng > span ? (ng - 1 - span) / (U * stride) + 1 : 0;
  const uint32_t nsteps = __builtin_amdgcn_readfirstlane((uint32_t)steps);
  uint64_t g = tid;
  if (src) {
    const uint64_t s0 = src + (ga - d0);
    for (uint32_t i = 0; i < nsteps; ++i, g += U * stride) {
      u32x4 v[U];
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = ldu16<NTL>(s0 + (g + k * stride) * 16);
#pragma unroll
      for (int k = 0; k < U; ++k) st16<NTS>(ga + (g + k * stride) * 16, v[k]);
    }
    for (; g < ng; g += stride) st16<NTS>(ga + g * 16, ldu16<NTL>(s0 + g * 16));
  } else {
    for (; g < ng; g += stride) st16<NTS>(ga + g * 16, u32x4{0, 0, 0, 0});
  }
}

}  // namespace
}  // namespace hf3fs_crc
