// md5_kernels.hip -- see md5_kernels.h.  The kernels read segment records, offsets, states and the
// segments' bytes; they write the call's scratch, and d_out (FINAL) or d_state (otherwise).
//
// Who writes what (one launch per line; a word has one writer per launch):
//   prep     blocks[f] for every file: md5_call_blocks of the incoming tail and the segment lengths
//   count    count[k][s] for every bucket k and share s: files of share s in bucket k (zeros too)
//   scan     count becomes its exclusive scan in (bucket, share) order: where share s starts bucket k
//   scatter  perm: share s walks its files in ascending order, each goes to the next place of its
//            bucket's run -- every place is written, ties keep ascending file index
//   hash     d_out[16 f ..) or d_state[f] of the file of every lane
// Nothing is read that an earlier launch of the same call has not written (option poison).
#include "md5_kernels.h"

#include "loadcheck.h"
#include "md5_core.h"

namespace hf3fs_crc {
namespace {

constexpr uint32_t kPieceBytes = 256;   // staged piece of a lane's current segment: 16 granules of 16 B
constexpr uint32_t kRowGranules = 17;   // row pitch 272 B: lane l's granule q sits in 16-byte slot
                                        // (l + q) mod 16 of the 256-byte bank row, so the 16 lanes of
                                        // every ds_read_b128 group read 16 different slots

unsigned grid_of(uint64_t n) {
  const uint64_t want = (n + 255) / 256;
  return (unsigned)(want < 4096 ? (want ? want : 1) : 4096);
}

// The count and scatter passes cut the files into contiguous shares, one per wave, each a
// multiple of 64 files: share s owns [s * per, min(n, (s + 1) * per)).
struct Shares {
  uint32_t shares;
  uint64_t per;
};
__host__ __device__ inline Shares shares_of(uint64_t n) {
  const uint64_t tiles = (n + 63) / 64;
  Shares s;
  s.shares = (uint32_t)(tiles < kMd5SharesMax ? (tiles ? tiles : 1) : kMd5SharesMax);
  s.per = (tiles + s.shares - 1) / s.shares * 64;
  return s;
}

__device__ __forceinline__ uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

__global__ __launch_bounds__(256) void k_md5_prep(const hf3fs_crc_md5_seg* __restrict__ segs,
                                                  const uint64_t* __restrict__ file_off, const uint64_t n_files,
                                                  const uint64_t n_segs, const hf3fs_crc_md5_state* state,
                                                  const uint32_t flags, uint64_t* __restrict__ blocks) {
  const bool init = (flags & HF3FS_MD5_INIT) != 0, final = (flags & HF3FS_MD5_FINAL) != 0;
  for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_files;
       f += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t lo = min_u64(file_off[f], n_segs), hi = min_u64(file_off[f + 1], n_segs);
    uint64_t bytes = 0;
    for (uint64_t k = lo; k < hi; ++k) bytes += segs[k].length;
    const uint32_t tail_len = init ? 0u : (uint32_t)(state[f].total % 64);
    blocks[f] = md5_call_blocks(tail_len, bytes, final);
  }
}

// Lane l of a share's wave keeps the numbers of buckets l, l + 64, l + 128 and l + 192.
static_assert(kMd5Buckets == 4 * 64, "four buckets per lane");
struct LaneBuckets {
  uint32_t v[4];
};
__device__ __forceinline__ uint32_t pick(const LaneBuckets& b, uint32_t q) {  // q is wave-uniform
  return q == 0 ? b.v[0] : q == 1 ? b.v[1] : q == 2 ? b.v[2] : b.v[3];
}
__device__ __forceinline__ void bump(LaneBuckets& b, uint32_t q, uint32_t by) {
  b.v[0] += q == 0 ? by : 0u;
  b.v[1] += q == 1 ? by : 0u;
  b.v[2] += q == 2 ? by : 0u;
  b.v[3] += q == 3 ? by : 0u;
}

// One tile of 64 files: for every bucket among them, in the order of its first file, visit(bucket,
// lanes of the bucket).  The loop is wave-uniform.
template <class Visit>
__device__ __forceinline__ void for_each_bucket(const bool active, const uint32_t bucket, Visit visit) {
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const uint32_t k0 = (uint32_t)__shfl((int)bucket, leader, 64);
    const unsigned long long same = __ballot(active && bucket == k0);
    visit(k0, same);
    todo &= ~same;
  }
}

__global__ __launch_bounds__(64) void k_md5_count(const uint64_t* __restrict__ blocks, const uint64_t n_files,
                                                  uint32_t* __restrict__ count) {
  const Shares sh = shares_of(n_files);
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  const uint64_t lo = (uint64_t)s * sh.per, hi = min_u64(lo + sh.per, n_files);
  LaneBuckets mine = {{0, 0, 0, 0}};
  for (uint64_t i0 = lo; i0 < hi; i0 += 64) {  // wave-uniform
    const uint64_t i = i0 + lane;
    const bool active = i < hi;
    const uint32_t k = active ? md5_bucket(blocks[i]) : 0u;
    for_each_bucket(active, k, [&](uint32_t k0, unsigned long long same) {
      if (lane == (k0 & 63)) bump(mine, k0 >> 6, (uint32_t)__popcll(same));
    });
  }
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) count[(uint64_t)(q * 64 + lane) * sh.shares + s] = mine.v[q];
}

// One workgroup, thread k = bucket k: the row of bucket k is scanned by its thread, the rows'
// totals by the workgroup.
__global__ __launch_bounds__(256) void k_md5_scan(uint32_t* __restrict__ count, const uint32_t shares) {
  static_assert(kMd5Buckets == 256, "k_md5_scan: one thread per bucket");
  __shared__ uint32_t sums[256];
  uint32_t* row = count + (uint64_t)threadIdx.x * shares;
  uint32_t total = 0;
  for (uint32_t s = 0; s < shares; ++s) total += row[s];
  sums[threadIdx.x] = total;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {  // inclusive scan of the 256 row totals
    const uint32_t add = threadIdx.x >= d ? sums[threadIdx.x - d] : 0u;
    __syncthreads();
    sums[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t run = sums[threadIdx.x] - total;
  for (uint32_t s = 0; s < shares; ++s) {
    const uint32_t c = row[s];
    row[s] = run;
    run += c;
  }
}

__global__ __launch_bounds__(64) void k_md5_scatter(const uint64_t* __restrict__ blocks, const uint64_t n_files,
                                                    const uint32_t* __restrict__ count, uint32_t* __restrict__ perm) {
  const Shares sh = shares_of(n_files);
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  const uint64_t lo = (uint64_t)s * sh.per, hi = min_u64(lo + sh.per, n_files);
  LaneBuckets next;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) next.v[q] = count[(uint64_t)(q * 64 + lane) * sh.shares + s];
  for (uint64_t i0 = lo; i0 < hi; i0 += 64) {  // wave-uniform
    const uint64_t i = i0 + lane;
    const bool active = i < hi;
    const uint32_t k = active ? md5_bucket(blocks[i]) : 0u;
    for_each_bucket(active, k, [&](uint32_t k0, unsigned long long same) {
      const uint32_t base = (uint32_t)__shfl((int)pick(next, k0 >> 6), (int)(k0 & 63), 64);
      if (active && k == k0) {
        const uint64_t at = (uint64_t)base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (at < n_files) perm[at] = (uint32_t)i;  // (at < the files counted: the permutation's length)
      }
      if (lane == (k0 & 63)) bump(next, k0 >> 6, (uint32_t)__popcll(same));
    });
  }
}

// The four or five aligned 16-byte granules that hold the 64 bytes at addr, which starts r bytes
// into the first.  Every granule loaded holds a byte of the block: for r == 0 the fifth may lie
// past the segment and is not touched.
__device__ __forceinline__ void load_granules(const uint64_t addr, uint32_t g[20], uint32_t& r) {
  r = (uint32_t)addr & 15u;
  const uint4* p = (const uint4*)(uintptr_t)(addr - r);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 v = lc_ok((uint64_t)(uintptr_t)(p + q), 16, kSiteMd5Granules) ? p[q] : make_uint4(0, 0, 0, 0);
    g[4 * q] = v.x, g[4 * q + 1] = v.y, g[4 * q + 2] = v.z, g[4 * q + 3] = v.w;
  }
  uint4 last = make_uint4(0, 0, 0, 0);
  if (r && lc_ok((uint64_t)(uintptr_t)(p + 4), 16, kSiteMd5Granules)) last = p[4];
  g[16] = last.x, g[17] = last.y, g[18] = last.z, g[19] = last.w;
}

// The next block of a lane's stream straight from memory.  Inside one segment: a hole gives zeros,
// bytes come as the aligned granules the block touches.  Anywhere else (tail bytes left, a segment
// boundary within the 64 bytes, the padding): the byte-granular cursor.
__device__ __forceinline__ void block_direct(Md5Stream& s, const bool pad, uint32_t w[16]) {
  if (md5_stream_run64(s)) {
    if (s.addr == 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) w[i] = 0;
    } else {
      uint32_t g[20], r;
      load_granules(s.addr, g, r);
      md5_words_from_granules(g, r, w);
    }
    md5_stream_skip64(s);
  } else {
    md5_stream_block(s, pad, w);
  }
}

// Lane = file, wave = 64 neighbouring places of the permutation.  Without kStage every lane loads
// its own blocks (block_direct), one block ahead of the block function.  kStage: before every four blocks
// the wave stages, for each lane whose next 64 bytes lie in one segment, the aligned 256-byte piece
// around the lane's position: 16 lanes load one file's piece as one coalesced row of dwordx4, four
// files per load.  A lane then takes the whole blocks of its piece from its LDS row and everything
// else (blocks past the piece, holes, tails, boundaries, padding) through block_direct.
template <bool kStage>
__global__ __launch_bounds__(64) void k_md5_hash(const hf3fs_crc_md5_seg* __restrict__ segs,
                                                 const uint64_t* __restrict__ file_off, const uint64_t n_files,
                                                 const uint64_t n_segs, hf3fs_crc_md5_state* state, uint8_t* out,
                                                 const uint32_t flags, const uint64_t* __restrict__ blocks,
                                                 const uint32_t* __restrict__ perm) {
  __shared__ uint4 rows[kStage ? 64 * kRowGranules : 1];
  const bool init = (flags & HF3FS_MD5_INIT) != 0, final = (flags & HF3FS_MD5_FINAL) != 0;
  const uint32_t lane = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * 64 + lane;
  const bool live = i < n_files;
  uint64_t f = 0;
  if (live) {
    f = perm ? perm[i] : i;
    if (f >= n_files) f = i;  // (never: perm is a permutation)
  }
  Md5Stream s;
  uint32_t h[4];
  uint64_t left = 0;
  md5_init(h);
  if (live) {
    const uint64_t lo = min_u64(file_off[f], n_segs), hi = min_u64(file_off[f + 1], n_segs);
    md5_stream_open(s, segs, lo, hi, init ? nullptr : &state[f]);
    if (!init) {
#pragma unroll
      for (int k = 0; k < 4; ++k) h[k] = state[f].h[k];
    }
    left = blocks[f];
  } else {
    md5_stream_open(s, segs, 0, 0, nullptr);
  }

  if (!kStage) {
    // Every lane loads its own block, one block ahead: the granules of the block after this one
    // are requested before this one's 64 steps, which hide the loads' latency.
    uint32_t g[20], r = 0;
    bool ahead = false;
#pragma unroll
    for (int q = 0; q < 20; ++q) g[q] = 0;
    auto fetch = [&]() {
      ahead = left != 0 && md5_stream_run64(s) && s.addr != 0;
      if (ahead) load_granules(s.addr, g, r);
    };
    fetch();
    while (__any(left != 0)) {  // wave-uniform
      if (left) {
        uint32_t w[16];
        if (ahead) {
          md5_words_from_granules(g, r, w);
          md5_stream_skip64(s);
        } else {
          block_direct(s, final, w);
        }
        --left;
        fetch();
        md5_block(h, w);
      }
    }
  }
  while (kStage && __any(left != 0)) {  // wave-uniform
    uint32_t have = 0, r = 0;  // whole blocks of the lane's staged piece, and where the first starts
    if (kStage) {
      uint64_t piece = 0;
      uint32_t granules = 0;
      if (left && md5_stream_run64(s) && s.addr) {
        r = (uint32_t)s.addr & 15u;
        piece = s.addr - r;
        const uint64_t room = kPieceBytes - r;            // bytes of the piece from the position on
        const uint64_t usable = s.rem < room ? s.rem : room;
        granules = (uint32_t)((r + usable + 15) >> 4);    // every one holds a byte of the segment
        have = (uint32_t)(usable >> 6);
      }
      if (__any(granules != 0)) {
#pragma unroll 4
        for (uint32_t it = 0; it < 16; ++it) {
          const int j = (int)(it * 4 + (lane >> 4));
          const uint32_t c = lane & 15u;
          const uint32_t a_lo = (uint32_t)__shfl((int)(uint32_t)piece, j, 64);
          const uint32_t a_hi = (uint32_t)__shfl((int)(uint32_t)(piece >> 32), j, 64);
          const uint32_t jn = (uint32_t)__shfl((int)granules, j, 64);
          if (c < jn) {
            const uint4* p = (const uint4*)(uintptr_t)(((uint64_t)a_hi << 32) | a_lo);
            rows[(uint32_t)j * kRowGranules + c] =
                lc_ok((uint64_t)(uintptr_t)(p + c), 16, kSiteMd5StageRow) ? p[c] : make_uint4(0, 0, 0, 0);
          }
        }
      }
      __syncthreads();  // (one wave: the rows are written before any lane reads its own)
    }
#pragma unroll 1
    for (uint32_t k = 0; k < 4; ++k) {
      if (left) {
        uint32_t w[16];
        if (kStage && k < have) {
          uint32_t g[20];
#pragma unroll
          for (int q = 0; q < 5; ++q) {  // (q == 4 is only looked at for r != 0: then 4 k + 4 <= 15)
            const uint4 v = rows[lane * kRowGranules + 4 * k + q];
            g[4 * q] = v.x, g[4 * q + 1] = v.y, g[4 * q + 2] = v.z, g[4 * q + 3] = v.w;
          }
          md5_words_from_granules(g, r, w);
          md5_stream_skip64(s);
        } else {
          block_direct(s, final, w);
        }
        md5_block(h, w);
        --left;
      }
    }
    if (kStage) __syncthreads();  // (the rows are read before the next pieces overwrite them)
  }

  if (!live) return;
  if (final) {
    uint8_t* o = out + 16 * f;
    if (((uintptr_t)out & 3u) == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) ((uint32_t*)o)[k] = h[k];  // little-endian words: MD5_Final's byte order
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) o[k] = (uint8_t)(h[k >> 2] >> (8 * (k & 3)));
    }
  } else {
    uint32_t h_out[4], tail[16];
    uint64_t total = 0;
    md5_state_out(s, h, h_out, &total, tail);
    hf3fs_crc_md5_state* st = &state[f];
#pragma unroll
    for (int k = 0; k < 4; ++k) st->h[k] = h_out[k];
    st->total = total;
    uint32_t* tw = (uint32_t*)st->tail;  // (offset 24 of an 8-byte aligned record)
#pragma unroll
    for (int k = 0; k < 16; ++k) tw[k] = tail[k];
    st->reserved = 0;
  }
}

size_t round16(size_t bytes) { return (bytes + 15) & ~size_t(15); }

}  // namespace

size_t md5_scratch_bytes(uint64_t n_files) {
  return round16(n_files * 8) + round16(n_files * 4) + round16((size_t)kMd5Buckets * shares_of(n_files).shares * 4);
}

void md5_scratch_carve(void* base, uint64_t n_files, Md5Scratch* s) {
  uint8_t* p = (uint8_t*)base;
  auto take = [&](size_t bytes) {
    uint8_t* r = p;
    p += round16(bytes);
    return r;
  };
  s->shares = shares_of(n_files).shares;
  s->blocks = (uint64_t*)take(n_files * 8);
  s->perm = (uint32_t*)take(n_files * 4);
  s->count = (uint32_t*)take((size_t)kMd5Buckets * s->shares * 4);
}

hipError_t launch_md5_batch(const hf3fs_crc_md5_seg* segs, const uint64_t* file_off, uint64_t n_files,
                            uint64_t n_segs, hf3fs_crc_md5_state* state, uint8_t* out, uint32_t flags, bool sort,
                            bool stage, const Md5Scratch& s, hipStream_t st) {
  hipLaunchKernelGGL(k_md5_prep, dim3(grid_of(n_files)), dim3(256), 0, st, segs, file_off, n_files, n_segs, state,
                     flags, s.blocks);
  if (sort) {
    hipLaunchKernelGGL(k_md5_count, dim3(s.shares), dim3(64), 0, st, s.blocks, n_files, s.count);
    hipLaunchKernelGGL(k_md5_scan, dim3(1), dim3(256), 0, st, s.count, s.shares);
    hipLaunchKernelGGL(k_md5_scatter, dim3(s.shares), dim3(64), 0, st, s.blocks, n_files, s.count, s.perm);
  }
  const uint32_t* perm = sort ? s.perm : nullptr;
  const dim3 grid((unsigned)((n_files + 63) / 64));
  if (stage)
    hipLaunchKernelGGL(k_md5_hash<true>, grid, dim3(64), 0, st, segs, file_off, n_files, n_segs, state, out, flags,
                       s.blocks, perm);
  else
    hipLaunchKernelGGL(k_md5_hash<false>, grid, dim3(64), 0, st, segs, file_off, n_files, n_segs, state, out, flags,
                       s.blocks, perm);
  return hipGetLastError();
}

}  // namespace hf3fs_crc
