// client_read_kernels.hip -- see client_read_kernels.h.  The kernels read and write 40-byte IO
// records, 24-byte parent and block records, 8-byte offsets and four info words; no byte of a
// caller's data buffer is loaded here (the range kernels of crc_kernels.hip hash the prep's jobs)
// and none is stored anywhere.  Every decision is client_read_plan.h's.
//
// Who writes what:
//   prep    addr[i], len[i] for every child, maxl[0] by atomicMax
//   merge   ios[i].computed and ios[i].status (one thread per child); d_parents[p], d_blocks[p]
//           (one thread per parent); d_info by atomicAdd (zeroed before the launch)
// A child's result after the verify is a function of its input fields and its hashed value
// only, so the thread that merges a parent recomputes its children's verdicts and never reads
// another thread's stores: records are loaded through inputs_of, which leaves the output words out.
#include "client_read_kernels.h"

#include "client_read_plan.h"
#include "gf2.h"
#include "loadcheck.h"

namespace hf3fs_crc {
namespace {

unsigned grid_of(uint64_t n, unsigned per = 256) {
  const uint64_t want = (n + per - 1) / per;
  return (unsigned)(want < 4096 ? (want ? want : 1) : 4096);
}

struct GfTables {
  const DeviceTables* tabs;
  __device__ __forceinline__ uint32_t shift(uint32_t v, uint64_t nbytes, uint8_t type) const {
    const uint32_t poly = poly_of(type);
    return gf_mul(v, xpow8_bytes((int64_t)nbytes, &tabs->poly[type == kTypeCrc32 ? 1 : 0], poly), poly);
  }
};

struct Batch {
  hf3fs_crc_client_read_io* ios;
  uint64_t n_ios;
  const uint32_t* v;  // null without VERIFY
  uint8_t type;
  uint32_t max_len;
  bool verify;
};

// The input fields of record i behind HF3FS_LC_REC's index check (an index >= n is logged and
// gives a zeroed record), not the whole record: other threads of the merge launch store
// `computed` and `status`, so no thread of it loads those two words.
__device__ __forceinline__ hf3fs_crc_client_read_io inputs_of(const hf3fs_crc_client_read_io* ios, uint64_t i,
                                                              uint64_t n) {
  hf3fs_crc_client_read_io io{};
  if (!lc_desc_ok(i, n)) return io;
  const hf3fs_crc_client_read_io* p = ios + i;
  io.data = p->data;
  io.length = p->length;
  io.read_len = p->read_len;
  io.status_in = p->status_in;
  io.checksum = p->checksum;
  io.checksum_type = p->checksum_type;
  return io;
}

__device__ __forceinline__ ClientChild child_at(const Batch& b, uint64_t i) {
  const hf3fs_crc_client_read_io io = inputs_of(b.ios, i, b.n_ios);
  const uint32_t hashed = client_read_hashes(io, b.type, b.max_len, b.verify) ? b.v[i] : 0u;
  return client_read_verdict(io, hashed, b.type, b.max_len, b.verify);
}

__device__ __forceinline__ void store_verdict(const Batch& b, uint64_t i, const ClientChild& c) {
  b.ios[i].computed = c.computed;
  b.ios[i].status = c.status;
}

// Parent p's children [lo, hi) of the batch: the caller's offsets, clamped.
__device__ __forceinline__ void children_of(const uint64_t* parent_off, uint64_t p, uint64_t n_parents, uint64_t n_ios,
                                            uint64_t* lo, uint64_t* hi) {
  uint64_t b1 = HF3FS_LC_REC(parent_off, p + 1, n_parents + 1);
  uint64_t b0 = HF3FS_LC_REC(parent_off, p, n_parents + 1);
  if (b1 > n_ios) b1 = n_ios;
  if (b0 > b1) b0 = b1;
  *lo = b0;
  *hi = b1;
}

struct Counts {
  uint32_t bad_children, bad_parents, hard_parents;
};

__device__ __forceinline__ void count_parent(Counts& n, const ClientParent& p) {
  n.bad_parents += p.status != 0 ? 1u : 0u;
  n.hard_parents += p.status != 0 && p.status != kClientChunkNotFound ? 1u : 0u;
}

__device__ __forceinline__ ClientSum shfl_down_sum(const ClientSum& s, int d) {
  ClientSum r;
  r.len[0] = __shfl_down(s.len[0], d, 64);
  r.len[1] = __shfl_down(s.len[1], d, 64);
  r.v[0] = __shfl_down(s.v[0], d, 64);
  r.v[1] = __shfl_down(s.v[1], d, 64);
  r.nv = __shfl_down(s.nv, d, 64);
  r.fix = __shfl_down(s.fix, d, 64);
  r.fail = __shfl_down(s.fail, d, 64);
  r.length = __shfl_down(s.length, d, 64);
  r.block_len = __shfl_down(s.block_len, d, 64);
  r.has = __shfl_down(s.has, d, 64);
  return r;
}

__global__ __launch_bounds__(256) void k_client_read_prep(const hf3fs_crc_client_read_io* __restrict__ ios,
                                                          const uint64_t n_ios, const uint8_t type,
                                                          const uint32_t max_len, uint64_t* __restrict__ addr,
                                                          uint64_t* __restrict__ len, uint32_t* __restrict__ maxl) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ios;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const hf3fs_crc_client_read_io io = inputs_of(ios, i, n_ios);
    const bool need = client_read_hashes(io, type, max_len, true);
    addr[i] = need ? io.data : 0;
    len[i] = need ? io.read_len : 0;
    if (need) atomicMax(maxl, io.read_len);
  }
}

// WAVE = false: one lane per parent, the reference's loop in registers (without offsets the
// lane's one child is its parent, and verdict and merge share the record load).
// WAVE = true: one wave per parent; lane l folds its contiguous run of the children, then the
// ordered tree of digest_kernels.hip's k_digest_wave runs over the wave in registers.
template <bool WAVE>
__global__ __launch_bounds__(256) void k_client_read_merge(const Batch b, const uint64_t* __restrict__ parent_off,
                                                           const uint64_t n_parents,
                                                           hf3fs_crc_client_read_result* __restrict__ parents,
                                                           hf3fs_crc_block_digest* __restrict__ blocks,
                                                           uint32_t* __restrict__ info,
                                                           const DeviceTables* __restrict__ tabs) {
  __shared__ uint32_t total[3];
  if (threadIdx.x < 3) total[threadIdx.x] = 0;
  __syncthreads();
  const GfTables gf{tabs};
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, threads = (uint64_t)gridDim.x * blockDim.x;
  Counts n{0, 0, 0};
  if (!parent_off) {  // (n_parents == n_ios)
    for (uint64_t i = tid; i < b.n_ios; i += threads) {
      const ClientChild c = child_at(b, i);
      store_verdict(b, i, c);
      n.bad_children += c.status != 0 ? 1u : 0u;
      ClientSeq s = client_seq_begin();
      client_seq_step(s, c, 0u, gf);
      client_parent_emit(s.p, i, parents ? parents + i : nullptr, blocks ? blocks + i : nullptr);
      count_parent(n, s.p);
    }
  } else {
    for (uint64_t i = tid; i < b.n_ios; i += threads) {
      const ClientChild c = child_at(b, i);
      store_verdict(b, i, c);
      n.bad_children += c.status != 0 ? 1u : 0u;
    }
    if (!WAVE) {  // (verify only, both outputs null, still merges: d_info counts the parents)
      for (uint64_t p = tid; p < n_parents; p += threads) {
        uint64_t lo, hi;
        children_of(parent_off, p, n_parents, b.n_ios, &lo, &hi);
        ClientSeq s = client_seq_begin();
        for (uint64_t i = lo; i < hi; ++i) client_seq_step(s, child_at(b, i), (uint32_t)(i - lo), gf);
        client_parent_emit(s.p, lo, parents ? parents + p : nullptr, blocks ? blocks + p : nullptr);
        count_parent(n, s.p);
      }
    } else {
      const uint32_t lane = threadIdx.x & 63;
      for (uint64_t p = tid >> 6; p < n_parents; p += threads >> 6) {  // wave-uniform
        uint64_t lo, hi;
        children_of(parent_off, p, n_parents, b.n_ios, &lo, &hi);
        const uint64_t k = hi - lo, run = (k + 63) / 64;
        ClientSum acc = client_sum_identity();
        for (uint64_t j = lane * run, e = j + run < k ? j + run : k; j < e; ++j)
          acc = client_sum_join(acc, client_sum_of(child_at(b, lo + j), (uint32_t)j), gf);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {  // ordered: lane l joins lane l + d's summary on its right
          const ClientSum o = shfl_down_sum(acc, d);
          if ((lane & (2 * d - 1)) == 0) acc = client_sum_join(acc, o, gf);
        }
        if (lane == 0) {
          const ClientParent r =
              client_sum_finish(acc, k, [&](uint32_t j) { return child_at(b, lo + j); }, gf);
          client_parent_emit(r, lo, parents ? parents + p : nullptr, blocks ? blocks + p : nullptr);
          count_parent(n, r);
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    n.bad_children += __shfl_xor(n.bad_children, d, 64);
    n.bad_parents += __shfl_xor(n.bad_parents, d, 64);
    n.hard_parents += __shfl_xor(n.hard_parents, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n.bad_children) atomicAdd(&total[0], n.bad_children);
    if (n.bad_parents) atomicAdd(&total[1], n.bad_parents);
    if (n.hard_parents) atomicAdd(&total[2], n.hard_parents);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (total[0]) atomicAdd(&info[HF3FS_CLIENT_READ_INFO_BAD_CHILDREN], total[0]);
    if (total[1]) atomicAdd(&info[HF3FS_CLIENT_READ_INFO_BAD_PARENTS], total[1]);
    if (total[2]) atomicAdd(&info[HF3FS_CLIENT_READ_INFO_HARD_PARENTS], total[2]);
  }
}

}  // namespace

hipError_t launch_client_read_prep(const hf3fs_crc_client_read_io* ios, uint64_t n_ios, uint8_t type, uint32_t max_len,
                                   uint64_t* addr, uint64_t* len, uint32_t* maxl, hipStream_t st) {
  hipLaunchKernelGGL(k_client_read_prep, dim3(grid_of(n_ios)), dim3(256), 0, st, ios, n_ios, type, max_len, addr, len,
                     maxl);
  return hipGetLastError();
}

hipError_t launch_client_read_merge(hf3fs_crc_client_read_io* ios, uint64_t n_ios, const uint64_t* parent_off,
                                    uint64_t n_parents, uint8_t type, uint32_t max_len, bool verify, bool wave,
                                    const uint32_t* v, hf3fs_crc_client_read_result* parents,
                                    hf3fs_crc_block_digest* blocks, uint32_t* info, const DeviceTables* tabs,
                                    hipStream_t st) {
  const Batch b{ios, n_ios, v, type, max_len, verify};
  if (wave && parent_off) {
    // a wave per parent, four per workgroup; the children's verdicts stride over the same grid
    const unsigned g = grid_of(n_parents, 4), gc = grid_of(n_ios);
    hipLaunchKernelGGL(k_client_read_merge<true>, dim3(g > gc ? g : gc), dim3(256), 0, st, b, parent_off, n_parents,
                       parents, blocks, info, tabs);
  } else {
    hipLaunchKernelGGL(k_client_read_merge<false>, dim3(grid_of(n_ios > n_parents ? n_ios : n_parents)), dim3(256), 0,
                       st, b, parent_off, n_parents, parents, blocks, info, tabs);
  }
  return hipGetLastError();
}

}  // namespace hf3fs_crc
