// order_kernels.hip -- see order_kernels.h.  These kernels only move 56-byte records and 4-byte
// indices; the bytes are hashed and written by the update pipeline between the steps.
#include "order_kernels.h"
#include "loadcheck.h"

namespace hf3fs_crc {
namespace {

unsigned grid_of(uint64_t n) {
  const uint64_t want = (n + 255) / 256;
  return (unsigned)(want < 4096 ? (want ? want : 1) : 4096);
}

// Every table word and the control words: the call reads none of them before this launch wrote it.
__global__ __launch_bounds__(256) void k_order_clear(unsigned long long* __restrict__ keys,
                                                     uint32_t* __restrict__ head, uint32_t* __restrict__ ctl,
                                                     const uint32_t table) {
  if (blockIdx.x == 0 && threadIdx.x < kOrdWords) ctl[threadIdx.x] = 0u;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < table; i += (uint64_t)gridDim.x * blockDim.x) {
    keys[i] = 0ull;
    head[i] = kOrderNone;
  }
}

// IO i claims (or finds) the slot of its chunk address and pushes itself onto the slot's list.
// Fibonacci hashing on the 64-bit address: chunks at consecutive small strides spread over the
// table.  The table holds >= 2 n slots for <= n keys, so a probe sequence always ends.
__global__ __launch_bounds__(256) void k_order_insert(const hf3fs_crc_update_io* __restrict__ const ios,
                                                      const uint64_t n, unsigned long long* __restrict__ keys,
                                                      uint32_t* __restrict__ head, uint32_t* __restrict__ next,
                                                      uint32_t* __restrict__ slot, const uint32_t table,
                                                      const uint32_t shift) {
  const uint32_t mask = table - 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = HF3FS_LC_REC(ios, i, n).chunk;
    uint32_t at = kOrderNone, link = kOrderNone;
    if (key) {  // (chunk 0 stays a chain of its own: rank 0, it fails or not as in update_batch)
      uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> shift) & mask;
      for (uint32_t probe = 0; probe < table; ++probe, h = (h + 1) & mask) {
        const unsigned long long prev = atomicCAS(&keys[h], 0ull, key);
        if (prev == 0ull || prev == key) {
          at = h;
          break;
        }
      }
      if (at != kOrderNone) link = atomicExch(&head[at], (uint32_t)i);
    }
    slot[i] = at;
    next[i] = link;
  }
}

// rank / pred / succ of every IO from its chunk's list.  The list's order depends on which
// atomicExch came first; counts, a maximum and a minimum over it do not: the plan is the same
// for every run.  A walk is bounded by n steps (a list holds every IO at most once).
__global__ __launch_bounds__(256) void k_order_rank(const uint32_t* __restrict__ const slot,
                                                    const uint32_t* __restrict__ const head,
                                                    const uint32_t* __restrict__ const next,
                                                    uint32_t* __restrict__ rank, uint32_t* __restrict__ pred,
                                                    uint32_t* __restrict__ succ, uint32_t* __restrict__ ctl,
                                                    const uint64_t n, const uint32_t max_rounds) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n;
       i0 += (uint64_t)gridDim.x * blockDim.x) {  // wave-uniform
    const uint64_t i = i0 + lane;
    uint32_t total = 0, late = 0;
    if (i < n) {
      const uint32_t s = slot[i];
      uint32_t r = 0, p = kOrderNone, q = kOrderNone;
      total = 1;
      if (s != kOrderNone) {
        total = 0;
        uint32_t j = head[s];
        for (uint64_t steps = 0; j != kOrderNone && j < n && steps < n; ++steps) {
          ++total;
          if (j < i) {
            ++r;
            if (p == kOrderNone || j > p) p = j;
          } else if (j > i && j < q) {
            q = j;
          }
          j = next[j];
        }
      }
      rank[i] = r;
      pred[i] = p;
      succ[i] = q;
      late = r >= max_rounds ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      total = max(total, (uint32_t)__shfl_xor(total, d, 64));
      late += __shfl_xor(late, d, 64);
    }
    if (lane == 0) {
      atomicMax(&ctl[kOrdChainMax], total);
      if (late) atomicAdd(&ctl[kOrdNotApplied], late);
    }
  }
}

// The step before round r.  Who writes what (no word has two writers, no reader races a writer):
//   IO i of rank r - 1 (it was active in the round that just ran): its output fields and status
//     go from round[i] to ios[i]; the state they describe -- after a failed IO that is the state
//     it started from, the pipeline leaves out_* = the input fields then -- goes into the input
//     fields of ios[succ] and, with the rest of that record, into round[succ]: succ has rank r.
//   IO i of rank r == 0: round[i] = ios[i].
//   every IO of another rank than r: round[i] = a no-op record (all zero: update_type 0).
//   r == max_rounds (last launch): an IO of rank >= max_rounds walks back to its chunk's last
//     applied IO and takes that state into its input and output fields, NOT_APPLIED, case 0.
__global__ __launch_bounds__(256) void k_order_step(hf3fs_crc_update_io* __restrict__ ios,
                                                    hf3fs_crc_update_io* __restrict__ round,
                                                    const uint32_t* __restrict__ const rank,
                                                    const uint32_t* __restrict__ const pred,
                                                    const uint32_t* __restrict__ const succ,
                                                    const uint32_t* __restrict__ const ctl, const uint64_t n,
                                                    const uint32_t r, const uint32_t max_rounds,
                                                    uint32_t* __restrict__ info) {
  const bool last = r == max_rounds;
  if (last && info && blockIdx.x == 0 && threadIdx.x == 0) {
    info[0] = ctl[kOrdChainMax];
    info[1] = ctl[kOrdNotApplied];
  }
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ri = rank[i];
    if (r > 0 && ri == r - 1) {
      const hf3fs_crc_update_io o = round[i];
      ios[i].out_size = o.out_size;
      ios[i].out_checksum = o.out_checksum;
      ios[i].out_checksum_type = o.out_checksum_type;
      ios[i].checksum_case = o.checksum_case;
      ios[i].status = o.status;
      const uint32_t j = succ[i];
      if (!last && j != kOrderNone && j < n) {
        hf3fs_crc_update_io nx = HF3FS_LC_REC(ios, j, n);
        nx.chunk_size = o.out_size;
        nx.chunk_checksum_type = o.out_checksum_type;
        nx.chunk_checksum = o.out_checksum;
        ios[j].chunk_size = nx.chunk_size;
        ios[j].chunk_checksum_type = nx.chunk_checksum_type;
        ios[j].chunk_checksum = nx.chunk_checksum;
        round[j] = nx;
      }
    }
    if (!last) {
      if (ri != r)
        round[i] = hf3fs_crc_update_io{};
      else if (r == 0)
        round[i] = HF3FS_LC_REC(ios, i, n);
    } else if (ri >= max_rounds) {
      uint32_t p = pred[i];
      for (uint64_t steps = 0; steps < n && p < n && rank[p] >= max_rounds; ++steps) p = pred[p];
      if (p < n) {
        const hf3fs_crc_update_io o = round[p];
        ios[i].chunk_size = o.out_size;
        ios[i].chunk_checksum_type = o.out_checksum_type;
        ios[i].chunk_checksum = o.out_checksum;
        ios[i].out_size = o.out_size;
        ios[i].out_checksum = o.out_checksum;
        ios[i].out_checksum_type = o.out_checksum_type;
      }
      ios[i].checksum_case = 0;
      ios[i].status = HF3FS_CRC_NOT_APPLIED;
    }
  }
}

}  // namespace

size_t order_scratch_bytes(uint64_t n) {
  uint64_t table = 2;
  while (table < 2 * n) table <<= 1;
  // ctl, keys, head, five index arrays, the round array; 16-byte rounding of each piece
  return 64 + table * (8 + 4) + n * 5 * 4 + n * sizeof(hf3fs_crc_update_io) + 10 * 16;
}

void order_scratch_carve(void* base, uint64_t n, OrderScratch* s) {
  uint64_t table = 2;
  while (table < 2 * n) table <<= 1;
  uint8_t* p = (uint8_t*)base;
  auto take = [&](size_t bytes) {
    uint8_t* r = p;
    p += (bytes + 15) & ~size_t(15);
    return r;
  };
  s->ctl = (uint32_t*)take(64);
  s->keys = (unsigned long long*)take(table * 8);
  s->head = (uint32_t*)take(table * 4);
  s->next = (uint32_t*)take(n * 4);
  s->slot = (uint32_t*)take(n * 4);
  s->rank = (uint32_t*)take(n * 4);
  s->pred = (uint32_t*)take(n * 4);
  s->succ = (uint32_t*)take(n * 4);
  s->round = (hf3fs_crc_update_io*)take(n * sizeof(hf3fs_crc_update_io));
  s->table = (uint32_t)table;
}

hipError_t launch_order_plan(const hf3fs_crc_update_io* ios, uint64_t n, uint32_t max_rounds, const OrderScratch& s,
                             hipStream_t st) {
  uint32_t log2 = 0;
  while ((1u << log2) < s.table) ++log2;
  hipLaunchKernelGGL(k_order_clear, dim3(grid_of(s.table)), dim3(256), 0, st, s.keys, s.head, s.ctl, s.table);
  hipLaunchKernelGGL(k_order_insert, dim3(grid_of(n)), dim3(256), 0, st, ios, n, s.keys, s.head, s.next, s.slot,
                     s.table, 64u - log2);
  hipLaunchKernelGGL(k_order_rank, dim3(grid_of(n)), dim3(256), 0, st, s.slot, s.head, s.next, s.rank, s.pred, s.succ,
                     s.ctl, n, max_rounds);
  return hipGetLastError();
}

hipError_t launch_order_step(hf3fs_crc_update_io* ios, uint64_t n, uint32_t r, uint32_t max_rounds,
                             const OrderScratch& s, uint32_t* info, hipStream_t st) {
  hipLaunchKernelGGL(k_order_step, dim3(grid_of(n)), dim3(256), 0, st, ios, s.round, s.rank, s.pred, s.succ, s.ctl, n,
                     r, max_rounds, info);
  return hipGetLastError();
}

}  // namespace hf3fs_crc
