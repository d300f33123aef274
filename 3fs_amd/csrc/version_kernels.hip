// version_kernels.hip -- see version_kernels.h.  Like the order kernels these only move records
// and indices; the bytes are hashed and written by the update pipeline between the steps.
#include "version_kernels.h"
#include "loadcheck.h"

#include "update_plan.h"
#include "version_plan.h"

namespace hf3fs_crc {
namespace {

unsigned grid_of(uint64_t n) {
  const uint64_t want = (n + 255) / 256;
  return (unsigned)(want < 4096 ? (want ? want : 1) : 4096);
}

__device__ __forceinline__ void store_out(hf3fs_crc_update_ver* v, const VerState& s) {
  v->out_chain_ver = s.chain_ver;
  v->out_update_ver = s.update_ver;
  v->out_commit_ver = s.commit_ver;
  v->out_chunk_state = s.chunk_state;
  v->out_recycle_state = s.recycle_state;
}
__device__ __forceinline__ void store_before(hf3fs_crc_update_ver* v, const VerState& s) {
  v->chain_ver = s.chain_ver;
  v->update_ver = s.update_ver;
  v->commit_ver = s.commit_ver;
  v->meta_chunk_size = s.meta_chunk_size;
  v->chunk_state = s.chunk_state;
  v->recycle_state = s.recycle_state;
}
__device__ __forceinline__ VerState load_out(const hf3fs_crc_update_ver& v) {
  return VerState{v.out_chain_ver, v.out_update_ver, v.out_commit_ver, v.meta_chunk_size, v.out_chunk_state,
                  v.out_recycle_state};
}

struct StepArgs {
  hf3fs_crc_update_io* ios;
  hf3fs_crc_update_ver* ver;
  hf3fs_crc_update_io* round;
  const uint32_t *rank, *pred, *succ;
  uint32_t *dec, *octl, *vout, *info;
  uint64_t *vaddr, *vlen;
  uint64_t n;
  uint32_t r, max_rounds, max_len;
  int mode;
  uint8_t type;
};

__device__ __forceinline__ VerVerdict ladder_of(const hf3fs_crc_update_io& io, const hf3fs_crc_update_ver& v,
                                                const StepArgs& a, bool* verify) {
  *verify = false;
  if (io.update_type == HF3FS_UPDATE_COMMIT)
    return commit_ladder(ver_before(v), v.io_ver, v.job_chain_ver, io.flags, v.is_force != 0);
  const Eff e = derive(io, a.max_len, a.type, a.mode);
  *verify = e.ok && e.verify;
  return update_ladder(ver_before(v), v.io_ver, v.job_chain_ver, io.flags, e.ok, a.max_len);
}

// Job j enters round a.r: io and v hold its records with the before-state in place.
__device__ __forceinline__ void decide(const StepArgs& a, uint32_t j, const hf3fs_crc_update_io& io,
                                       const hf3fs_crc_update_ver& v) {
  bool verify;
  const VerVerdict d = ladder_of(io, v, a, &verify);
  store_out(&a.ver[j], d.next);  // (an admitted job's: taken back if the pipeline refuses it)
  uint64_t addr = 0, len = 0;
  if (d.where == kVerAdmit) {
    a.round[j] = io;
    a.dec[j] = 0u;
  } else {
    a.round[j] = hf3fs_crc_update_io{};
    a.ios[j].out_size = io.chunk_size;
    a.ios[j].out_checksum = io.chunk_checksum;
    a.ios[j].out_checksum_type = io.chunk_checksum_type;
    a.ios[j].checksum_case = 0;
    a.ios[j].status = d.status;
    const bool hash = d.where == kVerLate && verify;
    a.dec[j] = ((uint32_t)d.status & kDecStatusMask) | ((uint32_t)d.where << kDecWhereShift) |
               (hash ? kDecVerifyBit : 0u);
    if (hash) {
      addr = io.payload;
      len = io.length;
      atomicMax(&a.octl[kOrdVerMaxLen], io.length);
    }
  }
  a.vaddr[j] = addr;
  a.vlen[j] = len;
}

// Who writes what, on top of k_order_step's rules: dec / vaddr / vlen / round of job j and out_*
// of ver[j] are written by the thread of j's predecessor in the step before j's round (by j's own
// thread at r == 0) and read in later launches only -- but for out_* of a job that entered its
// round, which its own thread takes back in the next step when the pipeline refused it; the
// NOT_APPLIED walk of the last step therefore never reads those and runs the ladder again instead.
__global__ __launch_bounds__(256) void k_version_step(const StepArgs a) {
  const bool last = a.r == a.max_rounds;
  const uint64_t n = a.n;
  if (a.r == 0 && a.info && blockIdx.x == 0 && threadIdx.x < HF3FS_VER_INFO_WORDS) a.info[threadIdx.x] = 0u;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ri = a.rank[i];
    if (a.r > 0 && ri == a.r - 1) {
      const hf3fs_crc_update_ver v = HF3FS_LC_REC(a.ver, i, a.n);
      uint32_t size, cval;
      uint8_t ctype;
      VerState after = load_out(v);
      if (a.dec[i] == 0u) {
        const hf3fs_crc_update_io o = a.round[i];
        a.ios[i].out_size = o.out_size;
        a.ios[i].out_checksum = o.out_checksum;
        a.ios[i].out_checksum_type = o.out_checksum_type;
        a.ios[i].checksum_case = o.checksum_case;
        a.ios[i].status = o.status;
        if (o.status != HF3FS_CRC_OK) {
          after = ver_before(v);
          store_out(&a.ver[i], after);
        }
        size = o.out_size, ctype = o.out_checksum_type, cval = o.out_checksum;
      } else {  // decided in the step before its round: nothing of it is rewritten here
        const hf3fs_crc_update_io me = HF3FS_LC_REC(a.ios, i, a.n);
        size = me.chunk_size, ctype = me.chunk_checksum_type, cval = me.chunk_checksum;
      }
      const uint32_t j = a.succ[i];
      if (!last && j != kOrderNone && j < n) {
        hf3fs_crc_update_io nx = HF3FS_LC_REC(a.ios, j, a.n);
        nx.chunk_size = size;
        nx.chunk_checksum_type = ctype;
        nx.chunk_checksum = cval;
        a.ios[j].chunk_size = size;
        a.ios[j].chunk_checksum_type = ctype;
        a.ios[j].chunk_checksum = cval;
        hf3fs_crc_update_ver nv = HF3FS_LC_REC(a.ver, j, a.n);
        store_before(&nv, after);
        store_before(&a.ver[j], after);
        decide(a, j, nx, nv);
      }
    }
    if (a.r == 0) a.vout[i] = 0u;  // the hashing pass xors its parts in
    if (!last) {
      if (ri != a.r) {
        a.round[i] = hf3fs_crc_update_io{};
        if (a.r == 0) {
          a.dec[i] = 0u;
          a.vaddr[i] = 0;
          a.vlen[i] = 0;
        }
      } else if (a.r == 0) {
        decide(a, (uint32_t)i, HF3FS_LC_REC(a.ios, i, a.n), HF3FS_LC_REC(a.ver, i, a.n));
      }
    } else if (ri >= a.max_rounds) {
      uint32_t p = a.pred[i];
      for (uint64_t steps = 0; steps < n && p < n && a.rank[p] >= a.max_rounds; ++steps) p = a.pred[p];
      hf3fs_crc_update_ver mine = HF3FS_LC_REC(a.ver, i, a.n);
      VerState st = ver_before(mine);
      if (p < n) {
        const hf3fs_crc_update_ver pv = HF3FS_LC_REC(a.ver, p, a.n);
        // (input fields of ios[p] only: its thread is writing the outputs)
        uint32_t size = HF3FS_LC_REC(a.ios, p, a.n).chunk_size, cval = HF3FS_LC_REC(a.ios, p, a.n).chunk_checksum;
        uint8_t ctype = HF3FS_LC_REC(a.ios, p, a.n).chunk_checksum_type;
        const uint8_t pflags = HF3FS_LC_REC(a.ios, p, a.n).flags;
        if (a.dec[p] == 0u) {
          const hf3fs_crc_update_io o = a.round[p];
          size = o.out_size, ctype = o.out_checksum_type, cval = o.out_checksum;
          st = ver_before(pv);
          if (o.status == HF3FS_CRC_OK)
            st = update_ladder(st, pv.io_ver, pv.job_chain_ver, pflags, true, a.max_len).next;
        } else {
          st = load_out(pv);
        }
        a.ios[i].chunk_size = size;
        a.ios[i].chunk_checksum_type = ctype;
        a.ios[i].chunk_checksum = cval;
        a.ios[i].out_size = size;
        a.ios[i].out_checksum = cval;
        a.ios[i].out_checksum_type = ctype;
        store_before(&a.ver[i], st);
      }
      store_out(&a.ver[i], st);
      a.ios[i].checksum_case = 0;
      a.ios[i].status = HF3FS_CRC_NOT_APPLIED;
    }
  }
}

__global__ __launch_bounds__(256) void k_version_settle(hf3fs_crc_update_io* __restrict__ ios,
                                                        const uint32_t* __restrict__ const rank,
                                                        const uint32_t* __restrict__ const dec,
                                                        const uint32_t* __restrict__ const vout,
                                                        const uint32_t* __restrict__ const octl, const uint64_t n,
                                                        const uint32_t max_rounds, uint32_t* __restrict__ info) {
  if (info && blockIdx.x == 0 && threadIdx.x == 0) {
    info[HF3FS_VER_INFO_CHAIN_MAX] = octl[kOrdChainMax];
    info[HF3FS_VER_INFO_NOT_APPLIED] = octl[kOrdNotApplied];
  }
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n;
       i0 += (uint64_t)gridDim.x * blockDim.x) {  // wave-uniform
    const uint64_t i = i0 + lane;
    uint32_t kind = 0;  // bit per info word 2..7
    if (i < n && rank[i] < max_rounds) {
      const uint32_t d = dec[i];
      int32_t status = HF3FS_LC_REC(ios, i, n).status;
      if (((d >> kDecWhereShift) & 0xffu) == kVerLate) {
        status = (int32_t)(d & kDecStatusMask);
        if ((d & kDecVerifyBit) && vout[i] != HF3FS_LC_REC(ios, i, n).write_checksum) status = HF3FS_CRC_CHECKSUM_MISMATCH;
        ios[i].status = status;
      }
      const bool commit = HF3FS_LC_REC(ios, i, n).update_type == HF3FS_UPDATE_COMMIT;
      if (status == HF3FS_CRC_OK) {
        kind = commit ? 2u : 1u;
      } else {
        kind = 4u;
        if (status == HF3FS_CRC_CHECKSUM_MISMATCH || status == HF3FS_CRC_CHAIN_VERSION_MISMATCH ||
            status == HF3FS_CRC_CHUNK_VERSION_MISMATCH)
          kind |= 8u;
        if (commit && status == HF3FS_CRC_CHUNK_NOT_CLEAN) kind |= 16u;
        if (commit && status == HF3FS_CRC_CHUNK_STALE_COMMIT) kind |= 32u;
      }
    }
    if (info) {
#pragma unroll
      for (int w = 0; w < 6; ++w) {
        const uint32_t c = (uint32_t)__popcll(__ballot((kind >> w) & 1u));
        if (lane == 0 && c) atomicAdd(&info[HF3FS_VER_INFO_UPDATES + w], c);
      }
    }
  }
}

}  // namespace

size_t version_scratch_bytes(uint64_t n) { return n * (4 + 8 + 8 + 4) + 4 * 16; }

void version_scratch_carve(void* base, uint64_t n, VersionScratch* s) {
  uint8_t* p = (uint8_t*)base;
  auto take = [&](size_t bytes) {
    uint8_t* r = p;
    p += (bytes + 15) & ~size_t(15);
    return r;
  };
  s->vaddr = (uint64_t*)take(n * 8);
  s->vlen = (uint64_t*)take(n * 8);
  s->dec = (uint32_t*)take(n * 4);
  s->vout = (uint32_t*)take(n * 4);
}

hipError_t launch_version_step(hf3fs_crc_update_io* ios, hf3fs_crc_update_ver* ver, uint64_t n, uint32_t r,
                               uint32_t max_rounds, uint32_t max_len, uint8_t type, int mode, const OrderScratch& os,
                               const VersionScratch& vs, uint32_t* info, hipStream_t st) {
  const StepArgs a{ios,      ver,      os.round, os.rank, os.pred, os.succ,    vs.dec,  os.ctl, vs.vout,
                   info,     vs.vaddr, vs.vlen,  n,       r,       max_rounds, max_len, mode,   type};
  hipLaunchKernelGGL(k_version_step, dim3(grid_of(n)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_version_settle(hf3fs_crc_update_io* ios, uint64_t n, uint32_t max_rounds, const OrderScratch& os,
                                 const VersionScratch& vs, uint32_t* info, hipStream_t st) {
  hipLaunchKernelGGL(k_version_settle, dim3(grid_of(n)), dim3(256), 0, st, ios, os.rank, vs.dec, vs.vout, os.ctl, n,
                     max_rounds, info);
  return hipGetLastError();
}

}  // namespace hf3fs_crc
