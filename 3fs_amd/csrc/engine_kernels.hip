// engine_kernels.hip -- see engine_kernels.h.  Like the order and version kernels these only move
// records and indices; the bytes are hashed and written by the update pipeline between the steps.
#include "engine_kernels.h"
#include "loadcheck.h"

#include "engine_plan.h"
#include "update_plan.h"

namespace hf3fs_crc {
namespace {

unsigned grid_of(uint64_t n) {
  const uint64_t want = (n + 255) / 256;
  return (unsigned)(want < 4096 ? (want ? want : 1) : 4096);
}

// The state a job starts from: the before-fields of its job record and the committed
// {size, checksum} of its IO record.
__device__ __forceinline__ EngState load_before(const hf3fs_crc_update_io& io, const hf3fs_crc_engine_job& j) {
  return EngState{j.addr,   io.chunk_size, io.chunk_checksum, j.chain_ver,   j.chunk_ver, io.chunk_checksum_type,
                  j.w_addr, j.w_len,       j.w_checksum,      j.w_chain_ver, j.w_chunk_ver};
}
// The state a DECIDED job left: out_* of its job record and the outputs of its IO record.
__device__ __forceinline__ EngState load_out(const hf3fs_crc_update_io& io, const hf3fs_crc_engine_job& j) {
  return EngState{j.out_addr,   io.out_size, io.out_checksum, j.out_chain_ver,   j.out_chunk_ver, io.out_checksum_type,
                  j.out_w_addr, j.out_w_len, j.out_w_checksum, j.out_w_chain_ver, j.out_w_chunk_ver};
}
__device__ __forceinline__ void store_before(hf3fs_crc_update_io* io, hf3fs_crc_engine_job* j, const EngState& s) {
  io->chunk_size = s.size;
  io->chunk_checksum_type = s.ctype;
  io->chunk_checksum = s.checksum;
  j->addr = s.addr;
  j->chain_ver = s.chain_ver;
  j->chunk_ver = s.chunk_ver;
  j->w_addr = s.w_addr;
  j->w_len = s.w_len;
  j->w_checksum = s.w_checksum;
  j->w_chain_ver = s.w_chain_ver;
  j->w_chunk_ver = s.w_chunk_ver;
}
__device__ __forceinline__ void store_out(hf3fs_crc_engine_job* j, const EngState& s) {
  j->out_addr = s.addr;
  j->out_chain_ver = s.chain_ver;
  j->out_chunk_ver = s.chunk_ver;
  j->out_w_addr = s.w_addr;
  j->out_w_len = s.w_len;
  j->out_w_checksum = s.w_checksum;
  j->out_w_chain_ver = s.w_chain_ver;
  j->out_w_chunk_ver = s.w_chunk_ver;
}
// The IO record's outputs of a job that did not go through the pipeline: the committed state
// after it (a refusal: the input state repeated), case 0.
__device__ __forceinline__ void store_io_out(hf3fs_crc_update_io* io, const EngState& s, int32_t status) {
  io->out_size = s.size;
  io->out_checksum = s.checksum;
  io->out_checksum_type = s.ctype;
  io->checksum_case = 0;
  io->status = status;
}

struct StepArgs {
  hf3fs_crc_update_io* ios;
  hf3fs_crc_engine_job* jobs;
  hf3fs_crc_update_io* round;
  const uint32_t *rank, *pred, *succ;
  uint32_t *dec, *octl, *vout, *info;
  uint64_t *vaddr, *vlen, *rdst;
  uint64_t n;
  uint32_t r, max_rounds, max_len;
  int mode;
};

__device__ __forceinline__ EngVerdict decision_of(const hf3fs_crc_update_io& io, const hf3fs_crc_engine_job& j,
                                                  const StepArgs& a, bool* verify) {
  *verify = false;
  const EngState s = load_before(io, j);
  if (io.update_type == HF3FS_UPDATE_COMMIT) return engine_commit(s, j.job_chain_ver);
  const Eff e = derive(io, a.max_len, kTypeCrc32c, a.mode);
  *verify = e.ok && e.verify;
  return engine_update(s, j.io_ver, j.job_chain_ver, j.dst, io.update_type, io.flags, io.offset, io.length, e.ok);
}

// Job j enters round a.r: io and job hold its records with the before-state in place.
__device__ __forceinline__ void decide(const StepArgs& a, uint32_t j, const hf3fs_crc_update_io& io,
                                       const hf3fs_crc_engine_job& job) {
  bool verify;
  const EngVerdict d = decision_of(io, job, a, &verify);
  // (an admitted job's out_*: w_len / w_checksum are set, or all of it taken back, by its own thread next step)
  store_out(&a.jobs[j], d.next);
  a.jobs[j].out_cow = d.where == kEngAdmit ? d.cow : 0;
  a.jobs[j].detail = d.detail;
  uint64_t addr = 0, len = 0, dst = 0;
  if (d.where == kEngAdmit) {
    hf3fs_crc_update_io rec = io;
    rec.chunk = job.addr;  // `chunk` of the caller's record is a key only
    a.round[j] = rec;
    a.dec[j] = 0u;
    dst = d.cow ? job.dst : 0;
  } else {
    a.round[j] = hf3fs_crc_update_io{};
    store_io_out(&a.ios[j], d.next, d.status);
    const bool hash = d.where == kEngLate && verify;
    a.dec[j] = ((uint32_t)d.status & kDecStatusMask) | ((uint32_t)d.where << kDecWhereShift) |
               (hash ? kDecVerifyBit : 0u);
    if (hash) {
      addr = io.payload;
      len = io.length;
      atomicMax(&a.octl[kOrdVerMaxLen], io.length);
    }
  }
  a.rdst[j] = dst;
  a.vaddr[j] = addr;
  a.vlen[j] = len;
}

// Who writes what follows version_kernels.hip:89-93 on top of k_order_step's rules: dec / vaddr /
// vlen / rdst / round of job j, the before-fields of both its records and out_*, out_cow, detail
// of jobs[j] are written by the thread of j's predecessor in the step before j's round (by j's own
// thread at r == 0) and read in later launches only -- but for out_* / out_cow of a job that
// entered its round, which its own thread completes (w_len, w_checksum) or takes back (the
// pipeline refused it) in the next step, together with the outputs of ios[j].  The NOT_APPLIED
// walk of the last step therefore never reads those words of an admitted job: it takes the job's
// before-fields and the round array and runs the decision again.
__global__ __launch_bounds__(256) void k_engine_step(const StepArgs a) {
  const bool last = a.r == a.max_rounds;
  const uint64_t n = a.n;
  if (a.r == 0 && a.info && blockIdx.x == 0 && threadIdx.x < HF3FS_ENGINE_INFO_WORDS) a.info[threadIdx.x] = 0u;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t ri = a.rank[i];
    if (a.r > 0 && ri == a.r - 1) {
      const hf3fs_crc_update_io me = HF3FS_LC_REC(a.ios, i, a.n);
      const hf3fs_crc_engine_job job = HF3FS_LC_REC(a.jobs, i, a.n);
      EngState after;
      if (a.dec[i] == 0u) {
        const hf3fs_crc_update_io o = a.round[i];
        a.ios[i].out_size = o.out_size;
        a.ios[i].out_checksum = o.out_checksum;
        a.ios[i].out_checksum_type = o.out_checksum_type;
        a.ios[i].checksum_case = o.checksum_case;
        a.ios[i].status = o.status;
        if (o.status == HF3FS_CRC_OK) {
          after = load_before(me, job);  // the committed part: an update does not change it
          after.w_addr = job.out_w_addr;
          after.w_len = o.out_size;
          after.w_checksum = o.out_checksum;
          after.w_chain_ver = job.out_w_chain_ver;
          after.w_chunk_ver = job.out_w_chunk_ver;
          a.jobs[i].out_w_len = o.out_size;
          a.jobs[i].out_w_checksum = o.out_checksum;
        } else {
          after = load_before(me, job);
          store_out(&a.jobs[i], after);
          a.jobs[i].out_cow = 0;
        }
      } else {  // decided in the step before its round: nothing of it is rewritten here
        after = load_out(me, job);
      }
      const uint32_t j = a.succ[i];
      if (!last && j != kOrderNone && j < n) {
        hf3fs_crc_update_io nx = HF3FS_LC_REC(a.ios, j, a.n);
        hf3fs_crc_engine_job nj = HF3FS_LC_REC(a.jobs, j, a.n);
        store_before(&nx, &nj, after);
        store_before(&a.ios[j], &a.jobs[j], after);
        decide(a, j, nx, nj);
      }
    }
    if (a.r == 0) a.vout[i] = 0u;  // the hashing pass xors its parts in
    if (!last) {
      if (ri != a.r) {
        a.round[i] = hf3fs_crc_update_io{};
        a.rdst[i] = 0;
        if (a.r == 0) {
          a.dec[i] = 0u;
          a.vaddr[i] = 0;
          a.vlen[i] = 0;
        }
      } else if (a.r == 0) {
        decide(a, (uint32_t)i, HF3FS_LC_REC(a.ios, i, a.n), HF3FS_LC_REC(a.jobs, i, a.n));
      }
    } else if (ri >= a.max_rounds) {
      uint32_t p = a.pred[i];
      for (uint64_t steps = 0; steps < n && p < n && a.rank[p] >= a.max_rounds; ++steps) p = a.pred[p];
      EngState st = load_before(HF3FS_LC_REC(a.ios, i, a.n), HF3FS_LC_REC(a.jobs, i, a.n));
      if (p < n) {
        // input fields and before-fields of p only: its thread is writing the outputs
        hf3fs_crc_update_io pio{};
        pio.chunk_size = HF3FS_LC_REC(a.ios, p, a.n).chunk_size;
        pio.chunk_checksum_type = HF3FS_LC_REC(a.ios, p, a.n).chunk_checksum_type;
        pio.chunk_checksum = HF3FS_LC_REC(a.ios, p, a.n).chunk_checksum;
        hf3fs_crc_engine_job pj{};
        pj.addr = HF3FS_LC_REC(a.jobs, p, a.n).addr;
        pj.chain_ver = HF3FS_LC_REC(a.jobs, p, a.n).chain_ver;
        pj.chunk_ver = HF3FS_LC_REC(a.jobs, p, a.n).chunk_ver;
        pj.w_addr = HF3FS_LC_REC(a.jobs, p, a.n).w_addr;
        pj.w_len = HF3FS_LC_REC(a.jobs, p, a.n).w_len;
        pj.w_checksum = HF3FS_LC_REC(a.jobs, p, a.n).w_checksum;
        pj.w_chain_ver = HF3FS_LC_REC(a.jobs, p, a.n).w_chain_ver;
        pj.w_chunk_ver = HF3FS_LC_REC(a.jobs, p, a.n).w_chunk_ver;
        if (a.dec[p] == 0u) {
          st = load_before(pio, pj);
          const hf3fs_crc_update_io o = a.round[p];
          if (o.status == HF3FS_CRC_OK) {
            const EngVerdict d =
                engine_update(st, HF3FS_LC_REC(a.jobs, p, a.n).io_ver, HF3FS_LC_REC(a.jobs, p, a.n).job_chain_ver, HF3FS_LC_REC(a.jobs, p, a.n).dst, HF3FS_LC_REC(a.ios, p, a.n).update_type,
                              HF3FS_LC_REC(a.ios, p, a.n).flags, HF3FS_LC_REC(a.ios, p, a.n).offset, HF3FS_LC_REC(a.ios, p, a.n).length, true);
            st = eng_written(d.next, o.out_size, o.out_checksum);
          }
        } else {
          st = load_out(HF3FS_LC_REC(a.ios, p, a.n), HF3FS_LC_REC(a.jobs, p, a.n));
        }
        store_before(&a.ios[i], &a.jobs[i], st);
      }
      store_out(&a.jobs[i], st);
      a.jobs[i].out_cow = 0;
      a.jobs[i].detail = HF3FS_ENGINE_DETAIL_NONE;
      store_io_out(&a.ios[i], st, HF3FS_CRC_NOT_APPLIED);
    }
  }
}

__global__ __launch_bounds__(256) void k_engine_settle(hf3fs_crc_update_io* __restrict__ ios,
                                                       hf3fs_crc_engine_job* __restrict__ jobs,
                                                       const uint32_t* __restrict__ const rank,
                                                       const uint32_t* __restrict__ const dec,
                                                       const uint32_t* __restrict__ const vout,
                                                       const uint32_t* __restrict__ const octl, const uint64_t n,
                                                       const uint32_t max_rounds, uint32_t* __restrict__ info) {
  if (info && blockIdx.x == 0 && threadIdx.x == 0) {
    info[HF3FS_ENGINE_INFO_CHAIN_MAX] = octl[kOrdChainMax];
    info[HF3FS_ENGINE_INFO_NOT_APPLIED] = octl[kOrdNotApplied];
  }
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n;
       i0 += (uint64_t)gridDim.x * blockDim.x) {  // wave-uniform: every lane reaches the ballots
    const uint64_t i = i0 + lane;
    uint32_t kind = 0;  // bit per info word 2..7
    if (i < n && rank[i] < max_rounds) {
      const uint32_t d = dec[i];
      int32_t status = HF3FS_LC_REC(ios, i, n).status;
      uint8_t detail = HF3FS_LC_REC(jobs, i, n).detail;
      if (((d >> kDecWhereShift) & 0xffu) == kEngLate) {
        status = (int32_t)(d & kDecStatusMask);
        if ((d & kDecVerifyBit) && vout[i] != HF3FS_LC_REC(ios, i, n).write_checksum) {
          status = HF3FS_CRC_CHECKSUM_MISMATCH;
          detail = HF3FS_ENGINE_DETAIL_NONE;
          jobs[i].detail = detail;
        }
        ios[i].status = status;
      }
      const bool commit = HF3FS_LC_REC(ios, i, n).update_type == HF3FS_UPDATE_COMMIT;
      if (status == HF3FS_CRC_OK) {
        kind = commit ? 2u : 1u;
        if (!commit) kind |= HF3FS_LC_REC(jobs, i, n).out_cow ? 8u : 16u;
      } else {
        kind = 4u;
        if (status == HF3FS_CRC_INVALID_ARG && detail == HF3FS_ENGINE_DETAIL_IN_WRITING) kind |= 32u;
      }
    }
    if (info) {
#pragma unroll
      for (int w = 0; w < 6; ++w) {
        const uint32_t c = (uint32_t)__popcll(__ballot((kind >> w) & 1u));
        if (lane == 0 && c) atomicAdd(&info[HF3FS_ENGINE_INFO_UPDATES + w], c);
      }
    }
  }
}

}  // namespace

size_t engine_scratch_bytes(uint64_t n) { return version_scratch_bytes(n) + n * 8 + 16; }

void engine_scratch_carve(void* base, uint64_t n, EngineScratch* s) {
  version_scratch_carve(base, n, &s->v);
  const size_t used = (version_scratch_bytes(n) + 15) & ~size_t(15);
  s->rdst = (uint64_t*)((uint8_t*)base + used);
}

hipError_t launch_engine_step(hf3fs_crc_update_io* ios, hf3fs_crc_engine_job* jobs, uint64_t n, uint32_t r,
                              uint32_t max_rounds, uint32_t max_len, int mode, const OrderScratch& os,
                              const EngineScratch& es, uint32_t* info, hipStream_t st) {
  const StepArgs a{ios,      jobs,     os.round,   os.rank,  os.pred, os.succ, es.v.dec,   os.ctl, es.v.vout, info,
                   es.v.vaddr, es.v.vlen, es.rdst, n,        r,       max_rounds, max_len, mode};
  hipLaunchKernelGGL(k_engine_step, dim3(grid_of(n)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_engine_settle(hf3fs_crc_update_io* ios, hf3fs_crc_engine_job* jobs, uint64_t n,
                                uint32_t max_rounds, const OrderScratch& os, const EngineScratch& es, uint32_t* info,
                                hipStream_t st) {
  hipLaunchKernelGGL(k_engine_settle, dim3(grid_of(n)), dim3(256), 0, st, ios, jobs, os.rank, es.v.dec, es.v.vout,
                     os.ctl, n, max_rounds, info);
  return hipGetLastError();
}

}  // namespace hf3fs_crc
