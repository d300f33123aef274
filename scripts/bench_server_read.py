#!/usr/bin/env python3
"""hf3fs_crc_server_read_prepare / _complete on an MI355X: records for profiles/server_read.jsonl
(appended).  Everything is measured in this one process.

  hash     --jobs reads (1 Mi) of 4-64 KiB out of one arena, the d5 KVCache shape, one request of 32
           jobs each, a CRC32C asked for, nothing transmitted (xmit 2): complete hashes every read.
           The bar is hf3fs_crc_read_result_batch over the same bytes; the margin is the bar's own
           run-to-run spread, min to max over its repetitions.  Both figures, their ratio, the
           margin and by how much complete lands outside it (0 inside) are in the record.
  inline   --small-jobs reads (64 Ki) of 4-64 KiB in requests of 32, no checksum, packed into an
           inline arena: complete against the host's sequential loop on one core (the plan's
           functions compiled with g++ -O2) plus the copies it needs: the records down, the packed
           bytes copied on the device one read at a time, the records back.
  rdma     the same reads listed for RDMA: complete against the host loop and its two record copies.
  prepare  --reqs requests (32,768) of 32 jobs: prepare against the host loop and its two copies.
Every digest, status, list entry and inline byte is compared with the host loop's (exact).  Every
timing: HIP events around the device calls, perf_counter around the host's, a warm-up call before
each timed region, the median of --reps calls.

    python scripts/bench_server_read.py
"""
import argparse
import ctypes
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
hf = importlib.import_module("3fs_amd")
L = hf._lib
JOB, REQ, WR = hf.server_read_job_dtype(), hf.server_read_req_dtype(), hf.server_read_wr_dtype()
READ = np.dtype([("data", "<u8"), ("offset", "<u4"), ("length", "<u4"), ("chunk_len", "<u4"),
                 ("batch_checksum_type", "u1"), ("chunk_checksum_type", "u1"), ("recalculate", "u1"), ("reserved0", "u1"),
                 ("chunk_checksum", "<u4"), ("out_checksum", "<u4"), ("out_checksum_type", "u1"), ("reserved1", "u1", (3,)),
                 ("status", "<i4"), ("reserved2", "<u4"), ("pad", "<u4")])
assert JOB.itemsize == 192 and REQ.itemsize == 128 and READ.itemsize == 48
CRC32C = hf.CRC32C
SMALL, BIG, MAX_LEN = 4 << 20, 64 << 20, 64 << 10

HOST_LOOP = r"""
#include "%s"
using namespace hf3fs_crc;
extern "C" void host_prepare(hf3fs_crc_server_read_job* j, uint64_t n, hf3fs_crc_server_read_req* q,
                             const uint64_t* off, uint64_t n_reqs, uint32_t small_buf, uint32_t big_buf) {
  for (uint64_t r = 0; r < n_reqs; ++r)
    server_read_prepare_request(q[r], off[r], off[r + 1], small_buf, big_buf, [&](uint64_t i) { return j[i]; },
                                [&](uint64_t i, const hf3fs_crc_server_read_job& o) { j[i] = o; });
  (void)n;
}
// Complete without hashing: v holds the range values (or is null when nothing hashes).
extern "C" void host_complete(hf3fs_crc_server_read_job* j, uint64_t n, hf3fs_crc_server_read_req* q,
                              const uint64_t* off, uint64_t n_reqs, uint8_t type, uint32_t max_len, const uint32_t* v,
                              hf3fs_crc_server_read_wr* wr, uint64_t* totals) {
  uint64_t bytes = 0, listed = 0;
  for (uint64_t r = 0; r < n_reqs; ++r) {
    q[r].inline_off = bytes, q[r].wr_first = (uint32_t)listed, q[r].n_ok = q[r].wr_fails = 0, q[r].wr_bytes = 0;
    for (uint64_t i = off[r]; i < off[r + 1]; ++i) {
      const ServerReadRoute o = server_read_route(j[i], q[r], type, max_len);
      const ServerReadDone d = server_read_settle(j[i], q[r], o, o.hashes ? v[i] : 0u);
      if (d.packs) j[i].inline_off = bytes, bytes += j[i].result_len;
      if (d.listed) wr[listed++] = server_read_wr_of(j[i], (uint32_t)i, (uint32_t)r), q[r].wr_bytes += j[i].result_len;
      q[r].n_ok += d.ok, q[r].wr_fails += d.wr_failed;
    }
    q[r].inline_bytes = bytes - q[r].inline_off, q[r].wr_count = (uint32_t)listed - q[r].wr_first;
  }
  totals[0] = bytes, totals[1] = listed;
  (void)n;
}
"""


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def timed(call, reps):
    call()  # warm-up: scratch growth, code load, caches
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def host_timed(call, reps):
    call()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def host_loop():
    """server_read_plan.h's loops as a host library, or None without a host compiler."""
    if not shutil.which("g++"):
        return None
    d = tempfile.mkdtemp(prefix="server_read_host_")
    src, lib = os.path.join(d, "loop.cpp"), os.path.join(d, "loop.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP % os.path.join(REPO, "3fs_amd", "csrc", "server_read_plan.h"))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", src, "-o", lib])
    h = ctypes.CDLL(lib)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    h.host_prepare.argtypes = [vp, u64, vp, vp, u64, ctypes.c_uint32, ctypes.c_uint32]
    h.host_complete.argtypes = [vp, u64, vp, vp, u64, ctypes.c_uint8, ctypes.c_uint32, vp, vp, vp]
    return h


def reads(n, per_req, arena, rng, checksum_type, xmit):
    """n reads of 4-64 KiB (whole 4 KiB blocks at block offsets) out of the arena, per_req to a request."""
    jobs, reqs = np.zeros(n, dtype=JOB), np.zeros((n + per_req - 1) // per_req, dtype=REQ)
    ro = np.minimum(np.arange(reqs.size + 1, dtype=np.uint64) * per_req, n).astype(np.uint64)
    jobs["length"] = rng.integers(1, 17, n) * 4096
    jobs["offset"] = rng.integers(0, 16, n) * 4096
    jobs["chunk_len"] = 1 << 20
    jobs["chunk_checksum_type"], jobs["up_to_date"], jobs["has_rkey"] = CRC32C, 1, 1
    jobs["rdmabuf_size"], jobs["commit_ver"], jobs["update_ver"], jobs["update_ver_now"] = 1 << 20, 1, 1, 1
    jobs["remote_addr"], jobs["rkey"] = rng.integers(1, 1 << 47, n), rng.integers(0, 1 << 32, n)
    if arena is not None:
        span = arena.numel() - (64 << 10)
        jobs["localbuf"] = arena.data_ptr() + rng.integers(0, span // 4096, n) * 4096
        jobs["res"] = jobs["length"]
    reqs["checksum_type"], reqs["xmit"], reqs["max_msg_sz"] = checksum_type, xmit, 1 << 30
    return jobs, reqs, ro


def shape_hash(args, dev, host):
    rng = np.random.default_rng(5)
    n = args.jobs
    arena = torch.empty(args.arena_mib << 20, dtype=torch.uint8, device=dev)
    for at in range(0, arena.numel(), 1 << 30):
        arena[at:at + (1 << 30)].random_(0, 256)
    jobs, reqs, ro = reads(n, 32, arena, rng, CRC32C, hf.SERVER_READ_XMIT_NONE)
    rd = np.zeros(n, dtype=READ)
    rd["data"], rd["offset"], rd["length"], rd["chunk_len"] = jobs["localbuf"], jobs["offset"], jobs["length"], 1 << 20
    rd["batch_checksum_type"] = rd["chunk_checksum_type"] = CRC32C
    d_rd, d_jobs, d_reqs, d_ro = up(rd, dev), up(jobs, dev), up(reqs, dev), up(ro, dev)
    pinfo = torch.zeros(8, dtype=torch.int32, device=dev)
    cinfo = torch.zeros(8, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    hf.server_read_prepare(d_jobs, n, d_reqs, d_ro, reqs.size, pinfo, SMALL, BIG, stream=st)
    bar = timed(lambda: L.read_result_batch(CRC32C, d_rd, n, MAX_LEN, stream=st), args.reps)
    new = timed(lambda: hf.server_read_complete(CRC32C, d_jobs, n, d_reqs, d_ro, reqs.size, cinfo, MAX_LEN, stream=st),
                args.reps)
    torch.cuda.synchronize()
    got, ref = d_jobs.cpu().numpy().view(JOB), d_rd.cpu().numpy().view(READ)
    words = cinfo.cpu().numpy().tolist()
    exact = (np.array_equal(got["checksum"], ref["out_checksum"]) and bool((got["result_status"] == 0).all())
             and bool((ref["status"] == 0).all()) and np.array_equal(got["result_len"], jobs["length"])
             and words == [n, 0, 0, 0, 0, 0, 0, n])
    bar_ms, new_ms = float(np.median(bar)), float(np.median(new))
    margin = max(bar) - min(bar)
    total = int(jobs["length"].sum())
    return dict(record="hash", jobs=n, bytes=total, reps=args.reps, read_result_batch_ms=bar_ms,
                read_result_batch_all_ms=bar, server_read_complete_ms=new_ms, server_read_complete_all_ms=new,
                read_result_batch_gb_s=total / bar_ms / 1e6, server_read_complete_gb_s=total / new_ms / 1e6,
                ratio=new_ms / bar_ms, margin_ms=margin, margin_pct=100 * margin / bar_ms,
                outside_margin_ms=max(0.0, new_ms - bar_ms - margin), within_margin=bool(new_ms <= bar_ms + margin),
                exact=bool(exact))


def shape_xmit(args, dev, host, xmit):
    rng = np.random.default_rng(6 + xmit)
    n = args.small_jobs
    arena = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    arena.random_(0, 256)
    jobs, reqs, ro = reads(n, 32, arena, rng, hf.NONE, xmit)
    jobs["res"][::97] = -5
    jobs["has_rkey"][::89] = 0
    cap = int(jobs["length"].sum())
    d_jobs, d_reqs, d_ro = up(jobs, dev), up(reqs, dev), up(ro, dev)
    inline = torch.zeros(cap, dtype=torch.uint8, device=dev)
    wr = torch.zeros(n * WR.itemsize, dtype=torch.uint8, device=dev)
    pinfo = torch.zeros(8, dtype=torch.int32, device=dev)
    cinfo = torch.zeros(8, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    hf.server_read_prepare(d_jobs, n, d_reqs, d_ro, reqs.size, pinfo, SMALL, BIG, stream=st)
    torch.cuda.synchronize()
    prepared_j, prepared_r = d_jobs.cpu().numpy().view(JOB).copy(), d_reqs.cpu().numpy().view(REQ).copy()
    inl = xmit == hf.SERVER_READ_XMIT_INLINE
    new = timed(lambda: hf.server_read_complete(CRC32C, d_jobs, n, d_reqs, d_ro, reqs.size, cinfo, MAX_LEN,
                                                inline=inline if inl else None, inline_cap=cap if inl else 0,
                                                wr=None if inl else wr, wr_cap=0 if inl else n, stream=st), args.reps)
    torch.cuda.synchronize()
    got_j, got_r = d_jobs.cpu().numpy().view(JOB), d_reqs.cpu().numpy().view(REQ)
    line = dict(record="inline" if inl else "rdma", jobs=n, requests=int(reqs.size), bytes=cap, reps=args.reps,
                server_read_complete_ms=float(np.median(new)), server_read_complete_all_ms=new)
    exact = None
    if host is not None:
        hj, hr = prepared_j.copy(), prepared_r.copy()
        hwr, totals = np.zeros(n, dtype=WR), np.zeros(2, dtype=np.uint64)
        host_dst = torch.zeros(cap if inl else 1, dtype=torch.uint8, device=dev)
        d_hj, d_hr = up(prepared_j, dev), up(prepared_r, dev)
        arena_at = arena.data_ptr()

        def host_call():
            # the records come from the device and go back to it; the loop runs on one core; the
            # packed bytes are copied on the device, one read at a time (the reference's memcpy)
            a, b = d_hj.cpu().numpy().view(JOB).copy(), d_hr.cpu().numpy().view(REQ).copy()
            host.host_complete(a.ctypes.data, n, b.ctypes.data, ro.ctypes.data, reqs.size, CRC32C, MAX_LEN, None,
                               hwr.ctypes.data, totals.ctypes.data)
            if inl:
                for i in np.flatnonzero((a["result_status"] == 0) & (a["result_len"] > 0)):
                    src = int(a["localbuf"][i]) + int(a["head_len"][i]) - arena_at
                    ln, at = int(a["result_len"][i]), int(a["inline_off"][i])
                    host_dst[at:at + ln].copy_(arena[src:src + ln], non_blocking=True)
            up(a, dev), up(b, dev)
            hj[:], hr[:] = a, b
        host_ms = host_timed(host_call, max(1, args.reps // 2))
        lj, lr = prepared_j.copy(), prepared_r.copy()   # (kept alive: the loop works in place, complete reads no output)
        loop_only = host_timed(lambda: host.host_complete(lj.ctypes.data, n, lr.ctypes.data, ro.ctypes.data, reqs.size,
                                                          CRC32C, MAX_LEN, None, hwr.ctypes.data, totals.ctypes.data),
                               args.reps)
        exact = hj.tobytes() == got_j.tobytes() and hr.tobytes() == got_r.tobytes()
        words = cinfo.cpu().numpy().view(np.uint32).tolist()
        if inl:
            exact = exact and bool(torch.equal(host_dst, inline)) and words[2] == int(totals[0]) and words[4] == 0
        else:
            k = int(totals[1])
            exact = exact and wr.cpu().numpy()[:k * WR.itemsize].tobytes() == hwr[:k].tobytes() and words[5] == k
        line.update(host_with_copies_ms=float(np.median(host_ms)), host_with_copies_all_ms=host_ms,
                    host_loop_ms=float(np.median(loop_only)), host_loop_all_ms=loop_only,
                    speedup_over_host_with_copies=float(np.median(host_ms)) / float(np.median(new)))
    line["exact"] = exact
    return line


def shape_prepare(args, dev, host):
    rng = np.random.default_rng(9)
    n = args.reqs * 32
    jobs, reqs, ro = reads(n, 32, None, rng, CRC32C, hf.SERVER_READ_XMIT_NONE)
    jobs["engine"] = rng.random(n) < 0.3
    jobs["commit_ver"] = np.where(rng.random(n) < 0.02, 2, 1)
    jobs["up_to_date"][rng.integers(0, n, args.reqs // 100)] = 0
    d_jobs, d_reqs, d_ro = up(jobs, dev), up(reqs, dev), up(ro, dev)
    pinfo = torch.zeros(8, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    small, big = 256 << 10, 1 << 20
    new = timed(lambda: hf.server_read_prepare(d_jobs, n, d_reqs, d_ro, reqs.size, pinfo, small, big, 32, stream=st),
                args.reps)
    torch.cuda.synchronize()
    got_j, got_r = d_jobs.cpu().numpy().view(JOB), d_reqs.cpu().numpy().view(REQ)
    line = dict(record="prepare", jobs=n, requests=int(reqs.size), reps=args.reps,
                server_read_prepare_ms=float(np.median(new)), server_read_prepare_all_ms=new,
                info=pinfo.cpu().numpy().tolist())
    exact = None
    if host is not None:
        hj, hr = jobs.copy(), reqs.copy()
        d_hj, d_hr = up(jobs, dev), up(reqs, dev)

        def host_call():
            a, b = d_hj.cpu().numpy().view(JOB).copy(), d_hr.cpu().numpy().view(REQ).copy()
            host.host_prepare(a.ctypes.data, n, b.ctypes.data, ro.ctypes.data, reqs.size, small, big)
            up(a, dev), up(b, dev)
            hj[:], hr[:] = a, b
        host_ms = host_timed(host_call, args.reps)
        lj, lr = jobs.copy(), reqs.copy()   # (kept alive; prepare reads no field it writes but an engine job's commit_ver,
        #                                       which it sets to the same value every time)
        loop_only = host_timed(lambda: host.host_prepare(lj.ctypes.data, n, lr.ctypes.data, ro.ctypes.data, reqs.size,
                                                         small, big), args.reps)
        exact = hj.tobytes() == got_j.tobytes() and hr.tobytes() == got_r.tobytes()
        line.update(host_with_copies_ms=float(np.median(host_ms)), host_with_copies_all_ms=host_ms,
                    host_loop_ms=float(np.median(loop_only)), host_loop_all_ms=loop_only,
                    speedup_over_host_with_copies=float(np.median(host_ms)) / float(np.median(new)))
    line["exact"] = exact
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "server_read.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--records", default="hash,inline,rdma,prepare")
    ap.add_argument("--jobs", type=int, default=1 << 20)
    ap.add_argument("--small-jobs", type=int, default=1 << 16)
    ap.add_argument("--reqs", type=int, default=32768)
    ap.add_argument("--arena-mib", type=int, default=16384)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host = host_loop()
    common = {"device": torch.cuda.get_device_name(0), "library": L.load().hf3fs_crc_version().decode()}
    ok = True
    for name in args.records.split(","):
        if name == "hash":
            line = shape_hash(args, dev, host)
        elif name == "prepare":
            line = shape_prepare(args, dev, host)
        else:
            line = shape_xmit(args, dev, host, hf.SERVER_READ_XMIT_INLINE if name == "inline" else hf.SERVER_READ_XMIT_RDMA)
        line = dict(line, **common)
        print(json.dumps(line), flush=True)
        ok &= line["exact"] is not False   # (the margin is reported, not gated)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
