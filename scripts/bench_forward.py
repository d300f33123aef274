#!/usr/bin/env python3
"""hf3fs_crc_forward_prepare / _complete on an MI355X: records for profiles/forward.jsonl (appended).

  syncing  --jobs jobs (4096), each a 64 KiB - 1 MiB write into a 4 MiB chunk whose successor is
           SYNCING, so prepare hashes every chunk whole (16 GiB) before it builds the outgoing
           whole-chunk writes; one chunk's stored checksum is wrong.  The bar is
           hf3fs_crc_scrub_batch over the same chunks in the same process; the margin is the bar's
           own run-to-run spread, min to max over its repetitions.  Both figures, the margin and
           by how much prepare lands outside it (0 inside) are in the record.
  plain    --plain-jobs jobs (1 Mi) that hash nothing: writes to serving successors, answered in
           agreement.  Prepare and complete each, against the sequential loop of
           3fs_amd/csrc/forward_plan.h over the same records on one host core (compiled here with
           g++ -O2; without a host compiler the host figures are null).
Every timing: HIP events, a warm-up call before each timed region, the median of --reps calls.

    python scripts/bench_forward.py
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
JOB = hf.forward_job_dtype()
SCRUB = np.dtype([("data", "<u8"), ("length", "<u4"), ("checksum_type", "u1"), ("fin", "u1"), ("reserved", "<u2"),
                  ("checksum", "<u4"), ("computed", "<u4"), ("status", "<i4"), ("reserved2", "<u4")])
assert JOB.itemsize == 192 and SCRUB.itemsize == 32
CRC32C = hf.CRC32C
CHUNK = 4 << 20

HOST_LOOP = r"""
#include "%s"
using namespace hf3fs_crc;
extern "C" void host_prepare(hf3fs_crc_forward_job* j, uint64_t n, uint8_t type, uint32_t max_len, uint32_t max_inline) {
  for (uint64_t i = 0; i < n; ++i) forward_prepare_settle(j[i], forward_route(j[i], type, max_len), 0u, max_inline);
}
extern "C" void host_complete(hf3fs_crc_forward_job* j, uint64_t n, uint8_t type, uint32_t max_len) {
  for (uint64_t i = 0; i < n; ++i) forward_complete_settle(j[i], type, max_len, 0u);
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


def write_jobs(n, payload, lengths, chunk_size):
    """Successful local writes of version 5 on chain version 7, each with a successor."""
    j = np.zeros(n, dtype=JOB)
    j["update_type"], j["payload"], j["length"], j["chunk_size"] = hf.UPDATE_WRITE, payload, lengths, chunk_size
    j["req_update_ver"] = j["upd_update_ver"] = 5
    j["upd_commit_ver"], j["upd_length"] = 4, lengths
    j["req_checksum_type"] = j["upd_checksum_type"] = CRC32C
    j["chain_ver"], j["has_successor"] = 7, 1
    return j


def shape_syncing(args, dev):
    rng = np.random.default_rng(8)
    n = args.jobs
    arena = torch.empty(n * CHUNK, dtype=torch.uint8, device=dev)
    for at in range(0, n * CHUNK, 1 << 30):
        arena[at:at + (1 << 30)].random_(0, 256)
    addrs = (np.arange(n, dtype=np.uint64) * CHUNK + arena.data_ptr()).astype(np.uint64)
    d_addr, d_len = up(addrs, dev), up(np.full(n, CHUNK, dtype=np.uint64), dev)
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    L.create_batch(CRC32C, d_addr, d_len, out, n, CHUNK, stream=st)
    torch.cuda.synchronize()
    values = out.cpu().numpy().view(np.uint32).copy()
    bad = int(rng.integers(0, n))
    values[bad] ^= 1 << 7
    scrub = np.zeros(n, dtype=SCRUB)
    scrub["data"], scrub["length"], scrub["checksum_type"], scrub["checksum"] = addrs, CHUNK, CRC32C, values
    jobs = write_jobs(n, addrs, (rng.integers(16, 257, n) * 4096).astype(np.uint32), CHUNK)
    jobs["successor_syncing"], jobs["chunk"], jobs["chunk_len"] = 1, addrs, CHUNK
    jobs["chunk_checksum_type"], jobs["chunk_checksum"], jobs["chunk_update_ver"] = CRC32C, values, 5
    d_scrub, d_jobs = up(scrub, dev), up(jobs, dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    info = torch.zeros(hf.FORWARD_INFO_WORDS, dtype=torch.int32, device=dev)
    bar = timed(lambda: L.scrub_batch(CRC32C, d_scrub, n, CHUNK, count, stream=st), args.reps)
    new = timed(lambda: hf.forward_prepare(CRC32C, d_jobs, n, info, CHUNK, args.max_inline, stream=st), args.reps)
    torch.cuda.synchronize()
    got = d_jobs.cpu().numpy().view(JOB)
    words = info.cpu().numpy().tolist()
    exact = (np.flatnonzero(got["status"] == 4080).tolist() == [bad] and int(count.item()) == 1
             and words[:6] == [n - 1, 1, 0, n, 1, 0] and np.array_equal(got["computed"], values ^ np.where(np.arange(n) == bad, 1 << 7, 0).astype(np.uint32))
             and bool((got["out_length"][got["action"] == hf.FORWARD_SEND] == CHUNK).all()))
    bar_ms, new_ms = float(np.median(bar)), float(np.median(new))
    margin = max(bar) - min(bar)
    total = n * CHUNK
    return dict(record="syncing", jobs=n, chunk_bytes=CHUNK, bytes=total, reps=args.reps, scrub_batch_ms=bar_ms,
                scrub_batch_all_ms=bar, forward_prepare_ms=new_ms, forward_prepare_all_ms=new,
                scrub_batch_gb_s=total / bar_ms / 1e6, forward_prepare_gb_s=total / new_ms / 1e6, ratio=new_ms / bar_ms,
                margin_ms=margin, outside_margin_ms=max(0.0, new_ms - bar_ms - margin),
                within_margin=bool(new_ms <= bar_ms + margin), exact=bool(exact))


def host_loop():
    """forward_plan.h's loop as a host library, or None without a host compiler."""
    if not shutil.which("g++"):
        return None
    d = tempfile.mkdtemp(prefix="forward_host_")
    src, lib = os.path.join(d, "loop.cpp"), os.path.join(d, "loop.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP % os.path.join(REPO, "3fs_amd", "csrc", "forward_plan.h"))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", src, "-o", lib])
    h = ctypes.CDLL(lib)
    h.host_prepare.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint32]
    h.host_complete.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_uint32]
    return h


def host_timed(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def shape_plain(args, dev):
    rng = np.random.default_rng(9)
    n = args.plain_jobs
    pay = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)   # named by the records, never read
    jobs = write_jobs(n, pay.data_ptr(), (rng.integers(1, 257, n) * 4096).astype(np.uint32), CHUNK)
    jobs["req_update_ver"] = np.where(rng.random(n) < .5, 0, 5)
    jobs["upd_checksum"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    jobs["has_successor"] = rng.random(n) < .97
    # the successors' answers, in place before prepare (it leaves a sent job's response alone)
    jobs["fwd_length"], jobs["fwd_checksum_type"], jobs["fwd_checksum"] = jobs["length"], CRC32C, jobs["upd_checksum"]
    jobs["fwd_commit_ver"], jobs["fwd_commit_chain_ver"] = 5, 7
    late = rng.random(n) < .01
    jobs["fwd_status"] = np.where(late, 4010, 0)
    d_jobs = up(jobs, dev)
    idx = torch.zeros(n, dtype=torch.int32, device=dev)
    pinfo = torch.zeros(hf.FORWARD_INFO_WORDS, dtype=torch.int32, device=dev)
    dinfo = torch.zeros(hf.FORWARD_INFO_WORDS, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    prep = timed(lambda: hf.forward_prepare(CRC32C, d_jobs, n, pinfo, CHUNK, args.max_inline, stream=st), args.reps)
    done = timed(lambda: hf.forward_complete(CRC32C, d_jobs, n, dinfo, CHUNK, commit_idx=idx, stream=st), args.reps)
    torch.cuda.synchronize()
    got = d_jobs.cpu().numpy().view(JOB)
    commits = int(dinfo[0].item())
    want = np.flatnonzero((jobs["has_successor"] == 0) | ~late)
    exact = commits == want.size and np.array_equal(idx.cpu().numpy().view(np.uint32)[:commits], want)
    host = host_loop()
    host_prep = host_done = None
    if host is not None:
        mine = jobs.copy()
        host_prep = host_timed(lambda: host.host_prepare(mine.ctypes.data, n, CRC32C, CHUNK, args.max_inline), args.reps)
        host_done = host_timed(lambda: host.host_complete(mine.ctypes.data, n, CRC32C, CHUNK), args.reps)
        exact = exact and mine.tobytes() == got.tobytes()
    med = lambda x: None if x is None else float(np.median(x))  # noqa: E731
    line = dict(record="plain", jobs=n, reps=args.reps, forward_prepare_ms=med(prep), forward_prepare_all_ms=prep,
                forward_complete_ms=med(done), forward_complete_all_ms=done, host_prepare_ms=med(host_prep),
                host_prepare_all_ms=host_prep, host_complete_ms=med(host_done), host_complete_all_ms=host_done,
                commits=commits, exact=bool(exact))
    if host is not None:
        line["prepare_speedup"] = med(host_prep) / med(prep)
        line["complete_speedup"] = med(host_done) / med(done)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forward.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--records", default="syncing,plain")
    ap.add_argument("--jobs", type=int, default=4096)
    ap.add_argument("--plain-jobs", type=int, default=1 << 20)
    ap.add_argument("--max-inline", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    common = {"device": torch.cuda.get_device_name(0), "library": L.load().hf3fs_crc_version().decode()}
    ok = True
    for name in args.records.split(","):
        line = dict((shape_syncing if name == "syncing" else shape_plain)(args, dev), **common)
        print(json.dumps(line), flush=True)
        ok &= line["exact"]   # (the margin is reported, not gated)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
