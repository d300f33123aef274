#!/usr/bin/env python3
"""hf3fs_crc_range_query / hf3fs_crc_file_length on an MI355X: records for profiles/range_query.jsonl
(appended).  Everything is measured in this one process.

  query_last   --records (8 Mi) table records, --ops (1 Mi) QUERY ops whose ranges hold 8 chunks each,
               max_chunks 1 (queryLastChunk as the meta service's length sync sends it)
  query_total  the same ops unlimited (queryTotalChunk)
  remove       the same table, 1,024 REMOVE ops that list --ops chunks in all
  table_pass   the same table and no op: the count, scan and apply launches alone
  file_length  the fold over the --ops finished ops of query_total in files of 4
  file_length_1024  the same ops under 256 chain ids in files of 1024, the fold's quadratic worst shape
  bench_py     (--bench-py-parent / --bench-py-final) bench.py's headline with the parent commit's library and
               with this one, from result files of runs alternated on one box; no GPU is touched
Each against the reference's sequential loop restated in C++ (g++ -O2) on one host core over the same
arrays: per op a binary-search seek to `end`, then the paged walk of processQueryResults /
queryChunks at page size 1000; per file queryChunksByChain with a std::map and queryChunks' fold.
The bar's own spread (min to max over its repetitions, in per cent of its median) is recorded next
to each ratio.  Every op, file, list entry and info word is compared with the host loop's (exact).
Timing: HIP events around the device call, perf_counter around the host's, a warm-up call before
each timed region, the median of --reps calls.  A ratio is reported, none is asserted.

    python scripts/bench_range.py
"""
import argparse
import ctypes
import importlib
import json
import os
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
META, OP, FILE = hf.sync_meta_dtype(), hf.range_op_dtype(), hf.file_len_dtype()
INODE = 0x0123456789AB0000

HOST_LOOP = r"""
#include <algorithm>
#include <map>
#include <vector>
#include "%s"
namespace {
struct Id {
  uint64_t hi, lo;
  bool operator<(const Id& o) const { return hi < o.hi || (hi == o.hi && lo < o.lo); }
  bool operator==(const Id& o) const { return hi == o.hi && lo == o.lo; }
};
// ChunkStore::queryChunks: seek to `end` (a binary search, as the store's iterator does), descend.
void query_chunks(const hf3fs_crc_sync_meta* t, uint64_t n, Id begin, Id end, uint32_t max_num, std::vector<uint32_t>& out) {
  out.clear();
  int64_t lo = 0, hi = (int64_t)n;  // the first record above `end`
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (end < Id{t[mid].id_hi, t[mid].id_lo}) hi = mid; else lo = mid + 1;
  }
  for (int64_t it = lo - 1; it >= 0 && out.size() < max_num; --it) {
    const Id id{t[it].id_hi, t[it].id_lo};
    if (id == end) continue;
    if (id < begin) break;
    out.push_back((uint32_t)it);
  }
}
}  // namespace
extern "C" void host_range(const hf3fs_crc_sync_meta* t, uint64_t n, hf3fs_crc_range_op* ops, uint64_t n_ops,
                           uint32_t* list, uint64_t list_cap, uint32_t page, uint32_t* info) {
  std::vector<uint32_t> result;
  uint64_t listed = 0, chunks = 0, ok = 0;
  for (uint64_t k = 0; k < n_ops; ++k) {
    hf3fs_crc_range_op& op = ops[k];
    op.last_hi = op.last_lo = op.total_len = 0, op.total_chunks = op.last_len = 0, op.last_index = 0xFFFFFFFFu, op.more = 0;
    op.reserved1[0] = op.reserved1[1] = op.reserved1[2] = 0;
    op.list_first = listed < 0xFFFFFFFFull ? (uint32_t)listed : 0xFFFFFFFFu;
    op.status = op.status_in ? op.status_in : (op.kind == 1 || op.kind == 2 ? 0 : 3);
    if (op.status) continue;
    ++ok;
    const Id begin{op.begin_hi, op.begin_lo};
    Id current_end{op.end_hi, op.end_lo};
    const uint32_t to_process = op.max_chunks ? std::min(op.max_chunks, UINT32_MAX - 1) : UINT32_MAX - 1;
    uint32_t results = 0;
    bool have = false;
    Id last{0, 0};
    while (true) {
      const uint32_t current_max = std::min(to_process - results + 1, page);
      query_chunks(t, n, begin, current_end, current_max, result);
      bool done = false;
      for (uint32_t index : result) {
        if (t[index].recycle_state != 0) continue;
        if (results < to_process) {
          const Id id{t[index].id_hi, t[index].id_lo};
          if (!have || last < id) last = id, op.last_len = t[index].length, op.last_index = index, have = true;
          op.total_len += t[index].length;
          op.total_chunks++;
          if (op.kind == 2) {
            if (listed < list_cap) list[listed] = index;
            ++listed;
          }
        }
        if (++results >= to_process + 1) { done = true; break; }
      }
      if (done || result.size() < current_max) break;
      current_end = Id{t[result.back()].id_hi, t[result.back()].id_lo};
    }
    op.last_hi = last.hi, op.last_lo = last.lo;
    op.more = results > to_process;
    chunks += op.total_chunks;
  }
  info[0] = (uint32_t)ok, info[1] = (uint32_t)(n_ops - ok), info[2] = (uint32_t)chunks, info[3] = (uint32_t)(chunks >> 32);
  info[4] = (uint32_t)listed, info[5] = (uint32_t)(listed >> 32), info[6] = listed > list_cap, info[7] = 0;
}
struct QueryResult { uint64_t length, lastChunk, lastChunkLen, totalChunkLen, totalNumChunks; };
extern "C" void host_files(const hf3fs_crc_range_op* ops, uint64_t n_ops, hf3fs_crc_file_len* files, uint64_t n_files) {
  for (uint64_t i = 0; i < n_files; ++i) {
    hf3fs_crc_file_len& f = files[i];
    f.status = 0, f.length = f.total_len = f.total_chunks = 0, f.last_chunk = f.last_chunk_len = 0;
    if (f.n_file_ops > 1024 || (uint64_t)f.first_op + f.n_file_ops > n_ops) { f.status = 3; continue; }
    std::map<uint32_t, QueryResult> chunks;
    for (uint32_t q = f.first_op; q < f.first_op + f.n_file_ops && !f.status; ++q) {
      const hf3fs_crc_range_op& r = ops[q];
      if (r.status) { if (r.status == 7007) continue; f.status = r.status; break; }
      if (r.total_chunks == 0) continue;
      const uint64_t ino = (r.last_hi & 0xFFFFFFFFFFFFull) << 16 | r.last_lo >> 48, chunk = r.last_lo & 0xFFFFFFFFull;
      if ((r.last_hi == 0x0000FFFFFFFFFFFFull && r.last_lo == 0xFFFF000000000000ull) || ino != f.inode) { f.status = 2; break; }
      if ((f.flags & 1) && f.n_file_ops < f.stripe_size && chunk >= f.n_file_ops) { f.status = 3019; break; }
      chunks[r.chain_id] = QueryResult{chunk * f.chunk_size + r.last_len, chunk, r.last_len, r.total_len, r.total_chunks};
    }
    if (f.status) continue;
    for (auto it = chunks.begin(); it != chunks.end(); ++it) {
      if (it == chunks.begin() || f.length < it->second.length)
        f.length = it->second.length, f.last_chunk = (uint32_t)it->second.lastChunk, f.last_chunk_len = (uint32_t)it->second.lastChunkLen;
      f.total_len += it->second.totalChunkLen, f.total_chunks += it->second.totalNumChunks;
    }
  }
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
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def host_loop():
    d = tempfile.mkdtemp(prefix="range_host_")
    src, lib = os.path.join(d, "loop.cpp"), os.path.join(d, "loop.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP % os.path.join(REPO, "include", "hf3fs_crc.h"))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", src, "-o", lib])
    h = ctypes.CDLL(lib)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    h.host_range.argtypes = [vp, u64, vp, u64, vp, u64, u32, vp]
    h.host_files.argtypes = [vp, u64, vp, u64]
    h.host_range.restype = h.host_files.restype = None
    return h


def stats(name, ms):
    med = float(np.median(ms))
    return {f"{name}_ms": med, f"{name}_all_ms": [float(x) for x in ms],
            f"{name}_spread_pct": 100.0 * (max(ms) - min(ms)) / med if med else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=8 << 20)
    ap.add_argument("--ops", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "range_query.jsonl"))
    ap.add_argument("--bench-py-parent", nargs="+", metavar="JSON", default=None,
                    help="with --bench-py-final: files holding bench.py's result line, measured with the parent "
                         "commit's library (HF3FS_CRC_LIB) on the same box; appends a bench_py record and exits")
    ap.add_argument("--bench-py-final", nargs="+", metavar="JSON", default=None)
    a = ap.parse_args()
    if a.bench_py_parent or a.bench_py_final:
        def values(paths):
            return [json.loads(open(p).read().strip().splitlines()[-1])["value"] for p in paths]
        parent, final = values(a.bench_py_parent), values(a.bench_py_final)
        pm, fm = float(np.median(parent)), float(np.median(final))
        rec = {"record": "bench_py", "unit": "GB/s", "order": "parent, final alternated in one visit to one box",
               "parent_gb_s": parent, "final_gb_s": final, "parent_median": pm, "final_median": fm,
               "ratio": fm / pm, "parent_spread_pct": 100.0 * (max(parent) - min(parent)) / pm,
               "final_inside_parent_range": bool(min(parent) <= fm <= max(parent))}
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))
        return 0
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0xBE7C4)
    h = host_loop()
    common = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "host_reps": a.host_reps, "page": 1000}
    n, n_ops = a.records, a.ops
    per = n // n_ops  # records per op's range: 8

    # the table: chunks 0.. of one inode, one record in 16 being removed
    meta = np.zeros(n, dtype=META)
    meta["id_hi"], meta["id_lo"] = INODE >> 16, np.arange(n, dtype=np.uint64)
    meta["length"] = rng.integers(1, 1 << 22, n)
    meta["recycle_state"] = np.where(rng.random(n) < 1 / 16, 1, 0)
    d_meta = up(meta, dev)
    records = []

    def run_ops(record, ops, list_cap):
        d_ops, d_info = up(ops, dev), torch.zeros(8, dtype=torch.int32, device=dev)
        d_list = torch.zeros(max(list_cap, 1), dtype=torch.int32, device=dev)
        call = lambda: L.range_query(d_meta, n, d_ops, ops.size, d_info, d_list if list_cap else None, list_cap,  # noqa: E731
                                     stream=torch.cuda.current_stream())
        gpu = timed(call, a.reps)
        got = d_ops.cpu().numpy().view(OP)
        want, info, lst = ops.copy(), np.zeros(8, dtype=np.uint32), np.zeros(max(list_cap, 1), dtype=np.uint32)
        host = host_timed(lambda: h.host_range(meta.ctypes.data, n, want.ctypes.data, want.size, lst.ctypes.data, list_cap,
                                               1000, info.ctypes.data), a.host_reps)
        exact = (got.tobytes() == want.tobytes() and d_info.cpu().numpy().view(np.uint32).tolist() == info.tolist()
                 and np.array_equal(d_list.cpu().numpy().view(np.uint32)[:list_cap], lst[:list_cap]))
        rec = {"record": record, "table_records": n, "ops": int(ops.size), "list_entries": int(info[4]),
               "chunks": int(info[2]) | int(info[3]) << 32, **stats("range_query", gpu), **stats("host_loop", host),
               "exact": bool(exact), **common}
        rec["speedup_over_host_loop"] = rec["host_loop_ms"] / rec["range_query_ms"]
        records.append(rec)
        print(json.dumps(rec), flush=True)
        return want

    ops = np.zeros(n_ops, dtype=OP)
    first = np.arange(n_ops, dtype=np.uint64) * np.uint64(per)
    order = rng.permutation(n_ops)  # the ops arrive in no order of their ranges
    ops["begin_hi"] = ops["end_hi"] = INODE >> 16
    ops["begin_lo"], ops["end_lo"] = first[order], first[order] + np.uint64(per)
    ops["kind"], ops["chain_id"] = hf.RANGE_QUERY, rng.integers(0, 1 << 16, n_ops)
    ops["max_chunks"] = 1
    run_ops("query_last", ops, 0)
    ops["max_chunks"] = 0
    finished = run_ops("query_total", ops, 0)
    rem = np.zeros(1024, dtype=OP)
    span = n // 1024
    rem["begin_hi"] = rem["end_hi"] = INODE >> 16
    rem["begin_lo"] = np.arange(1024, dtype=np.uint64) * np.uint64(span)
    rem["end_lo"] = rem["begin_lo"] + np.uint64(span)
    rem["kind"], rem["max_chunks"] = hf.RANGE_REMOVE, n_ops // 1024
    run_ops("remove", rem, n_ops)

    # the table pass alone (count, scan, apply; no op): what every call pays before its searches.  Bytes: the
    # 48-byte records read by count and by apply, 12 bytes of prefix written per record.
    d_info0 = torch.zeros(8, dtype=torch.int32, device=dev)
    gpu = timed(lambda: L.range_query(d_meta, n, None, 0, d_info0, None, 0, stream=torch.cuda.current_stream()), a.reps)
    rec = {"record": "table_pass", "table_records": n, "ops": 0, **stats("range_query", gpu),
           "bytes": n * (48 * 2 + 12), **common}
    rec["gb_s"] = rec["bytes"] / rec["range_query_ms"] / 1e6
    records.append(rec)
    print(json.dumps(rec), flush=True)

    # the fold: files of 4 over the finished ops (their ids are the one inode's)
    n_files = n_ops // 4
    files = np.zeros(n_files, dtype=FILE)
    files["inode"], files["first_op"], files["n_file_ops"] = INODE, 4 * np.arange(n_files), 4
    files["chunk_size"], files["stripe_size"] = 1 << 22, 4
    d_ops, d_files, d_info = up(finished, dev), up(files, dev), torch.zeros(8, dtype=torch.int32, device=dev)
    gpu = timed(lambda: L.file_length(d_ops, n_ops, d_files, n_files, d_info, stream=torch.cuda.current_stream()), a.reps)
    want = files.copy()
    host = host_timed(lambda: h.host_files(finished.ctypes.data, n_ops, want.ctypes.data, n_files), a.host_reps)
    rec = {"record": "file_length", "ops": n_ops, "files": n_files, **stats("file_length", gpu), **stats("host_loop", host),
           "exact": bool(d_files.cpu().numpy().tobytes() == want.tobytes()),
           "info": d_info.cpu().numpy().view(np.uint32).tolist(), **common}
    rec["speedup_over_host_loop"] = rec["host_loop_ms"] / rec["file_length_ms"]
    records.append(rec)
    print(json.dumps(rec), flush=True)
    # the fold's worst shape: files of 1024 ops (the record format's bound) with 256 chain ids, so three ops
    # in four are replaced by a later one of their chain; one lane per file, quadratic in the op count
    crowded = finished.copy()
    crowded["chain_id"] = rng.integers(0, 256, n_ops)
    n_big = n_ops // 1024
    big = np.zeros(n_big, dtype=FILE)
    big["inode"], big["first_op"], big["n_file_ops"] = INODE, 1024 * np.arange(n_big), 1024
    big["chunk_size"], big["stripe_size"] = 1 << 22, 1024
    d_ops, d_files = up(crowded, dev), up(big, dev)
    gpu = timed(lambda: L.file_length(d_ops, n_ops, d_files, n_big, d_info, stream=torch.cuda.current_stream()), a.reps)
    want = big.copy()
    host = host_timed(lambda: h.host_files(crowded.ctypes.data, n_ops, want.ctypes.data, n_big), a.host_reps)
    rec = {"record": "file_length_1024", "ops": n_ops, "files": n_big, **stats("file_length", gpu),
           **stats("host_loop", host), "exact": bool(d_files.cpu().numpy().tobytes() == want.tobytes()),
           "info": d_info.cpu().numpy().view(np.uint32).tolist(), **common}
    rec["speedup_over_host_loop"] = rec["host_loop_ms"] / rec["file_length_ms"]
    records.append(rec)
    print(json.dumps(rec), flush=True)
    with open(a.out, "a") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    return 0 if all(r.get("exact", True) for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())
