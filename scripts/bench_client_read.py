#!/usr/bin/env python3
"""hf3fs_crc_client_read_batch on an MI355X: records for profiles/client_read.jsonl (appended) and
profiles/client_read_threshold.jsonl (rewritten).

  d5         --blocks blocks (1 M) of 4, 8, 16, 32 or 64 KiB in one HBM arena, one child per
             parent, VERIFY, 0.01 % of the blocks corrupted.  The bar is hf3fs_crc_read_result_batch
             (recalculate over the same bytes, in this process): the new record formats move about
             0.2 % more bytes, so the call may be slower than the bar by that plus the bar's own
             spread, (max - min) / median of its repetitions.  Both figures and the ratio are in
             the record; `within_margin` says whether the ratio kept to them, and the script
             exits 1 when it did not.
  split      --parents parents (64 Ki) x 16 children of 256 KiB (the children share an arena of
             --arena-gib, read-only, so the bytes hashed are the shape's), against what a host
             needs without the call: read_result_batch, a synchronize, the records copied back,
             a merge on the host (element-wise over the parents: the CPU oracle's combine_batch
             on 16 threads, one pass per child position) and the parents uploaded.  Reported only.
  threshold  parents of 1, 2, 4, ... 1024 children (2^22 children per call, no VERIFY: the merge
             kernel alone) under both schedules (forced through max_children).  The last line
             names the switch-over: the largest child count up to which one lane per parent is
             not slower than one wave per parent.
Every timing: HIP events, a warm-up call before each timed region, the median of --reps calls.

    python scripts/bench_client_read.py
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle")]
hf = importlib.import_module("3fs_amd")
L = hf._lib
IO, RESULT = hf.client_read_io_dtype(), hf.client_read_result_dtype()
READ = np.dtype([("data", "<u8"), ("offset", "<u4"), ("length", "<u4"), ("chunk_len", "<u4"), ("batch_type", "u1"),
                 ("chunk_type", "u1"), ("recalculate", "u1"), ("r0", "u1"), ("chunk_checksum", "<u4"),
                 ("out_checksum", "<u4"), ("out_type", "u1"), ("r1", "u1", (3,)), ("status", "<i4"), ("r2", "<u4"), ("pad", "<u4")])
assert IO.itemsize == 40 and READ.itemsize == 48
CRC32C = hf.CRC32C


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


def random_arena(nbytes, dev):
    arena = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for at in range(0, nbytes, 1 << 30):
        arena[at:at + (1 << 30)].random_(0, 256)
    return arena


def device_checksums(addrs, lens, dev):
    """ChecksumInfo::create of every range, by the library itself (the server's side of the read)."""
    d_addr, d_len = up(addrs.astype(np.uint64), dev), up(lens.astype(np.uint64), dev)
    out = torch.zeros(addrs.size, dtype=torch.int32, device=dev)
    L.create_batch(CRC32C, d_addr, d_len, out, addrs.size, int(lens.max()), stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def records(addrs, lens, values):
    ios = np.zeros(addrs.size, dtype=IO)
    ios["data"], ios["length"], ios["read_len"], ios["checksum"], ios["checksum_type"] = addrs, lens, lens, values, CRC32C
    rd = np.zeros(addrs.size, dtype=READ)
    rd["data"], rd["length"], rd["chunk_len"], rd["chunk_checksum"] = addrs, lens, lens, values
    rd["batch_type"] = rd["chunk_type"] = CRC32C
    rd["recalculate"] = 1
    return ios, rd


def shape_d5(args, dev):
    rng = np.random.default_rng(5)
    n = args.blocks
    lens = (4096 << rng.integers(0, 5, n)).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    total = int(lens.sum())
    arena = random_arena(total, dev)
    addrs = (offs + arena.data_ptr()).astype(np.uint64)
    values = device_checksums(addrs, lens, dev)
    bad = rng.choice(n, max(1, n // 10000), replace=False)
    values[bad] ^= 1 << 7
    ios, rd = records(addrs, lens, values)
    d_ios, d_rd = up(ios, dev), up(rd, dev)
    parents = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
    blocks = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    max_len = int(lens.max())
    bar = timed(lambda: L.read_result_batch(CRC32C, d_rd, n, max_len, stream=st), args.reps)
    new = timed(lambda: hf.client_read_batch(CRC32C, d_ios, n, info, max_len=max_len, verify=True, parents=parents,
                                             blocks=blocks, stream=st), args.reps)
    torch.cuda.synchronize()
    got_new = np.flatnonzero(d_ios.cpu().numpy().view(IO)["status"] == 7015)
    got_bar = np.flatnonzero(d_rd.cpu().numpy().view(READ)["status"] == 4080)
    bar_ms, new_ms = float(np.median(bar)), float(np.median(new))
    spread = (max(bar) - min(bar)) / bar_ms
    fmt = 0.002
    return dict(record="d5", blocks=n, bytes=total, reps=args.reps, corrupted=int(bad.size),
                read_result_batch_ms=bar_ms, read_result_batch_all_ms=bar, client_read_batch_ms=new_ms,
                client_read_batch_all_ms=new, read_result_batch_gb_s=total / bar_ms / 1e6,
                client_read_batch_gb_s=total / new_ms / 1e6, ratio=new_ms / bar_ms, format_margin=fmt,
                bar_spread=spread, allowed_ratio=1 + fmt + spread, within_margin=bool(new_ms / bar_ms <= 1 + fmt + spread),
                exact=bool(np.array_equal(got_new, np.sort(bad)) and np.array_equal(got_bar, np.sort(bad))
                           and info.cpu().numpy().tolist()[:3] == [bad.size] * 3))


def host_merge(rd, kids, orc):
    """The merge of :1607-1633 over read-result records, vectorised over the parents."""
    status = rd["status"].reshape(-1, kids)
    value = rd["out_checksum"].reshape(-1, kids)
    length = rd["length"].reshape(-1, kids).astype(np.uint64)
    failed = status != 0
    first = np.where(failed.any(axis=1), failed.argmax(axis=1), kids)
    acc = value[:, 0].copy()
    for j in range(1, kids):
        acc = orc.combine_batch(acc, value[:, j], length[:, j], threads=16)
    out = np.zeros(status.shape[0], dtype=RESULT)
    ok = first == kids
    out["length"] = np.where(ok, length.sum(axis=1).astype(np.uint32), 0)
    out["checksum"], out["checksum_type"] = np.where(ok, acc, 0), np.where(ok, CRC32C, 0)
    out["status"] = np.where(ok, 0, status[np.arange(status.shape[0]), np.minimum(first, kids - 1)])
    out["failed_child"] = np.where(ok, 0xFFFFFFFF, np.arange(status.shape[0]) * kids + first)
    out["block_len"] = length.sum(axis=1).astype(np.uint32)
    return out


def shape_split(args, dev):
    import oracle
    oracle.lib()
    rng = np.random.default_rng(6)
    kids, child = 16, 256 << 10
    n = args.parents * kids
    slots = max(1, min(n, int(args.arena_gib * 2 ** 30) // child))
    arena = random_arena(slots * child, dev)
    addrs = ((np.arange(n) % slots) * child + arena.data_ptr()).astype(np.uint64)
    lens = np.full(n, child, dtype=np.int64)
    slot_values = device_checksums(addrs[:slots], lens[:slots], dev)
    values = slot_values[np.arange(n) % slots].copy()
    bad = rng.choice(n, max(1, n // 10000), replace=False)
    values[bad] ^= 1 << 9
    ios, rd = records(addrs, lens, values)
    d_ios, d_rd = up(ios, dev), up(rd, dev)
    d_off = up(np.arange(args.parents + 1, dtype=np.uint64) * kids, dev)
    parents = torch.zeros(args.parents * 24, dtype=torch.uint8, device=dev)
    parents2 = torch.zeros(args.parents * 24, dtype=torch.uint8, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    new = timed(lambda: hf.client_read_batch(CRC32C, d_ios, n, info, parent_off=d_off, n_parents=args.parents,
                                             max_children=kids, max_len=child, verify=True, parents=parents, stream=st),
                args.reps)
    host_parts = []

    def two_calls():
        L.read_result_batch(CRC32C, d_rd, n, child, stream=st)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        back = d_rd.cpu().numpy().view(READ)
        t1 = time.perf_counter()
        merged = host_merge(back, kids, oracle)
        t2 = time.perf_counter()
        parents2.copy_(torch.from_numpy(merged.view(np.uint8)))
        torch.cuda.synchronize()
        host_parts.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
        return merged

    two_calls()  # warm-up
    wall, merged = [], None
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        merged = two_calls()
        wall.append((time.perf_counter() - t0) * 1e3)
    got = parents.cpu().numpy().view(RESULT)
    # a recalculate mismatch is 4080 on the storage side and 7015 on the client's: the same parents fail
    same = (np.array_equal(got["status"] != 0, merged["status"] != 0) and np.array_equal(got["failed_child"], merged["failed_child"])
            and np.array_equal(got["checksum"][got["status"] == 0], merged["checksum"][merged["status"] == 0])
            and np.array_equal(got["length"], merged["length"]))
    new_ms, two_ms = float(np.median(new)), float(np.median(wall))
    parts = np.median(np.array(host_parts[1:]), axis=0) * 1e3
    return dict(record="split", parents=args.parents, children=kids, child_bytes=child, bytes=n * child,
                arena_bytes=slots * child, reps=args.reps, corrupted=int(bad.size), client_read_batch_ms=new_ms,
                client_read_batch_all_ms=new, client_read_batch_gb_s=n * child / new_ms / 1e6, two_call_host_ms=two_ms,
                two_call_host_all_ms=wall, host_copy_back_ms=float(parts[0]), host_merge_ms=float(parts[1]),
                host_upload_ms=float(parts[2]), speedup=two_ms / new_ms, exact=bool(same),
                failed_parents=int((got["status"] != 0).sum()))


def threshold(args, dev):
    rng = np.random.default_rng(7)
    total = 1 << 22
    ios = np.zeros(total, dtype=IO)
    ios["read_len"] = rng.integers(1, 1 << 20, total)
    ios["length"] = ios["read_len"]
    ios["checksum"], ios["checksum_type"] = rng.integers(0, 1 << 32, total), CRC32C
    d_ios = up(ios, dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    lines, outs = [], {}
    for kids in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
        n_par = total // kids
        d_off = up(np.arange(n_par + 1, dtype=np.uint64) * kids, dev)
        parents = torch.zeros(n_par * 24, dtype=torch.uint8, device=dev)
        blocks = torch.zeros(n_par * 24, dtype=torch.uint8, device=dev)
        ms = {}
        for name, bound in (("lane", 1), ("wave", 1 << 30)):  # (max_children only chooses the schedule)
            ms[name] = timed(lambda: hf.client_read_batch(CRC32C, d_ios, total, info, parent_off=d_off,
                                                          n_parents=n_par, max_children=bound, verify=False,
                                                          parents=parents, blocks=blocks, stream=st), args.reps)
            torch.cuda.synchronize()
            outs[name] = parents.cpu().numpy().tobytes()
        lines.append(dict(record="threshold", children=kids, parents=n_par, ios=total, reps=args.reps,
                          lane_ms=float(np.median(ms["lane"])), wave_ms=float(np.median(ms["wave"])),
                          lane_all_ms=ms["lane"], wave_all_ms=ms["wave"], same_parents=outs["lane"] == outs["wave"]))
        print(json.dumps(lines[-1]), flush=True)
    chosen = 0
    for line in lines:
        if line["lane_ms"] > line["wave_ms"]:
            break
        chosen = line["children"]
    lines.append(dict(record="threshold_chosen", lane_max_children=chosen,
                      rule="the largest measured child count up to which one lane per parent is not slower than one wave"))
    print(json.dumps(lines[-1]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "client_read.jsonl"))
    ap.add_argument("--threshold-out", default=os.path.join(REPO, "profiles", "client_read_threshold.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--records", default="d5,split,threshold")
    ap.add_argument("--blocks", type=int, default=1 << 20)
    ap.add_argument("--parents", type=int, default=1 << 16)
    ap.add_argument("--arena-gib", type=float, default=16.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    common = {"device": torch.cuda.get_device_name(0), "library": L.load().hf3fs_crc_version().decode()}
    ok = True
    for name in args.records.split(","):
        if name == "threshold":
            lines = [dict(x, **common) for x in threshold(args, dev)]
            os.makedirs(os.path.dirname(os.path.abspath(args.threshold_out)), exist_ok=True)
            with open(args.threshold_out, "w") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")
            ok &= all(x.get("same_parents", True) for x in lines)
            continue
        line = dict((shape_d5 if name == "d5" else shape_split)(args, dev), **common)
        print(json.dumps(line), flush=True)
        ok &= line["exact"] and line.get("within_margin", True)  # (d5: the margin gates; split is reported only)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
