#!/usr/bin/env python3
"""hf3fs_crc_md5_batch on an MI355X: a record for profiles/md5_batch.jsonl, no gate.

Shapes (one JSON line per shape and setting):
  a  65,536 files x 256 KiB, one segment each                   md5_stage x md5_sort, all four
  b  65,536 files, log-uniform 4 KiB - 4 MiB, 64 KiB segments   all four (total capped by --cap-gib)
  c  1,024 files x 16 MiB, one segment each                     the library's defaults
  d  524,288 files, log-uniform 4 KiB - 256 KiB, one segment    md5_stage 0, md5_sort 0 and 1 (eight
     each                                                       waves per SIMD: where bucketing can pay)
Per line: GB/s and ms per batch (HIP events, a warm-up call before the timed ones, the median of
--reps calls, every setting of a shape in this one process on the same bytes) and the lane
utilisation, computed here from the lengths: sum of blocks / (64 x sum over waves of the wave's
longest file), with the library's bucket order when md5_sort = 1.
Baseline, line "host": hashlib.md5 over the same bytes copied to host memory, on a pool of 16
threads (hashlib releases the GIL; 16 is a node's CPU quota, not os.cpu_count()); copies are not
timed.  Every digest of every GPU setting must equal hashlib's.

    python scripts/bench_md5.py --out profiles/md5_batch.jsonl
"""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
hf = importlib.import_module("3fs_amd")
L = hf._lib
THREADS = 16
SLAB = 2 << 30


def blocks_of(lengths):
    return lengths // 64 + np.where(lengths % 64 < 56, 1, 2)


def bucket_of(blocks):
    """md5_bucket of 3fs_amd/csrc/md5_core.h (the longest first)."""
    b = np.maximum(blocks, 1).astype(np.uint64)
    o = np.floor(np.log2(b.astype(np.float64))).astype(np.int64)
    o = np.where((np.uint64(1) << o.astype(np.uint64)) > b, o - 1, o)
    sub = np.where(o >= 2, (b >> np.maximum(o - 2, 0).astype(np.uint64)) & np.uint64(3),
                   (b << np.maximum(2 - o, 0).astype(np.uint64)) & np.uint64(3)).astype(np.int64)
    return np.where(blocks == 0, 255, 254 - (4 * o + sub))


def lane_utilisation(lengths, sort):
    blocks = blocks_of(lengths)
    order = np.argsort(bucket_of(blocks), kind="stable") if sort else np.arange(blocks.size)
    b = blocks[order]
    pad = (-b.size) % 64
    waves = np.concatenate([b, np.zeros(pad, dtype=b.dtype)]).reshape(-1, 64)
    return float(b.sum() / (64 * waves.max(axis=1).sum()))


class Shape:
    def __init__(self, name, lengths, seg_bytes, dev):
        self.name, self.lengths = name, lengths
        self.offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        self.total = int(self.offsets[-1])
        self.arena = torch.empty(self.total + 64, dtype=torch.uint8, device=dev)
        for at in range(0, self.arena.numel(), 1 << 30):
            self.arena[at:at + (1 << 30)].random_(0, 256)
        base = self.arena.data_ptr()
        if seg_bytes:
            segs, off = [], [0]
            for o, n in zip(self.offsets[:-1], lengths):
                cuts = np.arange(0, n, seg_bytes, dtype=np.int64)
                segs.append(np.stack([base + o + cuts, np.minimum(cuts + seg_bytes, n) - cuts], axis=1))
                off.append(off[-1] + cuts.size)
            segs = np.concatenate(segs).astype(np.uint64)
        else:  # one segment per file
            segs = np.stack([base + self.offsets[:-1], lengths], axis=1).astype(np.uint64)
            off = np.arange(lengths.size + 1)
        self.n_files, self.n_segs = lengths.size, segs.shape[0]
        self.d_segs = torch.from_numpy(segs.view(np.int64)).to(dev)
        self.d_off = torch.from_numpy(np.array(off, dtype=np.int64)).to(dev)
        self.out = torch.zeros(16 * self.n_files, dtype=torch.uint8, device=dev)

    def call(self):
        L.md5_batch(self.d_segs, self.d_off, self.n_files, self.n_segs, out=self.out,
                    stream=torch.cuda.current_stream())

    def timed(self, reps):
        self.out.zero_()
        self.call()  # warm-up: scratch growth, code load, caches
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self.call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), self.out.cpu().numpy().tobytes()

    def host(self):
        """(seconds of hashing on THREADS threads, digests): slabs of files through pinned memory."""
        pinned = torch.empty(max(SLAB, int(self.lengths.max())), dtype=torch.uint8, pin_memory=True)
        view = pinned.numpy()
        digests, seconds, f = [], 0.0, 0
        with ThreadPoolExecutor(THREADS) as pool:
            while f < self.n_files:
                g = f + 1
                while g < self.n_files and self.offsets[g + 1] - self.offsets[f] <= pinned.numel():
                    g += 1
                lo, hi = int(self.offsets[f]), int(self.offsets[g])
                pinned[:hi - lo].copy_(self.arena[lo:hi])
                torch.cuda.synchronize()
                spans = [(int(self.offsets[k]) - lo, int(self.offsets[k + 1]) - lo) for k in range(f, g)]
                t0 = time.perf_counter()
                digests += list(pool.map(lambda s: hashlib.md5(view[s[0]:s[1]]).digest(), spans, chunksize=8))
                seconds += time.perf_counter() - t0
                f = g
        return seconds, b"".join(digests)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "md5_batch.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--files", type=int, default=65536)
    ap.add_argument("--cap-gib", type=float, default=0.0, help="cap of shape b's bytes (0: 40 %% of free HBM)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    free, _ = torch.cuda.mem_get_info()
    cap = int(args.cap_gib * 2 ** 30) if args.cap_gib else int(free * 0.4)
    rng = np.random.default_rng(5)
    defaults = (int(L.get_option("md5_stage")), int(L.get_option("md5_sort")))
    lines = []
    for name in args.shapes.split(","):
        if name == "a":
            lengths, seg, modes = np.full(args.files, 256 << 10, dtype=np.int64), 0, None
        elif name == "b":
            lengths = np.exp(rng.uniform(np.log(4 << 10), np.log(4 << 20), args.files)).astype(np.int64)
            if lengths.sum() > cap:
                lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), cap))]
            seg, modes = 64 << 10, None
        elif name == "c":
            lengths, seg, modes = np.full(1024, 16 << 20, dtype=np.int64), 0, [defaults]
        else:
            lengths = np.exp(rng.uniform(np.log(4 << 10), np.log(256 << 10), 8 * args.files)).astype(np.int64)
            seg, modes = 0, [(0, 0), (0, 1)]
        shape = Shape(name, lengths, seg, dev)
        host_s, want = shape.host()
        common = {"shape": name, "files": int(lengths.size), "bytes": shape.total, "segments": shape.n_segs,
                  "device": torch.cuda.get_device_name(0)}
        lines.append(dict(common, setting="host", threads=THREADS, ms=host_s * 1e3, gb_s=shape.total / host_s / 1e9))
        print(json.dumps(lines[-1]), flush=True)
        for stage, sort in modes or [(0, 0), (0, 1), (1, 0), (1, 1)]:
            with L.option("md5_stage", stage), L.option("md5_sort", sort):
                ms, got = shape.timed(args.reps)
            lines.append(dict(common, setting="gpu", md5_stage=stage, md5_sort=sort, default=(stage, sort) == defaults,
                              reps=args.reps, ms=ms, gb_s=shape.total / ms / 1e6,
                              lane_utilisation=lane_utilisation(lengths, sort), exact=got == want))
            print(json.dumps(lines[-1]), flush=True)
        del shape
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    return 0 if all(x.get("exact", True) for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
