"""A/B of hf3fs_crc_update_cow_batch against what a caller could do before it.

Variants take turns inside ONE process (box-to-box spread is 3-8 %), after a
warm-up, timed with stream events around `--calls` calls:

  cow      d3's batch -- 4096 DISTINCT 4 MiB chunks, writes U[64 KiB, 1 MiB], DELTA -- applied out of
           place: update_cow_batch (A) vs a device-to-device copy of every old chunk to its
           destination followed by an in-place update_batch on the copies, the copy as one
           hipMemcpyAsync per chunk of chunk_size bytes (B) or as ONE copy of the contiguous arena
           (C).  The three must leave equal records and equal bytes in [0, out_size) of every
           destination.
  inplace  the in-place path of this build against another build of the library (--parent-lib,
           loaded beside it): bench.py's headline (create_strided over 4096 x 4 MiB), d3 DELTA
           update_batch, a latency-bound batch of 256 of its IOs and the out-of-place variant A
           (update_cow_batch), the two libraries alternating, `--runs` runs each.  Before the
           timing one line per (n, max_len, mode) with what the three *_scratch_bytes functions
           of either library return ("equal": the builds ask for the same bytes).
  d3loop   d3 DELTA update_batch alone, `--runs` x `--calls` calls of the library this process loaded
           (HF3FS_CRC_LIB names another build): the loop a kernel trace of one build is taken of.
  syncing  a whole-chunk resync batch (4096 x 4 MiB, syncing, out of place) vs verify_strided of
           the payloads plus one copy of the same bytes.  For the record only.

One JSON line per variant to --out (default profiles/update_cow_ab.jsonl).
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle")]
hf = importlib.import_module("3fs_amd")
L = hf._lib

REC = np.dtype([("chunk", "<u8"), ("payload", "<u8"), ("offset", "<u4"), ("length", "<u4"), ("chunk_size", "<u4"),
                ("update_type", "u1"), ("chunk_checksum_type", "u1"), ("write_checksum_type", "u1"), ("flags", "u1"),
                ("chunk_checksum", "<u4"), ("write_checksum", "<u4"), ("out_size", "<u4"), ("out_checksum", "<u4"),
                ("out_checksum_type", "u1"), ("checksum_case", "u1"), ("reserved1", "u1", (2,)), ("status", "<i4")])
assert REC.itemsize == 56
CHUNK, N = 4 << 20, 4096
SEED = 0x3F5C3C00
OUT_FIELDS = ("out_size", "out_checksum", "out_checksum_type", "checksum_case", "status")


def dev_records(rec, dev):
    return torch.from_numpy(rec.view(np.uint8).copy()).to(dev)


def host_records(t):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=REC)


def timed(fn, calls, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(calls):
        fn()
    e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(variants, reps, calls, s, warm=3):
    for fn in variants.values():  # warm-up: first-use kernel loads, scratch growth, the apply's hint
        for _ in range(warm):
            fn()
    s.synchronize()
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            out[k].append(timed(fn, calls, s))
    return out


def line(bench, variant, shape, v, box, **more):
    d = {"bench": bench, "variant": variant, "shape": shape, "ms_per_batch": round(statistics.median(v), 4),
         "min": round(min(v), 4), "max": round(max(v), 4), "runs": [round(x, 4) for x in v], "box": box}
    d.update(more)
    return d


def same_images(a, b, out_size, dev, slab=256):
    """bytes [0, out_size[i]) of chunk i equal in the arenas a and b."""
    col = torch.arange(CHUNK, device=dev, dtype=torch.int32)
    for i0 in range(0, N, slab):
        sz = torch.tensor(out_size[i0:i0 + slab].astype(np.int32), device=dev)
        x = a[i0 * CHUNK:(i0 + slab) * CHUNK].view(-1, CHUNK)
        y = b[i0 * CHUNK:(i0 + slab) * CHUNK].view(-1, CHUNK)
        if bool(((x != y) & (col[None, :] < sz[:, None])).any().item()):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "update_cow_ab.jsonl"))
    ap.add_argument("--only", choices=["cow", "inplace", "syncing", "d3loop"], default=None)
    ap.add_argument("--parent-lib", default=None, help="another build of libhf3fs_crc.so for the in-place A/B")
    ap.add_argument("--branch-first", action="store_true", help="in-place A/B: this build takes the first turn")
    ap.add_argument("--variants", default=None, help="comma list of cow variants to time (a kernel trace of one)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(dev)
    rng = np.random.default_rng(3)
    box = torch.cuda.get_device_name(0)
    mode = hf.MODE_DELTA
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    D2D = 3
    lines = []
    shape = "4096 distinct 4 MiB chunks, U[64 KiB, 1 MiB], DELTA"
    with torch.cuda.stream(s):
        chunks = torch.empty(N * CHUNK, dtype=torch.uint8, device=dev)
        payload = torch.empty(N * CHUNK, dtype=torch.uint8, device=dev)
        L.fill_synth(chunks, CHUNK, CHUNK, N, SEED, 0, stream=s)
        L.fill_synth(payload, CHUNK, CHUNK, N, SEED ^ 0xABCD, 0, stream=s)
        sizes = rng.integers(2 << 20, CHUNK + 1, N).astype(np.int64)
        src_addr = (chunks.data_ptr() + np.arange(N) * CHUNK).astype(np.uint64)
        pay_addr = (payload.data_ptr() + np.arange(N) * CHUNK).astype(np.uint64)
        A = torch.tensor(src_addr.view(np.int64), device=dev)
        P = torch.tensor(pay_addr.view(np.int64), device=dev)
        cks = torch.zeros(N, dtype=torch.int32, device=dev)
        L.create_batch(hf.CRC32C, A, torch.tensor(sizes, device=dev), cks, N, CHUNK, stream=s)

        def payload_checksums(lens):
            out = torch.zeros(N, dtype=torch.int32, device=dev)
            L.create_batch(hf.CRC32C, P, torch.tensor(lens.astype(np.int64), device=dev), out, N, CHUNK, stream=s)
            s.synchronize()
            return out.cpu().numpy().astype(np.uint32)

        def records(base, offs, lens, pck, flags=0):
            r = np.zeros(N, dtype=REC)
            r["chunk"], r["payload"] = base, pay_addr
            r["offset"], r["length"], r["chunk_size"] = offs, lens, sizes
            r["update_type"], r["chunk_checksum_type"], r["write_checksum_type"] = hf.UPDATE_WRITE, hf.CRC32C, hf.CRC32C
            r["chunk_checksum"], r["write_checksum"], r["flags"] = ck_h, pck, flags
            return r

        s.synchronize()
        ck_h = cks.cpu().numpy().astype(np.uint32)
        lens = rng.integers(64 << 10, (1 << 20) + 1, N)
        offs = np.array([rng.integers(0, CHUNK - l + 1) for l in lens])
        pck = payload_checksums(lens)

        if a.only in (None, "cow", "syncing"):
            dest = torch.zeros(N * CHUNK, dtype=torch.uint8, device=dev)
            dst_addr = (dest.data_ptr() + np.arange(N) * CHUNK).astype(np.uint64)
            d_dst = torch.tensor(dst_addr.view(np.int64), device=dev)

        # ---- cow: out of place, three ways ----------------------------------------------------------
        if a.only in (None, "cow"):
            ios_a = dev_records(records(src_addr, offs, lens, pck), dev)   # chunk = the old version
            ios_b = dev_records(records(dst_addr, offs, lens, pck), dev)   # chunk = the copy
            copy_bytes = [int(x) for x in sizes]
            srcs, dsts = [int(x) for x in src_addr], [int(x) for x in dst_addr]
            st = ctypes.c_void_p(s.cuda_stream)

            def run_a():
                L.update_cow(hf.CRC32C, ios_a, d_dst, N, CHUNK, mode=mode, stream=s)

            def run_b():
                for i in range(N):
                    hip.hipMemcpyAsync(dsts[i], srcs[i], copy_bytes[i], D2D, st)
                L.update_batch(hf.CRC32C, ios_b, N, CHUNK, mode=mode, stream=s)

            def run_c():
                hip.hipMemcpyAsync(dest.data_ptr(), chunks.data_ptr(), N * CHUNK, D2D, st)
                L.update_batch(hf.CRC32C, ios_b, N, CHUNK, mode=mode, stream=s)

            results = {}
            for name, fn, ios in (("a", run_a, ios_a), ("b", run_b, ios_b), ("c", run_c, ios_b)):
                dest.zero_()
                fn()
                s.synchronize()
                results[name] = (host_records(ios), dest.clone() if name != "c" else dest)
            ra, rb, rc = results["a"][0], results["b"][0], results["c"][0]
            fields_same = all(np.array_equal(ra[f], rb[f]) and np.array_equal(ra[f], rc[f]) for f in OUT_FIELDS)
            all_ok = bool((ra["status"] == 0).all())
            whole_ab = bool(torch.equal(results["a"][1], results["b"][1]))  # both write [0, out_size) of zeroed chunks
            images_ac = same_images(results["a"][1], results["c"][1], ra["out_size"], dev)
            del results
            variants = {"update_cow_batch": run_a, "memcpy_per_chunk+update_batch": run_b,
                        "memcpy_arena+update_batch": run_c}
            if a.variants:
                variants = {k: v for k, v in variants.items() if k in set(a.variants.split(","))}
            t = alternate(variants, a.reps, a.calls, s)
            old_bytes = int(sizes.sum())
            under = int(np.maximum(np.minimum(offs + lens, sizes) - np.minimum(offs, sizes), 0).sum())
            for k, v in t.items():
                lines.append(line("cow", k, shape, v, box, reps=a.reps, calls=a.calls, records_equal=fields_same,
                                  all_ok=all_ok, arenas_equal_a_b=whole_ab, images_equal_a_c=images_ac,
                                  old_bytes=old_bytes, old_bytes_under_writes=under, payload_bytes=int(lens.sum())))
            del ios_a, ios_b

        # ---- syncing: whole-chunk resync ----------------------------------------------------------------
        if a.only in (None, "syncing"):
            full = np.full(N, CHUNK)
            pck_full = payload_checksums(full)
            ios_s = dev_records(records(src_addr, np.zeros(N, dtype=np.int64), full, pck_full, flags=hf.FLAG_SYNCING), dev)
            expected = torch.tensor(pck_full.view(np.int32), device=dev)
            mism = torch.zeros(N, dtype=torch.uint8, device=dev)
            count = torch.zeros(1, dtype=torch.int32, device=dev)
            st = ctypes.c_void_p(s.cuda_stream)

            def run_sync():
                L.update_cow(hf.CRC32C, ios_s, d_dst, N, CHUNK, mode=mode, stream=s)

            def run_verify_copy():
                L.verify_strided(hf.CRC32C, payload, CHUNK, CHUNK, N, expected, mism, count, stream=s)
                hip.hipMemcpyAsync(dest.data_ptr(), payload.data_ptr(), N * CHUNK, D2D, st)

            dest.zero_()
            run_sync()
            s.synchronize()
            rs = host_records(ios_s)
            good = bool((rs["status"] == 0).all() and (rs["out_size"] == CHUNK).all() and
                        np.array_equal(rs["out_checksum"], pck_full) and torch.equal(dest, payload))
            t = alternate({"update_cow_batch_syncing": run_sync, "verify_strided+memcpy_arena": run_verify_copy},
                          a.reps, a.calls, s)
            for k, v in t.items():
                lines.append(line("syncing", k, "4096 x 4 MiB whole-chunk resync, out of place", v, box, reps=a.reps,
                                  calls=a.calls, correct=good))
            del ios_s

        # ---- d3loop: the in-place d3 batch of the loaded library, for a kernel trace ---------------------------
        if a.only == "d3loop":
            ios = dev_records(records(src_addr, offs, lens, pck), dev)
            t = alternate({os.path.basename(os.environ.get("HF3FS_CRC_LIB") or "branch"):
                           lambda: L.update_batch(hf.CRC32C, ios, N, CHUNK, mode=mode, stream=s)}, a.runs, a.calls, s)
            for k, v in t.items():
                lines.append(line("d3loop", k, shape, v, box, calls=a.calls))

        # ---- inplace: this build against another one ---------------------------------------------------------------
        if a.only in (None, "inplace") and a.parent_lib:
            if a.only is not None:
                dest = torch.zeros(N * CHUNK, dtype=torch.uint8, device=dev)
                dst_addr = (dest.data_ptr() + np.arange(N) * CHUNK).astype(np.uint64)
                d_dst = torch.tensor(dst_addr.view(np.int64), device=dev)
            other = ctypes.CDLL(a.parent_lib)
            sizing = ("hf3fs_crc_update_scratch_bytes", "hf3fs_crc_update_ordered_scratch_bytes",
                      "hf3fs_crc_update_cow_scratch_bytes")
            for name in ("hf3fs_crc_update_batch", "hf3fs_crc_create_strided", "hf3fs_crc_update_cow_batch") + sizing:
                res, args = L.SIGNATURES[name]
                getattr(other, name).restype, getattr(other, name).argtypes = res, args
            mine = L.load()
            # the scratch a call asks for, both builds: (n, max_len) x mode x the three sizing functions
            for n_, ml in ((1, 4 << 10), (256, 1 << 20), (4096, 4 << 20)):
                for m in (hf.MODE_REFERENCE, hf.MODE_DELTA):
                    got = {k: [int(lib.hf3fs_crc_update_scratch_bytes(n_, m)),
                               int(lib.hf3fs_crc_update_ordered_scratch_bytes(n_, ml, m, 4)),
                               int(lib.hf3fs_crc_update_cow_scratch_bytes(n_, ml, m))]
                           for k, lib in (("parent", other), ("branch", mine))}
                    lines.append({"bench": "scratch_bytes", "n": n_, "max_len": ml, "mode": int(m),
                                  "functions": [f[len("hf3fs_crc_"):] for f in sizing], "parent": got["parent"],
                                  "branch": got["branch"], "equal": got["parent"] == got["branch"], "box": box})
            ios = dev_records(records(src_addr, offs, lens, pck), dev)
            ios_cow = dev_records(records(src_addr, offs, lens, pck), dev)  # chunk = the old version, image in dest
            out = torch.zeros(N, dtype=torch.int32, device=dev)
            st = s.cuda_stream

            def d3(lib):
                return lambda: lib.hf3fs_crc_update_batch(hf.CRC32C, ios.data_ptr(), N, CHUNK, mode, st)

            def headline(lib):
                return lambda: lib.hf3fs_crc_create_strided(hf.CRC32C, chunks.data_ptr(), CHUNK, CHUNK, N, 0xFFFFFFFF,
                                                            out.data_ptr(), st)

            def small(lib):  # a latency-bound batch: the first 256 records (prep, hashes and apply barely fill the chip)
                return lambda: lib.hf3fs_crc_update_batch(hf.CRC32C, ios.data_ptr(), 256, CHUNK, mode, st)

            def cow(lib):  # variant A of the cow section: d3's batch out of place
                return lambda: lib.hf3fs_crc_update_cow_batch(hf.CRC32C, ios_cow.data_ptr(), d_dst.data_ptr(), N, CHUNK,
                                                              mode, st)

            for bench, make in (("inplace_d3_delta", d3), ("inplace_small_delta", small), ("inplace_headline", headline),
                                ("cow_d3_delta", cow)):
                pair = {"parent": make(other), "branch": make(mine)}
                if a.branch_first:
                    pair = dict(reversed(list(pair.items())))
                t = alternate(pair, a.runs, a.calls, s)
                for k, v in t.items():
                    what = {"inplace_d3_delta": shape, "inplace_small_delta": "256 of those IOs, DELTA",
                            "inplace_headline": "create_strided 4096 x 4 MiB",
                            "cow_d3_delta": shape + ", update_cow_batch out of place"}[bench]
                    lines.append(line(bench, k, what, v, box, calls=a.calls, first_turn=next(iter(pair)), gb_per_s=round(N * CHUNK / statistics.median(v) / 1e6, 1)
                                      if bench.endswith("headline") else None))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")
            print(json.dumps(d))


if __name__ == "__main__":
    main()
