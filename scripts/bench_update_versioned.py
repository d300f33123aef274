"""What the version ladder costs on top of hf3fs_crc_update_ordered.

The d3 shape's queue -- 4096 IOs, writes U[64 KiB, 1 MiB] on 4 MiB chunks, DELTA -- arranged as
1024 chunks x 4 jobs, max_rounds 4.  Variants, alternated inside ONE process after a warm-up and
timed with stream events around `--calls` calls, `--reps` repetitions each (median, min, max):

  update_versioned          version records that admit every job
  update_ordered            the same queue without version records, this build
  parent_update_ordered     the same call of the parent commit's library (--parent-lib), the bar:
                            the expectation is the parent's median plus no more than the parent's
                            own max - min spread
  update_versioned_10pct    the same queue with 10 % of the jobs refused at rung 6 (a stale
                            io_ver, good payload): the deferred verify hashes their payloads

One JSON line per record to --out (default profiles/update_versioned.jsonl): the first compares
the three calls on the admitting queue, the second puts the refusing queue beside them.
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
hf = importlib.import_module("3fs_amd")
L = hf._lib

REC = np.dtype([("chunk", "<u8"), ("payload", "<u8"), ("offset", "<u4"), ("length", "<u4"), ("chunk_size", "<u4"),
                ("update_type", "u1"), ("chunk_checksum_type", "u1"), ("write_checksum_type", "u1"), ("flags", "u1"),
                ("chunk_checksum", "<u4"), ("write_checksum", "<u4"), ("out_size", "<u4"), ("out_checksum", "<u4"),
                ("out_checksum_type", "u1"), ("checksum_case", "u1"), ("reserved1", "u1", (2,)), ("status", "<i4")])
CHUNK, SLOT, C, D = 4 << 20, 1 << 20, 1024, 4
N = C * D
SEED = 0x3F5C3C00
CLEAN = 2


def to_dev(a, dev):
    return torch.from_numpy(a.view(np.uint8).copy()).to(dev)


def timed(fn, calls, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(calls):
        fn()
    e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(variants, reps, calls, s):
    for fn in variants.values():  # warm-up: first-use kernel loads, scratch growth, the apply's hint
        for _ in range(3):
            fn()
    s.synchronize()
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            out[k].append(timed(fn, calls, s))
    return out


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "spread_ms": round(max(v) - min(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "update_versioned.jsonl"))
    ap.add_argument("--parent-lib", default=None, help="libhf3fs_crc.so built from the parent commit")
    ap.add_argument("--variants", default=None, help="comma list of variants to run (a kernel trace of one)")
    ap.add_argument("--note", default=None, help="free text stored with both records (e.g. what a kernel trace showed)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(dev)
    rng = np.random.default_rng(3)
    mode = hf.MODE_DELTA
    with torch.cuda.stream(s):
        chunks = torch.empty(C * CHUNK, dtype=torch.uint8, device=dev)
        payload = torch.empty(N * SLOT, dtype=torch.uint8, device=dev)
        L.fill_synth(chunks, CHUNK, CHUNK, C, SEED, 0, stream=s)
        L.fill_synth(payload, SLOT, SLOT, N, SEED ^ 0xABCD, 0, stream=s)
        sizes = rng.integers(2 << 20, CHUNK + 1, C).astype(np.int64)
        A = torch.tensor((chunks.data_ptr() + np.arange(C) * CHUNK).astype(np.uint64).view(np.int64), device=dev)
        P = torch.tensor((payload.data_ptr() + np.arange(N) * SLOT).astype(np.uint64).view(np.int64), device=dev)
        cks = torch.zeros(C, dtype=torch.int32, device=dev)
        L.create_batch(hf.CRC32C, A, torch.tensor(sizes, device=dev), cks, C, CHUNK, stream=s)
        lens = rng.integers(64 << 10, (1 << 20) + 1, N)
        offs = np.array([rng.integers(0, CHUNK - ln + 1) for ln in lens])
        pck = torch.zeros(N, dtype=torch.int32, device=dev)
        L.create_batch(hf.CRC32C, P, torch.tensor(lens.astype(np.int64), device=dev), pck, N, SLOT, stream=s)
        s.synchronize()
        # job k * C + c is chunk c's k-th job
        rec = np.zeros(N, dtype=REC)
        cid = np.tile(np.arange(C), D)
        rec["chunk"] = chunks.data_ptr() + cid.astype(np.uint64) * np.uint64(CHUNK)
        rec["payload"] = payload.data_ptr() + np.arange(N).astype(np.uint64) * np.uint64(SLOT)
        rec["offset"], rec["length"] = offs, lens
        rec["update_type"], rec["chunk_checksum_type"], rec["write_checksum_type"] = hf.UPDATE_WRITE, hf.CRC32C, hf.CRC32C
        rec["write_checksum"] = pck.cpu().numpy().astype(np.uint32)
        rec["chunk_size"][:C], rec["chunk_checksum"][:C] = sizes, cks.cpu().numpy().astype(np.uint32)

        def ver_records(refuse):
            """io_ver = update_ver + 1 down each chain; a refused job repeats the chain's update_ver
            (kChunkStaleUpdate) and the chain goes on from the same version."""
            v = np.zeros(N, dtype=L.update_ver_dtype())
            v["job_chain_ver"], v["chain_ver"], v["meta_chunk_size"], v["chunk_state"] = 3, 3, CHUNK, CLEAN
            v["update_ver"], v["commit_ver"] = 7, 5
            uv = np.full(C, 7)
            for k in range(D):
                r = refuse[k * C:(k + 1) * C]
                v["io_ver"][k * C:(k + 1) * C] = np.where(r, uv, uv + 1)
                uv = uv + (~r)
            return v

        none = np.zeros(N, dtype=bool)
        tenth = np.random.default_rng(10).random(N) < 0.10
        ios = to_dev(rec, dev)
        ios_t = to_dev(rec, dev)
        ver_all, ver_10 = to_dev(ver_records(none), dev), to_dev(ver_records(tenth), dev)
        info = torch.zeros(8, dtype=torch.int32, device=dev)
        info_t = torch.zeros(8, dtype=torch.int32, device=dev)
        variants = {
            "update_versioned": lambda: L.update_versioned(hf.CRC32C, ios, ver_all, N, CHUNK, D, mode=mode, info=info,
                                                           stream=s),
            "update_ordered": lambda: L.update_ordered(hf.CRC32C, ios, N, CHUNK, D, mode=mode, info=info, stream=s),
            "update_versioned_10pct": lambda: L.update_versioned(hf.CRC32C, ios_t, ver_10, N, CHUNK, D, mode=mode,
                                                                 info=info_t, stream=s),
        }
        if a.parent_lib:
            parent = ctypes.CDLL(a.parent_lib)
            f = parent.hf3fs_crc_update_ordered
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                          ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]

            def run_parent():
                rc = f(hf.CRC32C, ios.data_ptr(), N, CHUNK, mode, D, info.data_ptr(), s.cuda_stream)
                assert rc == 0, rc

            variants["parent_update_ordered"] = run_parent
        if a.variants:
            variants = {k: fn for k, fn in variants.items() if k in set(a.variants.split(","))}
        t = alternate(variants, a.reps, a.calls, s)
        # what the last calls left: every job applied / a tenth refused as kChunkStaleUpdate
        checks = {}
        if "update_versioned" in variants:
            variants["update_versioned"]()
            s.synchronize()
            st = np.frombuffer(ios.cpu().numpy().tobytes(), dtype=REC)["status"]
            checks["versioned_all_ok"] = bool((st == 0).all()) and info.cpu().numpy().tolist()[:5] == [D, 0, N, 0, 0]
        if "update_versioned_10pct" in variants:
            st = np.frombuffer(ios_t.cpu().numpy().tobytes(), dtype=REC)["status"]
            checks["refused_are_4006"] = bool(((st == 4006) == tenth).all() and (st[~tenth] == 0).all())
            checks["refused_jobs"] = int(tenth.sum())
            checks["refused_payload_bytes"] = int(lens[tenth].sum())
    box = torch.cuda.get_device_name(0)
    common = {"shape": "1024 x 4 MiB chunks x 4 jobs, writes U[64 KiB, 1 MiB], DELTA, max_rounds 4", "reps": a.reps,
              "calls_per_rep": a.calls, "box": box, "date": time.strftime("%Y-%m-%d"), **checks}
    if a.note:
        common["note"] = a.note
    first = {"bench": "update_versioned vs update_ordered vs the parent's update_ordered", **common}
    for k in ("update_versioned", "update_ordered", "parent_update_ordered"):
        if k in t:
            first[k] = stats(t[k])
    if "parent_update_ordered" in t and "update_versioned" in t:
        bar = first["parent_update_ordered"]["median_ms"] + first["parent_update_ordered"]["spread_ms"]
        first["bar_ms"] = round(bar, 4)
        first["excess_over_parent_median_ms"] = round(first["update_versioned"]["median_ms"] -
                                                      first["parent_update_ordered"]["median_ms"], 4)
        first["within_bar"] = first["update_versioned"]["median_ms"] <= bar
    second = {"bench": "update_versioned with 10 % of the jobs refused at rung 6", **common}
    for k in ("update_versioned_10pct", "update_versioned"):
        if k in t:
            second[k] = stats(t[k])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in (first, second):
            fh.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))
    sys.exit(0 if all(v is not False for v in checks.values()) else 1)


if __name__ == "__main__":
    main()
