"""What a chunk-engine queue costs as one hf3fs_crc_update_engine call.

1024 chunks of 4 MiB, each with the queue U C U C (max_rounds 4): 2048 engine writes U[64 KiB,
1 MiB] inside the committed length, so every one copies on write into a destination of its own,
DELTA.  Variants, alternated inside ONE process after a warm-up and timed with stream events
around `--calls` calls, `--reps` repetitions each (median, min, max):

  update_engine       the queue in one call, nothing decided on the host
  two_cow_batches     the same 2048 writes as two hf3fs_crc_update_cow_batch calls of 1024 IOs with
                      d_dst and the second batch's chunk state prepared on the host beforehand: what
                      a host that ALREADY KNEW the outcome of the first batch would submit.  The
                      real alternative adds a synchronize and a read-back between the two.

One JSON line to --out (default profiles/update_engine.jsonl).
"""
import argparse
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
N, W = C * D, C * D // 2
SEED = 0x3F5C3C00


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "update_engine.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(dev)
    rng = np.random.default_rng(3)
    mode = hf.MODE_DELTA
    with torch.cuda.stream(s):
        chunks = torch.empty(C * CHUNK, dtype=torch.uint8, device=dev)
        dsts = torch.empty(W * CHUNK, dtype=torch.uint8, device=dev)
        payload = torch.empty(W * SLOT, dtype=torch.uint8, device=dev)
        L.fill_synth(chunks, CHUNK, CHUNK, C, SEED, 0, stream=s)
        L.fill_synth(payload, SLOT, SLOT, W, SEED ^ 0xABCD, 0, stream=s)
        sizes = rng.integers(2 << 20, CHUNK + 1, C).astype(np.int64)
        A = torch.tensor((chunks.data_ptr() + np.arange(C) * CHUNK).astype(np.uint64).view(np.int64), device=dev)
        P = torch.tensor((payload.data_ptr() + np.arange(W) * SLOT).astype(np.uint64).view(np.int64), device=dev)
        cks = torch.zeros(C, dtype=torch.int32, device=dev)
        L.create_batch(hf.CRC32C, A, torch.tensor(sizes, device=dev), cks, C, CHUNK, stream=s)
        lens = rng.integers(64 << 10, (1 << 20) + 1, W)
        offs = np.array([rng.integers(0, (2 << 20) - ln + 1) for ln in lens])  # inside every committed length
        pck = torch.zeros(W, dtype=torch.int32, device=dev)
        L.create_batch(hf.CRC32C, P, torch.tensor(lens.astype(np.int64), device=dev), pck, W, SLOT, stream=s)
        s.synchronize()
        pck = pck.cpu().numpy().astype(np.uint32)
        caddr = chunks.data_ptr() + np.arange(C).astype(np.uint64) * np.uint64(CHUNK)
        daddr = dsts.data_ptr() + np.arange(W).astype(np.uint64) * np.uint64(CHUNK)
        paddr = payload.data_ptr() + np.arange(W).astype(np.uint64) * np.uint64(SLOT)

        # job k * C + c is chunk c's k-th job: U (write k / 2), C, U, C
        rec = np.zeros(N, dtype=REC)
        jobs = np.zeros(N, dtype=L.engine_job_dtype())
        rec["chunk"] = np.tile(caddr, D)
        rec["flags"], rec["chunk_checksum_type"] = hf.FLAG_ENGINE, hf.CRC32C
        jobs["job_chain_ver"] = 3
        for k in range(D):
            sl = slice(k * C, (k + 1) * C)
            if k % 2:
                rec["update_type"][sl] = hf.UPDATE_COMMIT
                continue
            w = slice((k // 2) * C, (k // 2 + 1) * C)
            rec["update_type"][sl], rec["write_checksum_type"][sl] = hf.UPDATE_WRITE, hf.CRC32C
            rec["payload"][sl], rec["offset"][sl], rec["length"][sl] = paddr[w], offs[w], lens[w]
            rec["write_checksum"][sl], jobs["dst"][sl] = pck[w], daddr[w]
        rec["chunk_size"][:C], rec["chunk_checksum"][:C] = sizes, cks.cpu().numpy().astype(np.uint32)
        jobs["addr"][:C], jobs["chain_ver"][:C], jobs["chunk_ver"][:C] = caddr, 3, 4
        ios, jr = to_dev(rec, dev), to_dev(jobs, dev)
        info = torch.zeros(8, dtype=torch.int32, device=dev)

        # the two batches a host that knew the first one's outcome would submit
        L.update_engine(hf.CRC32C, ios, jr, N, CHUNK, D, mode=mode, info=info, stream=s)
        s.synchronize()
        done = np.frombuffer(ios.cpu().numpy().tobytes(), dtype=REC)
        batch = []
        for k in (0, 2):
            b = done[k * C:(k + 1) * C].copy()
            b["chunk"] = caddr if k == 0 else daddr[:C]  # the second write reads the first one's image
            d = daddr[(k // 2) * C:(k // 2 + 1) * C].view(np.int64)
            batch.append((to_dev(b, dev), torch.tensor(d, device=dev)))

        def two_batches():
            for b, d in batch:
                L.update_cow(hf.CRC32C, b, d, C, CHUNK, mode=mode, stream=s)

        variants = {
            "update_engine": lambda: L.update_engine(hf.CRC32C, ios, jr, N, CHUNK, D, mode=mode, info=info, stream=s),
            "two_cow_batches": two_batches,
        }
        t = alternate(variants, a.reps, a.calls, s)
        variants["update_engine"]()
        s.synchronize()
        st = np.frombuffer(ios.cpu().numpy().tobytes(), dtype=REC)["status"]
        words = info.cpu().numpy().tolist()
        checks = {"engine_all_ok": bool((st == 0).all()) and words == [D, 0, W, W, 0, W, 0, 0]}
        two = [np.frombuffer(b.cpu().numpy().tobytes(), dtype=REC) for b, _ in batch]
        checks["same_checksums"] = all(
            bool((x["out_checksum"] == done["out_checksum"][k * C:(k + 1) * C]).all() and (x["status"] == 0).all())
            for x, k in zip(two, (0, 2)))
    line = {"bench": "update_engine vs two update_cow_batch calls prepared with hindsight",
            "shape": "1024 x 4 MiB chunks x (U C U C), writes U[64 KiB, 1 MiB] copy-on-write, DELTA, max_rounds 4",
            "reps": a.reps, "calls_per_rep": a.calls, "box": torch.cuda.get_device_name(0),
            "date": time.strftime("%Y-%m-%d"), "written_bytes": int(lens.sum()), **checks}
    for k in variants:
        line[k] = stats(t[k])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    sys.exit(0 if all(v is not False for v in checks.values()) else 1)


if __name__ == "__main__":
    main()
