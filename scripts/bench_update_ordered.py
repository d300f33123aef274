"""A/B of hf3fs_crc_update_ordered against what a caller could do before it.

Two questions, each answered by alternating the variants inside ONE process (box-to-box spread
is 3-8 %), after a warm-up, timed with stream events around `--calls` calls:

  overhead   d3's batch -- 4096 DISTINCT 4 MiB chunks, writes U[64 KiB, 1 MiB], DELTA: what does
             the ordered call cost when there is nothing to order?  update_batch vs
             update_ordered(max_rounds = 1) vs update_ordered(max_rounds = 4) on the same records.
  chains     4096 IOs as 1024 chunks x 4 sequential IOs: update_ordered(max_rounds = 4) (A) vs
             the caller-side planner (B): four update_batch calls of 1024 pre-split IOs with a
             device-side copy of {out_size, out_checksum} into the next wave's records between
             them (tests/bench_suite.py's chain_in).  A and B must leave equal chunk checksums,
             equal to the oracle's on a seeded sample of 64 chunks.

One JSON line per variant to --out (default profiles/update_ordered_ab.jsonl).
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
sys.path[:0] = [REPO, os.path.join(REPO, "oracle")]
hf = importlib.import_module("3fs_amd")
L = hf._lib

REC = np.dtype([("chunk", "<u8"), ("payload", "<u8"), ("offset", "<u4"), ("length", "<u4"), ("chunk_size", "<u4"),
                ("update_type", "u1"), ("chunk_checksum_type", "u1"), ("write_checksum_type", "u1"), ("flags", "u1"),
                ("chunk_checksum", "<u4"), ("write_checksum", "<u4"), ("out_size", "<u4"), ("out_checksum", "<u4"),
                ("out_checksum_type", "u1"), ("checksum_case", "u1"), ("reserved1", "u1", (2,)), ("status", "<i4")])
assert REC.itemsize == 56
W = REC.itemsize // 4
COL_SIZE, COL_CK, COL_OUT_SIZE, COL_OUT_CK, COL_STATUS = (REC.fields[f][1] // 4 for f in (
    "chunk_size", "chunk_checksum", "out_size", "out_checksum", "status"))  # 32-bit columns of a record
CHUNK, SLOT, N = 4 << 20, 1 << 20, 4096
SEED = 0x3F5C3C00


def dev_records(rec, dev):
    return torch.from_numpy(rec.view(np.uint8).copy()).to(dev)


def cols(t, n):
    return t.view(torch.int32).view(n, W)


def timed(fn, calls, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(calls):
        fn()
    e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / calls


KEEP = None  # --variants


def alternate(variants, reps, calls, s):
    """{name: [ms per call, one figure per repetition]}, the variants taking turns."""
    if KEEP:
        variants = {k: fn for k, fn in variants.items() if k in KEEP}
    for fn in variants.values():  # warm-up: first-use kernel loads, scratch growth, the apply's hint
        for _ in range(3):
            fn()
    s.synchronize()
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            out[k].append(timed(fn, calls, s))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "update_ordered_ab.jsonl"))
    ap.add_argument("--only", choices=["overhead", "chains"], default=None)
    ap.add_argument("--variants", default=None, help="comma list of variant names to time (a kernel trace of one)")
    a = ap.parse_args()
    global KEEP
    KEEP = set(a.variants.split(",")) if a.variants else None
    import oracle
    oracle.lib()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(dev)
    rng = np.random.default_rng(3)
    box = torch.cuda.get_device_name(0)
    mode = hf.MODE_DELTA
    lines = []
    with torch.cuda.stream(s):
        chunks = torch.empty(N * CHUNK, dtype=torch.uint8, device=dev)
        payload = torch.empty(N * SLOT, dtype=torch.uint8, device=dev)
        L.fill_synth(chunks, CHUNK, CHUNK, N, SEED, 0, stream=s)
        L.fill_synth(payload, SLOT, SLOT, N, SEED ^ 0xABCD, 0, stream=s)
        sizes = rng.integers(2 << 20, CHUNK + 1, N).astype(np.int64)
        A = torch.tensor((chunks.data_ptr() + np.arange(N) * CHUNK).astype(np.uint64).view(np.int64), device=dev)
        P = torch.tensor((payload.data_ptr() + np.arange(N) * SLOT).astype(np.uint64).view(np.int64), device=dev)
        cks = torch.zeros(N, dtype=torch.int32, device=dev)
        L.create_batch(hf.CRC32C, A, torch.tensor(sizes, device=dev), cks, N, CHUNK, stream=s)

        def payload_checksums(lens):
            out = torch.zeros(N, dtype=torch.int32, device=dev)
            L.create_batch(hf.CRC32C, P, torch.tensor(lens.astype(np.int64), device=dev), out, N, SLOT, stream=s)
            s.synchronize()
            return out.cpu().numpy().astype(np.uint32)

        def records(chunk_ids, slots, offs, lens, size0, ck0, pck):
            r = np.zeros(len(chunk_ids), dtype=REC)
            r["chunk"] = chunks.data_ptr() + chunk_ids.astype(np.uint64) * np.uint64(CHUNK)
            r["payload"] = payload.data_ptr() + slots.astype(np.uint64) * np.uint64(SLOT)
            r["offset"], r["length"], r["chunk_size"] = offs, lens, size0
            r["update_type"], r["chunk_checksum_type"], r["write_checksum_type"] = hf.UPDATE_WRITE, hf.CRC32C, hf.CRC32C
            r["chunk_checksum"], r["write_checksum"] = ck0, pck
            return r

        s.synchronize()
        ck_h = cks.cpu().numpy().astype(np.uint32)
        pristine = chunks[:1024 * CHUNK].clone()  # the chains part starts from chunks that match ck_h

        # ---- overhead: d3's batch, nothing to order ------------------------------------------------
        if a.only in (None, "overhead"):
            lens = rng.integers(64 << 10, (1 << 20) + 1, N)
            offs = np.array([rng.integers(0, CHUNK - l + 1) for l in lens])
            ids = np.arange(N)
            ios = dev_records(records(ids, ids, offs, lens, sizes, ck_h, payload_checksums(lens)), dev)
            info = torch.zeros(2, dtype=torch.int32, device=dev)
            variants = {
                "update_batch": lambda: L.update_batch(hf.CRC32C, ios, N, CHUNK, mode=mode, stream=s),
                "update_ordered_r1": lambda: L.update_ordered(hf.CRC32C, ios, N, CHUNK, 1, mode=mode, info=info, stream=s),
                "update_ordered_r4": lambda: L.update_ordered(hf.CRC32C, ios, N, CHUNK, 4, mode=mode, info=info, stream=s),
            }
            t = alternate(variants, a.reps, a.calls, s)
            status_ok = bool((cols(ios, N)[:, COL_STATUS] == 0).all().item())
            base = statistics.median(t.get("update_batch", [0.0]))
            for k, v in t.items():
                lines.append({"bench": "overhead", "variant": k, "shape": "4096 distinct 4 MiB chunks, U[64 KiB, 1 MiB], DELTA",
                              "ms_per_batch": round(statistics.median(v), 4), "min": round(min(v), 4),
                              "max": round(max(v), 4), "diff_vs_update_batch_ms": round(statistics.median(v) - base, 4),
                              "spread_ms": round(max(v) - min(v), 4), "reps": a.reps, "calls": a.calls,
                              "all_ok": status_ok, "info": info.cpu().numpy().tolist(), "box": box})
            del ios

        # ---- chains: 1024 chunks x 4 sequential IOs -------------------------------------------------
        if a.only in (None, "chains"):
            C, D = 1024, 4
            size = sizes[:C].copy()
            waves = []
            for k in range(D):
                lens = rng.integers(64 << 10, (1 << 20) + 1, C)
                offs = np.array([rng.integers(0, CHUNK - l + 1) for l in lens])
                app = rng.random(C) < 0.25  # sequential appends among them
                fits = app & (size + lens <= CHUNK)
                offs[fits] = size[fits]
                waves.append((offs, lens))
                size = np.maximum(size, offs + lens)
            all_lens = np.concatenate([w[1] for w in waves])
            pck = payload_checksums(all_lens)
            ids = np.arange(C)
            wave_recs = [records(ids, k * C + ids, waves[k][0], waves[k][1], sizes[:C] if k == 0 else 0,
                                 ck_h[:C] if k == 0 else 0, pck[k * C:(k + 1) * C]) for k in range(D)]
            ord_ios = dev_records(np.concatenate(wave_recs), dev)  # IO k * C + c: chunk c's k-th IO
            wave_ios = [dev_records(r, dev) for r in wave_recs]
            info = torch.zeros(2, dtype=torch.int32, device=dev)

            def run_a():
                L.update_ordered(hf.CRC32C, ord_ios, C * D, CHUNK, D, mode=mode, info=info, stream=s)

            def run_b():  # the caller-side planner: pre-split waves + device-side metadata copies
                for k in range(D):
                    if k:
                        prev, cur = cols(wave_ios[k - 1], C), cols(wave_ios[k], C)
                        cur[:, COL_SIZE] = prev[:, COL_OUT_SIZE]
                        cur[:, COL_CK] = prev[:, COL_OUT_CK]
                    L.update_batch(hf.CRC32C, wave_ios[k], C, CHUNK, mode=mode, stream=s)

            chunks[:C * CHUNK].copy_(pristine)
            snap = pristine
            run_a()
            s.synchronize()
            fa = cols(ord_ios, C * D)[(D - 1) * C:, :].clone()
            bytes_a = chunks[:C * CHUNK].clone()
            chunks[:C * CHUNK].copy_(snap)
            run_b()
            s.synchronize()
            fb = cols(wave_ios[D - 1], C)
            same = bool((fa[:, COL_OUT_CK] == fb[:, COL_OUT_CK]).all().item() and
                        (fa[:, COL_OUT_SIZE] == fb[:, COL_OUT_SIZE]).all().item() and
                        (cols(ord_ios, C * D)[:, COL_STATUS] == 0).all().item() and
                        (fb[:, COL_STATUS] == 0).all().item() and torch.equal(bytes_a, chunks[:C * CHUNK]))
            del bytes_a
            if not same:  # say which part differs
                st_a = cols(ord_ios, C * D)[:, COL_STATUS].cpu().numpy()
                st_b = np.concatenate([cols(w, C)[:, COL_STATUS].cpu().numpy() for w in wave_ios])
                print("statuses A", dict(zip(*np.unique(st_a, return_counts=True))), "B",
                      dict(zip(*np.unique(st_b, return_counts=True))), "checksums differ",
                      int((fa[:, COL_OUT_CK] != fb[:, COL_OUT_CK]).sum().item()), "sizes differ",
                      int((fa[:, COL_OUT_SIZE] != fb[:, COL_OUT_SIZE]).sum().item()), file=sys.stderr)
            out_size =fa[:, COL_OUT_SIZE].cpu().numpy().astype(np.uint32)
            out_ck = fa[:, COL_OUT_CK].cpu().numpy().astype(np.uint32)
            oracle_ok = bool((out_size == size.astype(np.uint32)).all())
            for c in np.random.default_rng(64).choice(C, 64, replace=False):
                h = chunks[int(c) * CHUNK:int(c) * CHUNK + int(out_size[c])].cpu().numpy()
                oracle_ok = oracle_ok and oracle.crc32c_raw(h) == int(out_ck[c])
            chunks[:C * CHUNK].copy_(snap)
            t = alternate({"A_update_ordered_r4": run_a, "B_four_update_batch_waves": run_b}, a.reps, a.calls, s)
            base = statistics.median(t.get("B_four_update_batch_waves", [0.0]))
            for k, v in t.items():
                lines.append({"bench": "chains", "variant": k, "shape": "1024 x 4 MiB chunks x 4 sequential IOs, U[64 KiB, 1 MiB], DELTA",
                              "ms_per_queue": round(statistics.median(v), 4), "min": round(min(v), 4),
                              "max": round(max(v), 4), "diff_vs_B_ms": round(statistics.median(v) - base, 4),
                              "reps": a.reps, "calls": a.calls, "a_equals_b": same, "oracle_sample_64_ok": oracle_ok,
                              "info": info.cpu().numpy().tolist(), "box": box})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            ln["date"] = time.strftime("%Y-%m-%d")
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))
    bad = [ln for ln in lines if ln.get("all_ok") is False or ln.get("a_equals_b") is False
           or ln.get("oracle_sample_64_ok") is False]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
