#!/usr/bin/env python3
"""Host time per call of four entry points of the host layer: one record of profiles/host_layer.jsonl.

The time for the call to return with the stream idle (synchronize, clock, call, clock), after 50
warm-up calls, as the median of 1,000 calls, for hf3fs_crc_scrub_batch, hf3fs_crc_forward_prepare
(whole-chunk writes to SYNCING successors), hf3fs_crc_client_write_prepare with VERIFY and
hf3fs_crc_update_ordered with max_rounds = 4, each over n = 256 records of 4 KiB.  One process
measures one build of the library (HF3FS_CRC_LIB names another one); --label tags the record.  An
A/B runs this script in fresh processes, one at a time, alternating the builds.

    python scripts/bench_host_layer.py --label new
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
sys.path[:0] = [REPO]
hf = importlib.import_module("3fs_amd")
L = hf._lib
N, LEN = 256, 4096
SCRUB = np.dtype([("data", "<u8"), ("length", "<u4"), ("checksum_type", "u1"), ("fin", "u1"), ("reserved", "<u2"),
                  ("checksum", "<u4"), ("computed", "<u4"), ("status", "<i4"), ("reserved2", "<u4")])


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def host_us(call, warmup, reps):
    for _ in range(warmup):
        call()
    us = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter_ns()
        call()
        us.append((time.perf_counter_ns() - t0) / 1e3)
    torch.cuda.synchronize()
    return float(np.median(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="new")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=1000)
    args = ap.parse_args()
    L.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    chunks = torch.empty(N * LEN, dtype=torch.uint8, device=dev).random_(0, 256)
    payload = torch.empty(N * LEN, dtype=torch.uint8, device=dev).random_(0, 256)
    c_addr = (np.arange(N, dtype=np.uint64) * LEN + chunks.data_ptr()).astype(np.uint64)
    p_addr = (np.arange(N, dtype=np.uint64) * LEN + payload.data_ptr()).astype(np.uint64)
    c_val = torch.zeros(N, dtype=torch.int32, device=dev)
    p_val = torch.zeros(N, dtype=torch.int32, device=dev)
    L.create_strided(hf.CRC32C, chunks, LEN, LEN, N, c_val, stream=st)
    L.create_strided(hf.CRC32C, payload, LEN, LEN, N, p_val, stream=st)
    torch.cuda.synchronize()
    c_val, p_val = c_val.cpu().numpy().view(np.uint32), p_val.cpu().numpy().view(np.uint32)

    scrub = np.zeros(N, dtype=SCRUB)
    scrub["data"], scrub["length"], scrub["checksum_type"], scrub["checksum"] = c_addr, LEN, hf.CRC32C, c_val
    d_scrub, count = up(scrub, dev), torch.zeros(1, dtype=torch.int32, device=dev)

    jobs = np.zeros(N, dtype=hf.forward_job_dtype())
    jobs["update_type"], jobs["payload"], jobs["length"], jobs["chunk_size"] = hf.UPDATE_WRITE, p_addr, LEN, LEN
    jobs["req_update_ver"] = jobs["upd_update_ver"] = 5
    jobs["upd_commit_ver"], jobs["upd_length"] = 4, LEN
    jobs["req_checksum_type"] = jobs["upd_checksum_type"] = hf.CRC32C
    jobs["chain_ver"], jobs["has_successor"], jobs["successor_syncing"] = 7, 1, 1
    jobs["chunk"], jobs["chunk_len"], jobs["chunk_checksum_type"] = c_addr, LEN, hf.CRC32C
    jobs["chunk_checksum"], jobs["chunk_update_ver"] = c_val, 5
    d_jobs, f_info = up(jobs, dev), torch.zeros(hf.FORWARD_INFO_WORDS, dtype=torch.int32, device=dev)

    wio = np.zeros(N, dtype=hf.client_write_io_dtype())
    wio["data"], wio["buf_base"], wio["buf_size"] = p_addr, payload.data_ptr(), N * LEN
    wio["length"], wio["chunk_size"], wio["checksum"], wio["checksum_type"] = LEN, LEN, p_val, hf.CRC32C
    d_wio, w_info = up(wio, dev), torch.zeros(hf.CLIENT_WRITE_INFO_WORDS, dtype=torch.int32, device=dev)

    uio = np.zeros(N, dtype=hf.update_io_dtype())
    uio["chunk"], uio["payload"], uio["length"], uio["chunk_size"] = c_addr, p_addr, LEN, LEN
    uio["update_type"], uio["chunk_checksum_type"], uio["write_checksum_type"] = hf.UPDATE_WRITE, hf.CRC32C, hf.CRC32C
    uio["chunk_checksum"], uio["write_checksum"] = c_val, p_val
    d_uio, u_info = up(uio, dev), torch.zeros(2, dtype=torch.int32, device=dev)

    calls = {
        "scrub_batch": lambda: L.scrub_batch(hf.CRC32C, d_scrub, N, LEN, count, stream=st),
        "forward_prepare": lambda: hf.forward_prepare(hf.CRC32C, d_jobs, N, f_info, LEN, stream=st),
        "client_write_prepare": lambda: hf.client_write_prepare(hf.CRC32C, d_wio, N, w_info, LEN, verify=True, stream=st),
        "update_ordered": lambda: L.update_ordered(hf.CRC32C, d_uio, N, LEN, 4, info=u_info, stream=st),
    }
    rec = dict(record="host_us", label=args.label, lib=os.path.basename(L.LIB_PATH), n=N, length=LEN,
               warmup=args.warmup, reps=args.reps)
    for name, call in calls.items():
        rec[name] = host_us(call, args.warmup, args.reps)
    torch.cuda.synchronize()
    # what the calls left: no scrub mismatch, every job and IO sent, the ordered call's info words
    rec["scrub_mismatches"] = int(count.item())
    rec["forward_info"] = f_info.cpu().numpy().tolist()[:6]
    rec["client_write_info"] = w_info.cpu().numpy().tolist()[:6]
    rec["ordered_info"] = u_info.cpu().numpy().tolist()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
