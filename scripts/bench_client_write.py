#!/usr/bin/env python3
"""hf3fs_crc_client_write_prepare / _complete on an MI355X: records appended to
profiles/client_write.jsonl.

  prepare_4m   4,096 IOs x 4 MiB, prepare(VERIFY) with update records.
  prepare_mix  --ios IOs (1 Mi) of 4, 8, 16, 32 or 64 KiB.
               The bar of both is hf3fs_crc_create_batch over the same bytes with its pointer and
               length lists already on the device, timed in the same process.  The new call
               hashes through the same range kernels, so it should sit within the bar's own
               run-to-run spread, (max - min) / median over --reps repetitions; both times, the
               ratio and the spread are in the record, `within_spread` says whether the ratio kept
               to 1 + spread, and the script exits 1 when it did not.  With HF3FS_CRC_LIB naming a
               library built from the parent commit only the bar is timed (record `bar_only`), to
               show that the bar itself has not moved.
  complete     --ios IOs in files of 32, complete(FROM_UPDATES) with expected values and the failed
               list, against the sequential host loop on one core over the same records (the fold
               vectorised over the files, one pass per IO position, the CPU oracle's combine_batch
               on one thread; the records copied back first, as a host without the call must).
               Reported only.
Every digest and every status of a batch is checked once outside the timed region: prepare's
against create_batch's values and, for a sample, the CPU oracle; complete's against the host loop.
Every timing: HIP events, a warm-up call before each timed region, the median of --reps calls.

    python scripts/bench_client_write.py
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
CRC32C = hf.CRC32C
HAS_NEW = hasattr(L.load(), "hf3fs_crc_client_write_prepare")


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


def shape_prepare(name, lens, args, dev):
    import oracle
    oracle.lib()
    n = lens.size
    offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    total = int(lens.sum())
    arena = random_arena(total, dev)
    addrs = (offs + arena.data_ptr()).astype(np.uint64)
    max_len = int(lens.max())
    d_addr, d_len = up(addrs, dev), up(lens.astype(np.uint64), dev)
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    bar = timed(lambda: L.create_batch(CRC32C, d_addr, d_len, out, n, max_len, stream=st), args.reps)
    torch.cuda.synchronize()
    values = out.cpu().numpy().view(np.uint32)
    sample = np.random.default_rng(1).choice(n, min(n, 8 if max_len > (1 << 20) else 64), replace=False)
    oracle_ok = all(int(values[i]) == oracle.create(CRC32C, arena[int(offs[i]):int(offs[i] + lens[i])].cpu().numpy().tobytes())[1]
                    for i in sample)
    bar_ms = float(np.median(bar))
    spread = (max(bar) - min(bar)) / bar_ms
    line = dict(record=name, ios=n, bytes=total, reps=args.reps, create_batch_ms=bar_ms, create_batch_all_ms=bar,
                create_batch_gb_s=total / bar_ms / 1e6, bar_spread=spread, oracle_sample_ok=bool(oracle_ok),
                bar_only=not HAS_NEW)
    if not HAS_NEW:
        line["exact"] = bool(oracle_ok)
        return line
    ios = np.zeros(n, dtype=hf.client_write_io_dtype())
    ios["data"], ios["buf_base"], ios["buf_size"] = addrs, arena.data_ptr(), total
    ios["length"], ios["chunk_size"] = lens, max_len
    d_ios = up(ios, dev)
    d_upd = torch.zeros(n * 56, dtype=torch.uint8, device=dev)
    info = torch.zeros(8, dtype=torch.int32, device=dev)
    new = timed(lambda: hf.client_write_prepare(CRC32C, d_ios, n, info, max_len, max_inline_bytes=4096, verify=True,
                                                updates=d_upd, stream=st), args.reps)
    torch.cuda.synchronize()
    got = d_ios.cpu().numpy().view(ios.dtype)
    upd = d_upd.cpu().numpy().view(hf.update_io_dtype())
    inline = int((lens <= 4096).sum())
    exact = (oracle_ok and (got["status"] == 0).all() and np.array_equal(got["checksum"], values)
             and (got["checksum_type"] == CRC32C).all() and np.array_equal(got["send_inline"], lens <= 4096)
             and np.array_equal(upd["write_checksum"], values) and np.array_equal(upd["payload"], addrs)
             and (upd["update_type"] == 1).all()
             and info.cpu().numpy().view(np.uint32).tolist() == [n, 0, 0, 0, inline, total & 0xFFFFFFFF, total >> 32, 0])
    new_ms = float(np.median(new))
    line.update(client_write_prepare_ms=new_ms, client_write_prepare_all_ms=new,
                client_write_prepare_gb_s=total / new_ms / 1e6, ratio=new_ms / bar_ms, allowed_ratio=1 + spread,
                within_spread=bool(new_ms / bar_ms <= 1 + spread), exact=bool(exact))
    return line


def host_fold(ios, per, expected, orc):
    """writeFile's loop over records whose files all have `per` IOs, vectorised over the files; the
    answers here are all typed CRC32C or failed, which is what the benchmark's batch holds."""
    final = np.where(ios["status"] != 0, ios["status"], ios["status_in"]).reshape(-1, per)
    value = ios["result_checksum"].reshape(-1, per)
    rlen = ios["result_len"].reshape(-1, per).astype(np.uint64)
    short = rlen != ios["length"].reshape(-1, per)
    code = np.where(final != 0, final, np.where(short, 33, 0))
    ended = code != 0
    first = np.where(ended.any(axis=1), ended.argmax(axis=1), per)
    acc = value[:, 0].copy()
    for j in range(1, per):
        acc = orc.combine_batch(acc, value[:, j], rlen[:, j], threads=1)
    files = np.zeros(final.shape[0], dtype=hf.client_write_file_dtype())
    ok = first == per
    rows = np.arange(final.shape[0])
    files["length"] = np.where(ok, rlen.sum(axis=1), 0)
    files["value"], files["type"] = np.where(ok, acc, 0), np.where(ok, CRC32C, 0)
    files["status"] = np.where(ok, 0, code[rows, np.minimum(first, per - 1)])
    files["failed_io"] = np.where(ok, 0xFFFFFFFF, rows * per + first)
    miss = ok & (files["value"] != expected)
    files["status"] = np.where(miss, 7015, files["status"])
    failed = np.flatnonzero(final.reshape(-1) != 0).astype(np.uint32)
    good = final.reshape(-1) == 0
    data_len = int(ios["result_len"][good].astype(np.uint64).sum())
    info = [int(failed.size), int(good.sum()), data_len & 0xFFFFFFFF, data_len >> 32, int((files["status"] != 0).sum()),
            int(miss.sum()), 0, 0]
    return files, failed, info


def shape_complete(args, dev):
    import oracle
    oracle.lib()
    rng = np.random.default_rng(8)
    per = 32
    n = args.ios // per * per
    nf = n // per
    ios = np.zeros(n, dtype=hf.client_write_io_dtype())
    ios["length"] = rng.integers(1, 1 << 22, n)
    ios["status_in"] = 7003
    ios["status"][rng.choice(n, n // 5000, replace=False)] = 7002
    upd = np.zeros(n, dtype=hf.update_io_dtype())
    upd["length"], upd["out_checksum"], upd["out_checksum_type"] = ios["length"], rng.integers(0, 1 << 32, n), CRC32C
    upd["status"][rng.choice(n, n // 5000, replace=False)] = 4080
    answered = ios.copy()
    sent = ios["status"] == 0
    for f, g in (("status_in", "status"), ("result_len", "length"), ("result_checksum", "out_checksum"),
                 ("result_checksum_type", "out_checksum_type")):
        answered[f] = np.where(sent, upd[g], ios[f])
    want_files, want_failed, want_info = host_fold(answered, per, np.zeros(nf, dtype=np.uint32), oracle)
    expected = want_files["value"].copy()
    expected[rng.choice(nf, 8, replace=False)] ^= 4
    d_ios, d_upd, d_exp = up(ios, dev), up(upd, dev), up(expected, dev)
    d_off = up(np.arange(nf + 1, dtype=np.uint64) * per, dev)
    files = torch.zeros(nf * 24, dtype=torch.uint8, device=dev)
    failed = torch.zeros(n, dtype=torch.int32, device=dev)
    info = torch.zeros(8, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    new = timed(lambda: hf.client_write_complete(d_ios, n, info, file_off=d_off, n_files=nf, max_ios_per_file=per,
                                                 updates=d_upd, expected=d_exp, files=files, failed=failed, failed_cap=n,
                                                 stream=st), args.reps)
    torch.cuda.synchronize()
    host = []
    for _ in range(max(3, args.reps // 3)):
        t0 = time.perf_counter()
        back = d_ios.cpu().numpy().view(ios.dtype)       # (the answers are in the records after the call)
        t1 = time.perf_counter()
        want_files, want_failed, want_info = host_fold(back, per, expected, oracle)
        host.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    got_files = files.cpu().numpy().view(want_files.dtype)
    got_failed = failed.cpu().numpy().view(np.uint32)[:want_failed.size]
    exact = (np.array_equal(d_ios.cpu().numpy().view(ios.dtype), answered) and got_files.tobytes() == want_files.tobytes()
             and np.array_equal(got_failed, want_failed) and info.cpu().numpy().view(np.uint32).tolist() == want_info)
    new_ms = float(np.median(new))
    copy_ms, fold_ms = (float(x) for x in np.median(np.array(host), axis=0))
    return dict(record="complete", ios=n, files=nf, ios_per_file=per, reps=args.reps, client_write_complete_ms=new_ms,
                client_write_complete_all_ms=new, host_copy_back_ms=copy_ms, host_loop_ms=fold_ms,
                speedup_over_host_loop=(copy_ms + fold_ms) / new_ms, failed_ios=int(want_failed.size),
                failed_files=want_info[4], mismatched_files=want_info[5], exact=bool(exact))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "client_write.jsonl"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--records", default="prepare_4m,prepare_mix,complete")
    ap.add_argument("--ios", type=int, default=1 << 20)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    assert args.reps >= 10, "the spread is taken over at least 10 repetitions"
    dev = torch.device("cuda:0")
    common = {"device": torch.cuda.get_device_name(0), "library": L.load().hf3fs_crc_version().decode(), "tag": args.tag}
    ok = True
    for name in args.records.split(","):
        if name == "complete":
            if not HAS_NEW:
                continue
            line = shape_complete(args, dev)
        elif name == "prepare_4m":
            line = shape_prepare(name, np.full(4096, 4 << 20, dtype=np.int64), args, dev)
        else:
            line = shape_prepare(name, (4096 << np.random.default_rng(5).integers(0, 5, args.ios)).astype(np.int64), args, dev)
        line = dict(line, **common)
        print(json.dumps(line), flush=True)
        ok &= line["exact"] and line.get("within_spread", True)  # (complete is reported only)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
