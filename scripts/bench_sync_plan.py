"""Time hf3fs_crc_sync_plan against the sequential host loop it replaces.

Tables: tests/sync_cases.large_tables -- the remote table is a fixed permutation of the local one
in which about 1 % of the chunks differ (every 400th record: an id the local table lacks, a lower
chain version, an uncommitted remote, a checksum that differs), so the expected plan is known in
closed form and the device result is checked against it before anything is timed.

  device   one plan of n x n records, device-resident tables: a warm-up, then stream events around
           `--calls` calls, `--reps` times.
  host     the sequential restatement of the reference loop in tests/cpp/fuzz_sync_plan.cpp
           (unordered_map of the local table, walk, erase), compiled here with g++ -O2 and run on
           the same tables on this machine's CPU (best of three, map build included: the reference
           builds its map per resync too).

One JSON line per size to --out (default profiles/sync_plan.jsonl).
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import sync_cases as sc  # noqa: E402

hf = importlib.import_module("3fs_amd")
L = hf._lib
SIZES = {"1M": 1_000_003, "8M": 8_000_009}


def timed(fn, calls, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(calls):
        fn()
    e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / calls


def host_loop(exe, local, remote, tmp):
    lp, rp = os.path.join(tmp, "local.bin"), os.path.join(tmp, "remote.bin")
    local.tofile(lp)
    remote.tofile(rp)
    out = subprocess.run([exe, "--time", lp, rp, str(sc.LARGE_CHAIN_VER), "0"], capture_output=True, text=True,
                         check=True, timeout=600).stdout
    os.remove(lp)
    os.remove(rp)
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1M,8M")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--every", type=int, default=400, help="4 of every `every` remote records differ")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sync_plan.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(dev)
    box = torch.cuda.get_device_name(0)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = None
        if not a.no_host:
            exe = os.path.join(tmp, "fuzz_sync_plan")
            subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(REPO, "tests", "cpp", "fuzz_sync_plan.cpp"),
                                   "-o", exe])
        for name in a.sizes.split(","):
            n = SIZES[name]
            local, remote, want = sc.large_tables(n, n, every=a.every)
            with torch.cuda.stream(s):
                d_local = torch.from_numpy(local.view(np.uint8)).to(dev)
                d_remote = torch.from_numpy(remote.view(np.uint8)).to(dev)
                write = torch.zeros(n, dtype=torch.int32, device=dev)
                remove = torch.zeros(n, dtype=torch.int32, device=dev)
                info = torch.zeros(16, dtype=torch.int32, device=dev)

                def plan():
                    L.sync_plan(d_local, n, d_remote, n, sc.LARGE_CHAIN_VER, info, write=write, remove=remove, stream=s)

                for _ in range(3):  # warm-up: code objects, the pair's scratch
                    plan()
                s.synchronize()
                got = dict(zip(sc.INFO, (int(x) for x in info.cpu().numpy().view(np.uint32))))
                correct = (got == want.info and
                           np.array_equal(write.cpu().numpy().view(np.uint32)[:want.write.size], want.write) and
                           np.array_equal(remove.cpu().numpy().view(np.uint32)[:want.remove.size], want.remove) and
                           np.array_equal(np.frombuffer(d_remote.cpu().numpy().tobytes(), dtype=sc.META)["out_class"],
                                          want.rclass))
                runs = [timed(plan, a.calls, s) for _ in range(a.reps)]
            d = {"bench": "sync_plan", "name": f"sync_plan_{name}",
                 "shape": f"{n} x {n} records, 4 of every {a.every} remote records differ", "n_local": n, "n_remote": n, "device_ms_per_plan": round(statistics.median(runs), 4),
                 "min": round(min(runs), 4), "max": round(max(runs), 4), "runs": [round(x, 4) for x in runs],
                 "reps": a.reps, "calls": a.calls, "correct": bool(correct), "n_write": got["n_write"],
                 "n_remove": got["n_remove"], "scratch_bytes": L.sync_plan_scratch_bytes(n, n), "box": box}
            if exe:
                h = host_loop(exe, local, remote, tmp)
                d["host_loop_ms"] = h["host_loop_ms"]
                d["host_agrees"] = (h["fatal"], h["n_write"], h["n_remove"]) == (0, got["n_write"], got["n_remove"])
                d["host_cpus"] = os.cpu_count()
            lines.append(d)
            del d_local, d_remote, write, remove
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")
            print(json.dumps(d))


if __name__ == "__main__":
    main()
