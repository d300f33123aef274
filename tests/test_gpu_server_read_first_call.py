"""hf3fs_crc_server_read_prepare and hf3fs_crc_server_read_complete as a fresh process's first library
calls, inside one stream capture: the context, the device tables and complete's scratch are first
allocated during the capture.  The child replays the graph once; every record, both d_info arrays,
the inline arena and the RDMA list are the model's (tests/server_read_cases.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import server_read_cases as sc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEN, SMALL, BIG, SLOT = 8192, 4096, 12288, 3 * 4096

_CHILD = r"""
import importlib, json, sys
import numpy as np, torch
repo, tests, path = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path[:0] = [repo, tests]
hf = importlib.import_module("3fs_amd")
z = np.load(path)
dev = torch.device("cuda:0")
arena = torch.from_numpy(z["arena"]).to(dev)
jobs_h = z["jobs"].copy().view(hf.server_read_job_dtype())
jobs_h["localbuf"] = np.where(jobs_h["localbuf"] != 0, jobs_h["localbuf"] + np.uint64(arena.data_ptr()), 0)
jobs = torch.from_numpy(jobs_h.view(np.uint8).copy()).to(dev)
reqs = torch.from_numpy(z["reqs"].copy()).to(dev)
ro = torch.from_numpy(z["ro"].copy()).to(dev)
n, n_reqs, cap = jobs_h.size, int(z["ro"].size) - 1, int(z["cap"])
pinfo = torch.full((8,), -1, dtype=torch.int32, device=dev)
cinfo = torch.full((8,), -1, dtype=torch.int32, device=dev)
inline = torch.full((cap,), 0x5A, dtype=torch.uint8, device=dev)
wr = torch.full((n * 32,), 0x5A, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library calls, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            st = torch.cuda.current_stream()
            hf.server_read_prepare(jobs, n, reqs, ro, n_reqs, pinfo, int(z["small"]), int(z["big"]), stream=st)
            hf.server_read_complete(int(z["ctype"]), jobs, n, reqs, ro, n_reqs, cinfo, int(z["max_len"]), inline=inline,
                                    inline_cap=cap, wr=wr, wr_cap=n, stream=st)
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "a server read call failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
u32 = lambda t: t.cpu().numpy().view(np.uint32).tolist()
print(json.dumps({"jobs": jobs.cpu().numpy().tolist(), "reqs": reqs.cpu().numpy().tolist(), "pinfo": u32(pinfo),
                  "cinfo": u32(cinfo), "inline": inline.cpu().numpy().tolist(), "wr": wr.cpu().numpy().tolist(),
                  "base": arena.data_ptr()}))
"""


def test_first_calls_in_process_are_captured(orc, tmp_path):
    rng = np.random.default_rng(0x5E1257)
    arena = rng.integers(0, 256, 20 * SLOT, dtype=np.uint8)
    counts = [3, 0, 40, 1, 21]
    n = sum(counts)
    jobs, reqs, ro = sc.new_jobs(n), sc.new_reqs(len(counts)), sc.offsets(counts)
    reqs["xmit"] = [sc.XMIT_INLINE, sc.XMIT_RDMA, sc.XMIT_RDMA, sc.XMIT_NONE, sc.XMIT_INLINE]
    reqs["recalculate"] = [1, 0, 1, 1, 0]
    jobs["offset"] = np.where(np.arange(n) % 2 == 0, 0, rng.integers(0, 8192, n))
    jobs["length"] = rng.choice([0, 1, 15, 16, 17, 1000, 4095, 4096, 4097], n)
    jobs["chunk_len"] = jobs["offset"] + jobs["length"] - np.where(np.arange(n) % 5 == 0, jobs["length"] // 3, 0)
    jobs["chunk_checksum_type"] = sc.CRC32C
    jobs["engine"] = np.arange(n) % 4 == 1
    # arena-relative addresses from 4096 on (0 stays 0: no buffer); the child adds the arena's base
    jobs["localbuf"] = 4096 + (np.arange(n) % 19) * SLOT + np.arange(n) % 16
    jobs["res"] = np.where(np.arange(n) % 11 == 3, -5, 12288)
    jobs["update_ver_now"][7] = 5
    jobs["meta_status"][9] = sc.CHUNK_METADATA_NOT_FOUND
    read = lambda a, ln: arena[a:a + ln].tobytes()  # noqa: E731
    for i in np.flatnonzero(jobs["offset"] == 0):
        j = jobs[i]
        value = orc.create(sc.CRC32C, read(int(j["localbuf"]), int(j["chunk_len"])))[1] ^ (1 if i % 6 == 4 else 0)
        j["chunk_checksum"] = value ^ 0xFFFFFFFF if j["engine"] else value
    cap = int(jobs["length"].sum())
    path = str(tmp_path / "case.npz")
    np.savez(path, arena=arena, jobs=jobs.view(np.uint8), reqs=reqs.view(np.uint8), ro=ro, ctype=sc.CRC32C,
             max_len=MAX_LEN, small=SMALL, big=BIG, cap=cap)
    want_j, want_r = jobs.copy(), reqs.copy()
    pinfo = sc.prepare(want_j, want_r, ro, SMALL, BIG)
    cinfo, inline, wr = sc.complete(want_j, want_r, ro, sc.CRC32C, MAX_LEN, read, orc, cap)
    assert cinfo[0] > n // 2 and cinfo[7] > 5 and wr.size > 10 and len(inline) > 4096 and 4080 in want_j["result_status"]
    p = subprocess.run([sys.executable, "-c", _CHILD, REPO, os.path.join(REPO, "tests"), path],
                       capture_output=True, text=True, timeout=150, env=dict(os.environ), cwd=REPO)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    got = lines[0]
    base = np.uint64(got["base"])
    want_j["localbuf"] = np.where(want_j["localbuf"] != 0, want_j["localbuf"] + base, 0)
    wr["local_addr"] += base
    have = np.array(got["jobs"], dtype=np.uint8).view(sc.JOB)
    for f in sc.JOB.names:
        assert np.array_equal(have[f], want_j[f]), f
    have_r = np.array(got["reqs"], dtype=np.uint8).view(sc.REQ)
    for f in sc.REQ.names:
        assert np.array_equal(have_r[f], want_r[f]), f
    assert got["pinfo"] == pinfo and got["cinfo"] == cinfo
    assert bytes(got["inline"][:len(inline)]) == inline and set(got["inline"][len(inline):]) <= {0x5A}
    have_wr = np.array(got["wr"], dtype=np.uint8)
    assert have_wr[:wr.nbytes].tobytes() == wr.tobytes() and (have_wr[wr.nbytes:] == 0x5A).all()
