"""hf3fs_crc_forward_prepare and hf3fs_crc_forward_complete as a fresh process's first library calls,
inside one stream capture: the context, the device tables and both calls' scratch are first
allocated during the capture.  The child replays the graph once; every record, both d_info arrays
and the commit list are the model's (tests/forward_cases.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import forward_cases as fc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEN, MAX_INLINE, N = 4096, 64, 65

_CHILD = r"""
import importlib, json, sys
import numpy as np, torch
repo, tests, path = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path[:0] = [repo, tests]
hf = importlib.import_module("3fs_amd")
z = np.load(path)
dev = torch.device("cuda:0")
arena = torch.from_numpy(z["arena"]).to(dev)
jobs_h = z["jobs"].copy().view(hf.forward_job_dtype())
for f in ("payload", "chunk"):
    jobs_h[f] = np.where(jobs_h[f] != 0, jobs_h[f] + np.uint64(arena.data_ptr()), 0)
jobs = torch.from_numpy(jobs_h.view(np.uint8).copy()).to(dev)
n = jobs_h.size
pinfo = torch.full((8,), -1, dtype=torch.int32, device=dev)
dinfo = torch.full((8,), -1, dtype=torch.int32, device=dev)
idx = torch.full((n,), -1, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library calls, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            st = torch.cuda.current_stream()
            hf.forward_prepare(int(z["ctype"]), jobs, n, pinfo, int(z["max_len"]), int(z["max_inline"]), stream=st)
            hf.forward_complete(int(z["ctype"]), jobs, n, dinfo, int(z["max_len"]), commit_idx=idx, stream=st)
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "a forward call failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
u32 = lambda t: t.cpu().numpy().view(np.uint32).tolist()
print(json.dumps({"jobs": jobs.cpu().numpy().tolist(), "pinfo": u32(pinfo), "dinfo": u32(dinfo), "idx": u32(idx),
                  "base": arena.data_ptr()}))
"""


def test_first_calls_in_process_are_captured(orc, tmp_path):
    rng = np.random.default_rng(0xF1257)
    arena = rng.integers(0, 256, 80 << 10, dtype=np.uint8)
    # arena-relative addresses from 4096 on (0 stays 0: no buffer); the child adds the arena's base
    lens = [0, 1, 15, 16, 17, 4095, 4096]
    chunks = [4096 + 4608 * k + (0, 1, 15)[k % 3] for k in range(7)]
    pays = [4096 + 4608 * (7 + k) + (15, 0, 1)[k % 3] for k in range(7)]
    cks = lambda at: [tuple(orc.create(fc.CRC32C, arena[a:a + n].tobytes())) for a, n in zip(at, lens)]  # noqa: E731
    jobs = fc.random_jobs(rng, N, fc.CRC32C, chunks, lens, cks(chunks), pays, lens, cks(pays), max_len=MAX_LEN)
    read = lambda a, n: arena[a:a + n].tobytes()  # noqa: E731
    prepared, _ = fc.model_prepare(jobs, fc.CRC32C, MAX_LEN, MAX_INLINE, orc, read)
    answered = fc.random_answers(rng, prepared.copy(), fc.CRC32C)
    for k in fc.RESPONSE:      # the answers are in place before the graph runs: prepare leaves a sent job's alone
        jobs[k] = answered[k]
    prepared, pinfo = fc.model_prepare(jobs, fc.CRC32C, MAX_LEN, MAX_INLINE, orc, read)
    done, commits, dinfo = fc.model_complete(prepared, fc.CRC32C, MAX_LEN, orc, read)
    assert pinfo[3] > 0 and commits.size > 5
    path = str(tmp_path / "case.npz")
    np.savez(path, arena=arena, jobs=jobs.view(np.uint8), ctype=fc.CRC32C, max_len=MAX_LEN, max_inline=MAX_INLINE)
    p = subprocess.run([sys.executable, "-c", _CHILD, REPO, os.path.join(REPO, "tests"), path],
                       capture_output=True, text=True, timeout=150, env=dict(os.environ), cwd=REPO)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    got = lines[0]
    want = done.copy()
    for f in ("payload", "chunk", "out_data"):
        want[f] = np.where(done[f] != 0, done[f] + np.uint64(got["base"]), 0)
    have = np.array(got["jobs"], dtype=np.uint8).view(fc.JOB)
    for f in fc.JOB.names:
        assert np.array_equal(have[f], want[f]), f
    assert got["pinfo"] == pinfo.tolist() and got["dinfo"] == dinfo.tolist()
    assert got["idx"][:commits.size] == commits.tolist() and set(got["idx"][commits.size:]) <= {0xFFFFFFFF}
