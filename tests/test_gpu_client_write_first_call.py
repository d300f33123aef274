"""hf3fs_crc_client_write_prepare and hf3fs_crc_client_write_complete as a fresh process's first
library calls, inside one stream capture: the context, the device tables and both calls' scratch
are first allocated during the capture.  The child replays the graph once; every IO record, the
update records, the file records, the failed list and both d_info arrays are the model's
(tests/client_write_cases.py).  The answers stand in the IO records before the graph runs (the
host's part between the two calls), so complete runs without FROM_UPDATES."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import client_write_cases as wc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEN, MAX_INLINE, ARENA = 4097, 64, 1 << 16

_CHILD = r"""
import importlib, json, sys
import numpy as np, torch
repo, tests, path = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path[:0] = [repo, tests]
hf = importlib.import_module("3fs_amd")
z = np.load(path)
dev = torch.device("cuda:0")
arena = torch.from_numpy(z["arena"]).to(dev)
ios_h = z["ios"].copy().view(hf.client_write_io_dtype())
for f in ("data", "buf_base"):
    ios_h[f] = np.where(ios_h[f] != 0, ios_h[f] + np.uint64(arena.data_ptr()), 0)
ios = torch.from_numpy(ios_h.view(np.uint8).copy()).to(dev)
upd = torch.from_numpy(z["updates"].copy()).to(dev)
off = torch.from_numpy(z["off"].view(np.int64)).to(dev)
n, nf = ios_h.size, off.numel() - 1
files = torch.full((nf * 24,), 0x5A, dtype=torch.uint8, device=dev)
failed = torch.full((n,), -1, dtype=torch.int32, device=dev)
pinfo = torch.full((8,), -1, dtype=torch.int32, device=dev)
dinfo = torch.full((8,), -1, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library calls, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            st = torch.cuda.current_stream()
            hf.client_write_prepare(int(z["ctype"]), ios, n, pinfo, int(z["max_len"]), max_inline_bytes=int(z["max_inline"]),
                                    verify=True, updates=upd, stream=st)
            hf.client_write_complete(ios, n, dinfo, file_off=off, n_files=nf, max_ios_per_file=int(z["max_ios"]),
                                     files=files, failed=failed, failed_cap=n, stream=st)
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "a client_write call failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
u32 = lambda t: t.cpu().numpy().view(np.uint32).tolist()
b = lambda t: t.cpu().numpy().view(np.uint8).tolist()
print(json.dumps({"ios": b(ios), "updates": b(upd), "files": b(files), "failed": u32(failed), "pinfo": u32(pinfo),
                  "dinfo": u32(dinfo), "base": arena.data_ptr()}))
"""


def test_first_calls_in_process_are_captured(orc, tmp_path):
    rng = np.random.default_rng(0xF1257)
    arena = wc.arena_bytes(ARENA, 0xF1257)
    # arena-relative addresses from 4096 on (0 stays 0: no buffer); the child adds the arena's base
    rows = []
    for k, ln in enumerate((0, 1, 15, 16, 17, 4095, 4096, 4097) * 8 + (40,)):
        rows.append((4096 + int(rng.integers(0, ARENA - 8400)) + k % 16, 4096, ARENA - 4096, 0, ln, 8192))
    rows[9] = rows[9][:3] + (8190, 15, 8192)      # leaves its chunk: 7002, alone
    rows[20] = rows[20][:4] + (5000, 8192)        # longer than max_len: 3
    ios = wc.ios_array(rows)
    counts = [0, 1, 17, 40, 7]
    read = lambda a, n: arena[a:a + n].tobytes()  # noqa: E731
    prep = wc.prepare_model(ios, wc.CRC32C, MAX_LEN, MAX_INLINE, True, orc, read)
    assert prep.status.tolist().count(0) == 63 and prep.info.tolist()[:4] == [63, 1, 1, 0] and 0 < prep.info[4] < 63
    answers = [(0, int(ios["length"][i]), (wc.CRC32C, int(rng.integers(0, 1 << 32)))) for i in range(ios.size)]
    answers[30] = (4080, 0, (wc.NONE, 0))
    answers[50] = (0, int(ios["length"][50]), (wc.CRC32, 5))
    sent = wc.with_answers(ios, -2, answers)      # prepare's outputs still poisoned: the graph writes them
    before = np.frombuffer(bytes(range(0x40, 0x40 + 56)) * ios.size, dtype=wc.UPDATE).copy()
    done = wc.complete_model(wc.with_answers(prep.apply(ios), prep.status, answers), wc.offsets_of(counts), orc)
    assert done.failed.tolist() == [9, 20, 30] and done.files["status"].tolist() == [0, 0, 7002, 3, 0]
    path = str(tmp_path / "case.npz")
    np.savez(path, arena=arena, ios=sent.view(np.uint8), updates=before.view(np.uint8), off=wc.offsets_of(counts),
             ctype=wc.CRC32C, max_len=MAX_LEN, max_inline=MAX_INLINE, max_ios=max(counts))
    p = subprocess.run([sys.executable, "-c", _CHILD, REPO, os.path.join(REPO, "tests"), path],
                       capture_output=True, text=True, timeout=150, env=dict(os.environ), cwd=REPO)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    got = lines[0]
    moved = ios.copy()
    for f in ("data", "buf_base"):
        moved[f] = ios[f] + np.uint64(got["base"])
    want = wc.with_answers(prep.apply(moved), prep.status, answers)
    have = np.array(got["ios"], dtype=np.uint8).view(wc.IO)
    for f in wc.IO.names:
        assert np.array_equal(have[f], want[f]), f
    assert np.array(got["updates"], dtype=np.uint8).tobytes() == prep.updates(moved, before).tobytes()
    assert np.array(got["files"], dtype=np.uint8).tobytes() == done.files.tobytes()
    assert got["failed"][:3] == [9, 20, 30] and set(got["failed"][3:]) == {0xFFFFFFFF}
    assert got["pinfo"] == prep.info.tolist() and got["dinfo"] == done.info.tolist()
