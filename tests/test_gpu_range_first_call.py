"""hf3fs_crc_range_query and hf3fs_crc_file_length as a fresh process's first library calls, inside one
stream capture: the context, the device tables and range_query's scratch are first allocated during
the capture.  The child replays the graph once; every op, every file, both d_info arrays and the list
are the model's (tests/range_cases.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import range_cases as rc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST_CAP = 4096

_CHILD = r"""
import importlib, json, sys
import numpy as np, torch
repo, tests, path = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path[:0] = [repo, tests]
hf = importlib.import_module("3fs_amd")
z = np.load(path)
dev = torch.device("cuda:0")
meta = torch.from_numpy(z["meta"].copy()).to(dev)
ops = torch.from_numpy(z["ops"].copy()).to(dev)
files = torch.from_numpy(z["files"].copy()).to(dev)
n_meta, n_ops, n_files, cap = meta.numel() // 48, ops.numel() // 96, files.numel() // 64, int(z["cap"])
info = torch.full((8,), -1, dtype=torch.int32, device=dev)
finfo = torch.full((8,), -1, dtype=torch.int32, device=dev)
lst = torch.full((4 * cap,), 0x5A, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library calls, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            st = torch.cuda.current_stream()
            hf.range_query(meta, n_meta, ops, n_ops, info, lst, cap, stream=st)
            hf.file_length(ops, n_ops, files, n_files, finfo, stream=st)
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "a range call failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
u32 = lambda t: t.cpu().numpy().view(np.uint32).tolist()
print(json.dumps({"ops": ops.cpu().numpy().tolist(), "files": files.cpu().numpy().tolist(), "info": u32(info),
                  "finfo": u32(finfo), "list": lst.cpu().numpy().tolist(), "meta": meta.cpu().numpy().tolist()}))
"""


def test_first_calls_in_process_are_captured(tmp_path):
    rng = np.random.default_rng(0xF125)
    meta = rc.random_table(rng, 1500, hi_values=(0x1234,), max_len=1 << 32)
    # every id of one inode: ChunkId(inode, 0, chunk) with chunk = id_lo's low word
    inode = (0x1234 << 16) | 0
    meta["id_lo"] &= np.uint64(0xFFFFFFFF)
    ops = rc.random_ops(rng, meta, 240, max_span=80)
    ops["chain_id"] = rng.integers(0, 12, 240)
    files = rc.new_files(60)
    files["inode"], files["first_op"], files["n_file_ops"] = inode, 4 * np.arange(60), 4
    files["chunk_size"], files["stripe_size"] = 4096, 4
    path = str(tmp_path / "case.npz")
    np.savez(path, meta=meta.view(np.uint8), ops=ops.view(np.uint8), files=files.view(np.uint8), cap=LIST_CAP)
    want, want_files = ops.copy(), files.copy()
    info, lst = rc.range_query(meta, want, LIST_CAP)
    finfo = rc.file_length(want, want_files)
    assert info[4] > 500 and info[1] > 5 and finfo[0] > 20 and finfo[1] > 5 and (want_files["length"] > 0).sum() > 20
    p = subprocess.run([sys.executable, "-c", _CHILD, REPO, os.path.join(REPO, "tests"), path],
                       capture_output=True, text=True, timeout=150, env=dict(os.environ), cwd=REPO)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    got = lines[0]
    have = np.array(got["ops"], dtype=np.uint8).view(rc.OP)
    for f in rc.OP.names:
        assert np.array_equal(have[f], want[f]), f
    have_f = np.array(got["files"], dtype=np.uint8).view(rc.FILE)
    for f in rc.FILE.names:
        assert np.array_equal(have_f[f], want_files[f]), f
    assert got["info"] == info and got["finfo"] == [int(x) for x in finfo]
    have_l = np.array(got["list"], dtype=np.uint8)
    assert np.array_equal(have_l[:4 * lst.size].view(np.uint32), lst) and (have_l[4 * lst.size:] == 0x5A).all()
    assert bytes(got["meta"]) == meta.tobytes()
