"""The record reads of hf3fs_crc_range_query / hf3fs_crc_file_length against the load-checked build.

Run as a program (by tests/test_gpu_range_footprint.py, with HF3FS_CRC_LIB naming
libhf3fs_crc_loadcheck.so) it lays table, ops, files, list and info of every case out in one yard, arms
the check around each call and reports what the check logged.  The two calls load no chunk byte: every
load from d_meta and d_ops is a record load through the check's record hook, which refuses and logs
an index at or past the array's count (`desc`), so a binary search's probe at n_meta, the order
check's neighbour at -1 (an index of 2^64 - 1) or a list entry's op probe at n_ops would be counted.
The outputs are compared with the model's (tests/range_cases.py), so a refused load, which reads as
zeros, shows there too.
"""
import json
import os
import sys

import numpy as np

import range_cases as rc

TABLES = (1, 255, 257, 1000)
ALIGN = 4096


def cases():
    out = []
    for k, n in enumerate(TABLES):
        rng = np.random.default_rng(0xF007 + k)
        meta = rc.random_table(rng, n, hi_values=(0x1234,), max_len=1 << 32)
        meta["id_lo"] &= np.uint64(0xFFFFFFFF)  # ids of one inode (0x1234 << 16)
        meta["recycle_state"][-1] = 0
        ops = rc.random_ops(rng, meta, 257 if n != 255 else 64, max_span=70)
        ids = rc.table_ids(meta)
        # probes at both ends: ranges below the first id, above the last, and the whole table
        rc.set_range(ops[0], 0, ids[0])
        rc.set_range(ops[1], ids[-1] + 1, rc.ident(rc.M64, rc.M64))
        rc.set_range(ops[2], 0, rc.ident(rc.M64, rc.M64))
        rc.set_range(ops[3], ids[-1], ids[-1] + 1)
        ops["status_in"][:4], ops["kind"][:4], ops["max_chunks"][:4] = 0, rc.REMOVE, [0, 0, 3, 1]
        files = rc.new_files(ops.size // 4 + 1)
        files["inode"], files["first_op"], files["n_file_ops"] = 0x1234 << 16, 4 * np.arange(files.size), 4
        files["chunk_size"], files["stripe_size"] = 4096, 4
        files["first_op"][-1], files["n_file_ops"][-1] = ops.size - 1, 1  # the last op of the array
        out.append(dict(name=f"{n} records, {ops.size} ops", meta=meta, ops=ops, files=files, list_cap=3000))
    return out


def main(out_path):
    import ctypes
    import importlib
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    for p in (repo, here):
        if p not in sys.path:
            sys.path.insert(0, p)
    hf = importlib.import_module("3fs_amd")
    L = hf._lib
    lib = L.load()
    arm, disarm, units = lib.hf3fs_crc_loadcheck_arm, lib.hf3fs_crc_loadcheck_disarm, lib.hf3fs_crc_loadcheck_units
    arm.restype = disarm.restype = units.restype = ctypes.c_int
    arm.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    b = importlib.import_module("3fs_amd.build")
    assert "range_kernels.hip" in b.CHECK_SOURCES
    assert units() == len(b.CHECK_SOURCES) + len(b.CHECK_ONLY), units()   # no unit's copy of the state was lost
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    size = 1 << 20
    yard = torch.zeros(size, dtype=torch.uint8, device=dev)
    bitmap = torch.zeros(size // 16 // 32 + 1, dtype=torch.int32, device=dev)
    site_map = torch.zeros(size // 16, dtype=torch.uint8, device=dev)
    log = torch.zeros(36 + 6 * 64, dtype=torch.int32, device=dev)
    base = yard.data_ptr()
    reports = {}
    for case in cases():
        meta, ops, files, cap = case["meta"], case["ops"], case["files"], case["list_cap"]
        at, offs = 0, {}
        img = np.full(size, 0x5A, dtype=np.uint8)
        for name, nbytes in (("meta", meta.nbytes), ("ops", ops.nbytes), ("files", files.nbytes), ("list", 4 * cap),
                             ("info", 32), ("finfo", 32)):
            offs[name] = at
            at += (nbytes + ALIGN - 1) // ALIGN * ALIGN + ALIGN
        assert at <= size
        for name, arr in (("meta", meta), ("ops", ops), ("files", files)):
            img[offs[name]:offs[name] + arr.nbytes] = arr.view(np.uint8)
        want_ops, want_files = ops.copy(), files.copy()
        info, lst = rc.range_query(meta, want_ops, cap)
        finfo = rc.file_length(want_ops, want_files)
        yard.copy_(torch.from_numpy(img))
        bitmap.zero_(), site_map.zero_(), log.zero_()
        torch.cuda.synchronize()
        assert arm(base, size, bitmap.data_ptr(), site_map.data_ptr(), log.data_ptr()) == 0
        try:
            L.range_query(base + offs["meta"], meta.size, base + offs["ops"], ops.size, base + offs["info"],
                          base + offs["list"], cap, stream=stream)
            L.file_length(base + offs["ops"], ops.size, base + offs["files"], files.size, base + offs["finfo"],
                          stream=stream)
            torch.cuda.synchronize()
        finally:
            assert disarm() == 0
        got = yard.cpu().numpy()
        outputs = "ok"
        keep = np.ones(size, dtype=bool)
        for what, name, want in (("the ops", "ops", want_ops.tobytes()), ("the files", "files", want_files.tobytes()),
                                 ("the list", "list", lst.tobytes()),
                                 ("d_info", "info", np.asarray(info, dtype=np.uint32).tobytes()),
                                 ("the fold's d_info", "finfo", np.asarray(finfo, dtype=np.uint32).tobytes())):
            o = offs[name]
            if got[o:o + len(want)].tobytes() != want and outputs == "ok":
                outputs = f"{what} differ from the model's"
            keep[o:o + len(want)] = False
        if outputs == "ok" and not np.array_equal(got[keep], img[keep]):
            outputs = "a byte outside the outputs changed"
        lg = log.cpu().numpy().view(np.uint32)
        entries = []
        for j in range(min(int(lg[34]), 64)):
            e = lg[36 + 6 * j:36 + 6 * j + 6]
            entries.append(dict(index=int(e[0]) | int(e[1]) << 32, site=int(e[3]), block=int(e[4]), thread=int(e[5])))
        reports[case["name"]] = dict(outside=int(lg[32]), desc=int(lg[33]), log=entries, outputs=outputs,
                                     listed=int(info[4]), granules=int(np.unpackbits(bitmap.cpu().numpy().view(np.uint8)).sum()))
    with open(out_path, "w") as f:
        json.dump(dict(reports=reports), f)
    print(f"range_footprint: {len(reports)} cases reported")


if __name__ == "__main__":
    main(sys.argv[1])
