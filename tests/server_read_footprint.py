"""The read footprint of hf3fs_crc_server_read_prepare / _complete against the load-checked build.

cases(orc) lays every buffer of a call out in one yard with tests/load_footprint.py's helpers (Yard,
Case, the granule sets); run as a program (by tests/test_gpu_server_read_footprint.py, with
HF3FS_CRC_LIB naming libhf3fs_crc_loadcheck.so) it arms the check around each call and reports the
granules the call's loads touched, in the format load_footprint.compare takes.

The contract (include/hf3fs_crc.h): complete loads the bytes [localbuf + head_len, +L) of a job that
hashes (the range kernels) or packs into the inline arena (the copy body), L the clipped length;
nothing else of any read buffer -- not its head, not its tail, not the bytes past L -- and no
record index at or past n.  Prepare loads no byte of any buffer.
"""
import json
import os
import sys

import numpy as np

import load_footprint as lf
import server_read_cases as sc

LENGTHS = (0, 1, 15, 16, 17, 100, 1000, 4095, 4096, 4097)
MAX_LEN, SMALL, BIG = 8192, 4096, 12288
BUFFERS = 24


def _case(k, name, call, n, ctype, orc, loading=True):
    c = lf.Case(name, 8 << 20)
    c.call, c.n, c.ctype = call, n, ctype
    c.img = np.random.default_rng(0x5EAD + k).integers(0, 256, c.yard.size, dtype=np.uint8)
    rng = np.random.default_rng(0xF00D + k)
    bufs = [c.yard.place(f"read buffer {b}", 3 * 4096, residue=b % 16) for b in range(BUFFERS)]
    counts = []
    while sum(counts) < n:
        counts.append(min(int(rng.choice([0, 1, 3, 20])), n - sum(counts)))
    jobs, reqs, ro = sc.new_jobs(n), sc.new_reqs(len(counts)), sc.offsets(counts)
    jobs["offset"] = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 8192, n))
    jobs["length"] = rng.choice(LENGTHS, n)
    head = jobs["offset"] % 4096
    end = jobs["offset"].astype(np.int64) + jobs["length"]
    jobs["chunk_len"] = np.where(rng.random(n) < 0.3, np.maximum(0, end - rng.integers(0, 300, n)), end)
    jobs["res"] = np.select([rng.random(n) < 0.1, rng.random(n) < 0.2], [np.full(n, -1, dtype=np.int64), (head + jobs["length"] // 2).astype(np.int64)], 12288)
    jobs["localbuf"] = np.asarray(bufs, dtype=np.uint64)[rng.integers(0, BUFFERS, n)]
    jobs["chunk_checksum_type"] = ctype
    jobs["engine"] = (rng.random(n) < 0.3) & (ctype == sc.CRC32C)
    jobs["update_ver_now"] = np.where(rng.random(n) < 0.05, 4, 1)
    jobs["meta_status"][rng.random(n) < 0.03] = sc.CHUNK_METADATA_NOT_FOUND
    if loading:
        reqs["checksum_type"] = np.where(rng.random(reqs.size) < 0.3, sc.NONE, ctype)
        reqs["xmit"] = rng.integers(0, 3, reqs.size)
        reqs["recalculate"] = rng.random(reqs.size) < 0.5
    else:   # no checksum asked for, nothing recalculated, nothing packed
        reqs["checksum_type"], reqs["xmit"] = sc.NONE, np.where(rng.random(reqs.size) < 0.5, sc.XMIT_RDMA, sc.XMIT_NONE)
    c.jobs, c.reqs, c.ro = jobs, reqs, ro
    read = lambda a, ln: c.img[a:a + ln].tobytes()  # noqa: E731
    pj, pr = jobs.copy(), reqs.copy()
    sc.prepare(pj, pr, ro, SMALL, BIG)
    loads = []
    c.inline_cap = int(jobs["length"].sum())
    info, _, _ = sc.complete(pj, pr, ro, ctype, MAX_LEN, read, orc, c.inline_cap, loads=loads)
    if call == "complete":
        c.jobs, c.reqs = jobs.copy(), reqs.copy()   # complete starts from prepared records
        sc.prepare(c.jobs, c.reqs, ro, SMALL, BIG)
        c.legal = sorted({(a, ln) for _, _, a, ln in loads})
        c.hashed = len({i for i, _, _, _ in loads})
    else:
        c.hashed = 0
    c.required = list(c.legal)
    assert (c.hashed > 0) == (loading and call == "complete")
    c.d_jobs = c.yard.place("job records", jobs.nbytes)
    c.d_reqs = c.yard.place("request records", reqs.nbytes)
    c.d_ro = c.yard.place("request offsets", ro.nbytes)
    c.d_info = c.yard.place("info", 4 * sc.INFO_WORDS)
    c.d_inline = c.yard.place("inline arena", max(c.inline_cap, 16))
    c.d_wr = c.yard.place("RDMA list", n * sc.WR.itemsize)
    c.yard.check()
    return c


def cases(orc):
    out = []
    for k, (call, n, ctype, loading) in enumerate((("complete", 65, sc.CRC32C, True), ("complete", 1000, sc.CRC32C, True),
                                                   ("complete", 65, sc.CRC32, True), ("complete", 65, sc.CRC32C, False),
                                                   ("complete", 1000, sc.CRC32C, False), ("prepare", 65, sc.CRC32C, True),
                                                   ("prepare", 1000, sc.CRC32C, True))):
        name = f"{call}[{n} jobs, {'crc32c' if ctype == sc.CRC32C else 'crc32'}{'' if loading else ', nothing loads'}]"
        out.append(_case(k, name, call, n, ctype, orc, loading))
    return out


def _run(case, L, orc, base, img, run):
    sent = case.jobs.copy()
    sent["localbuf"] = np.where(sent["localbuf"] != 0, sent["localbuf"] + np.uint64(base), 0)
    want_j, want_r = sent.copy(), case.reqs.copy()
    read = lambda a, ln: img[a - base:a - base + ln].tobytes()  # noqa: E731
    inline, wr = b"", np.zeros(0, dtype=sc.WR)
    if case.call == "prepare":
        info = sc.prepare(want_j, want_r, case.ro, SMALL, BIG)
    else:
        info, inline, wr = sc.complete(want_j, want_r, case.ro, case.ctype, MAX_LEN, read, orc, case.inline_cap)
    info = np.asarray(info, dtype=np.uint32)
    for at, arr in ((case.d_jobs, sent), (case.d_reqs, case.reqs), (case.d_ro, case.ro)):
        img[at:at + arr.nbytes] = arr.view(np.uint8)

    def call(stream):
        if case.call == "prepare":
            L.server_read_prepare(base + case.d_jobs, case.n, base + case.d_reqs, base + case.d_ro, case.reqs.size,
                                  base + case.d_info, SMALL, BIG, stream=stream)
        else:
            L.server_read_complete(case.ctype, base + case.d_jobs, case.n, base + case.d_reqs, base + case.d_ro,
                                   case.reqs.size, base + case.d_info, MAX_LEN, inline=base + case.d_inline,
                                   inline_cap=case.inline_cap, wr=base + case.d_wr, wr_cap=case.n, stream=stream)
    got = run(call)
    keep = np.ones(case.yard.size, dtype=bool)
    for what, at, want in (("the job records", case.d_jobs, want_j.tobytes()), ("the request records", case.d_reqs, want_r.tobytes()),
                           ("d_info", case.d_info, info.tobytes()), ("the inline arena", case.d_inline, inline),
                           ("the RDMA list", case.d_wr, wr.tobytes())):
        if got[at:at + len(want)].tobytes() != want:
            return f"{what} differ from the model's"
        keep[at:at + len(want)] = False
    return "ok" if np.array_equal(got[keep], img[keep]) else "a byte outside the outputs changed"


def main(out_path):
    import ctypes
    import importlib
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    for p in (repo, os.path.join(repo, "oracle"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import oracle
    oracle.lib()
    hf = importlib.import_module("3fs_amd")
    L = hf._lib
    lib = L.load()
    arm, disarm, units = lib.hf3fs_crc_loadcheck_arm, lib.hf3fs_crc_loadcheck_disarm, lib.hf3fs_crc_loadcheck_units
    arm.restype = disarm.restype = units.restype = ctypes.c_int
    arm.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    b = importlib.import_module("3fs_amd.build")
    assert "server_read_kernels.hip" in b.CHECK_SOURCES
    assert units() == len(b.CHECK_SOURCES) + len(b.CHECK_ONLY), units()   # no unit's copy of the state was lost
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    todo = cases(oracle)
    ymax = max(c.yard.size for c in todo)
    yard = torch.zeros(ymax, dtype=torch.uint8, device=dev)
    bitmap = torch.zeros(ymax // lf.G // 32 + 1, dtype=torch.int32, device=dev)
    site_map = torch.zeros(ymax // lf.G, dtype=torch.uint8, device=dev)
    log = torch.zeros(36 + 6 * 64, dtype=torch.int32, device=dev)
    base = yard.data_ptr()
    assert base % lf.PAGE == 0
    reports = {}
    for case in todo:
        img = case.img[:case.yard.size].copy()

        def run(call, case=case, img=img):
            yard[:case.yard.size].copy_(torch.from_numpy(img))
            bitmap.zero_(), site_map.zero_(), log.zero_()
            torch.cuda.synchronize()
            rc = arm(base, case.yard.size, bitmap.data_ptr(), site_map.data_ptr(), log.data_ptr())
            assert rc == 0, rc
            try:
                call(stream)
                torch.cuda.synchronize()
            finally:
                assert disarm() == 0
            return yard[:case.yard.size].cpu().numpy()

        outputs = _run(case, L, oracle, base, img, run)
        bits = np.unpackbits(bitmap.cpu().numpy().view(np.uint8), bitorder="little")[:case.n_granules].astype(bool)
        sm = site_map.cpu().numpy()[:case.n_granules]
        lg = log.cpu().numpy().view(np.uint32)
        entries = []
        for j in range(min(int(lg[34]), 64)):
            e = lg[36 + 6 * j:36 + 6 * j + 6]
            addr = int(e[0]) | int(e[1]) << 32
            entries.append(dict(address=addr, bytes=int(e[2]), site=int(e[3]), block=int(e[4]), thread=int(e[5]),
                                yard_offset=addr - base))
        reports[case.name] = dict(read=lf.runs_of(bits, sm), counters={str(j): int(lg[j]) for j in range(1, 18) if lg[j]},
                                  outside=int(lg[32]), desc=int(lg[33]), log=entries, outputs=outputs)
    with open(out_path, "w") as f:
        json.dump(dict(reports=reports), f)
    print(f"server_read_footprint: {len(reports)} calls reported")


if __name__ == "__main__":
    main(sys.argv[1])
