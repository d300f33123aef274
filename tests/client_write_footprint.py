"""The read footprint of hf3fs_crc_client_write_prepare / _complete against the load-checked build.

cases() lays every buffer of a call out in one yard with tests/load_footprint.py's helpers (Yard,
Case, the granule sets); run as a program (by tests/test_gpu_client_write_footprint.py, with
HF3FS_CRC_LIB naming libhf3fs_crc_loadcheck.so) it arms the check around each call and reports the
granules the call's loads touched, in the format load_footprint.compare takes.

The contract (include/hf3fs_crc.h): prepare may read the payload [data, data + length) of an IO
that is valid by itself, and with VERIFY must read it unless the batch is poisoned; nothing else of
any data buffer.  Without VERIFY, and in complete, no data byte is read at all.  No record index
>= n is read.
"""
import json
import os
import sys

import numpy as np

import client_write_cases as wc
import load_footprint as lf

LENGTHS = wc.LENGTHS
KINDS = ("valid", "valid", "range", "valid", "bad", "valid", "empty")


def _case(name, call, verify, ios_spec, ctype=wc.CRC32C, offender=None, counts=None, wave=False, yard=16 << 20):
    """ios_spec: (length, residue, kind) per IO, kind in valid / range (fails its own range) / bad
    (longer than max_len) / empty (length 0).  offender: index of an IO made to end one byte past
    its buffer, which poisons the batch."""
    c = lf.Case(name, yard)
    c.call, c.verify, c.ctype, c.wave = call, verify, ctype, wave
    c.max_len = max([n for n, _r, k in ios_spec if k != "bad"] + [1])
    rows = []
    for i, (n, res, kind) in enumerate(ios_spec):
        if kind == "empty":
            n = 0
        if kind == "bad":
            n = c.max_len + 1 + i % 7
        at = c.yard.place(f"payload{i}", max(n, 1), residue=res)
        data = at + 1 if i == offender else at
        rows.append((data, at, n, 60 if kind == "range" else 0, n, 8192 if kind != "range" else max(n, 1) + 59))
        if call == "prepare" and kind in ("valid", "empty") and i != offender and n:
            c.legal.append((at, n))
            if verify and offender is None:
                c.required.append((at, n))
    c.ios = wc.ios_array(rows)     # addresses = yard offsets; relocated when the call is made
    c.n = c.ios.size
    c.poisoned = offender is not None
    c.hashed = len(c.required)
    c.off = None if counts is None else wc.offsets_of(counts)
    c.n_files = 0 if counts is None else len(counts)
    c.d_ios = c.yard.place("IO records", c.ios.nbytes)
    c.d_upd = c.yard.place("update records", c.n * 56)
    c.d_off = c.yard.place("file offsets", (c.n_files + 1) * 8)
    c.d_exp = c.yard.place("expected values", max(c.n_files, 1) * 4)
    c.d_files = c.yard.place("file records", max(c.n_files, 1) * 24)
    c.d_failed = c.yard.place("failed list", c.n * 4)
    c.d_info = c.yard.place("info", 32)
    c.legal += [(c.d_ios, c.ios.nbytes), (c.d_upd, c.n * 56), (c.d_off, (c.n_files + 1) * 8), (c.d_exp, c.n_files * 4)]
    c.yard.check()
    return c


def _spec(n, seed):
    return [(LENGTHS[(i * 5 + seed) % len(LENGTHS)] if i % 9 == 0 else 1 + (i * 37 + seed) % 97, (i * 3 + seed) % 16,
             KINDS[(i + seed) % len(KINDS)]) for i in range(n)]


def cases():
    grid = [(n, r, "valid") for r in range(16) for n in LENGTHS]
    out = [_case("prepare[grid]", "prepare", True, grid[::2]),
           _case("prepare[grid crc32]", "prepare", True, grid[1::2], ctype=wc.CRC32),
           _case("prepare[65, dropped IOs among the valid]", "prepare", True, _spec(65, 1)),
           _case("prepare[1000]", "prepare", True, _spec(1000, 2)),
           _case("prepare[65, poisoned by IO 7]", "prepare", True, _spec(65, 0), offender=7),
           _case("prepare[1000, poisoned by the last IO]", "prepare", True, _spec(1000, 3) + [(40, 5, "valid")], offender=1000),
           _case("prepare[65, no VERIFY]", "prepare", False, _spec(65, 4)),
           _case("prepare[1000, no VERIFY, poisoned]", "prepare", False, _spec(1000, 5), offender=3),
           _case("complete[65, files of 5, one lane each]", "complete", True, _spec(65, 6), counts=[5] * 13),
           _case("complete[65, files of 5, one wave each]", "complete", True, _spec(65, 6), counts=[5] * 13, wave=True),
           _case("complete[1000, ragged files]", "complete", True, _spec(1000, 7), counts=[0, 1, 300, 0, 699], wave=True),
           _case("complete[1000, no files]", "complete", True, _spec(1000, 8))]
    assert len({c.name for c in out}) == len(out)
    return out


def _run(case, L, orc, base, img, run):
    n = case.n
    sent = case.ios.copy()
    sent["data"] += np.uint64(base)
    sent["buf_base"] += np.uint64(base)
    read = lambda a, k: img[a - base:a - base + k].tobytes()  # noqa: E731
    prep = wc.prepare_model(sent, case.ctype, case.max_len, 16, case.verify, orc, read)
    before = np.frombuffer(bytes(range(0x40, 0x40 + 56)) * n, dtype=wc.UPDATE).copy()
    img[case.d_upd:case.d_upd + n * 56] = before.view(np.uint8)
    if case.call == "prepare":
        img[case.d_ios:case.d_ios + sent.nbytes] = sent.view(np.uint8)

        def call(stream):
            L.client_write_prepare(case.ctype, base + case.d_ios, n, base + case.d_info, case.max_len, max_inline_bytes=16,
                                   verify=case.verify, updates=base + case.d_upd, stream=stream)
        got = run(call)
        outs = ((case.d_ios, prep.apply(sent)), (case.d_upd, prep.updates(sent, before)), (case.d_info, prep.info))
    else:
        ios = prep.apply(sent)                    # what prepare left; the answers come from the update records
        upd = prep.updates(sent, before)
        for i in range(n):                        # the server's outcome: mostly good, some refused, some typed otherwise
            upd["status"][i] = 4080 if i % 23 == 11 else 0
            upd["out_checksum_type"][i] = wc.CRC32 if i % 41 == 7 else case.ctype
            upd["out_checksum"][i] = (i * 2654435761) & wc.M32
        expected = np.arange(case.n_files, dtype=np.uint32)
        img[case.d_ios:case.d_ios + ios.nbytes] = ios.view(np.uint8)
        img[case.d_upd:case.d_upd + n * 56] = upd.view(np.uint8)
        if case.off is not None:
            img[case.d_off:case.d_off + case.off.nbytes] = case.off.view(np.uint8)
            img[case.d_exp:case.d_exp + expected.nbytes] = expected.view(np.uint8)
        want = wc.complete_model(ios, case.off, orc, updates=upd, expected=expected if case.n_files else None)

        def call(stream):
            L.client_write_complete(base + case.d_ios, n, base + case.d_info, file_off=base + case.d_off if case.n_files else None,
                                    n_files=case.n_files, max_ios_per_file=1 << 30 if case.wave else 1,
                                    updates=base + case.d_upd, expected=base + case.d_exp if case.n_files else None,
                                    files=base + case.d_files if case.n_files else None, failed=base + case.d_failed,
                                    failed_cap=n, stream=stream)
        got = run(call)
        outs = ((case.d_ios, want.ios), (case.d_files, want.files), (case.d_failed, want.failed), (case.d_info, want.info))
    keep = np.ones(case.yard.size, dtype=bool)
    for at, recs in outs:
        if got[at:at + recs.nbytes].tobytes() != recs.tobytes():
            return f"the output at yard +{at:#x} differs from the model's"
        keep[at:at + recs.nbytes] = False
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
    assert "client_write_kernels.hip" in b.CHECK_SOURCES
    assert units() == len(b.CHECK_SOURCES) + len(b.CHECK_ONLY), units()   # no unit's copy of the state was lost
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    todo = cases()
    ymax = max(c.yard.size for c in todo)
    yard = torch.zeros(ymax, dtype=torch.uint8, device=dev)
    bitmap = torch.zeros(ymax // lf.G // 32 + 1, dtype=torch.int32, device=dev)
    site_map = torch.zeros(ymax // lf.G, dtype=torch.uint8, device=dev)
    log = torch.zeros(36 + 6 * 64, dtype=torch.int32, device=dev)
    base = yard.data_ptr()
    assert base % lf.PAGE == 0
    reports = {}
    for k, case in enumerate(todo):
        img = np.random.default_rng(0xC117 + k).integers(0, 256, case.yard.size, dtype=np.uint8)

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
    print(f"client_write_footprint: {len(reports)} calls reported")


if __name__ == "__main__":
    main(sys.argv[1])
