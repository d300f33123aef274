"""The read footprint of hf3fs_crc_forward_prepare / _complete against the load-checked build.

cases(orc) lays every buffer of a call out in one yard with tests/load_footprint.py's helpers (Yard,
Case, the granule sets); run as a program (by tests/test_gpu_forward_footprint.py, with
HF3FS_CRC_LIB naming libhf3fs_crc_loadcheck.so) it arms the check around each call and reports the
granules the call's loads touched, in the format load_footprint.compare takes.

The contract (include/hf3fs_crc.h): prepare hashes the bytes [chunk, chunk + chunk_len) of a job
that takes the syncing read with a typed, non-empty chunk, complete the bytes [out_data, out_data +
out_length) of a sent job answered 4080 with a typed, non-empty buffer; nothing else of any data
buffer may be read, and no record index at or past n.
"""
import json
import os
import sys

import numpy as np

import forward_cases as fc
import load_footprint as lf

LENGTHS = (0, 1, 15, 16, 17, 4095, 4096)
RESIDUES = (0, 1, 15)
MAX_LEN, MAX_INLINE = 4096, 64
ADDRESSES = ("payload", "chunk", "out_data")


def _pool(c, kind, img, ctype, orc):
    addrs, lens, cks = [], [], []
    for res in RESIDUES:
        for n in LENGTHS:
            at = c.yard.place(f"{kind} of {n} at residue {res}", max(n, 1), residue=res)
            addrs.append(at)
            lens.append(n)
            cks.append(tuple(orc.create(ctype, img[at:at + n].tobytes())))
    return addrs, lens, cks


def _case(k, name, call, n, ctype, orc, hashing=True):
    c = lf.Case(name, 8 << 20)
    c.call, c.n, c.ctype = call, n, ctype
    c.img = np.random.default_rng(0xF0F0 + k).integers(0, 256, c.yard.size, dtype=np.uint8)
    chunks, payloads = _pool(c, "chunk", c.img, ctype, orc), _pool(c, "payload", c.img, ctype, orc)
    rng = np.random.default_rng(0x5EED + k)
    if hashing:
        jobs = fc.random_jobs(rng, n, ctype, *chunks, *payloads, max_len=MAX_LEN)
    else:   # plain writes to serving successors, answered without a 4080: no rung hashes
        jobs = np.concatenate([fc.plain_job(payload=payloads[0][i % 21], length=payloads[1][i % 21],
                                            req_checksum=payloads[2][i % 21][1], req_checksum_type=ctype)
                               for i in range(n)])
    read = lambda a, ln: c.img[a:a + ln].tobytes()  # noqa: E731
    prepared, pinfo = fc.model_prepare(jobs, ctype, MAX_LEN, MAX_INLINE, orc, read)
    if call == "prepare":
        c.jobs = jobs
        for i in range(n):
            _, bits = fc.prepare_one(jobs[i], ctype, MAX_LEN, MAX_INLINE, read, orc)
            if bits["sync_hashed"]:
                c.legal.append((int(jobs["chunk"][i]), int(jobs["chunk_len"][i])))
        c.hashed = int(pinfo[3])
    else:
        c.jobs = fc.random_answers(rng, prepared, ctype)
        if not hashing:
            c.jobs["fwd_status"] = np.where(c.jobs["fwd_status"] == fc.CHECKSUM_MISMATCH, 4010, c.jobs["fwd_status"])
        else:   # every third sent job is answered 4080
            again = (c.jobs["action"] == fc.SEND) & (np.arange(n) % 3 == 0)
            c.jobs["fwd_status"] = np.where(again, fc.CHECKSUM_MISMATCH, c.jobs["fwd_status"])
        c.hashed = 0
        for i in range(n):
            _, bits = fc.complete_one(c.jobs[i], ctype, MAX_LEN, read, orc)
            if bits["rehashed"]:
                c.legal.append((int(c.jobs["out_data"][i]), int(c.jobs["out_length"][i])))
                c.hashed += 1
    c.required = list(c.legal)
    assert (c.hashed > 0) == hashing and len(c.legal) == c.hashed
    c.d_jobs = c.yard.place("job records", c.jobs.nbytes)
    c.d_info = c.yard.place("info", 4 * fc.INFO_WORDS)
    c.d_idx = c.yard.place("commit list", 4 * n)
    c.yard.check()
    return c


def cases(orc):
    out, k = [], 0
    for call in ("prepare", "complete"):
        for n, ctype, hashing in ((65, fc.CRC32C, True), (1000, fc.CRC32C, True), (65, fc.CRC32, True),
                                  (65, fc.CRC32C, False), (1000, fc.CRC32C, False)):
            name = f"{call}[{n} jobs, {'crc32c' if ctype == fc.CRC32C else 'crc32'}{'' if hashing else ', nothing hashes'}]"
            out.append(_case(k, name, call, n, ctype, orc, hashing))
            k += 1
    return out


def _moved(jobs, base):
    a = jobs.copy()
    for f in ADDRESSES:
        a[f] = np.where(jobs[f] != 0, jobs[f] + np.uint64(base), 0)
    return a


def _run(case, L, orc, base, img, run):
    sent = _moved(case.jobs, base)
    read = lambda a, ln: img[a - base:a - base + ln].tobytes()  # noqa: E731
    if case.call == "prepare":
        want, info = fc.model_prepare(sent, case.ctype, MAX_LEN, MAX_INLINE, orc, read)
        idx = None
    else:
        want, idx, info = fc.model_complete(sent, case.ctype, MAX_LEN, orc, read)
    img[case.d_jobs:case.d_jobs + sent.nbytes] = sent.view(np.uint8)

    def call(stream):
        if case.call == "prepare":
            L.forward_prepare(case.ctype, base + case.d_jobs, case.n, base + case.d_info, MAX_LEN, MAX_INLINE,
                              stream=stream)
        else:
            L.forward_complete(case.ctype, base + case.d_jobs, case.n, base + case.d_info, MAX_LEN,
                               commit_idx=base + case.d_idx, stream=stream)
    got = run(call)
    if got[case.d_jobs:case.d_jobs + sent.nbytes].tobytes() != want.tobytes():
        return "the job records differ from the model's"
    if got[case.d_info:case.d_info + info.nbytes].tobytes() != info.tobytes():
        return "d_info differs from the model's"
    keep = np.ones(case.yard.size, dtype=bool)
    keep[case.d_jobs:case.d_jobs + sent.nbytes] = False
    keep[case.d_info:case.d_info + info.nbytes] = False
    if idx is not None:
        if got[case.d_idx:case.d_idx + idx.nbytes].tobytes() != idx.tobytes():
            return "the commit list differs from the model's"
        keep[case.d_idx:case.d_idx + idx.nbytes] = False
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
    assert "forward_kernels.hip" in b.CHECK_SOURCES
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
    print(f"forward_footprint: {len(reports)} calls reported")


if __name__ == "__main__":
    main(sys.argv[1])
