"""The read footprint of hf3fs_crc_client_read_batch against the load-checked build.

cases() lays every buffer of a call out in one yard with tests/load_footprint.py's helpers (Yard,
Case, the granule sets); run as a program (by tests/test_gpu_client_read.py::test_read_footprint,
with HF3FS_CRC_LIB naming libhf3fs_crc_loadcheck.so) it arms the check around each call and
reports the granules the call's loads touched, in the format load_footprint.compare takes.

The contract (include/hf3fs_crc.h): with VERIFY the bytes [data, data + read_len) of a child that
is compared and typed must be hashed, and nothing else of any data buffer may be read; without
VERIFY no data byte is read at all.
"""
import json
import os
import sys

import numpy as np

import client_read_cases as cc
import load_footprint as lf

LENGTHS = cc.VERIFY_LENGTHS


def _case(name, verify, kids, counts=None, ctype=cc.CRC32C, switches=None, wrong_every=0, wave=False):
    """kids: (read_len, residue, kind) per child, kind in typed / none / failed / foreign / short
    (read_len bytes of a buffer twice as long)."""
    c = lf.Case(name, 8 << 20)
    c.verify, c.ctype, c.switches, c.wrong_every = verify, ctype, dict(switches or {}), wrong_every
    rows = []
    for i, (n, res, kind) in enumerate(kids):
        room = 2 * n if kind == "short" else n
        at = c.yard.place(f"child{i}", max(room, 1), residue=res)
        t = {"none": cc.NONE, "foreign": cc.CRC32 if ctype == cc.CRC32C else cc.CRC32C}.get(kind, ctype)
        st = cc.CHUNK_NOT_FOUND if kind == "failed" else 0
        rows.append((at, room, n, st, (t, 0)))
        compared = verify and st == 0 and n > 0 and kind != "foreign"
        if compared and t != cc.NONE:
            c.legal.append((at, n))
            c.required.append((at, n))
    c.ios = cc.ios_array(rows)   # data = the yard offset; the checksums are filled in from the image
    c.off = None if counts is None else cc.offsets_of(counts)
    c.n_parents = len(rows) if counts is None else len(counts)
    c.max_children = 1 << 30 if wave else 1 if counts is None else max(counts)  # (the bound only chooses the schedule)
    c.max_len = max([r[2] for r in rows] + [1])
    c.d_ios = c.yard.place("IO records", c.ios.nbytes)
    c.d_off = c.yard.place("parent offsets", (c.n_parents + 1) * 8)
    c.d_par = c.yard.place("parents", c.n_parents * 24)
    c.d_blk = c.yard.place("blocks", c.n_parents * 24)
    c.d_info = c.yard.place("info", 16)
    c.legal += [(c.d_ios, c.ios.nbytes), (c.d_off, (c.n_parents + 1) * 8)]
    c.yard.check()
    return c


def cases():
    grid = [(n, r, "typed") for r in range(16) for n in LENGTHS]
    some = [(n, (3 * i) % 16, "typed") for i, n in enumerate(LENGTHS * 5)][:40]
    mixed = [(n, (5 * i + 1) % 16, ("typed", "none", "failed", "short", "typed", "foreign")[i % 6])
             for i, n in enumerate(LENGTHS * 4)]
    out = [_case("verify[grid residues 0-7]", True, grid[:72]),
           _case("verify[grid residues 8-15]", True, grid[72:]),
           _case("verify[grid crc32]", True, grid[::3], ctype=cc.CRC32),
           _case("verify[one bit wrong in every third]", True, grid[1::2], wrong_every=3),
           _case("verify[none, failed, short and foreign children]", True, mixed),
           _case("verify[static stride]", True, grid[::2], switches={"static": "1"}),
           _case("verify[parents of 3, one lane each]", True, some[:39], counts=[3] * 13),
           _case("verify[parents of 20, one wave each]", True, some, counts=[20, 20], wave=True),
           _case("verify[parents of 3, one wave each]", True, some[:39], counts=[3] * 13, wave=True),
           _case("verify[ragged parents with empty ones]", True, mixed, counts=[0, 1, 17, 0, 18, 0], wrong_every=5),
           _case("plain[grid]", False, grid[::2]),
           _case("plain[mixed children]", False, mixed),
           _case("plain[parents of 20, one wave each]", False, some, counts=[20, 20], wave=True)]
    assert len({c.name for c in out}) == len(out)
    return out


def _run(case, L, orc, base, img, run):
    ios = case.ios.copy()
    for i in range(ios.size):
        at, n, t = int(ios["data"][i]), int(ios["read_len"][i]), int(ios["checksum_type"][i])
        v = 0 if t == cc.NONE else orc.create(t, img[at:at + n].tobytes())[1]
        if case.wrong_every and i % case.wrong_every == 1:
            v ^= 1 << (i % 32)
        ios["checksum"][i] = v
    want = cc.model(ios, case.off, case.ctype, case.max_len, case.verify, orc, lambda a, n: img[a:a + n].tobytes())
    sent = ios.copy()
    sent["data"] += np.uint64(base)
    img[case.d_ios:case.d_ios + sent.nbytes] = sent.view(np.uint8)
    if case.off is not None:
        img[case.d_off:case.d_off + case.off.nbytes] = case.off.view(np.uint8)

    def call(stream):
        L.client_read_batch(case.ctype, base + case.d_ios, ios.size, base + case.d_info,
                            parent_off=None if case.off is None else base + case.d_off, n_parents=case.n_parents,
                            max_children=case.max_children, max_len=case.max_len, verify=case.verify,
                            parents=base + case.d_par, blocks=base + case.d_blk, stream=stream)
    got = run(call)
    g = got[case.d_ios:case.d_ios + sent.nbytes].view(cc.IO)
    exp = sent.copy()
    exp["computed"], exp["status"] = want.computed, want.status
    if g.tobytes() != exp.tobytes():
        return "the IO records differ from the model's"
    for at, recs in ((case.d_par, want.parents), (case.d_blk, want.blocks), (case.d_info, want.info)):
        if got[at:at + recs.nbytes].tobytes() != recs.tobytes():
            return f"the output at yard +{at:#x} differs from the model's"
    keep = np.ones(case.yard.size, dtype=bool)
    for at, n in ((case.d_ios, sent.nbytes), (case.d_par, want.parents.nbytes), (case.d_blk, want.blocks.nbytes),
                  (case.d_info, 16)):
        keep[at:at + n] = False
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
    assert "client_read_kernels.hip" in b.CHECK_SOURCES
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
        img = np.random.default_rng(0xF007 + k).integers(0, 256, case.yard.size, dtype=np.uint8)
        defaults = {name: L.get_option(name) for name in case.switches}
        for name, value in case.switches.items():
            L.set_option(name, value)

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
        for name, value in defaults.items():
            L.set_option(name, value)
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
    print(f"client_read_footprint: {len(reports)} calls reported")


if __name__ == "__main__":
    main(sys.argv[1])
