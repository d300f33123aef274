"""hf3fs_crc_client_read_batch on the GPU.

Every expectation comes from tests/client_read_cases.py: the reference's verify ladder and merge
loop restated in Python over the CPU oracle's CRC.  After every call the whole IO array (inputs
unchanged, `computed` and `status` the model's), every byte of the parent and block records, the
four info words, the guard bytes around every output array and the data arena (unchanged) are
compared.
"""
import functools
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import client_read_cases as cc
import host_memory as hm

torch = pytest.importorskip("torch")

import test_gpu_stream_queue as stream_queue  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64          # bytes in front of and behind every output array that no call may write
CANARY = 0x5A
REL = 1 << 16       # a case's data addresses are REL + the offset in its arena (0 stays 0: no buffer)
SWITCH = 128        # kClientLaneMaxChildren: parents of more children take one wave each
LANE, WAVE = 1, 1 << 30  # max_children that make any call take one lane / one wave per parent


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Case:
    """ios with arena-relative addresses, parent offsets (None: every IO its own parent), the
    arena's bytes (None: a case for calls without VERIFY only).  Never modified once built."""

    def __init__(self, ios, off, arena, ctype=cc.CRC32C, max_len=None, injected=None):
        self.ios, self.off, self.arena, self.ctype, self.injected = ios, off, arena, ctype, injected
        self.max_len = int(ios["read_len"].max()) if max_len is None and ios.size else (max_len or 0)
        self.n_parents = ios.size if off is None else off.size - 1
        self.max_children = 1 if off is None else int(np.diff(off.astype(np.int64)).max(initial=0))
        for a in (ios, off, arena):
            if a is not None:
                a.setflags(write=False)
        self._want = {}

    def want(self, verify, orc):
        if verify not in self._want:
            read = None if self.arena is None else lambda addr, n: self.arena[addr - REL:addr - REL + n].tobytes()
            self._want[verify] = cc.model(self.ios, self.off, self.ctype, self.max_len, verify, orc, read)
        return self._want[verify]


def _guarded(dev, nbytes):
    t = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
    return t, t[GUARD:GUARD + nbytes]


class Box:
    """Device images of one case: the arena, the records, the offsets and guarded outputs."""

    def __init__(self, dev, case, parents=True, blocks=True):
        self.case = case
        self.arena = None
        base = REL
        if case.arena is not None:
            self.arena = torch.from_numpy(case.arena.copy()).to(dev)
            base = self.arena.data_ptr()
            assert base % 16 == 0
        self.sent = case.ios.copy()
        self.sent["data"] = np.where(case.ios["data"] != 0, case.ios["data"] - np.uint64(REL) + np.uint64(base), 0)
        self.ios_raw, self.ios = _guarded(dev, max(self.sent.nbytes, 8))
        if self.sent.size:
            self.ios[:self.sent.nbytes].copy_(torch.from_numpy(self.sent.view(np.uint8).copy()))
        self.off = None if case.off is None else torch.from_numpy(case.off.view(np.int64).copy()).to(dev)
        self.par_raw, self.par = _guarded(dev, max(case.n_parents, 1) * 24)
        self.blk_raw, self.blk = _guarded(dev, max(case.n_parents, 1) * 24)
        self.info_raw, self.info = _guarded(dev, 16)
        self.use_parents, self.use_blocks = parents, blocks
        torch.cuda.synchronize()

    def call(self, hf, verify, stream=None, max_children=None):
        """max_children: LANE or WAVE force a schedule (the bound only chooses it, include/hf3fs_crc.h)."""
        c = self.case
        hf.client_read_batch(c.ctype, self.ios if c.ios.size else None, c.ios.size, self.info, parent_off=self.off,
                             n_parents=c.n_parents, max_children=c.max_children if max_children is None else max_children,
                             max_len=c.max_len, verify=verify,
                             parents=self.par if self.use_parents else None,
                             blocks=self.blk if self.use_blocks else None,
                             stream=stream or torch.cuda.current_stream())

    def check(self, want, what, sent=None, arena=None):
        torch.cuda.synchronize()
        c = self.case
        sent = self.sent if sent is None else sent
        for name, raw in (("d_ios", self.ios_raw), ("d_parents", self.par_raw), ("d_blocks", self.blk_raw),
                          ("d_info", self.info_raw)):
            g = raw.cpu().numpy()
            assert (g[:GUARD] == CANARY).all() and (g[-GUARD:] == CANARY).all(), f"{what}: bytes around {name} written"
        got = self.ios.cpu().numpy()[:sent.nbytes].view(cc.IO)
        exp = sent.copy()
        exp["computed"], exp["status"] = want.computed, want.status
        if got.tobytes() != exp.tobytes():
            for f in cc.IO.names:
                bad = np.flatnonzero((got[f] != exp[f]).reshape(got.size, -1).any(axis=1))
                if bad.size:
                    i = int(bad[0])
                    pytest.fail(f"{what}: {bad.size} IOs differ in {f}, first {i}: got {got[f][i]}, want {exp[f][i]} "
                                f"({sent[i]})")
        for name, on, t, exp_recs in (("parents", self.use_parents, self.par, want.parents),
                                      ("blocks", self.use_blocks, self.blk, want.blocks)):
            g = t.cpu().numpy()
            if not on:
                assert (g == CANARY).all(), f"{what}: a NULL {name} array was written"
                continue
            recs = g[:exp_recs.nbytes].view(exp_recs.dtype)
            if recs.tobytes() != exp_recs.tobytes():
                for f in exp_recs.dtype.names:
                    bad = np.flatnonzero((recs[f] != exp_recs[f]).reshape(recs.size, -1).any(axis=1))
                    if bad.size:
                        p = int(bad[0])
                        pytest.fail(f"{what}: {bad.size} {name} differ in {f}, first {p}: got {recs[p]}, want {exp_recs[p]}")
            assert (g[exp_recs.nbytes:] == CANARY).all(), f"{what}: {name} written past n_parents"
        info = self.info.cpu().numpy().view(np.uint32)
        assert info.tolist() == want.info.tolist(), f"{what}: info {dict(zip(cc.INFO, info.tolist()))}"
        if self.arena is not None:
            assert np.array_equal(self.arena.cpu().numpy(), c.arena if arena is None else arena), \
                f"{what}: the data arena changed"


def _run(hf, orc, dev, case, verify, what, parents=True, blocks=True, stream=None, max_children=None):
    box = Box(dev, case, parents, blocks)
    box.call(hf, verify, stream, max_children)
    want = case.want(verify, orc)
    box.check(want, what)
    return want


# ---- verify -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid(orc, ctype, kind):
    arena = cc.arena_bytes(cc.verify_grid_bytes(), 0xC11E + ctype)
    ios, injected = cc.verify_grid(REL, arena, ctype, kind, orc)
    return Case(ios, None, arena, ctype, max_len=4099, injected=injected)


@pytest.mark.parametrize("kind", ["typed", "none", "failed", "foreign"])
@pytest.mark.parametrize("ctype", [cc.CRC32C, cc.CRC32], ids=["crc32c", "crc32"])
def test_verify_grid(hf, orc, dev, ctype, kind):
    """Every address residue x nine lengths, right and with one bit wrong: the 7015 set is the
    injected set exactly, every `computed` is the oracle's."""
    case = _grid(orc, ctype, kind)
    want = _run(hf, orc, dev, case, True, f"verify grid {kind}")
    assert set(np.flatnonzero(want.status == cc.MISMATCH).tolist()) == case.injected
    assert bool(case.injected) == (kind in ("typed", "none"))
    if kind == "typed":
        assert len(case.injected) == 16 * 8 and np.count_nonzero(want.computed) >= 16 * 16 - 2
    if kind == "foreign":
        assert (want.status == cc.INVALID_ARG).all() and (want.computed == 0).all()
    if kind == "failed":
        assert set(want.status.tolist()) == {cc.CHUNK_NOT_FOUND, 4010}
    # the same records without VERIFY: nothing compared, nothing read, both CRC types pass
    want = _run(hf, orc, dev, case, False, f"verify grid {kind}, no VERIFY")
    assert not (want.status == cc.MISMATCH).any() and not (want.status == cc.INVALID_ARG).any()


def test_verify_only_and_bad_records(hf, orc, dev):
    """VERIFY with neither parents nor blocks; and the records the call refuses."""
    case = _grid(orc, cc.CRC32C, "typed")
    _run(hf, orc, dev, case, True, "verify only", parents=False, blocks=False)
    arena = cc.arena_bytes(4096, 5)
    rows = [(REL, 8, 8, 0, (7, 1)), (REL, 8, 8, 0, (cc.CRC32, 1)), (REL, 8, 9, 0, (cc.NONE, 0)), (0, 8, 8, 0, (cc.NONE, 0)),
            (REL, 99, 65, 0, (cc.NONE, 0)), (0, 8, 9, 4010, (7, 1)), (REL + 1, 64, 64, 0, (cc.CRC32C, 0))]
    bad = Case(cc.ios_array(rows), cc.offsets_of([3, 4]), arena, max_len=64)
    assert _run(hf, orc, dev, bad, True, "bad records").status.tolist() == [3, 3, 3, 3, 3, 4010, cc.MISMATCH]
    assert _run(hf, orc, dev, bad, False, "bad records, no VERIFY").status.tolist() == [3, 0, 0, 0, 0, 4010, 0]


@pytest.mark.parametrize("bound", [None, LANE, WAVE], ids=["chosen", "lane", "wave"])
@pytest.mark.parametrize("k", [3, SWITCH + 1])
def test_verify_only_with_offsets(hf, orc, dev, k, bound):
    """VERIFY of a split batch with neither d_parents nor d_blocks: the verdicts are written and
    d_info still counts the failing and the hard parents, under either schedule."""
    case = _shape(orc, k)
    want = _run(hf, orc, dev, case, True, f"verify only, {k} children", parents=False, blocks=False, max_children=bound)
    assert want.info[1] >= 6 and want.info[2] >= 4


# ---- merge shapes ---------------------------------------------------------------------------------
CHILDREN = (0, 1, 2, 3, 63, 64, 65, SWITCH - 1, SWITCH, SWITCH + 1, 1024, 1025)


@functools.lru_cache(maxsize=None)
def _shape(orc, k, ctype=cc.CRC32C):
    """Parents of k children with real bytes behind them (read_len 0..96 at any residue): a clean
    one, one with NONE-typed children mixed in, and for the first, a middle and the last position
    one parent whose child there carries a server error (it fails with and without VERIFY) and one
    whose child there has a wrong checksum (it fails with VERIFY only); between them parents of 0
    and 1 children so that the offsets are not a multiple of k."""
    rng = np.random.default_rng(1000 + k)
    arena = cc.arena_bytes(1 << 16, 77 + k)
    rows, counts = [], []

    def parent(n, fail=None, wrong=None, nones=False):
        for j in range(n):
            ln = 0 if j % 11 == 5 else int(rng.integers(1, 97))
            at = int(rng.integers(0, arena.size - 96))
            t = cc.NONE if nones and j % 3 == 1 else ctype
            v = 0 if t == cc.NONE else orc.create(t, arena[at:at + ln].tobytes())[1]
            st = 0
            if j == fail:
                st = cc.CHUNK_NOT_FOUND if n % 2 else 4010
            if j == wrong:
                ln, v = max(ln, 1), v ^ 0x10
            rows.append((REL + at, ln + j % 2, ln, st, (t, v)))
        counts.append(n)

    parent(k)
    parent(0)
    parent(k, nones=True)
    for pos in sorted({0, k // 2, k - 1}) if k else []:
        parent(k, fail=pos)
        parent(1)
        parent(k, wrong=pos)
    return Case(cc.ios_array(rows), cc.offsets_of(counts), arena, ctype, max_len=97)


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "plain"])
@pytest.mark.parametrize("k", CHILDREN)
def test_merge_shapes(hf, orc, dev, k, verify):
    """0 to 1,025 children per parent around the schedule switch-over, the failing child first, in
    the middle and last; under the schedule the call chooses and under the other one; with
    d_parents or d_blocks NULL in turn."""
    case = _shape(orc, k)
    want = _run(hf, orc, dev, case, verify, f"{k} children")
    if k >= 2:
        assert {0, cc.MISMATCH if verify else 0, cc.CHUNK_NOT_FOUND if k % 2 else 4010} <= set(want.parents["status"].tolist())
        assert cc.NOT_INITIALIZED in want.parents["status"]
    _run(hf, orc, dev, case, verify, f"{k} children, parents only", blocks=False)
    _run(hf, orc, dev, case, verify, f"{k} children, blocks only", parents=False)
    _run(hf, orc, dev, case, verify, f"{k} children, the other schedule",
         max_children=WAVE if case.max_children <= SWITCH else LANE)


@functools.lru_cache(maxsize=None)
def _singles(orc, n):
    rng = np.random.default_rng(n)
    arena = cc.arena_bytes(1 << 16, n)
    at = rng.integers(0, arena.size - 40, n)
    ln = rng.integers(0, 41, n)
    rows = []
    for i in range(n):
        v = orc.create(cc.CRC32C, arena[at[i]:at[i] + ln[i]].tobytes())[1]
        st = cc.CHUNK_NOT_FOUND if i % 97 == 13 else 4010 if i % 1009 == 500 else 0
        rows.append((REL + int(at[i]), 40, int(ln[i]), st, (cc.CRC32C, v ^ (1 if i % 61 == 7 else 0))))
    ios = cc.ios_array(rows)
    return Case(ios, None, arena, max_len=40), Case(ios.copy(), cc.offsets_of([1] * n), arena.copy(), max_len=40)


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "plain"])
@pytest.mark.parametrize("n", [1, 2, 257, 70001])
def test_one_child_per_parent(hf, orc, dev, n, verify):
    """The d5 shape: without offsets, with offsets under the lane schedule, and (a wave per block)
    under the wave schedule.  70,001 parents stride the grid and end in a partial workgroup."""
    null_off, with_off = _singles(orc, n)
    want = _run(hf, orc, dev, null_off, verify, f"{n} IOs, NULL offsets")
    if n == 70001:
        assert want.info[2] >= 60 and (np.count_nonzero(want.status == cc.MISMATCH) > 1000) == verify
    _run(hf, orc, dev, with_off, verify, f"{n} parents of one child")
    _run(hf, orc, dev, with_off, verify, f"{n} parents of one child, one wave each", max_children=WAVE)


# ---- arithmetic without data ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data_free():
    rng = np.random.default_rng(0xF4EE)
    rows, counts = [], []
    for n, kw in ((5, dict(big=True)), (40, dict(big=True, types=(cc.NONE, cc.CRC32C, cc.CRC32))),
                  (700, dict(big=True, types=(cc.CRC32C, cc.CRC32), zero_every=7)),
                  (64, dict(big=True, types=(cc.NONE, cc.NONE, cc.NONE, cc.CRC32))),
                  (17, dict(big=True, fail_at=(16,))), (300, dict(big=True, fail_at=(150, 151, 299))),
                  (3, dict(types=(cc.NONE,)))):
        rows += cc.random_children(rng, n, **kw)
        counts.append(n)
    rows += [(0, 0, 0xFFFFFFFF, 0, (cc.CRC32, 5)), (0, 0, 0xFFFFFFFF, 0, (cc.CRC32, 6)), (0, 0, 2, 0, (cc.CRC32, 7))]
    counts.append(3)                                   # 2^32 - 1 twice and 2: the sum wraps to 0
    rows += [(0, 1 << 31, 1 << 31, 0, (cc.CRC32C, int(rng.integers(0, 1 << 32)))) for _ in range(1025)]
    counts.append(1025)                                # 2^41 bytes behind child 0
    return Case(cc.ios_array(rows), cc.offsets_of(counts), None, max_len=0)


@pytest.mark.parametrize("lane_max", [None, LANE, WAVE], ids=["chosen", "lane", "wave"])
def test_arithmetic_without_data(hf, orc, dev, lane_max):
    """Without VERIFY no byte is read, so the children claim any read_len: up to 2^32 - 1, sums that
    wrap, 1,025 typed children of 2^31 bytes, every mix of types."""
    case = _data_free()
    want = _run(hf, orc, dev, case, False, "data-free", max_children=lane_max)
    p = want.parents
    assert p["length"][-2] == 0 and p["status"][-2] == 0 and p["length"][-1] == (1025 << 31) & cc.M32
    assert (want.computed == 0).all() and {cc.NONE, cc.CRC32C, cc.CRC32} == set(p["checksum_type"].tolist())


# ---- hand-over to the file digest ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _files(orc):
    """40 files of 1..9 blocks of 64 bytes asked for, each block a parent of 1..4 children; some
    blocks are holes (7007), some short, one fails hard (4010), one child's bytes are wrong."""
    rng = np.random.default_rng(0xF11E)
    arena = cc.arena_bytes(1 << 16, 0xF11E)
    rows, counts, file_counts = [], [], []
    for f in range(40):
        nb = 1 + f % 9
        file_counts.append(nb)
        for b in range(nb):
            kids = 1 + (f + b) % 4
            hole = (f * 7 + b) % 10 == 3
            short = (f * 7 + b) % 10 == 6
            for j in range(kids):
                ln = 64 // kids if j + 1 < kids else 64 - (kids - 1) * (64 // kids)
                got = ln // 2 if short and j + 1 == kids else ln
                at = int(rng.integers(0, arena.size - 64))
                v = orc.create(cc.CRC32C, arena[at:at + got].tobytes())[1]
                st = cc.CHUNK_NOT_FOUND if hole and j == 0 else 4010 if (f, b, j) == (17, 2, 0) else 0
                if (f, b, j) == (30, 1, 0):
                    v ^= 0x8000
                rows.append((REL + at, ln, got, st, (cc.CRC32C, v)))
            counts.append(kids)
    return Case(cc.ios_array(rows), cc.offsets_of(counts), arena, max_len=64), cc.offsets_of(file_counts)


def test_hand_over_to_file_digest(hf, orc, dev):
    """client_read_batch -> file_digest_batch_ex (with and without FILL_ZERO) on one stream, one
    synchronize: the digests are FileWrapper::readFile's over the model's parents."""
    case, file_off = _files(orc)
    want = case.want(True, orc)
    assert want.info.tolist()[2] == 2 and want.blocks["missing"].sum() >= 10
    assert (want.blocks["read_len"] < want.blocks["block_len"]).sum() >= 20
    box = Box(dev, case)
    d_off = torch.from_numpy(file_off.view(np.int64).copy()).to(dev)
    nf = file_off.size - 1
    outs = [torch.full((nf * 24,), CANARY, dtype=torch.uint8, device=dev) for _ in range(2)]
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    box.call(hf, True, stream=st)
    for out, fill in zip(outs, (True, False)):
        hf._lib.file_digest_batch(box.blk, d_off, out, nf, 9, stream=st, fill_zero=fill)
    st.synchronize()
    box.check(want, "hand-over")
    digest = np.dtype([("length", "<u8"), ("value", "<u4"), ("type", "u1"), ("r", "u1", (3,)), ("status", "<i4"), ("r2", "<u4")])
    for out, fill in zip(outs, (True, False)):
        got = out.cpu().numpy().view(digest)
        for f in range(nf):
            blocks = cc.digest_blocks(want.blocks[int(file_off[f]):int(file_off[f + 1])])
            status, ck = orc.file_digest(blocks, fill_zero=fill)
            have = (int(got["status"][f]), (int(got["type"][f]), int(got["value"][f])) if status == 0 else (0, 0))
            assert have == (status, tuple(ck) if status == 0 else (0, 0)), (f, fill, have, status, ck)
            assert int(got["length"][f]) == 64 * (int(file_off[f + 1]) - int(file_off[f]))
    hf._lib.release_stream(st)


# ---- contexts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lane_max", [LANE, WAVE], ids=["lane", "wave"])
def test_poisoned_scratch(hf, orc, dev, opts, lane_max):
    """Every scratch word is written before it is read: the results do not change when the call's
    scratch starts from a pattern."""
    opts("poison", 0xA5A5A5A5)
    st = torch.cuda.Stream(dev)
    for case in (_shape(orc, 65), _grid(orc, cc.CRC32C, "typed"), _shape(orc, 3)):
        _run(hf, orc, dev, case, True, "poisoned", stream=st, max_children=lane_max)
    hf._lib.release_stream(st)


def test_scratch_bytes_covers_the_call(hf, orc, dev):
    L = hf._lib
    st = torch.cuda.Stream(dev)
    big = _singles(orc, 70001)[0]
    _run(hf, orc, dev, big, True, "largest", stream=st)
    st0 = L.pair_scratch_stats(st)
    assert st0["call_bytes"] >= L.client_read_scratch_bytes(70001, 70001) > 0
    for case in (_shape(orc, 1025), _grid(orc, cc.CRC32, "typed"), big):
        assert L.client_read_scratch_bytes(case.ios.size, case.n_parents) <= st0["call_bytes"]
        _run(hf, orc, dev, case, True, "smaller", stream=st)
    assert L.pair_scratch_stats(st) == st0
    L.release_stream(st)


def test_empty_batch_zeroes_info(hf, orc, dev):
    info = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    for verify in (True, False):
        info.fill_(0x5A5A5A5A)
        hf.client_read_batch(cc.CRC32C, None, 0, info, verify=verify, parents=0x1000)
        torch.cuda.synchronize()
        assert info.cpu().numpy().view(np.uint32).tolist() == [0] * 4 + [0x5A5A5A5A] * 4
    none = Case(cc.ios_array([]), cc.offsets_of([0, 0, 0]), None)
    assert _run(hf, orc, dev, none, True, "three parents, no IO").parents["status"].tolist() == [7003] * 3


def test_captured_call_replans_at_every_replay(hf, orc, dev):
    """Captured once; replayed on the records and bytes as captured, then with a byte of the data
    flipped, with records and offsets rewritten in place, and back: each replay is exact."""
    case = _shape(orc, SWITCH + 1)  # (one wave per parent)
    box = Box(dev, case)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        box.call(hf, True, stream=torch.cuda.current_stream())
    read = lambda a: (lambda addr, n: a[addr - REL:addr - REL + n].tobytes())  # noqa: E731
    flipped = case.arena.copy()
    victim = int(np.flatnonzero((case.ios["read_len"] > 4) & (case.ios["status_in"] == 0))[3])
    flipped[int(case.ios["data"][victim]) - REL + 2] ^= 0x20
    ios2 = case.ios.copy()
    ios2["status_in"][::9] = cc.CHUNK_NOT_FOUND
    ios2["read_len"][1::5] = 0
    off2 = case.off.copy()
    off2[1:-1] = np.sort(np.random.default_rng(9).integers(0, case.ios.size + 1, off2.size - 2))
    variants = [(case.ios, case.off, case.arena), (case.ios, case.off, flipped), (ios2, off2, case.arena),
                (case.ios, case.off, case.arena)]
    for k, (ios, off, arena) in enumerate(variants):
        sent = ios.copy()
        sent["data"] = np.where(ios["data"] != 0, ios["data"] - np.uint64(REL) + np.uint64(box.arena.data_ptr()), 0)
        box.ios[:sent.nbytes].copy_(torch.from_numpy(sent.view(np.uint8).copy()))
        box.off.copy_(torch.from_numpy(off.view(np.int64).copy()))
        box.arena.copy_(torch.from_numpy(arena.copy()))
        for t in (box.par, box.blk, box.info):
            t.fill_(CANARY)
        torch.cuda.synchronize()
        g.replay()
        want = cc.model(ios, off, case.ctype, case.max_len, True, orc, read(arena))
        box.check(want, f"replay {k}", sent=sent, arena=arena)
        if k == 1:
            assert want.status[victim] == cc.MISMATCH
    del g


_CHILD = r"""
import importlib, json, sys
import numpy as np, torch
repo, tests, path = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path[:0] = [repo, tests]
hf = importlib.import_module("3fs_amd")
z = np.load(path)
dev = torch.device("cuda:0")
arena = torch.from_numpy(z["arena"]).to(dev)
ios_h = z["ios"].copy()
data = ios_h.view("<u8").reshape(-1, 5)[:, 0]
data += np.uint64(arena.data_ptr() - int(z["rel"]))
ios = torch.from_numpy(ios_h).to(dev)
off = torch.from_numpy(z["off"].view(np.int64)).to(dev)
n, npar = ios.numel() // 40, off.numel() - 1
parents = torch.full((npar * 24,), 0x5A, dtype=torch.uint8, device=dev)
blocks = torch.full((npar * 24,), 0x5A, dtype=torch.uint8, device=dev)
info = torch.full((4,), -1, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library call, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            hf.client_read_batch(int(z["ctype"]), ios, n, info, parent_off=off, n_parents=npar,
                                 max_children=int(z["max_children"]), max_len=int(z["max_len"]), verify=True,
                                 parents=parents, blocks=blocks, stream=torch.cuda.current_stream())
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "client_read_batch failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
b = lambda t: t.cpu().numpy().view(np.uint8).tolist()
print(json.dumps({"ios": b(ios), "parents": b(parents), "blocks": b(blocks), "info": info.cpu().numpy().view(np.uint32).tolist(),
                  "base": arena.data_ptr()}))
"""


def test_first_call_in_process_is_captured(orc, tmp_path):
    """A fresh process whose first library call is a verifying client_read_batch inside
    torch.cuda.graph(capture_error_mode="global"): the context and the call's scratch are first
    allocated during the capture.  The child replays the graph once; every output is exact."""
    case = _shape(orc, 17)
    want = case.want(True, orc)
    path = str(tmp_path / "case.npz")
    np.savez(path, arena=case.arena, ios=case.ios.view(np.uint8), off=case.off, rel=REL, ctype=case.ctype,
             max_children=case.max_children, max_len=case.max_len)
    p = subprocess.run([sys.executable, "-c", _CHILD, REPO, os.path.join(REPO, "tests"), path],
                       capture_output=True, text=True, timeout=150, env=dict(os.environ), cwd=REPO)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    got = lines[0]
    ios = np.array(got["ios"], dtype=np.uint8).view(cc.IO)
    assert np.array_equal(ios["computed"], want.computed) and np.array_equal(ios["status"], want.status)
    assert np.array_equal(ios["data"], case.ios["data"] - np.uint64(REL) + np.uint64(got["base"]))
    assert np.array(got["parents"], dtype=np.uint8).tobytes() == want.parents.tobytes()
    assert np.array(got["blocks"], dtype=np.uint8).tobytes() == want.blocks.tobytes()
    assert got["info"] == want.info.tolist()


def test_registered_host_memory(hf, orc, dev):
    """Records, offsets, outputs and the data all in host memory registered with the library."""
    case = _shape(orc, 17)
    want = case.want(True, orc)
    n, npar = case.ios.size, case.n_parents
    sizes = [case.arena.size, n * 40, (npar + 1) * 8, npar * 24 + 2 * GUARD, npar * 24 + 2 * GUARD, 16 + 2 * GUARD]
    bufs = [hm.Registered(s) for s in sizes]
    try:
        arena, ios, off, par, blk, info = bufs
        arena.write(case.arena)
        sent = case.ios.copy()
        sent["data"] = case.ios["data"] - np.uint64(REL) + np.uint64(arena.dev)
        ios.write(sent.view(np.uint8))
        off.write(case.off.view(np.uint8))
        for b in (par, blk, info):
            b.host[:] = CANARY
        hf.client_read_batch(case.ctype, ios.dev, n, info.dev + GUARD, parent_off=off.dev, n_parents=npar,
                             max_children=case.max_children, max_len=case.max_len, verify=True, parents=par.dev + GUARD,
                             blocks=blk.dev + GUARD, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        got = ios.read().view(cc.IO)
        assert np.array_equal(got["computed"], want.computed) and np.array_equal(got["status"], want.status)
        for b, exp in ((par, want.parents.tobytes()), (blk, want.blocks.tobytes()), (info, want.info.tobytes())):
            raw = b.read()
            assert raw[GUARD:GUARD + len(exp)].tobytes() == exp
            assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + len(exp):] == CANARY).all()
        assert np.array_equal(arena.read(), case.arena)
    finally:
        torch.cuda.synchronize()
        for b in bufs:
            b.close()


def test_two_threads(hf, orc, dev):
    """Two host threads, a stream each, three verifying calls each: every pair has its own scratch."""
    cases = [_shape(orc, SWITCH + 1), _shape(orc, 17)]  # (a wave and a lane per parent)
    for c in cases:
        c.want(True, orc)
    errors = []

    def work(case):
        try:
            st = torch.cuda.Stream(dev)
            boxes = [Box(dev, case) for _ in range(3)]
            for b in boxes:
                b.call(hf, True, stream=st)
            st.synchronize()
            for k, b in enumerate(boxes):
                b.check(case.want(True, orc), f"thread call {k}")
            hf._lib.release_stream(st)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(c,)) for c in cases]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]


def test_queued_behind_fill_synth_and_update(hf, orc, dev, opts):
    """fill_synth writes the chunks, an update_batch takes the pair's call buffer, and the client
    call verifies children cut from the freshly written chunks directly behind both: one stream,
    one wait.  Then the same queue again on poisoned scratch."""
    L = hf._lib
    chunks, chunk_len, seed = 16, (8 << 10) + 8, 0xC1
    arena = np.concatenate([orc.fill_synth(chunk_len, seed, 3 + i) for i in range(chunks)])
    rng = np.random.default_rng(3)
    rows, counts = [], []
    for p in range(120):
        kids = 1 + p % 5
        for j in range(kids):
            ln = int(rng.integers(0, 3000))
            at = int(rng.integers(0, arena.size - ln))
            v = orc.create(cc.CRC32C, arena[at:at + ln].tobytes())[1] ^ (4 if (p, j) == (51, 1) and ln else 0)
            rows.append((REL + at, ln, ln, 0, (cc.CRC32C, v)))
        counts.append(kids)
    case = Case(cc.ios_array(rows), cc.offsets_of(counts), arena, max_len=3000)
    want = case.want(True, orc)
    assert np.count_nonzero(want.status) == 1
    q = stream_queue.DeviceQueue(stream_queue._scenario(orc, "rounds", 1, 1), dev)
    st = torch.cuda.Stream(dev)
    for poison in (0, 0xA5A5A5A5):
        box = Box(dev, case)
        box.arena.zero_()
        q.restore()
        opts("poison", poison)
        torch.cuda.synchronize()
        L.fill_synth(box.arena, chunk_len, chunk_len, chunks, seed, 3, stream=st)
        q.call(L, 0, 1, st)
        box.call(hf, True, stream=st)
        st.synchronize()
        box.check(want, f"behind fill_synth and update_batch (poison {poison:#x})")
        q.check()
    L.release_stream(st)


# ---- the read footprint -----------------------------------------------------------------------
def test_read_footprint(tmp_path):
    """tests/client_read_footprint.py in a child process against the load-checked build: per call
    Required <= Read <= Legal over the data buffers, nothing refused, no descriptor index >= n,
    outputs equal to the model's; without VERIFY no granule of a data buffer is read."""
    import client_read_footprint as crf
    import load_footprint as lf
    check_lib = os.path.join(REPO, "3fs_amd", "lib", "libhf3fs_crc_loadcheck.so")
    assert os.path.exists(check_lib), f"{check_lib} missing: 3fs_amd/build.py builds it beside the default library"
    out = str(tmp_path / "client_read.json")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "client_read_footprint.py"), out],
                       capture_output=True, text=True, timeout=240, env=dict(os.environ, HF3FS_CRC_LIB=check_lib))
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    with open(out) as f:
        reports = json.load(f)["reports"]
    cases = crf.cases()
    assert sorted(reports) == sorted(c.name for c in cases) and len(cases) >= 12
    bad = []
    for c in cases:
        defects = lf.compare(c, reports[c.name])
        if defects:
            bad.append(lf.describe(c, defects))
        if not c.verify:
            read, _ = lf.mask_from_runs(reports[c.name]["read"], c.n_granules)
            assert not read.any(), f"{c.name}: {int(read.sum())} granules read without VERIFY"
            assert not reports[c.name]["counters"], (c.name, reports[c.name]["counters"])
        else:
            assert reports[c.name]["counters"], f"{c.name}: no checked load was counted"
    assert not bad, f"{len(bad)} of {len(cases)} calls:\n" + "\n".join(bad[:12])
