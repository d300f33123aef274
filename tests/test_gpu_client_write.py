"""hf3fs_crc_client_write_prepare / _complete on the GPU.

Every expectation comes from tests/client_write_cases.py: the reference's loops restated in Python
over the CPU oracle's CRC (and, end to end, the oracle's ChunkReplica::update).  After every call
the whole IO array, the whole update array around its guard pattern (so only the named fields may
change), every byte of the file records, the failed list, the eight info words, the guard bytes
around every output array and the data arena (unchanged) are compared.
"""
import functools

import numpy as np
import pytest

import client_write_cases as wc
import host_memory as hm

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
GUARD = 64          # bytes in front of and behind every output array that no call may write
CANARY = 0x5A
REL = 1 << 16       # a case's addresses are REL + the offset in its arena (0 stays 0: no buffer)
SWITCH = 128        # kClientWriteLaneMaxIos: files of more IOs take one wave each
LANE, WAVE = 1, 1 << 30  # max_ios_per_file that make any call take one lane / one wave per file
TYPES = pytest.mark.parametrize("ctype", [wc.CRC32C, wc.CRC32], ids=["crc32c", "crc32"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _guarded(dev, nbytes):
    t = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
    return t, t[GUARD:GUARD + nbytes]


def _put(t, a):
    if a.nbytes:
        t[:a.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))


def _guards_ok(what, **raws):
    for name, raw in raws.items():
        g = raw.cpu().numpy()
        assert (g[:GUARD] == CANARY).all() and (g[-GUARD:] == CANARY).all(), f"{what}: bytes around {name} written"


def _same_records(what, name, got, exp):
    if got.tobytes() == exp.tobytes():
        return
    assert got.size == exp.size, f"{what}: {name} count"
    for f in exp.dtype.names:
        bad = np.flatnonzero((got[f] != exp[f]).reshape(got.size, -1).any(axis=1))
        if bad.size:
            i = int(bad[0])
            pytest.fail(f"{what}: {bad.size} {name} differ in {f}, first {i}: got {got[f][i]}, want {exp[f][i]} ({exp[i]})")


def _relocate(ios, base):
    sent = ios.copy()
    for f in ("data", "buf_base"):
        sent[f] = np.where((ios[f] >= REL) & (ios[f] < (1 << 40)), ios[f] - np.uint64(REL) + np.uint64(base), ios[f])
    return sent


# ---- prepare ------------------------------------------------------------------------------------
class PrepCase:
    """ios with arena-relative addresses and the arena's bytes.  Never modified once built."""

    def __init__(self, ios, arena, ctype=wc.CRC32C, max_len=4097, max_inline=16):
        self.ios, self.arena, self.ctype, self.max_len, self.max_inline = ios, arena, ctype, max_len, max_inline
        ios.setflags(write=False)
        arena.setflags(write=False)
        self._want = {}

    def read(self, addr, n):
        assert REL <= addr and addr + n <= REL + self.arena.size, "the model read outside the arena"
        return self.arena[addr - REL:addr - REL + n].tobytes()

    def want(self, verify, orc):
        if verify not in self._want:
            self._want[verify] = wc.prepare_model(self.ios, self.ctype, self.max_len, self.max_inline, verify, orc, self.read)
        return self._want[verify]


def update_pattern(n):
    """Update records as a server prepared them: a pattern in every byte, so a stray store shows."""
    return np.frombuffer((bytes(range(0x40, 0x40 + 56)) * n), dtype=wc.UPDATE).copy()


class PrepBox:
    def __init__(self, dev, case, updates=True):
        self.case = case
        self.arena = torch.from_numpy(case.arena.copy()).to(dev)
        assert self.arena.data_ptr() % 16 == 0
        self.sent = _relocate(case.ios, self.arena.data_ptr())
        n = case.ios.size
        self.ios_raw, self.ios = _guarded(dev, max(n, 1) * 64)
        _put(self.ios, self.sent)
        self.before = update_pattern(n)
        self.upd_raw, self.upd = _guarded(dev, max(n, 1) * 56)
        _put(self.upd, self.before)
        self.use_updates = updates
        self.info_raw, self.info = _guarded(dev, 32)
        torch.cuda.synchronize()

    def call(self, hf, verify, stream=None):
        c = self.case
        hf.client_write_prepare(c.ctype, self.ios if c.ios.size else None, c.ios.size, self.info, c.max_len,
                                max_inline_bytes=c.max_inline, verify=verify,
                                updates=self.upd if self.use_updates else None, stream=stream or torch.cuda.current_stream())

    def check(self, want, what):
        torch.cuda.synchronize()
        c = self.case
        n = c.ios.size
        _guards_ok(what, d_ios=self.ios_raw, d_updates=self.upd_raw, d_info=self.info_raw)
        got = self.ios.cpu().numpy()[:n * 64].view(wc.IO)
        _same_records(what, "IOs", got, want.apply(self.sent))
        upd = self.upd.cpu().numpy()[:n * 56].view(wc.UPDATE)
        _same_records(what, "update records", upd, want.updates(self.sent, self.before) if self.use_updates else self.before)
        info = self.info.cpu().numpy().view(np.uint32)
        assert info.tolist() == want.info.tolist(), f"{what}: info {dict(zip(wc.PREP_INFO, info.tolist()))}, want {want.info.tolist()}"
        assert np.array_equal(self.arena.cpu().numpy(), c.arena), f"{what}: the data arena changed"


def _prep(hf, orc, dev, case, verify, what, updates=True, stream=None):
    box = PrepBox(dev, case, updates)
    box.call(hf, verify, stream)
    want = case.want(verify, orc)
    box.check(want, what)
    return want


ARENA = 1 << 16


def _case(rows, ctype=wc.CRC32C, seed=1, **kw):
    return PrepCase(wc.ios_array(rows), wc.arena_bytes(ARENA, seed), ctype, **kw)


GOOD = (REL + 256, REL, ARENA, 0, 40, 64)


@functools.lru_cache(maxsize=None)
def _counted(n, ctype):
    """n IOs of 0-16 bytes; every 37th fails its own range, every 53rd is a bad record (none when n is small)."""
    rng = np.random.default_rng(n)
    rows = wc.random_rows(rng, n, REL, ARENA)
    for i in range(36, n, 37):
        rows[i] = rows[i][:3] + (60, 5, 64)
    for i in range(52, n, 53):
        rows[i] = rows[i][:4] + (18, 64)
    return _case(rows, ctype, seed=n, max_len=16, max_inline=8)


@TYPES
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_prepare_counts(hf, orc, dev, ctype, n):
    case = _counted(n, ctype)
    want = _prep(hf, orc, dev, case, True, f"{n} IOs")
    assert want.info[0] + want.info[1] + want.info[2] == n and want.info[3] == 0
    if n >= 257:
        assert want.info[1] > 0 and want.info[2] > 0 and 0 < want.info[4] < want.info[0]
    _prep(hf, orc, dev, case, False, f"{n} IOs, no VERIFY")
    _prep(hf, orc, dev, case, True, f"{n} IOs, NULL updates", updates=False)


@TYPES
def test_prepare_grid_of_lengths_and_residues(hf, orc, dev, ctype):
    """Lengths 0, 1, 15, 16, 17, 4095, 4096, 4097 with data at every residue mod 16."""
    arena = wc.arena_bytes(wc.grid_bytes(), 0x6121D + ctype)
    case = PrepCase(wc.ios_array(wc.grid_rows(REL, arena.size)), arena, ctype, max_len=4097, max_inline=16)
    want = _prep(hf, orc, dev, case, True, "grid")
    assert (want.status == 0).all() and (want.checksum_type == ctype).all()
    assert set(want.checksum[np.flatnonzero(case.ios["length"] == 0)].tolist()) == {wc.M32}
    assert want.info.tolist() == [128, 0, 0, 0, 16 * 4, 16 * sum(wc.LENGTHS), 0, 0]
    none = _prep(hf, orc, dev, case, False, "grid, no VERIFY")
    assert (none.checksum == 0).all() and (none.checksum_type == wc.NONE).all() and none.info[5] == 0


@TYPES
def test_prepare_as_byte_runs(hf, orc, dev, ctype):
    """max_len only bounds the lengths, and from 1 MiB on a batch with n * max_len >= 1 GiB hashes
    as byte runs: the other schedule of the range kernels, over the same small payloads."""
    counted = _counted(4097, ctype)
    wide = PrepCase(counted.ios.copy(), counted.arena.copy(), ctype, max_len=1 << 20, max_inline=8)
    want = _prep(hf, orc, dev, wide, True, "4097 IOs as byte runs")
    assert want.info[2] == 0 and want.info[1] > 0                     # (18 bytes are no bad record under this bound)
    arena = wc.arena_bytes(wc.grid_bytes(), 0xB17E + ctype)
    grid = PrepCase(wc.ios_array(wc.grid_rows(REL, arena.size)), arena, ctype, max_len=8 << 20, max_inline=16)
    assert (_prep(hf, orc, dev, grid, True, "grid as byte runs").status == 0).all()
    below = PrepCase(grid.ios.copy(), arena.copy(), ctype, max_len=(8 << 20) - 1, max_inline=16)   # 1 GiB less 128 B: the planner
    assert np.array_equal(_prep(hf, orc, dev, below, True, "grid below the bound").checksum, grid.want(True, orc).checksum)


@TYPES
def test_prepare_grid_stride(hf, orc, dev, ctype):
    """2^20 + 300 IOs of 0-16 bytes: more than the grid holds at once.  The expectation is a numpy
    restatement of the rules for this shape (no offender, so no poison), itself held to the model
    on the first 3,000 IOs; the CRCs are the oracle's over the 4,096 distinct payloads."""
    n = (1 << 20) + 300
    rng = np.random.default_rng(20)
    arena = wc.arena_bytes(ARENA, 20)
    pool_at, pool_len = rng.integers(0, ARENA - 16, 4096), rng.integers(0, 17, 4096)
    pool_crc = np.array([orc.create(ctype, arena[a:a + k].tobytes())[1] for a, k in zip(pool_at, pool_len)], dtype=np.uint32)
    pick = rng.integers(0, 4096, n)
    ios = np.zeros(n, dtype=wc.IO)
    ios["data"], ios["buf_base"], ios["buf_size"] = REL + pool_at[pick], REL, ARENA
    ios["length"], ios["chunk_size"] = pool_len[pick], 64
    ios["offset"] = rng.integers(0, 49, n)
    ios["offset"][::37] = 64                      # own range: fails unless the length is 0
    ios["length"][5::53] = 17                     # bad records (max_len 16)
    ios["checksum"], ios["checksum_type"], ios["send_inline"], ios["status"] = wc.POISON_OUT, 0xA5, 0xA5, -2
    ios["status_in"] = wc.NOT_INITIALIZED
    bad = ios["length"] > 16
    rng_fail = ~bad & ((ios["offset"] + ios["length"]) > ios["chunk_size"])
    sent = ~bad & ~rng_fail
    exp = ios.copy()
    exp["status"] = np.where(bad, 3, np.where(rng_fail, 7002, 0))
    exp["checksum"] = np.where(sent, pool_crc[pick], 0)
    exp["checksum_type"] = np.where(sent, ctype, 0)
    exp["send_inline"] = sent & (ios["length"] <= 8)
    hashed = int(ios["length"][sent].sum())
    info = [int(sent.sum()), int(rng_fail.sum()), int(bad.sum()), 0, int(exp["send_inline"].sum()), hashed & wc.M32, hashed >> 32, 0]
    head = PrepCase(ios[:3000].copy(), arena.copy(), ctype, max_len=16, max_inline=8).want(True, orc)
    assert head.apply(ios[:3000]).tobytes() == exp[:3000].tobytes() and min(info[:3]) > 1000
    d_arena = torch.from_numpy(arena).to(dev)
    relocated = _relocate(ios, d_arena.data_ptr())
    d_ios = torch.from_numpy(relocated.view(np.uint8).reshape(-1)).to(dev)
    d_info = torch.full((8,), -1, dtype=torch.int32, device=dev)
    hf.client_write_prepare(ctype, d_ios, n, d_info, 16, max_inline_bytes=8, verify=True, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = d_ios.cpu().numpy().view(wc.IO)
    want = _relocate(exp, d_arena.data_ptr())
    for f in wc.IO.names:
        bad_at = np.flatnonzero((got[f] != want[f]).reshape(n, -1).any(axis=1))
        assert not bad_at.size, f"{bad_at.size} IOs differ in {f}, first {bad_at[0]}: {got[bad_at[0]]} want {want[bad_at[0]]}"
    assert d_info.cpu().numpy().view(np.uint32).tolist() == info


def test_range_rule(hf, orc, dev):
    rows = [GOOD[:3] + (24, 40, 64),                      # offset + length == chunk_size
            GOOD[:3] + (25, 40, 64),                      # + 1
            GOOD[:3] + (0, 0, 0),                         # chunk_size 0
            GOOD[:3] + (0xFFFFFFF0, 0x20, 0x100),         # the uint32 sum wraps to 0x10: passes
            GOOD[:3] + (0xFFFFFFF0, 0x10, 0x100),         # wraps to 0 exactly: passes
            GOOD[:3] + (0xFFFFFF00, 0x20, 0xFFFFFF10)]    # no wrap, beyond: fails
    want = _prep(hf, orc, dev, _case(rows), True, "range rule")
    assert want.status.tolist() == [0, 7002, 7002, 0, 0, 7002] and want.info.tolist()[:4] == [3, 3, 0, 0]


def test_containment(hf, orc, dev):
    edge = [(REL, REL, ARENA, 0, 40, 64),                          # data == buf_base
            (REL + ARENA - 40, REL, ARENA, 0, 40, 64),             # data + length == buf_base + buf_size
            (REL + ARENA, REL, ARENA, 0, 0, 64),                   # an empty range at the very end
            (REL + 512, REL + 512, 40, 0, 40, 64)]                 # a buffer of exactly the IO
    want = _prep(hf, orc, dev, _case(edge), True, "containment edges")
    assert want.status.tolist() == [0] * 4 and want.info[3] == 0
    for name, off in (("one past the end", (REL + ARENA - 39, REL, ARENA, 0, 40, 64)),
                      ("data below the buffer", (REL + 100, REL + 101, ARENA - 101, 0, 40, 64)),
                      ("data + length wraps", (wc.M64 - 8, 1 << 41, wc.M64 - (1 << 41), 0, 40, 64)),
                      ("buf_base + buf_size wraps", ((1 << 63) + 64, 1 << 63, 1 << 63, 0, 40, 64)),
                      ("data == 0", (0, REL, ARENA, 0, 40, 64)), ("buf_base == 0", (REL, 0, wc.M64, 0, 40, 64))):
        want = _prep(hf, orc, dev, _case([GOOD, off, GOOD]), True, name)
        assert want.status.tolist() == [7002] * 3 and want.info.tolist() == [0, 0, 0, 1, 0, 80, 0, 0], name


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "plain"])
def test_poison(hf, orc, dev, verify):
    off = (REL + ARENA - 3, REL, ARENA, 0, 4, 64)
    for name, rows in (("first", [off] + [GOOD] * 70), ("last", [GOOD] * 70 + [off]), ("alone", [off]),
                       ("among dropped", [GOOD[:3] + (60, 40, 64), off, GOOD[:4] + (5000, 8192), GOOD])):
        want = _prep(hf, orc, dev, _case(rows), verify, f"offender {name}")
        assert want.info[3] == 1 and want.info[0] == 0 and not (want.status == 0).any(), name
        assert (want.checksum == 0).all() and (want.checksum_type == 0).all() and (want.send_inline == 0).all()
    # an offender that rule 1 or rule 2 already dropped does not poison
    rows = [GOOD, (0, 0, 0, 60, 40, 64), (REL + ARENA, REL, ARENA, 0, 5000, 8192), (REL - 1, REL, ARENA, 0, 4, 0), GOOD]
    want = _prep(hf, orc, dev, _case(rows), verify, "dropped offenders")
    assert want.status.tolist() == [0, 7002, 3, 7002, 0] and want.info.tolist()[:4] == [2, 2, 1, 0]


def test_bad_records_and_inline(hf, orc, dev):
    rows = [GOOD[:4] + (4097, 8192), GOOD[:4] + (4098, 8192), GOOD[:4] + (16, 64), GOOD[:4] + (17, 64), GOOD[:4] + (0, 64)]
    want = _prep(hf, orc, dev, _case(rows), True, "max_len and inline")
    assert want.status.tolist() == [0, 3, 0, 0, 0] and want.send_inline.tolist() == [0, 0, 1, 0, 1]
    zero = _prep(hf, orc, dev, _case(rows, max_inline=0), False, "inline 0")
    assert zero.send_inline.tolist() == [0, 0, 0, 0, 1]            # 0 against 0
    assert zero.info.tolist() == [4, 0, 1, 0, 1, 0, 0, 0]


def test_empty_prepare_sets_info(hf, dev):
    info = torch.full((12,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    for verify in (True, False):
        info.fill_(0x5A5A5A5A)
        hf.client_write_prepare(wc.CRC32C, None, 0, info, 64, verify=verify, updates=0x1000)
        torch.cuda.synchronize()
        assert info.cpu().numpy().view(np.uint32).tolist() == [0] * 8 + [0x5A5A5A5A] * 4


# ---- complete -----------------------------------------------------------------------------------
class DoneCase:
    """ios as complete receives them, file offsets, optional update records and expected values."""

    def __init__(self, ios, off, updates=None, expected=None):
        self.ios, self.off, self.updates, self.expected = ios, off, updates, expected
        self.n_files = 0 if off is None else off.size - 1
        self.max_ios = 1 if off is None else int(np.diff(off.astype(np.int64)).max(initial=1))
        self._want = None

    def want(self, orc):
        if self._want is None:
            self._want = wc.complete_model(self.ios, self.off, orc, self.updates, self.expected)
        return self._want


class DoneBox:
    def __init__(self, dev, case, failed_cap=None):
        self.case = case
        n = case.ios.size
        self.ios_raw, self.ios = _guarded(dev, max(n, 1) * 64)
        _put(self.ios, case.ios)
        self.off = None if case.off is None else torch.from_numpy(case.off.view(np.int64).copy()).to(dev)
        self.upd = None if case.updates is None else torch.from_numpy(case.updates.view(np.uint8).reshape(-1).copy()).to(dev)
        self.exp = None if case.expected is None else torch.from_numpy(np.asarray(case.expected, dtype=np.uint32).view(np.int32).copy()).to(dev)
        self.files_raw, self.files = _guarded(dev, max(case.n_files, 1) * 24)
        self.cap = n if failed_cap is None else failed_cap
        self.failed_raw, self.failed = _guarded(dev, max(self.cap, 1) * 4)
        self.info_raw, self.info = _guarded(dev, 32)
        torch.cuda.synchronize()

    def call(self, hf, stream=None, max_ios=None):
        c = self.case
        hf.client_write_complete(self.ios if c.ios.size else None, c.ios.size, self.info, file_off=self.off,
                                 n_files=c.n_files, max_ios_per_file=c.max_ios if max_ios is None else max_ios,
                                 updates=self.upd, expected=self.exp, files=self.files if c.n_files else None,
                                 failed=self.failed if self.cap else None, failed_cap=self.cap,
                                 stream=stream or torch.cuda.current_stream())

    def images(self):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy().tobytes() for t in (self.ios_raw, self.files_raw, self.failed_raw, self.info_raw))

    def check(self, want, what):
        torch.cuda.synchronize()
        c = self.case
        n = c.ios.size
        _guards_ok(what, d_ios=self.ios_raw, d_files=self.files_raw, d_failed=self.failed_raw, d_info=self.info_raw)
        _same_records(what, "IOs", self.ios.cpu().numpy()[:n * 64].view(wc.IO), want.ios)
        files = self.files.cpu().numpy()
        _same_records(what, "files", files[:c.n_files * 24].view(wc.FILE), want.files)
        assert (files[c.n_files * 24:] == CANARY).all(), f"{what}: files written past n_files"
        failed = self.failed.cpu().numpy()
        k = min(self.cap, want.failed.size)
        assert failed[:k * 4].view(np.uint32).tolist() == want.failed[:k].tolist(), f"{what}: the failed list"
        assert (failed[k * 4:] == CANARY).all(), f"{what}: the failed list written past min(count, failed_cap)"
        info = self.info.cpu().numpy().view(np.uint32)
        assert info.tolist() == want.info.tolist(), f"{what}: info {dict(zip(wc.DONE_INFO, info.tolist()))}, want {want.info.tolist()}"
        if self.upd is not None:
            assert self.upd.cpu().numpy().tobytes() == c.updates.tobytes(), f"{what}: the update records changed"


def _done(hf, orc, dev, case, what, failed_cap=None, stream=None, max_ios=None):
    box = DoneBox(dev, case, failed_cap)
    box.call(hf, stream, max_ios)
    want = case.want(orc)
    box.check(want, what)
    return want, box.images()


FILE_SIZES = (0, 1, 2, 63, 64, 65, SWITCH, SWITCH + 1, 1000)


@functools.lru_cache(maxsize=None)
def _shapes(orc, k, ctype=wc.CRC32C):
    """Files of k IOs, one per variant of the fold (those that need an IO are left out for k == 0),
    with files of 0 and 1 IOs between them so that the offsets are not a multiple of k."""
    rng = np.random.default_rng(3000 + k)
    other = wc.CRC32 if ctype == wc.CRC32C else wc.CRC32C
    lengths, status, answers, counts, names = [], [], [], [], []

    def file(name, n, edit=None, types=(ctype,), zero_every=0):
        ans, lens = wc.random_answers(rng, n, types=types, zero_every=zero_every, big=n < 100)
        st = [0] * n
        if edit:
            edit(ans, lens, st)
        answers.extend(ans), lengths.extend(lens), status.extend(st), counts.append(len(ans)), names.append(name)

    def at(pos, answer=None, length=None, st=None, insert=False):
        def edit(ans, lens, sts):
            if insert:
                ans.insert(pos, answer), lens.insert(pos, answer[1] if length is None else length), sts.insert(pos, 0)
                return
            if answer is not None:
                ans[pos] = answer
                lens[pos] = answer[1]
            if length is not None:
                lens[pos] = length
            if st is not None:
                sts[pos] = st
        return edit

    def both(*edits):
        def edit(ans, lens, sts):
            for e in edits:
                e(ans, lens, sts)
        return edit

    file("clean", k)
    file("empty", 0)
    file("zero lengths", k, zero_every=3)
    file("all NONE", k, types=(wc.NONE,))
    file("one", 1)
    if k:
        for pos in sorted({0, k // 2, k - 1}):
            file(f"status at {pos}", k, at(pos, answer=(4010, 7, (ctype, 1))))
            file(f"short at {pos}", k, at(pos, length=5, answer=(0, 4, (ctype, 1))))
            file(f"unknown type at {pos}", k, at(pos, answer=(0, 9, (7, 1))))
            file(f"prepare status at {pos}", k, at(pos, st=wc.CLIENT_INVALID_ARG))
        if k > 1:
            file("two enders", k, both(at((k - 1) // 2, answer=(7003, 0, (0, 0))), at(k - 1, answer=(4080, 0, (0, 0)))))
        file("foreign zero in front", k, at(0, answer=(0, 0, (other, 5)), insert=True))
        file("foreign zero behind", k, at(k, answer=(0, 0, (other, 5)), insert=True))
        file("foreign zero in the middle", k, at(max(k // 2, 1), answer=(0, 0, (other, 5)), insert=True))
        file("NONE zero behind", k, at(k, answer=(0, 0, (wc.NONE, 0)), insert=True))
        file("NONE with bytes behind", k, at(k, answer=(0, 12, (wc.NONE, 0)), insert=True))
        file("foreign with bytes behind", k, at(k, answer=(0, 12, (other, 3)), insert=True))
        file("NONE in front, typed behind", k, at(0, answer=(0, 12, (wc.NONE, 77)), insert=True))
    ios = wc.ios_array([(0, 0, 0, 0, ln, 64) for ln in lengths])
    return DoneCase(wc.with_answers(ios, status, answers), wc.offsets_of(counts)), names


@TYPES
@pytest.mark.parametrize("k", FILE_SIZES)
def test_fold_shapes_under_both_schedules(hf, orc, dev, k, ctype):
    case, names = _shapes(orc, k, ctype)
    want, chosen = _done(hf, orc, dev, case, f"files of {k}")
    st = dict(zip(names, want.files["status"].tolist()))
    assert st["clean"] == st["empty"] == st["zero lengths"] == st["all NONE"] == 0
    if k:
        assert st["foreign zero in front"] == 0 and st["NONE in front, typed behind"] == 0
        for name in ("foreign zero behind", "NONE zero behind", "NONE with bytes behind", "foreign with bytes behind",
                     "foreign zero in the middle"):
            assert st[name] == 4080, name
        if k > 1:
            f = names.index("two enders")
            assert st["two enders"] == 7003 and want.files["failed_io"][f] == int(case.off[f]) + (k - 1) // 2
        assert {st[f"status at {k - 1}"], st[f"short at {k - 1}"], st[f"unknown type at {k - 1}"],
                st[f"prepare status at {k - 1}"]} == {4010, 33, 3, 7002}
        assert want.files["type"][names.index("all NONE")] == wc.NONE and want.files["type"][0] == ctype
    _, lane = _done(hf, orc, dev, case, f"files of {k}, one lane each", max_ios=LANE)
    _, wave = _done(hf, orc, dev, case, f"files of {k}, one wave each", max_ios=WAVE)
    assert chosen == lane == wave


def test_expected_values_and_failed_list(hf, orc, dev):
    base, names = _shapes(orc, 65)
    want = base.want(orc)
    expected = want.files["value"].copy()
    clean = [f for f in range(base.n_files) if want.files["status"][f] == 0]
    miss = clean[::2]
    expected[miss] ^= 0x100
    case = DoneCase(base.ios, base.off, expected=expected)
    got, _ = _done(hf, orc, dev, case, "d_expected")
    assert got.files["status"][miss].tolist() == [7015] * len(miss) and got.info[5] == len(miss)
    assert (got.files["failed_io"][miss] == wc.NO_IO).all() and got.info[4] == want.info[4] + len(miss)
    assert (got.files["status"][clean[1::2]] == 0).all()
    count = int(want.info[0])
    assert count >= 8 and np.array_equal(want.failed, np.flatnonzero(
        (base.ios["status"] != 0) | (base.ios["status_in"] != 0)))
    for cap in (0, 3, count - 1, count, base.ios.size):
        _done(hf, orc, dev, base, f"failed_cap {cap}", failed_cap=cap)
    # without files: the IO verdicts, the list and the counters alone
    got, _ = _done(hf, orc, dev, DoneCase(base.ios, None), "no files")
    assert got.info.tolist()[:4] == want.info.tolist()[:4] and got.info.tolist()[4:] == [0] * 4


def test_data_length_carries_into_the_high_word(hf, orc, dev):
    ios = wc.ios_array([(0, 0, 0, 0, 0xFFFFFF00, 64)] * 700)
    case = DoneCase(wc.with_answers(ios, [0] * 700, [(0, 0xFFFFFF00, (wc.CRC32C, i)) for i in range(700)]), wc.offsets_of([700]))
    want, _ = _done(hf, orc, dev, case, "2.8 TiB of answers")
    assert want.info[3] == (700 * 0xFFFFFF00) >> 32 and want.files["length"][0] == 700 * 0xFFFFFF00


def test_empty_complete_sets_info_and_files(hf, orc, dev):
    info = torch.full((12,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    hf.client_write_complete(None, 0, info)
    torch.cuda.synchronize()
    assert info.cpu().numpy().view(np.uint32).tolist() == [0] * 8 + [0x5A5A5A5A] * 4
    want, _ = _done(hf, orc, dev, DoneCase(wc.ios_array([]), wc.offsets_of([0, 0, 0])), "three files, no IO")
    assert want.files["status"].tolist() == [0, 0, 0] and want.files["failed_io"].tolist() == [wc.NO_IO] * 3


# ---- end to end: Bench.cc's writeFileAndCheck -----------------------------------------------------
CHUNK = 4096


class Bench:
    """Files cut by prepareBlocks, every block on a fresh chunk of its own."""

    def __init__(self, orc, ctype, ranges, seed=7):
        self.ctype = ctype
        rng = np.random.default_rng(seed)
        total = sum(end - start for start, end in ranges)
        self.arena = rng.integers(0, 256, max(total, 16), dtype=np.uint8)
        rows, counts, self.file_bytes, at = [], [], [], 0
        for start, end in ranges:
            blocks = wc.prepare_blocks(start, end, CHUNK)
            self.file_bytes.append((at, end - start))
            for _chunk, off, length in blocks:
                rows.append((REL + at, REL, self.arena.size, off, length, CHUNK))
                at += length
            counts.append(len(blocks))
        self.ios = wc.ios_array(rows)
        self.off = wc.offsets_of(counts)
        self.n = self.ios.size
        self.expected = np.array([orc.create(ctype, self.arena[a:a + k].tobytes())[1] for a, k in self.file_bytes], dtype=np.uint32)

    def updates(self, chunks_base):
        u = np.frombuffer(bytes([0xEE]) * (56 * self.n), dtype=wc.UPDATE).copy()
        u["chunk"] = chunks_base + np.arange(self.n, dtype=np.uint64) * CHUNK
        u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = 0, wc.NONE, 0   # fresh chunks
        return u

    def model(self, orc, arena_at_update, expected=True):
        """prepare over the arena as it is, the oracle's ChunkReplica::update over the arena as the
        update sees it, complete over those answers."""
        read = lambda a, k: self.arena[a - REL:a - REL + k].tobytes()  # noqa: E731
        prep = wc.prepare_model(self.ios, self.ctype, CHUNK, 0, True, orc, read)
        assert (prep.status == 0).all()
        upd = np.zeros(self.n, dtype=wc.UPDATE)
        chunks = np.zeros((self.n, CHUNK), dtype=np.uint8)
        for i in range(self.n):
            off, ln, a = int(self.ios["offset"][i]), int(self.ios["length"][i]), int(self.ios["data"][i]) - REL
            chunk = bytearray(CHUNK)
            st, size, ck = orc.replica_apply(chunk, 0, (wc.NONE, 0), orc.WRITE, off, ln, arena_at_update[a:a + ln].tobytes(),
                                             (int(prep.checksum_type[i]), int(prep.checksum[i])), chunk_size=CHUNK)
            upd["status"][i], upd["length"][i], upd["out_size"][i] = st, ln, size
            upd["out_checksum_type"][i], upd["out_checksum"][i] = ck
            chunks[i] = np.frombuffer(bytes(chunk), dtype=np.uint8)
        done = wc.complete_model(prep.apply(self.ios), self.off, orc, updates=upd, expected=self.expected if expected else None)
        return prep, upd, chunks, done


class BenchBox:
    def __init__(self, dev, bench):
        self.b = bench
        self.arena = torch.from_numpy(bench.arena.copy()).to(dev)
        self.chunks = torch.full((bench.n * CHUNK,), 0xCC, dtype=torch.uint8, device=dev)
        self.sent = _relocate(bench.ios, self.arena.data_ptr())
        self.ios = torch.from_numpy(self.sent.view(np.uint8).reshape(-1).copy()).to(dev)
        self.upd0 = bench.updates(self.chunks.data_ptr())
        self.upd = torch.from_numpy(self.upd0.view(np.uint8).reshape(-1).copy()).to(dev)
        self.off = torch.from_numpy(bench.off.view(np.int64).copy()).to(dev)
        self.exp = torch.from_numpy(bench.expected.view(np.int32).copy()).to(dev)
        nf = bench.off.size - 1
        self.files = torch.full((nf * 24,), CANARY, dtype=torch.uint8, device=dev)
        self.failed = torch.full((bench.n * 4,), CANARY, dtype=torch.uint8, device=dev)
        self.info = torch.full((16,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def queue(self, hf, mode, stream, sync=False, between=None, expected=True):
        b = self.b
        step = (lambda: stream.synchronize()) if sync else (lambda: None)
        hf.client_write_prepare(b.ctype, self.ios, b.n, self.info[:8], CHUNK, verify=True, updates=self.upd, stream=stream)
        step()
        if between:
            between()
        hf._lib.update_batch(b.ctype, self.upd, b.n, CHUNK, mode=mode, stream=stream)
        step()
        hf.client_write_complete(self.ios, b.n, self.info[8:], file_off=self.off, n_files=b.off.size - 1,
                                 max_ios_per_file=int(np.diff(b.off.astype(np.int64)).max()), updates=self.upd,
                                 expected=self.exp if expected else None, files=self.files, failed=self.failed,
                                 failed_cap=b.n, stream=stream)

    def images(self):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy().tobytes() for t in (self.ios, self.upd, self.files, self.failed, self.info, self.chunks))

    def check(self, model, what):
        torch.cuda.synchronize()
        prep, upd, chunks, done = model
        b = self.b
        got = self.ios.cpu().numpy().view(wc.IO)
        want = done.ios.copy()
        want["data"], want["buf_base"] = self.sent["data"], self.sent["buf_base"]
        _same_records(what, "IOs", got, want)
        u = self.upd.cpu().numpy().view(wc.UPDATE)
        request = prep.updates(self.sent, self.upd0)
        for f in ("chunk", "payload", "offset", "length", "chunk_size", "update_type", "chunk_checksum_type",
                  "write_checksum_type", "flags", "chunk_checksum", "write_checksum"):
            assert np.array_equal(u[f], request[f]), f"{what}: update field {f}"
        for f in ("status", "out_checksum", "out_checksum_type"):
            assert np.array_equal(u[f], upd[f]), f"{what}: update field {f}: {u[f].tolist()} want {upd[f].tolist()}"
        ok = upd["status"] == 0
        assert np.array_equal(u["out_size"][ok], upd["out_size"][ok])
        _same_records(what, "files", self.files.cpu().numpy().view(wc.FILE), done.files)
        failed = self.failed.cpu().numpy()
        assert failed[:done.failed.size * 4].view(np.uint32).tolist() == done.failed.tolist()
        assert (failed[done.failed.size * 4:] == CANARY).all()
        info = self.info.cpu().numpy().view(np.uint32).tolist()
        assert info == prep.info.tolist() + done.info.tolist(), f"{what}: info {info}"
        dev_chunks = self.chunks.cpu().numpy().reshape(b.n, CHUNK)
        for i in range(b.n):
            if ok[i]:
                size = int(upd["out_size"][i])
                assert np.array_equal(dev_chunks[i, :size], chunks[i, :size]), f"{what}: chunk {i}"
            else:
                assert (dev_chunks[i] == 0xCC).all(), f"{what}: chunk {i} of a refused update was written"


RANGES = [(0, 3 * CHUNK), (0, 1), (0, CHUNK + 17), (CHUNK, 2 * CHUNK), (0, 5 * CHUNK - 1), (2 * CHUNK, 2 * CHUNK + 300)]
MODES = pytest.mark.parametrize("mode", [0, 1], ids=["reference", "delta"])


@functools.lru_cache(maxsize=None)
def _bench(orc, ctype):
    return Bench(orc, ctype, RANGES)


@MODES
@TYPES
def test_write_file_and_check(hf, orc, dev, ctype, mode):
    """prepare(VERIFY) -> update_batch on fresh chunks -> complete(FROM_UPDATES, expected) queued on
    one stream with no synchronize between the calls: every file 0 with the oracle's CRC of its
    bytes; byte-identical with a twin that synchronizes after every call."""
    b = _bench(orc, ctype)
    model = b.model(orc, b.arena)
    assert (model[3].files["status"] == 0).all() and np.array_equal(model[3].files["value"], b.expected)
    assert model[3].files["length"].tolist() == [k for _a, k in b.file_bytes]
    st = torch.cuda.Stream(dev)
    box, twin = BenchBox(dev, b), BenchBox(dev, b)
    box.queue(hf, mode, st)
    st.synchronize()
    box.check(model, "queued")
    twin.queue(hf, mode, st, sync=True)
    st.synchronize()
    twin.check(model, "twin")
    a, t = box.images(), twin.images()
    assert a[2:5] == t[2:5]                                    # files, failed list, info: byte-identical
    assert _relocate_back(a, box) == _relocate_back(t, twin)   # (the two boxes' addresses differ)
    hf._lib.release_stream(st)


def _relocate_back(images, box):
    ios = np.frombuffer(images[0], dtype=wc.IO).copy()
    upd = np.frombuffer(images[1], dtype=wc.UPDATE).copy()
    ios["data"] -= np.uint64(box.arena.data_ptr())
    ios["buf_base"] -= np.uint64(box.arena.data_ptr())
    upd["payload"] -= np.uint64(box.arena.data_ptr())
    upd["chunk"] -= np.uint64(box.chunks.data_ptr())
    return ios.tobytes(), upd.tobytes(), images[5]


@MODES
def test_payload_flipped_between_prepare_and_update(hf, orc, dev, mode):
    """One payload byte flips after prepare hashed it: exactly that IO is 4080, its file is 4080 and
    names it, the failed list holds it alone, its chunk is untouched."""
    b = _bench(orc, wc.CRC32C)
    victim = 5
    flipped = b.arena.copy()
    at = int(b.ios["data"][victim]) - REL + 9
    flipped[at] ^= 0x40
    model = b.model(orc, flipped)
    done = model[3]
    f = int(np.searchsorted(b.off, victim, side="right")) - 1
    assert done.failed.tolist() == [victim] and done.ios["status_in"][victim] == 4080
    assert (done.files["status"] != 0).sum() == 1 and done.files["status"][f] == 4080 and done.files["failed_io"][f] == victim
    st = torch.cuda.Stream(dev)
    box = BenchBox(dev, b)

    def flip():
        with torch.cuda.stream(st):
            box.arena[at] ^= 0x40

    box.queue(hf, mode, st, between=flip)
    st.synchronize()
    box.check(model, "flipped")
    hf._lib.release_stream(st)


@MODES
def test_range_starting_mid_chunk_equals_the_model(hf, orc, dev, mode):
    """A file range that starts inside a fresh chunk: the chunk checksum the server answers with
    covers the zero gap in front of the payload, so the fold is not the CRC of the written bytes.
    That is the reference's behaviour and stays."""
    b = Bench(orc, wc.CRC32C, [(100, 2 * CHUNK + 50), (CHUNK - 1, CHUNK + 1)], seed=11)
    model = b.model(orc, b.arena, expected=False)
    done = model[3]
    assert (done.files["status"] == 0).all() and (done.files["value"] != b.expected).all()
    gap = bytes(100) + b.arena[:CHUNK - 100].tobytes()
    assert model[1]["out_checksum"][0] == orc.create(wc.CRC32C, gap)[1]
    st = torch.cuda.Stream(dev)
    box = BenchBox(dev, b)
    box.queue(hf, mode, st, expected=False)
    st.synchronize()
    box.check(model, "mid-chunk")
    hf._lib.release_stream(st)


# ---- contexts -------------------------------------------------------------------------------------
def test_poisoned_scratch(hf, orc, dev, opts):
    """Every scratch word is written before it is read: nothing changes when the calls' scratch
    starts from a pattern."""
    opts("poison", 0xA5A5A5A5)
    st = torch.cuda.Stream(dev)
    for verify in (True, False):
        _prep(hf, orc, dev, _counted(4097, wc.CRC32C), verify, "poisoned prepare", stream=st)
        _prep(hf, orc, dev, _case([GOOD, (0, REL, ARENA, 0, 4, 64), GOOD]), verify, "poisoned, poisoned batch", stream=st)
    for bound in (LANE, WAVE):
        _done(hf, orc, dev, _shapes(orc, 65)[0], "poisoned complete", stream=st, max_ios=bound)
    b = _bench(orc, wc.CRC32C)
    box = BenchBox(dev, b)
    box.queue(hf, 1, st)
    st.synchronize()
    box.check(b.model(orc, b.arena), "poisoned queue")
    hf._lib.release_stream(st)


def test_scratch_bytes_covers_both_calls(hf, orc, dev):
    L = hf._lib
    st = torch.cuda.Stream(dev)
    big = _counted(4097, wc.CRC32C)
    _prep(hf, orc, dev, big, True, "largest", stream=st)
    st0 = L.pair_scratch_stats(st)
    assert 0 < st0["call_bytes"] <= L.client_write_scratch_bytes(4097, 100)   # (the figure bounds any device's run tables)
    _done(hf, orc, dev, _shapes(orc, 65)[0], "complete", stream=st)
    _prep(hf, orc, dev, _counted(257, wc.CRC32), True, "smaller", stream=st)
    assert L.pair_scratch_stats(st) == st0
    L.release_stream(st)


def test_three_call_queue_in_one_graph(hf, orc, dev):
    """prepare -> update_batch -> complete captured once; replayed as captured, then with the
    payloads rewritten, then with records rewritten in place (an IO made to fail its range, another
    to poison the batch), and back: each replay is exact."""
    b = _bench(orc, wc.CRC32C)
    box = BenchBox(dev, b)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    with torch.cuda.graph(g, stream=side):
        box.queue(hf, 1, torch.cuda.current_stream())

    def variant(arena, ios):
        v = Bench.__new__(Bench)
        v.__dict__.update(b.__dict__)
        v.arena, v.ios = arena, ios
        v.expected = np.array([orc.create(v.ctype, arena[a:a + k].tobytes())[1] for a, k in b.file_bytes], dtype=np.uint32)
        return v

    arena2 = wc.arena_bytes(b.arena.size, 99)
    for k, v in enumerate((b, variant(arena2, b.ios), b)):
        fresh = BenchBox.__new__(BenchBox)
        fresh.__dict__.update(box.__dict__)
        fresh.b = v
        box.arena.copy_(torch.from_numpy(v.arena.copy()))
        box.ios.copy_(torch.from_numpy(_relocate(v.ios, box.arena.data_ptr()).view(np.uint8).reshape(-1).copy()))
        box.upd.copy_(torch.from_numpy(box.upd0.view(np.uint8).reshape(-1).copy()))
        box.exp.copy_(torch.from_numpy(v.expected.view(np.int32).copy()))
        box.chunks.fill_(0xCC)
        for t in (box.files, box.failed):
            t.fill_(CANARY)
        box.info.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        fresh.check(v.model(orc, v.arena), f"replay {k}")
    # records rewritten: IO 2 leaves its chunk (7002, alone); then IO 4 loses its buffer (poison)
    for k, edit in enumerate((lambda r: r["offset"].__setitem__(2, CHUNK), lambda r: r["buf_base"].__setitem__(4, 0))):
        ios = b.ios.copy()
        edit(ios)
        sent = _relocate(ios, box.arena.data_ptr())
        box.arena.copy_(torch.from_numpy(b.arena.copy()))
        box.ios.copy_(torch.from_numpy(sent.view(np.uint8).reshape(-1).copy()))
        box.upd.copy_(torch.from_numpy(box.upd0.view(np.uint8).reshape(-1).copy()))
        box.exp.copy_(torch.from_numpy(b.expected.view(np.int32).copy()))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        read = lambda a, n: b.arena[a - REL:a - REL + n].tobytes()  # noqa: E731
        prep = wc.prepare_model(ios, b.ctype, CHUNK, 0, True, orc, read)
        got = box.ios.cpu().numpy().view(wc.IO)
        assert got["status"].tolist() == prep.status.tolist() and np.array_equal(got["checksum"], prep.checksum)
        info = box.info.cpu().numpy().view(np.uint32).tolist()
        assert info[:8] == prep.info.tolist()
        if k == 0:
            assert prep.status.tolist().count(7002) == 1 and info[8] == 1
            files = box.files.cpu().numpy().view(wc.FILE)
            assert files["status"][0] == 7002 and files["failed_io"][0] == 2 and (files["status"][1:] == 0).all()
        else:
            assert prep.info[3] == 1 and info[8] == b.n and info[9] == 0
            u = box.upd.cpu().numpy().view(wc.UPDATE)
            assert (u["update_type"] == 0).all() and (u["status"] == 3).all()
    del g


def test_registered_host_memory_for_the_records(hf, orc, dev):
    """IO records, update records, offsets, expected values and every output in host memory
    registered with the library; payloads and chunks on the device."""
    b = _bench(orc, wc.CRC32)
    model = b.model(orc, b.arena)
    box = BenchBox(dev, b)
    nf = b.off.size - 1
    sizes = [b.n * 64, b.n * 56, (nf + 1) * 8, nf * 4, nf * 24 + 2 * GUARD, b.n * 4 + 2 * GUARD, 64 + 2 * GUARD]
    bufs = [hm.Registered(max(s, 8)) for s in sizes]
    try:
        ios, upd, off, exp, files, failed, info = bufs
        ios.write(box.sent.view(np.uint8).reshape(-1))
        upd.write(box.upd0.view(np.uint8).reshape(-1))
        off.write(b.off.view(np.uint8))
        exp.write(b.expected.view(np.uint8))
        for x in (files, failed, info):
            x.host[:] = CANARY
        st = torch.cuda.current_stream()
        hf.client_write_prepare(b.ctype, ios.dev, b.n, info.dev + GUARD, CHUNK, verify=True, updates=upd.dev, stream=st)
        hf._lib.update_batch(b.ctype, upd.dev, b.n, CHUNK, mode=1, stream=st)
        hf.client_write_complete(ios.dev, b.n, info.dev + GUARD + 32, file_off=off.dev, n_files=nf, max_ios_per_file=5,
                                 updates=upd.dev, expected=exp.dev, files=files.dev + GUARD, failed=failed.dev + GUARD,
                                 failed_cap=b.n, stream=st)
        torch.cuda.synchronize()
        prep, want_upd, _chunks, done = model
        got = ios.read().view(wc.IO)
        for f in ("status", "checksum", "checksum_type", "send_inline", "status_in", "result_len", "result_checksum",
                  "result_checksum_type"):
            assert np.array_equal(got[f], done.ios[f]), f
        u = upd.read().view(wc.UPDATE)
        assert np.array_equal(u["out_checksum"], want_upd["out_checksum"]) and (u["status"] == 0).all()
        for x, want in ((files, done.files.tobytes()), (failed, b""), (info, prep.info.tobytes() + done.info.tobytes())):
            raw = x.read()
            assert raw[GUARD:GUARD + len(want)].tobytes() == want
            assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + len(want):] == CANARY).all()
    finally:
        torch.cuda.synchronize()
        for x in bufs:
            x.close()
