"""hf3fs_crc_server_read_prepare / hf3fs_crc_server_read_complete on the GPU.

Every expectation comes from tests/server_read_cases.py: batchRead, setReadJobResult, setResult,
copyToRespBuffer and addBufferToBatch restated in Python over the CPU oracle's CRC.  After every
round the whole job and request arrays (every field: inputs unchanged, outputs the model's), the
eight info words of either call, the inline arena, the RDMA list, the guard bytes around every
output array and the data arena (unchanged) are compared, exactly.

Shapes: reads of at most 4097 bytes at offsets below 8192 with max_len 8192 out of 256 shared slots;
lengths {0, 1, 15, 16, 17, 100, 1000, 4095, 4096, 4097}; job counts 1, 255, 256, 257, 513 (one lane
per job, 256 per workgroup and per share of the scan) and 70,001 (more than one share per workgroup
row: shares of 256-job tiles, a partial last one); requests of 0, 1 and 300 jobs, the latter
straddling tiles and shares; 2^20 + 300 jobs that hash and copy nothing (the grid-stride loops: at
most 4096 x 256 lanes)."""
import numpy as np
import pytest

import server_read_cases as sc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
GUARD = 64
CANARY = 0x5A
MAX_LEN = 8192
SLOT = 3 * 4096 + 64
N_SLOTS = 256
SMALL, BIG = 4096, 12288   # reads are 0, 4096 or 8192 bytes long: the longest take a big buffer and leave room
LENGTHS = (0, 1, 15, 16, 17, 100, 1000, 4095, 4096, 4097)
CTYPES = pytest.mark.parametrize("ctype", [sc.CRC32C, sc.CRC32], ids=["crc32c", "crc32"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class World:
    """One device arena of read buffers and its host mirror; never written by the library."""

    def __init__(self, dev):
        rng = np.random.default_rng(0x5E2D)
        self.size = N_SLOTS * SLOT
        self.host = rng.integers(0, 256, self.size, dtype=np.uint8)
        self.dev = torch.from_numpy(self.host).to(dev)
        self.base = self.dev.data_ptr()
        assert self.base % 16 == 0
        self.bytes = self.host.tobytes()
        torch.cuda.synchronize()

    def slot(self, k, residue=0):
        return self.base + k * SLOT + residue

    def read(self, addr, n):
        o = addr - self.base
        assert 0 <= o and o + n <= self.size, f"the model read outside the arena: {addr:#x} + {n}"
        return self.bytes[o:o + n]

    def unchanged(self, what):
        assert np.array_equal(self.dev.cpu().numpy(), self.host), f"{what}: the data arena changed"


@pytest.fixture(scope="module")
def world(dev):
    return World(dev)


def _guarded(dev, nbytes):
    t = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
    return t, t[GUARD:GUARD + nbytes]


class Run:
    """Device images of one batch: records, offsets, d_info of either call, the inline arena and
    the RDMA list, each between guards."""

    def __init__(self, dev, jobs, reqs, ro, inline_cap, wr_cap):
        self.n, self.n_reqs, self.inline_cap, self.wr_cap = jobs.size, reqs.size, inline_cap, wr_cap
        self.raw = {}
        self.t = {}
        for name, nbytes in (("jobs", max(jobs.nbytes, 8)), ("reqs", max(reqs.nbytes, 8)), ("ro", ro.nbytes),
                             ("pinfo", 4 * sc.INFO_WORDS), ("cinfo", 4 * sc.INFO_WORDS),
                             ("inline", max(inline_cap, 1)), ("wr", max(wr_cap, 1) * sc.WR.itemsize)):
            self.raw[name], self.t[name] = _guarded(dev, nbytes)
        self.put(jobs, reqs, ro)

    def put(self, jobs, reqs, ro):
        for name, arr in (("jobs", jobs), ("reqs", reqs), ("ro", ro)):
            if arr.size:
                self.t[name][:arr.nbytes].copy_(torch.from_numpy(arr.view(np.uint8).copy()))
        for name in ("pinfo", "cinfo", "inline", "wr"):
            self.t[name].fill_(CANARY)
        torch.cuda.synchronize()

    def prepare(self, hf, stream=None):
        hf.server_read_prepare(self.t["jobs"] if self.n else None, self.n, self.t["reqs"] if self.n_reqs else None,
                               self.t["ro"] if self.n_reqs else None, self.n_reqs, self.t["pinfo"], SMALL, BIG,
                               stream=stream or torch.cuda.current_stream())

    def complete(self, hf, ctype, stream=None):
        hf.server_read_complete(ctype, self.t["jobs"] if self.n else None, self.n,
                                self.t["reqs"] if self.n_reqs else None, self.t["ro"] if self.n_reqs else None,
                                self.n_reqs, self.t["cinfo"], MAX_LEN,
                                inline=self.t["inline"] if self.inline_cap else None, inline_cap=self.inline_cap,
                                wr=self.t["wr"] if self.wr_cap else None, wr_cap=self.wr_cap,
                                stream=stream or torch.cuda.current_stream())

    def host(self, name, dtype=np.uint8, count=None):
        a = self.t[name].cpu().numpy()
        return a.view(dtype) if count is None else a[:count * np.dtype(dtype).itemsize].view(dtype)

    def guards(self, what):
        for name, raw in self.raw.items():
            g = raw.cpu().numpy()
            assert (g[:GUARD] == CANARY).all() and (g[-GUARD:] == CANARY).all(), f"{what}: bytes around {name} written"


def _same_records(got, want, what):
    if got.tobytes() == want.tobytes():
        return
    for name in want.dtype.names:
        bad = np.flatnonzero((got[name] != want[name]).reshape(want.size, -1).any(axis=1))
        assert bad.size == 0, f"{what}: field {name} differs at {bad[:8].tolist()}: got {got[name][bad[:4]]}, " \
                              f"want {want[name][bad[:4]]}"


def check(run, world, orc, ctype, jobs, reqs, ro, what, prepared=True):
    """Compares everything after prepare + complete with the model (jobs / reqs: the records as
    uploaded; they are prepared and completed here, in place)."""
    pinfo = sc.prepare(jobs, reqs, ro, SMALL, BIG) if prepared else None
    cinfo, inline, wr = sc.complete(jobs, reqs, ro, ctype, MAX_LEN, world.read, orc, run.inline_cap)
    _same_records(run.host("jobs", sc.JOB, run.n), jobs, what + ", jobs")
    _same_records(run.host("reqs", sc.REQ, run.n_reqs), reqs, what + ", requests")
    if prepared:
        assert run.host("pinfo", np.uint32).tolist() == pinfo, f"{what}: prepare's d_info"
    assert run.host("cinfo", np.uint32).tolist() == cinfo, f"{what}: complete's d_info"
    arena = run.host("inline")
    if inline is None:
        assert (arena == CANARY).all(), f"{what}: the inline arena was written after an overflow"
    else:
        assert arena[:len(inline)].tobytes() == inline, f"{what}: inline bytes"
        assert (arena[len(inline):] == CANARY).all(), f"{what}: the inline arena written past the bytes needed"
    listed = min(wr.size, run.wr_cap)
    got = run.host("wr")
    _same_records(got[:listed * sc.WR.itemsize].view(sc.WR), wr[:listed], what + ", RDMA list")
    assert (got[listed * sc.WR.itemsize:] == CANARY).all(), f"{what}: d_wr written past the list or wr_cap"
    assert np.array_equal(run.host("ro", np.uint64), ro), f"{what}: d_req_off changed"
    run.guards(what)
    world.unchanged(what)
    return pinfo, cinfo, inline, wr


def round_trip(hf, orc, dev, world, ctype, jobs, reqs, ro, what, inline_cap=None, wr_cap=None, stream=None):
    """prepare -> complete queued on one stream, one synchronize, then everything compared."""
    if inline_cap is None:
        inline_cap = int(jobs["length"].sum()) + 16
    if wr_cap is None:
        wr_cap = jobs.size + 1
    run = Run(dev, jobs, reqs, ro, inline_cap, wr_cap)
    run.prepare(hf, stream)
    run.complete(hf, ctype, stream)
    torch.cuda.synchronize()
    return run, check(run, world, orc, ctype, jobs, reqs, ro, what)


# ---- case builders ----------------------------------------------------------------------------------
def ladder(world, orc, ctype, counts, seed, rungs=True):
    """Requests of these job counts with every rung at its own rate (rungs=False: healthy reads)."""
    rng = np.random.default_rng(seed)
    n = int(sum(counts))
    jobs, reqs, ro = sc.new_jobs(n), sc.new_reqs(len(counts)), sc.offsets(counts)
    other = sc.CRC32 if ctype == sc.CRC32C else sc.CRC32C
    pick = lambda p: rng.random(n) < (p if rungs else 0.0)
    offset = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 8192, n)).astype(np.uint32)
    length = rng.choice(LENGTHS, n).astype(np.uint32)
    head = offset % 4096
    jobs["offset"], jobs["length"] = offset, length
    jobs["inner_offset"] = rng.integers(0, 1 << 40, n) * 4096
    jobs["remote_addr"], jobs["rkey"] = rng.integers(1, 1 << 47, n), rng.integers(0, 1 << 32, n)
    jobs["localbuf"] = world.base + rng.integers(0, N_SLOTS, n) * SLOT + np.where(rng.random(n) < 0.5, 0, rng.integers(0, 16, n))
    jobs["localbuf"][pick(0.02)] = 0
    end = offset.astype(np.int64) + length
    shape = rng.integers(0, 4, n)
    jobs["chunk_len"] = np.select([shape == 0, shape == 1, shape == 2], [end, end + rng.integers(1, 5000, n),
                                                                         np.maximum(0, end - rng.integers(1, 600, n))],
                                  np.maximum(0, offset.astype(np.int64) - rng.integers(0, 3, n)))
    full_res = head.astype(np.int64) + length + ((4096 - end % 4096) % 4096)
    kind = rng.integers(0, 10, n) if rungs else np.full(n, 9)
    jobs["res"] = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                            [-rng.integers(1, 100, n), head // 2, head + length // 2, full_res + 4096], full_res)
    jobs["engine"] = pick(0.3)
    jobs["chunk_checksum_type"] = np.select([pick(0.15), pick(0.04)], [sc.NONE, other], ctype)
    jobs["meta_status"][pick(0.03)] = sc.CHUNK_METADATA_NOT_FOUND
    jobs["meta_status"][pick(0.01)] = sc.CHUNK_METADATA_GET_ERROR
    jobs["commit_ver"] = np.where(pick(0.06), 7, 1)
    jobs["update_ver_now"] = np.where(pick(0.05), 2, 1)
    jobs["meta_status_now"][pick(0.03)] = sc.CHUNK_METADATA_NOT_FOUND
    jobs["has_rkey"] = ~pick(0.03)
    jobs["rdmabuf_size"] = np.where(pick(0.3), length, 1 << 20)
    # the stored checksum of a chunk the read covers whole: right, or with a bit flipped
    clip = np.minimum(np.minimum(np.maximum(0, jobs["res"] - head), length), np.maximum(0, jobs["chunk_len"].astype(np.int64) - offset))
    for i in np.flatnonzero((offset == 0) & (clip == jobs["chunk_len"]) & (jobs["res"] >= 0) & (jobs["localbuf"] != 0)):
        j = jobs[i]
        stored = sc.CRC32C if j["engine"] else int(j["chunk_checksum_type"])
        value = 0 if stored == sc.NONE else orc.create(stored, world.read(int(j["localbuf"]), int(clip[i])))[1]
        if rungs and rng.random() < 0.2:
            value ^= 1 << int(rng.integers(0, 32))
        j["chunk_checksum"] = value ^ 0xFFFFFFFF if j["engine"] else value
    reqs["checksum_type"] = np.select([rng.random(reqs.size) < 0.25, rng.random(reqs.size) < (0.04 if rungs else 0)],
                                      [sc.NONE, other], ctype)
    reqs["xmit"] = rng.integers(0, 3, reqs.size)
    reqs["read_uncommitted"] = rng.random(reqs.size) < 0.3
    reqs["recalculate"] = rng.random(reqs.size) < 0.5
    reqs["max_msg_sz"] = np.where(rng.random(reqs.size) < (0.2 if rungs else 0), 1000, 1 << 30)
    if rungs:   # one request in ten is ended by its first loop
        for r in np.flatnonzero((rng.random(reqs.size) < 0.1) & (np.asarray(counts) > 0)):
            i = int(ro[r]) + int(rng.integers(0, counts[r]))
            which = rng.integers(0, 3)
            if which == 0:
                jobs["target_status"][i] = sc.CHAIN_VERSION_MISMATCH
            elif which == 1:
                jobs["up_to_date"][i] = 0
            else:
                jobs["rdmabuf_size"][i], jobs["length"][i] = 5, 4097
    return jobs, reqs, ro


def split(n, rng, sizes=(0, 1, 1, 2, 7, 31)):
    counts = []
    while sum(counts) < n:
        counts.append(min(int(rng.choice(sizes)), n - sum(counts)))
    return counts + [0]


# ---- the ladder -------------------------------------------------------------------------------------
@CTYPES
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_every_rung_against_the_model(hf, orc, dev, world, ctype, n):
    counts = split(n, np.random.default_rng(n))
    jobs, reqs, ro = ladder(world, orc, ctype, counts, seed=n * 3 + ctype)
    round_trip(hf, orc, dev, world, ctype, jobs, reqs, ro, f"{n} jobs")


def test_the_ladder_reaches_every_rung(orc, dev, world):
    """The builder's cases, seen through the model: every status and every rung's outcome occurs."""
    jobs, reqs, ro = ladder(world, orc, sc.CRC32C, split(513, np.random.default_rng(513)), seed=513 * 3 + 1)
    more = ladder(world, orc, sc.CRC32C, split(257, np.random.default_rng(257)), seed=257 * 3 + 1)
    seen_prep, seen_done, kinds, reuse = set(), set(), set(), 0
    for j, q, o in ((jobs, reqs, ro), more):
        sc.prepare(j, q, o, SMALL, BIG)
        sc.complete(j, q, o, sc.CRC32C, MAX_LEN, world.read, orc, 1 << 30)
        seen_prep |= set(j["status"].tolist())
        seen_done |= set(zip(j["result_status"].tolist(), j["engine"].tolist()))
        kinds |= set(j["buf_kind"].tolist())
        reuse += int(((j["buf_kind"] == sc.BUF_BIG) & (j["buf_off"] > 0)).sum())
    assert {0, 3, 4001, 4002, 4004, 4032, 4081} <= seen_prep
    for code in (0, 3, 4010, 4080):
        assert (code, 0) in seen_done and (code, 1) in seen_done, code
    assert (4004, 0) in seen_done and (4001, 0) in seen_done
    assert kinds == {sc.BUF_NONE, sc.BUF_SMALL, sc.BUF_BIG} and reuse > 0


def test_requests_of_300_jobs_and_of_none(hf, orc, dev, world):
    counts = [0, 300, 0, 0, 300, 1, 300, 300, 0]
    jobs, reqs, ro = ladder(world, orc, sc.CRC32C, counts, seed=300, rungs=False)
    reqs["xmit"] = [0, 1, 1, 0, 0, 1, 1, 0, 1]
    jobs["res"][5], jobs["res"][700] = -1, -1
    run, (pinfo, cinfo, inline, wr) = round_trip(hf, orc, dev, world, sc.CRC32C, jobs, reqs, ro, "300-job requests")
    assert pinfo[0] == 9 and wr.size > 500 and len(inline) > 100000


def test_70001_jobs(hf, orc, dev, world):
    rng = np.random.default_rng(70001)
    counts = split(70001 - 600, rng, sizes=(0, 1, 3, 17, 64)) + [300, 300]
    jobs, reqs, ro = ladder(world, orc, sc.CRC32C, counts, seed=70001)
    short = jobs["length"] > 100     # keep the model's hashing short: most jobs read 0..100 bytes
    jobs["length"][short & (rng.random(jobs.size) < 0.9)] = 64
    round_trip(hf, orc, dev, world, sc.CRC32C, jobs, reqs, ro, "70,001 jobs")


def test_grid_stride_loops_over_2_20_plus_300_jobs(hf, dev, world):
    """2^20 + 300 jobs in requests of 32 (the last of 12) that hash and copy nothing: no checksum is
    asked for and the RDMA list is counted (shares of two tiles each) but not stored.  Expectations in
    closed form."""
    n = (1 << 20) + 300
    counts = [32] * (n // 32) + [n % 32]
    jobs, reqs, ro = sc.new_jobs(n), sc.new_reqs(len(counts), checksum_type=sc.NONE, xmit=sc.XMIT_RDMA), sc.offsets(counts)
    k = np.arange(n)
    jobs["offset"], jobs["length"], jobs["chunk_len"] = 4096 * (k % 5) + 7, 4000, 1 << 20
    jobs["inner_offset"] = k * 4096
    jobs["localbuf"] = world.base
    jobs["res"] = np.where(k % 3 == 0, 2000, 8192)
    jobs["meta_status"][k % 1001 == 0] = sc.CHUNK_METADATA_NOT_FOUND
    run = Run(dev, jobs, reqs, ro, 0, 0)
    run.prepare(hf)
    run.complete(hf, sc.CRC32C)
    torch.cuda.synchronize()
    failed = k % 1001 == 0
    jobs["head_len"], jobs["tail_len"], jobs["read_len"] = 7, 4096 - 4007, 4096
    jobs["buf_ordinal"], jobs["buf_off"], jobs["buf_kind"] = k % 32, 0, sc.BUF_SMALL    # SMALL holds one read
    jobs["status"] = np.where(failed, sc.CHUNK_METADATA_NOT_FOUND, 0)
    jobs["read_offset"] = np.where(failed, 0, k * 4096 + 4096 * (k % 5))
    jobs["result_status"] = jobs["status"]
    jobs["result_len"] = np.where(failed, 0, np.where(k % 3 == 0, 1993, 4000))
    jobs["checksum"], jobs["checksum_type"], jobs["inline_off"] = 0, sc.NONE, 0
    cnt = np.asarray(counts)
    reqs["status"], reqs["failed_job"] = 0, sc.NO_JOB
    reqs["total_len"], reqs["total_head"], reqs["total_tail"] = 4000 * cnt, 7 * cnt, 89 * cnt
    reqs["n_small"], reqs["n_big"] = cnt, 0
    reqs["n_ok"] = cnt - np.add.reduceat(failed.astype(np.int64), ro[:-1].astype(np.int64))
    starts = ro[:-1].astype(np.int64)
    reqs["wr_count"] = reqs["n_ok"]
    reqs["wr_first"] = np.concatenate([[0], np.cumsum(reqs["n_ok"])[:-1]])
    reqs["wr_bytes"] = np.add.reduceat(jobs["result_len"].astype(np.int64), starts)
    for name in ("inline_off", "inline_bytes", "wr_fails"):
        reqs[name] = 0
    _same_records(run.host("jobs", sc.JOB, n), jobs, "2^20 + 300 jobs")
    _same_records(run.host("reqs", sc.REQ, reqs.size), reqs, "2^20 + 300 jobs, requests")
    nf = int(failed.sum())
    assert run.host("pinfo", np.uint32).tolist() == [len(counts), 0, n - nf, nf, n, 0, 0, 0]
    assert run.host("cinfo", np.uint32).tolist() == [n - nf, nf, 0, 0, 0, n - nf, 0, 0]
    run.guards("2^20 + 300 jobs")


def test_prepare_alone_with_large_reads_and_2019(hf, dev):
    """The carve at the reference's sizes through the binding's SMALL / BIG: reads up to three
    blocks, big buffers reused, requests above BIG refused; and the wrapping offset + length."""
    rng = np.random.default_rng(2019)
    counts = split(513, rng)
    n = sum(counts)
    jobs, reqs, ro = sc.new_jobs(n), sc.new_reqs(len(counts)), sc.offsets(counts)
    jobs["offset"] = rng.integers(0, 1 << 32, n)
    jobs["length"] = rng.choice([0, 1, 4096, 4097, 8192, 9000, 12288], n, p=[.1, .2, .3, .1, .2, .09, .01])
    jobs["offset"][::7] = 0xFFFFFFFF - rng.integers(0, 4096, jobs["offset"][::7].size)
    jobs["engine"] = rng.random(n) < 0.3
    jobs["commit_ver"] = np.where(rng.random(n) < 0.1, 5, 1)
    run = Run(dev, jobs, reqs, ro, 0, 0)
    run.prepare(hf)
    torch.cuda.synchronize()
    pinfo = sc.prepare(jobs, reqs, ro, SMALL, BIG)
    _same_records(run.host("jobs", sc.JOB, n), jobs, "prepare alone")
    _same_records(run.host("reqs", sc.REQ, reqs.size), reqs, "prepare alone, requests")
    assert run.host("pinfo", np.uint32).tolist() == pinfo
    assert sc.RDMA_NO_BUF in reqs["status"] and 0 in reqs["status"] and pinfo[5] > 0
    run.guards("prepare alone")


# ---- res ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [0, 1], ids=["replica", "engine"])
def test_res_values(hf, orc, dev, world, engine):
    """res negative, below head, above length, and reaching past chunk_len."""
    jobs, reqs, ro = sc.new_jobs(5), sc.new_reqs(1), sc.offsets([5])
    jobs["offset"], jobs["length"], jobs["chunk_len"], jobs["engine"] = 4096 + 100, 500, 8192, engine
    jobs["chunk_checksum_type"] = sc.CRC32C
    jobs["localbuf"] = [world.slot(k, k) for k in range(5)]
    jobs["res"] = [-9, 99, 100 + 500 + 3496 + 4096, 4096, 4096]
    jobs["chunk_len"][4] = 4096 + 100 + 200
    run, _ = round_trip(hf, orc, dev, world, sc.CRC32C, jobs, reqs, ro, "res values")
    assert jobs["result_status"].tolist() == [sc.CHUNK_READ_FAILED, 0, 0, 0, 0]
    assert jobs["result_len"].tolist() == [0, 0, 500, 500, 200]


# ---- the inline arena -----------------------------------------------------------------------------------
def inline_batch(world, lengths, src_res, xmit=sc.XMIT_INLINE, counts=None):
    n = len(lengths)
    counts = counts or [n]
    jobs, reqs, ro = sc.new_jobs(n), sc.new_reqs(len(counts), checksum_type=sc.NONE, xmit=xmit), sc.offsets(counts)
    jobs["length"], jobs["chunk_len"] = lengths, 1 << 20
    jobs["offset"] = 4096 + np.asarray(src_res) % 16
    jobs["localbuf"] = [world.slot(k % N_SLOTS) for k in range(n)]
    jobs["res"] = 12288
    return jobs, reqs, ro


def test_inline_every_source_and_destination_residue(hf, orc, dev, world):
    """A filler job of 0..15 bytes puts the next job at every destination residue; that job's
    source has every residue; its length runs through 0..70."""
    lengths, src, cur, k = [], [], 0, 0
    for sres in range(16):
        for dres in range(16):
            fill = (dres - cur) % 16
            lengths += [fill, k % 71]
            src += [(sres + 5) % 16, sres]
            cur += fill + k % 71
            k += 1
    jobs, reqs, ro = inline_batch(world, lengths, src)
    run, (_, cinfo, inline, _) = round_trip(hf, orc, dev, world, sc.CRC32C, jobs, reqs, ro, "inline residues",
                                            inline_cap=cur)
    assert len(inline) == cur == cinfo[2] and cinfo[4] == 0
    pairs = {(int(j["offset"]) % 16, int(j["inline_off"]) % 16) for j in jobs[1::2]}
    assert len(pairs) == 256 and set(jobs["length"][1::2].tolist()) == set(range(71))


@pytest.mark.parametrize("length", [4095, 4096, 4097])
def test_inline_block_lengths(hf, orc, dev, world, length):
    lengths = [length, 3, length, 13, length, 1, length]
    jobs, reqs, ro = inline_batch(world, lengths, [0, 1, 7, 2, 15, 3, 8], counts=[3, 0, 4])
    round_trip(hf, orc, dev, world, sc.CRC32C, jobs, reqs, ro, f"inline {length}", inline_cap=sum(lengths))


def test_inline_overflow_leaves_the_arena_untouched(hf, orc, dev, world):
    lengths = [70, 4097, 0, 16]
    jobs, reqs, ro = inline_batch(world, lengths, [1, 2, 3, 4])
    run, (_, cinfo, inline, _) = round_trip(hf, orc, dev, world, sc.CRC32C, jobs, reqs, ro, "inline overflow",
                                            inline_cap=sum(lengths) - 1)
    assert inline is None and cinfo[2:5] == [sum(lengths), 0, 1]
    assert jobs["result_status"].tolist() == [0] * 4 and jobs["inline_off"].tolist() == [0, 70, 4167, 4167]


def test_all_three_xmit_kinds_in_one_call(hf, orc, dev, world):
    lengths = [100, 17, 4096, 1, 1000, 15, 16, 4097, 0]
    jobs, reqs, ro = inline_batch(world, lengths, range(9), counts=[2, 2, 1, 2, 2])
    reqs["xmit"] = [sc.XMIT_INLINE, sc.XMIT_RDMA, sc.XMIT_NONE, sc.XMIT_INLINE, sc.XMIT_RDMA]
    reqs["checksum_type"] = sc.CRC32C
    run, (_, cinfo, inline, wr) = round_trip(hf, orc, dev, world, sc.CRC32C, jobs, reqs, ro, "three xmit kinds")
    assert len(inline) == 100 + 17 + 15 + 16 and wr["job"].tolist() == [2, 3, 7, 8]
    assert reqs["inline_off"].tolist() == [0, 117, 117, 117, 148]


# ---- the RDMA list ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wr_cap", [0, 1, 100, 256, 400])
def test_rdma_list_under_wr_cap(hf, orc, dev, world, wr_cap):
    jobs, reqs, ro = ladder(world, orc, sc.CRC32C, [300, 0, 213], seed=9, rungs=True)
    reqs["xmit"] = sc.XMIT_RDMA
    jobs["target_status"], jobs["up_to_date"] = 0, 1
    jobs["rdmabuf_size"] = np.maximum(jobs["rdmabuf_size"], jobs["length"])
    run, (_, cinfo, _, wr) = round_trip(hf, orc, dev, world, sc.CRC32C, jobs, reqs, ro, f"wr_cap {wr_cap}", wr_cap=wr_cap)
    assert cinfo[5] == wr.size > 256 and cinfo[6] > 0


# ---- contexts -------------------------------------------------------------------------------------------
def test_prepare_checked_before_complete(hf, orc, dev, world):
    """A synchronize between the calls: prepare's outputs alone, complete's fields still as uploaded."""
    jobs, reqs, ro = ladder(world, orc, sc.CRC32C, split(257, np.random.default_rng(4)), seed=4)
    run = Run(dev, jobs, reqs, ro, 1 << 20, 300)
    run.prepare(hf)
    torch.cuda.synchronize()
    want_j, want_r = jobs.copy(), reqs.copy()
    pinfo = sc.prepare(want_j, want_r, ro, SMALL, BIG)
    _same_records(run.host("jobs", sc.JOB, run.n), want_j, "prepare")
    _same_records(run.host("reqs", sc.REQ, run.n_reqs), want_r, "prepare, requests")
    assert run.host("pinfo", np.uint32).tolist() == pinfo
    assert (run.host("cinfo") == CANARY).all()
    run.complete(hf, sc.CRC32C)
    torch.cuda.synchronize()
    check(run, world, orc, sc.CRC32C, jobs, reqs, ro, "complete after a checked prepare")


def test_poisoned_scratch(hf, orc, dev, world, opts):
    """Every scratch word is written before it is read: the results do not change when the call's
    scratch starts from a pattern."""
    opts("poison", 0xA5A5A5A5)
    st = torch.cuda.Stream(dev)
    for n in (257, 1000):
        jobs, reqs, ro = ladder(world, orc, sc.CRC32C, split(n, np.random.default_rng(n)), seed=n)
        with torch.cuda.stream(st):
            round_trip(hf, orc, dev, world, sc.CRC32C, jobs, reqs, ro, f"poisoned, {n} jobs", stream=st)
    hf._lib.release_stream(st)


def test_both_calls_in_one_graph_replay_on_rewritten_records(hf, orc, dev, world):
    """prepare and complete captured in one graph; replayed on the records as captured, then with
    res and the version fields rewritten, and back."""
    first = ladder(world, orc, sc.CRC32C, split(513, np.random.default_rng(11)), seed=11)
    second = tuple(a.copy() for a in first)
    rng = np.random.default_rng(12)
    j2 = second[0]
    j2["res"] = np.where(rng.random(j2.size) < 0.5, j2["res"] // 2, j2["res"])
    j2["update_ver_now"] = np.where(rng.random(j2.size) < 0.3, 3, j2["update_ver_now"])
    j2["commit_ver"] = np.where(rng.random(j2.size) < 0.3, 9, j2["commit_ver"])
    second[1]["xmit"] = (second[1]["xmit"] + 1) % 3
    run = Run(dev, first[0], first[1], first[2], 1 << 21, 600)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        run.prepare(hf, torch.cuda.current_stream())
        run.complete(hf, sc.CRC32C, torch.cuda.current_stream())
    for k, (jobs, reqs, ro) in enumerate((first, second, first)):
        jobs, reqs = jobs.copy(), reqs.copy()
        run.put(jobs, reqs, ro)
        g.replay()
        torch.cuda.synchronize()
        check(run, world, orc, sc.CRC32C, jobs, reqs, ro, f"replay {k}")


def test_written_by_update_batch_read_back_verified_by_the_client(hf, orc, dev):
    """One queue, one synchronize: update_batch writes 64 new chunks, prepare and complete read them
    back whole (with the recalculation) into an inline response, client_read_batch verifies the
    response's blocks against the checksums complete answered."""
    n, size = 64, 4096
    rng = np.random.default_rng(64)
    payload = torch.from_numpy(rng.integers(0, 256, n * size, dtype=np.uint8)).to(dev)
    chunks = torch.zeros(n * size, dtype=torch.uint8, device=dev)
    ios = np.zeros(n, dtype=hf.update_io_dtype())
    ios["chunk"], ios["payload"] = chunks.data_ptr() + size * np.arange(n), payload.data_ptr() + size * np.arange(n)
    ios["length"], ios["chunk_size"], ios["update_type"] = size, 0, hf.UPDATE_WRITE
    ios["chunk_checksum_type"] = ios["write_checksum_type"] = hf.CRC32C
    host_payload = payload.cpu().numpy()
    ios["write_checksum"] = [orc.create(sc.CRC32C, host_payload[k * size:(k + 1) * size].tobytes())[1] for k in range(n)]
    d_ios = torch.from_numpy(ios.view(np.uint8).copy()).to(dev)
    jobs, reqs, ro = sc.new_jobs(n), sc.new_reqs(2, xmit=sc.XMIT_INLINE), sc.offsets([40, 24])
    reqs["recalculate"] = 1
    jobs["length"], jobs["chunk_len"], jobs["res"] = size, size, size
    jobs["chunk_checksum_type"] = sc.CRC32C
    jobs["localbuf"] = ios["chunk"]
    run = Run(dev, jobs, reqs, ro, n * size, 0)
    cio = np.zeros(n, dtype=hf.client_read_io_dtype())
    cio["data"], cio["length"] = run.t["inline"].data_ptr() + size * np.arange(n), size
    cio["status_in"] = -1    # overwritten on the device below
    d_cio = torch.from_numpy(cio.view(np.uint8).copy()).to(dev)
    cinfo = torch.full((hf.CLIENT_READ_INFO_WORDS,), -1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    hf._lib.update_batch(hf.CRC32C, d_ios, n, size, hf.MODE_REFERENCE, stream=st)
    # the host's part between the calls, here on the device so that nothing waits: the chunk
    # metadata from the update records into the job records, the answers into the client's records
    jf, uf, cf = sc.JOB.fields, ios.dtype.fields, cio.dtype.fields
    jv = run.t["jobs"][:jobs.nbytes].view(torch.int32).view(n, -1)
    uv = d_ios.view(torch.int32).view(n, -1)
    jv[:, jf["chunk_checksum"][1] // 4] = uv[:, uf["out_checksum"][1] // 4]
    run.prepare(hf, st)
    run.complete(hf, sc.CRC32C, st)
    cv = d_cio.view(torch.int32).view(n, -1)
    cv[:, cf["read_len"][1] // 4] = jv[:, jf["result_len"][1] // 4]
    cv[:, cf["status_in"][1] // 4] = jv[:, jf["result_status"][1] // 4]
    cv[:, cf["checksum"][1] // 4] = jv[:, jf["checksum"][1] // 4]
    d_cio.view(n, -1)[:, cf["checksum_type"][1]] = run.t["jobs"][:jobs.nbytes].view(n, -1)[:, jf["checksum_type"][1]]
    hf.client_read_batch(hf.CRC32C, d_cio, n, cinfo, max_len=size, verify=True, stream=st)
    torch.cuda.synchronize()
    got = run.host("jobs", sc.JOB, n)
    updated = d_ios.cpu().numpy().view(ios.dtype)
    assert updated["status"].tolist() == [0] * n and updated["out_checksum_type"].tolist() == [hf.CRC32C] * n
    assert got["result_status"].tolist() == [0] * n and got["result_len"].tolist() == [size] * n
    assert run.host("inline").tobytes() == host_payload.tobytes()
    for k in (0, 39, 40, 63):
        assert got["checksum"][k] == orc.create(sc.CRC32C, host_payload[k * size:(k + 1) * size].tobytes())[1]
    assert got["checksum_type"].tolist() == [sc.CRC32C] * n
    done = d_cio.cpu().numpy().view(cio.dtype)
    assert done["status"].tolist() == [0] * n and np.array_equal(done["computed"], got["checksum"])
    assert cinfo.cpu().numpy().view(np.uint32).tolist()[:2] == [0, 0]
    run.guards("end to end")
