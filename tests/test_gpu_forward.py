"""hf3fs_crc_forward_prepare / hf3fs_crc_forward_complete on the GPU.

Every expectation comes from tests/forward_cases.py: handleUpdate, forward and doForward restated in
Python over the CPU oracle's CRC.  After every call the whole record array (every field: inputs
unchanged, outputs the model's, a sent job's response fields untouched by prepare), the eight info
words, the commit list, the guard bytes around every output array and the data arena (unchanged)
are compared.

Shapes: chunks of 4 KiB with max_len 4096; chunk and payload lengths {0, 1, 15, 16, 17, 4095, 4096}
at address residues 0, 1 and 15 mod 16, intact and with one bit flipped; both CRC types; n in
{1, 63, 64, 65, 1000} (one lane per job, 256 per workgroup: a partial wave, a full one, one lane
more, and four workgroups of which the last is partial; the commit list's shares are 256 jobs).
"""
import functools

import numpy as np
import pytest

import forward_cases as fc
import update_footprint as ufp

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
GUARD = 64          # bytes in front of and behind every output array that no call may write
CANARY = 0x5A
MAX_LEN = 4096
LENGTHS = (0, 1, 15, 16, 17, 4095, 4096)
RESIDUES = (0, 1, 15)
SLOT = 4096 + 64    # arena bytes per buffer
SIZES = (1, 63, 64, 65, 1000)
CTYPES = pytest.mark.parametrize("ctype", [fc.CRC32C, fc.CRC32], ids=["crc32c", "crc32"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class World:
    """One device arena and its host mirror: a pool of chunks and a pool of payloads (every length
    x residue, each once intact and once with a bit flipped after its checksum was taken), and
    three rows of 64 slots for the end-to-end chain.  The pools are never written again."""

    def __init__(self, dev, orc):
        rng = np.random.default_rng(0xF0A4D)
        per_pool = len(LENGTHS) * len(RESIDUES) * 2
        self.size = (2 * per_pool + 3 * 64) * SLOT
        self.host = rng.integers(0, 256, self.size, dtype=np.uint8)
        self.dev = torch.empty(self.size, dtype=torch.uint8, device=dev)
        self.base = self.dev.data_ptr()
        assert self.base % 16 == 0
        self.pool = {"chunk": [], "payload": []}
        cur = 0
        for kind in ("chunk", "payload"):
            for flipped in (False, True):
                for res in RESIDUES:
                    for n in LENGTHS:
                        off = cur + res
                        ck = {t: tuple(orc.create(t, self.host[off:off + n].tobytes())) for t in (fc.CRC32C, fc.CRC32)}
                        if flipped and n:
                            self.host[off + n // 2] ^= 1 << (n % 8)
                        self.pool[kind].append(dict(addr=self.base + off, len=n, res=res, flipped=flipped and n > 0, ck=ck))
                        cur += SLOT
        self.rows = [cur + r * 64 * SLOT for r in range(3)]   # head chunks, successor chunks, payloads
        self.pristine = self.host.copy()
        self.upload()

    def upload(self):
        self.dev.copy_(torch.from_numpy(self.host))
        torch.cuda.synchronize()

    def reset(self):
        self.host[:] = self.pristine
        self.upload()

    def read(self, addr, n):
        o = addr - self.base
        assert 0 <= o and o + n <= self.size, f"the model read outside the arena: {addr:#x} + {n}"
        return self.host[o:o + n].tobytes()

    def unchanged(self, what):
        assert np.array_equal(self.dev.cpu().numpy(), self.host), f"{what}: the data arena changed"

    def lists(self, kind, ctype, flipped=None):
        bufs = [b for b in self.pool[kind] if flipped is None or b["flipped"] == flipped]
        return [b["addr"] for b in bufs], [b["len"] for b in bufs], [b["ck"][ctype] for b in bufs]


@pytest.fixture(scope="module")
def world(dev, orc):
    return World(dev, orc)


def _guarded(dev, nbytes):
    t = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
    return t, t[GUARD:GUARD + nbytes]


class Run:
    """Device images of one batch: the records, d_info and d_commit_idx, each between guards."""

    def __init__(self, dev, jobs):
        self.n = jobs.size
        self.raw_jobs, self.jobs = _guarded(dev, max(jobs.nbytes, 8))
        self.raw_info, self.info = _guarded(dev, 4 * fc.INFO_WORDS)
        self.raw_idx, self.idx = _guarded(dev, 4 * max(self.n, 1))
        self.put(jobs)

    def put(self, jobs):
        if jobs.size:
            self.jobs[:jobs.nbytes].copy_(torch.from_numpy(jobs.view(np.uint8).copy()))
        self.info.fill_(CANARY)
        torch.cuda.synchronize()

    def get(self):
        return self.jobs.cpu().numpy()[:self.n * fc.JOB.itemsize].view(fc.JOB)

    def info_words(self):
        return self.info.cpu().numpy().view(np.uint32).tolist()

    def guards(self, what):
        for name, raw in (("d_jobs", self.raw_jobs), ("d_info", self.raw_info), ("d_commit_idx", self.raw_idx)):
            g = raw.cpu().numpy()
            assert (g[:GUARD] == CANARY).all() and (g[-GUARD:] == CANARY).all(), f"{what}: bytes around {name} written"

    def prepare(self, hf, ctype, max_inline, stream=None):
        hf.forward_prepare(ctype, self.jobs if self.n else None, self.n, self.info, MAX_LEN, max_inline,
                           stream=stream or torch.cuda.current_stream())

    def complete(self, hf, ctype, stream=None, idx=True):
        hf.forward_complete(ctype, self.jobs if self.n else None, self.n, self.info, MAX_LEN,
                            commit_idx=self.idx if idx else None, stream=stream or torch.cuda.current_stream())

    def commit_list(self, count):
        idx = self.idx.cpu().numpy().view(np.uint32)
        assert (self.idx.cpu().numpy()[4 * count:] == CANARY).all(), "d_commit_idx written past the COMMIT count"
        return idx[:count]


def same(got, want, what):
    if got.tobytes() == want.tobytes():
        return
    for f in fc.JOB.names:
        bad = np.flatnonzero((got[f] != want[f]).reshape(got.size, -1).any(axis=1))
        if bad.size:
            i = int(bad[0])
            pytest.fail(f"{what}: {bad.size} jobs differ in {f}, first {i}: got {got[f][i]}, want {want[f][i]}\n"
                        f"{dict(zip(fc.JOB.names, want[i].tolist()))}")


def check_prepare(run, world, want, info, what):
    torch.cuda.synchronize()
    same(run.get(), want, f"{what}: prepare")
    assert run.info_words() == info.tolist(), f"{what}: prepare info {dict(zip(fc.PREP_INFO, run.info_words()))}"
    assert (run.idx.cpu().numpy() == CANARY).all(), f"{what}: prepare wrote d_commit_idx"
    run.guards(what)
    world.unchanged(what)


def check_complete(run, world, want, commits, info, what, idx=True):
    torch.cuda.synchronize()
    same(run.get(), want, f"{what}: complete")
    assert run.info_words() == info.tolist(), f"{what}: complete info {dict(zip(fc.DONE_INFO, run.info_words()))}"
    if idx:
        assert run.commit_list(commits.size).tolist() == commits.tolist(), f"{what}: the commit list"
    else:
        assert (run.idx.cpu().numpy() == CANARY).all(), f"{what}: a NULL d_commit_idx was written"
    run.guards(what)
    world.unchanged(what)


def round_trip(hf, orc, dev, world, jobs, ctype, what, max_inline=64, commit_share=None, stream=None, seed=7):
    """prepare, the successor's answers written by the host, complete; everything against the model."""
    run = Run(dev, jobs)
    run.prepare(hf, ctype, max_inline, stream)
    prepared, pinfo = fc.model_prepare(jobs, ctype, MAX_LEN, max_inline, orc, world.read)
    check_prepare(run, world, prepared, pinfo, what)
    answered = fc.random_answers(np.random.default_rng(seed), prepared.copy(), ctype, commit_share)
    run.put(answered)
    run.complete(hf, ctype, stream)
    done, commits, dinfo = fc.model_complete(answered, ctype, MAX_LEN, orc, world.read)
    check_complete(run, world, done, commits, dinfo, what)
    return prepared, pinfo, done, commits, dinfo


@functools.lru_cache(maxsize=None)
def _mixed(world, ctype, n, seed=0):
    rng = np.random.default_rng(1000 * ctype + n + seed)
    return fc.random_jobs(rng, n, ctype, *world.lists("chunk", ctype), *world.lists("payload", ctype), max_len=MAX_LEN)


# ---- every branch ---------------------------------------------------------------------------------
@CTYPES
@pytest.mark.parametrize("n", SIZES)
def test_every_branch_against_the_model(hf, orc, dev, world, ctype, n):
    jobs = _mixed(world, ctype, n)
    _, pinfo, done, commits, dinfo = round_trip(hf, orc, dev, world, jobs, ctype, f"{n} mixed jobs")
    if n == 1000:   # the batch reaches every counted outcome of both calls
        assert (pinfo[:6] > 0).all(), dict(zip(fc.PREP_INFO, pinfo.tolist()))
        assert (dinfo > 0).all(), dict(zip(fc.DONE_INFO, dinfo.tolist()))
        assert {fc.STALE_UPDATE, 0} <= set(jobs["upd_status"].tolist())
        assert {0, 3, 4010, 4080, 4081, 4082, 7015} <= set(done["final_status"].tolist())
        assert 100 < commits.size < 900


def test_hand_worked_jobs(hf, orc, dev, world):
    """The jobs of tests/test_forward_model.py's branches in one batch, over real buffers."""
    c = world.pool["chunk"][5]      # 4095 bytes at residue 0, intact
    p = world.pool["payload"][4]    # 17 bytes
    sync = dict(successor_syncing=1, chunk=c["addr"], chunk_len=c["len"], chunk_checksum_type=fc.CRC32C,
                chunk_checksum=c["ck"][fc.CRC32C][1], chunk_update_ver=9, chunk_commit_chain_ver=3)
    pay = dict(payload=p["addr"], length=p["len"], upd_length=p["len"], req_checksum=p["ck"][fc.CRC32C][1])
    rows = [dict(), dict(req_update_ver=0), dict(req_update_ver=6), dict(upd_status=fc.MISSING_UPDATE),
            dict(upd_status=fc.ADVANCE_UPDATE), dict(upd_status=fc.COMMITTED_UPDATE), dict(upd_status=fc.STALE_UPDATE),
            dict(upd_status=4010), dict(update_type=fc.COMMIT_TYPE), dict(has_successor=0), sync,
            dict(sync, req_flags=fc.REQ_SYNCING | fc.REQ_INLINE, length=MAX_LEN, chunk_size=MAX_LEN),
            dict(sync, length=MAX_LEN, chunk_size=MAX_LEN), dict(sync, length=MAX_LEN, chunk_size=MAX_LEN, engine_job=1),
            dict(sync, update_type=fc.REMOVE), dict(sync, chunk_status_in=4010),
            dict(sync, length=MAX_LEN, chunk_size=MAX_LEN, chunk_status_in=7007),
            dict(sync, chunk_checksum=sync["chunk_checksum"] ^ 0x100), dict(sync, chunk_checksum_type=fc.NONE, chunk_checksum=0),
            dict(sync, chunk_checksum_type=fc.NONE, chunk_checksum=1), dict(sync, chunk_checksum_type=fc.CRC32),
            dict(sync, chunk_len=4097), dict(sync, chunk=0), dict(update_type=fc.REMOVE, length=0, payload=0),
            dict(update_type=fc.TRUNCATE, payload=0, length=50)]
    jobs = np.concatenate([fc.plain_job(**dict(pay, **r)) for r in rows])
    prepared, pinfo, _, _, _ = round_trip(hf, orc, dev, world, jobs, fc.CRC32C, "hand-worked", max_inline=4095)
    assert prepared["status"].tolist()[:10] == [0, 0, 4082, 4007, 4012, 0, 0, 4010, 3, 0]
    assert prepared["action"].tolist()[:10] == [2, 2, 1, 1, 1, 1, 2, 1, 1, 3]
    assert prepared["status"].tolist()[10:23] == [0, 0, 0, 0, 0, 4010, 7007, 4080, 0, 4080, 3, 3, 3]
    assert prepared["out_length"].tolist()[10:15] == [4095, 4095, MAX_LEN, MAX_LEN, 17]
    assert prepared["out_flags"][10] == fc.OUT_SYNCING | fc.OUT_COMMIT_CHAIN_VER | fc.OUT_INLINE
    assert pinfo.tolist()[:6] == [11, 13, 1, 3, 2, 4]


# ---- the two hashing rungs ------------------------------------------------------------------------
@CTYPES
def test_syncing_reads_of_intact_and_flipped_chunks(hf, orc, dev, world, ctype):
    """Every chunk of the pool behind a partial write to a SYNCING successor: the 4080 set is the
    flipped set exactly, every `computed` is the oracle's, every intact chunk goes out whole."""
    pool = world.pool["chunk"]
    jobs = np.concatenate([fc.plain_job(successor_syncing=1, chunk=c["addr"], chunk_len=c["len"], chunk_checksum_type=ctype,
                                        chunk_checksum=c["ck"][ctype][1], chunk_update_ver=2, upd_checksum_type=ctype,
                                        req_checksum_type=ctype, payload=world.pool["payload"][2]["addr"], length=15)
                           for c in pool])
    prepared, pinfo, done, _, _ = round_trip(hf, orc, dev, world, jobs, ctype, "syncing reads", max_inline=16)
    flipped = [i for i, c in enumerate(pool) if c["flipped"]]
    assert np.flatnonzero(prepared["status"] == 4080).tolist() == flipped and len(flipped) == 18
    assert set(prepared["status"].tolist()) == {0, 4080}
    for i, c in enumerate(pool):
        assert prepared["computed"][i] == orc.create(ctype, world.read(c["addr"], c["len"]))[1]
        if not c["flipped"]:
            assert (prepared["out_data"][i], prepared["out_length"][i]) == (c["addr"], c["len"])
            assert bool(prepared["out_flags"][i] & fc.OUT_INLINE) == (c["len"] <= 16)
    assert pinfo.tolist()[:6] == [len(pool) - 18, 18, 0, len(pool) - 6, 18, 0]   # six empty chunks hash nothing
    assert np.count_nonzero(done["buffer_corrupted"]) == 0   # an intact chunk answered 4080 is not a corrupted buffer


@CTYPES
def test_outgoing_buffers_behind_a_4080_answer(hf, orc, dev, world, ctype):
    """Every payload of the pool sent as it is and answered 4080: buffer_corrupted is set for the
    flipped ones exactly; the same for whole chunks sent after a syncing read."""
    pays = world.pool["payload"]
    jobs = np.concatenate([fc.plain_job(payload=p["addr"], length=p["len"], upd_length=p["len"], req_checksum_type=ctype,
                                        req_checksum=p["ck"][ctype][1], upd_checksum_type=ctype) for p in pays])
    run = Run(dev, jobs)
    run.prepare(hf, ctype, 0)
    prepared, pinfo = fc.model_prepare(jobs, ctype, MAX_LEN, 0, orc, world.read)
    check_prepare(run, world, prepared, pinfo, "plain payloads")
    assert pinfo.tolist()[:6] == [len(pays), 0, 0, 0, 0, 0]
    for i in range(len(pays)):
        fc.answer(prepared, i, fwd_status=4080 if i % 7 != 6 else 0)
    run.put(prepared)
    run.complete(hf, ctype)
    done, commits, dinfo = fc.model_complete(prepared, ctype, MAX_LEN, orc, world.read)
    check_complete(run, world, done, commits, dinfo, "4080 answers")
    want = [i for i, p in enumerate(pays) if p["flipped"] and i % 7 != 6]
    assert np.flatnonzero(done["buffer_corrupted"]).tolist() == want and len(want) >= 12
    assert commits.tolist() == [i for i in range(len(pays)) if i % 7 == 6]
    assert dinfo[5] == sum(1 for i, p in enumerate(pays) if p["len"] and i % 7 != 6) and dinfo[6] == len(want)


# ---- the commit list ------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [1 / 3, 1.0, 0.0], ids=["third", "all", "none"])
def test_commit_list_of_1000(hf, orc, dev, world, share):
    p = world.pool["payload"][3]
    rng = np.random.default_rng(33)
    jobs = np.concatenate([fc.plain_job(payload=p["addr"], length=p["len"], upd_length=p["len"],
                                        req_checksum=p["ck"][fc.CRC32C][1])] * 1000)
    jobs["upd_checksum"] = rng.integers(0, 1 << 32, 1000, dtype=np.uint64)
    run = Run(dev, jobs)
    run.prepare(hf, fc.CRC32C, 64)
    prepared, pinfo = fc.model_prepare(jobs, fc.CRC32C, MAX_LEN, 64, orc, world.read)
    check_prepare(run, world, prepared, pinfo, f"commit share {share}")
    assert pinfo.tolist() == [1000, 0, 0, 0, 0, 0, 0, 0]   # (a call in which nothing hashes)
    answered = fc.random_answers(np.random.default_rng(11), prepared.copy(), fc.CRC32C, share)
    run.put(answered)
    run.complete(hf, fc.CRC32C)
    done, commits, dinfo = fc.model_complete(answered, fc.CRC32C, MAX_LEN, orc, world.read)
    check_complete(run, world, done, commits, dinfo, f"commit share {share}")
    got_info, got_idx = run.info_words(), run.idx.cpu().numpy()
    assert got_info[0] == commits.size and got_info[1] == 1000 - commits.size
    if share == 1.0:
        assert commits.tolist() == list(range(1000)) and got_idx.view(np.uint32).tolist() == list(range(1000))
    elif share == 0.0:   # every share counts 0, the scan sets 0, the scatter writes no word
        assert commits.size == 0 and got_info[0] == 0 and got_info[1] == 1000
        assert (got_idx == CANARY).all(), "d_commit_idx written though no job commits"
        assert set(done["final_status"].tolist()) == {4010, 4080, 4081, 4082}
    else:   # 1000 draws at 1/3: mean 333, standard deviation 14.9; the bound is four of them
        assert 273 < commits.size < 393 and (np.diff(commits.astype(np.int64)) > 0).all()
        assert set(np.unique(commits // 256).tolist()) == {0, 1, 2, 3}   # every share of 256 jobs contributes


def test_null_commit_list_and_empty_batch(hf, orc, dev, world):
    jobs = _mixed(world, fc.CRC32C, 65)
    prepared, _ = fc.model_prepare(jobs, fc.CRC32C, MAX_LEN, 64, orc, world.read)
    answered = fc.random_answers(np.random.default_rng(2), prepared.copy(), fc.CRC32C)
    run = Run(dev, answered)
    run.complete(hf, fc.CRC32C, idx=False)
    done, commits, dinfo = fc.model_complete(answered, fc.CRC32C, MAX_LEN, orc, world.read)
    check_complete(run, world, done, commits, dinfo, "NULL d_commit_idx", idx=False)
    empty = Run(dev, fc.blank(0))
    for call in (lambda: empty.prepare(hf, fc.CRC32C, 0), lambda: empty.complete(hf, fc.CRC32C)):
        empty.info.fill_(CANARY)
        call()
        torch.cuda.synchronize()
        assert empty.info_words() == [0] * fc.INFO_WORDS
        empty.guards("n == 0")
        assert (empty.idx.cpu().numpy() == CANARY).all() and (empty.jobs.cpu().numpy() == CANARY).all()


# ---- contexts -------------------------------------------------------------------------------------
def test_poisoned_scratch(hf, orc, dev, world, opts):
    """Every scratch word is written before it is read: the results do not change when the call's
    scratch starts from a pattern."""
    opts("poison", 0xA5A5A5A5)
    st = torch.cuda.Stream(dev)
    for n in (65, 1000):
        round_trip(hf, orc, dev, world, _mixed(world, fc.CRC32C, n), fc.CRC32C, f"poisoned, {n} jobs", stream=st)
    hf._lib.release_stream(st)


def test_scratch_does_not_grow_after_the_largest_call(hf, orc, dev, world):
    L = hf._lib
    st = torch.cuda.Stream(dev)
    round_trip(hf, orc, dev, world, _mixed(world, fc.CRC32C, 1000), fc.CRC32C, "largest", stream=st)
    st0 = L.pair_scratch_stats(st)
    assert 0 < st0["call_bytes"] <= L.forward_scratch_bytes(1000)
    for n in (65, 1000, 1):
        round_trip(hf, orc, dev, world, _mixed(world, fc.CRC32, n), fc.CRC32, "smaller", stream=st)
    assert L.pair_scratch_stats(st) == st0
    L.release_stream(st)


def test_scratch_is_a_function_of_n_alone(hf, orc, dev, world):
    """A complete first, then a prepare of the same n whose max_len bound makes it hash as byte runs
    (n * max_len >= 1 GiB): both reserve the run tables, so the pair's buffer does not grow.  At
    12,000 jobs the tables (82 KB on 256 CUs) decide between a buffer of 256 KiB and one of 512 KiB."""
    L = hf._lib
    n, ctype, wide = 12000, fc.CRC32C, 1 << 20
    jobs = fc.random_jobs(np.random.default_rng(12), n, ctype, *world.lists("chunk", ctype),
                          *world.lists("payload", ctype), max_len=MAX_LEN)
    prepared, _ = fc.model_prepare(jobs, ctype, MAX_LEN, 64, orc, world.read)
    answered = fc.random_answers(np.random.default_rng(13), prepared.copy(), ctype)
    st = torch.cuda.Stream(dev)
    run = Run(dev, answered)
    run.complete(hf, ctype, st)
    done, commits, dinfo = fc.model_complete(answered, ctype, MAX_LEN, orc, world.read)
    check_complete(run, world, done, commits, dinfo, "complete first")
    st0 = L.pair_scratch_stats(st)
    assert 0 < st0["call_bytes"] <= L.forward_scratch_bytes(n)
    run = Run(dev, jobs)
    hf.forward_prepare(ctype, run.jobs, n, run.info, wide, 64, stream=st)
    want, pinfo = fc.model_prepare(jobs, ctype, wide, 64, orc, world.read)
    check_prepare(run, world, want, pinfo, "prepare as byte runs")
    assert pinfo[3] > 1000 and pinfo[4] > 500
    assert L.pair_scratch_stats(st) == st0
    L.release_stream(st)


def _with_answers(jobs, ctype, orc, world, seed):
    """The records as the host hands them to a graph that holds both calls: the answers of the jobs
    prepare will send are in place already (prepare leaves a sent job's response alone)."""
    prepared, _ = fc.model_prepare(jobs, ctype, MAX_LEN, 64, orc, world.read)
    answered = fc.random_answers(np.random.default_rng(seed), prepared.copy(), ctype)
    start = jobs.copy()
    for k in fc.RESPONSE:
        start[k] = answered[k]
    return start


def _expect_both(start, ctype, orc, world):
    prepared, _ = fc.model_prepare(start, ctype, MAX_LEN, 64, orc, world.read)
    return fc.model_complete(prepared, ctype, MAX_LEN, orc, world.read)


def test_both_calls_in_one_graph_replan_at_every_replay(hf, orc, dev, world):
    """prepare and complete captured in one graph; replayed on the records as captured, then after
    the records are rewritten and one chunk has a bit flipped, and back."""
    ctype = fc.CRC32C
    first = _with_answers(_mixed(world, ctype, 65), ctype, orc, world, 1)
    run = Run(dev, first)
    pinfo = torch.full((fc.INFO_WORDS,), -1, dtype=torch.int32, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        hf.forward_prepare(ctype, run.jobs, run.n, pinfo, MAX_LEN, 64, stream=torch.cuda.current_stream())
        run.complete(hf, ctype, stream=torch.cuda.current_stream())
    victim = next(c for c in world.pool["chunk"] if c["len"] == 4095 and c["res"] == 1 and not c["flipped"])
    at = victim["addr"] - world.base + 2000
    try:
        for k, (seed, flip) in enumerate(((0, False), (5, True), (0, False))):
            if flip:
                world.host[at] ^= 0x04
            else:
                world.host[at] = world.pristine[at]
            world.upload()
            start = _with_answers(_mixed(world, ctype, 65, seed), ctype, orc, world, 1 + seed)
            if flip:   # the rewritten records read the flipped chunk: its job is a 4080 now
                start["chunk"][3], start["chunk_len"][3] = victim["addr"], victim["len"]
                start["chunk_checksum_type"][3], start["chunk_checksum"][3] = victim["ck"][ctype]
                start["update_type"][3], start["upd_status"][3], start["req_update_ver"][3] = fc.WRITE, 0, 0
                start["has_successor"][3] = start["successor_syncing"][3] = 1
                start["req_flags"][3], start["chunk_status_in"][3] = fc.REQ_SYNCING, 0
            run.put(start)
            run.idx.fill_(CANARY)
            torch.cuda.synchronize()
            g.replay()
            done, commits, dinfo = _expect_both(start, ctype, orc, world)
            check_complete(run, world, done, commits, dinfo, f"replay {k}")
            if flip:
                assert (done["status"][3], done["final_status"][3]) == (4080, 4080)
    finally:
        world.reset()
    del g


# ---- behind hf3fs_crc_update_versioned, and the whole chain ---------------------------------------
def _head_batch(world, orc, hf, ctype, seed):
    """64 writes, one per head chunk, as update_versioned takes them, the head's bytes and metadata
    after them worked out on the host, and the forward jobs filled from that: every fourth
    successor is SYNCING (and starts empty), every sixteenth target has none."""
    rng = np.random.default_rng(seed)
    head, succ, pay = world.rows
    ios = np.zeros(64, dtype=ufp.REC)
    ver = np.zeros(64, dtype=hf._lib.update_ver_dtype())
    jobs = fc.blank(64)
    succ_state = []
    for i in range(64):
        h, s, p = head + i * SLOT, succ + i * SLOT, pay + i * SLOT + RESIDUES[i % 3]
        size0 = (0, 100, 2048, 4095, 4096)[i % 5]
        syncing = i % 4 == 1
        if i % 8 < 2:
            off, ln = 0, MAX_LEN
        else:
            ln = LENGTHS[1 + int(rng.integers(0, 6))]
            off = int(rng.integers(0, MAX_LEN - ln + 1))
        old = world.host[h:h + size0].copy()
        if syncing:
            succ_state.append((0, tuple(orc.create(ctype, b""))))
        else:
            world.host[s:s + size0] = old
            succ_state.append((size0, tuple(orc.create(ctype, old.tobytes()))))
        data = world.host[p:p + ln].copy()
        size1 = max(size0, off + ln)
        new = np.zeros(size1, dtype=np.uint8)
        new[:size0] = old
        new[off:off + ln] = data
        wck, ck0, ck1 = (orc.create(ctype, x.tobytes()) for x in (data, old, new))
        io_ver = 0 if i % 2 == 0 else 4
        ios[i] = (world.base + h, world.base + p, off, ln, size0, fc.WRITE, ctype, ctype, 0, ck0[1], wck[1], 0, 0, 0, 0,
                  (0, 0), -1)
        for k, v in dict(io_ver=io_ver, job_chain_ver=7, chain_ver=7, update_ver=3, commit_ver=3, meta_chunk_size=MAX_LEN,
                         chunk_state=0).items():
            ver[k][i] = v
        for k, v in dict(update_type=fc.WRITE, offset=off, length=ln, chunk_size=MAX_LEN, payload=world.base + p,
                         req_update_ver=io_ver, req_checksum_type=ctype, req_checksum=wck[1], upd_status=0,
                         upd_length=ln, upd_update_ver=4, upd_commit_ver=3, upd_checksum_type=ctype, upd_checksum=ck1[1],
                         chain_ver=7, has_successor=int(i % 16 != 7), successor_syncing=int(syncing),
                         chunk=world.base + h, chunk_len=size1, chunk_checksum_type=ctype, chunk_checksum=ck1[1],
                         chunk_update_ver=4, chunk_commit_chain_ver=7).items():
            jobs[k][i] = v
        world.host[h:h + size1] = new      # the mirror holds the head as the update leaves it ...
        ios["out_size"][i], ios["out_checksum"][i] = size1, ck1[1]   # (kept for the comparison; the call overwrites them)
    before = world.host.copy()
    for i in range(64):                    # ... and the device the head as the update finds it
        h = head + i * SLOT
        before[h:h + SLOT] = world.pristine[h:h + SLOT]
    world.dev.copy_(torch.from_numpy(before))
    torch.cuda.synchronize()
    return ios, ver, jobs, succ_state


def _queue_update_and_prepare(hf, dev, world, ctype, ios, ver, run, st, then=None):
    d_ios = torch.from_numpy(ios.view(np.uint8).copy()).to(dev)
    d_ver = torch.from_numpy(ver.view(np.uint8).copy()).to(dev)
    vinfo = torch.zeros(8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hf._lib.update_versioned(ctype, d_ios, d_ver, 64, MAX_LEN, 1, mode=hf.MODE_REFERENCE, info=vinfo, stream=st)
    run.prepare(hf, ctype, 64, st)
    if then:
        then()
    st.synchronize()
    got_ios = d_ios.cpu().numpy().view(ufp.REC)
    got_ver = d_ver.cpu().numpy().view(ver.dtype)
    assert (got_ios["status"] == 0).all(), got_ios["status"].tolist()
    assert np.array_equal(got_ios["out_size"], ios["out_size"]) and np.array_equal(got_ios["out_checksum"], ios["out_checksum"])
    assert (got_ver["out_update_ver"] == 4).all() and (got_ver["out_commit_ver"] == 3).all()
    return got_ios, got_ver


@CTYPES
def test_queued_behind_update_versioned(hf, orc, dev, world, ctype):
    """update_versioned writes the head chunks; prepare, queued directly behind it, hashes them for
    the syncing successors against the checksums the update must have left; complete follows with
    the answers in place.  One stream, one wait at the end."""
    try:
        ios, ver, jobs, _ = _head_batch(world, orc, hf, ctype, 21)
        start = _with_answers(jobs, ctype, orc, world, 4)
        run = Run(dev, start)
        pinfo = run.info
        dinfo_t = torch.full((fc.INFO_WORDS,), -1, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(dev)

        def then():
            hf.forward_complete(ctype, run.jobs, 64, dinfo_t, MAX_LEN, commit_idx=run.idx, stream=st)

        _queue_update_and_prepare(hf, dev, world, ctype, ios, ver, run, st, then)
        prepared, want_pinfo = fc.model_prepare(start, ctype, MAX_LEN, 64, orc, world.read)
        done, commits, want_dinfo = fc.model_complete(prepared, ctype, MAX_LEN, orc, world.read)
        assert pinfo.cpu().numpy().view(np.uint32).tolist() == want_pinfo.tolist()
        assert want_pinfo[3] >= 3 and want_pinfo[4] == 0 and want_pinfo[2] == 4   # hashed, none mismatched
        same(run.get(), done, "queued")
        assert dinfo_t.cpu().numpy().view(np.uint32).tolist() == want_dinfo.tolist()
        assert run.commit_list(commits.size).tolist() == commits.tolist()
        run.guards("queued")
        world.unchanged("queued")
        hf._lib.release_stream(st)
    finally:
        world.reset()


@CTYPES
def test_chain_of_head_and_successor(hf, orc, dev, world, ctype):
    """update_versioned on the head, prepare, the outgoing records applied to the successor's chunks
    with update_batch (SYNCING where prepare says so), its results as the answers, complete, and
    the commit list as COMMIT jobs for update_versioned: both replicas end with the same bytes and
    checksums, and every commit is applied."""
    L = hf._lib
    try:
        ios, ver, jobs, succ_state = _head_batch(world, orc, hf, ctype, 22)
        run = Run(dev, jobs)
        st = torch.cuda.Stream(dev)
        got_ios, got_ver = _queue_update_and_prepare(hf, dev, world, ctype, ios, ver, run, st)
        prepared, pinfo = fc.model_prepare(jobs, ctype, MAX_LEN, 64, orc, world.read)
        check_prepare(run, world, prepared, pinfo, "chain: prepare")
        assert pinfo.tolist()[:3] == [60, 0, 4] and pinfo[3] >= 3 and pinfo[4] == 0 and pinfo[5] == 0
        # the "send": the successor applies what prepare built
        sent = np.flatnonzero(prepared["action"] == fc.SEND)
        sios = np.zeros(sent.size, dtype=ufp.REC)
        succ = world.rows[1]
        for k, i in enumerate(sent):
            size, ck = succ_state[i]
            o = prepared[i]
            sios[k] = (world.base + succ + i * SLOT, o["out_data"], o["out_offset"], o["out_length"], size,
                       o["out_update_type"], ctype, o["out_checksum_type"],
                       hf.FLAG_SYNCING if o["out_flags"] & fc.OUT_SYNCING else 0, ck[1], o["out_checksum"], 0, 0, 0, 0,
                       (0, 0), -1)
        d_sios = torch.from_numpy(sios.view(np.uint8).copy()).to(dev)
        L.update_batch(ctype, d_sios, sent.size, MAX_LEN, mode=hf.MODE_REFERENCE, stream=st)
        st.synchronize()
        sres = d_sios.cpu().numpy().view(ufp.REC)
        assert (sres["status"] == 0).all(), sres["status"].tolist()
        for k, i in enumerate(sent):
            fc.answer(prepared, i, fwd_status=int(sres["status"][k]), fwd_length=int(sios["length"][k]),
                      fwd_checksum_type=int(sres["out_checksum_type"][k]), fwd_checksum=int(sres["out_checksum"][k]),
                      fwd_commit_ver=int(prepared["res_update_ver"][i]), fwd_commit_chain_ver=7)
        after_send = world.dev.cpu().numpy()
        run.put(prepared)
        run.complete(hf, ctype, st)
        st.synchronize()
        done, commits, dinfo = fc.model_complete(prepared, ctype, MAX_LEN, orc, world.read)
        same(run.get(), done, "chain: complete")
        assert commits.tolist() == list(range(64)) and run.commit_list(64).tolist() == list(range(64))
        assert dinfo.tolist() == [64, 0, 0, 0, 0, 0, 0, 0] == run.info_words()
        # the commit list as COMMIT jobs on the head
        cios = got_ios.copy()
        cios["update_type"] = hf.UPDATE_COMMIT
        cios["chunk_size"], cios["chunk_checksum"] = got_ios["out_size"], got_ios["out_checksum"]
        cios["chunk_checksum_type"] = got_ios["out_checksum_type"]
        cver = got_ver.copy()
        for k in ("chain_ver", "update_ver", "commit_ver", "chunk_state", "recycle_state"):
            cver[k] = got_ver["out_" + k]
        cver["io_ver"], cver["job_chain_ver"] = done["commit_ver"], done["commit_chain_ver"]
        d_cios = torch.from_numpy(cios.view(np.uint8).copy()).to(dev)
        d_cver = torch.from_numpy(cver.view(np.uint8).copy()).to(dev)
        L.update_versioned(ctype, d_cios, d_cver, 64, MAX_LEN, 1, mode=hf.MODE_REFERENCE, stream=st)
        st.synchronize()
        rios, rver = d_cios.cpu().numpy().view(ufp.REC), d_cver.cpu().numpy().view(ver.dtype)
        assert (rios["status"] == 0).all(), rios["status"].tolist()
        assert (rver["out_commit_ver"] == 4).all() and (rver["out_chunk_state"] == 0).all()   # COMMIT, version 4
        # both replicas
        final = world.dev.cpu().numpy()
        assert np.array_equal(final, after_send)          # complete and the commits touch no byte
        head = world.rows[0]
        for k, i in enumerate(sent):
            size = int(got_ios["out_size"][i])
            assert int(sres["out_size"][k]) == size, i
            assert (int(sres["out_checksum_type"][k]), int(sres["out_checksum"][k])) == (ctype, int(got_ios["out_checksum"][i]))
            h, s = head + i * SLOT, succ + i * SLOT
            assert np.array_equal(final[h:h + size], final[s:s + size]), f"replicas of chunk {i} differ"
            assert np.array_equal(final[h:h + size], world.host[h:h + size])
        L.release_stream(st)
    finally:
        world.reset()
