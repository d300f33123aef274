"""Batch calls queued back to back on one stream, one wait at the end: what include/hf3fs_crc.h
promises ("asynchronous on stream", no host synchronisation) and a storage worker relies on.

Every other GPU test puts the call under test between two host synchronizes.  Here all tensors
are made and filled first (one torch.cuda.synchronize()), the library calls then go onto a fresh
stream with nothing between them, one wait follows, and only then are results copied back:

  a. six update_batch calls on the same 32 chunks, each reading what the one before wrote
     (tests/stream_queue.py check_queue), byte-identical with the twin run that synchronizes
     after every call; rounds of 8..32 IOs that regrow the pair buffer in mid-queue.
  b. a scrub and a read-result batch directly behind the updates, on the same stream and on a
     second one across an event; release_stream as the one wait.
  c. every case of tests/batch_cases.py through one pair buffer, an update between every two.
  d. device-side hand-overs: create -> verify, create -> combine -> finalize -> serialize,
     frames' computed column -> their header column, create -> block table -> file digest.
  e. the six updates and the scrub captured into one graph.

All comparisons are bit-exact against the oracle (tests/update_footprint.py, tests/batch_cases.py)."""
import functools

import numpy as np
import pytest

import batch_cases as bc
import stream_queue as sq
import update_footprint as fp
from test_gpu_batch_contexts import OnDevice, check, timeline

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
LINE = 16 << 10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _scenario(orc, kind, ctype=fp.CRC32C, rounds=6):
    """Built once and shared: the expected images do not depend on how the calls are queued."""
    if kind == "engine":
        return fp.engine_scenario(orc, rounds=rounds)
    if kind == "growth":
        return sq.growth_scenario(orc)
    if kind == "growth_wide":
        return sq.growth_scenario(orc, sq.GROWTH_COUNTS_WIDE, max_len=4096, gap=2048)
    return fp.rounds_scenario(orc, ctype, n=32, max_len=128 << 10, rounds=rounds)


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def _set_pipeline(opts, pipeline):
    """"default": no switch (the pair's hint decides per call); "fused"; "oneshot": the three-pass
    pipeline with the one-shot apply (its finalize on the side stream); "ticketed"."""
    if pipeline == "fused":
        opts("update_pipeline", "fused")
    elif pipeline != "default":
        opts("update_pipeline", "unfused")
        opts("apply_grid", 1 if pipeline == "oneshot" else 0)


class DeviceQueue:
    """A scenario with every round resident: one arena, a payload and a record buffer per round."""

    def __init__(self, scn, dev, ctype=None):
        self.scn, self.ctype = scn, scn.ctype if ctype is None else ctype
        img = scn.image_before(0)
        self.raw = torch.empty(img.size + LINE, dtype=torch.uint8, device=dev)
        lift = (-self.raw.data_ptr()) % LINE  # the arena starts on a 16 KiB line
        self.arena = self.raw[lift:lift + img.size]
        self.arena0 = _up(img, dev)
        self.pays = [_up(scn.payload_image(k), dev) for k in range(len(scn.rounds))]
        self.sent = sq.queue_records(scn, self.arena.data_ptr(), [p.data_ptr() for p in self.pays])
        self.recs0 = [_up(b, dev) for b in self.sent]
        self.recs = [torch.empty_like(b) for b in self.recs0]
        self.counts = sq.round_counts(scn)
        self.restore()

    def restore(self):
        self.arena.copy_(self.arena0)
        for r, r0 in zip(self.recs, self.recs0):
            r.copy_(r0)
        torch.cuda.synchronize()

    def call(self, L, k, mode, st):
        L.update_batch(self.ctype, self.recs[k].data_ptr() + fp.REC_GUARD, self.counts[k], self.scn.max_len,
                       mode=mode, stream=st.cuda_stream)

    def enqueue(self, L, mode, st, sync_each=False):
        for k in range(len(self.recs)):
            self.call(L, k, mode, st)
            if sync_each:
                st.synchronize()

    def fetch(self):
        return self.arena.cpu().numpy(), [p.cpu().numpy() for p in self.pays], [r.cpu().numpy() for r in self.recs]

    def check(self):
        got = self.fetch()
        sq.check_queue(self.scn, got[0], got[1], got[2], self.sent)
        return got


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: the chunk arena differs between the queue and its twin"
    for k, (x, y) in enumerate(zip(a[2], b[2])):
        assert np.array_equal(x, y), f"{what}: round {k}'s record buffer differs between the queue and its twin"


# ---- a. update rounds queued on the same chunks ----------------------------------------------------
ROWS = [(p, m, "rounds", fp.CRC32C) for p in ("default", "fused", "oneshot", "ticketed") for m in (0, 1)] + \
    [("default", m, "rounds", fp.CRC32) for m in (0, 1)] + \
    [(p, m, "engine", fp.CRC32C) for p in ("default", "oneshot") for m in (0, 1)]
ROW_IDS = [f"{p}-mode{m}-{k}-{'crc32c' if t == fp.CRC32C else 'crc32'}" for p, m, k, t in ROWS]


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_queued_update_rounds(hf, orc, dev, opts, row):
    """Six update_batch calls on the same 32 chunks with no host step between them, then the twin
    with a synchronize after each call: both must leave the oracle's bytes, and the same bytes."""
    pipeline, mode, kind, ctype = row
    L = hf._lib
    _set_pipeline(opts, pipeline)
    q = DeviceQueue(_scenario(orc, kind, ctype), dev)
    L.anomalies(0, reset=True)
    st = torch.cuda.Stream(dev)
    q.enqueue(L, mode, st)
    st.synchronize()
    queued = q.check()
    q.restore()
    q.enqueue(L, mode, st, sync_each=True)
    twin = q.check()
    _same(queued, twin, ROW_IDS[ROWS.index(row)])
    a = L.anomalies(0)
    assert a["count"] == 0, a
    L.release_stream(st)


ROOMY = 256 << 10  # pair_buffer sizes the call buffer up to a multiple of 64 Ki words (roomy_words, hf3fs_crc_api.hip)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["growth", "growth_wide"])
def test_queue_regrows_pair_buffer(hf, orc, dev, kind, mode):
    """Rounds of 8, 32, 4, 32, 16, 32 IOs on 128 KiB chunks, built by slicing each round's records;
    the same queue a second time on the same stream allocates nothing.  At these counts the call
    buffer's first allocation (rounded up to 256 KiB) already holds 32 IOs, so the wide row repeats
    it with 64, 2048, 32, 2048, 512, 2048 IOs on 4 KiB chunks: the second call needs more than
    the first one's 256 KiB, and pair_buffer has to wait for the stream, free and reallocate with
    the first call still queued."""
    L = hf._lib
    q = DeviceQueue(_scenario(orc, kind), dev)
    assert q.counts == list(sq.GROWTH_COUNTS if kind == "growth" else sq.GROWTH_COUNTS_WIDE)
    L.anomalies(0, reset=True)
    st = torch.cuda.Stream(dev)
    L.release_stream(st)  # (streams come from a pool: whatever an earlier test left on this one goes)
    start = L.pair_scratch_stats(st)
    assert start["call_bytes"] == 0
    q.enqueue(L, mode, st)
    L.stream_wait(st)
    q.check()
    q.restore()
    before = L.pair_scratch_stats(st)
    if kind == "growth_wide":
        assert L.update_scratch_bytes(q.counts[0], mode) <= ROOMY < L.update_scratch_bytes(q.counts[1], mode)
        assert before["allocations"] >= start["allocations"] + 2 and before["call_bytes"] > ROOMY, (start, before)
    q.enqueue(L, mode, st)
    L.stream_wait(st)
    after = L.pair_scratch_stats(st)
    q.check()
    assert after["allocations"] == before["allocations"], (before, after)
    assert L.anomalies(0)["count"] == 0
    L.release_stream(st)


# ---- b. a record batch directly behind the updates ------------------------------------------------
class FollowUp:
    def __init__(self, q, dev):
        self.q = q
        self.fu = sq.followup_records(q.scn, q.arena.data_ptr())
        self.scrub0, self.read0 = _up(self.fu["scrub"], dev), _up(self.fu["read"], dev)
        self.scrub, self.read = torch.empty_like(self.scrub0), torch.empty_like(self.read0)
        self.count = torch.empty(1, dtype=torch.int32, device=dev)
        self.restore()

    def restore(self):
        self.scrub.copy_(self.scrub0)
        self.read.copy_(self.read0)
        self.count.fill_(0x5E5E5E5E)
        torch.cuda.synchronize()

    def enqueue(self, L, st):
        n, ctype = self.q.scn.n, self.q.ctype
        L.scrub_batch(ctype, self.scrub.data_ptr(), n, self.fu["max_len"], self.count.data_ptr(), stream=st.cuda_stream)
        L.read_result_batch(ctype, self.read.data_ptr(), n, self.fu["max_len"], stream=st.cuda_stream)

    def check(self):
        sq.check_followup(self.fu, self.scrub.cpu().numpy().view(bc.SCRUB_DT), self.read.cpu().numpy().view(bc.READ_DT),
                          self.count.cpu().numpy().view(np.uint32)[0])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pipeline,kind", [("default", "rounds"), ("oneshot", "rounds"), ("oneshot", "engine")])
def test_records_behind_updates_same_stream(hf, orc, dev, opts, pipeline, kind, mode):
    """scrub_batch and read_result_batch over every chunk queued directly behind the six updates:
    no mismatch, the oracle's values.  release_stream, with nothing in front of it, is the wait;
    then the same on the same stream handle, whose pair record is gone."""
    L = hf._lib
    _set_pipeline(opts, pipeline)
    q = DeviceQueue(_scenario(orc, kind), dev)
    f = FollowUp(q, dev)
    L.anomalies(0, reset=True)
    st = torch.cuda.Stream(dev)
    for _ in range(2):
        q.enqueue(L, mode, st)
        f.enqueue(L, st)
        L.release_stream(st)
        f.check()
        q.check()
        q.restore()
        f.restore()
    assert L.anomalies(0)["count"] == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["rounds", "engine"])
def test_records_behind_updates_across_event(hf, orc, dev, opts, kind, mode):
    """The record batches run on a second stream that waits for an event recorded behind the last
    one-shot update: the side stream's finalize of every call must be in front of that event."""
    L = hf._lib
    _set_pipeline(opts, "oneshot")
    q = DeviceQueue(_scenario(orc, kind), dev)
    f = FollowUp(q, dev)
    st, st2, ev = torch.cuda.Stream(dev), torch.cuda.Stream(dev), torch.cuda.Event()
    q.enqueue(L, mode, st)
    ev.record(st)
    st2.wait_event(ev)
    f.enqueue(L, st2)
    st2.synchronize()
    f.check()
    q.check()
    L.release_stream(st)
    L.release_stream(st2)


# ---- c. every entry point through one pair buffer -------------------------------------------------
def test_every_entry_point_through_one_pair_buffer(hf, orc, dev, cus, opts):
    """Every case of tests/batch_cases.py queued on one stream with a one-shot update_batch between
    every two: each call carves the pair's one call buffer its own way and starts on what another
    entry point left there.  In the cases' order, in reverse without a new allocation, and once
    more on poisoned scratch."""
    L = hf._lib
    names = list(bc.CASES)
    _set_pipeline(opts, "oneshot")
    q = DeviceQueue(_scenario(orc, "rounds", fp.CRC32C, len(names) - 1), dev)
    steps = {n: timeline(n, cus)[0] for n in names}
    dvs = {n: OnDevice(bc.CASES[n], steps[n][0], dev) for n in names}
    assert sum(bc.CASES[n].device_bytes(steps[n][0]) for n in names) < 4 << 30
    L.anomalies(0, reset=True)
    st = torch.cuda.Stream(dev)
    L.release_stream(st)
    allocs = None
    for what, order, poison in (("in order", names, 0), ("reversed", names[::-1], 0),
                                ("reversed, poisoned", names[::-1], 0xA5A5A5A5)):
        if poison:
            opts("poison", poison)
        for k, n in enumerate(order):
            if k:
                q.call(L, k - 1, 1, st)
            dvs[n].run(L, steps[n][0], st.cuda_stream)
        st.synchronize()
        if poison:
            opts("poison", 0)
        now = L.pair_scratch_stats(st)["allocations"]
        if what == "reversed":
            assert now == allocs, f"the reversed queue allocated: {allocs} -> {now}"
        allocs = now
        for n in names:
            check(dvs[n], steps[n][0], steps[n][1], f"{n} ({what})")
        q.check()
        q.restore()
        for n in names:
            dvs[n].load(steps[n][0])
    a = L.anomalies(0)
    assert a["count"] == 0 and a["kinds"] == 0, a
    L.release_stream(st)


# ---- d. hand-over on the device --------------------------------------------------------------------
def _i32(n, dev, fill=0x5E5E5E5E):
    return torch.full((n,), fill, dtype=torch.int32, device=dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_create_then_verify_on_device(hf, orc, dev):
    """create_strided's output is verify_strided's `expected` with no host step; one bit flipped by
    a device op must be the one mismatch.  Then the same through create_batch / verify_batch with
    the library's own `computed` scratch."""
    L = hf._lib
    n, ln, j = 64, (64 << 10) + 100, 37
    stride = ln + 28
    host = np.random.default_rng(0xD1).integers(0, 256, n * stride, dtype=np.uint8)
    buf = _up(host, dev)
    addrs = torch.from_numpy(buf.data_ptr() + np.arange(n, dtype=np.int64) * stride).to(dev)
    lens = torch.full((n,), ln, dtype=torch.int64, device=dev)
    out = [_i32(n, dev) for _ in range(2)]
    mism = [torch.full((n,), 0x5E, dtype=torch.uint8, device=dev) for _ in range(4)]
    cnt = [_i32(1, dev) for _ in range(4)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream
    L.create_strided(bc.CRC32C, buf, stride, ln, n, out[0], stream=s)
    L.verify_strided(bc.CRC32C, buf, stride, ln, n, out[0], mism[0], cnt[0], stream=s)
    with torch.cuda.stream(st):
        out[0][j:j + 1].bitwise_xor_(0x100)
    L.verify_strided(bc.CRC32C, buf, stride, ln, n, out[0], mism[1], cnt[1], stream=s)
    L.create_batch(bc.CRC32C, addrs, lens, out[1], n, ln, stream=s)
    L.verify_batch(bc.CRC32C, addrs, lens, out[1], mism[2], cnt[2], n, ln, computed=None, stream=s)
    with torch.cuda.stream(st):
        out[1][j:j + 1].bitwise_xor_(-(1 << 31))  # (int32 view of bit 31)
    L.verify_batch(bc.CRC32C, addrs, lens, out[1], mism[3], cnt[3], n, ln, computed=None, stream=s)
    st.synchronize()
    want = bc.crc_ranges(bc.CRC32C, host, np.arange(n, dtype=np.uint64) * np.uint64(stride), np.full(n, ln, dtype=np.uint64))
    flipped = want.copy()
    flipped[j] ^= 0x100
    assert np.array_equal(_u32(out[0]), flipped)
    flipped[j] = want[j] ^ np.uint32(1 << 31)
    assert np.array_equal(_u32(out[1]), flipped)
    for k in range(4):
        bad = {j} if k % 2 else set()
        assert int(_u32(cnt[k])[0]) == len(bad), (k, _u32(cnt[k]))
        assert set(np.flatnonzero(mism[k].cpu().numpy()).tolist()) == bad, k
        assert int(mism[k].cpu().numpy().max()) <= 1, k
    L.release_stream(st)


@pytest.mark.parametrize("ctype", [bc.CRC32C, bc.CRC32], ids=["crc32c", "crc32"])
def test_halves_to_serialized_records(hf, orc, dev, ctype):
    """create_batch of both halves of 256 ranges -> combine_batch -> finalize_batch ->
    serialize_batch: the 6-byte records decode to the finalized CRC of the whole ranges."""
    L = hf._lib
    h = sq.halves_chain(np.random.default_rng(0xD2))
    n = h["whole"].shape[0]
    arena = _up(h["arena"], dev)

    def ranges(r):
        return (torch.from_numpy((r[:, 0] + np.uint64(arena.data_ptr())).view(np.int64).copy()).to(dev),
                torch.from_numpy(r[:, 1].view(np.int64).copy()).to(dev))
    a1, l1 = ranges(h["first"])
    a2, l2 = ranges(h["second"])
    c1, c2 = _i32(n, dev), _i32(n, dev)
    ser = torch.full((6 * n,), 0x5E, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream
    L.create_batch(ctype, a1, l1, c1, n, int(h["first"][:, 1].max()), stream=s)
    L.create_batch(ctype, a2, l2, c2, n, int(h["second"][:, 1].max()), stream=s)
    L.combine_batch(ctype, c1, c2, l2, n, stream=s)
    L.finalize_batch(c1, n, stream=s)
    L.serialize_batch(ctype, c1, n, ser, stream=s)
    st.synchronize()
    want = ~bc.crc_ranges(ctype, h["arena"], h["whole"][:, 0], h["whole"][:, 1])
    assert np.array_equal(_u32(c1), want)
    got = ser.cpu().numpy().reshape(n, 6)
    for i in range(n):
        rc, (t, v), used = L.checksum_deserialize(got[i].tobytes())
        assert (rc, t, v, used) == (0, ctype, int(want[i]), 6), (i, rc, t, hex(v), hex(int(want[i])))
    L.release_stream(st)


@pytest.mark.parametrize("frame_stream", ["0", "1"])
def test_frames_computed_becomes_header(hf, orc, dev, opts, frame_stream):
    """3000 frames whose header checksum holds only the compressed bit: the first
    frame_verify_batch reports them all and computes calcSerde, a device copy moves `computed`
    into `checksum`, the second call must find every frame right."""
    L = hf._lib
    opts("frame_stream", frame_stream)
    inp = sq.frames_chain(np.random.default_rng(0xD3))
    n = inp["frames"].size
    arena, frames = _up(inp["arena"], dev), _up(inp["frames"], dev)
    snap = torch.empty_like(frames)
    cnt = [_i32(1, dev), _i32(1, dev)]
    cols = frames.view(torch.int32).view(n, 6)  # offset (2 words), size, checksum, computed, status
    torch.cuda.synchronize()
    st = torch.cuda.Stream(dev)
    L.frame_verify_batch(arena, frames, n, inp["max_size"], cnt[0], stream=st.cuda_stream)
    with torch.cuda.stream(st):
        snap.copy_(frames)
        cols[:, 3].copy_(cols[:, 4])
        cols[:, 4:6].fill_(0x5E5E5E5E)
    L.frame_verify_batch(arena, frames, n, inp["max_size"], cnt[1], stream=st.cuda_stream)
    st.synchronize()
    first, second = snap.cpu().numpy().view(bc.FRAME_DT), frames.cpu().numpy().view(bc.FRAME_DT)
    assert int(_u32(cnt[0])[0]) == n and (first["status"] == bc.CHECKSUM_MISMATCH).all()
    assert np.array_equal(first["computed"], inp["computed"])
    assert int(_u32(cnt[1])[0]) == 0
    assert not second["status"].any(), np.flatnonzero(second["status"])[:5]
    assert np.array_equal(second["computed"], inp["computed"]) and np.array_equal(second["checksum"], inp["computed"])
    for f in ("offset", "size"):
        assert np.array_equal(second[f], inp["frames"][f])
    L.release_stream(st)


@pytest.mark.parametrize("kind", ["wave", "split"])
def test_file_digest_from_device_made_checksums(hf, orc, dev, kind):
    """create_batch over every block's bytes, a device copy into the block table's checksum column,
    file_digest_batch: every file's value equals create_batch over the whole file, and the oracle."""
    L = hf._lib
    d = sq.digest_chain(np.random.default_rng(0xD4), kind)
    nb, nf = d["blocks"].size, d["file_off"].size - 1
    arena, blocks, file_off = _up(d["arena"], dev), _up(d["blocks"], dev), _up(d["file_off"], dev)

    def ranges(r):
        return (torch.from_numpy((r[:, 0] + np.uint64(arena.data_ptr())).view(np.int64).copy()).to(dev),
                torch.from_numpy(r[:, 1].view(np.int64).copy()).to(dev))
    ba, bl = ranges(d["block_ranges"])
    fa, fl = ranges(d["file_ranges"])
    bsum, fsum = _i32(nb, dev), _i32(nf, dev)
    out = torch.full((nf * bc.FILE_DT.itemsize,), 0x5E, dtype=torch.uint8, device=dev)
    cols = blocks.view(torch.int32).view(nb, 6)  # read_len, block_len (2 words each), checksum, type
    torch.cuda.synchronize()
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream
    L.create_batch(bc.CRC32C, ba, bl, bsum, nb, d["max_block_len"], stream=s)
    with torch.cuda.stream(st):
        cols[:, 4].copy_(bsum)
    L.file_digest_batch(blocks, file_off, out, nf, d["max_blocks"], stream=s)
    L.create_batch(bc.CRC32C, fa, fl, fsum, nf, d["max_file_len"], stream=s)
    st.synchronize()
    got = out.cpu().numpy().view(bc.FILE_DT)
    want = bc.crc_ranges(bc.CRC32C, d["arena"], d["file_ranges"][:, 0], d["file_ranges"][:, 1])
    assert np.array_equal(_u32(bsum), bc.crc_ranges(bc.CRC32C, d["arena"], d["block_ranges"][:, 0], d["block_ranges"][:, 1]))
    assert not got["status"].any(), np.flatnonzero(got["status"])[:5]
    assert (got["type"] == bc.CRC32C).all() and np.array_equal(got["length"], d["file_ranges"][:, 1])
    assert np.array_equal(got["value"], _u32(fsum)), "digest of the blocks' checksums != create over the whole files"
    assert np.array_equal(got["value"], want)
    L.release_stream(st)


# ---- e. one graph, many calls ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pipeline", ["default", "oneshot"])
def test_queue_in_one_graph(hf, orc, dev, opts, pipeline, mode):
    """The six updates and the scrub captured into ONE graph as the capture stream's first library
    calls (one-shot: six side-stream branches); replayed twice from restored chunks and records.
    The captured calls' memory is the graph's: live while it exists, gone with it."""
    L = hf._lib
    _set_pipeline(opts, pipeline)
    q = DeviceQueue(_scenario(orc, "rounds"), dev)
    f = FollowUp(q, dev)
    L.anomalies(0, reset=True)
    L.release_graph_scratch()
    base = L.graph_scratch_stats()
    cs = torch.cuda.Stream(dev)
    L.release_stream(cs)  # (pooled stream: no pair record, the captured calls are its first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        q.enqueue(L, mode, cs)
        L.scrub_batch(q.ctype, f.scrub.data_ptr(), q.scn.n, f.fu["max_len"], f.count.data_ptr(), stream=cs.cuda_stream)
    torch.cuda.synchronize()
    owned = L.graph_scratch_stats()
    assert owned["live"] > base["live"] and owned["live_bytes"] > base["live_bytes"], (base, owned)
    for rep in range(2):
        g.replay()
        torch.cuda.synchronize()
        q.check()
        scrub = f.scrub.cpu().numpy().view(bc.SCRUB_DT)
        assert int(_u32(f.count)[0]) == 0 and not scrub["status"].any(), (rep, np.flatnonzero(scrub["status"]))
        assert np.array_equal(scrub["computed"], f.fu["computed"]), rep
        q.restore()
        f.restore()
    assert L.anomalies(0)["count"] == 0
    del g
    torch.cuda.synchronize()
    L.release_graph_scratch()
    end = L.graph_scratch_stats()
    assert end["dead"] == 0 and end["live"] == base["live"], (base, end)
    L.release_stream(cs)
