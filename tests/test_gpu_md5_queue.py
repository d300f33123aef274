"""hf3fs_crc_md5_batch where tests/test_gpu_md5.py stops: file counts at which the bucketing pass's
shares carry over several tiles and prep's grid strides, batches that occupy many buckets at once,
the reference loop (INIT, updates, FINAL with the state carried on the device) queued without waits,
behind the kernel that wrote the bytes, through one pair buffer with other entry points, from two
host threads, as one graph, and from seeded states whose totals need the bit length's upper word.

The builders, the runs and the checkers are tests/md5_queue.py's (held to a stand-in library by
tests/test_md5_queue_model.py): every digest is compared with hashlib.md5 of the file's bytes per
file index, every 96-byte state with md5_cases.State, outputs start from a sentinel between guard
bytes.  Unless a test says otherwise it runs under the four settings of md5_stage x md5_sort.
"""
import functools
import threading

import numpy as np
import pytest

import batch_cases as bc
import md5_cases as mc
import md5_queue as mq
import update_footprint as fp

torch = pytest.importorskip("torch")

import test_gpu_batch_contexts as contexts  # noqa: E402
import test_gpu_stream_queue as stream_queue  # noqa: E402
import test_gpu_sync_plan as sync_plan  # noqa: E402

pytestmark = pytest.mark.gpu
ROOMY = 256 << 10  # the granule of a pair's call buffer (roomy_words, hf3fs_crc_api.hip)
SEED = 0x5EED


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(params=mq.MODES, ids=[f"stage{s}-sort{o}" for s, o in mq.MODES])
def mode(request, opts):
    stage, sort = request.param
    opts("md5_stage", stage)
    opts("md5_sort", sort)
    return request.param


class Buf:
    def __init__(self, t):
        self.t, self.addr = t, t.data_ptr()


class Gpu:
    """The backend of md5_queue's runs: buffers in HBM, the calls on one side stream."""

    def __init__(self, hf, dev, stream=None):
        self.hf, self.dev = hf, dev
        self.stream = stream or torch.cuda.Stream(dev)

    def upload(self, array):
        return Buf(torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).to(self.dev))

    def write(self, buf, array, at=0):
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()
        buf.t[at:at + raw.size].copy_(torch.from_numpy(raw))

    def read(self, buf):
        return buf.t.cpu().numpy()

    def ready(self):
        torch.cuda.synchronize()  # uploads ran on the current stream: they are done before the side stream starts

    def wait(self):
        self.stream.synchronize()

    def md5_batch(self, segs, off, n, n_segs, out=0, state=0, flags=mq.BOTH):
        self.hf.md5_batch(segs or None, off, n, n_segs, out=out or None, state=state or None, flags=flags,
                          stream=self.stream)


@pytest.fixture
def be(hf, dev):
    """A backend on a stream whose pair record is released before and after the test."""
    g = Gpu(hf, dev)
    hf._lib.release_stream(g.stream)
    yield g
    torch.cuda.synchronize()
    hf._lib.release_stream(g.stream)


# ---- A. large counts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mq.COUNTS)
def test_tiny_files_at_large_counts(be, mode, n):
    """Files of 0..130 bytes: from 16,385 on every share of the count and scatter passes carries
    its bucket numbers over two or more tiles, about half the shares or fewer are empty and one
    ends in a partial tile; at 2^20 + 300 prep's grid is capped and strides
    (tests/test_md5_queue_model.py asserts the geometry).  16,384 is the last single-tile count."""
    mq.run_one_shot(be, mq.tiny(n), f"tiny files x {n}")


@pytest.mark.parametrize("n", mq.SPREAD_COUNTS)
def test_spread_files_occupy_many_buckets(be, mode, n):
    """A hole and 1..200 real bytes per file, in either order: 51 or 52 of the 256 buckets are
    occupied, 8 or more in 128 (219) of the shares, one file's hole is 2 MiB + 17 bytes."""
    mq.run_one_shot(be, mq.spread(n), f"spread files x {n}")


def test_two_calls_at_70001(be, mode):
    """INIT with 0..63 bytes per file, FINAL with the spread files behind it, no wait between: all
    70,001 states are (H0, length, bytes) byte for byte after both calls, every digest is hashlib's."""
    n = mq.TWO_CALL_COUNT
    mq.run_two_calls(be, mq.head(n), mq.spread(n), mq.two_call_digests(n), f"two calls x {n}")


# ---- B. the reference loop queued without waits ---------------------------------------------------------
@pytest.mark.parametrize("n_bytes", [130, 4097])
def test_loop_queued_without_waits(be, mode, n_bytes):
    """INIT, update, update, FINAL with all records resident and no host step between the calls;
    the twin that waits after every call leaves the same bytes."""
    loop = mq.four_calls(n_bytes)
    queued = mq.run_loop(be, loop, f"queued loop of {n_bytes} bytes")
    twin = mq.run_loop(be, loop, f"waiting twin of {n_bytes} bytes", wait_each=True)
    assert queued == twin, "the queue and its twin leave different bytes"


GROWTH = (64, 5000, 64, 20000)


def test_loops_of_growing_file_counts(hf, be, mode):
    """Four loops of 64, 5,000, 64 and 20,000 files queued on a pair that starts without a buffer:
    the buffer grows with the first three loops still queued, and a second pass allocates nothing."""
    L = hf._lib
    assert L.md5_scratch_bytes(5000) <= ROOMY < L.md5_scratch_bytes(20000)
    runs = [mq.LoopRun(be, mq.four_calls(130, n, seed=20 + k)) for k, n in enumerate(GROWTH)]
    be.ready()
    start = L.pair_scratch_stats(be.stream)
    assert start["call_bytes"] == 0
    for r in runs:
        r.queue()
    be.wait()
    first = L.pair_scratch_stats(be.stream)
    for n, r in zip(GROWTH, runs):
        r.check(f"loop of {n} files")
        r.reset()
    assert 1 <= first["allocations"] - start["allocations"] <= 2 and first["call_bytes"] > ROOMY, (start, first)
    be.ready()
    for r in runs:
        r.queue()
    be.wait()
    second = L.pair_scratch_stats(be.stream)
    for n, r in zip(GROWTH, runs):
        r.check(f"loop of {n} files, second pass")
    assert second == first, (first, second)


# ---- C. behind the kernel that wrote the bytes; one pair buffer for several entry points -----------------
CHUNKS, CHUNK_LEN = 64, (12 << 10) + 8


@functools.lru_cache(maxsize=None)
def _synth_files(orc):
    """200 files of 1..5 segments cut at unaligned positions from 64 synthetic chunks laid end to
    end; every fourth file's first segment lies across a chunk boundary."""
    arena = np.concatenate([orc.fill_synth(CHUNK_LEN, SEED, 11 + i) for i in range(CHUNKS)])
    arena.setflags(write=False)
    rng = np.random.default_rng(31)
    files = []
    for f in range(200):
        segs = []
        for k in range(int(rng.integers(1, 6))):
            n = int(rng.integers(0, 3001))
            at = int(rng.integers(0, arena.size - n + 1))
            if f % 4 == 0 and k == 0:
                n = max(n, 2)
                at = int(rng.integers(1, CHUNKS)) * CHUNK_LEN - int(rng.integers(1, n))
            segs.append((at, n))
        files.append(segs)
    batch = mq.Batch.of_files(arena, files)
    cross = (batch.seg_at // CHUNK_LEN != (batch.seg_at + batch.seg_len.astype(np.int64) - 1) // CHUNK_LEN) & (batch.seg_len > 0)
    assert cross.sum() >= 50 and len(set((batch.seg_at % 16).tolist())) == 16
    return batch


@pytest.mark.parametrize("where", ["same_stream", "across_event"])
def test_behind_fill_synth(hf, orc, dev, be, mode, where):
    """fill_synth writes 64 chunks on the stream and md5_batch hashes files cut from them directly
    behind it (or on a second stream behind an event), with no host wait: the bytes are the oracle's."""
    batch = _synth_files(orc)
    chunks = Buf(torch.zeros(CHUNKS * CHUNK_LEN, dtype=torch.uint8, device=dev))
    second = Gpu(hf, dev)
    run = mq.OneShot(second if where == "across_event" else be, batch, arena=chunks)
    be.ready()
    hf._lib.fill_synth(chunks.t, CHUNK_LEN, CHUNK_LEN, CHUNKS, SEED, 11, stream=be.stream)
    if where == "across_event":
        ev = torch.cuda.Event()
        ev.record(be.stream)
        second.stream.wait_event(ev)
    run.queue()
    run.be.wait()
    run.check(f"behind fill_synth, {where}")
    assert np.array_equal(chunks.t.cpu().numpy(), batch.arena)
    hf._lib.release_stream(second.stream)


@pytest.mark.parametrize("update_mode", [0, 1])
def test_behind_queued_updates(hf, orc, dev, be, mode, update_mode):
    """Six update_batch calls on 32 chunks and, directly behind them, the MD5 of every chunk up to
    its final size: the bytes are the scenario's image after the last round."""
    L = hf._lib
    scn = stream_queue._scenario(orc, "rounds")
    q = stream_queue.DeviceQueue(scn, dev)
    image = scn.image_after(len(scn.rounds) - 1)
    assert any(scn.sizes) and max(scn.sizes) <= scn.max_len
    batch = mq.Batch.of_files(image, [[(scn.lay.bases[c], scn.sizes[c])] for c in range(scn.n)])
    run = mq.OneShot(be, batch, arena=Buf(q.arena))
    be.ready()
    q.enqueue(L, update_mode, be.stream)
    run.queue()
    be.wait()
    run.check(f"behind six updates, mode {update_mode}")
    q.check()


@functools.lru_cache(maxsize=None)
def _ragged(n):
    lay = mc.ragged_layout(n)
    arena = lay.arena()
    arena.setflags(write=False)
    return mq.Batch.of_files(arena, lay.files)


def test_md5_shares_the_pair_buffer(hf, orc, dev, cus, be, mode, opts):
    """md5_batch of 1,000 ragged files and of 200 on one stream, and between the two a one-shot
    update_batch, a sync_plan of (5000, 5000) and a verify_blocks with library scratch: each call
    carves the pair's one call buffer its own way and starts on what another left there.  Forward,
    reversed without a new allocation, and reversed on poisoned scratch."""
    L = hf._lib
    stream_queue._set_pipeline(opts, "oneshot")
    q = stream_queue.DeviceQueue(stream_queue._scenario(orc, "rounds", fp.CRC32C, 1), dev)
    tables = sync_plan._random(5000, 5000, 51)
    box = sync_plan.Box(dev, tables[0].size, tables[1].size)
    box.load(tables[0], tables[1])
    name = "verify_blocks_scratch"
    inp, ref = contexts.timeline(name, cus)[0]
    blocks = contexts.OnDevice(bc.CASES[name], inp, dev)
    md5s = [mq.OneShot(be, _ragged(1000)), mq.OneShot(be, _ragged(200))]
    others = [lambda: q.call(L, 0, 1, be.stream),
              lambda: box.plan(hf, tables[2], tables[3], stream=be.stream),
              lambda: blocks.run(L, inp, be.stream.cuda_stream)]
    forward = [md5s[0].queue] + others + [md5s[1].queue]
    L.anomalies(0, reset=True)
    be.ready()
    allocs = None
    for what, order, poison in (("in order", forward, 0), ("reversed", forward[::-1], 0),
                                ("reversed, poisoned", forward[::-1], 0xA5A5A5A5)):
        if poison:
            opts("poison", poison)
        for call in order:
            call()
        be.wait()
        if poison:
            opts("poison", 0)
        now = L.pair_scratch_stats(be.stream)["allocations"]
        if what == "reversed":
            assert now == allocs, f"the reversed queue allocated: {allocs} -> {now}"
        allocs = now
        for m in md5s:
            m.check(f"{m.batch.n} ragged files ({what})")
            m.reset()
        sync_plan._check(box.fetch(), tables[0], tables[1], tables[4], f"sync_plan ({what})")
        contexts.check(blocks, inp, ref, f"{name} ({what})")
        q.check()
        q.restore()
        box.load(tables[0], tables[1])
        blocks.load(inp)
    a = L.anomalies(0)
    assert a["count"] == 0 and a["kinds"] == 0, a


def test_two_threads_two_streams(hf, dev, mode):
    """Two host threads, each with its own stream and files, start together and queue the four-call
    loop 20 times: every digest and state is exact, and each (stream, thread) pair has its own buffer."""
    L = hf._lib
    loops = [mq.four_calls(4097, 48, seed=41), mq.four_calls(130, 20000, seed=42)]
    backs = [Gpu(hf, dev) for _ in loops]
    for b in backs:
        L.release_stream(b.stream)
    runs = [mq.LoopRun(b, loop) for b, loop in zip(backs, loops)]
    torch.cuda.synchronize()
    errors, call_bytes = [], [None, None]
    gate = threading.Barrier(2)

    def work(k):
        try:
            torch.cuda.set_device(dev)
            gate.wait(timeout=30)
            for _ in range(20):
                runs[k].queue()
            backs[k].wait()
            call_bytes[k] = L.pair_scratch_stats(backs[k].stream)["call_bytes"]
            L.release_stream(backs[k].stream)
        except Exception as e:  # noqa: BLE001
            errors.append(f"thread {k}: {type(e).__name__}: {e}")

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, r in enumerate(runs):
        r.check(f"thread {k}")
    assert call_bytes == [L.md5_scratch_bytes(48), L.md5_scratch_bytes(20000)] and call_bytes[0] < call_bytes[1]


# ---- D. the whole loop as one graph -----------------------------------------------------------------------
@pytest.mark.parametrize("poison", [0, 0xA5A5A5A5], ids=["plain", "poisoned"])
def test_loop_in_one_graph(hf, dev, mode, opts, poison):
    """INIT, update, update, FINAL captured into one graph as the capture stream's first library
    calls (poisoned: the fill of each call's scratch is part of the graph).  Between the replays the
    bytes are rewritten in place, one d_file_off entry of the second call moves a segment to the
    next file, and d_state is filled with 0xA5, which INIT must not read.  The captured calls'
    memory is the graph's: live while it exists, gone with it."""
    L = hf._lib
    loop = mq.four_calls(4097)
    L.release_graph_scratch()
    base = L.graph_scratch_stats()
    cs = torch.cuda.Stream(dev)
    L.release_stream(cs)
    be = Gpu(hf, dev, cs)
    run = mq.LoopRun(be, loop)
    torch.cuda.synchronize()
    if poison:
        opts("poison", poison)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        run.queue()
    if poison:
        opts("poison", 0)
    torch.cuda.synchronize()
    owned = L.graph_scratch_stats()
    assert owned["live"] > base["live"] and owned["live_bytes"] > base["live_bytes"], (base, owned)
    g.replay()
    torch.cuda.synchronize()
    run.check("replay 0")
    arena2 = np.random.default_rng(99).integers(0, 256, loop.arena.size, dtype=np.uint8)
    moved, f, off = mq.moved_boundary(loop, arena2)
    assert moved.digests[16 * f:16 * f + 32] != loop.digests[16 * f:16 * f + 32] and moved.lengths[f] != loop.lengths[f]
    be.write(run.arena, arena2)
    be.write(run.placed[1][2][2], off)
    run.reset()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    run.check("replay 1", loop=moved)
    del g
    torch.cuda.synchronize()
    L.release_graph_scratch()
    end = L.graph_scratch_stats()
    assert end["dead"] == 0 and end["live"] == base["live"], (base, end)
    L.release_stream(cs)


# ---- E. totals past 2^32 bits ---------------------------------------------------------------------------------
def test_seeded_states_with_large_totals(be, mode):
    """States seeded with totals around 2^29 (the bit length's upper word becomes non-zero), 2^32,
    2^61 and 2^64, random h and a consistent tail, and the states of hole-only files of 2^29 - 1 ..
    2^32 + 5 bytes whose digests hashlib knows: FINAL alone, an update of 0..200 bytes and FINAL,
    and the update alone, after which total holds the sum as a 64-bit value (it wraps at 2^64, as
    the bit length does)."""
    mq.run_seeded(be, mq.seeded(), "seeded states")
