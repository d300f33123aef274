"""Ordered, versioned, copy-on-write and chunk-engine updates queued back to back on one stream,
one wait at the end (tests/update_queue.py).

tests/test_gpu_stream_queue.py queues hf3fs_crc_update_batch; the per-entry-point files put every
call between two host synchronizes.  Queued, these four calls meet what a synchronized call never
does: the pinned hint word is read while the call that writes it is still running (so the plan is
the ticketed apply, or a one-shot grid sized from an OLDER call's pieces per IO), the side stream's
finalize of call k is ordered in front of call k + 1 by the join alone, and the pair buffer that
holds call k's control words is carved another way -- or regrown -- for call k + 1.

All tensors are made and filled first (one torch.cuda.synchronize()), the library calls go onto a
fresh stream with nothing between them, one wait follows, and only then is anything copied back:

  a. every queue kind (ordered x5, versioned x5, cow x4, engine x4, mixed x8) against the models
     and, byte for byte, against its twin that synchronizes after every call
  b. a second pass on the hints the first pass left, then a third from cold hints
  c. density swing: piece-poor and piece-rich calls alternating (update_batch, ordered, cow)
  d. growth: the pair buffer regrown with the first call still queued (ordered, versioned)
  e. scrub and read-result batches directly behind the last update, and across an event; behind
     the versioned queue also sync_plan -> sync_scrub_fill -> scrub_batch
  f. two threads, each with its own stream and chunk set, at the same time
  g. the mixed queue captured into one graph

All comparisons are bit-exact against the models; hf3fs_crc_anomalies stays empty."""
import functools
import threading

import numpy as np
import pytest

import batch_cases as bc
import cow_cases as cc
import stream_queue as sq
import update_footprint as fp
import update_queue as uq

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
LINE = 16 << 10
BIG = 128 << 10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _built(orc, kind, max_len=BIG, ctype=fp.CRC32C):
    """Built once and shared: the expected images do not depend on how the calls are queued."""
    return {"ordered": lambda: uq.chain_queue(orc, max_len, ctype=ctype),
            "versioned": lambda: uq.chain_queue(orc, max_len, versioned=True),
            "cow": lambda: uq.cow_queue(orc, max_len, ctype=ctype),
            "engine": lambda: uq.engine_queue(orc, max_len),
            "mixed": lambda: uq.mixed_queue(orc, max_len),
            "mixed_b": lambda: uq.mixed_queue(orc, max_len, seed=0x313E),
            "density_batch": lambda: uq.density_queue(orc, uq.BATCH),
            "density_ordered": lambda: uq.density_queue(orc, uq.ORDERED),
            "density_cow": lambda: uq.cow_density_queue(orc),
            "growth_ordered": lambda: uq.growth_queue(orc),
            "growth_versioned": lambda: uq.growth_queue(orc, versioned=True)}[kind]()


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def _set_pipeline(opts, pipeline):
    """"default": no switch (the pair's hint decides per call); "fused"; "oneshot": the three-pass
    pipeline with the one-shot apply (its finalize on the side stream); "ticketed"; "piece4": default
    with 4 KiB pieces, so a piece-rich call has the most pieces per IO."""
    if pipeline == "fused":
        opts("update_pipeline", "fused")
    elif pipeline == "piece4":
        opts("apply_piece_kib", 4)
    elif pipeline != "default":
        opts("update_pipeline", "unfused")
        opts("apply_grid", 1 if pipeline == "oneshot" else 0)


class _Resident:
    """One arena on a 16 KiB line; every call's payloads and buffers resident at once."""

    def _arena(self, img, dev):
        self.raw = torch.empty(img.size + LINE, dtype=torch.uint8, device=dev)
        lift = (-self.raw.data_ptr()) % LINE
        self.arena = self.raw[lift:lift + img.size]
        self.arena0 = _up(img, dev)

    def enqueue(self, L, mode, st, sync_each=False):
        for k in range(self.ncalls):
            self.call(L, k, mode, st)
            if sync_each:
                st.synchronize()


class DeviceQueue(_Resident):
    """An update_queue.Queue or EngineQueue on the device."""

    def __init__(self, q, dev):
        self.q, self.ncalls = q, len(q.calls)
        self._arena(q.arena0, dev)
        self.pays = [_up(c.pay, dev) for c in q.calls]
        self.sent = [q.buffers(k, self.arena.data_ptr(), self.pays[k].data_ptr()) for k in range(self.ncalls)]
        self.bufs0 = [{n: _up(b, dev) for n, b in s.items() if b is not None} for s in self.sent]
        self.bufs = [{n: torch.empty_like(b) for n, b in s.items()} for s in self.bufs0]
        self.restore()

    def restore(self):
        self.arena.copy_(self.arena0)
        for b, b0 in zip(self.bufs, self.bufs0):
            for n in b:
                b[n].copy_(b0[n])
        torch.cuda.synchronize()

    def call(self, L, k, mode, st):
        c, q, b = self.q.calls[k], self.q, self.bufs[k]
        rec, s = b["rec"].data_ptr() + fp.REC_GUARD, st.cuda_stream
        if c.entry == uq.ORDERED:
            L.update_ordered(q.ctype, rec, c.n, q.max_len, c.max_rounds, mode=mode, info=b["info"].data_ptr(), stream=s)
        elif c.entry == uq.VERSIONED:
            L.update_versioned(q.ctype, rec, b["ver"].data_ptr() + uq.VER_GUARD, c.n, q.max_len, c.max_rounds, mode=mode,
                               info=b["info"].data_ptr(), stream=s)
        elif c.entry == uq.BATCH:
            L.update_batch(q.ctype, rec, c.n, q.max_len, mode=mode, stream=s)
        elif c.entry == uq.COW:
            L.update_cow(q.ctype, rec, b["dst"].data_ptr() + cc.DST_GUARD, c.n, q.max_len, mode=mode, stream=s)
        else:
            L.update_engine(fp.CRC32C, rec, b["jr"].data_ptr() + uq.JOB_GUARD, c.n, q.max_len, c.max_rounds, mode=mode,
                            info=b["info"].data_ptr(), stream=s)

    def check(self):
        arena = self.arena.cpu().numpy()
        pays = [p.cpu().numpy() for p in self.pays]
        got = [{n: (b[n].cpu().numpy().view(np.uint32) if n == "info" else b[n].cpu().numpy()) if n in b else None
                for n in s} for b, s in zip(self.bufs, self.sent)]
        if isinstance(self.q, uq.EngineQueue):
            uq.check_engine_queue(self.q, self.arena.data_ptr(), arena, pays, got, self.sent)
        else:
            uq.check_queue(self.q, arena, pays, got, self.sent)
        return [arena] + [g[n] for g in got for n in sorted(g) if g[n] is not None]


class DeviceCowQueue(_Resident):
    """An update_queue.CowQueue on the device: one record and one destination buffer per call."""

    def __init__(self, q, dev):
        self.q, self.ncalls = q, len(q.scns)
        self._arena(q.arena0, dev)
        self.pays = [_up(s.payload_image(0), dev) for s in q.scns]
        a = self.arena.data_ptr()
        self.sent = [s.record_buffer(a, self.pays[k].data_ptr()) for k, s in enumerate(q.scns)]
        self.sent_dst = [s.dst_buffer(a) for s in q.scns]
        self.recs0, self.dsts0 = [_up(b, dev) for b in self.sent], [_up(b, dev) for b in self.sent_dst]
        self.recs, self.dsts = [torch.empty_like(b) for b in self.recs0], [torch.empty_like(b) for b in self.dsts0]
        self.restore()

    def restore(self):
        self.arena.copy_(self.arena0)
        for x, x0 in zip(self.recs + self.dsts, self.recs0 + self.dsts0):
            x.copy_(x0)
        torch.cuda.synchronize()

    def call(self, L, k, mode, st):
        q = self.q
        L.update_cow(q.ctype, self.recs[k].data_ptr() + fp.REC_GUARD, self.dsts[k].data_ptr() + cc.DST_GUARD, q.n, q.max_len,
                     mode=mode, stream=st.cuda_stream)

    def check(self):
        arena = self.arena.cpu().numpy()
        recs, dsts = [r.cpu().numpy() for r in self.recs], [d.cpu().numpy() for d in self.dsts]
        uq.check_cow_queue(self.q, arena, [p.cpu().numpy() for p in self.pays], recs, self.sent, dsts, self.sent_dst)
        return [arena] + recs + dsts


class DeviceMixed(_Resident):
    """update_queue.mixed_queue: the replica calls and the engine call in the plan's order."""

    def __init__(self, m, dev):
        self.m, self.ncalls = m, len(m.plan)
        self.part = {"q": DeviceQueue(m.q, dev), "e": DeviceQueue(m.e, dev)}

    def restore(self):
        for p in self.part.values():
            p.restore()

    def call(self, L, k, mode, st):
        which, j = self.m.plan[k]
        self.part[which].call(L, j, mode, st)

    def check(self):
        return self.part["q"].check() + self.part["e"].check()


def _resident(built, dev):
    if isinstance(built, uq.Mixed):
        return DeviceMixed(built, dev)
    return DeviceCowQueue(built, dev) if isinstance(built, uq.CowQueue) else DeviceQueue(built, dev)


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"{what}: {'the chunk arena' if i == 0 else f'buffer {i}'} differs between the " \
                                     f"queue and its synchronized twin"


def _fresh_stream(L, dev):
    st = torch.cuda.Stream(dev)
    L.release_stream(st)  # (streams come from a pool: whatever an earlier test left on this one goes)
    return st


# ---- a. the queue against its synchronized twin ------------------------------------------------------
def _rows():
    rows = []
    for max_len in (BIG, 512):
        for kind in ("ordered", "versioned", "mixed"):
            rows += [(kind, p, m, max_len, fp.CRC32C) for p in ("default", "fused", "oneshot", "ticketed") for m in (0, 1)]
        for kind in ("cow", "engine"):  # (no fused and no ticketed form)
            rows += [(kind, p, m, max_len, fp.CRC32C) for p in ("default", "oneshot") for m in (0, 1)]
    rows += [(kind, "default", m, BIG, fp.CRC32) for kind in ("ordered", "cow") for m in (0, 1)]
    return rows


ROWS = _rows()
ROW_IDS = [f"{k}-{p}-mode{m}-{ml}-{'crc32c' if t == fp.CRC32C else 'crc32'}" for k, p, m, ml, t in ROWS]


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_queue_equals_its_synchronized_twin(hf, orc, dev, opts, row):
    """The calls of one queue with no host step between them, then the twin with a synchronize after
    each call: both must leave the models' bytes and records, and the same ones.  In "default" the
    hint decides, so the queue and its twin take different plans by construction."""
    kind, pipeline, mode, max_len, ctype = row
    L = hf._lib
    _set_pipeline(opts, pipeline)
    d = _resident(_built(orc, kind, max_len, ctype), dev)
    L.anomalies(0, reset=True)
    st = _fresh_stream(L, dev)
    d.enqueue(L, mode, st)
    st.synchronize()
    queued = d.check()
    d.restore()
    d.enqueue(L, mode, st, sync_each=True)
    twin = d.check()
    _same(queued, twin, ROW_IDS[ROWS.index(row)])
    a = L.anomalies(0)
    assert a["count"] == 0, a
    L.release_stream(st)


# ---- b. a second pass on warm hints ---------------------------------------------------------------------
def _three_passes(L, d, mode, st, what):
    """Cold, then on the hints (and the pair buffer) the first pass left -- every call now plans on
    a hint another call wrote -- then cold again after release_stream."""
    d.enqueue(L, mode, st)
    st.synchronize()
    first = d.check()
    d.restore()
    before = L.pair_scratch_stats(st)
    d.enqueue(L, mode, st)
    st.synchronize()
    after = L.pair_scratch_stats(st)
    _same(first, d.check(), f"{what}: second pass")
    assert after["allocations"] == before["allocations"], (before, after)
    d.restore()
    L.release_stream(st)
    d.enqueue(L, mode, st)
    st.synchronize()
    _same(first, d.check(), f"{what}: third pass")
    d.restore()
    return first, before


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["ordered", "versioned", "cow", "engine", "mixed"])
def test_second_pass_on_warm_hints(hf, orc, dev, kind, mode):
    L = hf._lib
    d = _resident(_built(orc, kind), dev)
    L.anomalies(0, reset=True)
    st = _fresh_stream(L, dev)
    _three_passes(L, d, mode, st, kind)
    assert L.anomalies(0)["count"] == 0
    L.release_stream(st)


# ---- c. density swing -------------------------------------------------------------------------------------
DENSITY = [(e, p, m) for e in ("batch", "ordered", "cow")
           for p in (("default", "oneshot", "piece4") if e == "cow" else ("default", "fused", "oneshot", "ticketed", "piece4"))
           for m in (0, 1)]  # (a)'s pipeline x mode product (copy-on-write has no fused and no ticketed form), and 4 KiB pieces


@pytest.mark.parametrize("entry,pipeline,mode", DENSITY)
def test_density_swing(hf, orc, dev, opts, entry, pipeline, mode):
    """Six calls of 64 IOs on 64 chunks of 128 KiB alternating between truncates / 1-byte writes and
    writes of the whole chunk: a grid sized from the previous call's pieces per IO is far too small
    for a rich call (~1000 pieces at 8 KiB, ~2000 at 4 KiB against 64 + 3 %) and far too large for
    a poor one.  Queue, twin, and the passes on warm and cold hints."""
    L = hf._lib
    _set_pipeline(opts, pipeline)
    d = _resident(_built(orc, f"density_{entry}"), dev)
    L.anomalies(0, reset=True)
    st = _fresh_stream(L, dev)
    first, _ = _three_passes(L, d, mode, st, f"density {entry}")
    d.enqueue(L, mode, st, sync_each=True)
    _same(first, d.check(), f"density {entry} {pipeline}")
    assert L.anomalies(0)["count"] == 0
    L.release_stream(st)


# ---- d. growth ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["ordered", "versioned"])
def test_queue_regrows_pair_buffer(hf, orc, dev, kind, mode):
    """Calls of 8, 2048, 32, 2048, 512, 2048 jobs on 4 KiB chunks: the second call needs more than
    the first one's allocation, so pair_buffer has to wait for the stream, free and reallocate with
    the first call still queued -- its control words, round array and chunk hash table live there."""
    L = hf._lib
    q = _built(orc, f"growth_{kind}")
    d = _resident(q, dev)
    assert [c.n for c in q.calls] == list(uq.GROWTH_COUNTS)
    need = L.update_versioned_scratch_bytes if kind == "versioned" else L.update_ordered_scratch_bytes
    small, large = (need(q.calls[k].n, q.max_len, q.calls[k].max_rounds, mode=mode) for k in (0, 1))
    assert 0 < small <= uq.FIRST_ALLOCATION < large, (small, large)
    L.anomalies(0, reset=True)
    st = _fresh_stream(L, dev)
    start = L.pair_scratch_stats(st)
    assert start["call_bytes"] == 0
    d.enqueue(L, mode, st)
    L.stream_wait(st)
    d.check()
    d.restore()
    before = L.pair_scratch_stats(st)
    assert before["allocations"] >= start["allocations"] + 2 and before["call_bytes"] >= large, (start, before)
    d.enqueue(L, mode, st)
    L.stream_wait(st)
    after = L.pair_scratch_stats(st)
    d.check()
    assert after["allocations"] == before["allocations"], (before, after)
    assert L.anomalies(0)["count"] == 0
    L.release_stream(st)


# ---- e. followers ---------------------------------------------------------------------------------------------
class FollowUp:
    """Scrub and read-result records over every chunk's final state, where the queue left it."""

    def __init__(self, d, dev):
        q = d.q
        self.n, self.ctype = q.n, q.ctype
        self.fu = sq.followup_records(q, d.arena.data_ptr())
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
        L.scrub_batch(self.ctype, self.scrub.data_ptr(), self.n, self.fu["max_len"], self.count.data_ptr(), stream=st.cuda_stream)
        L.read_result_batch(self.ctype, self.read.data_ptr(), self.n, self.fu["max_len"], stream=st.cuda_stream)

    def check(self):
        sq.check_followup(self.fu, self.scrub.cpu().numpy().view(bc.SCRUB_DT), self.read.cpu().numpy().view(bc.READ_DT),
                          self.count.cpu().numpy().view(np.uint32)[0])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("across", [False, True], ids=["same_stream", "across_event"])
@pytest.mark.parametrize("kind", ["ordered", "versioned", "cow"])
def test_records_behind_the_last_update(hf, orc, dev, opts, kind, across, mode):
    """scrub_batch and read_result_batch over the final chunks -- for the copy-on-write queue at the
    places the chunks moved to -- directly behind the last update with no host step: on the same
    stream (default pipeline), and on a second stream across an event (one-shot: the side stream's
    finalize of every call must be in front of that event)."""
    L = hf._lib
    _set_pipeline(opts, "oneshot" if across else "default")
    d = _resident(_built(orc, kind), dev)
    f = FollowUp(d, dev)
    checked = int(np.count_nonzero(f.fu["types"] != fp.NONE))
    assert checked >= d.q.n // 2, checked
    L.anomalies(0, reset=True)
    st = _fresh_stream(L, dev)
    if across:
        st2, ev = _fresh_stream(L, dev), torch.cuda.Event()
        d.enqueue(L, mode, st)
        ev.record(st)
        st2.wait_event(ev)
        f.enqueue(L, st2)
        st2.synchronize()
        L.release_stream(st2)
    else:
        d.enqueue(L, mode, st)
        f.enqueue(L, st)
        st.synchronize()
    f.check()
    d.check()
    assert L.anomalies(0)["count"] == 0
    L.release_stream(st)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("across", [False, True], ids=["same_stream", "across_event"])
def test_resync_plan_behind_the_versioned_queue(hf, orc, dev, opts, across, mode):
    """hf3fs_crc_sync_plan -> hf3fs_crc_sync_scrub_fill -> hf3fs_crc_scrub_batch directly behind the
    last versioned update, the local table taken from the model's final state: the exact plan and
    lists, and the scrub of every forwarded chunk finds the stored checksum over the bytes the queue
    left -- zero mismatches."""
    import sync_cases as sc
    L = hf._lib
    _set_pipeline(opts, "oneshot" if across else "default")
    q = _built(orc, "versioned")
    d = _resident(q, dev)
    local, remote, want = uq.sync_tables(q)
    n, nr, guard, canary = local.size, remote.size, 64, 0x7C7C7C7C
    d_local, d_remote = _up(local, dev), _up(remote, dev)
    addrs = torch.from_numpy(d.arena.data_ptr() + np.array(q.lay.bases, dtype=np.int64)).to(dev)
    write = torch.full((n + guard,), canary, dtype=torch.int32, device=dev)
    remove = torch.full((nr + guard,), canary, dtype=torch.int32, device=dev)
    info = torch.full((16 + guard,), canary, dtype=torch.int32, device=dev)
    scrub = torch.full((n * bc.SCRUB_DT.itemsize + 64,), 0xEE, dtype=torch.uint8, device=dev)
    count = torch.full((1,), 77, dtype=torch.int32, device=dev)
    L.anomalies(0, reset=True)
    torch.cuda.synchronize()
    st = _fresh_stream(L, dev)
    d.enqueue(L, mode, st)
    last = st
    if across:
        last, ev = _fresh_stream(L, dev), torch.cuda.Event()
        ev.record(st)
        last.wait_event(ev)
    L.sync_plan(d_local, n, d_remote, nr, uq.SYNC_CHAIN_VER, info, write=write, remove=remove, stream=last.cuda_stream)
    L.sync_scrub_fill(d_local, addrs, write, info, n, scrub, stream=last.cuda_stream)
    L.scrub_batch(q.ctype, scrub, n, q.max_len, count, stream=last.cuda_stream)
    last.synchronize()
    d.check()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    assert dict(zip(sc.INFO, (int(x) for x in u32(info)[:16]))) == want.info
    assert (u32(info)[16:] == canary).all()
    assert u32(write)[:len(want.write)].tolist() == want.write and (u32(write)[len(want.write):] == canary).all()
    assert (u32(remove) == canary).all() and want.remove == []
    for name, t, sent, cls, peer in (("local", d_local, local, want.lclass, want.lpeer),
                                     ("remote", d_remote, remote, want.rclass, want.rpeer)):
        exp = sent.copy()
        exp["out_class"], exp["out_peer"] = np.asarray(cls, dtype=np.uint8), np.asarray(peer, dtype=np.uint32)
        assert t.cpu().numpy().tobytes() == exp.tobytes(), f"{name} table"
    assert int(count.item()) == 0, f"{int(count.item())} forwarded chunks do not hold their stored checksum"
    raw = scrub.cpu().numpy()
    assert (raw[n * bc.SCRUB_DT.itemsize:] == 0xEE).all()
    recs = raw[:n * bc.SCRUB_DT.itemsize].view(bc.SCRUB_DT)
    exp = np.zeros(n, dtype=bc.SCRUB_DT)
    for k, i in enumerate(want.write):
        exp[k]["data"] = d.arena.data_ptr() + q.lay.bases[i]
        exp[k]["length"], exp[k]["checksum_type"] = local["length"][i], local["checksum_type"][i]
        exp[k]["checksum"] = exp[k]["computed"] = local["checksum"][i]
    for f in bc.SCRUB_DT.names:
        assert np.array_equal(recs[f], exp[f]), (f, recs[f][:len(want.write)], exp[f][:len(want.write)])
    assert L.anomalies(0)["count"] == 0
    L.release_stream(st)
    if across:
        L.release_stream(last)


# ---- f. two workers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_two_workers_run_the_mixed_queue_at_once(hf, orc, dev, mode):
    """Two threads, each with its own stream and its own chunk set, queue the mixed calls at the same
    time and wait once each: the hint words and the pair buffers are per (stream, thread) pair."""
    L = hf._lib
    ds = [_resident(_built(orc, kind), dev) for kind in ("mixed", "mixed_b")]
    sts = [_fresh_stream(L, dev) for _ in ds]
    L.anomalies(0, reset=True)
    errors, gate = [], threading.Barrier(2)

    def once(d, st):
        try:
            gate.wait(timeout=30)
            d.enqueue(L, mode, st)
            st.synchronize()
            L.release_stream(st)  # (a pair record belongs to the thread that made it)
        except BaseException as e:  # (reported below, on the main thread)
            errors.append(e)

    threads = [threading.Thread(target=once, args=(d, st)) for d, st in zip(ds, sts)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors and not any(t.is_alive() for t in threads), errors
    for d in ds:
        d.check()
    assert L.anomalies(0)["count"] == 0


# ---- g. one graph ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_mixed_queue_in_one_graph(hf, orc, dev, mode):
    """The eight calls of the mixed queue captured into ONE graph on a side stream after an eager
    warm-up pass on it; replayed twice from restored chunks and records.  The captured calls' memory
    is the graph's: live while it exists, gone with it."""
    L = hf._lib
    d = _resident(_built(orc, "mixed"), dev)
    L.anomalies(0, reset=True)
    L.release_graph_scratch()
    base = L.graph_scratch_stats()
    cs = _fresh_stream(L, dev)
    d.enqueue(L, mode, cs)
    cs.synchronize()
    d.check()
    d.restore()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        d.enqueue(L, mode, cs)
    torch.cuda.synchronize()
    owned = L.graph_scratch_stats()
    assert owned["live"] > base["live"] and owned["live_bytes"] > base["live_bytes"], (base, owned)
    for rep in range(2):
        g.replay()
        torch.cuda.synchronize()
        d.check()
        d.restore()
    assert L.anomalies(0)["count"] == 0
    del g
    torch.cuda.synchronize()
    L.release_graph_scratch()
    end = L.graph_scratch_stats()
    assert end["dead"] == 0 and end["live"] == base["live"] and end["live_bytes"] == base["live_bytes"], (base, end)
    L.release_stream(cs)
