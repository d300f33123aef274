"""tests/update_queue.py checked on the CPU.  Numpy stand-ins play the library for a whole queue of
ordered, versioned, copy-on-write, chunk-engine and plain update calls: they read nothing but the
buffers a backend is sent (the records with the state the last call's model left, the payloads,
the arena's bytes) and apply the entry points' own models call by call.  The faithful stand-ins
must pass every checker; each one seeded with one ordering or lifetime defect of the kind only a
queue can show must be rejected with a message naming the call and the IO or the chunk."""
import functools
import re

import numpy as np
import pytest

import cow_cases as cc
import engine_cases as ec
import ordered_cases as oc
import update_footprint as fp
import update_queue as uq
import versioned_cases as vc

M32 = 0xFFFFFFFF
CHUNK_ADDR, PAY_ADDR, PAY_STEP = 0x7F0000000000, 0x7E0000000000, 1 << 32
VERSION_RUNGS = (vc.COMMITTED_UPDATE, vc.STALE_UPDATE, vc.MISSING_UPDATE, vc.ADVANCE_UPDATE)


def _body(buf, guard, n, dtype):
    return buf[guard:guard + n * dtype.itemsize].view(dtype)


def _payload(u, pay, pay_addr):
    return pay[int(u["payload"]) - pay_addr:int(u["payload"]) - pay_addr + int(u["length"])].tobytes()


class QueueStandIn:
    """update_queue.Queue's calls from their buffers alone: jobs decoded from the IO and version
    records, bytes from the arena, ordered_cases.simulate / versioned_cases.simulate on top."""

    def __init__(self, orc, q):
        self.orc, self.q = orc, q
        self.pay_addrs = [PAY_ADDR + k * PAY_STEP for k in range(len(q.calls))]
        self.sent = [q.buffers(k, CHUNK_ADDR, self.pay_addrs[k]) for k in range(len(q.calls))]
        self.chunk_at = {b: r % q.n for r, b in enumerate(q.lay.bases)}

    def play(self, k, arena, bufs, pay, read=None, keep_failed=None, alien=None):
        q, call = self.q, self.q.calls[k]
        n, ml = call.n, q.max_len
        rec = _body(bufs["rec"], fp.REC_GUARD, n, fp.REC)
        ver = _body(bufs["ver"], uq.VER_GUARD, n, vc.VER) if bufs["ver"] is not None else None
        src = arena if read is None else read
        dst = _body(bufs["dst"], cc.DST_GUARD, n, np.dtype("<u8")) if bufs.get("dst") is not None else np.zeros(n, "<u8")
        chunks, state, jobs, base_of = {}, {}, [], {}
        for i in range(n):
            u = rec[i]
            base = int(u["chunk"]) - CHUNK_ADDR
            c = self.chunk_at[base]
            if c not in chunks:
                base_of[c] = base
                chunks[c] = bytearray(src[base:base + ml].tobytes())
                ck = (int(u["chunk_checksum_type"]), int(u["chunk_checksum"]))
                if ver is None:
                    state[c] = (int(u["chunk_size"]), ck)
                else:
                    v = ver[i]
                    state[c] = vc.Meta(int(u["chunk_size"]), ck, int(v["chain_ver"]), int(v["update_ver"]),
                                       int(v["commit_ver"]), int(v["chunk_state"]), int(v["recycle_state"]),
                                       int(v["meta_chunk_size"]))
            kind = {fp.WRITE: "W", fp.TRUNCATE: "T", fp.EXTEND: "E", vc.COMMIT_JOB: "C"}[int(u["update_type"])]
            j = dict(c=c, chunk=c, k=kind, kind=kind, off=int(u["offset"]), ln=int(u["length"]),
                     sync=bool(int(u["flags"]) & vc.FLAG_SYNCING))
            if kind == "W":
                j["data"] = _payload(u, pay, self.pay_addrs[k])
                j["wck"] = (int(u["write_checksum_type"]), int(u["write_checksum"]))
                if alien is not None and alien[0] == i:  # the payload hash of another call's IO
                    j["data"] = alien[1]
            if ver is not None:
                j["ver"], j["jcv"], j["force"] = int(ver[i]["io_ver"]), int(ver[i]["job_chain_ver"]), bool(ver[i]["is_force"])
            jobs.append(j)
        if ver is not None:
            expect, info = vc.simulate(self.orc, jobs, chunks, state, ml, call.max_rounds)
            r, v = vc.expected(rec, ver, expect)
            rec[:], ver[:] = r, v
            failed = [e[0] != vc.OK for e in expect]
        else:
            expect = oc.simulate(self.orc, jobs, chunks, state, ml, call.max_rounds, q.ctype, False)
            r = oc.expected_records(None, rec, expect)
            if call.entry in (uq.BATCH, uq.COW):
                for f in uq.STATE_IO:
                    r[f] = rec[f]
            rec[:] = r
            depth = {}
            for j in jobs:
                depth[j["c"]] = depth.get(j["c"], 0) + 1
            info = (max(depth.values()), sum(1 for e in expect if e[0] == oc.NOT_APPLIED))
            failed = [e[0] != oc.OK for e in expect]
        if bufs["info"] is not None:
            bufs["info"][:] = info
        moved = {}
        for i, j in enumerate(jobs):  # copy-on-write: bytes [0, out_size) to the destination, the source stays
            d = int(dst[i])
            if d and d != int(rec[i]["chunk"]) and not failed[i]:
                moved[j["c"]] = (d - CHUNK_ADDR, int(rec[i]["out_size"]))
        for c, ch in chunks.items():
            if c in moved:
                b, size = moved[c]
                arena[b:b + size] = np.frombuffer(bytes(ch[:size]), dtype=np.uint8)
            else:
                arena[base_of[c]:base_of[c] + ml] = np.frombuffer(bytes(ch), dtype=np.uint8)
        if keep_failed is not None:
            j = jobs[keep_failed]
            assert failed[keep_failed] and j["k"] == "W" and j["off"] + j["ln"] <= ml
            b = base_of[j["c"]] + j["off"]
            arena[b:b + j["ln"]] = np.frombuffer(j["data"], dtype=np.uint8)

    def run(self, fault=None, at=None):
        q, K = self.q, len(self.q.calls)
        arena = q.arena0.copy()
        pays = [c.pay.copy() for c in q.calls]
        got = [{n: (None if b is None else b.copy()) for n, b in s.items()} for s in self.sent]
        order = list(range(K))
        if fault == "swapped":
            order[at], order[at + 1] = order[at + 1], order[at]
        if fault == "last_skipped":
            order = order[:-1]
        before = None
        for k in order:
            if fault == "missed_join" and k == at:
                before = arena.copy()  # what call at + 1 reads: the bytes before call `at`
            alien = None
            if fault == "next_call_hash" and k == at[0]:  # IO at[1] hashed from call k + 1's payload of the same index
                u = _body(self.sent[k + 1]["rec"], fp.REC_GUARD, q.calls[k + 1].n, fp.REC)[at[1]]
                alien = (at[1], _payload(u, pays[k + 1], self.pay_addrs[k + 1]))
            self.play(k, arena, got[k], pays[k], read=before if fault == "missed_join" and k == at + 1 else None,
                      keep_failed=at[1] if fault == "failed_io_written" and at[0] == k else None, alien=alien)
        if fault == "shared_scratch":  # call `at` finalized from the control words of call at + 1
            a = _body(got[at]["rec"], fp.REC_GUARD, q.calls[at].n, fp.REC)
            b = _body(got[at + 1]["rec"], fp.REC_GUARD, q.calls[at + 1].n, fp.REC)
            m = min(a.size, b.size)
            for f in fp.OUTPUT_FIELDS:
                a[f][:m] = b[f][:m]
        if fault == "info_of_next":
            got[at]["info"][:] = got[at + 1]["info"]
        if fault == "arena_guard":
            arena[q.lay.bases[at] + q.max_len] ^= 0x40
        if fault == "version_guard":
            got[at]["ver"][-uq.VER_GUARD] ^= 0x40
        return arena, pays, got, self.sent


class CowStandIn:
    """update_queue.CowQueue's calls from their records, destination arrays and the arena's bytes:
    oracle.replica_apply on a copy of the source, the result placed at the destination."""

    def __init__(self, orc, q):
        self.orc, self.q = orc, q
        self.pay_addrs = [PAY_ADDR + k * PAY_STEP for k in range(len(q.scns))]
        self.sent = [s.record_buffer(CHUNK_ADDR, self.pay_addrs[k]) for k, s in enumerate(q.scns)]
        self.sent_dst = [s.dst_buffer(CHUNK_ADDR) for s in q.scns]

    def play(self, k, arena, recbuf, dstbuf, pay, stale_source=None, keep_failed=None):
        q, orc, ml = self.q, self.orc, self.q.max_len
        rec = _body(recbuf, fp.REC_GUARD, q.n, fp.REC)
        dst = _body(dstbuf, cc.DST_GUARD, q.n, np.dtype("<u8"))
        for i in range(q.n):
            u = rec[i]
            base, s0 = int(u["chunk"]) - CHUNK_ADDR, int(u["chunk_size"])
            ck = (int(u["chunk_checksum_type"]), int(u["chunk_checksum"]))
            wck = (int(u["write_checksum_type"]), int(u["write_checksum"]))
            off, ln, kind = int(u["offset"]), int(u["length"]), int(u["update_type"])
            sync = bool(int(u["flags"]) & cc.FLAG_SYNCING)
            d = int(dst[i])
            oop = d not in (0, int(u["chunk"]))
            src = stale_source if stale_source is not None and oop else arena
            work = bytearray(src[base:base + ml].tobytes())
            data = _payload(u, pay, self.pay_addrs[k]) if kind == fp.WRITE else b""
            if kind != fp.WRITE:
                e = (fp.INVALID_ARG, s0, ck, 0) if sync else orc.replica_apply(work, s0, ck, kind, 0, ln, with_case=True)
            elif not sync:
                e = orc.replica_apply(work, s0, ck, fp.WRITE, off, ln, data, wck, chunk_size=ml, with_case=True)
            elif off != 0 or ln > ml:
                e = (fp.INVALID_ARG, s0, ck, 0)
            elif wck[0] != fp.NONE and ln and tuple(orc.create(wck[0], data)) != wck:
                e = (fp.CHECKSUM_MISMATCH, s0, ck, 0)
            else:  # the chunk becomes the payload (ChunkReplica.cc:289,334-339,392)
                work[:ln] = data
                e = (fp.OK, ln, (wck[0], 0 if wck[0] == fp.NONE or not ln else tuple(orc.create(wck[0], data))[1]),
                     1 if wck[0] == fp.NONE or not ln else 2)
            u["status"], u["out_size"], u["checksum_case"] = e[0], e[1], e[3]
            u["out_checksum_type"], u["out_checksum"] = e[2]
            if e[0] == fp.OK and oop:
                arena[d - CHUNK_ADDR:d - CHUNK_ADDR + e[1]] = np.frombuffer(bytes(work[:e[1]]), dtype=np.uint8)
            elif e[0] == fp.OK:
                arena[base:base + ml] = np.frombuffer(bytes(work), dtype=np.uint8)
            elif keep_failed == i:
                assert kind == fp.WRITE and off + ln <= ml
                arena[base + off:base + off + ln] = np.frombuffer(data, dtype=np.uint8)

    def run(self, fault=None, at=None):
        q, K = self.q, len(self.q.scns)
        snaps = self.run()[4] if fault == "source_after_next" else None
        arena = q.arena0.copy()
        pays = [s.payload_image(0).copy() for s in q.scns]
        recs, dsts = [b.copy() for b in self.sent], [b.copy() for b in self.sent_dst]
        order = list(range(K))
        if fault == "swapped":
            order[at], order[at + 1] = order[at + 1], order[at]
        if fault == "last_skipped":
            order = order[:-1]
        after = []
        for k in order:
            self.play(k, arena, recs[k], dsts[k], pays[k],
                      stale_source=snaps[k + 1] if fault == "source_after_next" and k == at else None,
                      keep_failed=at[1] if fault == "failed_io_written" and at[0] == k else None)
            after.append(arena.copy())
        if fault == "dst_guard":
            dsts[at][cc.DST_GUARD - 1] ^= 0x40
        return arena, pays, recs, self.sent, after, dsts, self.sent_dst

    def check(self, r):
        uq.check_cow_queue(self.q, r[0], r[1], r[2], r[3], r[5], r[6])


class EngineStandIn:
    """update_queue.EngineQueue's calls from d_ios, d_jobs and the arena: engine_cases.simulate."""

    def __init__(self, orc, q):
        self.orc, self.q = orc, q
        self.pay_addrs = [PAY_ADDR + k * PAY_STEP for k in range(len(q.calls))]
        self.sent = [q.buffers(k, CHUNK_ADDR, self.pay_addrs[k]) for k in range(len(q.calls))]

    def play(self, k, arena, bufs, pay):
        q, call = self.q, self.q.calls[k]
        rec = _body(bufs["rec"], fp.REC_GUARD, call.n, fp.REC)
        jr = _body(bufs["jr"], uq.JOB_GUARD, call.n, ec.JOB)
        rel = lambda a: int(a) - CHUNK_ADDR if int(a) else 0
        ids, chunks, jobs = {}, [], []
        for i in range(call.n):
            u, v = rec[i], jr[i]
            key = int(u["chunk"])
            if key not in ids:
                ids[key] = len(chunks)
                w = None
                if int(v["w_addr"]):
                    w = ec.Writing(rel(v["w_addr"]), int(v["w_len"]), (~int(v["w_checksum"])) & M32, int(v["w_chain_ver"]),
                                   int(v["w_chunk_ver"]))
                ch = ec.Chunk(rel(v["addr"]), int(u["chunk_size"]), (~int(u["chunk_checksum"])) & M32, int(v["chain_ver"]),
                              int(v["chunk_ver"]), w)
                chunks.append(ch)
            kind = {fp.WRITE: "W", fp.TRUNCATE: "T", fp.EXTEND: "E", ec.COMMIT_JOB: "C"}[int(u["update_type"])]
            j = dict(c=ids[key], k=kind, off=int(u["offset"]), ln=int(u["length"]), ver=int(v["io_ver"]),
                     jcv=int(v["job_chain_ver"]), dst=rel(v["dst"]), sync=bool(int(u["flags"]) & ec.FLAG_SYNCING),
                     engine=bool(int(u["flags"]) & ec.FLAG_ENGINE))
            if kind == "W":
                j["data"] = _payload(u, pay, self.pay_addrs[k])
                j["wfin"] = None if int(u["write_checksum_type"]) == fp.NONE else (~int(u["write_checksum"])) & M32
            jobs.append(j)
        expect, info = ec.simulate(self.orc, jobs, arena, chunks, q.max_len, call.max_rounds)
        r, j = ec.expected(rec, jr, expect, CHUNK_ADDR)
        rec[:], jr[:] = r, j
        bufs["info"][:] = info

    def run(self, fault=None, at=None):
        q, K = self.q, len(self.q.calls)
        arena = q.arena0.copy()
        pays = [c.pay.copy() for c in q.calls]
        got = [{n: b.copy() for n, b in s.items()} for s in self.sent]
        order = list(range(K))
        if fault == "swapped":
            order[at], order[at + 1] = order[at + 1], order[at]
        if fault == "last_skipped":
            order = order[:-1]
        for k in order:
            self.play(k, arena, got[k], pays[k])
        if fault == "info_of_next":
            got[at]["info"][:] = got[at + 1]["info"]
        if fault == "job_guard":
            got[at]["jr"][-uq.JOB_GUARD] ^= 0x40
        return CHUNK_ADDR, arena, pays, got, self.sent


# ---- the queues (small: the checkers do not depend on the size) ------------------------------------------
@functools.lru_cache(maxsize=None)
def _queue(orc, name):
    return {"ordered": lambda: uq.chain_queue(orc, 512),
            "ordered_crc32": lambda: uq.chain_queue(orc, 4096, ctype=fp.CRC32),
            "versioned": lambda: uq.chain_queue(orc, 512, versioned=True),
            "versioned_4k": lambda: uq.chain_queue(orc, 4096, versioned=True),
            "mixed": lambda: uq.mixed_queue(orc, 512).q,
            "density_ordered": lambda: uq.density_queue(orc, uq.ORDERED, max_len=2048, n=16),
            "density_batch": lambda: uq.density_queue(orc, uq.BATCH, max_len=2048, n=16),
            "growth_ordered": lambda: uq.growth_queue(orc, counts=(4, 24, 2, 24, 8, 24), max_len=512),
            "growth_versioned": lambda: uq.growth_queue(orc, True, counts=(4, 24, 2, 24, 8, 24), max_len=512)}[name]()


QUEUES = ["ordered", "ordered_crc32", "versioned", "versioned_4k", "mixed", "density_ordered", "density_batch",
          "growth_ordered", "growth_versioned"]


@pytest.mark.parametrize("name", QUEUES)
def test_faithful_stand_in_passes(orc, name):
    q = _queue(orc, name)
    uq.check_queue(q, *QueueStandIn(orc, q).run())


@pytest.mark.parametrize("max_len", [512, 8192])
def test_faithful_cow_stand_in_passes(orc, max_len):
    q = uq.cow_queue(orc, max_len)
    si = CowStandIn(orc, q)
    si.check(si.run())
    si = CowStandIn(orc, uq.cow_density_queue(orc, max_len=2048, n=16))
    si.check(si.run())


@pytest.mark.parametrize("max_len", [512, 8192])
def test_faithful_engine_stand_in_passes(orc, max_len):
    q = uq.engine_queue(orc, max_len)
    uq.check_engine_queue(q, *EngineStandIn(orc, q).run())
    m = uq.mixed_queue(orc, max_len)
    uq.check_engine_queue(m.e, *EngineStandIn(orc, m.e).run())
    assert [p for p in m.plan if p[0] == "q"] == [("q", k) for k in range(len(m.q.calls))] and ("e", 0) in m.plan


def test_the_queues_hold_what_they_are_for(orc):
    """The traffic the GPU tests rely on is really in the queues."""
    for versioned in (False, True):
        q = _queue(orc, "versioned" if versioned else "ordered")
        st = [set(c.statuses) for c in q.calls]
        assert len(q.calls) == 5 and all(32 <= c.n <= 64 and c.max_rounds == 4 for c in q.calls)
        assert oc.CHECKSUM_MISMATCH in st[1] and oc.NOT_APPLIED in st[2] and oc.INVALID_ARG in st[3]
        assert q.calls[2].info[:2] == (5, 1)
        late = next(j for j, s in zip(q.calls[2].jobs, q.calls[2].statuses) if s == oc.NOT_APPLIED)
        again = q.calls[3].jobs[0]
        assert (again["c"], again["k"], again.get("data")) == (late["c"], late["k"], late.get("data"))
        kinds = {(j["k"], j.get("flavour", "")) for c in q.calls for j in c.jobs}
        assert {("W", ""), ("W", "none"), ("W", "corrupt"), ("T", ""), ("E", "")} <= kinds
        if versioned:
            flat = [s for c in q.calls for s in c.statuses]
            refused = sum(s in VERSION_RUNGS for s in flat)
            assert 0.04 * len(flat) <= refused <= 0.2 * len(flat), (refused, len(flat))
            assert vc.CHAIN_VERSION_MISMATCH in st[0] and any(j.get("force") for j in q.calls[4].jobs)
            assert sum(c.info[3] for c in q.calls) >= 10  # commits that commit
    m = uq.mixed_queue(orc, 512)
    assert [c.entry for c in m.q.calls] == [uq.ORDERED, uq.BATCH, uq.VERSIONED, uq.COW, uq.ORDERED, uq.BATCH, uq.VERSIONED]
    assert len(m.plan) == 8 and all(32 <= c.n <= 64 for c in m.q.calls + m.e.calls)
    cow, after = m.q.calls[3], m.q.calls[4]  # the copy-on-write call moves chunks; the ordered call finds them there
    moved = {cow.chunk_of[i]: int(cow.dst[i]) for i in range(cow.n) if cow.dst[i] and cow.statuses[i] == oc.OK}
    stayed = {cow.chunk_of[i]: int(cow.rec["chunk"][i]) for i in range(cow.n) if cow.chunk_of[i] not in moved}
    assert len(moved) >= 20 and len(stayed) >= 4 and any(cow.dst[i] and cow.statuses[i] != oc.OK for i in range(cow.n))
    for i, c in enumerate(after.chunk_of):
        assert int(after.rec["chunk"][i]) == moved.get(c, stayed.get(c)), (i, c)
    for entry in (uq.ORDERED, uq.BATCH):
        q = _queue(orc, f"density_{entry}")
        for k, c in enumerate(q.calls):
            lens = [j["ln"] for j in c.jobs if j["k"] == "W"]
            assert (set(lens) == {q.max_len} and len(lens) == c.n) if k % 2 else set(lens) == {1}
    q = uq.cow_queue(orc, 512)
    assert len(q.scns) == 4
    for s in q.scns:
        r = s.rounds[0]
        assert {fp.OK, fp.CHECKSUM_MISMATCH, fp.INVALID_ARG} == {e[0] for e in r.expect}
        assert any(op.get("sync") for op in r.ops[:q.n]) and cc.IN_PLACE_ZERO in set(r.place)
    for k in range(1, 4):  # every call's sources are where the call before left the chunks
        prev, cur = q.scns[k - 1].rounds[0], q.scns[k].rounds[0]
        for c in range(q.n):
            moved = prev.place[c] == cc.OUT_OF_PLACE and prev.expect[c][0] == fp.OK
            assert int(cur.rec["chunk"][c]) == (int(prev.dst[c]) if moved else int(prev.rec["chunk"][c]))
    e = uq.engine_queue(orc, 512)
    assert len(e.calls) == 4 and all(32 <= c.n <= 64 for c in e.calls)
    assert ec.CHAIN_VERSION_MISMATCH in e.calls[1].statuses and all(c.info[5] and c.info[6] for c in e.calls)
    for c in range(e.n):  # update, commit, update, commit ... per chunk across the queue
        seq = [j["k"] == "C" for call in e.calls for j, s in zip(call.jobs, call.statuses) if j["c"] == c and s == ec.OK]
        assert all(a != b for a, b in zip(seq, seq[1:])) and not seq[0], (c, seq)


def test_sync_tables_come_from_the_final_state(orc):
    """The resync follower's local table is the versioned model's final state; the plan forwards the
    chunks the successor lacks or holds at a lower chain version, and nothing in it is fatal."""
    import sync_cases as sc
    q = _queue(orc, "versioned")
    local, remote, want = uq.sync_tables(q)
    assert local.size == q.n and remote.size == q.n - 2
    for c, m in enumerate(q.metas):
        assert (int(local["length"][c]), int(local["checksum_type"][c]), int(local["checksum"][c])) == m.io()
        assert (int(local["chain_ver"][c]), int(local["update_ver"][c]), int(local["commit_ver"][c])) == m.ver()[:3]
        assert int(local["chain_ver"][c]) == uq.SYNC_CHAIN_VER
    assert want.info["fatal"] == 0 and want.info["remote_miss"] == 2 and want.info["chain_ver_low"] == (q.n - 2 + 2) // 3
    assert want.info["n_write"] == len(want.write) == want.info["remote_miss"] + want.info["chain_ver_low"]
    assert want.remove == [] and want.info["skip"] == remote.size - want.info["chain_ver_low"]
    img = q.final_image()
    for i in want.write:  # what the scrub behind the plan must find: the stored value over the final bytes
        o, ln, t = q.lay.bases[i], int(local["length"][i]), int(local["checksum_type"][i])
        if t != fp.NONE and ln:
            assert tuple(orc.create(t, img[o:o + ln].tobytes())) == (t, int(local["checksum"][i])), i
    assert len({sc.MATCHED, sc.REMOTE_MISS} & set(want.lclass)) == 2


# ---- seeded defects ----------------------------------------------------------------------------------------
NAMED = r"call (\d+) \((\w+)\): (IO|job) (\d+) \(chunk (\d+)"


def _rejected(check, result, pattern=NAMED):
    with pytest.raises(AssertionError, match=pattern) as e:
        check(*result)
    return re.search(pattern, str(e.value))


@pytest.mark.parametrize("name", ["ordered", "versioned", "mixed"])
def test_seeded_queue_stand_ins_are_rejected(orc, name):
    q = _queue(orc, name)
    si = QueueStandIn(orc, q)
    chk = functools.partial(uq.check_queue, q)
    last = len(q.calls) - 1

    m = _rejected(chk, si.run("swapped", 1))                    # two adjacent calls swapped
    assert int(m.group(1)) in (1, 2)
    _rejected(chk, si.run("last_skipped"), rf"call {last} \(\w+\): IO \d+ \(chunk \d+")
    m = _rejected(chk, si.run("missed_join", 1))                # call 2 starts from the state before call 1
    assert int(m.group(1)) >= 2
    m = _rejected(chk, si.run("shared_scratch", 1))             # call 1 finalized from call 2's control words
    assert int(m.group(1)) == 1

    # a failed IO's payload bytes left in the chunk, where no later IO rewrites them
    k, i = next((last, i) for i, s in reversed(list(enumerate(q.calls[last].statuses))) if s == oc.CHECKSUM_MISMATCH)
    c = q.calls[k].jobs[i]["c"]
    _rejected(chk, si.run("failed_io_written", (k, i)), rf"chunk arena differs .* = chunk ({c}|{c + q.n}) \+.*chunk {c}( \(it lives in region \d+\))? was last written by "
                       rf"call \d+ IO \d+")

    # guard bytes: between two chunks of the arena, behind a call's version records
    _rejected(chk, si.run("arena_guard", 3), r"chunk arena differs in 1 bytes .* = guard after chunk 3: 0 B past its region")
    if name != "ordered":
        kv = next(k for k, call in enumerate(q.calls) if call.ver is not None)
        _rejected(chk, si.run("version_guard", kv), rf"call {kv} \(versioned\): ver guard changed .* \(behind IO \d+\)")

    if name == "mixed":
        return
    # d_info of call 1 holding call 2's counts
    assert q.calls[1].info != q.calls[2].info
    _rejected(chk, si.run("info_of_next", 1), rf"call 1 \({name}\): d_info .* \(IO count {q.calls[1].n}\)")
    if name == "versioned":  # a refused job's payload hash taken from the next call: 4080 instead of the rung's code
        k, i = next((k, i) for k, call in enumerate(q.calls[:-1]) for i, (j, s) in enumerate(zip(call.jobs, call.statuses))
                    if s in VERSION_RUNGS and j["k"] == "W" and j["ln"] and i < q.calls[k + 1].n and
                    q.calls[k + 1].jobs[i]["k"] == "W" and q.calls[k + 1].jobs[i]["ln"])
        m = _rejected(chk, si.run("next_call_hash", (k, i)))
        assert (int(m.group(1)), int(m.group(4))) == (k, i) and "field status: got 4080" in m.string


def test_seeded_cow_stand_ins_are_rejected(orc):
    q = uq.cow_queue(orc, 8192)
    si = CowStandIn(orc, q)
    named = r"call (\d+) \(cow\): .*round 0: chunk (\d+) "
    moved = r"chunk arena differs .* a region of chunk (\d+), which lives in region \d+ and was moved by call\(s\) \["

    def rejected(result, pattern):
        with pytest.raises(AssertionError, match=pattern) as e:
            si.check(result)
        return re.search(pattern, str(e.value))

    m = rejected(si.run("swapped", 1), named)
    assert int(m.group(1)) in (1, 2)
    rejected(si.run("last_skipped"), rf"call {len(q.scns) - 1} \(cow\): .*round 0: chunk \d+ ")
    # call 1 reading its sources after call 2 overwrote them: call 2 moves the chunks back there
    rejected(si.run("source_after_next", 1), rf"({named}|{moved})")
    k = len(q.scns) - 1
    i = next(i for i, e in enumerate(q.scns[k].rounds[0].expect) if e[0] == fp.CHECKSUM_MISMATCH)
    m = rejected(si.run("failed_io_written", (k, i)), moved)
    assert int(m.group(1)) == i
    rejected(si.run("dst_guard", 2), r"call 2 \(cow\): destination array or its guards changed at buffer offset \d+")


def test_seeded_engine_stand_ins_are_rejected(orc):
    q = uq.engine_queue(orc, 512)
    si = EngineStandIn(orc, q)
    chk = functools.partial(uq.check_engine_queue, q)
    m = _rejected(chk, si.run("swapped", 1))
    assert int(m.group(1)) in (1, 2)
    _rejected(chk, si.run("last_skipped"), rf"call {len(q.calls) - 1} \(engine\): job \d+ \(chunk \d+")
    assert q.calls[1].info != q.calls[2].info
    _rejected(chk, si.run("info_of_next", 1), rf"call 1 \(engine\): d_info .* \(job count {q.calls[1].n}\)")
    _rejected(chk, si.run("job_guard", 2), r"call 2 \(engine\): jr guard changed .* \(behind job \d+\)")


# ---- layouts -------------------------------------------------------------------------------------------------
def test_record_layouts_match_the_ctypes_mirrors(hf, orc):
    """What the builders write is what the library reads: the three record types against
    3fs_amd/_lib.py, and the entry points' constants."""
    L = hf._lib
    for name in fp.REC.names:
        assert fp.REC.fields[name][1] == getattr(hf.UpdateIO, name).offset, name
    assert fp.REC.itemsize == 56 == __import__("ctypes").sizeof(hf.UpdateIO)
    assert L.update_ver_dtype() == vc.VER and L.engine_job_dtype() == ec.JOB
    assert uq.INFO_WORDS[uq.VERSIONED] == L.VER_INFO_WORDS and ec.INFO_WORDS == L.ENGINE_INFO_WORDS
    assert (vc.FLAG_ENGINE, vc.FLAG_SYNCING) == (L.UPDATE_FLAG_ENGINE, L.UPDATE_FLAG_SYNCING)
    q = _queue(orc, "versioned")
    b = q.buffers(0, CHUNK_ADDR, PAY_ADDR)
    n = q.calls[0].n
    assert b["rec"].size == 2 * fp.REC_GUARD + n * 56 and b["ver"].size == 2 * uq.VER_GUARD + n * 48
    assert b["info"].size == 8 and b["dst"] is None
    rec = _body(b["rec"], fp.REC_GUARD, n, fp.REC)
    assert all(int(a) - CHUNK_ADDR in q.lay.bases for a in rec["chunk"])
    e = uq.engine_queue(orc, 512, calls=1)
    b = e.buffers(0, CHUNK_ADDR, PAY_ADDR)
    assert b["jr"].size == 2 * uq.JOB_GUARD + e.calls[0].n * 104 and b["info"].size == 8
