"""Queues of update calls on the SAME chunks, for tests/test_gpu_update_queue.py (the HIP library,
calls queued back to back on one stream with one wait at the end) and
tests/test_update_queue_model.py (numpy stand-ins that check the checkers).  Numpy only.

tests/stream_queue.py queues hf3fs_crc_update_batch.  Here the calls are hf3fs_crc_update_ordered,
hf3fs_crc_update_versioned, hf3fs_crc_update_cow_batch, hf3fs_crc_update_engine, and update_batch
between them.  Every expected value comes from the models those entry points already have --
ordered_cases.simulate, versioned_cases.simulate, engine_cases.simulate, cow_cases.CowScenario,
and the oracle underneath them -- driven call by call: call k + 1 is built from the state call k's
model left (chunk bytes, sizes, checksums, version records, the engine's writing list, and the
place each chunk moved to).

  Queue      one arena of n chunks (update_footprint.Layout: canary guards of MARGIN between
             them).  add(entry, jobs, max_rounds) appends one call; every call keeps its own
             payload image, record array, version array, destination array and d_info.  The
             records of call k + 1 carry the state the model says call k leaves: the device never
             hands it back through the host.
  CowQueue   copy-on-write calls: 2 n regions, chunk c lives in region c or n + c and every
             out-of-place IO that succeeds moves it to the other one, so call k + 1's sources are
             call k's destinations.
  EngineQueue
             update_engine calls: engine_cases.simulate over one arena keyed by address, the
             committed and writing state of every chunk carried on; call k + 1's chunk keys are the
             committed addresses call k left.
  traffic, chain_queue, mixed_queue, density_queue, growth_queue, cow_queue, cow_density_queue,
  engine_queue, sync_tables
             the queues the GPU tests run.
  check_queue / check_cow_queue / check_engine_queue
             after the whole queue: the WHOLE arena, every call's whole record buffer (output
             fields and the state fields the call rewrites), version / destination buffers, d_info
             and payloads.  A failure names the call, and the IO or the chunk.
"""
import numpy as np

import cow_cases as cc
import engine_cases as ec
import ordered_cases as oc
import sync_cases as sc
import update_footprint as fp
import versioned_cases as vc

ORDERED, VERSIONED, BATCH, COW = "ordered", "versioned", "batch", "cow"
ENTRIES = (ORDERED, VERSIONED, BATCH, COW)
INFO_FILL = 0x7777
INFO_WORDS = {ORDERED: 2, VERSIONED: vc.INFO_WORDS, BATCH: 0, COW: 0}
VER_GUARD = 1 << 10
SALT_VER = 0x6B
STATE_IO = ("chunk_size", "chunk_checksum_type", "chunk_checksum")


class Call:
    pass


def _guarded(body, guard, salt):
    buf = fp.canary(2 * guard + body.nbytes, salt)
    buf[guard:guard + body.nbytes] = body.view(np.uint8).reshape(-1)
    return buf


class Queue:
    """Calls of update_ordered / update_versioned / update_batch / update_cow_batch on one set of
    chunks (copy-on-write: every IO in place with a destination array of zeros, or add(move=True)).
    A job is a dict of versioned_cases.W / T / E / C; the entry points without version records
    ignore its versions."""

    engine = False  # (what stream_queue.followup_records reads of a scenario)

    def __init__(self, orc, n_chunks, max_len, ctype=fp.CRC32C, gap=fp.MARGIN, seed=1, name="queue", spare=False):
        """spare: every chunk gets a second region (n + c) a copy-on-write call can move it to."""
        self.orc, self.n, self.max_len, self.ctype, self.name = orc, n_chunks, max_len, ctype, name
        self.spare = spare
        self.lay = fp.Layout(2 * n_chunks if spare else n_chunks, max_len, gap)
        self.canary = fp.canary(self.lay.size, fp.SALT_CHUNKS)
        self.regions = [bytearray(self.canary[b:b + max_len].tobytes()) for b in self.lay.bases]
        self.loc = list(range(n_chunks))  # the region chunk c lives in: c or n + c
        self.metas = [vc.Meta(ck=(ctype, 0), meta_chunk_size=max_len) for _ in range(n_chunks)]
        self.rng = np.random.default_rng(seed)
        self.calls = []
        self.arena0 = None
        self._final = None
        self.last_writer = {}  # chunk -> (call, IO) of the last IO that was applied

    # -- state -------------------------------------------------------------------------------------
    @property
    def chunks(self):
        return [self.regions[r] for r in self.loc]

    def base(self, c):
        return self.lay.bases[self.loc[c]]

    def other(self, c):
        return c + self.n if self.loc[c] == c else c

    @property
    def sizes(self):
        return [m.size for m in self.metas]

    @property
    def cks(self):
        return [m.ck for m in self.metas]

    def preset(self, c, size):
        assert not self.calls
        data = self.rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        self.regions[c][:size] = data
        self.metas[c].size = size
        self.metas[c].ck = tuple(self.orc.create(self.ctype, data)) if size else (self.ctype, 0)

    def image(self):
        img = self.canary.copy()
        for r, b in enumerate(self.lay.bases):
            img[b:b + self.max_len] = np.frombuffer(bytes(self.regions[r]), dtype=np.uint8)
        return img

    # -- building ----------------------------------------------------------------------------------
    def add(self, entry, jobs, max_rounds=1, move=False):
        """move (copy-on-write only): every IO is out of place, its destination the chunk's other
        region, except jobs that say place=False (destination entry 0).  As cow_cases.CowScenario
        states it: the model runs on a copy of the source, an IO that succeeds leaves bytes
        [0, out_size) at the destination and the chunk lives there from then on; the source region
        stays what it was, and a failed IO leaves both."""
        assert entry in ENTRIES and (not move or (entry == COW and self.spare))
        if self.arena0 is None:
            self.arena0 = self.image()
            self.arena0.setflags(write=False)
        orc, n, k = self.orc, len(jobs), len(self.calls)
        jobs = [dict(j) for j in jobs]
        rec = np.zeros(n, dtype=fp.REC)
        ver = np.zeros(n, dtype=vc.VER) if entry == VERSIONED else None
        has_payload = np.zeros(n, dtype=bool)
        placed, first, cur = [], set(), fp.PAY_GUARD
        for i, job in enumerate(jobs):
            c, kind = job["c"], job["k"]
            u, m = rec[i], self.metas[c]
            u["chunk"] = self.base(c)
            if job.get("sync"):
                assert entry == VERSIONED, "only the versioned model states a syncing write"
                u["flags"] = vc.FLAG_SYNCING
            if ver is not None:
                v = ver[i]
                v["io_ver"], v["job_chain_ver"], v["is_force"] = job["ver"], job["jcv"], 1 if job.get("force") else 0
            if c not in first:  # the chunk's first job carries the state the last call left
                first.add(c)
                u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = m.io()
                if ver is not None:
                    for f, x in zip(vc.STATE_FIELDS, m.ver()):
                        v[f] = x
            else:
                assert entry in (ORDERED, VERSIONED), f"{entry}: chunk {c} twice in one call"
                u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = oc.JUNK
                if ver is not None:
                    for f, x in zip(vc.STATE_FIELDS, vc.JUNK_VER):
                        v[f] = x
            if kind == "C":
                assert entry == VERSIONED
                u["update_type"], u["offset"], u["length"], u["payload"] = vc.COMMIT_JOB, 0xFFFFFFF0, 77, 0
            elif kind in "TE":
                u["update_type"], u["length"] = (fp.TRUNCATE if kind == "T" else fp.EXTEND), job["ln"]
            else:
                off, ln = int(job["off"]), int(job["ln"])
                if "data" not in job:  # (a resubmitted job brings its payload along)
                    job["data"] = self.rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
                    wck = tuple(orc.create(self.ctype, job["data"]))
                    if job.get("flavour") == "corrupt":
                        wck = (wck[0], wck[1] ^ 0x10)
                    if job.get("flavour") == "none":
                        wck = (fp.NONE, 0)
                    job["wck"] = wck
                p = ((cur + 15) & ~15) + (self.base(c) + off + i * 7) % 16
                cur = p + ln + 64
                placed.append((p, job["data"]))
                has_payload[i] = True
                u["update_type"], u["offset"], u["length"], u["payload"] = fp.WRITE, off, ln, p
                u["write_checksum_type"], u["write_checksum"] = job["wck"]
        pay = fp.canary(cur + fp.PAY_GUARD, fp.SALT_PAYLOAD)
        for p, data in placed:
            pay[p:p + len(data)] = np.frombuffer(data, dtype=np.uint8)
        pay.setflags(write=False)

        call = Call()
        call.k, call.entry, call.n, call.max_rounds, call.jobs = k, entry, n, max_rounds, jobs
        call.rec, call.ver, call.has_payload, call.pay = rec, ver, has_payload, pay
        call.chunk_of = [j["c"] for j in jobs]
        call.dst = np.zeros(n, dtype=np.uint64)  # arena-relative, 0: in place
        if entry == VERSIONED:
            call.expect, call.info = vc.simulate(orc, jobs, self.chunks, self.metas, self.max_len, max_rounds)
            ok = [e[0] == vc.OK and j["k"] != "C" for e, j in zip(call.expect, jobs)]
        else:
            state = [(m.size, m.ck) for m in self.metas]
            ios = [dict(chunk=j["c"], kind="W", off=j["off"], ln=j["ln"], data=j["data"], wck=j["wck"]) if j["k"] == "W"
                   else dict(chunk=j["c"], kind=j["k"], ln=int(j["ln"])) for j in jobs]
            work = [bytearray(ch) for ch in self.chunks] if move else self.chunks
            call.expect = oc.simulate(orc, ios, work, state, self.max_len, max_rounds, self.ctype, False)
            for i, (j, e) in enumerate(zip(jobs, call.expect) if move else ()):
                c = j["c"]
                if not j.get("place", True):
                    if e[0] == oc.OK:
                        self.regions[self.loc[c]][:] = work[c]
                    continue
                call.dst[i] = self.lay.bases[self.other(c)]
                if e[0] == oc.OK:
                    self.regions[self.other(c)][:e[1]] = work[c][:e[1]]
                    self.loc[c] = self.other(c)
            for c in first:
                self.metas[c].size, self.metas[c].ck = state[c][0], tuple(state[c][1])
            depth = {}
            for c in call.chunk_of:
                depth[c] = depth.get(c, 0) + 1
            call.info = (max(depth.values()), sum(1 for e in call.expect if e[0] == oc.NOT_APPLIED))
            ok = [e[0] == oc.OK for e in call.expect]
        for i, good in enumerate(ok):
            if good:
                self.last_writer[call.chunk_of[i]] = (k, i)
        call.metas_after = [m.copy() for m in self.metas]
        call.statuses = [int(e[0]) for e in call.expect]
        self.calls.append(call)
        self._final = None
        return call

    def final_image(self):
        if self._final is None:
            self._final = self.image()
            self._final.setflags(write=False)
        return self._final

    # -- what a backend sends, and what it must find afterwards ----------------------------------------
    def buffers(self, k, chunk_addr, pay_addr):
        """Call k's buffers with absolute addresses: dict(rec=, ver=, dst=, info=); rec, ver and dst
        inside canary guards (REC_GUARD, VER_GUARD, cow_cases.DST_GUARD), absent ones None."""
        call = self.calls[k]
        rec = call.rec.copy()
        rec["chunk"] += np.uint64(chunk_addr)
        rec["payload"][call.has_payload] += np.uint64(pay_addr)
        words = INFO_WORDS[call.entry]
        return dict(rec=_guarded(rec, fp.REC_GUARD, fp.SALT_RECORDS),
                    ver=_guarded(call.ver, VER_GUARD, SALT_VER) if call.ver is not None else None,
                    dst=_guarded(np.where(call.dst != 0, call.dst + np.uint64(chunk_addr), 0).astype(np.uint64),
                                 cc.DST_GUARD, cc.SALT_DST) if call.entry == COW else None,
                    info=np.full(words, INFO_FILL, dtype=np.uint32) if words else None)

    def want(self, k, sent):
        """The buffers call k must leave, from the ones it was sent."""
        call = self.calls[k]
        out = {name: (None if b is None else b.copy()) for name, b in sent.items()}
        rec = out["rec"][fp.REC_GUARD:fp.REC_GUARD + call.n * fp.REC.itemsize].view(fp.REC)
        if call.entry == VERSIONED:
            ver = out["ver"][VER_GUARD:VER_GUARD + call.n * vc.VER.itemsize].view(vc.VER)
            r, v = vc.expected(rec, ver, call.expect)
            rec[:], ver[:] = r, v
        else:
            r = oc.expected_records(None, rec, call.expect)
            if call.entry in (BATCH, COW):  # (these two rewrite no input field)
                for f in STATE_IO:
                    r[f] = rec[f]
            rec[:] = r
        if out["info"] is not None:
            out["info"][:] = call.info
        return out


# ---- the checker -----------------------------------------------------------------------------------
def _first_record_diff(got, want, dtype, guard, n):
    g = got[guard:guard + n * dtype.itemsize].view(dtype)
    w = want[guard:guard + n * dtype.itemsize].view(dtype)
    for i in range(n):
        if g[i].tobytes() != w[i].tobytes():
            for f in dtype.names:
                if np.any(g[f][i] != w[f][i]):
                    return i, f, g[f][i], w[f][i]
    return None


def check_call(q, k, got, sent):
    """Call k's record, version and destination buffers (guards included) and d_info."""
    call = q.calls[k]
    what = f"call {k} ({call.entry})"
    want = q.want(k, sent)
    for name, dtype, guard in (("rec", fp.REC, fp.REC_GUARD), ("ver", vc.VER, VER_GUARD),
                               ("dst", np.dtype([("dst", "<u8")]), cc.DST_GUARD)):
        if want[name] is None:
            continue
        g, w = got[name], want[name]
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if np.array_equal(g, w):
            continue
        d = _first_record_diff(g, w, dtype, guard, call.n)
        if d is not None:
            i, f, gv, wv = d
            raise AssertionError(f"{what}: IO {i} (chunk {call.chunk_of[i]}, job {_brief(call.jobs[i])}) {name} field {f}: "
                                 f"got {gv}, want {wv} (status got {_status(got['rec'], i)}, want {call.statuses[i]})")
        pos = int(np.flatnonzero(g != w)[0])
        side = "in front of IO 0" if pos < guard else f"behind IO {call.n - 1}"
        raise AssertionError(f"{what}: {name} guard changed at buffer offset {pos} ({side})")
    if want["info"] is not None:
        assert [int(x) for x in got["info"]] == [int(x) for x in want["info"]], \
            f"{what}: d_info {[int(x) for x in got['info']]}, want {[int(x) for x in want['info']]} (IO count {call.n})"


def _status(recbuf, i):
    return int(recbuf[fp.REC_GUARD + i * fp.REC.itemsize:fp.REC_GUARD + (i + 1) * fp.REC.itemsize].view(fp.REC)[0]["status"])


def _brief(job):
    return {k: v for k, v in job.items() if k not in ("data",)}


def check_queue(q, got_arena, got_pays, got, sent):
    """After the whole queue.  got / sent: per call the dict of Queue.buffers."""
    assert len(got) == len(sent) == len(got_pays) == len(q.calls)
    for k, call in enumerate(q.calls):
        check_call(q, k, got[k], sent[k])
        if not np.array_equal(got_pays[k], call.pay):
            pos = int(np.flatnonzero(got_pays[k] != call.pay)[0])
            raise AssertionError(f"call {k} ({call.entry}): payload image changed at offset {pos} (IO count {call.n})")
    want = q.final_image()
    assert got_arena.shape == want.shape
    if not np.array_equal(got_arena, want):
        d = np.flatnonzero(got_arena != want)
        first, last = int(d[0]), int(d[-1])
        c = fp._chunk_of(q.lay, first) % q.n
        k, i = q.last_writer.get(c, (None, None))
        sizes = None if q.spare else q.sizes
        lives = f" (it lives in region {q.loc[c]})" if q.spare else ""
        raise AssertionError(
            f"chunk arena differs in {d.size} bytes after the queue; first at {first} = {q.lay.where(first, sizes)} "
            f"(got {int(got_arena[first]):#04x}, want {int(want[first]):#04x}), last at {last} = "
            f"{q.lay.where(last, sizes)}; chunk {c}{lives} was last written by call {k} IO {i}")


# ---- traffic -----------------------------------------------------------------------------------------
def _jobs_of(ops):
    out = []
    for op in ops:
        if op[1] == "W":
            out.append(vc.W(op[0], op[2], op[3], 0, flavour=op[4]))
        else:
            out.append((vc.T if op[1] == "T" else vc.E)(op[0], op[2], 0))
    return out


def traffic(q, rng, depths, versioned=False, refuse=0.1, commits=0.2):
    """One call's jobs: ordered_cases' mixed traffic (overwrite, append, gap, truncate, extend, full
    overwrite, NONE-typed writes) down chains of depths[c] jobs, interleaved.  versioned: io_ver
    follows each chunk's update_ver; `commits` of the slots hold a commit instead, `refuse` of the
    updates a version the ladder refuses (stale, committed or missing)."""
    order = oc._interleave(rng, list(depths))
    jobs = _jobs_of(oc._mixed_ops(rng, order, q.max_len, q.sizes))
    if not versioned:
        return jobs
    guess = [m.update_ver for m in q.metas]
    out = []
    for j in jobs:
        c = j["c"]
        if rng.random() < commits:
            out.append(vc.C(c, guess[c]))
            continue
        if rng.random() < refuse:
            j["ver"] = max(1, guess[c] + int(rng.choice([0, 2, -1])))
        else:
            guess[c] += 1
            j["ver"] = guess[c]
        out.append(j)
    return out


def _depths(rng, n_chunks, lo=32, hi=64, deepest=4):
    d = rng.integers(1, deepest + 1, n_chunks)
    while d.sum() < lo:
        d[int(rng.integers(0, n_chunks))] = deepest
    while d.sum() > hi:
        d[int(np.argmax(d))] -= 1
    return [int(x) for x in d]


def _first_write(jobs, pred=lambda j: True):
    return next(i for i, j in enumerate(jobs) if j["k"] == "W" and j["ln"] > 1 and pred(j))


def chain_queue(orc, max_len, versioned=False, ctype=fp.CRC32C, calls=5, n_chunks=16, seed=0x9E0):
    """ordered x5 / versioned x5: 32..64 jobs per call in chains 1..4 deep on 16 chunks, max_rounds 4.
    Call 1 and the last call hold a corrupted client checksum, call 2 a chain of 5 (its last job comes back
    NOT_APPLIED and call 3 resubmits it unchanged, in front), call 3 an INVALID_ARG write.
    versioned: about a tenth of the updates carry a version the ladder refuses, a fifth of the slots
    are commits; call 0 holds a chain-version refusal and call 4 a forced commit."""
    entry = VERSIONED if versioned else ORDERED
    q = Queue(orc, n_chunks, max_len, ctype, seed=seed + max_len + ctype,
              name=f"{entry}_{max_len}_{'crc32c' if ctype == fp.CRC32C else 'crc32'}")
    rng = np.random.default_rng(seed ^ 0x55)
    for c in range(n_chunks):
        if c % 3 == 1:
            q.preset(c, max_len // 4 + c)
    again = []
    for k in range(calls):
        depths = _depths(rng, n_chunks)
        if k == 2:
            depths[5] = 5
        jobs = traffic(q, rng, depths, versioned)
        if k == 0 and versioned:
            jobs[0]["jcv"] = 2  # below the chunk's chain version 3 on a COMMIT chunk
        if k == 1:
            jobs[_first_write(jobs)]["flavour"] = "corrupt"
        if k == 3:
            jobs = again + jobs
            jobs.insert(len(jobs) // 2, vc.W(int(rng.integers(0, n_chunks)), max_len, 4, 1))
        if k == 4 and versioned:
            i = next(i for i, j in enumerate(jobs) if j["k"] == "C")
            jobs[i]["force"] = True
        if k == calls - 1:  # (in the last call: nothing after the queue rewrites what a failed IO must not leave)
            i = max(i for i, j in enumerate(jobs) if j["k"] == "W" and j["ln"] > 1)
            jobs[i]["flavour"] = "corrupt"
        call = q.add(entry, jobs, max_rounds=4)
        again = [dict(j) for j, s in zip(call.jobs, call.statuses) if s == oc.NOT_APPLIED] if k == 2 else again
    return q


class Mixed:
    pass


def mixed_queue(orc, max_len, seed=0x313D):
    """mixed x8 on one pair: ordered -> update_batch -> versioned -> cow -> ordered -> engine ->
    update_batch -> versioned.  Seven calls share one chunk set, every chunk with a spare region:
    the copy-on-write call moves the chunks it writes (an eighth stay in place with entry 0), and
    the calls behind it find them at the destinations.  Chunk-engine
    chunks and replica chunks cannot share bytes (the flavours store different checksums), so the
    engine call has an arena of its own in the same queue.  Four hint words (ordered and versioned
    share one) and every carving of the pair buffer follow each other.
    -> .q (Queue), .e (EngineQueue), .plan: [("q" | "e", call index)] in queue order."""
    n_chunks = 32
    q = Queue(orc, n_chunks, max_len, seed=seed + max_len, name=f"mixed_{max_len}", spare=True)
    rng = np.random.default_rng(seed)
    for c in range(n_chunks):
        if c % 2:
            q.preset(c, 1 + (c * 37) % (max_len // 2))
    for k, entry in enumerate((ORDERED, BATCH, VERSIONED, COW, ORDERED, BATCH, VERSIONED)):
        if entry in (BATCH, COW):
            jobs = traffic(q, rng, [1] * n_chunks)
            jobs[_first_write(jobs)]["flavour"] = "corrupt"
            for j in jobs[3::8]:
                j["place"] = False  # (copy-on-write: destination entry 0; update_batch ignores it)
            q.add(entry, jobs, move=entry == COW)
        else:
            jobs = traffic(q, rng, _depths(rng, n_chunks, deepest=3), entry == VERSIONED)
            if k == 6:
                jobs[max(i for i, j in enumerate(jobs) if j["k"] == "W" and j["ln"] > 1)]["flavour"] = "corrupt"
            q.add(entry, jobs, max_rounds=4)
    m = Mixed()
    m.q, m.e, m.name = q, engine_queue(orc, max_len, calls=1, seed=seed), f"mixed_{max_len}"
    m.plan = [("q", 0), ("q", 1), ("q", 2), ("q", 3), ("q", 4), ("e", 0), ("q", 5), ("q", 6)]
    return m


def density_queue(orc, entry, max_len=128 << 10, n=64, calls=6, seed=0xDE57):
    """density swing x6: calls alternate between piece-poor (truncates and 1-byte writes) and
    piece-rich (writes of the whole max_len), n IOs on n chunks each, so a grid sized from the
    previous call's pieces per IO is wrong in both directions."""
    assert entry in (ORDERED, BATCH)
    q = Queue(orc, n, max_len, seed=seed, name=f"density_{entry}")
    rng = np.random.default_rng(seed + 1)
    for c in range(n):
        q.preset(c, 1000 + 13 * c)
    for k in range(calls):
        sizes = q.sizes
        if k % 2 == 0:
            jobs = [vc.T(c, max(1, sizes[c] // 2), 0) if (c + k) % 3 == 0 else
                    vc.W(c, int(rng.integers(0, max(1, sizes[c]))), 1, 0) for c in range(n)]
        else:
            jobs = [vc.W(c, 0, max_len, 0) for c in range(n)]
        order = rng.permutation(n)
        q.add(entry, [jobs[int(c)] for c in order], max_rounds=1)
    return q


GROWTH_COUNTS = (8, 2048, 32, 2048, 512, 2048)
FIRST_ALLOCATION = 256 << 10   # pair_buffer sizes the call buffer up to a multiple of 64 Ki words


def growth_queue(orc, versioned=False, counts=GROWTH_COUNTS, max_len=4096, seed=0x6120):
    """growth x6: calls of counts[k] jobs in chains of 2 on the first counts[k] / 2 chunks of 4 KiB,
    max_rounds 2.  The second call needs more call scratch than the first one's allocation."""
    entry = VERSIONED if versioned else ORDERED
    n_chunks = max(counts) // 2
    q = Queue(orc, n_chunks, max_len, gap=2048, seed=seed, name=f"growth_{entry}")
    rng = np.random.default_rng(seed + 2)
    for m in counts:
        q.add(entry, traffic(q, rng, [2] * (m // 2) + [0] * (n_chunks - m // 2), versioned), max_rounds=2)
    return q


# ---- copy-on-write -----------------------------------------------------------------------------------
class _MovedLayout:
    """update_footprint.Layout's regions in the order a CowScenario numbers them for one call."""

    def __init__(self, base, perm):
        self.base, self.perm = base, list(perm)
        self.n, self.max_len, self.gap, self.size = base.n, base.max_len, base.gap, base.size
        self.bases = [base.bases[p] for p in perm]

    def where(self, pos, sizes=None):
        return self.base.where(pos)


class CowQueue:
    """Copy-on-write calls of n IOs each, chunk c in region c or n + c: a cow_cases.CowScenario per
    call, numbered so that its source c is where the chunk lives and its destination the other
    region of the pair, started from the bytes, sizes and checksums the last call's model left."""

    engine = False

    def __init__(self, orc, n, max_len, ctype=fp.CRC32C, seed=0xC09, name="cow"):
        self.orc, self.n, self.max_len, self.ctype, self.seed, self.name = orc, n, max_len, ctype, seed, name
        self.phys_lay = fp.Layout(2 * n, max_len, gap=fp.MARGIN)
        self.loc = list(range(n))            # the region chunk c lives in
        self.sizes, self.cks = [0] * n, [(ctype, 0)] * n
        self.phys, self.scns, self.locs = None, [], []

    def other(self, c):
        return c + self.n if self.loc[c] == c else c

    def add(self, ops, presets=()):
        n, k = self.n, len(self.scns)
        scn = cc.CowScenario(self.orc, n, self.max_len, self.ctype, False, rot=0, seed=self.seed + 17 * k)
        perm = [self.loc[c] for c in range(n)] + [self.other(c) for c in range(n)]
        scn.lay = _MovedLayout(self.phys_lay, perm)
        if self.phys is None:
            for c, size in presets:
                scn.preset(c, size)
            self.sizes, self.cks = list(scn.sizes), list(scn.cks)
        else:
            scn.regions = [bytearray(self.phys[p]) for p in perm]
            scn.sizes, scn.cks = list(self.sizes), list(self.cks)
        scn.build(ops)
        r = scn.rounds[0]
        self.locs.append(list(self.loc))
        self.phys = [bytearray(r.image[b:b + self.max_len].tobytes()) for b in self.phys_lay.bases]
        for c, e in enumerate(r.expect):
            if e[0] == fp.OK:
                self.sizes[c], self.cks[c] = e[1], tuple(e[2])
                if r.place[c] == cc.OUT_OF_PLACE:
                    self.loc[c] = self.other(c)
        self.scns.append(scn)
        return scn

    @property
    def arena0(self):
        return self.scns[0].image_before(0)

    def final_image(self):
        return self.scns[-1].image_after(0)

    @property
    def lay(self):
        """Where every chunk lives after the last call (what stream_queue.followup_records reads)."""
        return _MovedLayout(self.phys_lay, self.loc)


def check_cow_queue(q, got_arena, got_pays, got_recs, sent_recs, got_dsts, sent_dsts):
    """After the whole queue: every call's records (update_footprint.check_records), payloads and
    destination array, and the whole arena -- sources, destinations and the canary between."""
    for k, scn in enumerate(q.scns):
        try:
            fp.check_records(scn, 0, got_recs[k], sent_recs[k])
            fp.check_payload(scn, 0, got_pays[k])
        except AssertionError as e:
            raise AssertionError(f"call {k} (cow): {e}") from None
        if not np.array_equal(got_dsts[k], sent_dsts[k]):
            pos = int(np.flatnonzero(got_dsts[k] != sent_dsts[k])[0])
            raise AssertionError(f"call {k} (cow): destination array or its guards changed at buffer offset {pos} "
                                 f"(entry {(pos - cc.DST_GUARD) // 8} of chunk {(pos - cc.DST_GUARD) // 8})")
    want = q.final_image()
    assert got_arena.shape == want.shape
    if not np.array_equal(got_arena, want):
        d = np.flatnonzero(got_arena != want)
        first = int(d[0])
        region = fp._chunk_of(q.phys_lay, first)
        c = region % q.n
        moved = [k for k in range(len(q.scns)) if q.scns[k].rounds[0].place[c] == cc.OUT_OF_PLACE and
                 q.scns[k].rounds[0].expect[c][0] == fp.OK]
        raise AssertionError(
            f"chunk arena differs in {d.size} bytes after the queue; first at {first} = region "
            f"{q.phys_lay.where(first)} (got {int(got_arena[first]):#04x}, want {int(want[first]):#04x}): a region of "
            f"chunk {c}, which lives in region {q.loc[c]} and was moved by call(s) {moved}, last by call "
            f"{moved[-1] if moved else None}")


def _cow_ops(q, rng, k, max_len):
    """One IO per chunk; the kind rotates with the call, so every chunk sees several."""
    ops = []
    for c in range(q.n):
        s = q.sizes[c]
        unit = max(8, max_len // 16)
        ln = int(rng.integers(1, unit))
        pick = (c + 3 * k) % 10 if s else 0
        if pick == 0:      # a gap write (the first write of an empty chunk)
            off = min(s + int(rng.integers(1, unit)), max_len - ln) if s else int(rng.integers(0, unit))
            ops.append(cc._w(off, ln, c % 16))
        elif pick == 1:    # append
            ops.append(cc._w(s, min(ln, max_len - s), c % 16) if s < max_len else dict(kind="T", target=s // 2))
        elif pick in (2, 7):  # overwrite inside
            off = int(rng.integers(0, s))
            ops.append(cc._w(off, min(ln, max_len - off), (c + k) % 16))
        elif pick == 3:
            ops.append(dict(kind="T", target=max(1, s - int(rng.integers(1, max(2, s // 2))))))
        elif pick == 4:
            ops.append(dict(kind="E", target=min(max_len, s + ln)))
        elif pick == 5:    # the whole content rewritten
            ops.append(cc._w(0, min(max_len, s + ln), 5))
        elif pick == 6:    # in place, no destination
            off = int(rng.integers(0, s))
            ops.append(cc._w(off, min(ln, max_len - off), 6, place=cc.IN_PLACE_ZERO))
        elif pick == 8:    # a syncing write: the chunk becomes the payload
            ops.append(cc._w(0, ln, 8, sync=True))
        else:              # a bad payload checksum / an INVALID_ARG IO: the chunk stays where it is
            ops.append(cc._w(1, ln, 9, corrupt=True) if (c // 10) % 2 else cc._w(max_len - 1, 2, 9))
    return ops


def cow_queue(orc, max_len, ctype=fp.CRC32C, n=32, calls=4, seed=0xC09):
    """cow x4: every call moves every chunk it writes successfully and out of place; call k + 1's
    sources are call k's destinations.  Syncing writes, IOs in place with destination entry 0, a
    corrupted client checksum and an INVALID_ARG IO in every call."""
    q = CowQueue(orc, n, max_len, ctype, seed=seed + max_len + ctype,
                 name=f"cow_{max_len}_{'crc32c' if ctype == fp.CRC32C else 'crc32'}")
    rng = np.random.default_rng(seed ^ 0x33)
    presets = [(c, 1 + (c * 37 + 11) % (max_len // 2)) for c in range(n) if c % 4]
    for c, size in presets:
        q.sizes[c] = size
    for k in range(calls):
        q.add(_cow_ops(q, rng, k, max_len), presets if k == 0 else ())
    return q


def cow_density_queue(orc, max_len=128 << 10, n=64, calls=6, seed=0xDE59):
    """density swing x6 for copy-on-write: piece-poor calls (truncates and 1-byte writes) and
    piece-rich ones (the whole max_len rewritten), every IO out of place."""
    q = CowQueue(orc, n, max_len, seed=seed, name="density_cow")
    rng = np.random.default_rng(seed + 1)
    presets = [(c, 1000 + 13 * c) for c in range(n)]
    for c, size in presets:
        q.sizes[c] = size
    for k in range(calls):
        if k % 2 == 0:
            ops = [dict(kind="T", target=max(1, q.sizes[c] // 2)) if (c + k) % 3 == 0 else
                   cc._w(int(rng.integers(0, max(1, q.sizes[c]))), 1, c % 16) for c in range(n)]
        else:
            ops = [cc._w(0, max_len, c % 16) for c in range(n)]
        q.add(ops, presets if k == 0 else ())
    return q


# ---- the chunk engine ----------------------------------------------------------------------------------
JOB_GUARD = 1 << 10
SALT_JOB = 0x2F
ENGINE = "engine"


class EngineQueue:
    """Calls of update_engine on one set of chunk-engine chunks: engine_cases.simulate over ONE
    arena image keyed by address (every committed allocation and every destination of every call,
    MARGIN of canary apart), the chunks' committed and writing state carried from call to call.
    Call k + 1's `chunk` keys are the committed addresses call k left."""

    def __init__(self, orc, n_chunks, max_len, regions, seed=0xE9, name="engine"):
        self.orc, self.n, self.max_len, self.name = orc, n_chunks, max_len, name
        self.lay = fp.Layout(regions, max_len, gap=fp.MARGIN if max_len > 4096 else 2048)
        self.mem = fp.canary(self.lay.size, fp.SALT_CHUNKS)
        self.used = 0
        self.rng = np.random.default_rng(seed)
        self.chunks = [ec.Chunk(self._alloc()) for _ in range(n_chunks)]
        self.calls, self.arena0 = [], None

    def _alloc(self):
        assert self.used < len(self.lay.bases), "more allocations than regions"
        self.used += 1
        return self.lay.bases[self.used - 1]

    def preset(self, c, size):
        assert not self.calls
        data = self.rng.integers(0, 256, size, dtype=np.uint8)
        ch = self.chunks[c]
        self.mem[ch.addr:ch.addr + size] = data
        ch.size, ch.fin = size, self.orc.rs_crc32c(data.tobytes()) if size else 0
        ch.ck = (fp.CRC32C, ec.raw(ch.fin))

    def add(self, jobs, max_rounds):
        if self.arena0 is None:
            self.arena0 = self.mem.copy()
            self.arena0.setflags(write=False)
        orc, n, k = self.orc, len(jobs), len(self.calls)
        jobs = [dict(j) for j in jobs]
        keys = [ch.addr for ch in self.chunks]
        for job in jobs:
            job["dst"] = self._alloc() if job["dst"] else 0
        rec, jr = np.zeros(n, dtype=fp.REC), np.zeros(n, dtype=ec.JOB)
        has_payload = np.zeros(n, dtype=bool)
        placed, first, cur = [], set(), fp.PAY_GUARD
        for i, job in enumerate(jobs):
            c, kind = job["c"], job["k"]
            u, v = rec[i], jr[i]
            u["chunk"] = keys[c]
            u["flags"] = ec.FLAG_ENGINE | (ec.FLAG_SYNCING if job.get("sync") else 0)
            v["io_ver"], v["job_chain_ver"], v["dst"] = job["ver"], job["jcv"], job["dst"]
            if c not in first:
                first.add(c)
                u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = self.chunks[c].io()
                state = self.chunks[c].job()
            else:
                u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = oc.JUNK
                state = ec.JUNK_JOB
            for f, x in zip(ec.BEFORE_FIELDS, state):
                v[f] = x
            for f, x in zip(ec.OUT_FIELDS, ec.JUNK_JOB):
                v[f] = x
            v["out_cow"], v["detail"] = 0x55, 0x66
            if kind == "C":
                u["update_type"], u["offset"], u["length"], u["payload"] = ec.COMMIT_JOB, 0xFFFFFFF0, 77, 0
            elif kind in "TE":
                u["update_type"], u["length"] = (fp.TRUNCATE if kind == "T" else fp.EXTEND), job["ln"]
            else:
                off, ln = int(job["off"]), int(job["ln"])
                data = self.rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
                p = ((cur + 15) & ~15) + (i * 7) % 16
                cur = p + ln + 64
                placed.append((p, data))
                has_payload[i] = True
                u["update_type"], u["offset"], u["length"], u["payload"] = fp.WRITE, off, ln, p
                fin = orc.rs_crc32c(data) ^ (0x100 if job["flavour"] == "corrupt" else 0)
                job["data"], job["wfin"] = data, (None if job["flavour"] == "none" else fin)
                u["write_checksum_type"], u["write_checksum"] = (fp.NONE, 0) if job["flavour"] == "none" else \
                    (fp.CRC32C, ec.raw(fin))
        pay = fp.canary(cur + fp.PAY_GUARD, fp.SALT_PAYLOAD)
        for p, data in placed:
            pay[p:p + len(data)] = np.frombuffer(data, dtype=np.uint8)
        pay.setflags(write=False)
        call = Call()
        call.k, call.entry, call.n, call.max_rounds, call.jobs = k, ENGINE, n, max_rounds, jobs
        call.rec, call.jr, call.has_payload, call.pay = rec, jr, has_payload, pay
        call.chunk_of = [j["c"] for j in jobs]
        call.expect, call.info = ec.simulate(orc, jobs, self.mem, self.chunks, self.max_len, max_rounds)
        call.statuses = [int(e[0]) for e in call.expect]
        self.calls.append(call)
        return call

    def final_image(self):
        return self.mem

    def buffers(self, k, chunk_addr, pay_addr):
        call = self.calls[k]
        rec, jr = call.rec.copy(), call.jr.copy()
        rec["chunk"] += np.uint64(chunk_addr)
        rec["payload"][call.has_payload] += np.uint64(pay_addr)
        for f in ("dst", "addr", "w_addr"):
            nz = jr[f] != 0
            jr[f][nz] += np.uint64(chunk_addr)
        return dict(rec=_guarded(rec, fp.REC_GUARD, fp.SALT_RECORDS), jr=_guarded(jr, JOB_GUARD, SALT_JOB),
                    info=np.full(ec.INFO_WORDS, INFO_FILL, dtype=np.uint32))

    def want(self, k, sent, chunk_addr):
        call = self.calls[k]
        out = {name: b.copy() for name, b in sent.items()}
        rec = out["rec"][fp.REC_GUARD:fp.REC_GUARD + call.n * fp.REC.itemsize].view(fp.REC)
        jr = out["jr"][JOB_GUARD:JOB_GUARD + call.n * ec.JOB.itemsize].view(ec.JOB)
        r, j = ec.expected(rec, jr, call.expect, chunk_addr)
        rec[:], jr[:] = r, j
        out["info"][:] = call.info
        return out


def check_engine_queue(q, chunk_addr, got_arena, got_pays, got, sent):
    """After the whole queue: every call's d_ios, d_jobs (guards included), d_info and payloads, and
    the whole arena: every allocation, every destination used or not, the canary between them."""
    for k, call in enumerate(q.calls):
        what = f"call {k} (engine)"
        want = q.want(k, sent[k], chunk_addr)
        for name, dtype, guard in (("rec", fp.REC, fp.REC_GUARD), ("jr", ec.JOB, JOB_GUARD)):
            g, w = got[k][name], want[name]
            assert g.shape == w.shape
            if np.array_equal(g, w):
                continue
            d = _first_record_diff(g, w, dtype, guard, call.n)
            if d is not None:
                i, f, gv, wv = d
                raise AssertionError(f"{what}: job {i} (chunk {call.chunk_of[i]}, {_brief(call.jobs[i])}) {name} field {f}: "
                                     f"got {gv}, want {wv} (status got {_status(got[k]['rec'], i)}, want {call.statuses[i]})")
            pos = int(np.flatnonzero(g != w)[0])
            raise AssertionError(f"{what}: {name} guard changed at buffer offset {pos} "
                                 f"({'in front of job 0' if pos < guard else f'behind job {call.n - 1}'})")
        assert [int(x) for x in got[k]["info"]] == list(call.info), \
            f"{what}: d_info {[int(x) for x in got[k]['info']]}, want {list(call.info)} (job count {call.n})"
        if not np.array_equal(got_pays[k], call.pay):
            raise AssertionError(f"{what}: payload image changed at offset "
                                 f"{int(np.flatnonzero(got_pays[k] != call.pay)[0])} (job count {call.n})")
    want = q.final_image()
    assert got_arena.shape == want.shape
    if not np.array_equal(got_arena, want):
        d = np.flatnonzero(got_arena != want)
        first = int(d[0])
        region = fp._chunk_of(q.lay, first)
        base = q.lay.bases[region]
        owner = [f"chunk {c} (committed)" for c, ch in enumerate(q.chunks) if ch.addr == base] + \
                [f"chunk {c} (writing)" for c, ch in enumerate(q.chunks) if ch.w is not None and ch.w.addr == base] + \
                [f"call {k} job {i} (chunk {j['c']}) destination" for k, call in enumerate(q.calls)
                 for i, j in enumerate(call.jobs) if j["dst"] == base]
        raise AssertionError(f"chunk arena differs in {d.size} bytes after the queue; first at {first} = region "
                             f"{q.lay.where(first)} (got {int(got_arena[first]):#04x}, want {int(want[first]):#04x}); "
                             f"that region is {', '.join(owner) or 'never used'}")


def engine_queue(orc, max_len, calls=4, n_chunks=32, seed=0xE9C):
    """engine x4: per chunk update, commit, update, commit ... across the queue, one or two jobs per
    chunk and call.  Appends go in place and overwrites copy on write -- the device decides from the
    committed length, every update brings a destination.  Call 1 holds a chain-version refusal,
    call 2 a corrupted client checksum."""
    q = EngineQueue(orc, n_chunks, max_len, regions=n_chunks * (1 + calls), seed=seed + max_len,
                    name=f"engine_{max_len}")
    rng = np.random.default_rng(seed)
    for c in range(n_chunks):
        if c % 2:
            q.preset(c, 1 + (c * 37) % (max_len // 2))
    unit = max(8, max_len // 16)
    for k in range(calls):
        chains = []
        for c in range(n_chunks):
            ch, chain = q.chunks[c], []
            live, size, ver = ch.w is not None, (ch.w.len if ch.w is not None else ch.size), \
                (ch.w.chunk_ver if ch.w is not None else ch.chunk_ver)
            for _ in range(1 + (c + k) % 2):
                if live:
                    chain.append(ec.C(c))
                    live = False
                    continue
                ln = int(rng.integers(1, unit))
                ver += 1
                if size and (c + k + len(chain)) % 3 == 0:      # an overwrite: copy on write
                    chain.append(ec.W(c, int(rng.integers(0, size)), ln, ver))
                elif (c + k) % 7 == 3 and size > 2:              # a shortening truncate: in place
                    chain.append(ec.T(c, size // 2, ver))
                    size //= 2
                else:                                           # an append: in place
                    ln = min(ln, max_len - size) or 1
                    chain.append(ec.W(c, min(size, max_len - ln), ln, ver))
                    size = max(size, min(size, max_len - ln) + ln)
                live = True
            chains.append(chain)
        jobs, order = [], oc._interleave(rng, [len(x) for x in chains])
        take = [0] * n_chunks
        for c in order:
            jobs.append(chains[c][take[c]])
            take[c] += 1
        if k == 1:
            next(j for j in jobs if j["k"] != "C")["jcv"] = 2   # below the chunk's chain version 3
        if k == 2:
            jobs[_first_write(jobs)]["flavour"] = "corrupt"
        q.add(jobs, max_rounds=4)
    return q


# ---- the resync comparison behind a versioned queue ------------------------------------------------------
SYNC_CHAIN_VER = 3


def sync_tables(q, seed=0x5C):
    """A local table taken from the model's final state of a versioned Queue (versions, state,
    length and checksum of every chunk) and a successor's table that lacks two chunks and holds a
    lower chain version for every third: those must be forwarded, none is fatal.
    -> (local, remote, sync_cases.Plan) for hf3fs_crc_sync_plan(chain_ver=SYNC_CHAIN_VER)."""
    local = sc.table(q.n)
    local["id_hi"], local["id_lo"] = 0xC0DE, np.arange(q.n)
    for c, m in enumerate(q.metas):
        r = local[c]
        r["chain_ver"], r["update_ver"], r["commit_ver"] = m.chain_ver, m.update_ver, m.commit_ver
        r["checksum_type"], r["checksum"], r["length"], r["chunk_size"] = m.ck[0], m.ck[1], m.size, q.max_len
        r["chunk_state"], r["recycle_state"] = m.state, m.recycle
    remote = local[np.random.default_rng(seed).permutation(q.n)[:q.n - 2]].copy()
    remote["chunk_size"] = 0
    remote["commit_ver"], remote["chunk_state"] = remote["update_ver"], sc.COMMIT
    remote["chain_ver"][np.arange(remote.size) % 3 == 0] -= 1
    return local, remote, sc.model(local, remote, SYNC_CHAIN_VER)
