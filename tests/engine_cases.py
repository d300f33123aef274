"""Chunk-engine queues (hf3fs_crc_update_engine) and what the reference leaves behind.

A Python model of Engine::update_chunk (src/storage/chunk_engine/src/core/engine.rs:288-468) behind
ChunkEngine::update (src/storage/store/ChunkEngine.cc:15-80) and of Engine::commit_chunk
(engine.rs:470-507) behind ChunkEngine::commit (ChunkEngine.cc:82-110), transcribed with line
citations and driven ONE JOB AT A TIME in index order over host images.  Per chunk the model keeps
the committed state and the writing state; all bytes live in one arena image keyed by address:
every committed allocation, every supplied writing version and every destination, a canary gap
apart.  A copy-on-write job applies oracle.engine_apply to a copy of the committed image and
stores [0, new_len) into the destination's image (the destination's bytes at or beyond new_len
keep their canary); an in-place job applies it to the committed image itself.  Checksums come from
oracle.engine_apply / oracle.rs_crc32c (finalized; the ABI carries raw = ~finalized).  Nothing
here looks at the library.

Used by tests/test_update_engine_model.py (CPU) and tests/test_gpu_update_engine.py (GPU).
"""
import numpy as np

import ordered_cases as oc
import update_footprint as fp

WRITE, REMOVE, TRUNCATE, EXTEND, COMMIT_JOB = 1, 2, 4, 8, 16  # UpdateType (Common.h:51-58)
OK, INVALID_ARG, NOT_APPLIED = 0, 3, 9002
MISSING_UPDATE, COMMITTED_UPDATE, CHECKSUM_MISMATCH, CHAIN_VERSION_MISMATCH = 4007, 4008, 4080, 4081
D_NONE, D_RECORD, D_IN_WRITING, D_NO_DST, D_NO_WRITING = 0, 1, 2, 3, 4  # HF3FS_ENGINE_DETAIL_*
STATUSES = (OK, INVALID_ARG, CHECKSUM_MISMATCH, CHAIN_VERSION_MISMATCH, COMMITTED_UPDATE, MISSING_UPDATE, NOT_APPLIED)
NONE, CRC32C, M32 = fp.NONE, fp.CRC32C, fp.M32
FLAG_ENGINE, FLAG_SYNCING = 1, 2
GUARD = oc.GUARD
GAP = 256 + 16
INFO_WORDS = 8

JOB = np.dtype([("dst", "<u8"), ("addr", "<u8"), ("w_addr", "<u8"), ("out_addr", "<u8"), ("out_w_addr", "<u8"),
                ("io_ver", "<u4"), ("job_chain_ver", "<u4"), ("chain_ver", "<u4"), ("chunk_ver", "<u4"),
                ("w_len", "<u4"), ("w_checksum", "<u4"), ("w_chain_ver", "<u4"), ("w_chunk_ver", "<u4"),
                ("out_chain_ver", "<u4"), ("out_chunk_ver", "<u4"), ("out_w_len", "<u4"), ("out_w_checksum", "<u4"),
                ("out_w_chain_ver", "<u4"), ("out_w_chunk_ver", "<u4"), ("out_cow", "u1"), ("detail", "u1"),
                ("reserved", "u1", (6,))])
assert JOB.itemsize == 104
ADDR_FIELDS = ("dst", "addr", "w_addr", "out_addr", "out_w_addr")
BEFORE_FIELDS = ("addr", "chain_ver", "chunk_ver", "w_addr", "w_len", "w_checksum", "w_chain_ver", "w_chunk_ver")
OUT_FIELDS = tuple("out_" + f for f in BEFORE_FIELDS)
# what later jobs of a chunk carry in the eight state fields (the junk address is never dereferenced)
JUNK_JOB = (0x7EAD0000BEE8, 0xAAAA0001, 0xBBBB0002, 0x7EAD0000F008, 0xCCCC0003, 0xDDDD0004, 0xEEEE0005, 0xFFFF0006)


def raw(fin):
    return (~fin) & M32


class Writing:
    """A writing-list entry (engine.rs:430-455): the version an update left and no commit took yet."""

    def __init__(self, addr, ln, fin, chain_ver, chunk_ver):
        self.addr, self.len, self.fin, self.chain_ver, self.chunk_ver = addr, ln, fin, chain_ver, chunk_ver


class Chunk:
    """The committed ChunkMeta (engine.rs:314-326) as far as the two functions read it, the
    allocation it lies in, and the chunk's writing-list entry."""

    def __init__(self, addr=0, size=0, fin=0, chain_ver=3, chunk_ver=4, w=None):
        self.addr, self.size, self.fin = addr, size, fin
        self.chain_ver, self.chunk_ver, self.w = chain_ver, chunk_ver, w
        self.ck = (CRC32C, raw(fin))  # what the IO record carries; repeated as given by every refusal

    def copy(self):
        c = Chunk(self.addr, self.size, self.fin, self.chain_ver, self.chunk_ver,
                  None if self.w is None else Writing(self.w.addr, self.w.len, self.w.fin, self.w.chain_ver,
                                                      self.w.chunk_ver))
        c.ck = self.ck
        return c

    def io(self):
        return (self.size, self.ck[0], self.ck[1])

    def job(self):
        w = self.w
        return (self.addr, self.chain_ver, self.chunk_ver) + (
            (0, 0, 0, 0, 0) if w is None else (w.addr, w.len, raw(w.fin), w.chain_ver, w.chunk_ver))


# ---- the two functions ------------------------------------------------------------------------------
def record_invalid(job, max_len):
    """Detail 1: the kInvalidArg answers the plain call gives for the record (ChunkReplica.cc:141-146
    bounds, a syncing IO that is not a WRITE at offset 0, a target past the chunk size), a record
    without the ENGINE flag, and update types the call does not take (REMOVE stays on the host)."""
    k = job["k"]
    if not job.get("engine", True) or k == "R":
        return True
    if k == "W":
        if job["off"] >= max_len or job["off"] + job["ln"] > max_len:
            return True
        return bool(job.get("sync")) and job["off"] != 0
    if k in "TE":
        return job["ln"] > max_len or bool(job.get("sync"))
    return k != "C"


def needs_cow(job, size):
    """engine.rs:377-380; the capacity clause never holds (capacity = max_len).  A truncate / extend
    reaches the engine with length 0 (ChunkEngine.cc:49-52)."""
    return bool(job.get("sync")) or (job["k"] == "W" and job["ln"] > 0 and job["off"] < size)


def update_job(orc, mem, ch, job, max_len):
    """Engine::update_chunk for one WRITE / TRUNCATE / EXTEND job on chunk `ch` and the arena `mem`
    (both updated on success, untouched otherwise) -> (status, detail, case, cow, out_size, out_fin)."""
    sync = bool(job.get("sync"))
    refuse = lambda status, detail=D_NONE: (status, detail, 0, 0, None, None)
    if record_invalid(job, max_len):
        return refuse(INVALID_ARG, D_RECORD)
    if job["k"] == "W" and job["ln"] != 0 and job["wfin"] is not None:          # engine.rs:297-311
        if orc.rs_crc32c(job["data"]) != job["wfin"]:                           # (without_checksum: hashed and used)
            return refuse(CHECKSUM_MISMATCH)
    if job["jcv"] < ch.chain_ver:                                               # :340-345
        return refuse(CHAIN_VERSION_MISMATCH)
    v = job["ver"]
    if sync:                                                                    # :347-348
        new_ver = v
    elif v > 0:                                                                 # :349-362
        if v <= ch.chunk_ver:
            return refuse(COMMITTED_UPDATE)
        if v > ((ch.chunk_ver + 1) & M32):
            return refuse(MISSING_UPDATE)
        new_ver = v
    else:                                                                       # :364
        new_ver = (ch.chunk_ver + 1) & M32
    cow = needs_cow(job, ch.size)                                               # :376-380
    if cow and not job["dst"]:
        return refuse(INVALID_ARG, D_NO_DST)
    if ch.w is not None:                                                        # :441-447 (before any byte here)
        return refuse(INVALID_ARG, D_IN_WRITING)
    old = mem[ch.addr:ch.addr + max_len]
    work = bytearray(old.tobytes())
    if job["k"] == "W":
        data = job["data"]
        e = orc.engine_apply(work, ch.size, ch.fin, data, job["off"], max_len, is_syncing=sync, exists=True,
                             data_ck=orc.rs_crc32c(data), with_case=True)
    else:
        e = orc.engine_apply(work, ch.size, ch.fin, b"", job["ln"], max_len, truncate=job["k"] == "T", exists=True,
                             with_case=True)
    assert e[0] == OK, "every refusal was taken above"
    new_len, new_fin, kase = e[1], e[2], e[3]
    if cow:                                                                     # copy_on_write (:381-389)
        mem[job["dst"]:job["dst"] + new_len] = np.frombuffer(bytes(work[:new_len]), dtype=np.uint8)
        where = job["dst"]
    else:                                                                       # safe_write (:391-400)
        mem[ch.addr:ch.addr + max_len] = np.frombuffer(bytes(work), dtype=np.uint8)
        where = ch.addr
    ch.w = Writing(where, new_len, new_fin, job["jcv"], new_ver)                # :425-428, :448-455
    return OK, D_NONE, kase, int(cow), new_len, new_fin


def commit_job(ch, job):
    """ChunkEngine::commit (ChunkEngine.cc:95-99) + Engine::commit_chunk (engine.rs:491-506): the
    writing version the job holds, with chain_ver = commitChainVer, becomes the committed chunk."""
    if ch.w is None:
        return INVALID_ARG, D_NO_WRITING
    w = ch.w
    ch.addr, ch.size, ch.fin, ch.chunk_ver = w.addr, w.len, w.fin, w.chunk_ver
    ch.chain_ver = job["jcv"]                                                   # ChunkEngine.cc:96
    ch.ck = (CRC32C, raw(w.fin))
    ch.w = None
    return OK, D_NONE


def simulate(orc, jobs, mem, chunks, max_len, max_rounds):
    """Apply `jobs` in order to `mem` / `chunks` (both updated).  -> per job (status, case, detail,
    cow, io state before, job state before, io outputs, job state after) and the eight info words."""
    seen, out = {}, []
    info = [0] * INFO_WORDS
    for job in jobs:
        c = job["c"]
        k = seen.get(c, 0)
        seen[c] = k + 1
        ch = chunks[c]
        io0, st0 = ch.io(), ch.job()
        if k >= max_rounds:
            out.append((NOT_APPLIED, 0, D_NONE, 0, io0, st0, io0, st0))
            info[1] += 1
            continue
        if job["k"] == "C":
            status, detail = commit_job(ch, job)
            kase, cow, io1 = 0, 0, ch.io()
        else:
            status, detail, kase, cow, new_len, new_fin = update_job(orc, mem, ch, job, max_len)
            io1 = (new_len, CRC32C, raw(new_fin)) if status == OK else io0      # ChunkEngine.cc:61-66
        if status != OK:
            assert (ch.io(), ch.job()) == (io0, st0), "a failure changes nothing"
        out.append((status, kase, detail, cow, io0, st0, io1, ch.job()))
        if status == OK:
            info[3 if job["k"] == "C" else 2] += 1
            if job["k"] != "C":
                info[5 if cow else 6] += 1
        else:
            info[4] += 1
            info[7] += detail == D_IN_WRITING
    info[0] = max(seen.values()) if seen else 0
    return out, tuple(info)


# ---- job constructors ----------------------------------------------------------------------------------
def W(c, off, ln, ver=0, jcv=3, flavour="", dst=True, **kw):
    return dict(c=c, k="W", off=off, ln=ln, ver=ver, jcv=jcv, flavour=flavour, dst=dst, **kw)


def T(c, target, ver=0, jcv=3, dst=True, **kw):
    return dict(c=c, k="T", ln=target, ver=ver, jcv=jcv, dst=dst, **kw)


def E(c, target, ver=0, jcv=3, dst=True, **kw):
    return dict(c=c, k="E", ln=target, ver=ver, jcv=jcv, dst=dst, **kw)


def C(c, jcv=3, **kw):
    return dict(c=c, k="C", ver=0x600DBAD, jcv=jcv, dst=False, **kw)  # io_ver of a commit is ignored


def R(c, ver=0, jcv=3):
    return dict(c=c, k="R", ver=ver, jcv=jcv, dst=True)


class Built:
    pass


def build(orc, name, n_chunks, max_len, max_rounds, jobs, seed, metas=None, preset=(), writing=None):
    """jobs: dicts from W / T / E / C / R in arrival order (flavour "" | "corrupt" | "none"; dst=False:
    no destination).  metas: {chunk: dict(chain_ver=, chunk_ver=)} for chunks that do not start at
    chain 3 / version 4; preset: {chunk: committed length}; writing: {chunk: (len, chain_ver,
    chunk_ver)} for chunks that start with a live writing version in an allocation of its own."""
    rng = np.random.default_rng(seed)
    jobs = [dict(j) for j in jobs]
    cur = [GUARD]
    regions = []

    def alloc():
        k = len(regions)
        b = ((cur[0] + 15) & ~15) + (k * 5) % 16
        cur[0] = b + max_len + GAP
        regions.append(b)
        return b

    chunks, fill = [], []
    for c in range(n_chunks):
        m = dict((metas or {}).get(c, {}))
        ln = dict(preset).get(c, 0)
        data = rng.integers(0, 256, ln, dtype=np.uint8)
        addr = alloc()
        fill.append((addr, data))
        ch = Chunk(addr, ln, orc.rs_crc32c(data.tobytes()) if ln else 0, m.get("chain_ver", 3), m.get("chunk_ver", 4))
        if writing and c in writing:
            wl, wchain, wver = writing[c]
            wdata = rng.integers(0, 256, wl, dtype=np.uint8)
            waddr = alloc()
            fill.append((waddr, wdata))
            ch.w = Writing(waddr, wl, orc.rs_crc32c(wdata.tobytes()) if wl else 0, wchain, wver)
        chunks.append(ch)
    keys = [ch.addr for ch in chunks]  # `chunk` of the IO record: the committed address at queue time
    size0 = [ch.size for ch in chunks]
    for job in jobs:
        job["dst"] = alloc() if job["dst"] else 0
    arena = fp.canary(cur[0] + GUARD, fp.SALT_CHUNKS)
    for addr, data in fill:
        arena[addr:addr + data.size] = data

    n = len(jobs)
    rec, jr = np.zeros(n, dtype=fp.REC), np.zeros(n, dtype=JOB)
    has_payload = np.zeros(n, dtype=bool)
    placed, first, pcur = [], set(), GUARD
    for i, job in enumerate(jobs):
        c, k = job["c"], job["k"]
        u, v = rec[i], jr[i]
        u["chunk"] = keys[c]
        u["flags"] = (FLAG_ENGINE if job.get("engine", True) else 0) | (FLAG_SYNCING if job.get("sync") else 0)
        v["io_ver"], v["job_chain_ver"], v["dst"] = job["ver"], job["jcv"], job["dst"]
        if c not in first:  # the chunk's first job carries the state; the later ones junk
            first.add(c)
            u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = chunks[c].io()
            state = chunks[c].job()
        else:
            u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = oc.JUNK
            state = JUNK_JOB
        for f, x in zip(BEFORE_FIELDS, state):
            v[f] = x
        for f, x in zip(OUT_FIELDS, JUNK_JOB):  # outputs are SET by the call
            v[f] = x
        v["out_cow"], v["detail"] = 0x55, 0x66
        job["stale_cow"] = k != "C" and needs_cow(job, size0[c])  # the decision a host would make at queue time
        if k == "C":  # payload, offset and length of a commit job are ignored: junk
            u["update_type"], u["offset"], u["length"], u["payload"] = COMMIT_JOB, 0xFFFFFFF0, 77, 0
        elif k == "R":
            u["update_type"] = REMOVE
        elif k in "TE":
            u["update_type"], u["length"] = (TRUNCATE if k == "T" else EXTEND), job["ln"]
        else:
            off, ln = int(job["off"]), int(job["ln"])
            data = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
            p = ((pcur + 15) & ~15) + (i * 7) % 16
            pcur = p + ln + 64
            placed.append((p, data))
            has_payload[i] = True
            u["update_type"], u["offset"], u["length"], u["payload"] = WRITE, off, ln, p
            fin = orc.rs_crc32c(data)
            if job["flavour"] == "corrupt":
                fin ^= 0x100
            job["data"], job["wfin"] = data, (None if job["flavour"] == "none" else fin)
            if job["flavour"] == "none":  # ChunkEngine.cc:43-45: without_checksum
                u["write_checksum_type"], u["write_checksum"] = NONE, 0
            else:
                u["write_checksum_type"], u["write_checksum"] = CRC32C, raw(fin)
    pay = fp.canary(pcur + GUARD, fp.SALT_PAYLOAD)
    for p, data in placed:
        pay[p:p + len(data)] = np.frombuffer(data, dtype=np.uint8)

    b = Built()
    b.name, b.n, b.n_chunks, b.max_len, b.max_rounds = name, n, n_chunks, max_len, max_rounds
    b.ctype, b.keys, b.regions, b.jobs = CRC32C, keys, regions, jobs
    b.rec, b.jr, b.has_payload, b.pay, b.arena0 = rec, jr, has_payload, pay, arena.copy()
    b.chunks0 = [ch.copy() for ch in chunks]
    mem = arena.copy()
    b.expect, b.info = simulate(orc, jobs, mem, chunks, max_len, max_rounds)
    b.arena1, b.chunks1 = mem.copy(), [ch.copy() for ch in chunks]
    b.again = None
    if b.info[1]:  # the NOT_APPLIED jobs resubmitted unchanged (as the call returns them)
        a = Built()
        a.idx = [i for i, e in enumerate(b.expect) if e[0] == NOT_APPLIED]
        a.n, a.max_len, a.max_rounds = len(a.idx), max_len, max_rounds
        chunks2 = [ch.copy() for ch in chunks]
        a.expect, a.info = simulate(orc, [jobs[i] for i in a.idx], mem, chunks2, max_len, max_rounds)
        a.arena1, a.chunks1 = mem.copy(), chunks2
        b.again = a
    return b


def truncated(orc, b, n):
    """What the first n jobs of case `b` alone leave (expect, info, arena1)."""
    t = Built()
    mem = b.arena0.copy()
    t.expect, t.info = simulate(orc, b.jobs[:n], mem, [ch.copy() for ch in b.chunks0], b.max_len, b.max_rounds)
    t.arena1 = mem
    return t


def record_arrays(b, arena_addr, pay_addr):
    """The two arrays with absolute addresses: `chunk` and every non-zero address field of the
    job records move by arena_addr (junk included: never dereferenced), payloads by pay_addr."""
    rec, jr = b.rec.copy(), b.jr.copy()
    rec["chunk"] += np.uint64(arena_addr)
    rec["payload"][b.has_payload] += np.uint64(pay_addr)
    for f in ("dst", "addr", "w_addr"):
        nz = jr[f] != 0
        jr[f][nz] += np.uint64(arena_addr)
    return rec, jr


def expected(sent_rec, sent_jr, expect, arena_addr):
    """The two arrays the call must leave: the sent ones with the output fields and, for every
    job, the input state fields it started from."""
    rec, jr = sent_rec.copy(), sent_jr.copy()
    lift = lambda f, x: (x + arena_addr if x else 0) if f.endswith("addr") else x
    for i, (status, kase, detail, cow, io0, st0, io1, st1) in enumerate(expect):
        rec["status"][i], rec["checksum_case"][i] = status, kase
        rec["chunk_size"][i], rec["chunk_checksum_type"][i], rec["chunk_checksum"][i] = io0
        rec["out_size"][i], rec["out_checksum_type"][i], rec["out_checksum"][i] = io1
        for f, x in zip(BEFORE_FIELDS, st0):
            jr[f][i] = lift(f, x)
        for f, x in zip(OUT_FIELDS, st1):
            jr[f][i] = lift(f, x)
        jr["out_cow"][i], jr["detail"][i] = cow, detail
    return rec, jr


# ---- the reference's own sequences (tests/golden/engine_queue_vectors.json) ------------------------------
def golden_queue(orc, seq, seed=0x601D):
    """One chunk and the job list of a golden sequence -> Built (payload bytes are drawn here: the
    vectors assert lengths, versions and statuses, not bytes)."""
    jobs = []
    for s in seq["jobs"]:
        if s["k"] == "C":
            jobs.append(C(0, s["chain_ver"]))
        else:
            jobs.append(W(0, s["offset"], s["length"], s["update_ver"], s["chain_ver"],
                          flavour="none" if s.get("without_checksum") else "", sync=bool(s.get("is_syncing")),
                          dst=True))
    init = seq["chunk"]
    b = build(orc, seq["name"], 1, seq["max_len"], len(jobs), jobs, seed,
              metas={0: dict(chain_ver=init["chain_ver"], chunk_ver=init["chunk_ver"])}, preset={0: init["len"]})
    return b


# ---- the cases -----------------------------------------------------------------------------------------
def singles(orc, max_len):
    """One job per chunk: every status and detail, the precedence pairs, version assignment, a
    syncing write at versions that wrap, truncate and extend in place."""
    q = max(8, max_len // 8)
    J, M, Wr, P, tags = [], {}, {}, {}, []

    def add(tag, job_of, meta=None, size=None, writing=None):
        c = len(tags)
        tags.append(tag)
        if meta is not None:
            M[c] = meta
        P[c] = q // 2 + c if size is None else size
        if writing is not None:
            Wr[c] = writing
        J.append(job_of(c))

    hi = dict(chain_ver=9)           # job_chain_ver 3 < 9
    live = (q, 3, 5)                 # a supplied writing version
    add("u_ok_append", lambda c: W(c, P[c], q, 5))
    add("u_ok_overwrite_cow", lambda c: W(c, 1, q, 5))
    add("u_ok_assign", lambda c: W(c, 3, q, 0))
    add("u_ok_none_write", lambda c: W(c, 0, q, 5, flavour="none"))
    add("u_ok_empty_chunk", lambda c: W(c, 0, q, 1, jcv=7, dst=False), dict(chain_ver=7, chunk_ver=0), size=0)
    add("u_ok_gap", lambda c: W(c, P[c] + 9, q, 5, dst=False))
    add("u_ok_len0_inside", lambda c: W(c, 2, 0, 5, dst=False))
    add("u_no_engine_flag", lambda c: W(c, 0, q, 5, engine=False))
    add("u_remove", lambda c: R(c))
    add("u_bounds", lambda c: W(c, max_len, 4, 5))
    add("u_4080", lambda c: W(c, 0, q, 5, flavour="corrupt"))
    add("u_4081", lambda c: W(c, 0, q, 5), hi)
    add("u_4008", lambda c: W(c, 0, q, 4))
    add("u_4008_lower", lambda c: W(c, 0, q, 2))
    add("u_4007", lambda c: W(c, 0, q, 6))
    add("u_no_dst", lambda c: W(c, 0, q, 5, dst=False))
    add("u_in_writing", lambda c: W(c, 0, q, 5), writing=live)
    add("u_in_writing_append", lambda c: W(c, P[c], q, 5, dst=False), writing=live)
    add("u_truncate_in_place", lambda c: T(c, 5, 5, dst=False))
    add("u_truncate_grow", lambda c: T(c, P[c] + 40, 5))
    add("u_extend_in_place", lambda c: E(c, P[c] + q, 5, jcv=4, dst=False))
    add("u_extend_shorter_noop", lambda c: E(c, 3, 5))
    add("u_truncate_4007", lambda c: T(c, 0, 9))
    add("u_sync_wraps", lambda c: W(c, 0, q, 0, sync=True), dict(chunk_ver=M32))
    add("u_sync_any_version", lambda c: W(c, 0, q + 3, 40, sync=True, jcv=5))
    add("u_sync_len0", lambda c: W(c, 0, 0, 2, sync=True))
    add("u_sync_no_dst", lambda c: W(c, 0, q, 2, sync=True, dst=False))
    add("u_sync_offset", lambda c: W(c, 1, q, 2, sync=True))
    add("u_assign_wraps", lambda c: W(c, P[c], q, 0, dst=False), dict(chunk_ver=M32))
    add("u_top_version", lambda c: W(c, P[c], q, M32, dst=False), dict(chunk_ver=M32 - 1))
    # precedence
    add("p_record_over_4080", lambda c: W(c, max_len - 1, 2, 5, flavour="corrupt"))
    add("p_4080_over_4081", lambda c: W(c, 0, q, 5, flavour="corrupt"), hi)
    add("p_4080_over_4008", lambda c: W(c, 0, q, 4, flavour="corrupt"))
    add("p_4080_over_4007", lambda c: W(c, 0, q, 6, flavour="corrupt"))
    add("p_4080_over_in_writing", lambda c: W(c, 0, q, 5, flavour="corrupt"), writing=live)
    add("p_4080_over_no_dst", lambda c: W(c, 0, q, 5, flavour="corrupt", dst=False))
    add("p_4081_over_4008", lambda c: W(c, 0, q, 4), hi)
    add("p_4007_over_no_dst", lambda c: W(c, 0, q, 6, dst=False))
    add("p_no_dst_over_in_writing", lambda c: W(c, 0, q, 5, dst=False), writing=live)
    add("p_none_write_4008", lambda c: W(c, 0, q, 4, flavour="none"))
    # commits
    add("c_ok_supplied_writing", lambda c: C(c, jcv=8), writing=(q + 7, 3, 5))
    add("c_ok_lower_chain", lambda c: C(c, jcv=1), hi, writing=(0, 9, 5))
    add("c_none", lambda c: C(c))
    n = len(tags)
    b = build(orc, f"singles_{max_len}", n, max_len, 2, J, 0xE51A, metas=M, preset=P, writing=Wr)
    b.tags = tags
    return b


def _mix(J, seed):
    """Interleave the chains of J, keeping each chunk's own order."""
    order = np.random.default_rng(seed).permutation(len(J))
    by_chunk = {}
    for j in J:
        by_chunk.setdefault(j["c"], []).append(j)
    take = {c: 0 for c in by_chunk}
    mixed = []
    for x in order:
        c = J[int(x)]["c"]
        mixed.append(by_chunk[c][take[c]])
        take[c] += 1
    return mixed


def chains(orc, max_len):
    """The queues the call exists for, one chunk each, interleaved in arrival order."""
    q = max(8, max_len // 16)
    J = []
    # 0: U C eight deep, appends (in place) and overwrites (copy on write) alternating: the committed
    #    address moves twice and the third append lands in a former dst
    s = q + 5
    for k in range(4):
        if k % 2 == 0:
            J += [W(0, s, q, 5 + k, jcv=3 + k), C(0, jcv=3 + k)]
            s += q
        else:
            J += [W(0, k, q, 0, jcv=3 + k), C(0, jcv=3 + k)]
    # 1: U U C: the second U is "in writing" and the commit commits the first
    J += [W(1, 0, q, 5), W(1, q, q, 5, dst=False), C(1)]
    # 2: a bad-payload U then a good U: the second is admitted, nothing is in writing
    J += [W(2, 0, q, 5, flavour="corrupt"), W(2, 0, q, 5), C(2)]
    # 3: C first, on a supplied writing version, then the chain goes on from what it committed
    J += [C(3, jcv=6), W(3, 2 * q, q, 8, jcv=6, dst=False), W(3, 0, q, 7, jcv=5), C(3, jcv=7)]
    # 4: C with none, then a U and its C, then C with none again
    J += [C(4), W(4, 0, q, 5), C(4), C(4)]
    # 5: a shortening truncate, its commit, then a write inside the old but past the new length: in
    #    place by the true state (a host deciding from the queue-time length would copy)
    J += [T(5, q, 5, dst=False), C(5), W(5, 2 * q, q, 6, dst=False), C(5)]
    # 6: append, commit, then a write at the old end: copy-on-write by the true length, in place by the stale one
    J += [W(6, 3 * q, q, 5, dst=False), C(6), W(6, 3 * q, q, 6), C(6)]
    # 7: a copy-on-write whose old committed allocation readers still rely on (never committed here)
    J += [W(7, q, 2 * q, 5)]
    # 8: an update met by a supplied writing version, its commit, then the update again
    J += [W(8, 0, q, 5), C(8, jcv=4), W(8, 0, q, 6, jcv=4), W(8, 0, q, 7, jcv=4)]
    # 9: a syncing write over a longer chunk, committed, then an append to the synced length
    J += [W(9, 0, q, 30, sync=True, jcv=5), C(9, jcv=5), W(9, q, q, 31, jcv=5, dst=False), C(9, jcv=5)]
    preset = {0: q + 5, 1: 0, 2: 2 * q, 3: q, 4: 0, 5: 4 * q, 6: 3 * q, 7: 4 * q, 8: q, 9: 5 * q}
    writing = {3: (2 * q, 3, 7), 8: (q + 1, 3, 5)}
    return build(orc, f"chains_{max_len}", 10, max_len, 8, _mix(J, 0xC4A2), 0xC4A2, preset=preset, writing=writing)


def overflow(orc, max_len, chains_n=6):
    """Chains of 5 under max_rounds 3 (append, commit, overwrite | bad write, commit, append): two
    jobs per chain come back NOT_APPLIED with committed and writing state after the third."""
    rng = np.random.default_rng(0x0F12)
    order = oc._interleave(rng, [5] * chains_n)
    q = max(8, max_len // 8)
    step, J = {}, []
    for c in order:
        k = step.get(c, 0)
        step[c] = k + 1
        J.append([W(c, 0, q + c, 5), C(c), W(c, 1, q, 6, flavour="corrupt" if c % 2 else ""),
                  C(c, jcv=4), W(c, q + c, q, 6 if c % 2 else 7, jcv=4, dst=bool(c % 2))][k])
    return build(orc, f"overflow_{max_len}", chains_n, max_len, 3, J, 0x0F12)


def random_queue(orc, max_len, seed, n_chunks=64, depth_max=8):
    """64 chunks, up to 8 jobs each: every job kind, both payload verdicts, versions that are mostly
    right and sometimes committed or missing, commits with and without a writing version, missing
    destinations, supplied writing versions."""
    rng = np.random.default_rng(seed)
    depths = [int(rng.integers(1, depth_max + 1)) for _ in range(n_chunks)]
    depths[0] = depth_max
    while sum(depths) > 256:  # n <= 256
        depths[1 + int(np.argmax(depths[1:]))] -= 1
    order = oc._interleave(rng, depths)
    M, Wr = {}, {}
    unit = max(8, max_len // 8)
    preset = {c: 1 + (c * 37) % (max_len // 2) for c in range(n_chunks) if c % 2}
    for c in range(n_chunks):
        M[c] = dict(chain_ver=int(rng.integers(2, 5)), chunk_ver=int(rng.integers(0, 6)))
        if rng.integers(0, 8) == 0:
            Wr[c] = (int(rng.integers(0, unit)), M[c]["chain_ver"], M[c]["chunk_ver"] + 1)
    ver = {c: M[c]["chunk_ver"] for c in M}      # what a well-behaved client would expect
    live = {c: c in Wr for c in M}
    J = []
    for c in order:
        pick = int(rng.integers(0, 16))
        jcv = int(rng.integers(2, 6))
        ln = int(rng.integers(1, unit))
        off = int(rng.integers(0, max_len - ln))
        slip = int(rng.choice([1, 1, 1, 1, 1, 0, 2]))
        dst = bool(rng.integers(0, 3))
        if live[c] and rng.integers(0, 4):
            pick = 12  # mostly a commit follows an update
        if pick < 7:
            flavour = "corrupt" if rng.integers(0, 5) == 0 else ("none" if rng.integers(0, 8) == 0 else "")
            J.append(W(c, off, ln, max(0, ver[c] + slip), jcv, flavour, dst=dst))
            live[c] = True
        elif pick == 7:
            J.append(W(c, off, ln, 0, jcv, dst=dst))
            live[c] = True
        elif pick == 8:
            J.append(T(c, int(rng.integers(0, max_len)), ver[c] + 1, jcv, dst=dst))
            live[c] = True
        elif pick == 9:
            J.append(E(c, int(rng.integers(0, max_len + 2)), ver[c] + 1, jcv, dst=dst))
            live[c] = True
        elif pick < 14:
            J.append(C(c, jcv))
            ver[c] += int(live[c])
            live[c] = False
        elif pick == 14:
            J.append(W(c, 0, ln, ver[c] + 5, jcv, sync=True, dst=dst))
            ver[c] += 4
            live[c] = True
        else:
            J.append(R(c) if rng.integers(0, 2) else W(c, off, ln, ver[c] + 1, jcv, engine=False))
    return build(orc, f"random_{max_len}_{seed:x}", n_chunks, max_len, depth_max, J, seed, metas=M, preset=preset,
                 writing=Wr)


def distinct(orc, max_len, n=48):
    """All chunks distinct, no commits, no writing state, admitting versions: what
    hf3fs_crc_update_cow_batch does with the same records when the host chooses d_dst by the rule."""
    rng = np.random.default_rng(0xD157)
    unit = max(8, max_len // 8)
    J = []
    preset = {c: int(rng.integers(0, max_len // 2)) for c in range(n) if c % 4}
    for c in range(n):
        ln = int(rng.integers(0, unit))
        off = int(rng.integers(0, max_len - ln))
        kind = c % 8
        if kind == 6:
            J.append(T(c, int(rng.integers(0, max_len)), 5))
        elif kind == 7:
            J.append(E(c, int(rng.integers(0, max_len)), 0))
        elif kind == 5:
            J.append(W(c, 0, ln, 9, sync=True))
        else:
            J.append(W(c, off, ln, 5, flavour="none" if c % 5 == 0 else ("corrupt" if c % 11 == 3 else "")))
    return build(orc, f"distinct_{max_len}", n, max_len, 1, J, 0xD157, preset=preset)


SIZES = (512, 128 << 10)
SEEDS = (0xE7A1, 0xE7A2, 0xE7A3)


def all_cases(orc):
    """name -> builder: every case the GPU tests run (built on demand; the model test builds all)."""
    out = {}
    for ml in SIZES:
        out[f"singles_{ml}"] = lambda ml=ml: singles(orc, ml)
        out[f"chains_{ml}"] = lambda ml=ml: chains(orc, ml)
        out[f"overflow_{ml}"] = lambda ml=ml: overflow(orc, ml)
        out[f"distinct_{ml}"] = lambda ml=ml: distinct(orc, ml)
        for s in SEEDS:
            out[f"random_{ml}_{s:x}"] = lambda ml=ml, s=s: random_queue(orc, ml, s)
    return out
