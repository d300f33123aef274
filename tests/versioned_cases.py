"""Versioned update queues (hf3fs_crc_update_versioned) and what the reference leaves behind.

A Python model of the part of ChunkReplica::update that decides whether a job may run at all
(src/storage/store/ChunkReplica.cc:132-245) and of ChunkReplica::commit (:397-467): the two
ladders transcribed with line citations and driven ONE JOB AT A TIME in index order over host
images of the chunks -- the serialisation the reference gets from the chunk lock.  Bytes, sizes
and checksums come from the oracle calls tests/ordered_cases.py uses (oracle.replica_apply,
oracle.create); a syncing write is restated as in tests/cow_cases.py.  Nothing here looks at
the library.

Used by tests/test_update_versioned_model.py (CPU) and tests/test_gpu_update_versioned.py (GPU).
"""
import numpy as np

import ordered_cases as oc
import update_footprint as fp

WRITE, REMOVE, TRUNCATE, EXTEND, COMMIT_JOB = 1, 2, 4, 8, 16  # UpdateType (Common.h:51-58)
COMMIT, DIRTY, CLEAN = 0, 1, 2                                # ChunkState (Common.h:60-64)
OK, INVALID_ARG, NOT_APPLIED = 0, 3, 9002
NOT_CLEAN, STALE_UPDATE, MISSING_UPDATE, COMMITTED_UPDATE = 4005, 4006, 4007, 4008  # StatusCodeDetails.h:155-158
ADVANCE_UPDATE, SIZE_MISMATCH, STALE_COMMIT = 4012, 4015, 4023                      # :162,165,172
CHECKSUM_MISMATCH, CHAIN_VERSION_MISMATCH, CHUNK_VERSION_MISMATCH = 4080, 4081, 4082  # :186-188
UPDATE_CODES = (INVALID_ARG, SIZE_MISMATCH, NOT_CLEAN, CHAIN_VERSION_MISMATCH, CHECKSUM_MISMATCH, COMMITTED_UPDATE,
                STALE_UPDATE, MISSING_UPDATE, ADVANCE_UPDATE, OK)
COMMIT_CODES = (INVALID_ARG, CHAIN_VERSION_MISMATCH, CHUNK_VERSION_MISMATCH, NOT_CLEAN, STALE_COMMIT, OK)
FATAL = (CHECKSUM_MISMATCH, CHAIN_VERSION_MISMATCH, CHUNK_VERSION_MISMATCH)
NONE, CRC32C, M32 = fp.NONE, fp.CRC32C, fp.M32
FLAG_ENGINE, FLAG_SYNCING = 1, 2
GUARD = oc.GUARD

VER = np.dtype([("io_ver", "<u4"), ("job_chain_ver", "<u4"), ("chain_ver", "<u4"), ("update_ver", "<u4"),
                ("commit_ver", "<u4"), ("meta_chunk_size", "<u4"), ("chunk_state", "u1"), ("recycle_state", "u1"),
                ("is_force", "u1"), ("reserved0", "u1"), ("out_chain_ver", "<u4"), ("out_update_ver", "<u4"),
                ("out_commit_ver", "<u4"), ("out_chunk_state", "u1"), ("out_recycle_state", "u1"),
                ("reserved1", "u1", (2,)), ("reserved2", "<u4")])
assert VER.itemsize == 48
STATE_FIELDS = ("chain_ver", "update_ver", "commit_ver", "meta_chunk_size", "chunk_state", "recycle_state")
JUNK_VER = (0xAAAA0001, 0xBBBB0002, 0xCCCC0003, 0xDDDD0004, 7, 9)  # what later jobs carry in the six state fields
INFO_WORDS = 8


class Meta:
    """ChunkMetadata as far as the two functions read it (Common.h:652-677)."""

    def __init__(self, size=0, ck=(CRC32C, 0), chain_ver=3, update_ver=4, commit_ver=4, state=COMMIT, recycle=0,
                 meta_chunk_size=None):
        self.size, self.ck = size, tuple(ck)
        self.chain_ver, self.update_ver, self.commit_ver = chain_ver, update_ver, commit_ver
        self.state, self.recycle, self.meta_chunk_size = state, recycle, meta_chunk_size

    def copy(self):
        return Meta(self.size, self.ck, self.chain_ver, self.update_ver, self.commit_ver, self.state, self.recycle,
                    self.meta_chunk_size)

    def ver(self):
        return (self.chain_ver, self.update_ver, self.commit_ver, self.meta_chunk_size, self.state, self.recycle)

    def io(self):
        return (self.size, self.ck[0], self.ck[1])


# ---- the two ladders ---------------------------------------------------------------------------------
def record_invalid(job, max_len):
    """The kInvalidArg answers that come before any metadata is read: ChunkReplica.cc:141-146 and
    the ABI's own (a syncing IO that is not a WRITE at offset 0, a target past the chunk size, an
    update type the call does not take, chunk-engine jobs)."""
    k = job["k"]
    if job.get("engine") or k == "R":
        return True
    if k == "W":
        if job["off"] >= max_len or job["off"] + job["ln"] > max_len:  # :141-142
            return True
        return bool(job.get("sync")) and job["off"] != 0
    if k in "TE":
        return job["ln"] > max_len or bool(job.get("sync"))
    return k != "C"


def update_job(orc, chunk, m, job, max_len):
    """ChunkReplica::update for one WRITE / TRUNCATE / EXTEND job on metadata `m` and bytes `chunk`
    (both updated on success, untouched otherwise) -> (status, checksum case)."""
    sync = bool(job.get("sync"))
    if record_invalid(job, max_len):                                    # :141-146
        return INVALID_ARG, 0
    if m.meta_chunk_size != max_len:                                    # :176
        return SIZE_MISMATCH, 0
    if m.state == DIRTY and not sync:                                   # :181
        return NOT_CLEAN, 0
    if job["jcv"] < m.chain_ver and m.state == COMMIT:                  # :186
        return CHAIN_VERSION_MISMATCH, 0
    if job["k"] == "W" and job["wck"][0] != NONE and job["ln"] != 0:    # :193-207
        if tuple(orc.create(job["wck"][0], job["data"])) != tuple(job["wck"]):
            return CHECKSUM_MISMATCH, 0
    v = job["ver"]
    update_ver, commit_ver, recycle = m.update_ver, m.commit_ver, m.recycle
    if sync:                                                            # :211-215
        update_ver, commit_ver, recycle = v, (v - 1) & M32, 0
    elif v > 0:                                                         # :216-231
        if v <= m.commit_ver:
            return COMMITTED_UPDATE, 0
        if v <= m.update_ver:
            return STALE_UPDATE, 0
        if v > ((m.update_ver + 1) & M32):
            return MISSING_UPDATE, 0
        update_ver = v
    else:                                                               # :232-239
        update_ver = (m.update_ver + 1) & M32
        if update_ver > ((m.commit_ver + 1) & M32):
            return ADVANCE_UPDATE, 0
    # :241-304: the write itself, then CLEAN
    if job["k"] == "W" and sync:  # meta.size = writeIO.length (:289), updateChecksum with it (:334-339,392)
        ln, wck = job["ln"], job["wck"]
        chunk[:ln] = job["data"]
        if wck[0] == NONE or ln == 0:
            e = (OK, ln, (wck[0], 0), 1)
        else:
            e = (OK, ln, (wck[0], tuple(orc.create(wck[0], job["data"]))[1]), 2)
    elif job["k"] == "W":
        e = orc.replica_apply(chunk, m.size, m.ck, WRITE, job["off"], job["ln"], job["data"], job["wck"],
                              chunk_size=max_len, with_case=True)
    else:
        e = orc.replica_apply(chunk, m.size, m.ck, TRUNCATE if job["k"] == "T" else EXTEND, 0, job["ln"],
                              with_case=True)
    assert e[0] == OK, "every refusal was taken above"
    m.size, m.ck = e[1], tuple(e[2])
    m.update_ver, m.commit_ver, m.recycle = update_ver, commit_ver, recycle
    m.state, m.chain_ver = CLEAN, job["jcv"]                            # :242,304
    return OK, e[3]


def commit_job(m, job):
    """ChunkReplica::commit for one job on metadata `m` (updated on success) -> status."""
    if job.get("engine") or m.recycle != 0:  # (readyToRemove: store.remove, :458 -- left to the host)
        return INVALID_ARG
    if job["jcv"] < m.chain_ver:                                        # :419
        return CHAIN_VERSION_MISMATCH
    if job["ver"] > m.update_ver:                                       # :425
        return CHUNK_VERSION_MISMATCH
    if job.get("force"):                                                # :432-434
        m.state, m.commit_ver = CLEAN, job["ver"]
    elif m.state == DIRTY:                                              # :435-439
        return NOT_CLEAN
    elif m.commit_ver < job["ver"]:                                     # :440-441
        m.commit_ver = job["ver"]
    else:                                                               # :442-448
        return STALE_COMMIT
    if m.commit_ver == m.update_ver:                                    # :451-454
        m.state, m.chain_ver = COMMIT, job["jcv"]
    return OK


def simulate(orc, jobs, chunks, metas, max_len, max_rounds):
    """Apply `jobs` in order to `chunks` / `metas` (both updated).  -> per job (status, case,
    io state before, ver state before, io state after, ver state after) and the eight info words."""
    seen, out = {}, []
    info = [0] * INFO_WORDS
    for job in jobs:
        c = job["c"]
        k = seen.get(c, 0)
        seen[c] = k + 1
        m = metas[c]
        before_io, before_ver = m.io(), m.ver()
        if k >= max_rounds:
            out.append((NOT_APPLIED, 0, before_io, before_ver, before_io, before_ver))
            info[1] += 1
            continue
        if job["k"] == "C":
            status, kase = commit_job(m, job), 0
        else:
            status, kase = update_job(orc, chunks[c], m, job, max_len)
        if status != OK:
            assert (m.io(), m.ver()) == (before_io, before_ver), "a failure changes nothing"
        out.append((status, kase, before_io, before_ver, m.io(), m.ver()))
        if status == OK:
            info[3 if job["k"] == "C" else 2] += 1
        else:
            info[4] += 1
            info[5] += status in FATAL
            info[6] += job["k"] == "C" and status == NOT_CLEAN
            info[7] += job["k"] == "C" and status == STALE_COMMIT
    info[0] = max(seen.values()) if seen else 0
    return out, tuple(info)


# ---- job constructors ----------------------------------------------------------------------------------
def W(c, off, ln, ver, jcv=3, flavour="", **kw):
    return dict(c=c, k="W", off=off, ln=ln, ver=ver, jcv=jcv, flavour=flavour, **kw)


def T(c, target, ver, jcv=3, **kw):
    return dict(c=c, k="T", ln=target, ver=ver, jcv=jcv, **kw)


def E(c, target, ver, jcv=3, **kw):
    return dict(c=c, k="E", ln=target, ver=ver, jcv=jcv, **kw)


def C(c, ver, jcv=3, force=False, **kw):
    return dict(c=c, k="C", ver=ver, jcv=jcv, force=force, **kw)


def R(c, ver=0, jcv=3):
    return dict(c=c, k="R", ver=ver, jcv=jcv)


class Built:
    pass


def build(orc, name, n_chunks, max_len, max_rounds, jobs, seed, metas=None, preset=(), ctype=CRC32C, stride=None):
    """jobs: dicts from W / T / E / C / R in arrival order (flavour "" | "corrupt" | "none").
    metas: {chunk: Meta(...)} for chunks that do not start as an empty COMMIT chunk at versions 4/4,
    chain 3; preset: chunks that start with content."""
    rng = np.random.default_rng(seed)
    stride = stride or max_len + 256 + 16
    bases, arena_size = oc._layout(n_chunks, max_len, stride)
    arena = fp.canary(arena_size, fp.SALT_CHUNKS)
    state = []
    for c in range(n_chunks):
        m = (metas or {}).get(c, Meta()).copy()
        if m.meta_chunk_size is None:
            m.meta_chunk_size = max_len
        ln = dict(preset).get(c, 0)
        data = rng.integers(0, 256, ln, dtype=np.uint8)
        arena[bases[c]:bases[c] + ln] = data
        m.size, m.ck = ln, (tuple(orc.create(ctype, data.tobytes())) if ln else (ctype, 0))
        state.append(m)
    n = len(jobs)
    rec, ver = np.zeros(n, dtype=fp.REC), np.zeros(n, dtype=VER)
    has_payload = np.zeros(n, dtype=bool)
    placed, first, cur = [], set(), GUARD
    jobs = [dict(j) for j in jobs]
    for i, job in enumerate(jobs):
        c, k = job["c"], job["k"]
        u, v = rec[i], ver[i]
        u["chunk"] = bases[c]
        u["flags"] = (FLAG_ENGINE if job.get("engine") else 0) | (FLAG_SYNCING if job.get("sync") else 0)
        v["io_ver"], v["job_chain_ver"], v["is_force"] = job["ver"], job["jcv"], 1 if job.get("force") else 0
        if c not in first:  # the chunk's first job carries the state; the later ones junk
            first.add(c)
            u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = state[c].io()
            for f, x in zip(STATE_FIELDS, state[c].ver()):
                v[f] = x
        else:
            u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = oc.JUNK
            for f, x in zip(STATE_FIELDS, JUNK_VER):
                v[f] = x
        if k == "C":  # payload, offset and length of a commit job are ignored: junk
            u["update_type"], u["offset"], u["length"], u["payload"] = COMMIT_JOB, 0xFFFFFFF0, 77, 0
        elif k == "R":
            u["update_type"] = REMOVE
        elif k in "TE":
            u["update_type"], u["length"] = (TRUNCATE if k == "T" else EXTEND), job["ln"]
        else:
            off, ln = int(job["off"]), int(job["ln"])
            data = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
            p = ((cur + 15) & ~15) + (i * 7) % 16
            cur = p + ln + 64
            placed.append((p, data))
            has_payload[i] = True
            u["update_type"], u["offset"], u["length"], u["payload"] = WRITE, off, ln, p
            wck = tuple(orc.create(ctype, data))
            if job["flavour"] == "corrupt":
                wck = (wck[0], wck[1] ^ 0x10)
            if job["flavour"] == "none":
                wck = (NONE, 0)
            job["data"], job["wck"] = data, wck
            u["write_checksum_type"], u["write_checksum"] = wck
    pay = fp.canary(cur + GUARD, fp.SALT_PAYLOAD)
    for p, data in placed:
        pay[p:p + len(data)] = np.frombuffer(data, dtype=np.uint8)

    b = Built()
    b.name, b.n, b.n_chunks, b.max_len, b.max_rounds = name, n, n_chunks, max_len, max_rounds
    b.ctype, b.bases, b.jobs = ctype, bases, jobs
    b.rec, b.ver, b.has_payload, b.pay, b.arena0 = rec, ver, has_payload, pay, arena.copy()
    chunks = [bytearray(arena[x:x + max_len].tobytes()) for x in bases]
    b.expect, b.info = simulate(orc, jobs, chunks, state, max_len, max_rounds)

    def image(chs):
        a = arena.copy()
        for c, x in enumerate(bases):
            a[x:x + max_len] = np.frombuffer(bytes(chs[c]), dtype=np.uint8)
        return a

    b.arena1, b.metas = image(chunks), [m.copy() for m in state]
    b.again = None
    if b.info[1]:  # the NOT_APPLIED jobs resubmitted unchanged (as the call returns them)
        a = Built()
        a.idx = [i for i, e in enumerate(b.expect) if e[0] == NOT_APPLIED]
        a.n, a.max_len, a.max_rounds, a.bases = len(a.idx), max_len, max_rounds, bases
        chunks2, state2 = [bytearray(ch) for ch in chunks], [m.copy() for m in state]
        a.expect, a.info = simulate(orc, [jobs[i] for i in a.idx], chunks2, state2, max_len, max_rounds)
        a.arena1, a.metas = image(chunks2), state2
        b.again = a
    return b


def record_arrays(b, chunk_addr, pay_addr):
    rec = b.rec.copy()
    rec["chunk"] += np.uint64(chunk_addr)
    rec["payload"][b.has_payload] += np.uint64(pay_addr)
    return rec, b.ver.copy()


def expected(sent_rec, sent_ver, expect):
    """The two arrays the call must leave: the sent ones with the output fields and, for every
    job, the input state fields it started from."""
    rec, ver = sent_rec.copy(), sent_ver.copy()
    for i, (status, kase, io0, ver0, io1, ver1) in enumerate(expect):
        rec["status"][i], rec["checksum_case"][i] = status, kase
        rec["chunk_size"][i], rec["chunk_checksum_type"][i], rec["chunk_checksum"][i] = io0
        rec["out_size"][i], rec["out_checksum_type"][i], rec["out_checksum"][i] = io1
        for f, x in zip(STATE_FIELDS, ver0):
            ver[f][i] = x
        (ver["out_chain_ver"][i], ver["out_update_ver"][i], ver["out_commit_ver"][i], _,
         ver["out_chunk_state"][i], ver["out_recycle_state"][i]) = ver1
    return rec, ver


def admit_all(b, update_ver=7, commit_ver=5, chain_ver=3):
    """Version records for a case of ordered_cases that admit every IO: CLEAN chunks and io_ver =
    update_ver + 1 down each chain.  -> (sent ver array, expected ver array, info words 2..7)."""
    ver = np.zeros(b.n, dtype=VER)
    want = np.zeros(b.n, dtype=VER)
    depth = {}
    for i in range(b.n):
        c = int(b.rec["chunk"][i])
        k = depth.get(c, 0)
        depth[c] = k + 1
        ver["io_ver"][i] = want["io_ver"][i] = update_ver + k + 1
        ver["job_chain_ver"][i] = want["job_chain_ver"][i] = chain_ver
        before = (chain_ver, update_ver + k, commit_ver, b.max_len, CLEAN, 0)
        for f, x, junk in zip(STATE_FIELDS, before, JUNK_VER):
            ver[f][i] = x if k == 0 else junk
            want[f][i] = x
        assert b.expect[i][0] == OK, "admit_all is for cases whose IOs all succeed"
        want["out_chain_ver"][i], want["out_update_ver"][i] = chain_ver, update_ver + k + 1
        want["out_commit_ver"][i], want["out_chunk_state"][i] = commit_ver, CLEAN
    return ver, want, (b.n, 0, 0, 0, 0, 0)


# ---- the cases -----------------------------------------------------------------------------------------
def singles(orc, max_len):
    """One job per chunk; every status code of both ladders, and the precedence pairs."""
    q = max(8, max_len // 8)
    J, M, tags = [], {}, []

    def add(tag, job_of, meta=None):
        c = len(tags)
        tags.append(tag)
        if meta is not None:
            M[c] = meta
        J.append(job_of(c))

    lo = dict(chain_ver=9)  # job_chain_ver 3 < 9
    # ChunkReplica::update, one rung each
    add("u_ok", lambda c: W(c, 0, q, 5))
    add("u_ok_assign", lambda c: W(c, 3, q, 0))
    add("u_engine", lambda c: W(c, 0, q, 5, engine=True))
    add("u_remove", lambda c: R(c))
    add("u_bounds", lambda c: W(c, max_len, 4, 5))
    add("u_4015", lambda c: W(c, 0, q, 5), Meta(meta_chunk_size=max_len * 2))
    add("u_4005", lambda c: W(c, 0, q, 5), Meta(state=DIRTY))
    add("u_4081", lambda c: W(c, 0, q, 5), Meta(**lo))
    add("u_clean_low_chain_ok", lambda c: W(c, 0, q, 5), Meta(state=CLEAN, **lo))  # :186 needs COMMIT
    add("u_4080", lambda c: W(c, 0, q, 5, flavour="corrupt"))
    add("u_4008", lambda c: W(c, 0, q, 4))
    add("u_4006", lambda c: W(c, 0, q, 6), Meta(update_ver=6, commit_ver=4, state=CLEAN))
    add("u_4007", lambda c: W(c, 0, q, 6))
    add("u_4012", lambda c: W(c, 0, q, 0), Meta(update_ver=5, commit_ver=4, state=CLEAN))
    add("u_truncate_4007", lambda c: T(c, 0, 9))
    add("u_extend_ok", lambda c: E(c, q, 5, jcv=4))
    add("u_none_write_4006", lambda c: W(c, 0, q, 5, flavour="none"), Meta(update_ver=5, commit_ver=4, state=CLEAN))
    add("u_sync_dirty_recycling", lambda c: W(c, 0, q, 40, sync=True, jcv=5), Meta(state=DIRTY, recycle=1))
    add("u_sync_ver0_wraps", lambda c: W(c, 0, q, 0, sync=True))
    # precedence
    add("p_4015_over_4005", lambda c: W(c, 0, q, 5), Meta(meta_chunk_size=max_len // 2, state=DIRTY))
    add("p_4005_over_4081", lambda c: W(c, 0, q, 5), Meta(state=DIRTY, **lo))
    add("p_4081_over_payload", lambda c: W(c, 0, q, 5, flavour="corrupt"), Meta(**lo))
    add("p_invalid_over_4015", lambda c: W(c, max_len - 1, 2, 5), Meta(meta_chunk_size=7))
    for tag, ver, meta in (("4008", 4, Meta()), ("4006", 6, Meta(update_ver=6, commit_ver=4, state=CLEAN)),
                           ("4007", 6, Meta()), ("4012", 0, Meta(update_ver=5, commit_ver=4, state=CLEAN))):
        add(f"p_payload_over_{tag}", lambda c, ver=ver: W(c, 1, q, ver, flavour="corrupt"), meta)
        add(f"p_good_payload_{tag}", lambda c, ver=ver: W(c, 1, q, ver), meta)
    # ChunkReplica::commit
    up = dict(update_ver=6, commit_ver=4, state=CLEAN)
    add("c_ok_to_commit", lambda c: C(c, 6, jcv=8), Meta(**up))
    add("c_ok_stays_clean", lambda c: C(c, 5, jcv=8), Meta(**up))
    add("c_4081", lambda c: C(c, 6), Meta(chain_ver=9, **up))
    add("c_4082", lambda c: C(c, 7), Meta(**up))
    add("c_4005", lambda c: C(c, 6), Meta(update_ver=6, commit_ver=4, state=DIRTY))
    add("c_force_dirty", lambda c: C(c, 5, force=True), Meta(update_ver=6, commit_ver=4, state=DIRTY))
    add("c_force_backwards", lambda c: C(c, 2, force=True), Meta(**up))
    add("c_4023", lambda c: C(c, 4), Meta(**up))
    add("c_recycling", lambda c: C(c, 6), Meta(recycle=1, **up))
    add("c_engine", lambda c: C(c, 6, engine=True), Meta(**up))
    add("c_4081_over_4082", lambda c: C(c, 7), Meta(chain_ver=9, **up))
    n = len(tags)
    preset = [(c, q // 2 + c) for c in range(n)]
    b = build(orc, f"singles_{max_len}", n, max_len, 2, J, 0x51A6, metas=M, preset=preset)
    b.tags = tags
    return b


def pairs(orc, max_len):
    """The queues the issue names, one chunk each: a lost predecessor, duplicates, the head's
    write / commit ladder, commit transitions, a syncing write, and invalid jobs with neighbours."""
    q = max(8, max_len // 16)
    J, M = [], {}
    # 0: a bad-payload v+1 then v+2: 4080, 4007, the chunk untouched
    J += [W(0, 0, q, 5, flavour="corrupt"), W(0, q, q, 6)]
    # 1: a duplicate io_ver with another payload: OK, 4006, the first write's bytes
    J += [W(1, 0, q, 5), W(1, 0, q, 5)]
    # 2: the same with the commit between: OK, OK, 4008
    J += [W(2, 0, q, 5), C(2, 5), W(2, 0, q, 5)]
    # 3: the head: io_ver 0, write, commit, ... eight deep
    for k in range(4):
        J += [W(3, k * q, q, 0), C(3, 5 + k)]
    # 4: the head without its first commit: the second write is 4012, the commit still commits the first
    J += [W(4, 0, q, 0), W(4, q, q, 0), C(4, 5), W(4, q, q, 0), C(4, 6), W(4, 2 * q, q, 0), C(4, 7)]
    # 5: commit transitions: force on a DIRTY chunk, COMMIT only at commit_ver == update_ver, chain_ver from the job
    M[5] = Meta(update_ver=7, commit_ver=4, state=DIRTY)
    J += [C(5, 5), C(5, 5, force=True), C(5, 6, jcv=6), C(5, 6, jcv=6), C(5, 7, jcv=8), W(5, 0, q, 8, jcv=7),
          W(5, 0, q, 8, jcv=8)]
    # 6: a syncing write on a DIRTY, recycling chunk, then the chain goes on from its versions
    M[6] = Meta(update_ver=9, commit_ver=2, state=DIRTY, recycle=2)
    J += [W(6, 0, q, 6), W(6, 0, 2 * q, 20, sync=True), W(6, q, q, 21), C(6, 21), W(6, 0, q, 21)]
    # 7: ENGINE, REMOVE and a commit on a recycling chunk between valid neighbours
    M[7] = Meta(update_ver=4, commit_ver=4, state=CLEAN, recycle=1)
    J += [W(7, 0, q, 5), W(7, q, q, 6, engine=True), R(7), C(7, 6), W(7, q, q, 6), T(7, q + 3, 7)]
    order = np.random.default_rng(0x9A12).permutation(len(J))
    # interleave the chains, keeping each chunk's own order
    by_chunk = {}
    for j in J:
        by_chunk.setdefault(j["c"], []).append(j)
    take = {c: 0 for c in by_chunk}
    mixed = []
    for x in order:
        c = J[int(x)]["c"]
        mixed.append(by_chunk[c][take[c]])
        take[c] += 1
    preset = [(1, q + 5), (5, 3 * q), (6, 3 * q + 1)]
    return build(orc, f"pairs_{max_len}", 8, max_len, 8, mixed, 0x9A12, metas=M, preset=preset)


def overflow(orc, max_len, chains_n=6):
    """Chains of 5 under max_rounds 3 (write, commit, bad write, write, commit): two jobs per chain
    come back NOT_APPLIED with the state after the third."""
    rng = np.random.default_rng(0x0F11)
    order = oc._interleave(rng, [5] * chains_n)
    q = max(8, max_len // 8)
    step, J = {}, []
    for c in order:
        k = step.get(c, 0)
        step[c] = k + 1
        J.append([W(c, 0, q + c, 5), C(c, 5), W(c, q, q, 6, flavour="corrupt" if c % 2 else ""),
                  W(c, q + c, q, 6 if c % 2 else 7), C(c, 6 if c % 2 else 7)][k])
    return build(orc, f"overflow_{max_len}", chains_n, max_len, 3, J, 0x0F11)


def random_queue(orc, max_len, seed, n_chunks=64, depth_max=8):
    """64 chunks, up to 8 jobs each: every job kind, both payload verdicts, versions that are mostly
    right and sometimes stale, missing, committed or advanced."""
    rng = np.random.default_rng(seed)
    depths = [int(rng.integers(1, depth_max + 1)) for _ in range(n_chunks)]
    depths[0] = depth_max
    while sum(depths) > 256:  # n <= 256
        depths[1 + int(np.argmax(depths[1:]))] -= 1
    order = oc._interleave(rng, depths)
    M = {}
    for c in range(n_chunks):
        uv = int(rng.integers(1, 6))
        M[c] = Meta(chain_ver=int(rng.integers(2, 5)), update_ver=uv, commit_ver=uv - int(rng.integers(0, 2)),
                    state=int(rng.choice([COMMIT, CLEAN, CLEAN, DIRTY])), recycle=int(rng.integers(0, 8) == 0))
        if rng.integers(0, 16) == 0:
            M[c].meta_chunk_size = max_len + 1
        if M[c].commit_ver != M[c].update_ver and M[c].state == COMMIT:
            M[c].state = CLEAN
    guess = {c: M[c].update_ver for c in M}  # the update_ver a well-behaved client would expect
    unit = max(8, max_len // 8)
    J = []
    for c in order:
        pick = int(rng.integers(0, 16))
        jcv = int(rng.integers(2, 6))
        ln = int(rng.integers(1, unit))
        off = int(rng.integers(0, max_len - ln))
        slip = int(rng.choice([1, 1, 1, 1, 1, 0, 2, -1]))
        if pick < 7:
            flavour = "corrupt" if rng.integers(0, 5) == 0 else ("none" if rng.integers(0, 8) == 0 else "")
            J.append(W(c, off, ln, max(0, guess[c] + slip), jcv, flavour))
            guess[c] += int(flavour != "corrupt" and slip == 1)
        elif pick == 7:
            J.append(W(c, off, ln, 0, jcv))
        elif pick == 8:
            J.append(T(c, int(rng.integers(0, max_len)), guess[c] + 1, jcv))
            guess[c] += 1
        elif pick == 9:
            J.append(E(c, int(rng.integers(0, max_len + 2)), guess[c] + 1, jcv))
        elif pick < 14:
            J.append(C(c, max(0, guess[c] + int(rng.choice([0, 0, 0, 1, -1]))), jcv, force=bool(rng.integers(0, 6) == 0)))
        elif pick == 14:
            J.append(W(c, 0, ln, guess[c] + 5, jcv, sync=True))
            guess[c] += 5
        else:
            J.append(R(c) if rng.integers(0, 2) else W(c, off, ln, guess[c] + 1, jcv, engine=True))
    preset = [(c, 1 + (c * 37) % (max_len // 2)) for c in range(n_chunks) if c % 2]
    return build(orc, f"random_{max_len}_{seed:x}", n_chunks, max_len, depth_max, J, seed, metas=M, preset=preset)


def one_chunk(orc, max_len=128 << 10):
    """One chunk takes 64 jobs: the head's write / commit pairs with a stale retry and a bad payload."""
    J = []
    k = 0
    while len(J) < 64:
        J += [W(0, 1024 * k, 1024, 0), C(0, 5 + k)]
        if k % 5 == 2:
            J += [W(0, 0, 512, 5 + k), W(0, 7, 300, 0, flavour="corrupt")]  # 4008, 4080
        k += 1
    return build(orc, "one_chunk", 1, max_len, 64, J[:64], 0x0C02)


def capture_pair(orc, max_len=128 << 10):
    """Two queues of the same shape (same chunks, record count and payload room) whose records
    differ: the second groups the jobs differently and is refused where the first is applied."""
    q = 2048
    a = [W(c, 0, q, 5) for c in range(16)] + [C(c, 5) for c in range(16)] + [W(c, q, q, 6) for c in range(16)]
    b = [W(c // 2, (c % 2) * q, q, 5 + c % 2, flavour="corrupt" if c % 8 == 2 else "") for c in range(16)]
    b += [C(c // 4, 5 + c % 2, force=c % 4 == 3) for c in range(16)] + [W(8 + c // 2, q, q, 6) for c in range(16)]
    return (build(orc, "capture_a", 16, max_len, 6, a, 0xCA11), build(orc, "capture_b", 16, max_len, 6, b, 0xCA11))


SIZES = (512, 128 << 10)
SEEDS = (0x7E51, 0x7E52, 0x7E53)


def all_cases(orc):
    """name -> builder: every case the GPU tests run (built on demand; the model test builds all)."""
    out = {}
    for ml in SIZES:
        out[f"singles_{ml}"] = lambda ml=ml: singles(orc, ml)
        out[f"pairs_{ml}"] = lambda ml=ml: pairs(orc, ml)
        out[f"overflow_{ml}"] = lambda ml=ml: overflow(orc, ml)
        for s in SEEDS:
            out[f"random_{ml}_{s:x}"] = lambda ml=ml, s=s: random_queue(orc, ml, s)
    out["one_chunk"] = lambda: one_chunk(orc)
    out["capture_a"] = lambda: capture_pair(orc)[0]
    out["capture_b"] = lambda: capture_pair(orc)[1]
    return out
