"""Model and case builders of hf3fs_crc_forward_prepare / hf3fs_crc_forward_complete (the chain hop
between a target's local update and its commit).

The model follows the reference's own text: StorageOperator::handleUpdate
(src/storage/service/StorageOperator.cc:401-485) calls ReliableForwarding::forward (:113-134), which
calls doForward (:145-278), which for a syncing successor reads the whole chunk through
AioReadJob::setResult (src/storage/aio/BatchReadJob.cc:43-54).  It is written as those three
functions, with local variables named as theirs (`updateResult`, `commitIO`, `updateReq`), cut in two
where the request leaves the node: `prepare_one` runs up to messenger.update (:232), `complete_one`
from its answer on.  It shares no code with 3fs_amd/csrc/forward_plan.h; the CRC arithmetic is the
CPU oracle's and the record layout is written out here again (tests/test_forward_model.py compares
it with the package's and with the header).
"""
import numpy as np

JOB = np.dtype([
    ("payload", "<u8"), ("chunk", "<u8"), ("offset", "<u4"), ("length", "<u4"), ("chunk_size", "<u4"),
    ("req_update_ver", "<u4"), ("req_checksum", "<u4"), ("update_type", "u1"), ("req_checksum_type", "u1"),
    ("req_flags", "u1"), ("upd_checksum_type", "u1"),
    ("upd_status", "<i4"), ("upd_length", "<u4"), ("upd_update_ver", "<u4"), ("upd_commit_ver", "<u4"),
    ("upd_checksum", "<u4"),
    ("chain_ver", "<u4"), ("has_successor", "u1"), ("successor_syncing", "u1"), ("engine_job", "u1"),
    ("chunk_checksum_type", "u1"),
    ("chunk_len", "<u4"), ("chunk_checksum", "<u4"), ("chunk_update_ver", "<u4"), ("chunk_commit_chain_ver", "<u4"),
    ("chunk_status_in", "<i4"),
    ("out_data", "<u8"), ("status", "<i4"), ("res_length", "<u4"), ("res_update_ver", "<u4"),
    ("res_commit_ver", "<u4"), ("out_offset", "<u4"), ("out_length", "<u4"), ("out_checksum", "<u4"),
    ("out_update_ver", "<u4"), ("out_commit_chain_ver", "<u4"), ("computed", "<u4"), ("action", "u1"),
    ("is_syncing", "u1"), ("out_update_type", "u1"), ("out_checksum_type", "u1"), ("out_flags", "u1"),
    ("fwd_checksum_type", "u1"), ("reserved0", "u1", (2,)), ("fwd_status", "<i4"), ("fwd_length", "<u4"),
    ("fwd_checksum", "<u4"), ("fwd_commit_ver", "<u4"), ("fwd_commit_chain_ver", "<u4"),
    ("final_status", "<i4"), ("commit_ver", "<u4"), ("commit_chain_ver", "<u4"), ("fwd_update_ver", "<u4"),
    ("buffer_computed", "<u4"), ("final_action", "u1"), ("buffer_corrupted", "u1"), ("reserved1", "u1", (6,)),
])
assert JOB.itemsize == 192

INPUTS = JOB.names[:JOB.names.index("out_data")]
PREP_OUT = ("out_data", "status", "res_length", "res_update_ver", "res_commit_ver", "out_offset", "out_length",
            "out_checksum", "out_update_ver", "out_commit_chain_ver", "computed", "action", "is_syncing",
            "out_update_type", "out_checksum_type", "out_flags", "commit_ver", "commit_chain_ver")
RESPONSE = ("fwd_checksum_type", "fwd_status", "fwd_length", "fwd_checksum", "fwd_commit_ver", "fwd_commit_chain_ver")
DONE_OUT = ("final_status", "commit_ver", "commit_chain_ver", "fwd_update_ver", "buffer_computed", "final_action",
            "buffer_corrupted")

NONE, CRC32C, CRC32 = 0, 1, 2
WRITE, REMOVE, TRUNCATE, EXTEND, COMMIT_TYPE = 1, 2, 4, 8, 16
REQ_SYNCING, REQ_INLINE = 1, 2
OUT_SYNCING, OUT_INLINE, OUT_COMMIT_CHAIN_VER = 1, 2, 4
RETURN, SEND, NO_SUCCESSOR, COMMIT = 1, 2, 3, 4
INVALID_ARG = 3
STALE_UPDATE, MISSING_UPDATE, COMMITTED_UPDATE, ADVANCE_UPDATE = 4006, 4007, 4008, 4012
NO_SUCCESSOR_TARGET, CHECKSUM_MISMATCH, CHAIN_VERSION_MISMATCH, CHUNK_VERSION_MISMATCH = 4033, 4080, 4081, 4082
CLIENT_CHECKSUM_MISMATCH = 7015
INFO_WORDS = 8
PREP_INFO = ("sent", "returned", "no_successor", "sync_hashed", "sync_mismatched", "bad_records", "reserved6",
             "reserved7")
DONE_INFO = ("commits", "returned", "e7015", "e4081", "e4082", "rehashed", "corrupted", "unhashable")
POISON8, POISON32 = 0xA5, 0xA5A5A5A5  # what the builders leave in every output field


class Return(Exception):
    """co_return out of handleUpdate."""

    def __init__(self, status, length=0, update_ver=0, commit_ver=0, bad=False):
        self.status, self.length, self.update_ver, self.commit_ver, self.bad = status, length, update_ver, commit_ver, bad


def create(ctype, addr, length, read_bytes, orc):
    """ChecksumInfo::create (Common.h:150): NONE is {NONE, 0} before a byte is looked at."""
    if ctype == NONE:
        return (NONE, 0)
    return tuple(orc.create(ctype, read_bytes(addr, length) if length else b""))


def hashable(ctype, addr, length, call_type, max_len):
    """What the call can hash at all (include/hf3fs_crc.h); the reference has no such limits."""
    return ctype in (NONE, call_type) and length <= max_len and (addr != 0 or length == 0)


def prepare_one(j, call_type, max_len, max_inline, read_bytes, orc):
    """handleUpdate from :401 to the send at ReliableForwarding.cc:232 -> (fields to write, info bits)."""
    out = {k: 0 for k in PREP_OUT}
    bits = dict.fromkeys(PREP_INFO, 0)
    g = lambda k: int(j[k])  # noqa: E731
    try:
        if g("update_type") not in (WRITE, REMOVE, TRUNCATE, EXTEND):
            raise Return(INVALID_ARG, bad=True)
        # ---- StorageOperator.cc:401-434
        req_update_ver = g("req_update_ver")
        updateResult = dict(length=g("upd_length"), updateVer=g("upd_update_ver"), commitVer=g("upd_commit_ver"))
        code = g("upd_status")
        if code == 0:
            if req_update_ver == 0:                                        # :404
                req_update_ver = updateResult["updateVer"]
            elif req_update_ver != updateResult["updateVer"]:              # :406
                raise Return(CHUNK_VERSION_MISMATCH)
        elif code == MISSING_UPDATE:                                       # :411
            raise Return(code, **_res(updateResult))
        elif code == COMMITTED_UPDATE:                                     # :415
            raise Return(0, g("length"), req_update_ver, req_update_ver)
        elif code == STALE_UPDATE:                                         # :422
            updateResult["length"] = g("length")
            updateResult["updateVer"] = req_update_ver
        elif code == ADVANCE_UPDATE:                                       # :427
            raise Return(code, **_res(updateResult))
        else:                                                              # :431
            raise Return(code, **_res(updateResult))
        out["res_length"], out["res_update_ver"], out["res_commit_ver"] = (
            updateResult["length"], updateResult["updateVer"], updateResult["commitVer"])
        commitIO = dict(commitVer=updateResult["updateVer"], commitChainVer=0, isSyncing=0)   # :439-442
        # ---- ReliableForwarding::forward :113-117
        if not g("has_successor"):
            commitIO["commitChainVer"] = g("chain_ver")
            out.update(action=NO_SUCCESSOR, commit_ver=commitIO["commitVer"], commit_chain_ver=g("chain_ver"))
            out.update(dict.fromkeys(RESPONSE, 0), fwd_status=NO_SUCCESSOR_TARGET)
            bits["no_successor"] = 1
            return out, bits
        # ---- doForward :145-222
        updateReq = dict(updateType=g("update_type"), offset=g("offset"), length=g("length"), rdmabuf=g("payload"),
                         checksum=(g("req_checksum_type"), g("req_checksum")), updateVer=req_update_ver,
                         isSyncing=bool(g("req_flags") & REQ_SYNCING), inline=bool(g("req_flags") & REQ_INLINE),
                         commitChainVer=None)
        isSyncing = bool(g("successor_syncing"))                           # :152
        commitIO["isSyncing"] = int(isSyncing)
        if isSyncing:                                                      # :153-156
            updateReq["isSyncing"] = True
            updateReq["commitChainVer"] = g("chain_ver")
        wte = g("update_type") in (WRITE, TRUNCATE, EXTEND)
        readForSyncing = wte and isSyncing and (bool(g("req_flags") & REQ_SYNCING) or g("length") != g("chunk_size"))
        if readForSyncing:
            if g("chunk_status_in") != 0:                                  # :190 CO_RETURN_ON_ERROR
                raise Return(g("chunk_status_in"), **_res(updateResult))
            if not hashable(g("chunk_checksum_type"), g("chunk"), g("chunk_len"), call_type, max_len):
                raise Return(INVALID_ARG, bad=True, **_res(updateResult))
            # AioReadJob::setResult, BatchReadJob.cc:43-54 (recalculateChecksum, offset 0, whole chunk)
            stored = (g("chunk_checksum_type"), g("chunk_checksum"))
            real = create(stored[0], g("chunk"), g("chunk_len"), read_bytes, orc)
            out["computed"] = real[1]
            bits["sync_hashed"] = int(stored[0] != NONE and g("chunk_len") > 0)
            if real != stored:
                bits["sync_mismatched"] = 1
                raise Return(CHECKSUM_MISMATCH, **_res(updateResult))
            updateReq["inline"] = False                                    # :193-196
            length = g("chunk_len")                                        # :198
            updateReq["updateVer"] = g("chunk_update_ver")                 # :199
            if g("req_flags") & REQ_SYNCING:                               # :200-202
                updateReq["commitChainVer"] = g("chunk_commit_chain_ver")
            updateReq.update(offset=0, length=length, rdmabuf=g("chunk"), checksum=stored, updateType=WRITE)
            if length <= max_inline:                                       # :209-212
                updateReq["inline"] = True
        elif isSyncing and g("update_type") != REMOVE and not g("engine_job"):   # :215
            if g("chunk_status_in") != 0:                                  # :217-220
                raise Return(g("chunk_status_in"), **_res(updateResult))
            updateReq["updateVer"] = g("chunk_update_ver")                 # :221
        flags = (OUT_SYNCING if updateReq["isSyncing"] else 0) | (OUT_INLINE if updateReq["inline"] else 0)
        if updateReq["commitChainVer"] is not None:
            flags |= OUT_COMMIT_CHAIN_VER
        out.update(action=SEND, is_syncing=commitIO["isSyncing"], commit_ver=commitIO["commitVer"],
                   out_update_type=updateReq["updateType"], out_offset=updateReq["offset"],
                   out_length=updateReq["length"], out_data=updateReq["rdmabuf"],
                   out_checksum_type=updateReq["checksum"][0], out_checksum=updateReq["checksum"][1],
                   out_update_ver=updateReq["updateVer"], out_commit_chain_ver=updateReq["commitChainVer"] or 0,
                   out_flags=flags)
        bits["sent"] = 1
        return out, bits
    except Return as r:
        computed = out["computed"]
        out = {k: 0 for k in PREP_OUT}
        out.update(dict.fromkeys(RESPONSE, 0))
        out.update(action=RETURN, status=r.status, res_length=r.length, res_update_ver=r.update_ver,
                   res_commit_ver=r.commit_ver, computed=computed)
        bits.update(returned=1, bad_records=int(r.bad), sent=0)
        return out, bits


def _res(updateResult):
    return dict(length=updateResult["length"], update_ver=updateResult["updateVer"],
                commit_ver=updateResult["commitVer"])


def complete_one(j, call_type, max_len, read_bytes, orc):
    """From the successor's answer (ReliableForwarding.cc:233) to the commit decision
    (StorageOperator.cc:485) -> (fields to write, info bits)."""
    g = lambda k: int(j[k])  # noqa: E731
    out = {k: 0 for k in DONE_OUT}
    bits = dict.fromkeys(DONE_INFO, 0)
    if g("action") not in (SEND, NO_SUCCESSOR):
        out.update(final_action=RETURN, final_status=g("status"))
        bits["returned"] = 1
        return out, bits
    req_update_ver = g("req_update_ver")
    if g("upd_status") == 0 and req_update_ver == 0:                       # StorageOperator.cc:404-405
        req_update_ver = g("upd_update_ver")
    commitIO = dict(commitVer=g("res_update_ver"), commitChainVer=0)       # :441
    forward_update_ver = 0
    if g("action") == NO_SUCCESSOR:                                        # forward :113-117
        commitIO["commitChainVer"] = g("chain_ver")
    # ---- doForward :233-278: ioResult = (code, commitVer, commitChainVer, checksum)
    code = g("fwd_status")
    if code == 0:
        if g("chain_ver") < g("fwd_commit_chain_ver"):                     # :238
            code = CHAIN_VERSION_MISMATCH
            bits["e4081"] = 1
        elif g("is_syncing"):
            forward_update_ver = req_update_ver                            # :251
    elif code == CHECKSUM_MISMATCH:                                        # :263
        reqChecksum = (g("out_checksum_type"), g("out_checksum"))
        if not hashable(reqChecksum[0], g("out_data"), g("out_length"), call_type, max_len):
            bits["unhashable"] = 1
        else:
            real = create(reqChecksum[0], g("out_data"), g("out_length"), read_bytes, orc)   # :265-267
            out["buffer_computed"] = real[1]
            bits["rehashed"] = int(reqChecksum[0] != NONE and g("out_length") > 0)
            if reqChecksum != real:                                        # :268
                out["buffer_corrupted"] = 1
                bits["corrupted"] = 1
    # ---- forward :120-134
    if code == 0:
        commitIO["commitVer"] = g("fwd_commit_ver")
        commitIO["commitChainVer"] = g("fwd_commit_chain_ver")
        if g("fwd_commit_chain_ver") > g("chain_ver"):                     # :125 (doForward has answered already)
            code = CHAIN_VERSION_MISMATCH
            bits["e4081"] = 1
    # ---- handleUpdate :446-485
    out.update(commit_ver=commitIO["commitVer"], commit_chain_ver=commitIO["commitChainVer"],
               fwd_update_ver=forward_update_ver)
    if commitIO["commitVer"] != g("res_update_ver"):                       # :446
        out.update(final_action=RETURN, final_status=CHUNK_VERSION_MISMATCH)
        bits.update(e4082=1, returned=1)
        return out, bits
    if code == 0:
        fwd, upd = (g("fwd_checksum_type"), g("fwd_checksum")), (g("upd_checksum_type"), g("upd_checksum"))
        if g("update_type") == REMOVE and (fwd[0] == NONE or upd[0] == NONE or g("is_syncing")):   # :465
            pass
        elif fwd != upd:                                                   # :475
            out.update(final_action=RETURN, final_status=CLIENT_CHECKSUM_MISMATCH)
            bits.update(e7015=1, returned=1)
            return out, bits
    elif code != NO_SUCCESSOR_TARGET:                                      # :483
        out.update(final_action=RETURN, final_status=code)
        bits["returned"] = 1
        return out, bits
    out.update(final_action=COMMIT, final_status=0)                        # :487
    bits["commits"] = 1
    return out, bits


def model_prepare(jobs, call_type, max_len, max_inline, orc, read_bytes=None):
    """-> (the records after prepare, d_info).  A SEND job's response fields stay as they are."""
    after = jobs.copy()
    info = np.zeros(INFO_WORDS, dtype=np.uint32)
    for i in range(jobs.size):
        out, bits = prepare_one(jobs[i], call_type, max_len, max_inline, read_bytes, orc)
        for k, v in out.items():
            after[k][i] = v
        for w, name in enumerate(PREP_INFO):
            info[w] += bits[name]
    return after, info


def model_complete(jobs, call_type, max_len, orc, read_bytes=None):
    """-> (the records after complete, the ascending commit list, d_info)."""
    after = jobs.copy()
    info = np.zeros(INFO_WORDS, dtype=np.uint32)
    commits = []
    for i in range(jobs.size):
        out, bits = complete_one(jobs[i], call_type, max_len, read_bytes, orc)
        for k, v in out.items():
            after[k][i] = v
        for w, name in enumerate(DONE_INFO):
            info[w] += bits[name]
        if out["final_action"] == COMMIT:
            commits.append(i)
    return after, np.array(commits, dtype=np.uint32), info


# ---- builders -----------------------------------------------------------------------------------
def blank(n):
    """n records whose inputs are zero and whose every output field is poisoned: a call must
    overwrite what it owns."""
    a = np.zeros(n, dtype=JOB)
    for k in PREP_OUT + RESPONSE + DONE_OUT:
        a[k] = POISON8 if JOB[k].itemsize == 1 else (-2 if JOB[k].kind == "i" else POISON32)
    return a


def plain_job(**kw):
    """A successful local write of 100 bytes on a target with a serving successor: prepare sends it
    as it is, an answer that agrees commits it."""
    j = blank(1)
    base = dict(update_type=WRITE, offset=0, length=100, chunk_size=4096, payload=0x10000, req_update_ver=5,
                req_checksum_type=CRC32C, req_checksum=0x11111111, upd_status=0, upd_length=100, upd_update_ver=5,
                upd_commit_ver=4, upd_checksum_type=CRC32C, upd_checksum=0x22222222, chain_ver=7, has_successor=1)
    for k, v in dict(base, **kw).items():
        j[k] = v
    return j


def answer(j, i=0, **kw):
    """The successor's answer to job i: by default one that agrees with the local update."""
    base = dict(fwd_status=0, fwd_length=int(j["upd_length"][i]), fwd_checksum_type=int(j["upd_checksum_type"][i]),
                fwd_checksum=int(j["upd_checksum"][i]), fwd_commit_ver=int(j["res_update_ver"][i]),
                fwd_commit_chain_ver=int(j["chain_ver"][i]))
    for k, v in dict(base, **kw).items():
        j[k][i] = v


def random_jobs(rng, n, call_type, chunks, chunk_lens, chunk_cks, payloads, payload_lens, payload_cks, max_len=4096,
                other_type=None):
    """n random jobs over the given device chunks and payloads (addresses, lengths, (type, value)
    checksums of their bytes), spread over every branch of prepare."""
    other = other_type if other_type is not None else (CRC32 if call_type == CRC32C else CRC32C)
    j = blank(n)
    pick = lambda *xs, p=None: rng.choice(np.array(xs), size=n, p=p)  # noqa: E731
    ci, pi = rng.integers(0, len(chunks), n), rng.integers(0, len(payloads), n)
    j["update_type"] = pick(WRITE, REMOVE, TRUNCATE, EXTEND, COMMIT_TYPE, 0, p=[.55, .15, .1, .1, .05, .05])
    j["payload"] = np.asarray(payloads, dtype=np.uint64)[pi]
    j["length"] = np.asarray(payload_lens, dtype=np.uint32)[pi]
    j["offset"] = rng.integers(0, 64, n)
    j["chunk_size"] = np.where(rng.random(n) < .3, j["length"], max_len)
    j["req_checksum_type"] = np.asarray([c[0] for c in payload_cks], dtype=np.uint8)[pi]
    j["req_checksum"] = np.asarray([c[1] for c in payload_cks], dtype=np.uint32)[pi]
    unhashable = rng.random(n)  # outgoing buffers complete cannot re-hash after a 4080 answer
    j["req_checksum_type"] = np.where(unhashable < .08, other, j["req_checksum_type"])
    j["payload"] = np.where((unhashable >= .08) & (unhashable < .12), 0, j["payload"])
    j["req_flags"] = rng.integers(0, 4, n)
    j["upd_update_ver"] = rng.integers(1, 6, n)
    j["req_update_ver"] = np.where(rng.random(n) < .3, 0, np.where(rng.random(n) < .85, j["upd_update_ver"],
                                                                    j["upd_update_ver"] + 1))
    j["upd_status"] = pick(0, STALE_UPDATE, MISSING_UPDATE, COMMITTED_UPDATE, ADVANCE_UPDATE, 4010,
                           p=[.7, .1, .05, .05, .05, .05])
    j["upd_length"] = j["length"]
    j["upd_commit_ver"] = j["upd_update_ver"] - 1
    j["upd_checksum_type"] = pick(NONE, call_type, other, p=[.15, .75, .1])
    j["upd_checksum"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    j["chain_ver"] = rng.integers(1, 5, n)
    j["has_successor"] = rng.random(n) < .85
    j["successor_syncing"] = rng.random(n) < .6
    j["engine_job"] = rng.random(n) < .3
    j["chunk"] = np.asarray(chunks, dtype=np.uint64)[ci]
    j["chunk_len"] = np.asarray(chunk_lens, dtype=np.uint32)[ci]
    j["chunk_checksum_type"] = np.asarray([c[0] for c in chunk_cks], dtype=np.uint8)[ci]
    j["chunk_checksum"] = np.asarray([c[1] for c in chunk_cks], dtype=np.uint32)[ci]
    # a few stored checksums that do not describe the bytes, a few records the call cannot hash
    wrong = rng.random(n) < .1
    j["chunk_checksum"] = np.where(wrong, j["chunk_checksum"] ^ (1 << rng.integers(0, 32, n)).astype(np.uint32),
                                   j["chunk_checksum"])
    odd = rng.random(n)
    j["chunk_checksum_type"] = np.where(odd < .04, other, np.where(odd < .12, NONE, j["chunk_checksum_type"]))
    j["chunk_checksum"] = np.where((odd >= .06) & (odd < .12), 0, j["chunk_checksum"])
    j["chunk"] = np.where((odd >= .12) & (odd < .14), 0, j["chunk"])
    j["chunk_len"] = np.where((odd >= .14) & (odd < .16), max_len + 1, j["chunk_len"])
    j["chunk_update_ver"] = rng.integers(1, 9, n)
    j["chunk_commit_chain_ver"] = rng.integers(1, 5, n)
    j["chunk_status_in"] = np.where(rng.random(n) < .08, 4010, 0)
    return j


def random_answers(rng, j, call_type, commit_share=None):
    """The successor's answers for the SEND jobs of j (after prepare), spread over every branch of
    complete.  commit_share: the share of them that commits, exactly: those agree in everything and
    every other answer is one that never commits, whatever the job (4080, 4010, a foreign commit
    version, a higher chain version).  None: the default mix, with 4033 answers and checksum
    disagreements, which commit or not depending on the job."""
    n = j.size
    sent = j["action"] == SEND
    u = rng.random(n)
    agree = u < (commit_share if commit_share is not None else .45)
    other = rng.integers(1, 8, n) if commit_share is None else rng.choice(np.array([1, 2, 6, 7]), size=n)
    kind = np.where(agree, 0, other)
    st = np.select([kind == 1, kind == 2, kind == 3], [CHECKSUM_MISMATCH, 4010, NO_SUCCESSOR_TARGET], 0)
    for k, v in (("fwd_status", st), ("fwd_length", j["upd_length"]),
                 ("fwd_checksum_type", np.where(kind == 4, NONE, j["upd_checksum_type"])),
                 ("fwd_checksum", np.where(kind == 5, j["upd_checksum"] ^ 1, j["upd_checksum"])),
                 ("fwd_commit_ver", np.where(kind == 6, j["res_update_ver"] + 1, j["res_update_ver"])),
                 ("fwd_commit_chain_ver", np.where(kind == 7, j["chain_ver"] + 1, j["chain_ver"] - (u < .2)))):
        j[k] = np.where(sent, v, j[k]).astype(JOB[k])
    return j
