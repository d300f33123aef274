"""Model and case builders of hf3fs_crc_server_read_prepare / hf3fs_crc_server_read_complete (the
storage server's batchRead around its AIO).

The model follows the reference's own text.  `prepare` is StorageOperator::batchRead up to the
enqueue (src/storage/service/StorageOperator.cc:98-155) with AioReadJob's constructor
(src/storage/aio/BatchReadJob.cc:16-22), BufferPool::Buffer::tryAllocate / allocate
(src/storage/service/BufferPool.cc:102-141) and aioPrepareRead (src/storage/store/ChunkReplica.cc:38-76,
ChunkEngine.h:34-73); `complete` is setReadJobResult (src/storage/aio/AioStatus.cc:27-55),
AioReadJob::setResult (BatchReadJob.cc:24-63), aioFinishRead (StorageTarget.cc:299-304,
ChunkReplica.cc:79-100), copyToRespBuffer (BatchReadJob.cc:96-113), addBufferToBatch (:74-94) and
RDMAReqBatch::add (src/common/net/ib/IBSocket.cc:258-275).  Local variables are named as theirs.  It
shares no code with 3fs_amd/csrc/server_read_plan.h; the CRC arithmetic is the CPU oracle's and the
record layouts are written out here again (tests/test_server_read_model.py compares them with the
package's and with the header).
"""
import numpy as np

JOB = np.dtype([
    ("remote_addr", "<u8"), ("inner_offset", "<u8"), ("localbuf", "<u8"), ("res", "<i8"),
    ("read_offset", "<u8"), ("inline_off", "<u8"),
    ("offset", "<u4"), ("length", "<u4"), ("rdmabuf_size", "<u4"), ("rkey", "<u4"),
    ("target_status", "<i4"), ("meta_status", "<i4"), ("commit_ver", "<u4"), ("update_ver", "<u4"),
    ("chain_ver", "<u4"), ("chunk_len", "<u4"), ("chunk_checksum", "<u4"),
    ("meta_status_now", "<i4"), ("update_ver_now", "<u4"),
    ("head_len", "<u4"), ("tail_len", "<u4"), ("read_len", "<u4"), ("buf_ordinal", "<u4"), ("buf_off", "<u4"),
    ("status", "<i4"),
    ("result_len", "<u4"), ("result_status", "<i4"), ("checksum", "<u4"),
    ("has_rkey", "u1"), ("up_to_date", "u1"), ("engine", "u1"), ("chunk_checksum_type", "u1"),
    ("buf_kind", "u1"), ("checksum_type", "u1"), ("reserved", "u1", (50,)),
])
REQ = np.dtype([
    ("total_len", "<u8"), ("total_head", "<u8"), ("total_tail", "<u8"),
    ("inline_off", "<u8"), ("inline_bytes", "<u8"), ("wr_bytes", "<u8"),
    ("max_msg_sz", "<u4"), ("status", "<i4"), ("failed_job", "<u4"), ("n_small", "<u4"), ("n_big", "<u4"),
    ("n_ok", "<u4"), ("wr_first", "<u4"), ("wr_count", "<u4"), ("wr_fails", "<u4"),
    ("checksum_type", "u1"), ("xmit", "u1"), ("read_uncommitted", "u1"), ("recalculate", "u1"),
    ("reserved", "u1", (40,)),
])
WR = np.dtype([("remote_addr", "<u8"), ("local_addr", "<u8"), ("length", "<u4"), ("rkey", "<u4"), ("job", "<u4"),
               ("req", "<u4")])
assert JOB.itemsize == 192 and REQ.itemsize == 128 and WR.itemsize == 32

JOB_PREP_OUT = ("read_offset", "head_len", "tail_len", "read_len", "buf_ordinal", "buf_off", "status", "buf_kind")
JOB_DONE_OUT = ("inline_off", "result_len", "result_status", "checksum", "checksum_type")
REQ_PREP_OUT = ("total_len", "total_head", "total_tail", "status", "failed_job", "n_small", "n_big")
REQ_DONE_OUT = ("inline_off", "inline_bytes", "wr_bytes", "n_ok", "wr_first", "wr_count", "wr_fails")

NONE, CRC32C, CRC32 = 0, 1, 2
XMIT_RDMA, XMIT_INLINE, XMIT_NONE = 0, 1, 2
BUF_NONE, BUF_SMALL, BUF_BIG = 0, 1, 2
NO_JOB = 0xFFFFFFFF
INVALID_ARG, RDMA_NO_BUF = 3, 2019
CHUNK_METADATA_NOT_FOUND, CHUNK_METADATA_GET_ERROR, CHUNK_NOT_COMMIT, CHUNK_READ_FAILED = 4001, 4002, 4004, 4010
TARGET_STATE_INVALID, CHECKSUM_MISMATCH, CHAIN_VERSION_MISMATCH = 4032, 4080, 4081
INFO_WORDS = 8
PREP_INFO = ("reqs_ok", "reqs_failed", "jobs_ok", "jobs_failed", "small", "big", "reserved6", "reserved7")
DONE_INFO = ("ok", "failed", "inline_lo", "inline_hi", "inline_overflow", "wr", "wr_fails", "hashed")
kAIOAlignSize = 4096
U32 = 0xFFFFFFFF
POISON8, POISON32, POISON64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


class Error(Exception):
    """makeError(code)."""

    def __init__(self, code):
        self.code = int(code)


def new_jobs(n):
    """n jobs a healthy replica target would serve, every output field poisoned."""
    j = np.zeros(n, dtype=JOB)
    j["up_to_date"] = 1
    j["has_rkey"] = 1
    j["rdmabuf_size"] = 1 << 30
    j["commit_ver"] = j["update_ver"] = j["update_ver_now"] = 1
    j["chain_ver"] = 1
    poison(j, JOB_PREP_OUT + JOB_DONE_OUT)
    return j


def new_reqs(n, checksum_type=CRC32C, xmit=XMIT_NONE):
    r = np.zeros(n, dtype=REQ)
    r["checksum_type"] = checksum_type
    r["xmit"] = xmit
    r["max_msg_sz"] = 1 << 30
    poison(r, REQ_PREP_OUT + REQ_DONE_OUT)
    return r


def poison(recs, names):
    for name in names:
        kind = recs.dtype[name]
        if kind.kind == "i":
            recs[name] = -0x5A5A5A5B
        else:
            recs[name] = {1: POISON8, 4: POISON32, 8: POISON64}[kind.itemsize]


def offsets(counts):
    """d_req_off of requests with these job counts."""
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.uint64))]).astype(np.uint64)


# ---- prepare -------------------------------------------------------------------------------------
def aligned(offset, length):
    """AioReadJob::AioReadJob (BatchReadJob.cc:20-21) and alignedLength(): uint32_t arithmetic."""
    headLength = offset % kAIOAlignSize
    tailLength = (kAIOAlignSize - ((offset + length) & U32) % kAIOAlignSize) % kAIOAlignSize
    return headLength, tailLength, (length + headLength + tailLength) & U32


class Buffer:
    """BufferPool::Buffer: indices_ and current_ (a kind, a size and what takeFirst left)."""

    def __init__(self, rdmabufSize, bigRdmabufSize):
        self.rdmabufSize, self.bigRdmabufSize = rdmabufSize, bigRdmabufSize
        self.indices = []      # the kinds of the buffers taken
        self.current_size = 0  # current_.size()
        self.current_cap = 0

    def allocate(self, size):
        """tryAllocate (BufferPool.cc:102-119), then allocate (:121-141), as batchRead calls them
        (StorageOperator.cc:143-151: every failure is answered kRDMANoBuf).  The semaphores never
        fail here: waiting is the host's."""
        if not self.indices or self.current_size < size:
            if size > self.bigRdmabufSize:
                raise Error(RDMA_NO_BUF)
            elif size > self.rdmabufSize:
                self.indices.append(BUF_BIG)
                self.current_size = self.current_cap = self.bigRdmabufSize
            else:
                self.indices.append(BUF_SMALL)
                self.current_size = self.current_cap = self.rdmabufSize
        ret = (len(self.indices) - 1, self.indices[-1], self.current_cap - self.current_size)  # takeFirst
        self.current_size -= size
        return ret


def aio_prepare_read(j, readUncommitted):
    """StorageTarget::aioPrepareRead (StorageTarget.cc:289-297) on one record."""
    if j["meta_status"] != 0:                                   # ChunkReplica.cc:46-50, ChunkEngine.h:48-54
        raise Error(j["meta_status"])
    if j["engine"]:
        j["commit_ver"] = j["update_ver"]                       # ChunkEngine.h:61-62: both are chunk_ver
    elif j["commit_ver"] != j["update_ver"] and not readUncommitted:   # ChunkReplica.cc:61-66
        raise Error(CHUNK_NOT_COMMIT)
    headLength = int(j["offset"]) % kAIOAlignSize
    j["read_offset"] = (int(j["inner_offset"]) + int(j["offset"]) - headLength) & 0xFFFFFFFFFFFFFFFF


def prepare(jobs, reqs, req_off, small_buf, big_buf):
    """hf3fs_crc_server_read_prepare in place; returns the eight info words."""
    info = dict.fromkeys(PREP_INFO, 0)
    for r in range(reqs.size):
        lo, hi = int(req_off[r]), int(req_off[r + 1])
        req = reqs[r]
        try:
            totalLength = totalHeadLength = totalTailLength = 0
            for i in range(lo, hi):                             # StorageOperator.cc:101-130
                it = jobs[i]
                try:
                    if it["target_status"] != 0:
                        raise Error(it["target_status"])        # :107-111
                    if not it["up_to_date"]:
                        raise Error(TARGET_STATE_INVALID)       # :113-117
                    head, tail, _ = aligned(int(it["offset"]), int(it["length"]))
                    totalLength += int(it["length"])
                    totalHeadLength += head
                    totalTailLength += tail
                    if it["length"] > it["rdmabuf_size"]:
                        raise Error(INVALID_ARG)                # :122-128
                except Error as e:
                    e.job = i
                    raise
            buffer = Buffer(small_buf, big_buf)                 # :140
            placed = []
            for i in range(lo, hi):                             # :141-154
                try:
                    placed.append(buffer.allocate(aligned(int(jobs[i]["offset"]), int(jobs[i]["length"]))[2]))
                except Error as e:
                    e.job = i
                    raise
        except Error as e:                                      # co_return makeError(...)
            req["status"], req["failed_job"] = e.code, e.job
            req["total_len"] = req["total_head"] = req["total_tail"] = 0
            req["n_small"] = req["n_big"] = 0
            for i in range(lo, hi):
                j = jobs[i]
                j["head_len"], j["tail_len"], _ = aligned(int(j["offset"]), int(j["length"]))
                j["read_len"] = j["read_offset"] = j["buf_ordinal"] = j["buf_off"] = 0
                j["buf_kind"], j["status"] = BUF_NONE, e.code
            info["reqs_failed"] += 1
            info["jobs_failed"] += hi - lo
            continue
        req["status"], req["failed_job"] = 0, NO_JOB
        req["total_len"], req["total_head"], req["total_tail"] = totalLength, totalHeadLength, totalTailLength
        req["n_small"], req["n_big"] = buffer.indices.count(BUF_SMALL), buffer.indices.count(BUF_BIG)
        info["reqs_ok"] += 1
        info["small"] += int(req["n_small"])
        info["big"] += int(req["n_big"])
        for i, (ordinal, kind, off) in zip(range(lo, hi), placed):
            j = jobs[i]
            j["head_len"], j["tail_len"], j["read_len"] = aligned(int(j["offset"]), int(j["length"]))
            j["buf_ordinal"], j["buf_kind"], j["buf_off"] = ordinal, kind, off
            j["read_offset"] = 0
            try:
                aio_prepare_read(j, bool(req["read_uncommitted"]))
                j["status"] = 0
                info["jobs_ok"] += 1
            except Error as e:
                j["status"] = e.code
                info["jobs_failed"] += 1
    return [info[k] for k in PREP_INFO]


# ---- complete ------------------------------------------------------------------------------------
def chunk_checksum(j):
    """state_.chunkChecksum (ChunkReplica.cc:59, ChunkEngine.h:65)."""
    if j["engine"]:
        return (CRC32C, ~int(j["chunk_checksum"]) & U32)
    return (int(j["chunk_checksum_type"]), int(j["chunk_checksum"]))


def create(ctype, addr, length, read_bytes, orc):
    """ChecksumInfo::create (Common.h:150): NONE is {NONE, 0} before a byte is looked at."""
    if ctype == NONE:
        return (NONE, 0)
    return tuple(orc.create(ctype, read_bytes(addr, length) if length else b""))


def complete(jobs, reqs, req_off, call_type, max_len, read_bytes, orc, inline_cap=0, loads=None):
    """hf3fs_crc_server_read_complete in place.  Returns (info words, the inline arena's bytes or
    None on overflow, the full RDMA list as a WR array).  loads: a list that receives (job, "hash" or
    "pack", address, length) for every byte range the call has to load."""
    info = dict.fromkeys(DONE_INFO, 0)
    inlinebuf = bytearray()
    reqs_ = []
    for r in range(reqs.size):
        lo, hi = int(req_off[r]), int(req_off[r + 1])
        req = reqs[r]
        checksumType, recalculateChecksum = int(req["checksum_type"]), bool(req["recalculate"])
        results = {}    # job -> lengthInfo: an int, or an Error
        for i in range(lo, hi):
            j = jobs[i]
            j["result_len"], j["checksum"], j["checksum_type"], j["inline_off"] = 0, 0, NONE, 0
            if j["status"] != 0:                                    # never enqueued
                results[i] = Error(j["status"])
                continue
            chunkChecksum = chunk_checksum(j)
            if any(t not in (NONE, call_type) for t in (checksumType, chunkChecksum[0])):
                results[i] = Error(INVALID_ARG)                     # the call's limit
                continue
            res, headLength = int(j["res"]), int(j["head_len"])
            if res < 0:                                             # AioStatus.cc:40-53
                results[i] = Error(CHUNK_READ_FAILED)
                continue
            length = min(min(max(0, res - headLength), int(j["length"])),
                         max(0, int(j["chunk_len"]) - int(j["offset"])))   # :33-34
            if length > max_len:
                results[i] = Error(INVALID_ARG)                     # the call's limit
                continue
            # AioReadJob::setResult(length), BatchReadJob.cc:24-63
            lengthInfo = length
            full = j["offset"] == 0 and lengthInfo == j["chunk_len"]
            finish = None
            if not j["engine"]:                                     # StorageTarget.cc:299-304
                if j["meta_status_now"] != 0:
                    finish = Error(j["meta_status_now"])            # ChunkReplica.cc:85-88
                elif j["update_ver"] != j["update_ver_now"]:
                    finish = Error(CHUNK_NOT_COMMIT)                # :93-98
            reads = (checksumType != NONE and not (checksumType == chunkChecksum[0] and full)) or \
                    (finish is None and recalculateChecksum and full and chunkChecksum[0] != NONE)
            packs = req["xmit"] == XMIT_INLINE
            if j["localbuf"] == 0 and length > 0 and (reads or packs):
                results[i] = Error(INVALID_ARG)                     # the call's limit
                continue
            info["hashed"] += 1 if reads and length else 0          # one hashed range serves both rungs
            if loads is not None and reads and length:
                loads.append((i, "hash", int(j["localbuf"]) + headLength, length))
            dataBuf = int(j["localbuf"]) + headLength
            if checksumType == NONE:
                checksum = (NONE, 0)                                # :28-29
            elif checksumType == chunkChecksum[0] and full:
                checksum = chunkChecksum                            # :30-31
            else:
                checksum = create(checksumType, dataBuf, lengthInfo, read_bytes, orc)   # :32-35
            j["checksum_type"], j["checksum"] = checksum
            if finish is not None:
                lengthInfo = finish                                 # :38-41
            elif recalculateChecksum and full:                      # :43-54 (skipped after an error above)
                realChecksum = create(chunkChecksum[0], int(j["localbuf"]), length, read_bytes, orc)
                if realChecksum != chunkChecksum:
                    lengthInfo = Error(CHECKSUM_MISMATCH)
            results[i] = lengthInfo
        # the transmission (StorageOperator.cc:176-226)
        wr = []
        wr_fails = 0
        inline_off = len(inlinebuf)
        if req["xmit"] == XMIT_INLINE:                              # copyToRespBuffer, BatchReadJob.cc:96-113
            for i in range(lo, hi):
                if not isinstance(results[i], Error):
                    length = results[i]
                    jobs[i]["inline_off"] = len(inlinebuf)
                    if loads is not None and length:
                        loads.append((i, "pack", int(jobs[i]["localbuf"]) + int(jobs[i]["head_len"]), length))
                    inlinebuf += read_bytes(int(jobs[i]["localbuf"]) + int(jobs[i]["head_len"]), length) if length else b""
        elif req["xmit"] == XMIT_RDMA:                              # addBufferToBatch, :74-94
            for i in range(lo, hi):
                if not isinstance(results[i], Error):
                    j = jobs[i]
                    length = results[i]
                    # RDMAReqBatch::add, IBSocket.cc:258-275
                    if j["localbuf"] == 0 or not j["has_rkey"] or length > j["rdmabuf_size"] or \
                            length > req["max_msg_sz"]:
                        wr_fails += 1
                        results[i] = Error(INVALID_ARG)
                    else:
                        wr.append((int(j["remote_addr"]), int(j["localbuf"]) + int(j["head_len"]), length,
                                   int(j["rkey"]), i, r))
        n_ok = 0
        for i in range(lo, hi):
            if isinstance(results[i], Error):
                jobs[i]["result_status"], jobs[i]["result_len"] = results[i].code, 0
                jobs[i]["inline_off"] = 0
                info["failed"] += 1
            else:
                jobs[i]["result_status"], jobs[i]["result_len"] = 0, results[i]
                n_ok += 1
        info["ok"] += n_ok
        info["wr_fails"] += wr_fails
        reqs_.append((r, n_ok, inline_off, len(inlinebuf) - inline_off, wr, wr_fails))
    wr_all = []
    for r, n_ok, inline_off, inline_bytes, wr, wr_fails in reqs_:
        req = reqs[r]
        req["n_ok"], req["inline_off"], req["inline_bytes"] = n_ok, inline_off, inline_bytes
        req["wr_first"], req["wr_count"], req["wr_fails"] = len(wr_all), len(wr), wr_fails
        req["wr_bytes"] = sum(w[2] for w in wr)
        wr_all += wr
    info["wr"] = len(wr_all)
    info["inline_lo"], info["inline_hi"] = len(inlinebuf) & U32, len(inlinebuf) >> 32
    info["inline_overflow"] = 1 if len(inlinebuf) > inline_cap else 0
    wr_arr = np.zeros(len(wr_all), dtype=WR)
    for k, w in enumerate(wr_all):
        wr_arr[k] = w
    return [info[k] for k in DONE_INFO], (None if info["inline_overflow"] else bytes(inlinebuf)), wr_arr
