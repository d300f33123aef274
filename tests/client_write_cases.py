"""Model and case builders of hf3fs_crc_client_write_prepare / _complete (the client's batchWrite).

`prepare_model` restates what StorageClientImpl::batchWrite does before the send in the
reference's own shape: validateWriteDataRange (src/client/storage/StorageClientImpl.cc:994-1015,
uint32 arithmetic), validateDataRange over the survivors (:889-951 with RDMABuf::contains,
src/common/net/ib/RDMABuf.h:162) and sendWriteRequest's checksum and inline flag (:1878-1901).
`complete_model` restates setResultOfOp / collectFailedOps (:211-236, :1922), the counters
(:1958-1968), FileWrapper::writeFile's fold (src/client/cli/admin/FileWrapper.cc:218-248) over
ChecksumInfo::combine (src/fbs/storage/Common.h:179-198, its four steps in their order) and
Bench.cc's check (:41-48).  Both are sequential loops and share no code with
3fs_amd/csrc/client_write_plan.h: the CRC arithmetic is the CPU oracle's and the record layouts
are written out here again (tests/test_client_write_model.py compares them with the package's
and holds the model to examples worked by hand).
"""
import numpy as np

IO = np.dtype([("data", "<u8"), ("buf_base", "<u8"), ("buf_size", "<u8"), ("offset", "<u4"), ("length", "<u4"),
               ("chunk_size", "<u4"), ("checksum", "<u4"), ("checksum_type", "u1"), ("send_inline", "u1"),
               ("reserved0", "u1", (2,)), ("status", "<i4"), ("status_in", "<i4"), ("result_len", "<u4"),
               ("result_checksum", "<u4"), ("result_checksum_type", "u1"), ("reserved1", "u1", (3,))])
FILE = np.dtype([("length", "<u8"), ("value", "<u4"), ("type", "u1"), ("reserved", "u1", (3,)), ("status", "<i4"),
                 ("failed_io", "<u4")])
UPDATE = np.dtype([("chunk", "<u8"), ("payload", "<u8"), ("offset", "<u4"), ("length", "<u4"), ("chunk_size", "<u4"),
                   ("update_type", "u1"), ("chunk_checksum_type", "u1"), ("write_checksum_type", "u1"), ("flags", "u1"),
                   ("chunk_checksum", "<u4"), ("write_checksum", "<u4"), ("out_size", "<u4"), ("out_checksum", "<u4"),
                   ("out_checksum_type", "u1"), ("checksum_case", "u1"), ("reserved1", "u1", (2,)), ("status", "<i4")])
assert IO.itemsize == 64 and FILE.itemsize == 24 and UPDATE.itemsize == 56

NONE, CRC32C, CRC32 = 0, 1, 2
INVALID_ARG, INVALID_FORMAT, STORAGE_MISMATCH, CLIENT_INVALID_ARG, NOT_INITIALIZED, CLIENT_MISMATCH = (
    3, 33, 4080, 7002, 7003, 7015)
VERIFY, FROM_UPDATES = 1, 2
UPDATE_WRITE = 1
NO_IO = 0xFFFFFFFF
PREP_INFO = ("sent", "range", "bad_records", "poisoned", "inline", "hashed_lo", "hashed_hi", "reserved")
DONE_INFO = ("failed", "ok", "len_lo", "len_hi", "bad_files", "mismatched_files", "reserved0", "reserved1")
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
POISON_OUT = 0xA5A5A5A5  # what the builders leave in prepare's outputs; status gets -2


def ios_array(rows):
    """rows of (data, buf_base, buf_size, offset, length, chunk_size) -> an IO array whose prepare
    outputs are poisoned and whose answer is IOResult's default (7003)."""
    a = np.zeros(len(rows), dtype=IO)
    for i, (data, base, size, offset, length, chunk_size) in enumerate(rows):
        a[i] = (data, base, size, offset, length, chunk_size, POISON_OUT, 0xA5, 0xA5, (0, 0), -2, NOT_INITIALIZED, 0, 0,
                0, (0, 0, 0))
    return a


def with_answers(ios, status, answers):
    """A copy of ios as complete receives it: prepare's status and (status_in, result_len, (type, value))."""
    a = ios.copy()
    a["status"] = status
    for i, (st, rl, ck) in enumerate(answers):
        a["status_in"][i], a["result_len"][i], a["result_checksum_type"][i], a["result_checksum"][i] = st, rl, ck[0], ck[1]
    return a


# ---- before the send ----------------------------------------------------------------------------
def contains(base, size, data, length):
    """RDMABuf::contains in 64-bit unsigned sums; a sum that wraps is not contained."""
    if data + length > M64 or base + size > M64:
        return False
    return base <= data and data + length <= base + size


def own_range_ok(io):
    """validateWriteDataRange: chunkSize == 0 || offset + length > chunkSize, the sum in uint32_t."""
    return not (io["chunk_size"] == 0 or ((int(io["offset"]) + int(io["length"])) & M32) > io["chunk_size"])


def buffer_ok(io):
    return io["buf_base"] != 0 and io["data"] != 0 and contains(int(io["buf_base"]), int(io["buf_size"]),
                                                               int(io["data"]), int(io["length"]))


class Prepared:
    def __init__(self, status, checksum, checksum_type, send_inline, info, readable):
        self.status, self.checksum, self.checksum_type, self.send_inline = status, checksum, checksum_type, send_inline
        self.info, self.readable = info, readable

    def apply(self, ios):
        out = ios.copy()
        out["status"], out["checksum"], out["checksum_type"], out["send_inline"] = (
            self.status, self.checksum, self.checksum_type, self.send_inline)
        return out

    def updates(self, ios, before):
        """The update records after the call: only the request fields of `before` change."""
        u = before.copy()
        for i in range(ios.size):
            if self.status[i] == 0:
                u["payload"][i], u["offset"][i], u["length"][i] = ios["data"][i], ios["offset"][i], ios["length"][i]
                u["update_type"][i], u["flags"][i] = UPDATE_WRITE, 0
                u["write_checksum_type"][i], u["write_checksum"][i] = self.checksum_type[i], self.checksum[i]
            else:
                u["update_type"][i] = 0
        return u


def prepare_model(ios, ctype, max_len, max_inline, verify, orc, read_bytes=None):
    n = ios.size
    status = np.zeros(n, dtype=np.int32)
    survivors = []
    bad = rng_fail = 0
    for i in range(n):                                   # rule 1, then validateWriteDataRange
        if ios["length"][i] > max_len:
            status[i] = INVALID_ARG
            bad += 1
        elif not own_range_ok(ios[i]):
            status[i] = CLIENT_INVALID_ARG
            rng_fail += 1
        else:
            survivors.append(i)
    poisoned = any(not buffer_ok(ios[i]) for i in survivors)   # validateDataRange: all or nothing
    if poisoned:
        status[survivors] = CLIENT_INVALID_ARG
    readable = [i for i in survivors if buffer_ok(ios[i])]     # valid by themselves: may be read with VERIFY
    checksum = np.zeros(n, dtype=np.uint32)
    ctypes_ = np.zeros(n, dtype=np.uint8)
    inline = np.zeros(n, dtype=np.uint8)
    for i in range(n):                                   # sendWriteRequest
        if status[i] != 0:
            continue
        if verify:
            ln = int(ios["length"][i])
            ck = orc.create(ctype, read_bytes(int(ios["data"][i]), ln) if ln else b"")
            assert ck[0] == ctype
            ctypes_[i], checksum[i] = ck[0], ck[1]
        inline[i] = 1 if ios["length"][i] <= max_inline else 0
    hashed = sum(int(ios["length"][i]) for i in readable) if verify else 0
    info = np.array([int((status == 0).sum()), rng_fail, bad, 1 if poisoned else 0, int(inline.sum()), hashed & M32,
                     hashed >> 32, 0], dtype=np.uint32)
    return Prepared(status, checksum, ctypes_, inline, info, readable if verify else [])


# ---- after the answers --------------------------------------------------------------------------
def combine(acc, other, length, orc):
    """ChecksumInfo::combine -> (acc, error code or 0)."""
    if acc[0] != NONE and acc[0] != other[0]:
        return acc, STORAGE_MISMATCH                     # :180-183, before the length is looked at
    if length == 0:
        return acc, 0                                    # :184
    if acc[0] == NONE:
        return other, 0                                  # :186-188
    f = orc.crc32c_combine if acc[0] == CRC32C else orc.crc32_combine
    return (acc[0], int(f(~acc[1] & M32, other[1], length))), 0


def write_file(answers, orc):
    """writeFile's loop over one file's IOs; answers = [(final status, result_len, length, (type, value))]
    -> (status, length, (type, value), index of the IO that ended it or None)."""
    ck, total = (NONE, 0), 0                             # storage::ChecksumInfo checksum;
    for k, (st, succ, length, rck) in enumerate(answers):
        if st != 0:                                      # CO_RETURN_AND_LOG_ON_ERROR(writeIO.result.lengthInfo)
            return st, 0, (NONE, 0), k
        if rck[0] > CRC32:                               # no such ChecksumType: the call's own code
            return INVALID_ARG, 0, (NONE, 0), k
        if succ != length:
            return INVALID_FORMAT, 0, (NONE, 0), k
        ck, err = combine(ck, rck, succ, orc)
        if err:
            return err, 0, (NONE, 0), k
        total += succ
    return 0, total, ck, None


class Completed:
    def __init__(self, ios, files, failed, info):
        self.ios, self.files, self.failed, self.info = ios, files, failed, info


def complete_model(ios, file_off, orc, updates=None, expected=None):
    """ios as complete receives them; updates: FROM_UPDATES.  -> the IO array after the call, the
    file records, the full failed list, d_info."""
    out = ios.copy()
    n = ios.size
    if updates is not None:
        for i in range(n):
            if out["status"][i] == 0:
                out["status_in"][i], out["result_len"][i] = updates["status"][i], updates["length"][i]
                out["result_checksum"][i], out["result_checksum_type"][i] = (
                    updates["out_checksum"][i], updates["out_checksum_type"][i])
    final = [int(out["status"][i]) if out["status"][i] != 0 else int(out["status_in"][i]) for i in range(n)]
    failed = [i for i in range(n) if final[i] != 0]      # collectFailedOps, batch order
    data_len = sum(int(out["result_len"][i]) for i in range(n) if final[i] == 0)
    off = np.zeros(1, dtype=np.uint64) if file_off is None else np.asarray(file_off, dtype=np.uint64)
    files = np.zeros(off.size - 1, dtype=FILE)
    for f in range(files.size):
        hi = min(int(off[f + 1]), n)
        lo = min(int(off[f]), hi)
        ans = [(final[i], int(out["result_len"][i]), int(out["length"][i]),
                (int(out["result_checksum_type"][i]), int(out["result_checksum"][i]))) for i in range(lo, hi)]
        status, length, ck, ender = write_file(ans, orc)
        failed_io = NO_IO if ender is None else lo + ender
        if expected is not None and status == 0 and ck[1] != int(expected[f]):   # Bench.cc check: .value only
            status, failed_io = CLIENT_MISMATCH, NO_IO
        files[f] = (length, ck[1], ck[0], (0, 0, 0), status, failed_io)
    mism = 0 if expected is None else int(((files["status"] == CLIENT_MISMATCH) & (files["failed_io"] == NO_IO)).sum())
    info = np.array([len(failed), n - len(failed), data_len & M32, data_len >> 32, int((files["status"] != 0).sum()),
                     mism, 0, 0], dtype=np.uint32)
    return Completed(out, files, np.array(failed, dtype=np.uint32), info)


# ---- case builders ------------------------------------------------------------------------------
LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097)
SLOT = 4352  # bytes of arena per grid IO: 4097 + 15 of residue, rounded up to 256


def arena_bytes(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.uint64))]).astype(np.uint64)


def grid_rows(base, arena_size):
    """Every length of LENGTHS with `data` at every residue mod 16, each IO in the one buffer
    [base, base + arena_size), at the start of its chunk."""
    rows, slot = [], 0
    for res in range(16):
        for length in LENGTHS:
            rows.append((base + slot * SLOT + res, base, arena_size, 0, length, 4097))
            slot += 1
    return rows


def grid_bytes():
    return 16 * len(LENGTHS) * SLOT


def random_rows(rng, n, base, arena_size, max_length=16, chunk_size=64):
    """n valid IOs of 0..max_length bytes anywhere in the buffer."""
    at = rng.integers(0, arena_size - max_length, n)
    ln = rng.integers(0, max_length + 1, n)
    off = rng.integers(0, chunk_size - max_length + 1, n)
    return [(base + int(at[i]), base, arena_size, int(off[i]), int(ln[i]), chunk_size) for i in range(n)]


def prepare_blocks(offset, end, chunk_size):
    """FileWrapper::prepareBlocks (FileWrapper.cc:15-28): (chunk index, offset in chunk, length)."""
    blocks = []
    while offset < end:
        nxt = min((offset // chunk_size + 1) * chunk_size, end)
        blocks.append((offset // chunk_size, offset % chunk_size, nxt - offset))
        offset = nxt
    return blocks


def random_answers(rng, n, types=(CRC32C,), zero_every=0, big=False):
    """n good answers without data: (0, result_len, (type, value)) and the matching lengths."""
    ans, lengths = [], []
    for k in range(n):
        t = int(types[int(rng.integers(0, len(types)))])
        r = int(rng.integers(1, 1 << 32 if big else 1 << 20))
        if zero_every and k % zero_every == zero_every - 1:
            r = 0
        ans.append((0, r, (t, int(rng.integers(0, 1 << 32)))))
        lengths.append(r)
    return ans, lengths
