"""Model and case builders of hf3fs_crc_client_read_batch (the client's batchRead completion).

`model` restates the two loops of StorageClientImpl::batchRead in the reference's own shape: the
per-IO verify ladder (src/client/storage/StorageClientImpl.cc:1720-1737) and the split-read merge
(:1607-1633), sequential, lengths in uint32 arithmetic, ChecksumInfo::combine with its four
outcomes written out (src/fbs/storage/Common.h:179-198) and its return value dropped.  It shares
no code with 3fs_amd/csrc/client_read_plan.h: the CRC arithmetic is the CPU oracle's, the record
layouts are written out here again (tests/test_client_read_model.py compares them with the
package's and checks the model against parents merged by hand).
"""
import numpy as np

IO = np.dtype([("data", "<u8"), ("length", "<u4"), ("read_len", "<u4"), ("status_in", "<i4"), ("checksum", "<u4"),
               ("checksum_type", "u1"), ("reserved0", "u1", (3,)), ("computed", "<u4"), ("status", "<i4"),
               ("reserved1", "<u4")])
RESULT = np.dtype([("length", "<u4"), ("checksum", "<u4"), ("checksum_type", "u1"), ("reserved", "u1", (3,)),
                   ("status", "<i4"), ("failed_child", "<u4"), ("block_len", "<u4")])
BLOCK = np.dtype([("read_len", "<u8"), ("block_len", "<u8"), ("checksum", "<u4"), ("checksum_type", "u1"),
                  ("missing", "u1"), ("reserved", "u1", (2,))])
assert IO.itemsize == 40 and RESULT.itemsize == 24 and BLOCK.itemsize == 24

NONE, CRC32C, CRC32 = 0, 1, 2
INVALID_ARG, NOT_INITIALIZED, CHUNK_NOT_FOUND, MISMATCH = 3, 7003, 7007, 7015
VERIFY = 1
NO_CHILD = 0xFFFFFFFF
INFO = ("bad_children", "bad_parents", "hard_parents", "reserved")
M32 = 0xFFFFFFFF
POISON_OUT = 0xA5A5A5A5  # what the builders leave in `computed`; status gets -2: the call must overwrite both


def ios_array(rows):
    """rows of (data, length, read_len, status_in, (type, value)) -> an IO array with poisoned outputs."""
    a = np.zeros(len(rows), dtype=IO)
    for i, (data, length, read_len, status_in, ck) in enumerate(rows):
        a[i] = (data, length, read_len, status_in, ck[1], ck[0], (0, 0, 0), POISON_OUT, -2, 0)
    return a


def bad_record(io, ctype, max_len, verify):
    """Records the call refuses with status 3 (include/hf3fs_crc.h): the reference cannot hold them."""
    if io["status_in"] != 0:
        return False
    if io["checksum_type"] > CRC32:
        return True
    if not verify:
        return False
    if io["checksum_type"] not in (NONE, ctype):
        return True
    if io["read_len"] > max_len or io["read_len"] > io["length"]:
        return True
    return io["read_len"] > 0 and io["data"] == 0


def verify_one(io, ctype, max_len, verify, read_bytes, orc):
    """:1720-1737 for one readIO -> (status, computed, result.checksum as (type, value))."""
    ck = (int(io["checksum_type"]), int(io["checksum"]))
    if bad_record(io, ctype, max_len, verify):
        return INVALID_ARG, 0, ck
    if not verify:                                            # options.verifyChecksum()
        return int(io["status_in"]), 0, ck
    if io["status_in"] == 0 and io["read_len"] > 0:           # lengthInfo && *lengthInfo > 0
        if ck[0] == NONE:
            local = (NONE, 0)                                 # create(NONE, ...) (Common.h:150)
        else:
            local = tuple(orc.create(ck[0], read_bytes(int(io["data"]), int(io["read_len"]))))
        if local != ck:
            return MISMATCH, local[1], (NONE, 0)              # setErrorCodeOfOp: result = IOResult(7015)
        return 0, local[1], ck
    return int(io["status_in"]), 0, ck


def combine(acc, other, length, orc):
    """ChecksumInfo::combine with the return value dropped (:1630)."""
    if acc[0] != NONE and acc[0] != other[0]:
        return acc                                            # makeError(kChecksumMismatch): nothing changed
    if length == 0:
        return acc
    if acc[0] == NONE:
        return other
    f = orc.crc32c_combine if acc[0] == CRC32C else orc.crc32_combine
    return (acc[0], int(f(~acc[1] & M32, other[1], length)))


def merge_one(children, orc):
    """:1607-1633 for one parent; children = [(status, (type, value), read_len, length)] ->
    (status, length, (type, value), failed index or None, block_len)."""
    status, length, ck, failed = NOT_INITIALIZED, 0, (NONE, 0), None  # IOResult()
    for k, (st, cck, read_len, _length) in enumerate(children):
        if st != 0:                                           # !bool(splittedIO.result.lengthInfo)
            status, length, ck, failed = st, 0, cck, k        # parentIO->result = splittedIO.result
            break
        elif k == 0:
            status, length, ck = 0, read_len, cck
        else:
            length = (length + read_len) & M32                # uint32_t + uint32_t
            ck = combine(ck, cck, read_len, orc)
    block_len = sum(c[3] for c in children) & M32
    return status, length, ck, failed, block_len


class Outcome:
    """What one call must produce."""

    def __init__(self, computed, status, parents, blocks, info):
        self.computed, self.status, self.parents, self.blocks, self.info = computed, status, parents, blocks, info


def model(ios, parent_off, ctype, max_len, verify, orc, read_bytes=None):
    """parent_off: n_parents + 1 offsets, or None (every IO its own parent)."""
    n = ios.size
    after = [verify_one(ios[i], ctype, max_len, verify, read_bytes, orc) for i in range(n)]
    off = np.arange(n + 1, dtype=np.uint64) if parent_off is None else np.asarray(parent_off, dtype=np.uint64)
    n_parents = off.size - 1
    parents = np.zeros(n_parents, dtype=RESULT)
    blocks = np.zeros(n_parents, dtype=BLOCK)
    for p in range(n_parents):
        lo, hi = int(off[p]), int(off[p + 1])
        kids = [(after[i][0], after[i][2], int(ios["read_len"][i]), int(ios["length"][i])) for i in range(lo, hi)]
        status, length, ck, failed, block_len = merge_one(kids, orc)
        parents[p] = (length, ck[1], ck[0], (0, 0, 0), status, NO_CHILD if failed is None else lo + failed, block_len)
        blocks[p] = (length, block_len, ck[1], ck[0], 1 if status == CHUNK_NOT_FOUND else 0, (0, 0))
    info = np.array([sum(1 for a in after if a[0] != 0), int((parents["status"] != 0).sum()),
                     int(((parents["status"] != 0) & (parents["status"] != CHUNK_NOT_FOUND)).sum()), 0], dtype=np.uint32)
    return Outcome(np.array([a[1] for a in after], dtype=np.uint32), np.array([a[0] for a in after], dtype=np.int32),
                   parents, blocks, info)


def digest_blocks(blocks):
    """BLOCK records -> the tuples oracle.file_digest takes."""
    return [(int(b["read_len"]), int(b["block_len"]), (int(b["checksum_type"]), int(b["checksum"])), bool(b["missing"]))
            for b in blocks]


# ---- case builders ---------------------------------------------------------------------------
VERIFY_LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4099)
SLOT = 4352  # bytes of arena per verify child: 4099 + 15 of residue, rounded up to 256


def arena_bytes(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def verify_grid(base, arena, ctype, kind, orc):
    """The children of the verify grid for one kind: every address residue 0-15 x VERIFY_LENGTHS,
    each once with the right server checksum and once with one bit wrong (in the data when there
    is a byte to flip, else in the value).  Corrupts `arena` (host bytes) in place; base = the
    device address arena[0] will have, 16-byte aligned.  kind:
      "typed"     checksum_type = ctype
      "none"      NONE-typed children, server value 0 / non-zero in turn
      "failed"    status_in != 0 (nothing is compared whatever the bytes are)
      "foreign"   the other CRC type: status 3
    -> (IO array, set of indices that must come out 7015)."""
    rows, injected = [], set()
    slot = 0
    for res in range(16):
        for length in VERIFY_LENGTHS:
            for wrong in (False, True):
                at = slot * SLOT + res
                slot += 1
                data = arena[at:at + length]
                t = {"typed": ctype, "none": NONE, "failed": ctype, "foreign": CRC32 if ctype == CRC32C else CRC32C}[kind]
                value = 0 if t == NONE else orc.create(t, data.tobytes())[1]
                if wrong:
                    if kind == "none" or length == 0:
                        value ^= 1 << (slot % 32)
                    else:
                        arena[at + (slot * 7) % length] ^= 1 << (slot % 8)
                status_in = (CHUNK_NOT_FOUND if slot % 2 else 4010) if kind == "failed" else 0
                rows.append((base + at, length + (slot % 3), length, status_in, (t, value)))
                if wrong and status_in == 0 and length > 0 and kind in ("typed", "none"):
                    injected.add(len(rows) - 1)
    return ios_array(rows), injected


def verify_grid_bytes():
    return 16 * len(VERIFY_LENGTHS) * 2 * SLOT


def random_children(rng, n, fail_at=(), types=(CRC32C,), big=False, zero_every=0):
    """n children of a split read without data (for calls without VERIFY): random values, lengths
    to 2^32 - 1 with big else to 2^20; fail_at: indices whose status_in is an error."""
    rows = []
    for k in range(n):
        t = int(types[int(rng.integers(0, len(types)))])
        r = int(rng.integers(0, 1 << 32 if big else 1 << 20))
        if zero_every and k % zero_every == zero_every - 1:
            r = 0
        st = 0
        if k in fail_at:
            st = CHUNK_NOT_FOUND if k % 2 == 0 else 4010
        rows.append((0, int(rng.integers(0, 1 << 32)), r, st, (t, int(rng.integers(0, 1 << 32)))))
    return rows


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.uint64))]).astype(np.uint64)
