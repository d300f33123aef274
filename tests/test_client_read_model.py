"""The model of hf3fs_crc_client_read_batch (tests/client_read_cases.py) against parents merged by
hand, one per branch of StorageClientImpl.cc:1607-1633 and :1720-1737; the record layouts, the
binding and every argument error.  No GPU: the CRC values come from the CPU oracle, and where a
combine must give a known value it is the checksum of the concatenated bytes."""
import ctypes
import re

import numpy as np
import pytest

import client_read_cases as cc

A, B, C = b"the first split child", b"and the second, longer, split child", b"!tail"


def kid(status, ck, read_len, length=None):
    return (status, ck, read_len, read_len if length is None else length)


def crc(orc, t, data):
    return tuple(orc.create(t, data))


# ---- the merge, one parent per branch ----------------------------------------------------------
@pytest.mark.parametrize("t", [cc.CRC32C, cc.CRC32])
def test_clean_split_read_is_the_checksum_of_the_whole(orc, t):
    kids = [kid(0, crc(orc, t, A), len(A), 64), kid(0, crc(orc, t, B), len(B), 64), kid(0, crc(orc, t, C), len(C), 9)]
    assert cc.merge_one(kids, orc) == (0, len(A + B + C), crc(orc, t, A + B + C), None, 137)


def test_take_over_at_child_0_in_the_middle_and_at_the_last(orc):
    good = [kid(0, crc(orc, cc.CRC32C, x), len(x), 50) for x in (A, B, C)]
    sent = (cc.CRC32C, 0x1234)  # what the failing answer carried: it is copied with the status
    for at in range(3):
        kids = list(good)
        kids[at] = kid(cc.CHUNK_NOT_FOUND if at != 1 else 4010, sent, 777, 50)
        status, length, ck, failed, block_len = cc.merge_one(kids, orc)
        assert (status, length, ck, failed, block_len) == (kids[at][0], 0, sent, at, 150)
    # the loop ends there: a second failing child behind the first is never looked at
    kids = [good[0], kid(4010, sent, 0), kid(cc.CHUNK_NOT_FOUND, (cc.NONE, 0), 0)]
    assert cc.merge_one(kids, orc)[:4] == (4010, 0, sent, 1)


def test_verify_mismatch_takes_over_with_the_default_checksum(orc):
    data = np.frombuffer(A + B, dtype=np.uint8).copy()
    base = 0x7000
    right, wrong = crc(orc, cc.CRC32C, A), crc(orc, cc.CRC32C, B)
    ios = cc.ios_array([(base, 64, len(A), 0, right), (base + len(A), 64, len(B), 0, (cc.CRC32C, wrong[1] ^ 4))])
    read = lambda addr, n: data[addr - base:addr - base + n].tobytes()  # noqa: E731
    out = cc.model(ios, [0, 2], cc.CRC32C, 64, True, orc, read)
    assert out.status.tolist() == [0, cc.MISMATCH] and out.computed.tolist() == [right[1], wrong[1]]
    p = out.parents[0]
    assert (p["status"], p["length"], p["checksum_type"], p["checksum"], p["failed_child"]) == (cc.MISMATCH, 0, cc.NONE, 0, 1)
    assert out.info.tolist() == [1, 1, 1, 0]
    # without VERIFY nothing is compared and nothing read: the server's values are merged as they are
    out = cc.model(ios, [0, 2], cc.CRC32C, 64, False, orc, None)
    assert out.status.tolist() == [0, 0] and out.computed.tolist() == [0, 0]
    want = cc.combine(right, (cc.CRC32C, wrong[1] ^ 4), len(B), orc)
    p = out.parents[0]
    assert (p["status"], p["length"], p["checksum_type"], p["checksum"]) == (0, len(A + B), want[0], want[1])
    assert p["failed_child"] == cc.NO_CHILD and out.info.tolist() == [0, 0, 0, 0]


def test_none_typed_children_are_compared_with_the_default_checksum(orc):
    ios = cc.ios_array([(0x7000, 8, 8, 0, (cc.NONE, 0)), (0x7000, 8, 8, 0, (cc.NONE, 5)), (0x7000, 8, 0, 0, (cc.NONE, 5))])
    out = cc.model(ios, None, cc.CRC32C, 8, True, orc, lambda a, n: pytest.fail("a NONE child reads no byte"))
    assert out.status.tolist() == [0, cc.MISMATCH, 0] and out.computed.tolist() == [0, 0, 0]
    assert out.parents["checksum"].tolist() == [0, 0, 5]  # the zero-length child is not compared at all


def test_none_parent_adopts_a_child(orc):
    b = crc(orc, cc.CRC32, B)
    # child 0 is NONE: the first later child with a length is copied, whatever its type
    assert cc.merge_one([kid(0, (cc.NONE, 7), 10), kid(0, b, len(B))], orc) == (0, 10 + len(B), b, None, 10 + len(B))
    # ... a NONE one too (its value moves in), and a typed one after it still fixes the type
    assert cc.merge_one([kid(0, (cc.NONE, 7), 10), kid(0, (cc.NONE, 9), 3)], orc)[2] == (cc.NONE, 9)
    assert cc.merge_one([kid(0, (cc.NONE, 7), 10), kid(0, (cc.NONE, 9), 3), kid(0, b, len(B))], orc)[2] == b
    # from then on the parent is typed: the next child of that type is combined
    c = crc(orc, cc.CRC32, C)
    kids = [kid(0, (cc.NONE, 7), 10), kid(0, b, len(B)), kid(0, c, len(C))]
    assert cc.merge_one(kids, orc)[2] == crc(orc, cc.CRC32, B + C)


def test_type_mismatch_is_ignored_but_its_length_counts(orc):
    a, c = crc(orc, cc.CRC32C, A), crc(orc, cc.CRC32C, C)
    kids = [kid(0, a, len(A)), kid(0, crc(orc, cc.CRC32, B), len(B)), kid(0, (cc.NONE, 0), 4), kid(0, c, len(C))]
    status, length, ck, failed, _ = cc.merge_one(kids, orc)
    assert (status, failed) == (0, None) and length == len(A) + len(B) + 4 + len(C)
    assert ck == crc(orc, cc.CRC32C, A + C)  # as if the two foreign children were not there


def test_zero_length_child_changes_nothing(orc):
    a = crc(orc, cc.CRC32C, A)
    kids = [kid(0, a, len(A)), kid(0, (cc.CRC32C, 0xDEADBEEF), 0, 32)]
    assert cc.merge_one(kids, orc) == (0, len(A), a, None, len(A) + 32)
    # also while the parent is NONE, and child 0 is assigned even with length 0
    assert cc.merge_one([kid(0, (cc.NONE, 3), 0), kid(0, (cc.CRC32C, 8), 0)], orc)[2] == (cc.NONE, 3)
    assert cc.merge_one([kid(0, (cc.CRC32, 3), 0)], orc) == (0, 0, (cc.CRC32, 3), None, 0)


def test_parent_without_children_is_not_initialized(orc):
    assert cc.merge_one([], orc) == (cc.NOT_INITIALIZED, 0, (cc.NONE, 0), None, 0)
    out = cc.model(cc.ios_array([]), [0, 0, 0], cc.CRC32C, 0, True, orc)
    assert out.parents["status"].tolist() == [7003, 7003] and out.info.tolist() == [0, 2, 2, 0]
    assert out.blocks["missing"].tolist() == [0, 0]


def test_length_sum_wraps_at_2_to_32(orc):
    kids = [kid(0, (cc.CRC32C, 1), 0xFFFFFFF0), kid(0, (cc.CRC32C, 2), 0x20), kid(0, (cc.CRC32C, 3), 0xFFFFFFFF)]
    status, length, ck, _, block_len = cc.merge_one(kids, orc)
    assert (status, length, block_len) == (0, 0xF, 0xF)
    # each combine used the child's own 32-bit length, not the wrapped sum
    step = orc.crc32c_combine(~1 & cc.M32, 2, 0x20)
    assert ck == (cc.CRC32C, orc.crc32c_combine(~step & cc.M32, 3, 0xFFFFFFFF))


def test_bad_records(orc):
    rows = [(0x7000, 8, 8, 0, (7, 1)),                # an unknown type, with or without VERIFY
            (0x7000, 8, 8, 0, (cc.CRC32, 1)),         # the other CRC type: VERIFY only
            (0x7000, 8, 9, 0, (cc.NONE, 0)),          # more read than asked for: VERIFY only
            (0, 8, 8, 0, (cc.NONE, 0)),               # no buffer: VERIFY only
            (0x7000, 99, 65, 0, (cc.NONE, 0)),        # longer than max_len: VERIFY only
            (0, 8, 9, 4010, (7, 1))]                  # a failed IO keeps its status whatever else it holds
    ios = cc.ios_array(rows)
    assert cc.model(ios, None, cc.CRC32C, 64, True, orc).status.tolist() == [3, 3, 3, 3, 3, 4010]
    assert cc.model(ios, None, cc.CRC32C, 64, False, orc).status.tolist() == [3, 0, 0, 0, 0, 4010]


def test_block_records_feed_the_file_digest(orc):
    """FileWrapper.cc:132-163 over the model's block records: a hole (7007) and a short read."""
    a, b = crc(orc, cc.CRC32C, A), crc(orc, cc.CRC32C, B)
    ios = cc.ios_array([(0, 64, len(A), 0, a), (0, 64, 0, cc.CHUNK_NOT_FOUND, (cc.NONE, 0)), (0, 64, len(B), 0, b)])
    out = cc.model(ios, None, cc.CRC32C, 64, False, orc)
    assert out.blocks["missing"].tolist() == [0, 1, 0] and out.info.tolist() == [1, 1, 0, 0]
    status, ck = orc.file_digest(cc.digest_blocks(out.blocks), fill_zero=True)
    whole = A + bytes(64 - len(A)) + bytes(64) + B + bytes(64 - len(B))
    assert status == 0 and tuple(ck) == crc(orc, cc.CRC32C, whole)
    assert orc.file_digest(cc.digest_blocks(out.blocks), fill_zero=False)[0] == 33  # block 0 is short


# ---- the binding -------------------------------------------------------------------------------
def test_record_layouts(hf):
    io = dict(data=0, length=8, read_len=12, status_in=16, checksum=20, checksum_type=24, reserved0=25, computed=28,
              status=32, reserved1=36)
    res = dict(length=0, checksum=4, checksum_type=8, reserved=9, status=12, failed_child=16, block_len=20)
    blk = dict(read_len=0, block_len=8, checksum=16, checksum_type=20, missing=21, reserved=22)
    for struct, dtype, mine, want, size in ((hf.ClientReadIO, hf.client_read_io_dtype(), cc.IO, io, 40),
                                            (hf.ClientReadResult, hf.client_read_result_dtype(), cc.RESULT, res, 24),
                                            (None, hf.block_digest_dtype(), cc.BLOCK, blk, 24)):
        assert dtype.itemsize == mine.itemsize == size
        assert {n: dtype.fields[n][1] for n in dtype.names} == want
        assert {n: mine.fields[n][1] for n in mine.names} == want
        if struct is not None:
            assert ctypes.sizeof(struct) == size
            assert {n: getattr(struct, n).offset for n, _ in struct._fields_} == want


def test_constants_match_the_header(hf):
    text = open(hf._lib.HEADER).read()
    assert re.search(r"\bHF3FS_CLIENT_READ_VERIFY = 1\b", text) and hf.CLIENT_READ_VERIFY == cc.VERIFY == 1
    assert re.search(r"\bHF3FS_CRC_CLIENT_NOT_INITIALIZED = 7003\b", text)
    assert (hf.CLIENT_NOT_INITIALIZED, hf.CHUNK_NOT_FOUND) == (cc.NOT_INITIALIZED, cc.CHUNK_NOT_FOUND) == (7003, 7007)
    assert hf._lib.CLIENT_CHECKSUM_MISMATCH == cc.MISMATCH == 7015 and hf.INVALID_ARG == cc.INVALID_ARG
    for w, name in enumerate(cc.INFO[:3]):
        assert re.search(rf"\bHF3FS_CLIENT_READ_INFO_{name.upper()} = {w}\b", text), name
    assert re.search(r"\bHF3FS_CLIENT_READ_INFO_WORDS = 4\b", text)
    assert hf.CLIENT_READ_INFO_NAMES == cc.INFO and hf.CLIENT_READ_INFO_WORDS == 4
    assert hf.CLIENT_READ_NONE == cc.NO_CHILD
    for name in ("hf3fs_crc_client_read_batch", "hf3fs_crc_client_read_scratch_bytes"):
        assert name in hf._lib.SIGNATURES and hasattr(hf._lib.load(), name)


def test_errors_decided_without_a_device(hf):
    """Every argument error is returned before any device is touched: none of these calls needs one."""
    L = hf._lib
    p = 0x1000  # never dereferenced: the call fails first
    good = dict(ctype=cc.CRC32C, ios=p, n_ios=4, info=p, parent_off=p, n_parents=2, max_children=2, max_len=64,
                flags=cc.VERIFY, parents=p, blocks=p)
    cases = [dict(ctype=cc.NONE), dict(ctype=3),                     # the type
             dict(flags=2), dict(flags=0x80000001),                  # unknown flag bits
             dict(ios=None),                                         # null d_ios with n_ios > 0
             dict(info=None),                                        # null d_info
             dict(parent_off=None),                                  # null offsets need n_parents == n_ios
             dict(parents=None, blocks=None, flags=0),               # nothing to do
             dict(n_ios=(1 << 30) + 1), dict(n_parents=(1 << 30) + 1)]
    for change in cases:
        kw = dict(good, **change)
        with pytest.raises(hf.Hf3fsCrcError) as e:
            L.client_read_batch(**kw)
        assert e.value.code == hf.INVALID_ARG, change
    assert L.client_read_scratch_bytes((1 << 30) + 1, 1) == 0 == L.client_read_scratch_bytes(1, (1 << 30) + 1)
    small, big = L.client_read_scratch_bytes(100, 100), L.client_read_scratch_bytes(1 << 20, 1 << 20)
    assert 0 < small < big and big >= (1 << 20) * 20
