"""The model of hf3fs_crc_client_write_prepare / _complete (tests/client_write_cases.py) against
examples worked by hand, one per rule of StorageClientImpl.cc:889-951, 994-1015, 1878-1901 and per
step of FileWrapper.cc:218-248 over Common.h:179-198; the record layouts, the binding and every
argument error.  No GPU: the CRC values come from the CPU oracle, and where a fold must give a
known value it is the checksum of the concatenated bytes."""
import ctypes
import re

import numpy as np
import pytest

import client_write_cases as wc

A, B, C = b"the first block of the file", b"and the second block, a longer one", b"!tail"
BASE, SIZE = 0x7000, 0x1000


def crc(orc, t, data):
    return tuple(orc.create(t, data))


def reader(data, base=BASE):
    return lambda addr, n: data[addr - base:addr - base + n].tobytes()


def prep(rows, orc, verify=True, max_len=4096, max_inline=0, data=None, ctype=wc.CRC32C):
    ios = wc.ios_array(rows)
    read = (lambda a, n: pytest.fail("no byte may be read")) if data is None else reader(data)
    return wc.prepare_model(ios, ctype, max_len, max_inline, verify, orc, read)


# ---- before the send ---------------------------------------------------------------------------
def test_own_range_is_uint32_arithmetic(orc):
    rows = [(BASE, BASE, SIZE, 60, 4, 64),                       # offset + length == chunk_size: passes
            (BASE, BASE, SIZE, 61, 4, 64),                       # one more: 7002
            (BASE, BASE, SIZE, 0, 0, 0),                         # chunk_size 0: 7002
            (BASE, BASE, SIZE, 0xFFFFFFF0, 0x20, 0x100)]         # the sum wraps to 0x10 <= 0x100: passes
    p = prep(rows, orc, verify=False)
    assert p.status.tolist() == [0, 7002, 7002, 0]
    assert p.info.tolist() == [2, 2, 0, 0, 0, 0, 0, 0]           # (the zero-length IO would be inline: it is not sent)
    assert p.checksum.tolist() == [0] * 4 and p.checksum_type.tolist() == [wc.NONE] * 4


def test_containment_edges_and_wrapping_sums(orc):
    assert wc.contains(BASE, SIZE, BASE, 0) and wc.contains(BASE, SIZE, BASE, SIZE)
    assert wc.contains(BASE, SIZE, BASE + SIZE - 8, 8) and not wc.contains(BASE, SIZE, BASE + SIZE - 8, 9)
    assert not wc.contains(BASE, SIZE, BASE - 1, 8) and wc.contains(BASE, SIZE, BASE + SIZE, 0)
    assert not wc.contains(wc.M64 - 8, 16, wc.M64 - 8, 4)        # base + size wraps
    assert not wc.contains(1, wc.M64 - 1, wc.M64 - 2, 8)         # data + length wraps


def test_one_offender_poisons_every_survivor_but_not_the_dropped(orc):
    data = np.frombuffer(A + B, dtype=np.uint8)
    good = (BASE, BASE, SIZE, 0, len(A), 64)
    for offender in [(BASE + SIZE - 3, BASE, SIZE, 0, 4, 64), (0, BASE, SIZE, 0, 4, 64), (BASE, 0, SIZE, 0, 4, 64),
                     (BASE - 1, BASE, SIZE, 0, 4, 64)]:
        for rows in ([offender, good, good], [good, good, offender], [offender]):
            p = prep(rows + [(BASE, BASE, SIZE, 63, 4, 64), (BASE, BASE, SIZE, 0, 5000, 8192)], orc, data=data)
            assert p.status.tolist() == [7002] * len(rows) + [7002, 3]
            assert p.info.tolist()[:5] == [0, 1, 1, 1, 0] and (p.checksum == 0).all() and (p.checksum_type == 0).all()
            assert p.readable == [i for i, r in enumerate(rows) if r is good]   # valid by themselves: may be read
            assert p.info[5] == len(A) * len(p.readable)
    # an IO that rule 1 or rule 2 dropped is never looked at by the buffer check
    rows = [good, (0, 0, 0, 63, 4, 64), (0, 0, 0, 0, 5000, 8192)]
    p = prep(rows, orc, data=data)
    assert p.status.tolist() == [0, 7002, 3] and p.info.tolist() == [1, 1, 1, 0, 0, len(A), 0, 0]
    assert (p.checksum_type[0], p.checksum[0]) == crc(orc, wc.CRC32C, A)


@pytest.mark.parametrize("t", [wc.CRC32C, wc.CRC32])
def test_checksum_and_inline(orc, t):
    data = np.frombuffer(A + B, dtype=np.uint8)
    rows = [(BASE, BASE, SIZE, 0, len(A), 64), (BASE + len(A), BASE, SIZE, 8, len(B), 64), (BASE + 5, BASE, SIZE, 0, 0, 64)]
    p = prep(rows, orc, data=data, max_inline=len(A), ctype=t)
    assert list(zip(p.checksum_type.tolist(), p.checksum.tolist())) == [crc(orc, t, A), crc(orc, t, B), (t, wc.M32)]
    assert p.send_inline.tolist() == [1, 0, 1] and p.info.tolist() == [3, 0, 0, 0, 2, len(A + B), 0, 0]
    q = prep(rows, orc, verify=False, max_inline=0)
    assert q.checksum.tolist() == [0, 0, 0] and q.checksum_type.tolist() == [0, 0, 0] and q.send_inline.tolist() == [0, 0, 1]
    # the update records: only the request fields move
    before = np.frombuffer(bytes(range(56)) * 3, dtype=wc.UPDATE)
    ios = wc.ios_array(rows)
    after = p.updates(ios, before)
    for f in wc.UPDATE.names:
        moved = f in ("payload", "offset", "length", "update_type", "write_checksum_type", "flags", "write_checksum")
        if not moved:
            assert (after[f] == before[f]).all(), f
    assert after["update_type"].tolist() == [1, 1, 1] and after["payload"].tolist() == [r[0] for r in rows]


# ---- after the answers -------------------------------------------------------------------------
def ans(ck, n, status=0, length=None):
    return (status, n, n if length is None else length, ck)


@pytest.mark.parametrize("t", [wc.CRC32C, wc.CRC32])
def test_fold_of_whole_blocks_is_the_checksum_of_the_file(orc, t):
    answers = [ans(crc(orc, t, x), len(x)) for x in (A, B, C)]
    assert wc.write_file(answers, orc) == (0, len(A + B + C), crc(orc, t, A + B + C), None)
    assert wc.write_file([], orc) == (0, 0, (wc.NONE, 0), None)


def test_first_ender_wins_and_the_own_checks_come_first(orc):
    a, b = crc(orc, wc.CRC32C, A), crc(orc, wc.CRC32C, B)
    for at in range(3):
        answers = [ans(a, len(A)), ans(b, len(B)), ans(a, len(A))]
        answers[at] = ans(b, 7, status=4010)
        assert wc.write_file(answers, orc) == (4010, 0, (wc.NONE, 0), at)
    assert wc.write_file([ans(a, len(A)), ans(b, 3, status=7003), ans(b, 3, status=4010)], orc)[::3] == (7003, 1)
    assert wc.write_file([ans(a, len(A)), ans(b, 9, length=10)], orc) == (33, 0, (wc.NONE, 0), 1)         # short write
    assert wc.write_file([ans(a, len(A)), ans((7, 1), 4)], orc) == (3, 0, (wc.NONE, 0), 1)                 # unknown type
    # an IO that fails by itself and is typed otherwise: its own code, not 4080
    assert wc.write_file([ans(a, len(A)), ans((wc.CRC32, 1), 4, length=5)], orc)[0] == 33


def test_type_check_stands_before_the_zero_length_return(orc):
    a = crc(orc, wc.CRC32C, A)
    other0 = ans((wc.CRC32, 9), 0)
    # in front of the typed run the accumulator is NONE: it passes and changes nothing
    assert wc.write_file([other0, ans(a, len(A))], orc) == (0, len(A), a, None)
    # behind it the check fires although the length is 0
    assert wc.write_file([ans(a, len(A)), other0], orc) == (4080, 0, (wc.NONE, 0), 1)
    # a NONE answer behind a typed accumulator, with or without bytes
    assert wc.write_file([ans(a, len(A)), ans((wc.NONE, 0), 0)], orc)[::3] == (4080, 1)
    assert wc.write_file([ans(a, len(A)), ans((wc.NONE, 0), 4)], orc)[::3] == (4080, 1)
    # a zero-length typed answer does not adopt: the next typed one with bytes does, whatever its type
    b2 = crc(orc, wc.CRC32, B)
    assert wc.write_file([ans((wc.CRC32C, 5), 0), ans(b2, len(B))], orc) == (0, len(B), b2, None)


def test_all_none_answers_keep_the_last_value(orc):
    assert wc.write_file([ans((wc.NONE, 7), 10), ans((wc.NONE, 9), 3), ans((wc.NONE, 4), 0)], orc) == (0, 13, (wc.NONE, 9), None)
    b = crc(orc, wc.CRC32, B)
    assert wc.write_file([ans((wc.NONE, 7), 10), ans(b, len(B))], orc) == (0, 10 + len(B), b, None)


def test_complete_model_statuses_lists_and_counters(orc):
    a, b, c = (crc(orc, wc.CRC32C, x) for x in (A, B, C))
    ios = wc.ios_array([(0, 0, 0, 0, n, 64) for n in (len(A), len(B), len(C), 4, 4)])
    sent = wc.with_answers(ios, [0, 0, 0, 7002, 0], [(0, len(A), a), (0, len(B), b), (0, len(C), c), (0, 4, a), (7003, 0, (0, 0))])
    whole = crc(orc, wc.CRC32C, A + B + C)
    out = wc.complete_model(sent, [0, 3, 3, 5], orc, expected=[whole[1], 0, 0])
    assert out.failed.tolist() == [3, 4] and out.info.tolist() == [2, 3, len(A + B + C), 0, 1, 0, 0, 0]
    assert [tuple(f)[:3] + tuple(f)[4:] for f in out.files.tolist()] == [
        (len(A + B + C), whole[1], wc.CRC32C, 0, wc.NO_IO), (0, 0, wc.NONE, 0, wc.NO_IO), (0, 0, wc.NONE, 7002, 3)]
    assert out.ios.tobytes() == sent.tobytes()                  # without FROM_UPDATES no IO field moves
    miss = wc.complete_model(sent, [0, 3, 3, 5], orc, expected=[whole[1] ^ 1, 1, 0])
    assert miss.files["status"].tolist() == [7015, 7015, 7002] and miss.files["failed_io"].tolist() == [wc.NO_IO, wc.NO_IO, 3]
    assert miss.info.tolist()[4:6] == [3, 2]
    # FROM_UPDATES: a sent IO's answer is its update record's outcome, a not-sent IO keeps its own
    upd = np.zeros(5, dtype=wc.UPDATE)
    upd["status"], upd["length"] = [0, 4080, 0, 0, 0], [len(A), len(B), len(C), 4, 4]
    upd["out_checksum"], upd["out_checksum_type"] = [a[1], 0, c[1], 1, 2], [1, 0, 1, 1, 1]
    out = wc.complete_model(sent, [0, 3, 3, 5], orc, updates=upd)
    assert out.ios["status_in"].tolist() == [0, 4080, 0, 0, 0] and out.ios["result_checksum"].tolist() == [a[1], 0, c[1], a[1], 2]
    assert out.failed.tolist() == [1, 3] and out.files["status"].tolist() == [4080, 0, 7002]
    assert out.files["failed_io"].tolist() == [1, wc.NO_IO, 3]


def test_prepare_blocks_cuts_at_chunk_ends():
    assert wc.prepare_blocks(0, 0, 64) == []
    assert wc.prepare_blocks(10, 20, 64) == [(0, 10, 10)]
    assert wc.prepare_blocks(60, 200, 64) == [(0, 60, 4), (1, 0, 64), (2, 0, 64), (3, 0, 8)]
    assert wc.prepare_blocks(64, 128, 64) == [(1, 0, 64)]


# ---- the binding -------------------------------------------------------------------------------
def test_record_layouts(hf):
    io = dict(data=0, buf_base=8, buf_size=16, offset=24, length=28, chunk_size=32, checksum=36, checksum_type=40,
              send_inline=41, reserved0=42, status=44, status_in=48, result_len=52, result_checksum=56,
              result_checksum_type=60, reserved1=61)
    fil = dict(length=0, value=8, type=12, reserved=13, status=16, failed_io=20)
    for struct, dtype, mine, want, size in ((hf.ClientWriteIO, hf.client_write_io_dtype(), wc.IO, io, 64),
                                            (hf.ClientWriteFile, hf.client_write_file_dtype(), wc.FILE, fil, 24),
                                            (hf._lib.UpdateIO, hf.update_io_dtype(), wc.UPDATE, None, 56)):
        assert dtype.itemsize == mine.itemsize == size == ctypes.sizeof(struct)
        offsets = {n: getattr(struct, n).offset for n, _ in struct._fields_}
        assert {n: dtype.fields[n][1] for n in dtype.names} == offsets
        assert {n: mine.fields[n][1] for n in mine.names} == offsets
        assert want is None or offsets == want


def test_constants_match_the_header(hf):
    text = open(hf._lib.HEADER).read()
    assert re.search(r"\bHF3FS_CRC_CLIENT_INVALID_ARG = 7002\b", text) and hf.CLIENT_INVALID_ARG == wc.CLIENT_INVALID_ARG
    assert re.search(r"\bHF3FS_CLIENT_WRITE_VERIFY = 1\b", text) and hf.CLIENT_WRITE_VERIFY == wc.VERIFY == 1
    assert re.search(r"\bHF3FS_CLIENT_WRITE_FROM_UPDATES = 2\b", text) and hf.CLIENT_WRITE_FROM_UPDATES == wc.FROM_UPDATES
    assert hf.INVALID_FORMAT == wc.INVALID_FORMAT == 33 and hf._lib.CHECKSUM_MISMATCH == wc.STORAGE_MISMATCH
    words = {"hashed_lo": "HASHED_LO", "hashed_hi": "HASHED_HI", "len_lo": "LEN_LO", "len_hi": "LEN_HI"}
    for prefix, names in (("INFO", wc.PREP_INFO), ("DONE", wc.DONE_INFO)):
        for w, name in enumerate(names):
            if not name.startswith("reserved"):
                assert re.search(rf"\bHF3FS_CLIENT_WRITE_{prefix}_{words.get(name, name.upper())} = {w}\b", text), name
        assert re.search(rf"\bHF3FS_CLIENT_WRITE_{prefix}_WORDS = 8\b", text)
    assert hf.CLIENT_WRITE_INFO_NAMES == wc.PREP_INFO and hf.CLIENT_WRITE_DONE_NAMES == wc.DONE_INFO
    assert hf.CLIENT_WRITE_NONE == wc.NO_IO
    for name in ("hf3fs_crc_client_write_prepare", "hf3fs_crc_client_write_complete",
                 "hf3fs_crc_client_write_scratch_bytes"):
        assert name in hf._lib.SIGNATURES and hasattr(hf._lib.load(), name)


def test_errors_decided_without_a_device(hf):
    """Every argument error is returned before any device is touched: none of these calls needs one."""
    L = hf._lib
    p = 0x1000  # never dereferenced: the call fails first
    good = dict(ctype=wc.CRC32C, ios=p, n=4, info=p, max_len=64, max_inline_bytes=0, flags=wc.VERIFY, updates=p)
    for change in [dict(ctype=wc.NONE), dict(ctype=3), dict(flags=2), dict(flags=0x80000001), dict(ios=None),
                   dict(info=None), dict(n=(1 << 30) + 1)]:
        with pytest.raises(hf.Hf3fsCrcError) as e:
            L.client_write_prepare(**dict(good, **change))
        assert e.value.code == hf.INVALID_ARG, change
    good = dict(ios=p, n=4, info=p, file_off=p, n_files=2, max_ios_per_file=2, flags=wc.FROM_UPDATES, updates=p,
                expected=p, files=p, failed=p, failed_cap=4)
    for change in [dict(flags=1), dict(flags=4), dict(ios=None), dict(info=None), dict(n=(1 << 30) + 1),
                   dict(n_files=(1 << 30) + 1), dict(updates=None, flags=wc.FROM_UPDATES), dict(file_off=None),
                   dict(files=None), dict(failed=None)]:
        with pytest.raises(hf.Hf3fsCrcError) as e:
            L.client_write_complete(**dict(good, **change))
        assert e.value.code == hf.INVALID_ARG, change
    assert L.client_write_scratch_bytes((1 << 30) + 1, 1) == 0 == L.client_write_scratch_bytes(1, (1 << 30) + 1)
    small, big = L.client_write_scratch_bytes(100, 100), L.client_write_scratch_bytes(1 << 20, 1 << 20)
    assert 0 < small < big and big >= (1 << 20) * 20
