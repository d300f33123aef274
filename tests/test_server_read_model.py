"""The Python model of hf3fs_crc_server_read_prepare / _complete (tests/server_read_cases.py) against
requests worked by hand from the reference's lines, one at least for every rung; the record layouts
against the package's ctypes mirrors and the header's static_asserts; the binding; every argument
error (answered before a device is touched, so no GPU is needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

import server_read_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL, BIG = 64 << 10, 1 << 20


def one_request(n, **req_fields):
    jobs, reqs = sc.new_jobs(n), sc.new_reqs(1)
    for k, v in req_fields.items():
        reqs[k] = v
    return jobs, reqs, sc.offsets([n])


class Arena:
    """Host bytes at made-up addresses."""

    def __init__(self, base, data):
        self.base, self.data = base, bytes(data)

    def read(self, addr, n):
        o = addr - self.base
        assert 0 <= o and o + n <= len(self.data), (hex(addr), n)
        return self.data[o:o + n]


# ---- prepare -------------------------------------------------------------------------------------
def test_alignment_by_hand():
    assert sc.aligned(0, 4096) == (0, 0, 4096)
    assert sc.aligned(1, 1) == (1, 4094, 4096)
    assert sc.aligned(4095, 2) == (4095, 4095, 8192)
    assert sc.aligned(8192, 0) == (0, 0, 0)
    assert sc.aligned(100, 0) == (100, 3996, 4096)


def test_alignment_wraps_like_uint32():
    # offset + length = 2^32 + 904 wraps to 904: tail = 4096 - 904 = 3192; read_len wraps too
    off, length = 0xFFFFF000 + 1000, 4000
    head, tail, read_len = sc.aligned(off, length)
    assert (head, tail) == (1000, 3192)
    assert read_len == (length + head + tail) & 0xFFFFFFFF == 8192
    jobs, reqs, ro = one_request(1)
    jobs["offset"], jobs["length"], jobs["inner_offset"] = off, length, 1 << 40
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    assert jobs[0]["status"] == 0 and jobs[0]["read_len"] == 8192
    assert jobs[0]["read_offset"] == (1 << 40) + 0xFFFFF000
    assert reqs[0]["total_len"] == 4000 and reqs[0]["total_head"] == 1000 and reqs[0]["total_tail"] == 3192


def test_carve_small_then_big_then_small_from_big():
    # 16 KiB, 48 KiB fill the first small buffer; 128 KiB needs a big one; the next 4 KiB job takes
    # from the big buffer's room, not from a new small one; 1 MiB does not fit what is left
    lengths = [16 << 10, 48 << 10, 128 << 10, 4 << 10, 1 << 20, 4 << 10]
    jobs, reqs, ro = one_request(len(lengths))
    jobs["length"] = lengths
    info = sc.prepare(jobs, reqs, ro, SMALL, BIG)
    assert jobs["status"].tolist() == [0] * 6
    assert jobs["buf_ordinal"].tolist() == [0, 0, 1, 1, 2, 3]
    assert jobs["buf_kind"].tolist() == [sc.BUF_SMALL, sc.BUF_SMALL, sc.BUF_BIG, sc.BUF_BIG, sc.BUF_BIG, sc.BUF_SMALL]
    assert jobs["buf_off"].tolist() == [0, 16 << 10, 0, 128 << 10, 0, 0]
    assert (reqs[0]["n_small"], reqs[0]["n_big"]) == (2, 2)
    assert reqs[0]["status"] == 0 and reqs[0]["failed_job"] == sc.NO_JOB
    assert reqs[0]["total_len"] == sum(lengths)
    assert info == [1, 0, 6, 0, 2, 2, 0, 0]


def test_carve_2019_above_big_buf():
    jobs, reqs, ro = one_request(3)
    jobs["length"] = [4096, BIG + 1, 4096]      # read_len 1 MiB + 4 KiB
    info = sc.prepare(jobs, reqs, ro, SMALL, BIG)
    assert reqs[0]["status"] == sc.RDMA_NO_BUF and reqs[0]["failed_job"] == 1
    assert jobs["status"].tolist() == [sc.RDMA_NO_BUF] * 3 and jobs["read_len"].tolist() == [0] * 3
    assert jobs["buf_kind"].tolist() == [sc.BUF_NONE] * 3
    assert (reqs[0]["n_small"], reqs[0]["n_big"], reqs[0]["total_len"]) == (0, 0, 0)
    assert info == [0, 1, 0, 3, 0, 0, 0, 0]


def test_first_loop_failure_at_a_later_job_beats_an_earlier_carve_failure():
    jobs, reqs, ro = one_request(3)
    jobs["length"] = [4096, BIG + 1, 4096]
    jobs["up_to_date"][2] = 0
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    assert reqs[0]["status"] == sc.TARGET_STATE_INVALID and reqs[0]["failed_job"] == 2
    assert jobs["status"].tolist() == [sc.TARGET_STATE_INVALID] * 3


def test_first_loop_order_within_a_job_and_first_job_wins():
    jobs, reqs, ro = one_request(3)
    jobs["length"], jobs["rdmabuf_size"] = 8192, 4096            # every job: length > rdmabuf.size()
    jobs["up_to_date"][1] = 0
    jobs["target_status"][1] = sc.CHAIN_VERSION_MISMATCH
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    assert reqs[0]["status"] == sc.INVALID_ARG and reqs[0]["failed_job"] == 0
    jobs["rdmabuf_size"][0] = 8192
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    assert reqs[0]["status"] == sc.CHAIN_VERSION_MISMATCH and reqs[0]["failed_job"] == 1
    jobs["target_status"][1] = 0
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    assert reqs[0]["status"] == sc.TARGET_STATE_INVALID and reqs[0]["failed_job"] == 1


def test_aio_prepare_read_by_hand():
    jobs, reqs, ro = one_request(5)
    jobs["offset"], jobs["length"], jobs["inner_offset"] = 5000, 100, 1 << 20
    jobs["meta_status"][0] = sc.CHUNK_METADATA_NOT_FOUND
    jobs["commit_ver"][1], jobs["update_ver"][1] = 3, 4                         # replica, uncommitted
    jobs["engine"][2], jobs["commit_ver"][2], jobs["update_ver"][2] = 1, 3, 4   # engine: nothing is checked
    jobs["meta_status"][3], jobs["engine"][3] = sc.CHUNK_METADATA_GET_ERROR, 1
    info = sc.prepare(jobs, reqs, ro, SMALL, BIG)
    assert jobs["status"].tolist() == [4001, 4004, 0, 4002, 0]
    assert jobs["commit_ver"].tolist() == [1, 3, 4, 1, 1]
    assert jobs["read_offset"].tolist() == [0, 0, (1 << 20) + 4096, 0, (1 << 20) + 4096]
    assert jobs["head_len"].tolist() == [904] * 5 and jobs["read_len"].tolist() == [4096] * 5
    assert jobs["buf_off"].tolist() == [0, 4096, 8192, 12288, 16384]           # a failed job keeps its buffer
    assert info[:4] == [1, 0, 2, 3]
    reqs["read_uncommitted"] = 1
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    assert jobs["status"].tolist() == [4001, 0, 0, 4002, 0]


def test_requests_of_no_job_and_many_requests():
    jobs, reqs = sc.new_jobs(3), sc.new_reqs(4)
    jobs["length"] = 4096
    jobs["up_to_date"][1] = 0
    ro = sc.offsets([0, 1, 0, 2])
    info = sc.prepare(jobs, reqs, ro, SMALL, BIG)
    assert reqs["status"].tolist() == [0, 0, 0, sc.TARGET_STATE_INVALID]
    assert reqs["failed_job"].tolist() == [sc.NO_JOB, sc.NO_JOB, sc.NO_JOB, 1]
    assert reqs["n_small"].tolist() == [0, 1, 0, 0]
    assert info == [3, 1, 1, 2, 1, 0, 0, 0]


# ---- complete ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena(orc):
    rng = np.random.default_rng(7)
    return Arena(0x10000, rng.integers(0, 256, 64 << 10, dtype=np.uint8))


def ready(n, arena, orc, **req_fields):
    """n jobs reading [0, 1000) of 1000-byte chunks into 4 KiB slots of the arena, prepared."""
    jobs, reqs, ro = one_request(n, **req_fields)
    jobs["length"], jobs["chunk_len"], jobs["chunk_checksum_type"] = 1000, 1000, sc.CRC32C
    jobs["localbuf"] = arena.base + 4096 * np.arange(n)
    jobs["res"] = 4096
    for j in jobs:
        j["chunk_checksum"] = orc.create(sc.CRC32C, arena.read(int(j["localbuf"]), 1000))[1]
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    return jobs, reqs, ro


def test_clip_by_hand(arena, orc):
    jobs, reqs, ro = ready(6, arena, orc)
    jobs["offset"], jobs["length"], jobs["chunk_len"] = 100, 500, 1000
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    jobs["res"] = [-5, 50, 100 + 200, 4096, 4096, 0]
    jobs["chunk_len"][4] = 300          # reaches past chunk_len: 300 - 100
    jobs["chunk_len"][5] = 50           # chunk_len below offset: max(0, ...) and res == 0
    sc.complete(jobs, reqs, ro, sc.CRC32C, 4096, arena.read, orc)
    assert jobs["result_status"].tolist() == [sc.CHUNK_READ_FAILED, 0, 0, 0, 0, 0]
    assert jobs["result_len"].tolist() == [0, 0, 200, 500, 200, 0]
    assert jobs["checksum_type"].tolist() == [sc.NONE] + [sc.CRC32C] * 5
    assert jobs["checksum"][1] == 0xFFFFFFFF == jobs["checksum"][5]
    assert jobs["checksum"][2] == orc.create(sc.CRC32C, arena.read(int(jobs["localbuf"][2]) + 100, 200))[1]
    assert reqs[0]["n_ok"] == 5


def test_rung_1_by_hand(arena, orc):
    jobs, reqs, ro = ready(4, arena, orc)
    jobs["chunk_checksum"][0] ^= 1      # a full read reuses the stored value, right or wrong
    jobs["res"][1] = 999                # a short read is hashed
    jobs["chunk_checksum_type"][2] = sc.NONE
    jobs["engine"][3] = 1               # stored {CRC32C, ~fin}
    jobs["chunk_checksum"][3] = 0x12345678
    info, _, _ = sc.complete(jobs, reqs, ro, sc.CRC32C, 4096, arena.read, orc)
    assert jobs["result_status"].tolist() == [0] * 4
    assert jobs["checksum"][0] == jobs["chunk_checksum"][0]
    assert jobs["checksum"][1] == orc.create(sc.CRC32C, arena.read(int(jobs["localbuf"][1]), 999))[1]
    assert jobs["checksum"][2] == orc.create(sc.CRC32C, arena.read(int(jobs["localbuf"][2]), 1000))[1]
    assert jobs["checksum"][3] == 0x12345678 ^ 0xFFFFFFFF
    assert info[sc.DONE_INFO.index("hashed")] == 2
    reqs["checksum_type"] = sc.NONE
    info, _, _ = sc.complete(jobs, reqs, ro, sc.CRC32C, 4096, arena.read, orc)
    assert jobs["checksum_type"].tolist() == [sc.NONE] * 4 and jobs["checksum"].tolist() == [0] * 4
    assert info[sc.DONE_INFO.index("hashed")] == 0


def test_finish_read_and_recalculation_by_hand(arena, orc):
    jobs, reqs, ro = ready(7, arena, orc, recalculate=1)
    jobs["chunk_checksum"][0] ^= 1                       # 4080, the checksum keeps rung 1's value
    jobs["update_ver_now"][1] = 9                        # 4004
    jobs["meta_status_now"][2] = sc.CHUNK_METADATA_NOT_FOUND
    jobs["update_ver_now"][3], jobs["chunk_checksum"][3] = 9, 0   # rung 3 wins: rung 4 is skipped
    jobs["chunk_checksum_type"][4], jobs["chunk_checksum"][4] = sc.NONE, 0    # NONE, stored 0: equal
    jobs["chunk_checksum_type"][5], jobs["chunk_checksum"][5] = sc.NONE, 5    # NONE, stored 5: mismatch
    jobs["engine"][6], jobs["update_ver_now"][6] = 1, 9                        # engine: no finish check
    jobs["chunk_checksum"][6] ^= 0xFFFFFFFF                                    # the engine stores the fin value
    stored0 = int(jobs["chunk_checksum"][0])
    sc.complete(jobs, reqs, ro, sc.CRC32C, 4096, arena.read, orc)
    assert jobs["result_status"].tolist() == [4080, 4004, 4001, 4004, 0, 4080, 0]
    assert jobs["result_len"].tolist() == [0, 0, 0, 0, 1000, 0, 1000]
    assert jobs["checksum"][0] == stored0 and jobs["checksum_type"][0] == sc.CRC32C
    assert jobs["checksum_type"][5] == sc.CRC32C         # hashed: the stored type differs from the request's
    reqs["recalculate"] = 0
    sc.complete(jobs, reqs, ro, sc.CRC32C, 4096, arena.read, orc)
    assert jobs["result_status"].tolist() == [0, 4004, 4001, 4004, 0, 0, 0]


def test_inline_pack_by_hand(arena, orc):
    jobs, reqs = sc.new_jobs(5), sc.new_reqs(3, xmit=sc.XMIT_INLINE)
    ro = sc.offsets([2, 0, 3])
    jobs["offset"], jobs["length"], jobs["chunk_len"] = 10, [5, 7, 0, 3, 4], 4096
    jobs["localbuf"] = arena.base + 4096 * np.arange(5)
    jobs["res"] = 4096
    jobs["res"][3] = -1
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    info, inline, wr = sc.complete(jobs, reqs, ro, sc.CRC32C, 4096, arena.read, orc, inline_cap=16)
    want = b"".join(arena.read(arena.base + 4096 * k + 10, n) for k, n in ((0, 5), (1, 7), (4, 4)))
    assert inline == want and wr.size == 0
    assert jobs["inline_off"].tolist() == [0, 5, 12, 0, 12]
    assert reqs["inline_off"].tolist() == [0, 12, 12] and reqs["inline_bytes"].tolist() == [12, 0, 4]
    assert reqs["n_ok"].tolist() == [2, 0, 2]
    assert info[2:5] == [16, 0, 0]
    info, inline, _ = sc.complete(jobs, reqs, ro, sc.CRC32C, 4096, arena.read, orc, inline_cap=15)
    assert inline is None and info[2:5] == [16, 0, 1]
    assert jobs["result_status"].tolist() == [0, 0, 0, sc.CHUNK_READ_FAILED, 0]


def test_rdma_list_by_hand(arena, orc):
    jobs, reqs = sc.new_jobs(7), sc.new_reqs(2, xmit=sc.XMIT_RDMA)
    ro = sc.offsets([6, 1])
    jobs["offset"], jobs["length"], jobs["chunk_len"] = 4, 100, 4096
    jobs["localbuf"] = arena.base + 4096 * np.arange(7)
    jobs["remote_addr"], jobs["rkey"] = 0x7000 + np.arange(7), 40 + np.arange(7)
    jobs["res"] = 4096
    jobs["has_rkey"][1] = 0
    jobs["length"][2] = 0                   # a zero-length job is listed
    jobs["res"][3] = -1                     # an error is not
    reqs["max_msg_sz"][0] = 99
    jobs["length"][4] = 99
    jobs["localbuf"][5] = 0
    reqs["checksum_type"] = sc.NONE         # (so that job 5's null buffer is RDMAReqBatch::add's to refuse)
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    info, _, wr = sc.complete(jobs, reqs, ro, sc.CRC32C, 4096, arena.read, orc)
    assert jobs["result_status"].tolist() == [3, 3, 0, sc.CHUNK_READ_FAILED, 0, 3, 0]
    assert wr["job"].tolist() == [2, 4, 6] and wr["req"].tolist() == [0, 0, 1]
    assert wr["length"].tolist() == [0, 99, 100] and wr["rkey"].tolist() == [42, 44, 46]
    assert wr["local_addr"].tolist() == [arena.base + 4096 * k + 4 for k in (2, 4, 6)]
    assert reqs["wr_first"].tolist() == [0, 2] and reqs["wr_count"].tolist() == [2, 1]
    assert reqs["wr_fails"].tolist() == [3, 0] and reqs["wr_bytes"].tolist() == [99, 100]
    assert reqs["n_ok"].tolist() == [2, 1]
    assert info[5:7] == [3, 3]


def test_a_job_that_failed_prepare_takes_no_part(arena, orc):
    jobs, reqs, ro = ready(2, arena, orc, xmit=sc.XMIT_INLINE)
    jobs["meta_status"][0] = sc.CHUNK_METADATA_NOT_FOUND
    sc.prepare(jobs, reqs, ro, SMALL, BIG)
    jobs["res"][0] = -1
    _, inline, _ = sc.complete(jobs, reqs, ro, sc.CRC32C, 4096, arena.read, orc, inline_cap=4096)
    assert jobs["result_status"].tolist() == [4001, 0] and jobs["result_len"].tolist() == [0, 1000]
    assert (jobs["checksum_type"][0], jobs["checksum"][0]) == (sc.NONE, 0)
    assert inline == arena.read(int(jobs["localbuf"][1]), 1000)


def test_the_calls_limits(arena, orc):
    jobs, reqs, ro = ready(3, arena, orc)
    jobs["chunk_checksum_type"][0] = sc.CRC32        # a stored type the call does not hash in
    jobs["localbuf"][1], jobs["res"][1] = 0, 999     # bytes to hash behind a null buffer
    jobs["res"][2] = 600                             # above max_len below
    sc.complete(jobs, reqs, ro, sc.CRC32C, 512, arena.read, orc)
    assert jobs["result_status"].tolist() == [3, 3, 3]


# ---- layouts, binding, argument errors -------------------------------------------------------------
def test_layouts_match_the_package_and_the_header(hf):
    for mine, theirs, struct in ((sc.JOB, hf.server_read_job_dtype(), hf.ServerReadJob),
                                 (sc.REQ, hf.server_read_req_dtype(), hf.ServerReadReq),
                                 (sc.WR, hf.server_read_wr_dtype(), hf.ServerReadWr)):
        assert mine == theirs and mine.itemsize == ctypes.sizeof(struct)
        for name in mine.names:
            assert mine.fields[name][1] == getattr(struct, name).offset, name
    assert sc.JOB.itemsize % 64 == 0 and sc.REQ.itemsize % 64 == 0
    with open(os.path.join(REPO, "include", "hf3fs_crc.h")) as f:
        header = f.read()
    checked = 0
    for rec, field, off in re.findall(r"offsetof\(hf3fs_crc_server_read_(job|req|wr), (\w+)\) == (\d+)", header):
        assert {"job": sc.JOB, "req": sc.REQ, "wr": sc.WR}[rec].fields[field][1] == int(off), (rec, field)
        checked += 1
    assert checked == 23
    for rec, size in (("job", 192), ("req", 128), ("wr", 32)):
        assert f"sizeof(hf3fs_crc_server_read_{rec}) == {size}" in header


def test_constants_match_the_package_and_the_header(hf):
    assert (hf.RDMA_NO_BUF, hf.CHUNK_METADATA_NOT_FOUND, hf.CHUNK_METADATA_GET_ERROR, hf.CHUNK_NOT_COMMIT,
            hf.TARGET_STATE_INVALID) == (2019, 4001, 4002, 4004, 4032)
    assert (hf.SERVER_READ_XMIT_RDMA, hf.SERVER_READ_XMIT_INLINE, hf.SERVER_READ_XMIT_NONE) == (0, 1, 2)
    assert hf.SERVER_READ_INFO_NAMES == sc.PREP_INFO and hf.SERVER_READ_DONE_NAMES == sc.DONE_INFO
    assert hf.SERVER_READ_NONE == sc.NO_JOB and hf.SERVER_READ_INFO_WORDS == sc.INFO_WORDS
    with open(os.path.join(REPO, "include", "hf3fs_crc.h")) as f:
        header = f.read()
    for name, value in (("RDMA_NO_BUF", 2019), ("CHUNK_METADATA_NOT_FOUND", 4001), ("CHUNK_METADATA_GET_ERROR", 4002),
                        ("CHUNK_NOT_COMMIT", 4004), ("TARGET_STATE_INVALID", 4032)):
        assert re.search(rf"HF3FS_CRC_{name} = {value},", header), name
    for k, name in enumerate(sc.DONE_INFO):
        assert re.search(rf"HF3FS_SERVER_READ_DONE_{name.upper()} = {k},", header), name


def test_scratch_bytes(hf):
    sizes = [hf.server_read_scratch_bytes(n, 1) for n in (0, 1, 257, 70001, 1 << 20, 1 << 30)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and all(s % 4 == 0 for s in sizes)
    assert sizes[-1] >= (1 << 30) * (20 + 17)
    assert hf.server_read_scratch_bytes((1 << 30) + 1, 1) == 0 and hf.server_read_scratch_bytes(1, (1 << 30) + 1) == 0


A = 0x1000  # any non-null address: every call below is refused before a device is touched


@pytest.mark.parametrize("what, kw", [
    ("null jobs", dict(jobs=None)),
    ("null reqs", dict(reqs=None)),
    ("null offsets", dict(req_off=None)),
    ("no request", dict(n_reqs=0)),
    ("null info", dict(info=None)),
    ("too many jobs", dict(n=(1 << 30) + 1)),
    ("too many requests", dict(n_reqs=(1 << 30) + 1)),
])
def test_argument_errors_of_both_calls(hf, what, kw):
    args = dict(jobs=A, n=4, reqs=A, req_off=A, n_reqs=2, info=A)
    args.update(kw)
    with pytest.raises(hf.Hf3fsCrcError) as e:
        hf.server_read_prepare(args["jobs"], args["n"], args["reqs"], args["req_off"], args["n_reqs"], args["info"],
                               SMALL, BIG)
    assert e.value.code == hf.INVALID_ARG, what
    with pytest.raises(hf.Hf3fsCrcError) as e:
        hf.server_read_complete(hf.CRC32C, args["jobs"], args["n"], args["reqs"], args["req_off"], args["n_reqs"],
                                args["info"], 4096)
    assert e.value.code == hf.INVALID_ARG, what


@pytest.mark.parametrize("what, kw", [
    ("type NONE", dict(ctype=0)),
    ("type 3", dict(ctype=3)),
    ("null inline arena", dict(inline=None, inline_cap=1)),
    ("null write list", dict(wr=None, wr_cap=1)),
])
def test_argument_errors_of_complete(hf, what, kw):
    args = dict(ctype=hf.CRC32C, inline=A, inline_cap=0, wr=A, wr_cap=0)
    args.update(kw)
    with pytest.raises(hf.Hf3fsCrcError) as e:
        hf.server_read_complete(args["ctype"], A, 4, A, A, 2, A, 4096, inline=args["inline"],
                                inline_cap=args["inline_cap"], wr=args["wr"], wr_cap=args["wr_cap"])
    assert e.value.code == hf.INVALID_ARG, what
