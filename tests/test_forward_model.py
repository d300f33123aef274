"""The model of hf3fs_crc_forward_prepare / _complete (tests/forward_cases.py) against jobs worked by
hand, at least one per branch of StorageOperator.cc:401-485, ReliableForwarding.cc:113-278 and
BatchReadJob.cc:43-54, the expected fields written out with the reference line beside them; the
record layout (header against ctypes against the model's dtype), the binding and every argument
error.  No GPU: the CRC values come from the CPU oracle."""
import ctypes
import re

import numpy as np
import pytest

import forward_cases as fc

CHUNK = bytes(range(256)) * 2          # the stored chunk at 0x20000, 512 bytes
PAYLOAD = b"the bytes of one forwarded write" * 3 + b"!!!!"   # at 0x10000, 100 bytes
MEM = {0x20000: CHUNK, 0x10000: PAYLOAD}


def read(addr, n):
    for base, data in MEM.items():
        if base <= addr and addr + n <= base + len(data):
            return data[addr - base:addr - base + n]
    raise AssertionError("read outside the case's buffers: %#x + %d" % (addr, n))


def no_read(addr, n):
    raise AssertionError("this job reads no byte")


def prep(orc, j, reader=no_read, max_len=4096, max_inline=0, ctype=fc.CRC32C):
    after, info = fc.model_prepare(j, ctype, max_len, max_inline, orc, reader)
    return after[0], dict(zip(fc.PREP_INFO, info.tolist()))


def done(orc, j, reader=no_read, max_len=4096, ctype=fc.CRC32C):
    after, commits, info = fc.model_complete(j, ctype, max_len, orc, reader)
    return after[0], commits.tolist(), dict(zip(fc.DONE_INFO, info.tolist()))


def fields(rec, *names):
    return tuple(int(rec[k]) for k in names)


def syncing_job(orc, **kw):
    """A 100-byte write into a 512-byte chunk whose successor is SYNCING: the whole chunk goes out."""
    ck = orc.create(fc.CRC32C, CHUNK)
    base = dict(successor_syncing=1, chunk=0x20000, chunk_len=512, chunk_checksum_type=ck[0], chunk_checksum=ck[1],
                chunk_update_ver=9, chunk_commit_chain_ver=3, req_flags=fc.REQ_INLINE)
    return fc.plain_job(**dict(base, **kw))


# ---- A. the local result --------------------------------------------------------------------------
def test_a_success_sends_the_request_as_it_is(orc):
    r, info = prep(orc, fc.plain_job())
    assert fields(r, "action", "status", "res_length", "res_update_ver", "res_commit_ver") == (fc.SEND, 0, 100, 5, 4)
    assert fields(r, "commit_ver", "commit_chain_ver", "is_syncing") == (5, 0, 0)            # :441
    assert fields(r, "out_update_type", "out_offset", "out_length", "out_data") == (fc.WRITE, 0, 100, 0x10000)
    assert fields(r, "out_checksum_type", "out_checksum", "out_update_ver") == (fc.CRC32C, 0x11111111, 5)
    assert fields(r, "out_flags", "out_commit_chain_ver", "computed") == (0, 0, 0)
    assert r["fwd_status"] == -2                     # a sent job's response is the host's to write
    assert info == dict(dict.fromkeys(fc.PREP_INFO, 0), sent=1)


def test_a_unset_request_version_takes_the_result_s(orc):
    r, _ = prep(orc, fc.plain_job(req_update_ver=0, upd_update_ver=8))                        # :404-405
    assert fields(r, "action", "out_update_ver", "res_update_ver", "commit_ver") == (fc.SEND, 8, 8, 8)
    assert r["req_update_ver"] == 0                  # the input is not written


def test_a_version_mismatch_is_4082(orc):
    r, info = prep(orc, fc.plain_job(req_update_ver=6))                                       # :406-409
    assert fields(r, "action", "status", "res_length", "res_update_ver", "res_commit_ver") == (fc.RETURN, 4082, 0, 0, 0)
    assert fields(r, "fwd_status", "out_length", "commit_ver") == (0, 0, 0) and info["returned"] == 1


@pytest.mark.parametrize("code", [fc.MISSING_UPDATE, fc.ADVANCE_UPDATE, 4010])
def test_a_missing_advance_and_other_errors_return_the_local_result(orc, code):
    r, _ = prep(orc, fc.plain_job(upd_status=code, upd_length=33))                            # :411-414,427-434
    assert fields(r, "action", "status", "res_length", "res_update_ver", "res_commit_ver") == (fc.RETURN, code, 33, 5, 4)


def test_a_committed_update_returns_success(orc):
    r, _ = prep(orc, fc.plain_job(upd_status=fc.COMMITTED_UPDATE, upd_length=0, upd_update_ver=9, upd_commit_ver=9))
    assert fields(r, "action", "status", "res_length", "res_update_ver", "res_commit_ver") == (fc.RETURN, 0, 100, 5, 5)  # :417-419


def test_a_stale_update_goes_on_with_the_request_s_length_and_version(orc):
    r, _ = prep(orc, fc.plain_job(upd_status=fc.STALE_UPDATE, upd_length=0, upd_update_ver=9, upd_commit_ver=9))
    assert fields(r, "action", "status", "res_length", "res_update_ver", "res_commit_ver") == (fc.SEND, 0, 100, 5, 9)  # :424-425
    assert fields(r, "commit_ver", "out_update_ver") == (5, 5)


def test_unknown_update_type_is_a_bad_record(orc):
    for t in (0, fc.COMMIT_TYPE, 3):
        r, info = prep(orc, fc.plain_job(update_type=t))
        assert fields(r, "action", "status") == (fc.RETURN, 3) and info["bad_records"] == 1


# ---- B. forward / doForward -----------------------------------------------------------------------
def test_b_no_successor(orc):
    r, info = prep(orc, fc.plain_job(has_successor=0, successor_syncing=1))                   # :113-117
    assert fields(r, "action", "status", "commit_ver", "commit_chain_ver", "is_syncing") == (fc.NO_SUCCESSOR, 0, 5, 7, 0)
    assert fields(r, *fc.RESPONSE) == (0, 4033, 0, 0, 0, 0) and info["no_successor"] == 1
    assert fields(r, "out_length", "out_data", "out_flags") == (0, 0, 0)


def test_b_syncing_read_replaces_the_write_by_the_whole_chunk(orc):
    ck = orc.create(fc.CRC32C, CHUNK)
    r, info = prep(orc, syncing_job(orc), read)                 # length 100 != chunk_size 4096 (:158-159)
    assert fields(r, "action", "status", "is_syncing", "computed") == (fc.SEND, 0, 1, ck[1])
    assert fields(r, "out_update_type", "out_offset", "out_length", "out_data") == (fc.WRITE, 0, 512, 0x20000)   # :203-207
    assert fields(r, "out_checksum_type", "out_checksum", "out_update_ver") == (ck[0], ck[1], 9)                # :199,206
    # SYNCING and the chain version of :153-156; INLINE cleared (:193-196), 512 > max_inline 0
    assert fields(r, "out_flags", "out_commit_chain_ver") == (fc.OUT_SYNCING | fc.OUT_COMMIT_CHAIN_VER, 7)
    assert fields(r, "res_update_ver", "commit_ver") == (5, 5)
    assert info == dict(dict.fromkeys(fc.PREP_INFO, 0), sent=1, sync_hashed=1)


def test_b_syncing_read_of_a_syncing_request_takes_the_chunk_s_commit_chain_version(orc):
    j = syncing_job(orc, req_flags=fc.REQ_SYNCING, length=4096, chunk_size=4096)   # req.options.isSyncing (:159)
    r, _ = prep(orc, j, read, max_inline=512)
    assert fields(r, "action", "out_length", "out_commit_chain_ver") == (fc.SEND, 512, 3)    # :200-202
    assert r["out_flags"] == fc.OUT_SYNCING | fc.OUT_COMMIT_CHAIN_VER | fc.OUT_INLINE         # 512 <= 512 (:209-212)
    r, _ = prep(orc, j, read, max_inline=511)
    assert r["out_flags"] == fc.OUT_SYNCING | fc.OUT_COMMIT_CHAIN_VER


def test_b_full_chunk_write_is_not_read_but_takes_the_chunk_s_version(orc):
    j = syncing_job(orc, length=4096, chunk_size=4096)           # neither clause of :159 holds
    r, info = prep(orc, j)                                       # (no byte read)
    assert fields(r, "action", "out_length", "out_data", "out_update_ver", "computed") == (fc.SEND, 4096, 0x10000, 9, 0)  # :221
    assert r["out_flags"] == fc.OUT_SYNCING | fc.OUT_INLINE | fc.OUT_COMMIT_CHAIN_VER and r["out_commit_chain_ver"] == 7
    assert info["sync_hashed"] == 0
    # an engine job or a REMOVE does not query the chunk (:215): the request's version stays
    for change in (dict(engine_job=1), dict(update_type=fc.REMOVE, length=0, chunk_size=4096)):
        r, _ = prep(orc, syncing_job(orc, **dict(dict(length=4096, chunk_size=4096, chunk_status_in=4010), **change)))
        assert fields(r, "action", "out_update_ver", "is_syncing") == (fc.SEND, 5, 1), change


def test_b_failed_read_or_query_is_returned(orc):
    r, _ = prep(orc, syncing_job(orc, chunk_status_in=4010))                                  # :190
    assert fields(r, "action", "status", "computed", "is_syncing") == (fc.RETURN, 4010, 0, 0)
    r, _ = prep(orc, syncing_job(orc, length=4096, chunk_size=4096, chunk_status_in=7007))    # :217-220
    assert fields(r, "action", "status") == (fc.RETURN, 7007)


def test_b_flipped_chunk_bit_is_4080(orc):
    good = orc.create(fc.CRC32C, CHUNK)
    r, info = prep(orc, syncing_job(orc, chunk_checksum=good[1] ^ 0x100), read)               # BatchReadJob.cc:45-52
    assert fields(r, "action", "status", "computed", "out_length") == (fc.RETURN, 4080, good[1], 0)
    assert fields(r, "res_length", "res_update_ver") == (100, 5)
    assert info == dict(dict.fromkeys(fc.PREP_INFO, 0), returned=1, sync_hashed=1, sync_mismatched=1)


def test_b_none_typed_chunk_reads_nothing(orc):
    r, info = prep(orc, syncing_job(orc, chunk_checksum_type=fc.NONE, chunk_checksum=0))      # Common.h:150
    assert fields(r, "action", "computed", "out_checksum_type", "out_checksum", "out_length") == (fc.SEND, 0, 0, 0, 512)
    assert info["sync_hashed"] == 0
    r, info = prep(orc, syncing_job(orc, chunk_checksum_type=fc.NONE, chunk_checksum=1))
    assert fields(r, "action", "status") == (fc.RETURN, 4080) and info["sync_mismatched"] == 1


def test_b_empty_typed_chunk(orc):
    empty = orc.create(fc.CRC32C, b"")
    r, info = prep(orc, syncing_job(orc, chunk_len=0, chunk_checksum=empty[1], chunk=0))
    assert fields(r, "action", "computed", "out_length") == (fc.SEND, empty[1], 0) and info["sync_hashed"] == 0


def test_b_chunks_the_call_cannot_hash_are_bad_records(orc):
    for change in (dict(chunk_checksum_type=fc.CRC32), dict(chunk_len=4097), dict(chunk=0)):
        r, info = prep(orc, syncing_job(orc, **change))
        assert fields(r, "action", "status", "computed") == (fc.RETURN, 3, 0), change
        assert info["bad_records"] == 1 and info["sync_hashed"] == 0


# ---- C and D. the response and the commit decision --------------------------------------------------
def sent(orc, j, reader=no_read, **resp):
    after, _ = fc.model_prepare(j, fc.CRC32C, 4096, 0, orc, reader)
    assert after["action"][0] == fc.SEND
    fc.answer(after, **resp)
    return after


def test_c_agreeing_answer_commits(orc):
    r, commits, info = done(orc, sent(orc, fc.plain_job(), fwd_commit_chain_ver=6))
    assert fields(r, "final_action", "final_status", "commit_ver", "commit_chain_ver") == (fc.COMMIT, 0, 5, 6)  # :121-123
    assert fields(r, "fwd_update_ver", "buffer_corrupted", "buffer_computed") == (0, 0, 0)
    assert commits == [0] and info == dict(dict.fromkeys(fc.DONE_INFO, 0), commits=1)


def test_c_syncing_answer_carries_the_request_s_version(orc):
    j = sent(orc, syncing_job(orc, req_update_ver=0, upd_update_ver=5), read)
    r, commits, _ = done(orc, j)
    assert fields(r, "final_action", "fwd_update_ver") == (fc.COMMIT, 5) and commits == [0]   # :251 after :404-405


def test_c_higher_remote_chain_version_is_4081(orc):
    r, commits, info = done(orc, sent(orc, fc.plain_job(), fwd_commit_chain_ver=8))           # :238-245
    assert fields(r, "final_action", "final_status", "commit_ver", "commit_chain_ver") == (fc.RETURN, 4081, 5, 0)
    assert commits == [] and info == dict(dict.fromkeys(fc.DONE_INFO, 0), returned=1, e4081=1)


def test_c_4080_answer_rehashes_the_outgoing_buffer(orc):
    good = orc.create(fc.CRC32C, PAYLOAD)
    j = sent(orc, fc.plain_job(req_checksum=good[1]), fwd_status=4080)
    r, commits, info = done(orc, j, read)                                                     # :263-268
    assert fields(r, "final_action", "final_status", "buffer_corrupted", "buffer_computed") == (fc.RETURN, 4080, 0, good[1])
    assert commits == [] and info == dict(dict.fromkeys(fc.DONE_INFO, 0), returned=1, rehashed=1)
    j = sent(orc, fc.plain_job(req_checksum=good[1] ^ 2), fwd_status=4080)
    r, _, info = done(orc, j, read)                                                           # :269-274
    assert fields(r, "final_status", "buffer_corrupted", "buffer_computed") == (4080, 1, good[1])
    assert info["corrupted"] == 1 and info["rehashed"] == 1
    # the whole chunk after a syncing read is the buffer that went out
    j = sent(orc, syncing_job(orc), read, fwd_status=4080)
    r, _, info = done(orc, j, read)
    assert fields(r, "buffer_corrupted", "buffer_computed") == (0, orc.create(fc.CRC32C, CHUNK)[1])


def test_c_4080_answer_with_none_or_unhashable_buffers(orc):
    r, _, info = done(orc, sent(orc, fc.plain_job(req_checksum_type=fc.NONE, req_checksum=0), fwd_status=4080))
    assert fields(r, "final_status", "buffer_corrupted") == (4080, 0) and info["rehashed"] == 0
    r, _, info = done(orc, sent(orc, fc.plain_job(req_checksum_type=fc.NONE, req_checksum=9), fwd_status=4080))
    assert fields(r, "final_status", "buffer_corrupted") == (4080, 1) and info["corrupted"] == 1
    for change in (dict(req_checksum_type=fc.CRC32), dict(length=4097), dict(payload=0)):
        r, _, info = done(orc, sent(orc, fc.plain_job(**change), fwd_status=4080))
        assert fields(r, "final_status", "buffer_corrupted", "buffer_computed") == (4080, 0, 0), change
        assert info["unhashable"] == 1 and info["rehashed"] == 0


def test_d_commit_version_mismatch_is_4082(orc):
    r, commits, info = done(orc, sent(orc, fc.plain_job(), fwd_commit_ver=6))                 # :446-453
    assert fields(r, "final_action", "final_status", "commit_ver") == (fc.RETURN, 4082, 6)
    assert commits == [] and info["e4082"] == 1


def test_d_checksum_disagreement_is_7015(orc):
    for change in (dict(fwd_checksum=0x22222223), dict(fwd_checksum_type=fc.CRC32), dict(fwd_checksum_type=fc.NONE)):
        r, commits, info = done(orc, sent(orc, fc.plain_job(), **change))                     # :475-482
        assert fields(r, "final_action", "final_status") == (fc.RETURN, 7015), change
        assert commits == [] and info["e7015"] == 1


def test_d_remove_exemptions(orc):
    rm = dict(update_type=fc.REMOVE, length=0, payload=0)
    # either type NONE (:465-466)
    assert done(orc, sent(orc, fc.plain_job(**rm), fwd_checksum_type=fc.NONE, fwd_checksum=0))[1] == [0]
    assert done(orc, sent(orc, fc.plain_job(upd_checksum_type=fc.NONE, **rm), fwd_checksum_type=fc.CRC32C))[1] == [0]
    # a syncing successor
    assert done(orc, sent(orc, fc.plain_job(successor_syncing=1, **rm), fwd_checksum=1))[1] == [0]
    # otherwise a remove is compared like a write
    r, commits, _ = done(orc, sent(orc, fc.plain_job(**rm), fwd_checksum=1))
    assert fields(r, "final_status") == (7015,) and commits == []
    # and the exemption is the remove's alone
    assert done(orc, sent(orc, fc.plain_job(successor_syncing=1, length=4096), fwd_checksum=1))[1] == []


def test_d_forward_errors(orc):
    r, commits, info = done(orc, sent(orc, fc.plain_job(), fwd_status=4010))                  # :483-485
    assert fields(r, "final_action", "final_status", "commit_ver") == (fc.RETURN, 4010, 5) and commits == []
    assert info == dict(dict.fromkeys(fc.DONE_INFO, 0), returned=1)
    # 4033, from the successor or preset for a target without one, commits
    assert done(orc, sent(orc, fc.plain_job(), fwd_status=4033))[1] == [0]
    after, _ = fc.model_prepare(fc.plain_job(has_successor=0), fc.CRC32C, 4096, 0, orc)
    r, commits, _ = done(orc, after)
    assert fields(r, "final_action", "final_status", "commit_ver", "commit_chain_ver") == (fc.COMMIT, 0, 5, 7)
    assert commits == [0]


def test_d_returned_jobs_keep_their_status_and_complete_twice_is_the_same(orc):
    after, _ = fc.model_prepare(fc.plain_job(req_update_ver=6), fc.CRC32C, 4096, 0, orc)
    r, commits, info = done(orc, after)
    assert fields(r, "final_action", "final_status", "commit_ver") == (fc.RETURN, 4082, 0)
    assert commits == [] and info == dict(dict.fromkeys(fc.DONE_INFO, 0), returned=1)
    j = sent(orc, fc.plain_job(), fwd_commit_ver=6)
    once, _, _ = fc.model_complete(j, fc.CRC32C, 4096, orc)
    twice, _, _ = fc.model_complete(once, fc.CRC32C, 4096, orc)       # complete reads nothing it wrote
    assert once.tobytes() == twice.tobytes()
    fc.answer(once, fwd_commit_ver=5)                                  # the resent job's new answer
    assert fc.model_complete(once, fc.CRC32C, 4096, orc)[1].tolist() == [0]


def test_commit_list_is_ascending(orc):
    rng = np.random.default_rng(5)
    j = np.concatenate([fc.plain_job() for _ in range(40)])
    after, _ = fc.model_prepare(j, fc.CRC32C, 4096, 0, orc)
    for i in range(40):
        fc.answer(after, i, fwd_status=0 if rng.random() < .4 else 4010)
    _, commits, info = fc.model_complete(after, fc.CRC32C, 4096, orc)
    want = [i for i in range(40) if after["fwd_status"][i] == 0]
    assert commits.tolist() == want and info[0] == len(want) and info[1] == 40 - len(want)


# ---- the binding ------------------------------------------------------------------------------------
def header_offsets(text):
    """The offsets the header's field comments state, checked against its own static_asserts by
    every build; here they tie the comments to the ctypes mirror."""
    body = text[text.index("typedef struct hf3fs_crc_forward_job {"):text.index("} hf3fs_crc_forward_job;")]
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(\w+)(?:\[\d+\])?;\s*/\*\s*(\d+)\b", body)}


def test_record_layout(hf):
    text = open(hf._lib.HEADER).read()
    want = header_offsets(text)
    assert len(want) == len(fc.JOB.names) == len(hf.ForwardJob._fields_) and want["reserved1"] == 186
    assert ctypes.sizeof(hf.ForwardJob) == fc.JOB.itemsize == hf.forward_job_dtype().itemsize == 192
    assert 192 % 8 == 0 and "sizeof(hf3fs_crc_forward_job) == 192" in text
    assert {n: getattr(hf.ForwardJob, n).offset for n, _ in hf.ForwardJob._fields_} == want
    assert {n: fc.JOB.fields[n][1] for n in fc.JOB.names} == want
    dt = hf.forward_job_dtype()
    assert {n: dt.fields[n][1] for n in dt.names} == want
    assert [getattr(hf.ForwardJob, n).size for n, _ in hf.ForwardJob._fields_] == [fc.JOB[n].itemsize for n in fc.JOB.names]
    for m in re.finditer(r"offsetof\(hf3fs_crc_forward_job, (\w+)\) == (\d+)", text):   # the static_asserts
        assert want[m.group(1)] == int(m.group(2)), m.group(0)


def test_constants_match_the_header(hf):
    text = open(hf._lib.HEADER).read()
    L = hf._lib
    for name, mine, theirs in (("HF3FS_UPDATE_REMOVE", fc.REMOVE, hf.UPDATE_REMOVE),
                               ("HF3FS_CRC_NO_SUCCESSOR_TARGET", fc.NO_SUCCESSOR_TARGET, hf.NO_SUCCESSOR_TARGET),
                               ("HF3FS_FORWARD_REQ_SYNCING", fc.REQ_SYNCING, hf.FORWARD_REQ_SYNCING),
                               ("HF3FS_FORWARD_REQ_INLINE", fc.REQ_INLINE, hf.FORWARD_REQ_INLINE),
                               ("HF3FS_FORWARD_OUT_SYNCING", fc.OUT_SYNCING, hf.FORWARD_OUT_SYNCING),
                               ("HF3FS_FORWARD_OUT_INLINE", fc.OUT_INLINE, hf.FORWARD_OUT_INLINE),
                               ("HF3FS_FORWARD_OUT_COMMIT_CHAIN_VER", fc.OUT_COMMIT_CHAIN_VER,
                                hf.FORWARD_OUT_COMMIT_CHAIN_VER),
                               ("HF3FS_FORWARD_RETURN", fc.RETURN, hf.FORWARD_RETURN),
                               ("HF3FS_FORWARD_SEND", fc.SEND, hf.FORWARD_SEND),
                               ("HF3FS_FORWARD_NO_SUCCESSOR", fc.NO_SUCCESSOR, hf.FORWARD_NO_SUCCESSOR),
                               ("HF3FS_FORWARD_COMMIT", fc.COMMIT, hf.FORWARD_COMMIT),
                               ("HF3FS_FORWARD_INFO_WORDS", fc.INFO_WORDS, hf.FORWARD_INFO_WORDS)):
        assert re.search(rf"\b{name} = {mine}\b", text) and mine == theirs, name
    for w, name in enumerate(fc.PREP_INFO[:6]):
        assert re.search(rf"\bHF3FS_FORWARD_INFO_{name.upper()} = {w}\b", text), name
    for w, name in enumerate(fc.DONE_INFO):
        assert re.search(rf"\bHF3FS_FORWARD_DONE_{name.upper().lstrip('E')} = {w}\b", text), name
    assert hf.FORWARD_INFO_NAMES == fc.PREP_INFO and hf.FORWARD_DONE_NAMES == fc.DONE_INFO
    for name in ("hf3fs_crc_forward_prepare", "hf3fs_crc_forward_complete", "hf3fs_crc_forward_scratch_bytes"):
        assert name in L.SIGNATURES and hasattr(L.load(), name)


def test_errors_decided_without_a_device(hf):
    """Every argument error is returned before any device is touched: none of these calls needs one."""
    L = hf._lib
    p = 0x1000  # never dereferenced: the call fails first
    cases = [dict(ctype=fc.NONE), dict(ctype=3),     # the type
             dict(jobs=None),                        # null d_jobs with n > 0
             dict(info=None),                        # null d_info
             dict(n=(1 << 30) + 1)]
    for change in cases:
        for call, extra in ((L.forward_prepare, dict(max_inline_bytes=0)), (L.forward_complete, dict(commit_idx=p))):
            kw = dict(dict(ctype=fc.CRC32C, jobs=p, n=4, info=p, max_len=4096, **extra), **change)
            with pytest.raises(hf.Hf3fsCrcError) as e:
                call(**kw)
            assert e.value.code == hf.INVALID_ARG, (call.__name__, change)


def test_scratch_bytes(hf):
    L = hf._lib
    assert L.forward_scratch_bytes((1 << 30) + 1) == 0
    sizes = [L.forward_scratch_bytes(n) for n in (0, 1, 64, 1000, 1 << 16, 1 << 20, 1 << 24, 1 << 30)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    assert sizes[5] >= (1 << 20) * 21 and sizes[-1] >= (1 << 30) * 21   # addr, len, value and the commit flag per job
