"""tests/versioned_cases.py checked on the CPU: every rung of both ladders on hand-worked states,
the shapes the GPU tests name, hf3fs_crc_update_versioned's argument checks (they come before any
device is touched) and the record's layout against a compiled C probe of the header.  The GPU
runs are in tests/test_gpu_update_versioned.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ordered_cases as oc
import versioned_cases as vc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = vc.Meta


def _w(ver, jcv=3, **kw):
    return dict(vc.W(0, 0, 4, ver, jcv, **kw), data=b"abcd", wck=(vc.NONE, 0))


def _update(orc, meta, job, max_len=512):
    m = meta.copy()
    if m.meta_chunk_size is None:
        m.meta_chunk_size = max_len
    chunk = bytearray(max_len)
    before = (m.io(), m.ver())
    status, _ = vc.update_job(orc, chunk, m, job, max_len)
    if status != vc.OK:
        assert (m.io(), m.ver()) == before and chunk == bytearray(max_len)
    return status, m


def _commit(meta, job):
    m = meta.copy()
    before = m.ver()
    status = vc.commit_job(m, job)
    if status != vc.OK:
        assert m.ver() == before
    return status, m


# ---- ChunkReplica::update, rung by rung (ChunkReplica.cc:141-245) -------------------------------------
def test_update_ladder_by_hand(orc):
    clean = M(update_ver=6, commit_ver=4, state=vc.CLEAN)
    assert _update(orc, M(), dict(_w(5), engine=True))[0] == vc.INVALID_ARG
    assert _update(orc, M(), dict(_w(5), off=512))[0] == vc.INVALID_ARG                       # :141
    assert _update(orc, M(), vc.R(0))[0] == vc.INVALID_ARG
    assert _update(orc, M(meta_chunk_size=1024), _w(5))[0] == vc.SIZE_MISMATCH                 # :176
    assert _update(orc, M(state=vc.DIRTY), _w(5))[0] == vc.NOT_CLEAN                           # :181
    assert _update(orc, M(chain_ver=4), _w(5))[0] == vc.CHAIN_VERSION_MISMATCH                 # :186
    assert _update(orc, M(chain_ver=4, state=vc.CLEAN), _w(5))[0] == vc.OK                     # (COMMIT only)
    bad = dict(_w(5), wck=(vc.CRC32C, 1))
    assert _update(orc, M(), bad)[0] == vc.CHECKSUM_MISMATCH                                   # :193
    assert _update(orc, M(), dict(bad, ver=9))[0] == vc.CHECKSUM_MISMATCH                      # before :229
    assert _update(orc, M(chain_ver=4), bad)[0] == vc.CHAIN_VERSION_MISMATCH                   # after :186
    assert _update(orc, clean, _w(4))[0] == vc.COMMITTED_UPDATE                                # :217
    assert _update(orc, clean, _w(3))[0] == vc.COMMITTED_UPDATE
    assert _update(orc, clean, _w(5))[0] == vc.STALE_UPDATE                                    # :221
    assert _update(orc, clean, _w(6))[0] == vc.STALE_UPDATE
    assert _update(orc, clean, _w(8))[0] == vc.MISSING_UPDATE                                  # :225
    s, m = _update(orc, clean, _w(7, jcv=5))
    assert s == vc.OK and m.ver() == (5, 7, 4, 512, vc.CLEAN, 0) and m.size == 4               # :231,242,304
    assert _update(orc, clean, _w(0))[0] == vc.ADVANCE_UPDATE                                  # :234 (7 > 5)
    s, m = _update(orc, M(), _w(0))
    assert s == vc.OK and m.ver() == (3, 5, 4, 512, vc.CLEAN, 0)                               # :233
    # uint32 ChunkVer: update_ver + 1 wraps to 0, commit_ver + 1 too
    assert _update(orc, M(update_ver=vc.M32, commit_ver=vc.M32), _w(0))[0] == vc.OK
    assert _update(orc, M(update_ver=vc.M32, commit_ver=5, state=vc.CLEAN), _w(7))[0] == vc.STALE_UPDATE
    assert _update(orc, M(update_ver=vc.M32, commit_ver=5, state=vc.CLEAN), _w(0))[0] == vc.OK  # 0 > 6 is false
    # syncing (:211-215): DIRTY and recycling are no obstacle, any version is taken
    s, m = _update(orc, M(update_ver=9, commit_ver=2, state=vc.DIRTY, recycle=2), dict(_w(3, jcv=8), sync=True))
    assert s == vc.OK and m.ver() == (8, 3, 2, 512, vc.CLEAN, 0) and m.size == 4
    s, m = _update(orc, M(), dict(_w(0), sync=True))
    assert s == vc.OK and m.commit_ver == vc.M32
    assert _update(orc, M(meta_chunk_size=64), dict(_w(3), sync=True))[0] == vc.SIZE_MISMATCH
    assert _update(orc, M(), dict(_w(3), sync=True, off=1))[0] == vc.INVALID_ARG


# ---- ChunkReplica::commit (:397-467) ---------------------------------------------------------------------
def test_commit_ladder_by_hand():
    up = dict(update_ver=6, commit_ver=4, state=vc.CLEAN)
    assert _commit(M(chain_ver=4, **up), vc.C(0, 6))[0] == vc.CHAIN_VERSION_MISMATCH           # :419
    assert _commit(M(chain_ver=4, **up), vc.C(0, 7))[0] == vc.CHAIN_VERSION_MISMATCH           # before :425
    assert _commit(M(**up), vc.C(0, 7))[0] == vc.CHUNK_VERSION_MISMATCH                        # :425
    assert _commit(M(**up), vc.C(0, 7, force=True))[0] == vc.CHUNK_VERSION_MISMATCH
    assert _commit(M(update_ver=6, commit_ver=4, state=vc.DIRTY), vc.C(0, 6))[0] == vc.NOT_CLEAN  # :435
    s, m = _commit(M(update_ver=6, commit_ver=4, state=vc.DIRTY), vc.C(0, 5, force=True))      # :432
    assert s == vc.OK and m.ver() == (3, 6, 5, None, vc.CLEAN, 0)
    s, m = _commit(M(**up), vc.C(0, 5, jcv=9))                                                 # :440, not :451
    assert s == vc.OK and m.ver() == (3, 6, 5, None, vc.CLEAN, 0)
    s, m = _commit(M(**up), vc.C(0, 6, jcv=9))                                                 # :451-454
    assert s == vc.OK and m.ver() == (9, 6, 6, None, vc.COMMIT, 0)
    assert _commit(M(**up), vc.C(0, 4))[0] == vc.STALE_COMMIT                                  # :442
    assert _commit(M(**up), vc.C(0, 3))[0] == vc.STALE_COMMIT
    s, m = _commit(M(**up), vc.C(0, 3, force=True))                                            # force goes back
    assert s == vc.OK and m.commit_ver == 3 and m.state == vc.CLEAN
    s, m = _commit(M(update_ver=6, commit_ver=4, state=vc.DIRTY), vc.C(0, 6, force=True, jcv=4))
    assert s == vc.OK and m.ver() == (4, 6, 6, None, vc.COMMIT, 0)
    assert _commit(M(recycle=1, **up), vc.C(0, 6))[0] == vc.INVALID_ARG                        # store.remove: host
    assert _commit(M(**up), vc.C(0, 6, engine=True))[0] == vc.INVALID_ARG


# ---- the cases ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built(orc):
    return {name: make() for name, make in vc.all_cases(orc).items()}


def test_cases_reproduce_from_their_seed(orc, built):
    for name, make in vc.all_cases(orc).items():
        a, b = built[name], make()
        assert a.rec.tobytes() == b.rec.tobytes() and a.ver.tobytes() == b.ver.tobytes(), name
        assert a.pay.tobytes() == b.pay.tobytes() and a.arena0.tobytes() == b.arena0.tobytes(), name
        assert a.expect == b.expect and a.arena1.tobytes() == b.arena1.tobytes() and a.info == b.info, name


def test_final_checksums_match_final_bytes(orc, built):
    for name, b in built.items():
        for x, tag in ((b, name), (b.again, name + " (resubmitted)")):
            if x is None:
                continue
            for c, m in enumerate(x.metas):
                if m.size and m.ck[0] != vc.NONE:
                    base = b.bases[c]
                    data = x.arena1[base:base + m.size].tobytes()
                    assert tuple(m.ck) == tuple(orc.create(m.ck[0], data)), (tag, c)
            assert sum(x.info[1:5]) == x.n, tag


def test_the_cases_hold_what_the_gpu_tests_name(built):
    for ml in vc.SIZES:
        s = built[f"singles_{ml}"]
        got = dict(zip(s.tags, (e[0] for e in s.expect)))
        upd = {got[t] for t in got if t[0] in "up"}
        com = {got[t] for t in got if t[0] == "c"}
        assert upd == set(vc.UPDATE_CODES) and com == set(vc.COMMIT_CODES), ml
        assert s.info[0] == 1 and s.arena1.tobytes() != s.arena0.tobytes()
        assert got["p_4015_over_4005"] == 4015 and got["p_4005_over_4081"] == 4005
        assert got["p_4081_over_payload"] == 4081
        for code in (4008, 4006, 4007, 4012):
            assert got[f"p_payload_over_{code}"] == 4080 and got[f"p_good_payload_{code}"] == code
        i = s.tags.index("u_sync_dirty_recycling")
        assert s.expect[i][0] == vc.OK and s.expect[i][3][4:] == (vc.DIRTY, 1)
        assert s.expect[i][5] == (5, 40, 39, ml, vc.CLEAN, 0)
        p = built[f"pairs_{ml}"]
        by = {}
        for job, e in zip(p.jobs, p.expect):
            by.setdefault(job["c"], []).append(e)
        assert [e[0] for e in by[0]] == [4080, 4007] and by[0][1][4] == by[0][0][2]            # untouched
        assert [e[0] for e in by[1]] == [0, 4006] and [e[0] for e in by[2]] == [0, 0, 4008]
        assert [e[0] for e in by[3]] == [0] * 8 and by[3][-1][5][:3] == (3, 8, 8) and by[3][-1][5][4] == vc.COMMIT
        assert [e[0] for e in by[4]] == [0, 4012, 0, 0, 0, 0, 0] and by[4][2][5][1:3] == (5, 5)
        assert [e[0] for e in by[5]] == [4005, 0, 0, 4023, 0, 4081, 0]
        assert [e[5][4] for e in by[5]][:5] == [vc.DIRTY, vc.CLEAN, vc.CLEAN, vc.CLEAN, vc.COMMIT]
        assert by[5][4][5][0] == 8                                                              # chain_ver from the job
        assert [e[0] for e in by[6]] == [4005, 0, 0, 0, 4008] and by[6][1][5] == (3, 20, 19, ml, vc.CLEAN, 0)
        assert [e[0] for e in by[7]] == [0, 3, 3, 3, 0, 0]
        o = built[f"overflow_{ml}"]
        assert o.info[:2] == (5, 12) and o.again.n == 12 and o.again.info[1] == 0
        assert all(e[0] == vc.OK for e in o.again.expect)
        for seed in vc.SEEDS:
            r = built[f"random_{ml}_{seed:x}"]
            codes = {e[0] for e in r.expect}
            assert r.n_chunks == 64 and r.n <= 256 and r.info[0] <= 8
            assert codes >= (set(vc.UPDATE_CODES) | set(vc.COMMIT_CODES)), (ml, seed, sorted(codes))
            assert {j["k"] for j in r.jobs} == set("WTECR")
    assert built["one_chunk"].info[0] == 64 and built["one_chunk"].n == 64
    a, b = built["capture_a"], built["capture_b"]
    assert a.n == b.n and a.bases == b.bases and a.pay.size == b.pay.size
    assert [j["c"] for j in a.jobs] != [j["c"] for j in b.jobs] and a.info != b.info


def test_later_jobs_carry_junk_state(built):
    b = built["pairs_512"]
    seen = set()
    for i, job in enumerate(b.jobs):
        junk = tuple(int(b.ver[f][i]) for f in vc.STATE_FIELDS) == vc.JUNK_VER
        assert junk == (job["c"] in seen), i
        seen.add(job["c"])


def test_admit_all_records_follow_the_chains(orc):
    b = oc.chains(orc, 512)
    ver, want, tail = vc.admit_all(b)
    assert tail[0] == b.n and int(want["out_update_ver"].max()) == 7 + 12
    first = {}
    for i in range(b.n):
        c = int(b.rec["chunk"][i])
        assert int(ver["io_ver"][i]) == int(want["update_ver"][i]) + 1
        if c in first:
            assert int(want["update_ver"][i]) == int(want["out_update_ver"][first[c]])
        first[c] = i


# ---- the ABI ---------------------------------------------------------------------------------------------------
def test_update_versioned_argument_checks_need_no_device(hf):
    f = hf._lib.load().hf3fs_crc_update_versioned
    ver = np.zeros(4, dtype=vc.VER)
    p = ver.ctypes.data
    for v in (None, p):  # with and without version records: update_ordered's checks
        assert f(hf.CRC32C, None, v, 4, 512, hf.MODE_DELTA, 0, None, None) == hf.INVALID_ARG
        assert f(hf.CRC32C, None, v, 4, 512, hf.MODE_DELTA, 65, None, None) == hf.INVALID_ARG
        assert f(7, None, v, 4, 512, hf.MODE_DELTA, 4, None, None) == hf.INVALID_ARG
        assert f(hf.CRC32C, None, v, 4, 512, 2, 4, None, None) == hf.INVALID_ARG
        assert f(hf.CRC32C, None, v, 4, 512, hf.MODE_DELTA, 4, None, None) == hf.INVALID_ARG  # null ios
        assert f(hf.CRC32C, None, v, 0, 512, hf.MODE_REFERENCE, 4, None, None) == hf.OK
    with pytest.raises(hf.Hf3fsCrcError):
        hf.update_versioned(hf.CRC32C, None, p, 4, 512, 0)
    assert hf.update_versioned(hf.CRC32C, None, p, 0, 512, 64) == hf.OK
    L = hf._lib
    assert L.update_ver_dtype() == vc.VER and hf.UPDATE_COMMIT == vc.COMMIT_JOB == 16
    assert (L.CHUNK_NOT_CLEAN, L.CHUNK_STALE_UPDATE, L.CHUNK_MISSING_UPDATE, L.CHUNK_COMMITTED_UPDATE,
            L.CHUNK_ADVANCE_UPDATE, L.CHUNK_SIZE_MISMATCH, L.CHUNK_STALE_COMMIT, L.CHAIN_VERSION_MISMATCH,
            L.CHUNK_VERSION_MISMATCH) == (4005, 4006, 4007, 4008, 4012, 4015, 4023, 4081, 4082)
    assert L.VER_INFO_WORDS == vc.INFO_WORDS == len(L.VER_INFO_NAMES)


_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "hf3fs_crc.h"
#define F(f) printf("%s %zu\n", #f, offsetof(hf3fs_crc_update_ver, f))
int main(void) {
  printf("sizeof %zu\n", sizeof(hf3fs_crc_update_ver));
  F(io_ver); F(job_chain_ver); F(chain_ver); F(update_ver); F(commit_ver); F(meta_chunk_size); F(chunk_state);
  F(recycle_state); F(is_force); F(reserved0); F(out_chain_ver); F(out_update_ver); F(out_commit_ver);
  F(out_chunk_state); F(out_recycle_state); F(reserved1); F(reserved2);
  printf("commit %d words %d codes %d %d %d %d %d %d %d %d %d\n", HF3FS_UPDATE_COMMIT, HF3FS_VER_INFO_WORDS,
         HF3FS_CRC_CHUNK_NOT_CLEAN, HF3FS_CRC_CHUNK_STALE_UPDATE, HF3FS_CRC_CHUNK_MISSING_UPDATE,
         HF3FS_CRC_CHUNK_COMMITTED_UPDATE, HF3FS_CRC_CHUNK_ADVANCE_UPDATE, HF3FS_CRC_CHUNK_SIZE_MISMATCH,
         HF3FS_CRC_CHUNK_STALE_COMMIT, HF3FS_CRC_CHAIN_VERSION_MISMATCH, HF3FS_CRC_CHUNK_VERSION_MISMATCH);
  return 0;
}
"""


def test_record_layout_matches_a_c_probe_of_the_header(tmp_path):
    """The header compiled as C: size and every field offset of hf3fs_crc_update_ver equal the numpy
    dtype's, and the new constants have the reference's numbers."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(_PROBE)
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o",
                           str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    assert lines[0] == "sizeof 48"
    got = {a: int(b) for a, b in (x.split() for x in lines[1:18])}
    assert got == {name: vc.VER.fields[name][1] for name in vc.VER.names}
    assert lines[18] == "commit 16 words 8 codes 4005 4006 4007 4008 4012 4015 4023 4081 4082"
