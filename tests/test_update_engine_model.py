"""tests/engine_cases.py checked on the CPU: the reference's own two engine sequences
(tests/golden/engine_queue_vectors.json), every rung by hand, the shapes the GPU tests name with a
coverage assertion over the built cases, hf3fs_crc_update_engine's argument checks (they come
before any device is touched) and the job record's layout against a compiled C probe of the
header.  The GPU runs are in tests/test_gpu_update_engine.py."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import engine_cases as ec
import update_footprint as fp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built(orc):
    return {name: make() for name, make in ec.all_cases(orc).items()}


def _by_chunk(b):
    by = {}
    for job, e in zip(b.jobs, b.expect):
        by.setdefault(job["c"], []).append((job, e))
    return by


# ---- the reference's own sequences ---------------------------------------------------------------------
def test_golden_sequences_of_the_reference(orc):
    with open(os.path.join(REPO, "tests", "golden", "engine_queue_vectors.json")) as f:
        vectors = json.load(f)["sequences"]
    assert [v["name"] for v in vectors] == ["test_engine_writing_list", "test_engine_truncate_version_tail"]
    for seq in vectors:
        b = ec.golden_queue(orc, seq)
        assert len(b.expect) == len(seq["expect"]) == len(seq["jobs"])
        for i, (want, job, e) in enumerate(zip(seq["expect"], seq["jobs"], b.expect)):
            status, kase, detail, cow, io0, st0, io1, st1 = e
            what = (seq["name"], i)
            assert status == want["status"] and detail == want.get("detail", 0), what
            addr, chain_ver, chunk_ver, w_addr, w_len, w_raw, w_chain, w_ver = st1
            update_ok = job["k"] == "U" and status == ec.OK
            # the IOResult mapping of INTEGRATION.md 3.2: an update answers with the writing version's
            # versions, a refusal or a commit with the committed chunk's
            got_chain, got_ver = (w_chain, w_ver) if update_ok else (chain_ver, chunk_ver)
            if "out_chain_ver" in want:
                assert got_chain == want["out_chain_ver"], what
            if "out_commit_ver" in want:
                assert got_ver == want["out_commit_ver"], what
            if "writing_len" in want:
                assert w_addr != 0 and w_len == want["writing_len"], what
            if "writing_list_empty" in want:
                assert (w_addr == 0) == want["writing_list_empty"], what
            if "out_checksum_finalized" in want:
                assert ec.raw(io1[2]) == want["out_checksum_finalized"] and io1[0] == 0, what
            if "committed_len" in want:
                committed = io1[0] if job["k"] == "C" else io0[0]
                assert committed == want["committed_len"], what
    # (the appended version of the first sequence lies where the committed one does: safe_write)
    b = ec.golden_queue(orc, vectors[0])
    assert [e[3] for e in b.expect] == [0, 0, 0, 0] and b.expect[3][7][3] == b.expect[3][7][0]


# ---- both functions by hand -------------------------------------------------------------------------------
def _one(orc, job, max_len=512, size=100, writing=None, **meta):
    b = ec.build(orc, "hand", 1, max_len, 4, [job], 1, metas={0: meta}, preset={0: size},
                 writing={0: writing} if writing else None)
    return b.expect[0], b


def test_update_and_commit_by_hand(orc):
    W, T, C = ec.W, ec.T, ec.C
    e, b = _one(orc, W(0, 100, 8, 5))
    assert e[:4] == (0, 3, 0, 0) and e[7][3:] == (b.keys[0], 108, e[6][2], 3, 5)             # append: combine, in place
    assert e[7][:3] == e[5][:3] and e[6][0] == 108 and e[4][0] == 100                        # committed unchanged
    e, b = _one(orc, W(0, 99, 8, 0, jcv=7))
    assert e[:4] == (0, 4, 0, 1) and e[7][3] == int(b.jr["dst"][0]) and e[7][6:] == (7, 5)     # cow, version assigned
    assert b.arena1[b.keys[0]:b.keys[0] + 512].tobytes() == b.arena0[b.keys[0]:b.keys[0] + 512].tobytes()
    assert _one(orc, W(0, 99, 8, 5, dst=False))[0][:3] == (3, 0, ec.D_NO_DST)
    assert _one(orc, W(0, 100, 8, 5, dst=False), writing=(4, 3, 5))[0][:3] == (3, 0, ec.D_IN_WRITING)
    assert _one(orc, W(0, 100, 8, 5, engine=False))[0][:3] == (3, 0, ec.D_RECORD)
    assert _one(orc, ec.R(0))[0][:3] == (3, 0, ec.D_RECORD)
    assert _one(orc, W(0, 512, 1, 5))[0][:3] == (3, 0, ec.D_RECORD)
    assert _one(orc, W(0, 100, 8, 5, flavour="corrupt"))[0][0] == 4080
    assert _one(orc, W(0, 100, 8, 9, flavour="corrupt"), chain_ver=9)[0][0] == 4080          # before every rung
    assert _one(orc, W(0, 100, 8, 5, flavour="none"))[0][0] == 0                             # without_checksum
    assert _one(orc, W(0, 100, 8, 5, jcv=2))[0][0] == 4081
    assert _one(orc, W(0, 100, 8, 4))[0][0] == 4008 and _one(orc, W(0, 100, 8, 6))[0][0] == 4007
    assert _one(orc, W(0, 100, 8, 6), chunk_ver=5)[0][0] == 0
    # uint32 versions: chunk_ver + 1 wraps to 0
    e, _ = _one(orc, W(0, 100, 8, 0), chunk_ver=ec.M32)
    assert e[0] == 0 and e[7][7] == 0
    assert _one(orc, W(0, 100, 8, 1), chunk_ver=ec.M32)[0][0] == 4008                        # 1 <= 2^32 - 1
    e, _ = _one(orc, W(0, 0, 8, 0, sync=True), chunk_ver=77)                                 # syncing: any version
    assert e[:4] == (0, 2, 0, 1) and e[7][4] == 8 and e[7][7] == 0
    e, _ = _one(orc, T(0, 40, 5, dst=False))
    assert e[:4] == (0, 4, 0, 0) and e[6][0] == 40                                           # truncate in place
    e, b = _one(orc, C(0, jcv=1), writing=(60, 3, 9), chain_ver=5)                           # no ladder at commit
    w = b.chunks0[0].w
    assert e[:4] == (0, 0, 0, 0) and e[7] == (w.addr, 1, 9, 0, 0, 0, 0, 0) and e[6] == (60, ec.CRC32C, ec.raw(w.fin))
    assert _one(orc, C(0))[0][:3] == (3, 0, ec.D_NO_WRITING)


# ---- the cases ---------------------------------------------------------------------------------------------
def test_cases_reproduce_from_their_seed(orc, built):
    for name, make in ec.all_cases(orc).items():
        a, b = built[name], make()
        assert a.rec.tobytes() == b.rec.tobytes() and a.jr.tobytes() == b.jr.tobytes(), name
        assert a.pay.tobytes() == b.pay.tobytes() and a.arena0.tobytes() == b.arena0.tobytes(), name
        assert a.expect == b.expect and a.arena1.tobytes() == b.arena1.tobytes() and a.info == b.info, name


def test_final_checksums_match_final_bytes(orc, built):
    for name, b in built.items():
        for x, tag in ((b, name), (b.again, name + " (resubmitted)")):
            if x is None:
                continue
            for c, ch in enumerate(x.chunks1):
                assert ch.fin == orc.rs_crc32c(x.arena1[ch.addr:ch.addr + ch.size].tobytes()), (tag, c)
                if ch.w is not None:
                    assert ch.w.fin == orc.rs_crc32c(x.arena1[ch.w.addr:ch.w.addr + ch.w.len].tobytes()), (tag, c)
            assert sum(x.info[1:5]) == x.n and x.info[5] + x.info[6] == x.info[2], tag


def test_guards_and_unused_destinations_keep_their_canary(built):
    for name, b in built.items():
        touched = np.zeros(b.arena0.size, dtype=bool)
        for r in b.regions:
            touched[r:r + b.max_len] = True
        same = b.arena0 == b.arena1
        assert same[~touched].all(), name
        last_update = {}
        for i, (job, e) in enumerate(zip(b.jobs, b.expect)):
            if job["k"] != "C" and e[0] == ec.OK:
                last_update[job["c"]] = i
        for i, (job, e) in enumerate(zip(b.jobs, b.expect)):
            if job["dst"] and not (e[0] == ec.OK and e[3]):  # a dst its job did not use
                d = job["dst"]
                assert same[d:d + b.max_len].all(), (name, job)
            # bytes at or beyond the new length (where no later job of the chunk wrote in place there)
            if job["dst"] and e[0] == ec.OK and e[3] and last_update[job["c"]] == i:
                d, ln = job["dst"], e[6][0]
                assert same[d + ln:d + b.max_len].all(), (name, job)


def test_the_cases_cover_every_path(built):
    """So that the GPU run cannot pass with a path unvisited."""
    seen, cows, flags = set(), set(), set()
    for b in built.values():
        first = set()
        for i, (job, e) in enumerate(zip(b.jobs, b.expect)):
            status, kase, detail, cow = e[:4]
            seen.add((status, detail))
            if status == ec.OK and job["k"] != "C":
                cows.add(cow)
                if cow != int(job["stale_cow"]):
                    flags.add("cow_by_true_state" if cow else "in_place_by_true_state")
            supplied = job["c"] not in first and b.chunks0[job["c"]].w is not None
            if supplied and job["k"] == "C" and status == ec.OK:
                flags.add("commit_first_on_supplied_writing")
            if supplied and job["k"] != "C" and detail == ec.D_IN_WRITING:
                flags.add("update_met_by_supplied_writing")
            first.add(job["c"])
    assert seen >= {(0, 0), (3, 1), (3, 2), (3, 3), (3, 4), (4080, 0), (4081, 0), (4008, 0), (4007, 0), (9002, 0)}, seen
    assert all(d == 0 for s, d in seen if s != 3), seen
    assert cows == {0, 1}
    assert flags == {"cow_by_true_state", "in_place_by_true_state", "commit_first_on_supplied_writing",
                     "update_met_by_supplied_writing"}, flags


def test_the_cases_hold_what_the_gpu_tests_name(built):
    for ml in ec.SIZES:
        s = built[f"singles_{ml}"]
        got = dict(zip(s.tags, ((e[0], e[2]) for e in s.expect)))
        for tag, want in got.items():
            if tag.startswith("u_ok") or tag.startswith("c_ok"):
                assert want == (0, 0), tag
        assert got["u_no_engine_flag"] == got["u_remove"] == got["u_bounds"] == got["u_sync_offset"] == (3, 1)
        assert got["u_4080"] == (4080, 0) and got["u_4081"] == (4081, 0) and got["u_4008"] == (4008, 0)
        assert got["u_4007"] == got["u_truncate_4007"] == (4007, 0)
        assert got["u_no_dst"] == got["u_sync_no_dst"] == (3, 3) and got["c_none"] == (3, 4)
        assert got["u_in_writing"] == got["u_in_writing_append"] == (3, 2)
        assert got["p_record_over_4080"] == (3, 1)
        for tag in ("4081", "4008", "4007", "in_writing", "no_dst"):
            assert got[f"p_4080_over_{tag}"] == (4080, 0), tag
        assert got["p_4081_over_4008"] == (4081, 0) and got["p_4007_over_no_dst"] == (4007, 0)
        assert got["p_no_dst_over_in_writing"] == (3, 3) and got["p_none_write_4008"] == (4008, 0)
        by = dict(zip(s.tags, s.expect))
        assert by["u_ok_assign"][7][7] == 5 and by["u_assign_wraps"][7][7] == 0 and by["u_sync_wraps"][7][7] == 0
        assert by["u_top_version"][7][7] == ec.M32 and by["u_sync_any_version"][7][6:] == (5, 40)
        assert by["u_truncate_in_place"][3] == by["u_extend_in_place"][3] == 0
        assert by["u_sync_len0"][6][0] == 0 and by["u_sync_len0"][3] == 1
        assert by["c_ok_lower_chain"][7][1] == 1                                     # no ladder at commit
        assert s.info[0] == 1 and s.info[7] == 2

        c = _by_chunk(built[f"chains_{ml}"])
        st = lambda k: [e[0] for _, e in c[k]]
        det = lambda k: [e[2] for _, e in c[k]]
        cow = lambda k: [e[3] for _, e in c[k]]
        assert st(0) == [0] * 8 and cow(0) == [0, 0, 1, 0, 0, 0, 1, 0]
        addrs = [e[7][0] for _, e in c[0]]
        assert len(set(addrs)) == 3 and addrs[3] == c[0][2][0]["dst"] and addrs[7] == c[0][6][0]["dst"]
        assert c[0][4][1][7][3] == addrs[3]                                          # an append lands in a former dst
        assert (st(1), det(1)) == ([0, 3, 0], [0, 2, 0]) and c[1][2][1][6][0] == c[1][0][1][6][0]
        assert st(2) == [4080, 0, 0] and c[2][1][1][5][3] == 0                       # nothing was in writing
        assert st(3) == [0, 0, 4081, 0] and det(4) == [4, 0, 0, 4]
        assert st(5) == [0] * 4 and cow(5) == [0] * 4 and c[5][2][0]["stale_cow"]
        assert st(6) == [0] * 4 and cow(6) == [0, 0, 1, 0] and not c[6][2][0]["stale_cow"]
        assert st(7) == [0] and cow(7) == [1]
        assert (st(8), det(8)) == ([3, 0, 0, 4007], [2, 0, 0, 0])
        assert st(9) == [0] * 4 and cow(9) == [1, 0, 0, 0]

        o = built[f"overflow_{ml}"]
        assert o.info[:2] == (5, 12) and o.again.n == 12 and o.again.info[1] == 0
        late = [e for e in o.expect if e[0] == ec.NOT_APPLIED]
        assert any(e[5][3] != 0 for e in late) and any(e[5][3] == 0 for e in late)   # with and without writing state
        assert all(e[4] == e[6] and e[5] == e[7] for e in late)
        for seed in ec.SEEDS:
            r = built[f"random_{ml}_{seed:x}"]
            assert r.n_chunks == 64 and r.n <= 256 and r.info[0] <= 8
            assert {j["k"] for j in r.jobs} == set("WTECR")
            assert {e[0] for e in r.expect} >= {0, 3, 4080, 4081, 4008, 4007}, (ml, seed)
            assert {e[2] for e in r.expect} == {0, 1, 2, 3, 4}, (ml, seed)
            assert r.info[5] and r.info[6] and r.info[3]
        d = built[f"distinct_{ml}"]
        assert d.info[0] == 1 and d.info[3] == 0 and d.info[7] == 0 and d.info[5] and d.info[6]


def test_later_jobs_carry_junk_state(built):
    b = built["chains_512"]
    seen = set()
    for i, job in enumerate(b.jobs):
        junk = tuple(int(b.jr[f][i]) for f in ec.BEFORE_FIELDS) == ec.JUNK_JOB
        assert junk == (job["c"] in seen), i
        seen.add(job["c"])


# ---- the ABI ---------------------------------------------------------------------------------------------------
def test_update_engine_argument_checks_need_no_device(hf):
    L = hf._lib
    f = L.load().hf3fs_crc_update_engine
    jobs = np.zeros(4, dtype=ec.JOB)
    ios = np.zeros(4, dtype=fp.REC)
    p, q = jobs.ctypes.data, ios.ctypes.data
    assert f(hf.CRC32C, q, p, 4, 512, hf.MODE_DELTA, 0, None, None) == hf.INVALID_ARG        # max_rounds 0
    assert f(hf.CRC32C, q, p, 4, 512, hf.MODE_DELTA, 65, None, None) == hf.INVALID_ARG       # max_rounds 65
    assert f(7, q, p, 4, 512, hf.MODE_DELTA, 4, None, None) == hf.INVALID_ARG                # unknown type
    assert f(hf.CRC32C, q, p, 4, 512, 2, 4, None, None) == hf.INVALID_ARG                    # unknown mode
    assert f(hf.CRC32, q, p, 4, 512, hf.MODE_DELTA, 4, None, None) == hf.INVALID_ARG         # type != CRC32C
    assert f(hf.NONE, q, p, 4, 512, hf.MODE_DELTA, 4, None, None) == hf.INVALID_ARG
    assert f(hf.CRC32C, None, p, 4, 512, hf.MODE_DELTA, 4, None, None) == hf.INVALID_ARG     # null ios
    assert f(hf.CRC32C, q, None, 4, 512, hf.MODE_DELTA, 4, None, None) == hf.INVALID_ARG     # null jobs
    assert f(hf.CRC32, None, None, 0, 512, hf.MODE_REFERENCE, 4, None, None) == hf.INVALID_ARG
    with pytest.raises(hf.Hf3fsCrcError):
        hf.update_engine(hf.CRC32C, q, None, 4, 512, 4)
    g = L.update_engine_scratch_bytes
    assert g(4, 512, 0) == 0 and g(4, 512, 65) == 0 and g(4, 512, 4, mode=2) == 0
    assert L.engine_job_dtype() == ec.JOB
    assert L.ENGINE_INFO_WORDS == ec.INFO_WORDS == len(L.ENGINE_INFO_NAMES)
    assert (L.ENGINE_DETAIL_NONE, L.ENGINE_DETAIL_RECORD, L.ENGINE_DETAIL_IN_WRITING, L.ENGINE_DETAIL_NO_DST,
            L.ENGINE_DETAIL_NO_WRITING) == (ec.D_NONE, ec.D_RECORD, ec.D_IN_WRITING, ec.D_NO_DST, ec.D_NO_WRITING)


_FIELDS = [n for n in ec.JOB.names]
_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "hf3fs_crc.h"
#define F(f) printf("%s %zu\n", #f, offsetof(hf3fs_crc_engine_job, f))
int main(void) {
  printf("sizeof %zu align %zu\n", sizeof(hf3fs_crc_engine_job), _Alignof(hf3fs_crc_engine_job));
  """ + " ".join(f"F({n});" for n in _FIELDS) + r"""
  printf("details %d %d %d %d %d info %d %d %d %d %d %d %d %d words %d\n", HF3FS_ENGINE_DETAIL_NONE,
         HF3FS_ENGINE_DETAIL_RECORD, HF3FS_ENGINE_DETAIL_IN_WRITING, HF3FS_ENGINE_DETAIL_NO_DST,
         HF3FS_ENGINE_DETAIL_NO_WRITING, HF3FS_ENGINE_INFO_CHAIN_MAX, HF3FS_ENGINE_INFO_NOT_APPLIED,
         HF3FS_ENGINE_INFO_UPDATES, HF3FS_ENGINE_INFO_COMMITS, HF3FS_ENGINE_INFO_REFUSED, HF3FS_ENGINE_INFO_COW,
         HF3FS_ENGINE_INFO_IN_PLACE, HF3FS_ENGINE_INFO_IN_WRITING, HF3FS_ENGINE_INFO_WORDS);
  return 0;
}
"""


def test_record_layout_matches_a_c_probe_of_the_header(tmp_path):
    """The header compiled as C: size, alignment and every field offset of hf3fs_crc_engine_job equal
    the numpy dtype's, and the new enums have the numbers the model uses."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(_PROBE)
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o",
                           str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    assert lines[0] == f"sizeof {ec.JOB.itemsize} align 8" and ec.JOB.itemsize == 104
    k = len(_FIELDS)
    got = {a: int(b) for a, b in (x.split() for x in lines[1:1 + k])}
    assert got == {name: ec.JOB.fields[name][1] for name in ec.JOB.names}
    assert lines[1 + k] == "details 0 1 2 3 4 info 0 1 2 3 4 5 6 7 words 8"
