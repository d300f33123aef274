"""ASan + UBSan on the decisions of hf3fs_crc_forward_prepare / _complete (3fs_amd/csrc/forward_plan.h),
on the pattern of tests/test_client_read_sanitized.py: tests/cpp/fuzz_forward.cpp is a stand-alone
program that includes the header the kernels include and runs random jobs through it and through a
restatement of the reference's control flow (handleUpdate, forward, doForward, setResult as
functions of their own, with the reference's local structures); after prepare and after complete,
the latter twice as for a resent job, the two records must be equal byte for byte, no input field
may have changed, and the d_info counts must agree with what the reference's records show.  No GPU
and no Python process runs the code under test.  The sanitizer runtimes are linked statically, so
the program does not care what the environment preloads: the test neither sets nor strips
LD_PRELOAD.

Run size: 200,000 jobs.  With the generator's distribution the rarest branch (a failed queryChunk,
b_query_failed) is taken about 500 times in such a run, 1,006 times in 400,000; the test asks for
100 of every branch."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
JOBS = 200000
BRANCHES = (
    # A. StorageOperator.cc:401-434
    "bad_update_type", "a_version_adopted", "a_version_equal", "a_4082", "a_missing", "a_committed", "a_stale",
    "a_advance", "a_other_error",
    # B. ReliableForwarding.cc:113-222, BatchReadJob.cc:43-54
    "b_no_successor", "b_read_syncing_request", "b_read_partial_write", "b_read_failed", "b_read_bad_type",
    "b_read_bad_length", "b_read_bad_null", "b_read_none_mismatch", "b_read_mismatch", "b_read_none_ok",
    "b_read_empty_ok", "b_read_ok", "b_read_inline", "b_read_not_inline", "b_query", "b_query_failed", "b_plain",
    "b_syncing_remove", "b_syncing_engine_job",
    # C. ReliableForwarding.cc:233-278,120-134
    "c_ok", "c_ok_syncing", "c_4081", "c_4080_intact", "c_4080_corrupted", "c_4080_none_intact",
    "c_4080_none_corrupted", "c_4080_unhashable",
    # D. StorageOperator.cc:446-485
    "d_returned_in_prepare", "d_4082", "d_remove_exempt_none", "d_remove_exempt_syncing", "d_7015_type",
    "d_7015_value", "d_checksums_equal", "d_forward_error", "d_4033_answered", "d_4033_no_successor")
UNREACHABLE = "c_forward_4081_unreachable"  # forward's own chain-version check (:125) behind doForward's (:238)


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "fuzz_forward")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "cpp", "fuzz_forward.cpp"), "-o", exe])
    return exe


def test_forward_plan_under_asan_ubsan(fuzz_bin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([fuzz_bin, str(JOBS)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fuzz_forward"] == "ok", out
    assert out["jobs"] == JOBS and out["sent"] > JOBS // 4 and out["commits"] > JOBS // 8
    assert set(out["branches"]) == set(BRANCHES), set(out["branches"]) ^ set(BRANCHES)
    assert UNREACHABLE not in out["branches"]
    for name in BRANCHES:
        assert out["branches"][name] >= 100, (name, out)
