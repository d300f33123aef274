"""ASan + UBSan on the decisions of hf3fs_crc_client_write_prepare / _complete
(3fs_amd/csrc/client_write_plan.h), on the pattern of tests/test_client_read_sanitized.py:
tests/cpp/fuzz_client_write.cpp is a stand-alone program that includes the header the kernels
include.  It runs random batches through the plan's per-IO ladder, used as the two prepare kernels
use it, and through a restatement of the reference's two validation loops and its send; and
120,000 random files of 0 to 2,000 IOs (every mix of types, zero lengths, failing statuses, short
writes, unknown types, lengths up to 2^32 - 1) through a restatement of writeFile's loop, the plan's
own loop and its order-free summary, the latter bracketed as the wave schedule does it, at random,
and for files of at most 12 IOs cut in two at every position; every field of the file record must
agree.  No GPU and no Python process runs the code under test.  The sanitizer runtimes are linked
statically, so the program does not care what the environment preloads: the test neither sets nor
strips LD_PRELOAD."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
BRANCHES = ("no_ios", "end_status", "end_unknown_type", "end_short", "end_type_bytes", "end_type_zero_length",
            "end_type_none", "zero_length_pass", "foreign_zero_in_front", "adopt_typed", "adopt_none", "combine_crc32c",
            "combine_crc32", "end_first", "end_last", "clean")
FILES = 120000


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "fuzz_client_write")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "cpp", "fuzz_client_write.cpp"), "-o", exe])
    return exe


def test_client_write_plan_under_asan_ubsan(fuzz_bin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([fuzz_bin, str(FILES)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fuzz_client_write"] == "ok", out
    assert out["files"] == FILES and out["ios"] > 1000000 and out["cuts"] > 400000
    assert set(out["branches"]) == set(BRANCHES)
    for name in BRANCHES:  # every branch of the loop was taken by many files
        assert out["branches"][name] > 100, (name, out)
    assert out["batches"] >= FILES // 10 and out["prepare_poisoned_batches"] > 1000
    for kind in ("prepare_sent", "prepare_range", "prepare_bad_record", "prepare_poisoned", "prepare_hashed"):
        assert out[kind] > 1000, (kind, out)
