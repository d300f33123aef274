"""ASan + UBSan on the decisions of hf3fs_crc_client_read_batch (3fs_amd/csrc/client_read_plan.h), on
the pattern of tests/test_sync_plan_sanitized.py: tests/cpp/fuzz_client_read.cpp is a stand-alone
program that includes the header the kernels include and runs random parents of 0 to 2,000 children
(every mix of types, zero lengths, failing statuses, verify mismatches, bad records, lengths up to
2^32 - 1) through a restatement of the reference's merge loop and through the plan's own loop and
its order-free fold, the latter bracketed as the wave schedule does it and at random; every field of
the parent must agree, and every verdict must follow the rules restated in the program.  No GPU and
no Python process runs the code under test.  The sanitizer runtimes are linked statically, so the
program does not care what the environment preloads: the test neither sets nor strips LD_PRELOAD."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
BRANCHES = ("no_children", "take_first", "take_middle", "take_last", "take_mismatch", "take_bad_record",
            "adopt_typed", "adopt_none", "type_ignored", "zero_length", "combine_crc32c", "combine_crc32",
            "length_wrap", "clean")


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "fuzz_client_read")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "cpp", "fuzz_client_read.cpp"), "-o", exe])
    return exe


def test_client_read_plan_under_asan_ubsan(fuzz_bin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([fuzz_bin, "6000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fuzz_client_read"] == "ok", out
    assert out["parents"] == 6000 and out["children"] > 500000
    assert set(out["branches"]) == set(BRANCHES)
    for name in BRANCHES:  # every branch of the loop was taken by many parents
        assert out["branches"][name] > 100, (name, out)
    for kind in ("verdict_ok", "verdict_bad_record", "verdict_mismatch", "verdict_failed"):
        assert out[kind] > 1000, (kind, out)
