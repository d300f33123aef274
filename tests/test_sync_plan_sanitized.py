"""ASan + UBSan on the resync plan's decisions (3fs_amd/csrc/sync_plan.h), on the pattern of
tests/test_cow_planner_sanitized.py: tests/cpp/fuzz_sync_plan.cpp is a stand-alone program that
includes the header the kernels include and runs random pairs of tables (duplicate ids in both,
ids equal in one half only, empty sides, fatal rows) through a sequential restatement of the
reference loop (unordered_map, erase, break) and through the order-free form the kernels use
(probing table with lowest-index resolution, claims by minimum, classify, histogram, lists); every
class, peer, d_info word and list must agree.  No GPU and no Python process runs the code under
test.  The sanitizer runtimes are linked statically, so the program does not care what the
environment preloads: the test neither sets nor strips LD_PRELOAD."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "fuzz_sync_plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "cpp", "fuzz_sync_plan.cpp"), "-o", exe])
    return exe


def test_sync_plan_under_asan_ubsan(fuzz_bin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([fuzz_bin, "4000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fuzz_sync_plan"] == "ok", out
    assert out["tables"] == 4000 and out["records"] > 800000
    assert out["fatal_tables"] > 500 and out["calm_tables"] > 1500 and out["duplicates"] > 10000
    assert out["classes_seen"] == 15  # twelve remote classes and three local ones
