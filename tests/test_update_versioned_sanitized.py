"""ASan + UBSan on the version ladders (3fs_amd/csrc/version_plan.h), on the pattern of
tests/test_sync_plan_sanitized.py: tests/cpp/fuzz_version_ladder.cpp is a stand-alone program that
includes the header the kernels include and runs random queues (writes, truncates, extends and
commits over a few chunks, versions right, stale, missing, committed and advanced, near 0 and near
2^32, good and bad payloads, syncing, forced, engine and malformed jobs) through the two ladder
functions, handing state down each chunk's chain as the step kernel does, and through a sequential
restatement of ChunkReplica::update / ::commit over a map of chunk states; every status and every
state after every job must agree.  No GPU and no Python process runs the code under test.  The
sanitizer runtimes are linked statically, so the program does not care what the environment
preloads: the test neither sets nor strips LD_PRELOAD."""
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
    exe = str(tmp_path_factory.mktemp("san") / "fuzz_version_ladder")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "cpp", "fuzz_version_ladder.cpp"), "-o", exe])
    return exe


def test_version_ladders_under_asan_ubsan(fuzz_bin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([fuzz_bin, "4000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fuzz_version_ladder"] == "ok", out
    assert out["queues"] == 4000 and out["jobs"] > 150000
    assert out["deferred"] > 10000 and out["wraps"] > 1000
    assert out["update_codes"] == 10 and out["commit_codes"] == 6  # every answer of both ladders
