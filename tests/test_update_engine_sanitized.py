"""ASan + UBSan on the chunk engine's two decisions (3fs_amd/csrc/engine_plan.h), on the pattern of
tests/test_update_versioned_sanitized.py: tests/cpp/fuzz_engine_ladder.cpp is a stand-alone program
that includes the header the kernels include and runs random queues (writes, truncates, extends,
commits, removes and unknown types over a few chunks, versions right, committed and missing, near 0
and near 2^32, good and bad payloads, syncing, missing destinations, live holders the caller
supplies and malformed jobs) through engine_update / engine_commit, handing state down each chunk's
chain as the step kernel does, and through a sequential restatement of Engine::update_chunk /
::commit_chunk over maps of the committed chunks and the writing list; every status, every detail
and the state after every job must agree.  No GPU and no Python process runs the code under test.
The sanitizer runtimes are linked statically, so the program does not care what the environment
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
    exe = str(tmp_path_factory.mktemp("san") / "fuzz_engine_ladder")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "cpp", "fuzz_engine_ladder.cpp"), "-o", exe])
    return exe


def test_engine_decisions_under_asan_ubsan(fuzz_bin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([fuzz_bin, "4000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fuzz_engine_ladder"] == "ok", out
    assert out["queues"] == 4000 and out["jobs"] > 150000
    assert out["deferred"] > 10000 and out["wraps"] > 1000
    assert out["cows"] > 1000 and out["in_place"] > 1000
    assert out["statuses"] == 6   # 0, 3, 4080, 4081, 4008, 4007: every answer of the two decisions
    assert out["details"] == 5    # 0 and the four HF3FS_ENGINE_DETAIL_* reasons
