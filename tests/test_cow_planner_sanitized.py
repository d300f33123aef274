"""ASan + UBSan on the update path's planner (3fs_amd/csrc/update_plan.h), on the pattern of
tests/test_sanitizers.py: tests/cpp/fuzz_cow_planner.cpp is a stand-alone program that includes
the header the kernels include, enumerates every range and one-shot piece of 300 000 random IOs
(all chunk / destination / payload residues mod 16, 4 / 8 / 16 KiB pieces, sizes around every cut
line, failed and invalid IOs), plays the pieces into a byte map and compares it with a model of
the image.  No GPU and no Python process runs the code under test.  The sanitizer runtimes are
linked statically, so the program does not care what the environment preloads: the test neither
sets nor strips LD_PRELOAD."""
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
    exe = str(tmp_path_factory.mktemp("san") / "fuzz_cow_planner")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "cpp", "fuzz_cow_planner.cpp"), "-o", exe])
    return exe


def test_cow_planner_under_asan_ubsan(fuzz_bin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([fuzz_bin, "300000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fuzz_cow_planner"] == "ok", out
    assert out["ios"] == 300000 and out["out_of_place"] > 100000 and out["syncing"] > 5000 and out["invalid"] > 30000
