"""The scratch carve of hf3fs_crc_range_query fits its byte count and the public sizing function is
that count (tests/cpp/check_range_scratch.cpp), a program of its own beside
tests/cpp/check_scratch_layout.cpp and tests/cpp/check_server_read_scratch.cpp.  The sizes recorded in
tests/golden/scratch_sizes.json are other calls' and do not move: the program prints none of them,
and the test checks that the golden file names no size of this call.  A CPU test: the program calls
only sizing and carving functions of libhf3fs_crc.so, on a fake base."""
import importlib
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_carve_fits_and_public_size_is_the_carve(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    b = importlib.import_module("3fs_amd.build")
    b.build()
    exe = str(tmp_path / "check_range_scratch")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(REPO, "tests", "cpp", "check_range_scratch.cpp"), "-o", exe,
                           f"-L{b.LIBDIR}", "-lhf3fs_crc", f"-Wl,-rpath,{b.LIBDIR}", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ALL OK" in r.stdout
    sizes = {p[1]: int(p[2]) for p in (line.split() for line in r.stdout.splitlines()) if p[0] == "size"}
    assert len(sizes) == 13 * 6
    # 12 bytes of prefix per table record, 12 bytes per op, and the share arrays
    assert sizes["range_scratch_bytes/0/0"] >= 2048 * 36 + 16 + 12 + 8
    assert sizes["range_scratch_bytes/1073741824/0"] - sizes["range_scratch_bytes/0/0"] == 12 << 30
    assert sizes["range_scratch_bytes/0/1073741824"] - sizes["range_scratch_bytes/0/0"] == 12 << 30
    with open(os.path.join(REPO, "tests", "golden", "scratch_sizes.json")) as f:
        assert not any("range" in k for k in json.load(f))
