"""Every scratch carve fits its byte count, and no byte count moves (tests/cpp/check_scratch_layout.cpp).

A CPU test: the program calls only sizing and carving functions of libhf3fs_crc.so, on a fake base.
It fails as soon as a member of a layout outgrows the slack of its *_scratch_bytes.  The sizes it
prints -- every internal *_scratch_bytes, update_record_cap and the public sizing functions that
need no device -- are compared with tests/golden/scratch_sizes.json, recorded from the same
program: callers who pre-size with the public functions must keep getting the same figures, so a
change of the host layer that moves one has to say so by changing the golden file."""
import importlib
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_scratch_layouts_fit_and_sizes_unchanged():
    b = importlib.import_module("3fs_amd.build")
    b.build_cpp_tests()
    r = subprocess.run([b.CPP_CHECK_LAYOUT], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ALL OK" in r.stdout
    got = {}
    for line in r.stdout.splitlines():
        part = line.split()
        if part[0] == "size":
            got[part[1]] = int(part[2])
    with open(os.path.join(HERE, "golden", "scratch_sizes.json")) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    moved = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not moved, moved
