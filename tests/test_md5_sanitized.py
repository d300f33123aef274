"""ASan + UBSan on the byte handling of hf3fs_crc_md5_batch (3fs_amd/csrc/md5_core.h), on the
pattern of tests/test_sync_plan_sanitized.py: tests/cpp/fuzz_md5.cpp is a stand-alone program that
includes the header the kernels include.  This test writes the cases -- random contents, their cut
into segments with empty ones and holes, the address residue 0..15 of the first segment, the split
over 1-4 calls with the state carried, and hashlib's digest of each -- and the program replays them
through the core's cursor, granule, tail and padding functions the way the hash kernel walks a file.
No GPU and no Python process runs the code under test.  The sanitizer runtimes are linked
statically, so the program does not care what the environment preloads: the test neither sets nor
strips LD_PRELOAD.

A second kind of case is a file that is one hole of 2^29 - 1 .. 2^32 + 5 bytes: totals whose bit
length needs its upper word, where bytes cost nothing."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import md5_queue as mq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "fuzz_md5")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "cpp", "fuzz_md5.cpp"), "-o", exe])
    return exe


def _case(rng, n_bytes, n_calls, residue):
    """One line of the case file (its format is in fuzz_md5.cpp)."""
    content = bytearray(rng.integers(0, 256, n_bytes, dtype=np.uint8).tobytes())
    n_segs = int(rng.integers(0, 9))
    cuts = sorted(int(x) for x in rng.integers(0, n_bytes + 1, n_segs))
    if n_segs >= 2 and rng.random() < 0.3:
        cuts[1] = cuts[0]  # an empty segment
    edges = [0] + cuts + [n_bytes]
    segs = []
    for a, b in zip(edges, edges[1:]):
        hole = rng.random() < 0.2
        if hole:
            content[a:b] = bytes(b - a)
        segs.append((1 if hole else 0, b - a))
    call_of = sorted(int(x) for x in rng.integers(0, n_calls, len(segs)))  # ascending: file order
    words = [str(residue), hashlib.md5(content).hexdigest(), content.hex() or "-", str(n_calls)]
    for c in range(n_calls):
        mine = [s for s, k in zip(segs, call_of) if k == c]
        words.append(str(len(mine)))
        words += [f"{kind} {length}" for kind, length in mine]
    return " ".join(words)


def test_md5_core_under_asan_ubsan(fuzz_bin, tmp_path):
    rng = np.random.default_rng(0x3D5)
    lines = []
    for i in range(3000):
        n_bytes = int(rng.integers(0, 600)) if i % 8 else int(rng.integers(0, 5000))
        lines.append(_case(rng, n_bytes, 1 + i % 4, i % 16))
    for n_bytes in range(0, 130):  # every padding shape, one segment, one call
        lines.append(_case(np.random.default_rng(n_bytes), n_bytes, 1, n_bytes % 16))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([fuzz_bin, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fuzz_md5"] == "ok", out
    assert out["cases"] == len(lines) and out["calls"] > 7000
    assert out["tail_lengths"] == 64 and out["residues"] == 16  # every carried length, every alignment
    assert out["pad_one"] > 500 and out["pad_two"] > 100         # both padding shapes
    assert out["granule_blocks"] > 5000 and out["cursor_blocks"] > 5000 and out["hole_blocks"] > 200
    assert out["holes"] > 1000 and out["empty_segs"] > 500 and out["empty_calls"] > 300


def _md5_of_zeros(n):
    h, zeros = hashlib.md5(), bytes(1 << 24)
    for _ in range(n >> 24):
        h.update(zeros)
    h.update(zeros[:n & ((1 << 24) - 1)])
    return h.hexdigest()


def test_md5_core_long_holes_under_asan_ubsan(fuzz_bin, tmp_path):
    """A hole-only file of N bytes for N = 2^29 - 1, 2^29, 2^29 + 57 and 2^32 + 5 through the
    core's block count, hole blocks, state and padding: the digest is hashlib's of N zero bytes, so
    total * 8 and total % 64 hold where the bit length passes 32 bits.  The {h, total} the program
    prints before the padding are the seeds tests/test_gpu_md5_queue.py starts the GPU from
    (md5_queue.LONG_HOLES).  hashlib works through the same zeros while the program runs."""
    assert sorted(mq.LONG_HOLES) == [(1 << 29) - 1, 1 << 29, (1 << 29) + 57, (1 << 32) + 5]
    path = tmp_path / "holes.txt"
    path.write_text("".join(f"H {n} {digest}\n" for n, (_, digest) in mq.LONG_HOLES.items()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    with subprocess.Popen([fuzz_bin, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) as p:
        try:
            ours = {n: _md5_of_zeros(n) for n in mq.LONG_HOLES}
            stdout, stderr = p.communicate(timeout=600)
        except BaseException:
            p.kill()
            raise
    assert ours == {n: digest for n, (_, digest) in mq.LONG_HOLES.items()}
    assert p.returncode == 0, stdout[-2000:] + stderr[-4000:]
    lines = [json.loads(x) for x in stdout.strip().splitlines()]
    assert lines[-1]["fuzz_md5"] == "ok" and lines[-1]["cases"] == lines[-1]["long_holes"] == 4, lines[-1]
    assert lines[-1]["hole_blocks"] == sum(n // 64 * (2 if n < 1 << 30 else 1) for n in mq.LONG_HOLES)
    assert lines[-1]["pad_one"] > 0 and lines[-1]["pad_two"] > 0
    seeds = {x["hole"]: (tuple(x["h"]), x["total"]) for x in lines[:-1]}
    assert seeds == {n: (h, n) for n, (h, _) in mq.LONG_HOLES.items()}
