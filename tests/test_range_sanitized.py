"""ASan + UBSan on the decisions of hf3fs_crc_range_query and hf3fs_crc_file_length
(3fs_amd/csrc/range_plan.h), on the pattern of tests/test_server_read_sanitized.py:
tests/cpp/fuzz_range_plan.cpp is a stand-alone program that includes the header the kernels include
and holds its closed forms to restatements of the reference's loops: queryChunks' descending walk and
processQueryResults' paged loop (every op at two page sizes, which must agree), queryLastChunk's and
removeChunks' processors, and queryChunksByChain / queryChunks with a std::map.  Every probe of a
binary search is checked against its array's bounds.  No GPU and no Python process runs the code
under test.  The sanitizer runtimes are linked statically, so the program does not care what the
environment preloads: the test neither sets nor strips LD_PRELOAD.

Run size: 20,000 tables of up to 60 records with up to 12 ops each, and 80,000 files.  The rarest
branch (f_too_many_ops, 1 file in 40 of those whose segment fits) is taken about 2,000 times; the
test asks for 100 of every branch but the one fixed check of list_first's saturation."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ROUNDS = 20000
BRANCHES = (
    # the table and the op's own checks
    "r_unsorted", "r_status_in", "r_bad_kind",
    # the span: ChunkStore.cc:120-147
    "r_begin_equals_end", "r_begin_above_end", "r_no_normal_record", "r_end_is_a_record", "r_begin_is_a_record",
    # the paged loop: StorageOperator.cc:653-751
    "r_unlimited", "r_more", "r_limit_equals_normals", "r_limit_clamped", "r_several_pages", "r_page_of_one",
    "r_lowest_processed_by_rank", "r_total_len_past_32_bits",
    # the processors: :875-891, :949-971
    "r_query", "r_remove", "r_list",
    # queryChunksByChain: FileOperation.cc:127-176
    "f_too_many_ops", "f_segment_past_the_ops", "f_not_found_skipped", "f_op_status", "f_no_chunks_skipped",
    "f_invalid_id", "f_inode_mismatch", "f_busy", "f_dyn_below_stripe", "f_chain_replaced",
    # queryChunks: :45-76
    "f_length_tie", "f_later_chain_wins", "f_no_entry", "f_ok")
ONCE = "r_list_first_saturates"


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "fuzz_range_plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "cpp", "fuzz_range_plan.cpp"), "-o", exe])
    return exe


def test_range_plan_under_asan_ubsan(fuzz_bin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([fuzz_bin, str(ROUNDS)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fuzz_range_plan"] == "ok" and out["rounds"] == ROUNDS, out
    assert set(out["branches"]) == set(BRANCHES) | {ONCE}, set(out["branches"]) ^ (set(BRANCHES) | {ONCE})
    for name in BRANCHES:
        assert out["branches"][name] >= 100, (name, out)
