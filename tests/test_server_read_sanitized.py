"""ASan + UBSan on the decisions of hf3fs_crc_server_read_prepare / _complete
(3fs_amd/csrc/server_read_plan.h), on the pattern of tests/test_forward_sanitized.py:
tests/cpp/fuzz_server_read.cpp is a stand-alone program that includes the header the kernels include
and runs random requests through it and through a restatement of the reference's control flow
(batchRead, BufferPool::Buffer, aioPrepareRead, setReadJobResult, setResult, aioFinishRead,
copyToRespBuffer, addBufferToBatch and RDMAReqBatch::add as functions of their own, with the
reference's local structures); after prepare and after complete, the latter twice, the records must
be equal byte for byte, the inline layout and the RDMA list must be equal, and no input field may
have changed but an engine job's commit_ver.  No GPU and no Python process runs the code under
test.  The sanitizer runtimes are linked statically, so the program does not care what the
environment preloads: the test neither sets nor strips LD_PRELOAD.

Run size: 80,000 requests (about 550,000 jobs).  With the generator's distribution the rarest branch
(a big read served from a big buffer's room, p_carve_big_from_big) is taken 51 times in 20,000
requests, so about 200 times here; the test asks for 100 of every branch."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
REQUESTS = 80000
BRANCHES = (
    # prepare: StorageOperator.cc:98-155, BatchReadJob.cc:16-22, BufferPool.cc:102-141
    "p_empty_request", "p_offset_plus_length_wraps", "p_target_error", "p_not_up_to_date", "p_bad_buffer_size",
    "p_carve_first_small", "p_carve_fits", "p_carve_new_small", "p_carve_new_big", "p_carve_small_from_big",
    "p_carve_big_from_big", "p_carve_2019",
    # aioPrepareRead: ChunkReplica.cc:38-76, ChunkEngine.h:34-73
    "p_meta_error_replica", "p_meta_error_engine", "p_engine", "p_replica_4004", "p_replica_uncommitted_allowed",
    "p_replica_ok",
    # setReadJobResult: AioStatus.cc:27-55, and the call's limits
    "c_failed_in_prepare", "c_limit_type", "c_limit_length", "c_limit_null", "c_4010", "c_res_below_head",
    "c_clip_zero", "c_clip_res", "c_clip_length", "c_clip_chunk_len",
    # setResult: BatchReadJob.cc:24-63, aioFinishRead
    "c_rung1_none", "c_rung1_reuse", "c_rung1_reuse_engine", "c_rung1_create", "c_rung1_create_empty",
    "c_finish_engine", "c_finish_meta_error", "c_finish_4004", "c_finish_ok", "c_recalc_skipped_after_finish_error",
    "c_recalc_ok", "c_recalc_4080", "c_recalc_none_ok", "c_recalc_none_4080",
    # the transmission: BatchReadJob.cc:74-113, IBSocket.cc:258-275
    "x_inline", "x_inline_empty", "x_rdma_listed", "x_rdma_listed_empty", "x_rdma_null", "x_rdma_no_rkey",
    "x_rdma_max_msg_sz", "x_none")
UNREACHABLE = "x_rdma_buf_size_unreachable"  # length > rdmabuf.size() behind batchRead's own check (:122-128)


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "fuzz_server_read")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "cpp", "fuzz_server_read.cpp"), "-o", exe])
    return exe


def test_server_read_plan_under_asan_ubsan(fuzz_bin):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([fuzz_bin, str(REQUESTS)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["fuzz_server_read"] == "ok", out
    assert out["requests"] == REQUESTS and out["ok_requests"] > REQUESTS // 2 and out["ok_jobs"] > out["jobs"] // 4
    assert set(out["branches"]) == set(BRANCHES), set(out["branches"]) ^ set(BRANCHES)
    assert UNREACHABLE not in out["branches"]
    for name in BRANCHES:
        assert out["branches"][name] >= 100, (name, out)
