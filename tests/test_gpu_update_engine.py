"""hf3fs_crc_update_engine on the GPU: a chunk-engine target's queue of update and commit jobs.

Every expectation comes from tests/engine_cases.py: Engine::update_chunk and Engine::commit_chunk
transcribed from the reference and applied one job at a time in index order, bytes and checksums
from the oracle.  After every call the WHOLE d_ios array, the WHOLE d_jobs array (the overwritten
before-state of later jobs included, with junk sent in those fields), d_info and the WHOLE arena --
every committed allocation, every destination used or not, the guards between them -- must equal
the model's, and the payload arena must be unchanged.  Chunk sizes are 512 B (every range inside
one piece) and 128 KiB (several pieces at every apply_piece_kib).
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import engine_cases as ec
import update_footprint as fp

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = 16 << 10
MODES = [0, 1]
SIZES = list(ec.SIZES)
INFO_FILL = 0x7777


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(orc, name):
    """Built once and shared by every test and variant; never modified."""
    b = ec.all_cases(orc)[name]()
    for a in (b.rec, b.jr, b.pay, b.arena0, b.arena1):
        a.setflags(write=False)
    return b


class Box:
    """Device images of one case: the arena on a 16 KiB line, the payloads, both record arrays, d_info."""

    def __init__(self, dev, arena_size, pay_size, n):
        self.dev = dev
        raw = torch.empty(arena_size + LINE, dtype=torch.uint8, device=dev)
        lift = (-raw.data_ptr()) % LINE
        self.raw, self.arena = raw, raw[lift:lift + arena_size]
        self.pay = torch.empty(pay_size, dtype=torch.uint8, device=dev)
        self.rec = torch.empty(n * fp.REC.itemsize, dtype=torch.uint8, device=dev)
        self.jr = torch.empty(n * ec.JOB.itemsize, dtype=torch.uint8, device=dev)
        self.dst = torch.empty(n, dtype=torch.int64, device=dev)
        self.info = torch.full((ec.INFO_WORDS,), INFO_FILL, dtype=torch.int32, device=dev)

    def _up(self, a):
        return torch.from_numpy(np.array(a)).to(self.dev)

    def load(self, b):
        """Arena, payloads -> the two record arrays with absolute addresses, as sent."""
        self.arena[:b.arena0.size].copy_(self._up(b.arena0))
        self.pay[:b.pay.size].copy_(self._up(b.pay))
        return ec.record_arrays(b, self.arena.data_ptr(), self.pay.data_ptr())

    def send(self, rec, jr=None):
        self.rec[:rec.size * fp.REC.itemsize].copy_(self._up(rec.view(np.uint8)))
        if jr is not None:
            self.jr[:jr.size * ec.JOB.itemsize].copy_(self._up(jr.view(np.uint8)))
        self.info.fill_(INFO_FILL)
        torch.cuda.synchronize()

    def fetch(self, n, arena_size):
        torch.cuda.synchronize()
        rec = np.frombuffer(self.rec.cpu().numpy().tobytes()[:n * fp.REC.itemsize], dtype=fp.REC)
        jr = np.frombuffer(self.jr.cpu().numpy().tobytes()[:n * ec.JOB.itemsize], dtype=ec.JOB)
        return rec, jr, self.arena[:arena_size].cpu().numpy(), tuple(int(x) for x in self.info.cpu().numpy())


def _box_for(dev, *cases):
    return Box(dev, max(b.arena0.size for b in cases), max(b.pay.size for b in cases), max(b.n for b in cases))


def _same(got, want, dtype, what):
    if got.tobytes() == want.tobytes():
        return
    for name in dtype.names:
        bad = np.flatnonzero((got[name] != want[name]).reshape(got.size, -1).any(axis=1))
        if bad.size:
            i = int(bad[0])
            pytest.fail(f"{what}: {bad.size} jobs differ in {name}, first job {i}: got {got[name][i]}, "
                        f"want {want[name][i]}")
    pytest.fail(f"{what}: records differ")


def _same_arena(got, want, b, what):
    if got.tobytes() == want.tobytes():
        return
    pos = int(np.flatnonzero(got != want)[0])
    r = max(0, int(np.searchsorted(b.regions, pos, side="right")) - 1)
    pytest.fail(f"{what}: arena differs at {pos} (region {r} base {b.regions[r]} + {pos - b.regions[r]}, "
                f"max_len {b.max_len}): got {got[pos]}, want {want[pos]}")


def _engine(hf, box, b, mode, n=None, max_rounds=None, stream=None):
    hf.update_engine(b.ctype, box.rec, box.jr, b.n if n is None else n, b.max_len,
                     b.max_rounds if max_rounds is None else max_rounds, mode=mode, info=box.info,
                     stream=stream or torch.cuda.current_stream())


def _check(box, b, sent_rec, sent_jr, expect, info, arena1, what):
    rec, jr, arena, got_info = box.fetch(sent_rec.size, b.arena0.size)
    want_rec, want_jr = ec.expected(sent_rec, sent_jr, expect, box.arena.data_ptr())
    _same(rec, want_rec, fp.REC, f"{what}: d_ios")
    _same(jr, want_jr, ec.JOB, f"{what}: d_jobs")
    _same_arena(arena, arena1, b, what)
    assert got_info == tuple(info), what
    assert bytes(box.pay[:b.pay.size].cpu().numpy()) == b.pay.tobytes(), f"{what}: a payload byte changed"
    return rec, jr


def _run_and_check(hf, box, b, mode, what):
    rec, jr = box.load(b)
    box.send(rec, jr)
    _engine(hf, box, b, mode)
    return _check(box, b, rec, jr, b.expect, b.info, b.arena1, what)


# ---- 1. every status and detail, and what goes first -----------------------------------------------------
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_every_status_detail_and_the_precedence_pairs(hf, orc, dev, mode, max_len):
    """One job per chunk: each rung and each detail; a malformed record over 4080; 4080 over 4081,
    4008, 4007, "in writing" and a missing dst; 4081 over 4008; 4007 over a missing dst; io_ver 0
    assigns chunk_ver + 1; a syncing write at versions that wrap; truncate and extend in place;
    commits with and without a writing version.  Refused jobs leave the arena identical."""
    b = _case(orc, f"singles_{max_len}")
    rec, jr = _run_and_check(hf, _box_for(dev, b), b, mode, b.name)
    got = {(int(s), int(d)) for s, d in zip(rec["status"], jr["detail"])}
    assert got == {(0, 0), (3, 1), (3, 2), (3, 3), (3, 4), (4080, 0), (4081, 0), (4008, 0), (4007, 0)}
    assert set(int(x) for x in jr["out_cow"]) == {0, 1}


# ---- 2. the queues the call exists for ----------------------------------------------------------------------
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_chains_of_updates_and_commits(hf, orc, dev, mode, max_len):
    """Ten interleaved chains: U C eight deep with appends in place and overwrites copied (the
    committed address moves twice, a later append lands in a former dst); U U C; a bad-payload U
    then a good one; C first on a supplied writing version; C with none; a shortening truncate then
    a write inside the old length (in place by the true state); append, commit, write at the old end
    (copy-on-write by the true state); a copy-on-write whose committed allocation stays byte-identical;
    an update met by a supplied writing version; a syncing write."""
    b = _case(orc, f"chains_{max_len}")
    rec, jr = _run_and_check(hf, _box_for(dev, b), b, mode, b.name)
    by = {}
    for i, job in enumerate(b.jobs):
        by.setdefault(job["c"], []).append(i)
    assert [int(jr["out_cow"][i]) for i in by[5]] == [0, 0, 0, 0] and b.jobs[by[5][2]]["stale_cow"]
    assert [int(jr["out_cow"][i]) for i in by[6]] == [0, 0, 1, 0] and not b.jobs[by[6][2]]["stale_cow"]
    x = b.keys[7]  # readers of the committed version rely on it
    assert b.arena1[x:x + max_len].tobytes() == b.arena0[x:x + max_len].tobytes()
    assert int(jr["out_cow"][by[7][0]]) == 1


# ---- 3. depth overflow --------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_depth_overflow_and_resubmission(hf, orc, dev, mode, max_len):
    """Chains of 5 under max_rounds 3: the NOT_APPLIED jobs carry committed and writing state after
    the chunk's last applied job in both arrays; resubmitted unchanged they reach the model's end."""
    b = _case(orc, f"overflow_{max_len}")
    box = _box_for(dev, b)
    rec, jr = _run_and_check(hf, box, b, mode, b.name)
    late = np.flatnonzero(rec["status"] == ec.NOT_APPLIED)
    assert list(late) == b.again.idx
    assert (jr["w_addr"][late] != 0).any() and (jr["w_addr"][late] == 0).any()
    again_rec, again_jr = np.ascontiguousarray(rec[late]), np.ascontiguousarray(jr[late])
    box.send(again_rec, again_jr)
    _engine(hf, box, b, mode, n=late.size)
    _check(box, b, again_rec, again_jr, b.again.expect, b.again.info, b.again.arena1, "resubmitted")


# ---- 4. random queues -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ec.SEEDS)
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_random_queues(hf, orc, dev, mode, max_len, seed):
    """64 chunks, up to 8 jobs each, every job kind, both payload verdicts, supplied writing versions."""
    b = _case(orc, f"random_{max_len}_{seed:x}")
    _run_and_check(hf, _box_for(dev, b), b, mode, b.name)


# ---- 5. distinct chunks: update_cow_batch with the host's choice of d_dst ---------------------------------
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_distinct_chunks_equal_update_cow_batch(hf, orc, dev, mode, max_len):
    """All chunks distinct, no commits, no writing state, admitting versions: the IO records and every
    byte equal hf3fs_crc_update_cow_batch on the same records with d_dst chosen on the host by
    engine.rs:377-380 from the (here: true) queue-time length."""
    b = _case(orc, f"distinct_{max_len}")
    box = _box_for(dev, b)
    rec, jr = box.load(b)
    box.send(rec, jr)
    _engine(hf, box, b, mode)
    rec1, _ = _check(box, b, rec, jr, b.expect, b.info, b.arena1, b.name)
    arena1 = box.arena[:b.arena0.size].cpu().numpy()
    dst = np.array([int(jr["dst"][i]) if job["stale_cow"] else 0 for i, job in enumerate(b.jobs)], dtype=np.int64)
    assert (dst != 0).any() and (dst == 0).any()
    box.load(b)
    box.send(rec)
    box.dst[:b.n].copy_(torch.from_numpy(dst).to(dev))
    hf.update_cow(b.ctype, box.rec, box.dst, b.n, b.max_len, mode=mode, stream=torch.cuda.current_stream())
    rec0, _, arena0, _ = box.fetch(b.n, b.arena0.size)
    _same(rec1, rec0, fp.REC, "update_engine vs update_cow_batch")
    _same_arena(arena1, arena0, b, "update_engine vs update_cow_batch")


# ---- 6. options and lifetimes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_random_queue_under_poisoned_scratch(hf, orc, dev, opts, mode):
    """Every scratch word the call reads it wrote first: scratch filled with 0xA5A5A5A5, then
    0xFFFFFFFF, then not at all."""
    b = _case(orc, f"random_{128 << 10}_{ec.SEEDS[0]:x}")
    p = _case(orc, f"chains_{128 << 10}")
    box = _box_for(dev, b, p)
    for pattern in (0xA5A5A5A5, 0xFFFFFFFF, 0):
        opts("poison", pattern)
        _run_and_check(hf, box, b, mode, f"poison {pattern:#x}")
        _run_and_check(hf, box, p, mode, f"poison {pattern:#x} (chains)")


@pytest.mark.parametrize("option", [("apply_piece_kib", 4), ("apply_piece_kib", 16), ("apply_grid", 2)])
@pytest.mark.parametrize("mode", MODES)
def test_piece_size_and_short_grid(hf, orc, dev, opts, mode, option):
    """Pieces of 4 and 16 KiB, and one workgroup per CU looping over the pieces."""
    opts(*option)
    for name in (f"chains_{128 << 10}", f"random_{128 << 10}_{ec.SEEDS[1]:x}"):
        b = _case(orc, name)
        _run_and_check(hf, _box_for(dev, b), b, mode, f"{name} {option}")


@pytest.mark.parametrize("mode", MODES)
def test_scratch_does_not_grow_on_a_second_call(hf, orc, dev, mode):
    """After one call the pair's buffer holds update_engine_scratch_bytes and a second call of the
    same shape allocates nothing."""
    L = hf._lib
    b = _case(orc, f"chains_{128 << 10}")
    box = _box_for(dev, b)
    s = torch.cuda.Stream(dev)
    need = L.update_engine_scratch_bytes(b.n, b.max_len, b.max_rounds, mode=mode)
    assert need > L.update_cow_scratch_bytes(b.n, b.max_len, mode=mode) > 0
    assert L.update_engine_scratch_bytes(b.n, b.max_len, 65, mode=mode) == 0
    with torch.cuda.stream(s):
        for k in range(2):
            rec, jr = box.load(b)
            box.send(rec, jr)
            _engine(hf, box, b, mode, stream=s)
            _check(box, b, rec, jr, b.expect, b.info, b.arena1, f"call {k}")
            stats = L.pair_scratch_stats(s)
            if k == 0:
                first = stats
                assert first["call_bytes"] >= need
    assert stats == first
    L.release_stream(s)


@pytest.mark.parametrize("mode", MODES)
def test_captured_call_replans_after_the_records_were_rewritten(hf, orc, dev, mode):
    """One captured call replayed on two queues of the same shape whose records differ: ranking, the
    engine's decisions and the deferred verify all run in kernels, from what the records hold at
    replay time."""
    L = hf._lib
    a, b = _case(orc, f"random_{128 << 10}_{ec.SEEDS[0]:x}"), _case(orc, f"random_{128 << 10}_{ec.SEEDS[1]:x}")
    n = min(a.n, b.n)
    box = _box_for(dev, a, b)
    L.release_graph_scratch()
    base = L.graph_scratch_stats()
    rec, jr = box.load(a)
    box.send(rec, jr)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        _engine(hf, box, a, mode, n=n, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    for case in (a, b, a):
        short = ec.truncated(orc, case, n)
        rec, jr = box.load(case)
        rec, jr = np.ascontiguousarray(rec[:n]), np.ascontiguousarray(jr[:n])
        box.send(rec, jr)
        g.replay()
        _check(box, case, rec, jr, short.expect, short.info, short.arena1, f"replay of {case.name}")
    del g
    torch.cuda.synchronize()
    L.release_graph_scratch()
    end = L.graph_scratch_stats()
    assert end["live"] == base["live"] and end["live_bytes"] == base["live_bytes"] and end["dead"] == 0, (base, end)


# ---- the first library call of a process, captured ------------------------------------------------
_CHILD = r"""
import importlib, hashlib, json, sys, types
import numpy as np, torch
repo, tests, path, mode = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
sys.path[:0] = [repo, tests]
import engine_cases as ec
import update_footprint as fp
hf = importlib.import_module("3fs_amd")
z = np.load(path)
dev = torch.device("cuda:0")
raw = torch.empty(z["arena"].size + 16384, dtype=torch.uint8, device=dev)
lift = (-raw.data_ptr()) % 16384
arena = raw[lift:lift + z["arena"].size]
arena.copy_(torch.from_numpy(z["arena"]).to(dev))
pay = torch.from_numpy(z["pay"]).to(dev)
case = types.SimpleNamespace(rec=z["rec"], jr=z["jr"], has_payload=z["has_payload"])
rec, jr = ec.record_arrays(case, arena.data_ptr(), pay.data_ptr())
n = rec.size
d_ios = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
d_jobs = torch.from_numpy(jr.view(np.uint8).copy()).to(dev)
info = torch.full((8,), 0x7777, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library call, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            hf.update_engine(hf.CRC32C, d_ios, d_jobs, n, int(z["max_len"]), int(z["max_rounds"]), mode=mode, info=info,
                             stream=torch.cuda.current_stream())
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "update_engine failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
print(json.dumps({"rec_sha256": hashlib.sha256(d_ios.cpu().numpy().tobytes()).hexdigest(),
                  "jobs_sha256": hashlib.sha256(d_jobs.cpu().numpy().tobytes()).hexdigest(),
                  "status": np.frombuffer(d_ios.cpu().numpy().tobytes(), dtype=fp.REC)["status"].tolist(),
                  "info": info.cpu().numpy().tolist(),
                  "arena_sha256": hashlib.sha256(arena.cpu().numpy().tobytes()).hexdigest(),
                  "arena_ptr": int(arena.data_ptr()), "pay_ptr": int(pay.data_ptr())}))
"""


def test_first_call_in_process_is_a_captured_engine_call(orc, tmp_path):
    """A fresh process whose first library call is a DELTA update_engine inside
    torch.cuda.graph(capture_error_mode="global"); the child replays the graph once and reports
    digests of both record arrays and the arena."""
    repo = REPO
    b = _case(orc, f"chains_{128 << 10}")
    path = str(tmp_path / "inputs.npz")
    np.savez(path, arena=b.arena0, pay=b.pay, rec=b.rec, jr=b.jr, has_payload=b.has_payload, max_len=b.max_len,
             max_rounds=b.max_rounds)
    p = subprocess.run([sys.executable, "-c", _CHILD, repo, os.path.join(repo, "tests"), path, "1"],
                       capture_output=True, text=True, timeout=150, cwd=repo)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    got = lines[0]
    assert got["status"] == [e[0] for e in b.expect]
    sent_rec, sent_jr = ec.record_arrays(b, got["arena_ptr"], got["pay_ptr"])
    want_rec, want_jr = ec.expected(sent_rec, sent_jr, b.expect, got["arena_ptr"])
    assert got["rec_sha256"] == hashlib.sha256(want_rec.tobytes()).hexdigest()
    assert got["jobs_sha256"] == hashlib.sha256(want_jr.tobytes()).hexdigest()
    assert got["arena_sha256"] == hashlib.sha256(b.arena1.tobytes()).hexdigest()
    assert tuple(got["info"]) == b.info
