"""hf3fs_crc_update_ordered on the GPU: batches in arrival order whose IOs may share a chunk.

Every expectation comes from tests/ordered_cases.py: the oracle's ChunkReplica::update (or chunk
engine write) applied one IO at a time in index order.  After every call the WHOLE record array
(output fields and the three state input fields the call rewrites) and the WHOLE chunk arena,
canary guards included, must equal the model's.  Chunk sizes are the reference's own test sizes,
512 B and 128 KiB (TestStorageClientInterface.cc:431-457).
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ordered_cases as oc
import update_footprint as fp

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = 16 << 10
MODES = [0, 1]
SIZES = [512, 128 << 10]
PIPELINES = ["fused", "ticketed", "oneshot"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(orc, name):
    """Built once and shared by every test and variant; never modified."""
    b = oc.all_cases(orc)[name]()
    for a in (b.rec, b.pay, b.arena0, b.arena1):
        a.setflags(write=False)
    return b


def _set_pipeline(opts, pipeline):
    opts("update_pipeline", "fused" if pipeline == "fused" else "unfused")
    if pipeline == "ticketed":
        opts("apply_grid", 0)
    if pipeline == "oneshot":
        opts("apply_grid", 1)


class Box:
    """Device images of one case: the arena on a 16 KiB line, the payloads, the records, d_info."""

    def __init__(self, dev, arena_size, pay_size, n):
        self.dev = dev
        raw = torch.empty(arena_size + LINE, dtype=torch.uint8, device=dev)
        lift = (-raw.data_ptr()) % LINE
        self.raw, self.arena = raw, raw[lift:lift + arena_size]
        self.pay = torch.empty(pay_size, dtype=torch.uint8, device=dev)
        self.rec = torch.empty(n * fp.REC.itemsize, dtype=torch.uint8, device=dev)
        self.info = torch.full((2,), 0x7777, dtype=torch.int32, device=dev)

    def _up(self, a):
        return torch.from_numpy(np.array(a)).to(self.dev)

    def load(self, b, arena=None):
        """-> the record array as sent (absolute addresses)."""
        self.arena.copy_(self._up(b.arena0 if arena is None else arena))
        self.pay[:b.pay.size].copy_(self._up(b.pay))
        sent = oc.record_array(b, self.arena.data_ptr(), self.pay.data_ptr())
        self.send(sent)
        return sent

    def send(self, rec):
        self.rec[:rec.size * fp.REC.itemsize].copy_(self._up(rec.view(np.uint8)))
        self.info.fill_(0x7777)
        torch.cuda.synchronize()

    def fetch(self, n):
        torch.cuda.synchronize()
        rec = np.frombuffer(self.rec.cpu().numpy().tobytes()[:n * fp.REC.itemsize], dtype=fp.REC)
        return rec, self.arena.cpu().numpy(), [int(x) for x in self.info.cpu().numpy()]


def _box_for(dev, *cases):
    return Box(dev, max(b.arena0.size for b in cases), max(b.pay.size for b in cases), max(b.n for b in cases))


def _same_records(got, want, what):
    if got.tobytes() == want.tobytes():
        return
    for name in fp.REC.names:
        bad = np.flatnonzero((got[name] != want[name]).reshape(got.size, -1).any(axis=1))
        if bad.size:
            i = int(bad[0])
            pytest.fail(f"{what}: {bad.size} IOs differ in {name}, first IO {i}: got {got[name][i]}, "
                        f"want {want[name][i]} (status got {got['status'][i]}, want {want['status'][i]})")
    pytest.fail(f"{what}: records differ")


def _same_arena(got, want, b, what):
    if got.tobytes() == want.tobytes():
        return
    pos = int(np.flatnonzero(got != want)[0])
    c = max(0, int(np.searchsorted(b.bases, pos, side="right")) - 1)
    pytest.fail(f"{what}: arena differs at {pos} (chunk {c} base {b.bases[c]} + {pos - b.bases[c]}, "
                f"max_len {b.max_len}): got {got[pos]}, want {want[pos]}")


def _ordered(hf, box, b, mode, n=None, max_rounds=None, stream=None):
    hf._lib.update_ordered(b.ctype, box.rec, b.n if n is None else n, b.max_len,
                           b.max_rounds if max_rounds is None else max_rounds, mode=mode, info=box.info,
                           stream=stream or torch.cuda.current_stream())


def _run_and_check(hf, box, b, mode, what):
    sent = box.load(b)
    _ordered(hf, box, b, mode)
    rec, arena, info = box.fetch(b.n)
    _same_records(rec, oc.expected_records(b, sent), what)
    _same_arena(arena, b.arena1, b, what)
    assert tuple(info) == b.info, what
    assert bytes(box.pay[:b.pay.size].cpu().numpy()) == b.pay.tobytes(), f"{what}: a payload byte changed"
    return rec


# ---- 1. distinct chunks == update_batch --------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("max_rounds", [1, 4])
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_distinct_chunks_equal_update_batch(hf, orc, dev, opts, mode, max_len, max_rounds, pipeline):
    """64 IOs on 64 chunks: records and chunk images byte-identical to hf3fs_crc_update_batch from
    the same start (and to the oracle), d_info == [1, 0]."""
    _set_pipeline(opts, pipeline)
    b = _case(orc, f"distinct_{max_len}_r{max_rounds}")
    box = _box_for(dev, b)
    box.load(b)
    hf._lib.update_batch(b.ctype, box.rec, b.n, b.max_len, mode=mode, stream=torch.cuda.current_stream())
    rec0, arena0, _ = box.fetch(b.n)
    rec1 = _run_and_check(hf, box, b, mode, "ordered")
    _, arena1, info = box.fetch(b.n)
    _same_records(rec1, rec0, "ordered vs update_batch")
    _same_arena(arena1, arena0, b, "ordered vs update_batch")
    assert info == [1, 0]
    assert {oc.OK, oc.INVALID_ARG} <= set(int(s) for s in rec1["status"])


# ---- 2. chains -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_chains_match_the_sequential_oracle(hf, orc, dev, opts, mode, max_len, pipeline):
    """64 IOs over 8 chunks, 1..12 deep, interleaved: overwrite, append, gap, truncate, extend, full
    overwrite and NONE-typed writes, every IO starting from what its predecessor left."""
    _set_pipeline(opts, pipeline)
    b = _case(orc, f"chains_{max_len}")
    _run_and_check(hf, _box_for(dev, b), b, mode, b.name)


# ---- 3. failures mid-chain -----------------------------------------------------------------------
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_failed_ios_leave_no_trace_in_their_chain(hf, orc, dev, mode, max_len):
    """A corrupted client checksum (4080) and INVALID_ARG IOs with successors: the successors
    start from the untouched state, the chunk bytes show nothing of the failed IOs."""
    b = _case(orc, f"failures_{max_len}")
    rec = _run_and_check(hf, _box_for(dev, b), b, mode, b.name)
    assert {oc.CHECKSUM_MISMATCH, oc.INVALID_ARG, oc.OK} == set(int(s) for s in rec["status"])


# ---- 4. depth overflow ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_depth_overflow_and_resubmission(hf, orc, dev, mode, max_len):
    """Chains of 5 under max_rounds 3: ranks 0-2 applied, ranks 3-4 NOT_APPLIED with case 0 and
    the state after rank 2, d_info == [5, 2 x chains]; the NOT_APPLIED records resubmitted
    unchanged reach the model's final state."""
    b = _case(orc, f"overflow_{max_len}")
    box = _box_for(dev, b)
    rec = _run_and_check(hf, box, b, mode, b.name)
    late = np.flatnonzero(rec["status"] == oc.NOT_APPLIED)
    assert late.size == 2 * b.n_chunks == b.info[1] and list(late) == b.again.idx
    assert not rec["checksum_case"][late].any()
    again = np.ascontiguousarray(rec[late])
    box.send(again)
    _ordered(hf, box, b, mode, n=again.size)
    rec2, arena2, info2 = box.fetch(again.size)
    _same_records(rec2, oc.expected_records(b, again, b.again.expect), "resubmitted")
    _same_arena(arena2, b.again.arena1, b, "resubmitted")
    assert info2 == [2, 0]


# ---- 5. one chunk takes everything ---------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_one_chunk_takes_all_64_ios(hf, orc, dev, mode):
    b = _case(orc, "one_chunk")
    _run_and_check(hf, _box_for(dev, b), b, mode, b.name)


# ---- 6. engine flag --------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["fused", "unfused"])
@pytest.mark.parametrize("mode", MODES)
def test_engine_flag_chains(hf, orc, dev, opts, mode, pipeline):
    """16 sequential 8 KiB appends and a truncate per chunk with HF3FS_UPDATE_FLAG_ENGINE, against
    oracle.engine_apply applied sequentially."""
    opts("update_pipeline", pipeline)
    b = _case(orc, "engine")
    _run_and_check(hf, _box_for(dev, b), b, mode, b.name)


# ---- 7. table stress -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_table_stress_is_exact_and_deterministic(hf, orc, dev, mode):
    """4096 IOs on 1024 chunks of 512 B at consecutive addresses, 4 deep, shuffled: exact, and the
    same records and bytes in a second run."""
    b = _case(orc, "table_stress")
    box = _box_for(dev, b)
    rec1 = _run_and_check(hf, box, b, mode, "first run")
    rec2 = _run_and_check(hf, box, b, mode, "second run")
    assert rec1.tobytes() == rec2.tobytes()


# ---- 8. poison -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("mode", MODES)
def test_chains_under_poisoned_scratch(hf, orc, dev, opts, mode, pipeline):
    """Every scratch word the call reads it wrote first: the chains case with the scratch filled
    with 0xA5A5A5A5, then 0xFFFFFFFF, then not at all."""
    _set_pipeline(opts, pipeline)
    b = _case(orc, f"chains_{128 << 10}")
    box = _box_for(dev, b)
    for pattern in (0xA5A5A5A5, 0xFFFFFFFF, 0):
        opts("poison", pattern)
        _run_and_check(hf, box, b, mode, f"poison {pattern:#x}")


# ---- 9. capture ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["fused", "oneshot"])
@pytest.mark.parametrize("mode", MODES)
def test_captured_call_replans_at_every_replay(hf, orc, dev, opts, mode, pipeline):
    """One captured call (n = 64, max_rounds 4) replayed on two batches that group the chunks
    differently: ranking happens in kernels, from what d_ios holds at replay time.  After the graph
    is destroyed and release_graph_scratch is called nothing of it is live."""
    _set_pipeline(opts, pipeline)
    L = hf._lib
    a, b = _case(orc, "capture_a"), _case(orc, "capture_b")
    box = _box_for(dev, a, b)
    L.release_graph_scratch()
    base = L.graph_scratch_stats()
    box.load(a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        _ordered(hf, box, a, mode, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    owned = L.graph_scratch_stats()
    assert owned["live"] > base["live"]
    for case in (a, b, a):
        sent = box.load(case)
        g.replay()
        rec, arena, info = box.fetch(case.n)
        _same_records(rec, oc.expected_records(case, sent), f"replay of {case.name}")
        _same_arena(arena, case.arena1, case, f"replay of {case.name}")
        assert tuple(info) == case.info
    del g
    torch.cuda.synchronize()
    L.release_graph_scratch()
    end = L.graph_scratch_stats()
    assert end["live"] == base["live"] and end["live_bytes"] == base["live_bytes"] and end["dead"] == 0, (base, end)


_CHILD = r"""
import importlib, hashlib, json, sys
import numpy as np, torch
repo, tests, path, mode = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
sys.path[:0] = [repo, tests]
import update_footprint as fp
hf = importlib.import_module("3fs_amd")
z = np.load(path)
dev = torch.device("cuda:0")
raw = torch.empty(z["arena"].size + 16384, dtype=torch.uint8, device=dev)
lift = (-raw.data_ptr()) % 16384
arena = raw[lift:lift + z["arena"].size]
arena.copy_(torch.from_numpy(z["arena"]).to(dev))
pay = torch.from_numpy(z["pay"]).to(dev)
rec = z["rec"].copy()
rec["chunk"] += np.uint64(arena.data_ptr())
rec["payload"][z["has_payload"]] += np.uint64(pay.data_ptr())
n = rec.size
d_ios = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
info = torch.full((2,), 0x7777, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library call, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            hf._lib.update_ordered(hf.CRC32C, d_ios, n, int(z["max_len"]), int(z["max_rounds"]), mode=mode, info=info,
                                   stream=torch.cuda.current_stream())
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "update_ordered failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
print(json.dumps({"rec_sha256": hashlib.sha256(d_ios.cpu().numpy().tobytes()).hexdigest(),
                  "status": np.frombuffer(d_ios.cpu().numpy().tobytes(), dtype=fp.REC)["status"].tolist(),
                  "info": info.cpu().numpy().tolist(),
                  "arena_sha256": hashlib.sha256(arena.cpu().numpy().tobytes()).hexdigest(),
                  "arena_ptr": int(arena.data_ptr()), "pay_ptr": int(pay.data_ptr())}))
"""


def test_first_call_in_process_is_a_captured_ordered_call(orc, tmp_path):
    """A fresh process whose first library call is a DELTA update_ordered (three-pass pipeline,
    one-shot apply in round 0) inside torch.cuda.graph(capture_error_mode="global"); the child
    replays the graph once and reports digests of the records and the arena."""
    b = _case(orc, "capture_a")
    path = str(tmp_path / "inputs.npz")
    np.savez(path, arena=b.arena0, pay=b.pay, rec=b.rec, has_payload=b.has_payload, max_len=b.max_len,
             max_rounds=b.max_rounds)
    env = dict(os.environ, HF3FS_CRC_UPDATE_PIPELINE="unfused", HF3FS_CRC_APPLY_GRID="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, REPO, os.path.join(REPO, "tests"), path, "1"],
                       capture_output=True, text=True, timeout=150, env=env, cwd=REPO)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    got = lines[0]
    assert got["status"] == [e[0] for e in b.expect]
    want = oc.expected_records(b, oc.record_array(b, got["arena_ptr"], got["pay_ptr"]))
    assert got["rec_sha256"] == hashlib.sha256(want.tobytes()).hexdigest()
    assert got["arena_sha256"] == hashlib.sha256(b.arena1.tobytes()).hexdigest()
    assert tuple(got["info"]) == b.info


# ---- 10. neighbourly -------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("mode", MODES)
def test_plain_update_batch_after_an_ordered_call(hf, orc, dev, opts, mode, pipeline):
    """On one stream and thread: an ordered call, then a plain hf3fs_crc_update_batch (exact), then
    hf3fs_crc_release_stream."""
    _set_pipeline(opts, pipeline)
    L = hf._lib
    c, d = _case(orc, f"chains_{128 << 10}"), _case(orc, f"distinct_{128 << 10}_r1")
    s = torch.cuda.Stream(dev)
    bc_, bd = _box_for(dev, c), _box_for(dev, d)
    sent_c, sent_d = bc_.load(c), bd.load(d)
    with torch.cuda.stream(s):
        _ordered(hf, bc_, c, mode, stream=s)
        L.update_batch(d.ctype, bd.rec, d.n, d.max_len, mode=mode, stream=s)
    rec_c, arena_c, _ = bc_.fetch(c.n)
    rec_d, arena_d, _ = bd.fetch(d.n)
    _same_records(rec_c, oc.expected_records(c, sent_c), "ordered")
    _same_arena(arena_c, c.arena1, c, "ordered")
    want_d = oc.expected_records(d, sent_d)
    for f in ("chunk_size", "chunk_checksum_type", "chunk_checksum"):
        want_d[f] = sent_d[f]  # (update_batch rewrites no input field)
    _same_records(rec_d, want_d, "update_batch after ordered")
    _same_arena(arena_d, d.arena1, d, "update_batch after ordered")
    L.release_stream(s)


# ---- 11. pre-sized scratch ---------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("mode", MODES)
def test_largest_call_first_means_no_later_growth(hf, orc, dev, opts, mode, pipeline):
    """After one call of the largest (n, max_len, max_rounds) the pair's buffer holds at least
    update_ordered_scratch_bytes of every smaller shape, and smaller calls in the same mode --
    whichever apply their first round takes -- allocate nothing (hf3fs_crc_pair_scratch_stats)."""
    _set_pipeline(opts, pipeline)
    if pipeline == "oneshot":
        opts("apply_grid", -1)  # auto: the first call is ticketed, later ones one-shot
    L = hf._lib
    big, small = _case(orc, f"chains_{128 << 10}"), _case(orc, "chains_512")
    tiny = _case(orc, f"failures_{128 << 10}")
    s = torch.cuda.Stream(dev)
    boxes = {x.name: _box_for(dev, x) for x in (big, small, tiny)}
    sent = {x.name: boxes[x.name].load(x) for x in (big, small, tiny)}
    need = L.update_ordered_scratch_bytes(big.n, big.max_len, big.max_rounds, mode=mode)
    assert need > 0
    with torch.cuda.stream(s):
        _ordered(hf, boxes[big.name], big, mode, stream=s)
        s.synchronize()
        first = L.pair_scratch_stats(s)
        assert first["call_bytes"] >= need
        for x in (big, tiny, small, big):
            assert L.update_ordered_scratch_bytes(x.n, x.max_len, x.max_rounds, mode=mode) <= need
            sent[x.name] = boxes[x.name].load(x)
            _ordered(hf, boxes[x.name], x, mode, stream=s)
            rec, arena, info = boxes[x.name].fetch(x.n)
            _same_records(rec, oc.expected_records(x, sent[x.name]), x.name)
            _same_arena(arena, x.arena1, x, x.name)
        after = L.pair_scratch_stats(s)
    assert after == first, (first, after)
    L.release_stream(s)
