"""hf3fs_crc_update_versioned on the GPU: update_ordered with the reference's version ladder and
commit jobs.

Every expectation comes from tests/versioned_cases.py: ChunkReplica::update's admission ladder and
ChunkReplica::commit transcribed from the reference and applied one job at a time in index order,
bytes and checksums from the oracle.  After every call the WHOLE d_ios array, the WHOLE d_ver
array, d_info and the WHOLE chunk arena, canary guards included, must equal the model's.  Chunk
sizes are the reference's own test sizes, 512 B and 128 KiB.
"""
import functools

import numpy as np
import pytest

import ordered_cases as oc
import update_footprint as fp
import versioned_cases as vc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
LINE = 16 << 10
MODES = [0, 1]
SIZES = list(vc.SIZES)
PIPELINES = ["fused", "ticketed", "oneshot"]
INFO_FILL = 0x7777


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(orc, name):
    """Built once and shared by every test and variant; never modified."""
    b = vc.all_cases(orc)[name]()
    for a in (b.rec, b.ver, b.pay, b.arena0, b.arena1):
        a.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _ordered_case(orc, name):
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
    """Device images of one case: the arena on a 16 KiB line, the payloads, both record arrays, d_info."""

    def __init__(self, dev, arena_size, pay_size, n):
        self.dev = dev
        raw = torch.empty(arena_size + LINE, dtype=torch.uint8, device=dev)
        lift = (-raw.data_ptr()) % LINE
        self.raw, self.arena = raw, raw[lift:lift + arena_size]
        self.pay = torch.empty(pay_size, dtype=torch.uint8, device=dev)
        self.rec = torch.empty(n * fp.REC.itemsize, dtype=torch.uint8, device=dev)
        self.ver = torch.empty(n * vc.VER.itemsize, dtype=torch.uint8, device=dev)
        self.info = torch.full((vc.INFO_WORDS,), INFO_FILL, dtype=torch.int32, device=dev)

    def _up(self, a):
        return torch.from_numpy(np.array(a)).to(self.dev)

    def load(self, b):
        """Arena, payloads and the records with absolute addresses -> the record array as sent."""
        self.arena[:b.arena0.size].copy_(self._up(b.arena0))
        self.pay[:b.pay.size].copy_(self._up(b.pay))
        rec = b.rec.copy()
        rec["chunk"] += np.uint64(self.arena.data_ptr())
        rec["payload"][b.has_payload] += np.uint64(self.pay.data_ptr())
        return rec

    def send(self, rec, ver=None):
        self.rec[:rec.size * fp.REC.itemsize].copy_(self._up(rec.view(np.uint8)))
        if ver is not None:
            self.ver[:ver.size * vc.VER.itemsize].copy_(self._up(ver.view(np.uint8)))
        self.info.fill_(INFO_FILL)
        torch.cuda.synchronize()

    def fetch(self, n, arena_size):
        torch.cuda.synchronize()
        rec = np.frombuffer(self.rec.cpu().numpy().tobytes()[:n * fp.REC.itemsize], dtype=fp.REC)
        ver = np.frombuffer(self.ver.cpu().numpy().tobytes()[:n * vc.VER.itemsize], dtype=vc.VER)
        return rec, ver, self.arena[:arena_size].cpu().numpy(), tuple(int(x) for x in self.info.cpu().numpy())


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
    c = max(0, int(np.searchsorted(b.bases, pos, side="right")) - 1)
    pytest.fail(f"{what}: arena differs at {pos} (chunk {c} base {b.bases[c]} + {pos - b.bases[c]}, "
                f"max_len {b.max_len}): got {got[pos]}, want {want[pos]}")


def _versioned(hf, box, b, mode, n=None, ver=True, max_rounds=None, stream=None):
    hf.update_versioned(b.ctype, box.rec, box.ver if ver else None, b.n if n is None else n, b.max_len,
                        b.max_rounds if max_rounds is None else max_rounds, mode=mode, info=box.info,
                        stream=stream or torch.cuda.current_stream())


def _check(box, b, sent_rec, sent_ver, expect, info, arena1, what):
    rec, ver, arena, got_info = box.fetch(sent_rec.size, b.arena0.size)
    want_rec, want_ver = vc.expected(sent_rec, sent_ver, expect)
    _same(rec, want_rec, fp.REC, f"{what}: d_ios")
    _same(ver, want_ver, vc.VER, f"{what}: d_ver")
    _same_arena(arena, arena1, b, what)
    assert got_info == tuple(info), what
    assert bytes(box.pay[:b.pay.size].cpu().numpy()) == b.pay.tobytes(), f"{what}: a payload byte changed"
    return rec, ver


def _run_and_check(hf, box, b, mode, what):
    sent = box.load(b)
    box.send(sent, b.ver)
    _versioned(hf, box, b, mode)
    return _check(box, b, sent, b.ver, b.expect, b.info, b.arena1, what)


# ---- 1. without version records the call is update_ordered ------------------------------------------
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_null_ver_is_update_ordered_byte_for_byte(hf, orc, dev, mode, max_len):
    """d_ver == NULL on the chains case: records, arena and the two words of d_info are what
    hf3fs_crc_update_ordered leaves from the same start; the other six words are not touched."""
    b = _ordered_case(orc, f"chains_{max_len}")
    box = _box_for(dev, b)
    sent = box.load(b)
    box.send(sent)
    hf.update_ordered(b.ctype, box.rec, b.n, b.max_len, b.max_rounds, mode=mode, info=box.info,
                      stream=torch.cuda.current_stream())
    rec0, _, arena0, info0 = box.fetch(b.n, b.arena0.size)
    _same(rec0, oc.expected_records(b, sent), fp.REC, "update_ordered")
    assert box.load(b).tobytes() == sent.tobytes()
    box.send(sent)
    _versioned(hf, box, b, mode, ver=False)
    rec1, _, arena1, info1 = box.fetch(b.n, b.arena0.size)
    _same(rec1, rec0, fp.REC, "versioned(NULL) vs update_ordered")
    _same_arena(arena1, arena0, b, "versioned(NULL) vs update_ordered")
    assert info1 == info0 == b.info + (INFO_FILL,) * 6


# ---- 2. records that admit everything ------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_admit_all_records_equal_update_ordered(hf, orc, dev, opts, mode, max_len, pipeline):
    """CLEAN chunks and io_ver = update_ver + 1 down each chain: d_ios and the arena are
    update_ordered's byte for byte (and the oracle's), d_ver walks the versions."""
    _set_pipeline(opts, pipeline)
    b = _ordered_case(orc, f"chains_{max_len}")
    box = _box_for(dev, b)
    sent = box.load(b)
    box.send(sent)
    hf.update_ordered(b.ctype, box.rec, b.n, b.max_len, b.max_rounds, mode=mode, info=box.info,
                      stream=torch.cuda.current_stream())
    rec0, _, arena0, _ = box.fetch(b.n, b.arena0.size)
    ver, want_ver, tail = vc.admit_all(b)
    box.load(b)
    box.send(sent, ver)
    _versioned(hf, box, b, mode)
    rec1, ver1, arena1, info = box.fetch(b.n, b.arena0.size)
    _same(rec1, rec0, fp.REC, "versioned vs update_ordered")
    _same(rec1, oc.expected_records(b, sent), fp.REC, "versioned vs the oracle")
    _same_arena(arena1, arena0, b, "versioned vs update_ordered")
    _same_arena(arena1, b.arena1, b, "versioned vs the oracle")
    _same(ver1, want_ver, vc.VER, "d_ver")
    assert info == b.info + tail


# ---- 3. every status code, and what goes first ----------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_every_status_code_and_the_precedence_pairs(hf, orc, dev, opts, mode, max_len, pipeline):
    """One job per chunk: each rung of both ladders, 4015 over 4005, 4005 over a low chain version,
    4081 over a bad payload, a bad payload over 4008 / 4006 / 4007 / 4012 and the ladder's code for a
    good one.  Refused jobs leave the arena identical (the model's arena shows only the applied)."""
    _set_pipeline(opts, pipeline)
    b = _case(orc, f"singles_{max_len}")
    rec, _ = _run_and_check(hf, _box_for(dev, b), b, mode, b.name)
    got = dict(zip(b.tags, (int(s) for s in rec["status"])))
    assert {got[t] for t in got if t[0] in "up"} == set(vc.UPDATE_CODES)
    assert {got[t] for t in got if t[0] == "c"} == set(vc.COMMIT_CODES)
    refused = [c for c, e in enumerate(b.expect) if e[0] != vc.OK]
    for c in refused:
        x = b.bases[c]
        assert b.arena1[x:x + max_len].tobytes() == b.arena0[x:x + max_len].tobytes()


# ---- 4. the queues the ladder exists for ------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_lost_predecessors_duplicates_head_and_commits(hf, orc, dev, opts, mode, max_len, pipeline):
    """Eight interleaved chains: bad v+1 then v+2 (4080, 4007); a duplicate io_ver (4006; with the
    commit between, 4008); the head's write / commit ladder eight deep and without its first commit
    (4012); forced and partial commits; a syncing write on a DIRTY recycling chunk; ENGINE, REMOVE
    and a commit on a recycling chunk between valid neighbours."""
    _set_pipeline(opts, pipeline)
    b = _case(orc, f"pairs_{max_len}")
    _run_and_check(hf, _box_for(dev, b), b, mode, b.name)


@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_v2_behind_a_bad_v1_is_refused_where_update_ordered_applies_it(hf, orc, dev, mode, max_len):
    """A write with updateVer v+2 queued behind a v+1 whose payload fails its checksum: the
    reference answers kChunkMissingUpdate and the chunk stays as it was.  The same two records
    through hf3fs_crc_update_ordered apply the second write."""
    q = max(8, max_len // 16)
    b = vc.build(orc, "lost_predecessor", 1, max_len, 4, [vc.W(0, 0, q, 5, flavour="corrupt"), vc.W(0, q, q, 6)],
                 0x1057)
    box = _box_for(dev, b)
    rec, ver = _run_and_check(hf, box, b, mode, b.name)
    assert [int(s) for s in rec["status"]] == [vc.CHECKSUM_MISMATCH, vc.MISSING_UPDATE]
    assert b.arena1.tobytes() == b.arena0.tobytes() and int(ver["out_update_ver"][1]) == 4
    sent = box.load(b)
    box.send(sent)
    hf.update_ordered(b.ctype, box.rec, b.n, b.max_len, b.max_rounds, mode=mode,
                      stream=torch.cuda.current_stream())
    rec0, _, arena0, _ = box.fetch(b.n, b.arena0.size)
    assert [int(s) for s in rec0["status"]] == [vc.CHECKSUM_MISMATCH, vc.OK]
    x = b.bases[0]
    assert arena0[x + q:x + 2 * q].tobytes() == b.jobs[1]["data"]


# ---- 5. depth overflow --------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_depth_overflow_and_resubmission(hf, orc, dev, mode, max_len):
    """Chains of 5 under max_rounds 3: the NOT_APPLIED jobs carry the chunk's state after its last
    applied job in both arrays; resubmitted unchanged they reach the model's end state."""
    b = _case(orc, f"overflow_{max_len}")
    box = _box_for(dev, b)
    rec, ver = _run_and_check(hf, box, b, mode, b.name)
    late = np.flatnonzero(rec["status"] == vc.NOT_APPLIED)
    assert list(late) == b.again.idx
    again_rec, again_ver = np.ascontiguousarray(rec[late]), np.ascontiguousarray(ver[late])
    box.send(again_rec, again_ver)
    _versioned(hf, box, b, mode, n=late.size)
    _check(box, b, again_rec, again_ver, b.again.expect, b.again.info, b.again.arena1, "resubmitted")


# ---- 6. random queues -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("seed", vc.SEEDS)
@pytest.mark.parametrize("max_len", SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_random_queues(hf, orc, dev, opts, mode, max_len, seed, pipeline):
    """64 chunks, up to 8 jobs each, every job kind and both payload verdicts."""
    _set_pipeline(opts, pipeline)
    b = _case(orc, f"random_{max_len}_{seed:x}")
    _run_and_check(hf, _box_for(dev, b), b, mode, b.name)


# ---- 7. one chunk takes everything ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_one_chunk_takes_64_jobs(hf, orc, dev, mode):
    b = _case(orc, "one_chunk")
    _run_and_check(hf, _box_for(dev, b), b, mode, b.name)


# ---- 8. poison ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("mode", MODES)
def test_random_queue_under_poisoned_scratch(hf, orc, dev, opts, mode, pipeline):
    """Every scratch word the call reads it wrote first: scratch filled with 0xA5A5A5A5, then
    0xFFFFFFFF, then not at all."""
    _set_pipeline(opts, pipeline)
    b = _case(orc, f"random_{128 << 10}_{vc.SEEDS[0]:x}")
    p = _case(orc, f"pairs_{128 << 10}")
    box = _box_for(dev, b, p)
    for pattern in (0xA5A5A5A5, 0xFFFFFFFF, 0):
        opts("poison", pattern)
        _run_and_check(hf, box, b, mode, f"poison {pattern:#x}")
        _run_and_check(hf, box, p, mode, f"poison {pattern:#x} (pairs)")


# ---- 9. capture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["fused", "oneshot"])
@pytest.mark.parametrize("mode", MODES)
def test_captured_call_replans_after_the_records_were_rewritten(hf, orc, dev, opts, mode, pipeline):
    """One captured call replayed on two queues of the same shape whose records differ in grouping,
    versions and payload verdicts: ranking, the ladders and the deferred verify all run in kernels,
    from what d_ios and d_ver hold at replay time."""
    _set_pipeline(opts, pipeline)
    L = hf._lib
    a, b = _case(orc, "capture_a"), _case(orc, "capture_b")
    box = _box_for(dev, a, b)
    L.release_graph_scratch()
    base = L.graph_scratch_stats()
    box.send(box.load(a), a.ver)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        _versioned(hf, box, a, mode, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    for case in (a, b, a):
        sent = box.load(case)
        box.send(sent, case.ver)
        g.replay()
        _check(box, case, sent, case.ver, case.expect, case.info, case.arena1, f"replay of {case.name}")
    del g
    torch.cuda.synchronize()
    L.release_graph_scratch()
    end = L.graph_scratch_stats()
    assert end["live"] == base["live"] and end["live_bytes"] == base["live_bytes"] and end["dead"] == 0, (base, end)


# ---- 10. scratch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_scratch_bytes_cover_the_call(hf, orc, dev, mode):
    """After one call the pair's buffer holds update_versioned_scratch_bytes, which exceeds the
    ordered call's by the version arrays, and a second call allocates nothing."""
    L = hf._lib
    b = _case(orc, f"pairs_{128 << 10}")
    box = _box_for(dev, b)
    s = torch.cuda.Stream(dev)
    need = L.update_versioned_scratch_bytes(b.n, b.max_len, b.max_rounds, mode=mode)
    assert need > L.update_ordered_scratch_bytes(b.n, b.max_len, b.max_rounds, mode=mode) > 0
    assert L.update_versioned_scratch_bytes(b.n, b.max_len, 65, mode=mode) == 0
    with torch.cuda.stream(s):
        for k in range(2):
            sent = box.load(b)
            box.send(sent, b.ver)
            _versioned(hf, box, b, mode, stream=s)
            _check(box, b, sent, b.ver, b.expect, b.info, b.arena1, f"call {k}")
            stats = L.pair_scratch_stats(s)
            if k == 0:
                first = stats
                assert first["call_bytes"] >= need
    assert stats == first
    L.release_stream(s)
