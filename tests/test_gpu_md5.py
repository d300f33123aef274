"""hf3fs_crc_md5_batch on the GPU.

The checker of every digest is hashlib.md5 over the file's bytes (holes as zeros); the states of
calls without FINAL are compared, all 96 bytes, with the pure-Python model of tests/md5_cases.py
(held to hashlib by tests/test_md5_model.py).  Cases are built once and shared; unless a test says
otherwise it runs under the four settings of md5_stage x md5_sort.
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import host_memory as hm
import md5_cases as mc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
CANARY = 0xEE
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]
BOTH = mc.INIT | mc.FINAL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(params=MODES, ids=[f"stage{s}-sort{o}" for s, o in MODES])
def mode(request, opts):
    stage, sort = request.param
    opts("md5_stage", stage)
    opts("md5_sort", sort)
    return request.param


def _u8(dev, array):
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).to(dev)


class OnDevice:
    """An arena in HBM and the records of file lists that point into it."""

    def __init__(self, dev, arena):
        self.dev = dev
        self.arena = _u8(dev, arena)
        self.base = self.arena.data_ptr()
        assert self.base % 16 == 0

    def records(self, files):
        segs, off = mc.records(files, self.base)
        d_segs = _u8(self.dev, segs) if segs.size else None
        return d_segs, _u8(self.dev, off), len(files), int(segs.size)

    def digests(self, hf, files, state=None, flags=BOTH, stream=None):
        """One call -> the 16 n_files output bytes (FINAL), the out buffer's guards checked."""
        d_segs, d_off, n, n_segs = self.records(files)
        out = torch.full((16 * n + 2 * GUARD,), CANARY, dtype=torch.uint8, device=self.dev)
        hf.md5_batch(d_segs, d_off, n, n_segs, out=out.data_ptr() + GUARD, state=state, flags=flags,
                     stream=stream or torch.cuda.current_stream())
        torch.cuda.synchronize()
        raw = out.cpu().numpy()
        assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + 16 * n:] == CANARY).all(), "guard of d_out written"
        return raw[GUARD:GUARD + 16 * n].tobytes()


def _want(contents):
    return b"".join(hashlib.md5(c).digest() for c in contents)


def _compare(got, contents, what):
    want = _want(contents)
    if got != want:
        bad = [i for i in range(len(contents)) if got[16 * i:16 * i + 16] != want[16 * i:16 * i + 16]]
        pytest.fail(f"{what}: {len(bad)} of {len(contents)} digests differ, first files {bad[:8]} "
                    f"(lengths {[len(contents[i]) for i in bad[:8]]})")


@functools.lru_cache(maxsize=None)
def _layout(name, *args):
    """(arena, files, contents), built once and never modified."""
    lay = getattr(mc, name + "_layout")(*args)
    arena = lay.arena()
    arena.setflags(write=False)
    return arena, lay.files, mc.contents(arena, lay.files)


_DEVICE = {}


def _placed(dev, name, *args):
    """The layout's arena on the device, uploaded once for the module."""
    key = (name,) + args
    if key not in _DEVICE:
        _DEVICE[key] = OnDevice(dev, _layout(name, *args)[0])
    return _DEVICE[key]


def _one_shot(hf, dev, name, *args):
    arena, files, contents = _layout(name, *args)
    got = _placed(dev, name, *args).digests(hf, files)
    _compare(got, contents, name)
    return got


# ---- 1-4: vectors, lengths, segmentation, holes ----------------------------------------------------
def test_rfc1321_vectors(hf, dev, mode):
    got = _one_shot(hf, dev, "rfc")
    assert [hf.md5_hex(got[16 * i:16 * i + 16]) for i in range(7)] == [h for _, h in mc.RFC1321]


def test_length_sweep(hf, dev, mode):
    """Every length 0..200 and the 1 KiB / 4 KiB edges, base addresses of every residue mod 16; the
    padding edge 55 / 56 / 63 / 64 / 119 / 120 at every residue."""
    _one_shot(hf, dev, "sweep")


def test_segmentation(hf, dev, mode):
    """300 bytes as two segments cut at every position, and as three with random cuts (empty
    segments among them), every segment somewhere else in the arena at an unaligned address."""
    got = _one_shot(hf, dev, "segmentation")
    assert len(set(got[16 * i:16 * i + 16] for i in range(len(got) // 16))) == 1


def test_holes(hf, dev, mode):
    """Holes of 1, 63, 64, 65 and 5000 bytes first, in the middle and last, hole-only files: the
    MD5 of the zero-filled content."""
    _one_shot(hf, dev, "holes")
    assert any(c == bytes(5000) for c in _layout("holes")[2])


# ---- 5: streaming ----------------------------------------------------------------------------------
def _states(dev, n, fill=0xA5):
    return torch.full((n * 96,), fill, dtype=torch.uint8, device=dev)


@functools.lru_cache(maxsize=None)
def _two_calls(n_bytes):
    """mc.stream_two_calls and the packed model state of every split, computed once."""
    arena, content, first, second = mc.stream_two_calls(n_bytes)
    return arena, content, first, second, b"".join(s.pack() for s in mc.prefix_states(content))


@functools.lru_cache(maxsize=None)
def _four_calls(n_bytes):
    arena, content, calls, cuts = mc.stream_four_calls(n_bytes)
    return arena, content, calls, cuts, [s.pack() for s in mc.prefix_states(content)]


@pytest.mark.parametrize("n_bytes", [130, 4097])
def test_streaming_two_calls_every_split(hf, dev, mode, n_bytes):
    """File k: content[:k] with INIT, then content[k:] with FINAL.  After the first call every
    96-byte state is the model's (tail zero beyond total % 64, reserved 0); the digests are the
    one-shot call's and hashlib's; FINAL leaves the states as they were."""
    arena, content, first, second, want = _two_calls(n_bytes)
    box = OnDevice(dev, arena)
    n = n_bytes + 1
    state = _states(dev, n)
    d_segs, d_off, _, n_segs = box.records(first)
    hf.md5_batch(d_segs, d_off, n, n_segs, state=state, flags=mc.INIT)
    torch.cuda.synchronize()
    got = state.cpu().numpy().tobytes()
    bad = [k for k in range(n) if got[96 * k:96 * k + 96] != want[96 * k:96 * k + 96]]
    assert not bad, f"states of splits {bad[:8]} differ: got {got[96 * bad[0]:96 * bad[0] + 96].hex()}"
    digests = box.digests(hf, second, state=state, flags=mc.FINAL)
    assert digests == hashlib.md5(content).digest() * n
    assert state.cpu().numpy().tobytes() == want, "FINAL changed d_state"
    whole = [[(first[n_bytes][0][0], n_bytes)]]
    assert box.digests(hf, whole) == digests[:16]


@pytest.mark.parametrize("n_bytes", [130, 4097])
def test_streaming_four_calls(hf, dev, mode, n_bytes):
    """INIT, two pure updates, FINAL; calls without bytes, a last call without segments."""
    arena, content, calls, cuts, prefixes = _four_calls(n_bytes)
    box = OnDevice(dev, arena)
    n = len(cuts)
    state = _states(dev, n)
    for k, flags in enumerate((mc.INIT, 0, 0)):
        d_segs, d_off, _, n_segs = box.records(calls[k])
        hf.md5_batch(d_segs, d_off, n, n_segs, state=state, flags=flags)
        torch.cuda.synchronize()
        want = b"".join(prefixes[c[k + 1]] for c in cuts)
        assert state.cpu().numpy().tobytes() == want, f"states after call {k}"
    assert any(not f for f in calls[3]) and any(f for f in calls[3])
    assert box.digests(hf, calls[3], state=state, flags=mc.FINAL) == hashlib.md5(content).digest() * n


def test_final_call_without_any_segment(hf, dev, mode):
    """MD5_Final alone: n_segs == 0 and a null d_segs, the states carry everything."""
    contents = [bytes([i]) * n for i, n in enumerate((0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 1000))]
    state = _u8(dev, np.frombuffer(b"".join(mc.State().update(c).pack() for c in contents), dtype=np.uint8))
    n = len(contents)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    out = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    hf.md5_batch(None, off, n, 0, out=out, state=state, flags=mc.FINAL)
    torch.cuda.synchronize()
    _compare(out.cpu().numpy().tobytes(), contents, "final only")


# ---- 6: ragged batches -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_files", [1, 63, 64, 65, 200, 1000])
def test_ragged_batch(hf, dev, mode, n_files):
    """0 .. 100 KiB files, empty ones, one of 1 MiB + 17 bytes, up to eight segments each: every
    digest lands at its own file's index whatever order the lanes took the files in."""
    _one_shot(hf, dev, "ragged", n_files)


def test_ragged_batch_identical_under_every_setting(hf, dev, opts):
    arena, files, contents = _layout("ragged", 200)
    box = _placed(dev, "ragged", 200)
    got = []
    for stage, sort in MODES:
        opts("md5_stage", stage)
        opts("md5_sort", sort)
        got.append(box.digests(hf, files))
    assert got[0] == got[1] == got[2] == got[3] == _want(contents)


# ---- 7: footprint ----------------------------------------------------------------------------------
def test_footprint(hf, dev, mode):
    """d_out between guards at an aligned and at an odd address; FINAL with a state leaves the states
    alone; a call without FINAL leaves d_out alone; records, offsets and data are never written."""
    arena, files, contents = _layout("sweep")
    box = OnDevice(dev, arena)
    d_segs, d_off, n, n_segs = box.records(files)
    segs0, off0 = d_segs.cpu().numpy().copy(), d_off.cpu().numpy().copy()
    for lead in (GUARD, GUARD + 1, GUARD + 2):
        out = torch.full((16 * n + 2 * GUARD + 8,), CANARY, dtype=torch.uint8, device=dev)
        hf.md5_batch(d_segs, d_off, n, n_segs, out=out.data_ptr() + lead)
        torch.cuda.synchronize()
        raw = out.cpu().numpy()
        assert (raw[:lead] == CANARY).all() and (raw[lead + 16 * n:] == CANARY).all(), lead
        _compare(raw[lead:lead + 16 * n].tobytes(), contents, f"d_out at +{lead}")
    state = _states(dev, n)
    out = torch.full((16 * n,), CANARY, dtype=torch.uint8, device=dev)
    hf.md5_batch(d_segs, d_off, n, n_segs, out=out, state=state, flags=mc.INIT)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all(), "d_out written without FINAL"
    kept = state.cpu().numpy().tobytes()
    assert kept == b"".join(mc.State().update(c).pack() for c in contents)
    off_none = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    hf.md5_batch(None, off_none, n, 0, out=out, state=state, flags=mc.FINAL)
    torch.cuda.synchronize()
    assert state.cpu().numpy().tobytes() == kept, "FINAL wrote d_state"
    _compare(out.cpu().numpy().tobytes(), contents, "finalised")
    assert np.array_equal(d_segs.cpu().numpy(), segs0) and np.array_equal(d_off.cpu().numpy(), off0)
    assert np.array_equal(box.arena.cpu().numpy(), arena)


# ---- 8: poison -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0xFFFFFFFF, 0x00000001, 0xA5A5A5A5])
def test_poisoned_scratch(hf, dev, mode, opts, pattern):
    """Scratch pre-filled with junk: the output is unchanged, so every scratch word read was written
    by the call first."""
    opts("poison", pattern)
    _one_shot(hf, dev, "ragged", 200)


# ---- 9: capture ------------------------------------------------------------------------------------
def test_captured_call_replans_at_every_replay(hf, dev, mode):
    """A captured one-shot call, replayed twice: between the replays the bytes are rewritten and one
    d_file_off entry moves a segment from one file to its neighbour."""
    arena, files, contents = _layout("ragged", 65)
    box = OnDevice(dev, arena)
    d_segs, d_off, n, n_segs = box.records(files)
    out = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        hf.md5_batch(d_segs, d_off, n, n_segs, out=out, stream=torch.cuda.current_stream())
    g.replay()
    torch.cuda.synchronize()
    _compare(out.cpu().numpy().tobytes(), contents, "replay 0")
    arena2 = np.random.default_rng(99).integers(0, 256, arena.size, dtype=np.uint8)
    box.arena.copy_(torch.from_numpy(arena2))
    f = next(i for i in range(1, n - 1) if len(files[i]) >= 2 and files[i][-1][1] > 0)
    files2 = [list(x) for x in files]
    files2[f + 1].insert(0, files2[f].pop())
    _, off2 = mc.records(files2, box.base)
    d_off.copy_(_u8(dev, off2))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    want2 = mc.contents(arena2, files2)
    assert want2[f] != contents[f] and len(want2[f]) != len(mc.contents(arena2, files)[f])
    _compare(out.cpu().numpy().tobytes(), want2, "replay 1")
    del g


_CHILD = r"""
import importlib, json, sys
import numpy as np, torch
repo, tests, path = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path[:0] = [repo, tests]
hf = importlib.import_module("3fs_amd")
z = np.load(path)
dev = torch.device("cuda:0")
arena = torch.from_numpy(z["arena"]).to(dev)
segs = z["segs"].copy()
segs["data"] = np.where(z["hole"], 0, segs["data"] + np.uint64(arena.data_ptr()))
d_segs = torch.from_numpy(segs.view(np.uint8)).to(dev)
d_off = torch.from_numpy(z["off"].view(np.int64)).to(dev)
n = z["off"].size - 1
out = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library call, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            hf.md5_batch(d_segs, d_off, n, int(segs.size), out=out, stream=torch.cuda.current_stream())
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "md5_batch failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
print(json.dumps({"out": out.cpu().numpy().tobytes().hex()}))
"""


def test_md5_first_call_in_process_is_captured(tmp_path):
    """A fresh process whose first library call is an md5_batch inside
    torch.cuda.graph(capture_error_mode="global"): the context and the call's scratch are first
    allocated during the capture.  The child replays the graph once; every digest is exact."""
    arena, files, contents = _layout("ragged", 65)
    segs, off = mc.records(files, 0)
    hole = np.array([o is None for f in files for o, _ in f], dtype=bool)
    path = str(tmp_path / "case.npz")
    np.savez(path, arena=arena, segs=segs, off=off, hole=hole)
    p = subprocess.run([sys.executable, "-c", _CHILD, REPO, os.path.join(REPO, "tests"), path],
                       capture_output=True, text=True, timeout=150, env=dict(os.environ), cwd=REPO)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    _compare(bytes.fromhex(lines[0]["out"]), contents, "first call captured")


# ---- 10: registered host memory --------------------------------------------------------------------
def test_registered_host_memory(hf, dev, mode):
    """The length sweep with data, segment records, offsets and outputs in hf3fs_crc_host_register'ed
    host memory."""
    arena, files, contents = _layout("sweep")
    n = len(files)
    mem = []
    try:
        m_arena = hm.Registered(arena.size, lead=16)
        mem.append(m_arena)
        assert m_arena.dev % 16 == 0
        m_arena.write(arena)
        segs, off = mc.records(files, m_arena.dev)
        m_segs, m_off = hm.Registered(segs.nbytes, lead=8), hm.Registered(off.nbytes, lead=8)
        m_out = hm.Registered(16 * n + 2 * GUARD)
        mem += [m_segs, m_off, m_out]
        m_segs.write(segs.view(np.uint8))
        m_off.write(off.view(np.uint8))
        m_out.write(np.full(16 * n + 2 * GUARD, CANARY, dtype=np.uint8))
        hf.md5_batch(m_segs.dev, m_off.dev, n, int(segs.size), out=m_out.dev + GUARD,
                     stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        raw = m_out.read()
        assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + 16 * n:] == CANARY).all()
        _compare(raw[GUARD:GUARD + 16 * n].tobytes(), contents, "registered memory")
        assert np.array_equal(m_arena.read(), arena) and m_segs.read().tobytes() == segs.tobytes()
    finally:
        torch.cuda.synchronize()
        for m in mem:
            m.close()


# ---- 11: scratch -----------------------------------------------------------------------------------
def test_scratch_does_not_grow_after_the_largest_call(hf, dev):
    L = hf._lib
    st = torch.cuda.Stream(dev)
    arena, files, contents = _layout("ragged", 1000)
    box = _placed(dev, "ragged", 1000)
    with torch.cuda.stream(st):
        _compare(box.digests(hf, files, stream=st), contents, "largest")
        st0 = L.pair_scratch_stats(st)
        assert 0 < st0["call_bytes"] <= L.md5_scratch_bytes(1000)
        for name, args in (("ragged", (200,)), ("ragged", (1,)), ("sweep", ()), ("ragged", (1000,))):
            a, f, c = _layout(name, *args)
            assert L.md5_scratch_bytes(len(f)) <= L.md5_scratch_bytes(1000)
            _compare(_placed(dev, name, *args).digests(hf, f, stream=st), c, "smaller")
        st1 = L.pair_scratch_stats(st)
    assert st1 == st0
    L.release_stream(st)
