"""Every batch entry point in the three settings include/hf3fs_crc.h promises and the parity suite
only checks for update_batch and verify_blocks (cases, oracle references and the schedule model
are in tests/batch_cases.py):

  test_switch            each case eagerly at default switches and under every applicable row of
                         SWITCHES, one row at a time; the schedule the model expects at this
                         device's CU count must be the one the row declares.
  test_poisoned_scratch  after a twice-as-large call of the same entry point left a stale pair
                         buffer behind, the case runs with every library scratch word pre-filled
                         with a pattern: a word read before it is written shows as a wrong result.
  test_captured_replay   the case is the (stream, thread) pair's first call, captured into a
                         graph; it is replayed over inputs rewritten in place (what the device
                         must decide anew on every replay: segment counts from the device-side
                         length bound, the frames' route, the all-empty shortcut), after
                         release_stream and a larger eager call regrew the pair buffer, and its
                         memory is accounted for when the graph goes.

All comparisons are bit-exact against the oracle; every output holds a sentinel before each call
or replay."""
import copy
import zlib

import numpy as np
import pytest

import batch_cases as bc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
PATTERNS = [0xFFFFFFFF, 0xA5A5A5A5, 0x00000001]
ROWS = {bc.switch_key(row): row for row in [()] + list(bc.SWITCHES)}
LIST_RUNS = "list_runs=1,prehash_rep=1"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


_TIMELINES = {}


def timeline(name, cus, scale=1):
    """[(inputs, reference)]: the case as built, then after each of its mutations in turn.  Computed
    once per module and never changed (every user gets the same arrays and must not write them)."""
    key = (name, cus, scale)
    if key not in _TIMELINES:
        case = bc.CASES[name]
        rng = np.random.default_rng(zlib.crc32(name.encode()) + 1000 * scale)
        inp = case.build(cus, rng, scale)
        steps = [(copy.deepcopy(inp), case.reference(inp))]
        if scale == 1:
            for _mname, fn in case.mutations:
                fn(inp, rng)
                steps.append((copy.deepcopy(inp), case.reference(inp)))
        _TIMELINES[key] = steps
    return _TIMELINES[key]


class OnDevice:
    """The case's arena and buffers as device tensors at fixed addresses; load() rewrites them in
    place from host inputs and puts the sentinel back into every output."""

    def __init__(self, case, inp, dev):
        self.case, self.base, self.arena = case, 0, None
        if "arena" in inp:
            self.store = torch.empty(inp["arena"].size + 1024, dtype=torch.uint8, device=dev)
            pad = (-self.store.data_ptr()) % 1024  # the cases count residues from a 1 KiB boundary
            self.arena = self.store[pad:pad + inp["arena"].size]
            self.base = self.arena.data_ptr()
        images = case.buffers(inp, self.base)
        self.bufs = {k: torch.empty(a.nbytes, dtype=torch.uint8, device=dev) for k, a in images.items()}
        self.load(inp, images)

    def load(self, inp, images=None):
        images = images if images is not None else self.case.buffers(inp, self.base)
        if self.arena is not None:
            self.arena.copy_(torch.from_numpy(inp["arena"]))
        assert images.keys() == self.bufs.keys()
        self.dtypes = {k: a.dtype for k, a in images.items()}
        for k, a in images.items():
            assert a.nbytes == self.bufs[k].numel(), k
            self.bufs[k].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)))
        torch.cuda.synchronize()

    def run(self, L, inp, stream):
        p = {k: t.data_ptr() for k, t in self.bufs.items()}
        p["arena"] = self.base
        self.case.call(L, inp, p, stream)

    def results(self, inp):
        host = {k: t.cpu().numpy().view(self.dtypes[k]) for k, t in self.bufs.items()}
        return self.case.extract(inp, host)


def check(dv, inp, ref, what):
    got = dv.results(inp)
    assert got.keys() == ref.keys(), what
    for k, want in ref.items():
        if not np.array_equal(got[k], want):
            bad = np.flatnonzero(got[k] != want)[:5]
            pytest.fail(f"{what}: {k} differs at {np.count_nonzero(got[k] != want)} of {want.size}: "
                        f"first {bad.tolist()}, got {got[k][bad].tolist()}, want {want[bad].tolist()}")


# ---- a. every switch -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key", list(bc.LABELS), ids=[f"{n}-{k}" for n, k in bc.LABELS])
def test_switch(hf, opts, dev, cus, name, key):
    L, case = hf._lib, bc.CASES[name]
    inp, ref = timeline(name, cus)[0]
    row = ROWS[key]
    assert bc.case_label(case, inp, cus, dict(row)) == bc.LABELS[(name, key)], \
        f"{name} under {key} slipped to another schedule at {cus} CUs"
    for k, v in row:
        opts(k, v)
    dv = OnDevice(case, inp, dev)
    dv.run(L, inp, torch.cuda.current_stream())
    torch.cuda.synchronize()
    check(dv, inp, ref, f"{name} [{key}]")


# ---- b. poisoned scratch ---------------------------------------------------------------------------
POISONED = [(c.name, "default") for c in bc.CASES.values() if c.poisoned] + \
    [(n, LIST_RUNS) for n in bc.SWITCHES[ROWS[LIST_RUNS]]["cases"] if n.startswith("create_list")]


@pytest.mark.parametrize("pattern", PATTERNS, ids=[f"{p:08x}" for p in PATTERNS])
@pytest.mark.parametrize("name,key", POISONED, ids=[n if k == "default" else f"{n}-{k}" for n, k in POISONED])
def test_poisoned_scratch(hf, opts, dev, cus, name, key, pattern):
    L, case = hf._lib, bc.CASES[name]
    inp, ref = timeline(name, cus)[0]
    big, big_ref = timeline(name, cus, 2)[0]
    for k, v in ROWS[key]:
        opts(k, v)
    assert any(bc.library_memory(s, cus, dict(ROWS[key])) - {"counter"} for s in case.shapes(inp)), \
        "the case takes no library memory that is poisoned"
    s = torch.cuda.current_stream()
    if case.records:
        L.anomalies(0, reset=True)
    stale = OnDevice(case, big, dev)  # twice the records, other data: a larger, stale pair buffer
    stale.run(L, big, s)
    torch.cuda.synchronize()
    check(stale, big, big_ref, f"{name} x2")
    dv = OnDevice(case, inp, dev)
    opts("poison", pattern)
    dv.run(L, inp, s)
    torch.cuda.synchronize()
    opts("poison", 0)
    check(dv, inp, ref, f"{name} on scratch poisoned with {pattern:#x}")
    if case.records:
        a = L.anomalies(0)
        assert a["count"] == 0 and a["kinds"] == 0, a


# ---- c. captured and replayed ----------------------------------------------------------------------
CAPTURED = [(n, False) for n in bc.CASES] + [(n, True) for n in (
    "frames_walked", "frames_gaps", "frames_big", "read_result",
    "create_list_small_many_balanced", "verify_blocks_scratch")]  # (the last two: a poisoned balance region)


@pytest.mark.parametrize("name,poison", CAPTURED, ids=[n + ("-poisoned" if p else "") for n, p in CAPTURED])
def test_captured_replay(hf, opts, dev, cus, name, poison):
    L, case = hf._lib, bc.CASES[name]
    steps = timeline(name, cus)
    inp0, ref0 = steps[0]
    big, big_ref = timeline(name, cus, 2)[0]
    takes_memory = any(bc.library_memory(s, cus) for s in case.shapes(inp0))
    L.release_graph_scratch()
    base = L.graph_scratch_stats()
    cs = torch.cuda.Stream(dev)  # no eager call on it: the pair's first call is the captured one
    dv = OnDevice(case, inp0, dev)
    if poison:
        opts("poison", 0xA5A5A5A5)  # the fill is captured too: every replay starts from poison
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        dv.run(L, inp0, cs)
    if poison:
        opts("poison", 0)
    torch.cuda.synchronize()
    owned = L.graph_scratch_stats()
    if takes_memory:
        assert owned["live"] > base["live"] and owned["live_bytes"] > base["live_bytes"], (base, owned)
    g.replay()
    torch.cuda.synchronize()
    check(dv, inp0, ref0, f"{name}: first replay")
    for (mname, _fn), (inp, ref) in zip(case.mutations, steps[1:]):
        dv.load(inp)  # in place: the captured addresses, the outputs back at the sentinel
        g.replay()
        torch.cuda.synchronize()
        check(dv, inp, ref, f"{name}: replay after mutation {mname}")
    L.release_stream(cs)  # the pair's buffers go; a larger eager call regrows them
    other = OnDevice(case, big, dev)
    with torch.cuda.stream(cs):
        other.run(L, big, cs)
    cs.synchronize()
    check(other, big, big_ref, f"{name} x2 on the capture stream")
    dv.load(inp0)
    g.replay()
    torch.cuda.synchronize()
    check(dv, inp0, ref0, f"{name}: replay after release_stream and a larger eager call")
    del g
    torch.cuda.synchronize()
    gone = L.graph_scratch_stats()
    if takes_memory:
        assert gone["dead"] >= 1, (owned, gone)
    L.release_graph_scratch()
    end = L.graph_scratch_stats()
    assert end["dead"] == 0 and end["live"] == base["live"], (base, end)
    L.release_stream(cs)
