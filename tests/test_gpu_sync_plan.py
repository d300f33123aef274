"""hf3fs_crc_sync_plan and hf3fs_crc_sync_scrub_fill on the GPU.

Every expectation comes from tests/sync_cases.py: the reference's comparison loop restated in
Python (a dict, erase on visit, break), or for the one large case a closed-form pattern.  After
every call every out_class and out_peer of both tables, every input field (unchanged), every word
of d_info, both lists and the guard words behind them are compared.
"""
import functools
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import sync_cases as sc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8           # words behind each list and behind d_info that no call may write
CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _ladder(heavy, with_fatal):
    """(local, remote, chain_ver, flags, Plan), built once and never modified."""
    local, remote = sc.ladder_tables()
    flags = sc.HEAVY if heavy else 0
    if not with_fatal:
        remote = sc.without_fatal(local, remote, sc.LADDER_CHAIN_VER, flags)
    return _frozen(local, remote, sc.LADDER_CHAIN_VER, flags)


@functools.lru_cache(maxsize=None)
def _random(n_local, n_remote, seed, ids="mixed", fatal=False, local_dups=0, remote_triples=0, flags=0):
    local, remote, cv = sc.random_tables(n_local, n_remote, seed, ids=ids, fatal=fatal, local_dups=local_dups,
                                         remote_triples=remote_triples)
    return _frozen(local, remote, cv, flags)


def _frozen(local, remote, cv, flags):
    local.setflags(write=False)
    remote.setflags(write=False)
    return local, remote, cv, flags, sc.model(local, remote, cv, flags)


class Box:
    """Device images of one pair of tables with room for (cap_local, cap_remote) records."""

    def __init__(self, dev, cap_local, cap_remote):
        self.dev = dev
        self.local = torch.zeros(max(cap_local, 1) * 48, dtype=torch.uint8, device=dev)
        self.remote = torch.zeros(max(cap_remote, 1) * 48, dtype=torch.uint8, device=dev)
        self.write = torch.empty(cap_local + GUARD, dtype=torch.int32, device=dev)
        self.remove = torch.empty(cap_remote + GUARD, dtype=torch.int32, device=dev)
        self.info = torch.empty(16 + GUARD, dtype=torch.int32, device=dev)

    def load(self, local, remote):
        self.nl, self.nr = local.size, remote.size
        if self.nl:
            self.local[:self.nl * 48].copy_(torch.from_numpy(local.view(np.uint8).copy()))
        if self.nr:
            self.remote[:self.nr * 48].copy_(torch.from_numpy(remote.view(np.uint8).copy()))
        for t in (self.write, self.remove, self.info):
            t.fill_(CANARY)
        torch.cuda.synchronize()

    def plan(self, hf, cv, flags, stream=None, write=True, remove=True):
        hf.sync_plan(self.local if self.nl else None, self.nl, self.remote if self.nr else None, self.nr, cv,
                     self.info, write=self.write if write else None, remove=self.remove if remove else None,
                     flags=flags, stream=stream or torch.cuda.current_stream())

    def fetch(self):
        torch.cuda.synchronize()
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        return (np.frombuffer(self.local.cpu().numpy().tobytes()[:self.nl * 48], dtype=sc.META),
                np.frombuffer(self.remote.cpu().numpy().tobytes()[:self.nr * 48], dtype=sc.META),
                u32(self.info), u32(self.write), u32(self.remove))


def _check(got, local, remote, want, what, write=True, remove=True):
    g_local, g_remote, info, wlist, rlist = got
    for name, g, sent, cls, peer in (("local", g_local, local, want.lclass, want.lpeer),
                                     ("remote", g_remote, remote, want.rclass, want.rpeer)):
        exp = sent.copy()
        exp["out_class"] = np.asarray(cls, dtype=np.uint8)
        exp["out_peer"] = np.asarray(peer, dtype=np.uint32)
        if g.tobytes() != exp.tobytes():
            for f in sc.META.names:
                bad = np.flatnonzero(g[f] != exp[f])
                if bad.size:
                    i = int(bad[0])
                    pytest.fail(f"{what}: {bad.size} {name} records differ in {f}, first {i}: got {g[f][i]}, "
                                f"want {exp[f][i]}")
    got_info = dict(zip(sc.INFO, (int(x) for x in info[:16])))
    assert got_info == want.info, what
    assert (info[16:] == CANARY).all(), f"{what}: words behind d_info written"
    for name, lst, exp, on, cap in (("write", wlist, want.write, write, local.size),
                                    ("remove", rlist, want.remove, remove, remote.size)):
        assert (lst[cap:] == CANARY).all(), f"{what}: words behind the {name} list written"
        if not on:
            assert (lst == CANARY).all(), f"{what}: a NULL {name} list was written"
        elif not want.info["fatal"]:
            exp = np.asarray(exp, dtype=np.uint32)
            assert np.array_equal(lst[:exp.size], exp), f"{what}: {name} list"
            assert (lst[exp.size:] == CANARY).all(), f"{what}: {name} list written past its count"


def _run(hf, dev, case, what, **kw):
    local, remote, cv, flags, want = case
    box = Box(dev, local.size, remote.size)
    box.load(local, remote)
    box.plan(hf, cv, flags, **kw)
    _check(box.fetch(), local, remote, want, what, write=kw.get("write", True), remove=kw.get("remove", True))
    return want


# ---- the ladder ------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_fatal", [True, False], ids=["fatal", "calm"])
@pytest.mark.parametrize("heavy", [False, True], ids=["light", "heavy"])
def test_ladder_table(hf, dev, heavy, with_fatal):
    """The cross product of every condition the ladder tests (1944 chunks, remote order shuffled)."""
    want = _run(hf, dev, _ladder(heavy, with_fatal), f"ladder heavy={heavy} fatal={with_fatal}")
    assert want.info["fatal"] == int(with_fatal)
    if not with_fatal:
        assert want.info["n_write"] > 37 and want.info["n_remove"] == 37


# ---- sizes: wave, workgroup and table-size edges, empty sides --------------------------------------
SIZES = [(0, 0), (0, 1), (1, 0), (1, 1), (63, 65), (64, 64), (65, 63), (64, 256), (256, 257), (257, 256),
         (1024, 1025), (1025, 1024), (1, 5000), (5000, 1), (0, 5000), (5000, 0), (257, 5000), (5000, 5000)]


@pytest.mark.parametrize("n_local,n_remote", SIZES)
def test_sizes(hf, dev, n_local, n_remote):
    _run(hf, dev, _random(n_local, n_remote, 100 + n_local * 7 + n_remote), f"{n_local} x {n_remote}")


@pytest.mark.parametrize("n_local,n_remote", [(65, 63), (1025, 1024), (5000, 5000)])
def test_sizes_heavy(hf, dev, n_local, n_remote):
    _run(hf, dev, _random(n_local, n_remote, 17, flags=sc.HEAVY), f"heavy {n_local} x {n_remote}")


# ---- ids -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", ["share_lo", "share_hi", "small"])
def test_id_shapes(hf, dev, ids):
    """Ids that differ in one half only, and sequential small integers."""
    _run(hf, dev, _random(1025, 1024, 5, ids=ids), ids)


def test_remote_ids_three_times(hf, dev):
    """Only the lowest remote index of an id matches; the other two are REMOTE_ONLY."""
    case = _random(1025, 1024, 6, remote_triples=120)
    want = _run(hf, dev, case, "remote triples")
    assert want.info["n_remove"] > 256 + 100  # 256 foreign ids, and two of every id that appears three times


def test_local_duplicates(hf, dev):
    case = _random(1025, 1024, 7, local_dups=150)
    want = _run(hf, dev, case, "local duplicates")
    assert want.info["duplicates"] >= 100
    both = _random(1025, 1024, 8, local_dups=150, remote_triples=100, fatal=True)
    _run(hf, dev, both, "local duplicates, remote triples, fatal rows")


def test_one_id_everywhere(hf, dev):
    """Every record of both tables has the same id: one MATCHED pair, the rest DUPLICATE / REMOTE_ONLY."""
    local, remote, cv = sc.random_tables(300, 300, 9)
    local, remote = local.copy(), remote.copy()
    for t in (local, remote):
        t["id_hi"], t["id_lo"] = 5, 5
    remote["chain_ver"] = 0
    want = _run(hf, dev, _frozen(local, remote, cv, 0), "one id")
    assert want.info["duplicates"] == 299 and want.info["n_remove"] == 299


# ---- the break -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_local,n_remote,seed", [(1025, 1024, 21), (5000, 5000, 22), (65, 63, 23)])
def test_several_fatal_rows(hf, dev, n_local, n_remote, seed):
    """first_fatal is the lowest fatal index, the counters stop there, the counts are zero."""
    case = _random(n_local, n_remote, seed, fatal=True)
    want = case[4]
    fatal = [r for r, c in enumerate(want.rclass) if c in sc.FATAL]
    assert len(fatal) >= 3 and want.info["first_fatal"] == fatal[0] and want.info["n_write"] == 0
    _run(hf, dev, case, "several fatal rows")


# ---- NULL lists, poison, threads -------------------------------------------------------------------
@pytest.mark.parametrize("write,remove", [(False, True), (True, False), (False, False)])
def test_null_lists(hf, dev, write, remove):
    _run(hf, dev, _random(1025, 1024, 31), "null lists", write=write, remove=remove)
    _run(hf, dev, _ladder(False, True), "null lists, fatal", write=write, remove=remove)


@pytest.mark.parametrize("pattern", [0xFFFFFFFF, 0x00000001, 0xA5A5A5A5])
def test_poisoned_scratch(hf, dev, opts, pattern):
    """Scratch pre-filled with junk (all ones = every slot "empty", claims "none"; small integers =
    valid-looking indices): the plan is unchanged, so every scratch word read was written first."""
    opts("poison", pattern)
    _run(hf, dev, _random(1025, 1024, 41, local_dups=20, remote_triples=20), f"poison {pattern:#x}")
    _run(hf, dev, _ladder(False, True), f"poison {pattern:#x}, fatal")
    _run(hf, dev, _random(0, 0, 100), f"poison {pattern:#x}, empty")


def test_two_threads_two_streams(hf, dev):
    """Two threads plan different tables on their own streams at once: each (stream, thread) pair
    has its own scratch."""
    cases = [_random(5000, 5000, 51), _random(1025, 1024, 52, fatal=True)]
    boxes = [Box(dev, c[0].size, c[1].size) for c in cases]
    for box, c in zip(boxes, cases):
        box.load(c[0], c[1])
    streams = [torch.cuda.Stream(dev) for _ in cases]
    errors = []
    gate = threading.Barrier(2)

    def work(k):
        try:
            torch.cuda.set_device(dev)
            gate.wait(timeout=30)
            for _ in range(4):
                boxes[k].plan(hf, cases[k][2], cases[k][3], stream=streams[k])
            streams[k].synchronize()
        except Exception as e:  # noqa: BLE001
            errors.append(f"thread {k}: {type(e).__name__}: {e}")

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, (box, c) in enumerate(zip(boxes, cases)):
        _check(box.fetch(), c[0], c[1], c[4], f"thread {k}")
    for s in streams:
        hf._lib.release_stream(s)


# ---- a large table: the grid-stride loops, shares of many tiles per workgroup ----------------------
def test_large_tables(hf, dev):
    """1.1 M x 1.05 M records (more tiles than workgroups in every pass); the expectation is the
    closed form of sync_cases.large_tables, itself checked against the model at a small size
    (tests/test_sync_plan_model.py)."""
    local, remote, want = sc.large_tables()
    box = Box(dev, local.size, remote.size)
    box.load(local, remote)
    box.plan(hf, sc.LARGE_CHAIN_VER, 0)
    _check(box.fetch(), local, remote, want, "large")


# ---- scratch ---------------------------------------------------------------------------------------
def test_scratch_bytes_covers_every_smaller_call(hf, dev):
    L = hf._lib
    st = torch.cuda.Stream(dev)
    big = _random(5000, 5000, 51)
    with torch.cuda.stream(st):
        _run(hf, dev, big, "largest", stream=st)
        st0 = L.pair_scratch_stats(st)
        assert st0["call_bytes"] >= L.sync_plan_scratch_bytes(5000, 5000) > 0
        for case in (_random(1025, 1024, 31), _random(1, 5000, 100 + 7 + 5000), _random(5000, 1, 100 + 35000 + 1),
                     _random(0, 0, 100), big):
            assert L.sync_plan_scratch_bytes(case[0].size, case[1].size) <= st0["call_bytes"]
            _run(hf, dev, case, "smaller", stream=st)
        st1 = L.pair_scratch_stats(st)
    assert st1 == st0
    L.release_stream(st)


# ---- plan -> scrub-fill -> scrub -------------------------------------------------------------------
SCRUB = np.dtype([("data", "<u8"), ("length", "<u4"), ("checksum_type", "u1"), ("fin", "u1"), ("reserved", "<u2"),
                  ("checksum", "<u4"), ("computed", "<u4"), ("status", "<i4"), ("reserved2", "<u4")])


@functools.lru_cache(maxsize=None)
def _chunks(orc, n=96, seed=0x96):
    """n chunks of 1 B - 12 KiB at odd offsets of one arena, their stored CRC32C from the oracle, and
    a remote table that makes about a third of them forward.  -> arena, offsets, local, remote, Plan."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 12 << 10, n)
    lens[0], lens[1] = 1, 12 << 10
    offs, at = [], 1
    for ln in lens:
        offs.append(at)
        at += int(ln) + int(rng.integers(1, 128))
        at |= 1  # every chunk at an odd address offset
    arena = rng.integers(0, 256, at + 64, dtype=np.uint8)
    local = sc.table(n)
    local["id_hi"], local["id_lo"] = 0xC0DE, np.arange(n)
    local["chain_ver"], local["update_ver"], local["commit_ver"] = 4, 2, 2
    local["length"], local["chunk_size"], local["checksum_type"] = lens, 16 << 10, 1
    local["checksum"] = [orc.create(1, arena[o:o + int(ln)])[1] for o, ln in zip(offs, lens)]
    remote = local[rng.permutation(n)[:n - 10]].copy()  # ten chunks the successor never heard of
    remote["chunk_size"] = 0
    k = np.arange(remote.size)
    remote["chain_ver"][k % 5 == 0] = 3      # chain version low: forward
    remote["update_ver"][k % 9 == 1] = 3     # remote uncommitted: forward
    local.setflags(write=False)
    remote.setflags(write=False)
    arena.setflags(write=False)
    return arena, np.array(offs, dtype=np.uint64), local, remote, sc.model(local, remote, 4)


def _scrub_want(want, local, base, offs, bad_local):
    exp = np.zeros(local.size, dtype=SCRUB)
    for k, i in enumerate(want.write):
        exp[k]["data"] = base + int(offs[i])
        exp[k]["length"], exp[k]["checksum_type"] = local["length"][i], local["checksum_type"][i]
        exp[k]["checksum"] = exp[k]["computed"] = local["checksum"][i]
        if i == bad_local:
            exp[k]["status"] = 4080
    return exp


def test_plan_scrub_fill_scrub(hf, orc, dev):
    """96 chunks, about a third forwarded; one forwarded chunk has a flipped byte.  plan ->
    scrub_fill -> scrub_batch(n_local) with no host step between: one mismatch, on that record,
    status 4080; every padding record is an untouched {0, 0, NONE} with status 0."""
    L = hf._lib
    arena, offs, local, remote, want = _chunks(orc)
    n = local.size
    assert 24 <= want.info["n_write"] <= 48 and want.info["fatal"] == 0
    bad_local = want.write[len(want.write) // 2]
    d_arena = torch.from_numpy(arena.copy()).to(dev)
    pos = int(offs[bad_local]) + int(local["length"][bad_local]) // 2
    d_arena[pos] ^= 0x40
    addrs = torch.from_numpy((offs + np.uint64(d_arena.data_ptr())).view(np.int64)).to(dev)
    box = Box(dev, n, remote.size)
    box.load(local, remote)
    scrub = torch.full((n * 32 + 64,), 0xEE, dtype=torch.uint8, device=dev)
    cnt = torch.full((1,), 77, dtype=torch.int32, device=dev)
    box.plan(hf, 4, 0)
    L.sync_scrub_fill(box.local, addrs, box.write, box.info, n, scrub)
    L.scrub_batch(hf.CRC32C, scrub, n, 12 << 10, cnt)
    got = box.fetch()
    _check(got, local, remote, want, "end to end")
    assert int(cnt.item()) == 1
    raw = scrub.cpu().numpy()
    assert (raw[n * 32:] == 0xEE).all()
    recs = raw[:n * 32].view(SCRUB)
    exp = _scrub_want(want, local, d_arena.data_ptr(), offs, bad_local)
    bad_k = want.write.index(bad_local)
    exp["computed"][bad_k] = recs["computed"][bad_k]  # (whatever the flipped chunk hashes to)
    assert recs["computed"][bad_k] != exp["checksum"][bad_k]
    for f in SCRUB.names:
        assert np.array_equal(recs[f], exp[f]), f
    assert recs["status"][bad_k] == 4080 and np.count_nonzero(recs["status"]) == 1


# ---- capture ---------------------------------------------------------------------------------------
def test_captured_plan_replans_at_every_replay(hf, orc, dev):
    """plan + scrub_fill + scrub_batch captured once; replayed on the tables as captured, then on
    tables rewritten in place (other classes, other lists, a fatal table, and back): each replay is
    exact."""
    L = hf._lib
    arena, offs, local, remote, want = _chunks(orc)
    n, nr = local.size, remote.size
    d_arena = torch.from_numpy(arena.copy()).to(dev)
    addrs = torch.from_numpy((offs + np.uint64(d_arena.data_ptr())).view(np.int64)).to(dev)
    box = Box(dev, n, nr)
    box.load(local, remote)
    scrub = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        s = torch.cuda.current_stream()
        box.plan(hf, 4, 0, stream=s)
        L.sync_scrub_fill(box.local, addrs, box.write, box.info, n, scrub, stream=s)
        L.scrub_batch(hf.CRC32C, scrub, n, 12 << 10, cnt, stream=s)
    variants = [(local, remote)]
    r2 = remote.copy()
    r2["chain_ver"] = 4
    r2["update_ver"] = 2
    r2["checksum"][::7] ^= 1          # local.chain_ver == the argument: CHAIN_WRITING_CHECKSUM
    r2["id_lo"][3::11] += 1000        # REMOTE_ONLY, and their chunks become REMOTE_MISS
    variants.append((local, r2))
    l3 = local.copy()
    l3["chain_ver"] = 3               # != the argument: differing checksums are fatal now
    r3 = r2.copy()
    r3["chain_ver"] = 3
    variants.append((l3, r3))
    variants.append((local, remote))
    for k, (lo, re) in enumerate(variants):
        w = sc.model(lo, re, 4)
        box.load(lo, re)
        scrub.fill_(0xEE)
        g.replay()
        _check(box.fetch(), lo, re, w, f"replay {k}")
        recs = scrub.cpu().numpy().view(SCRUB)
        exp = _scrub_want(w, lo, d_arena.data_ptr(), offs, -1)
        for f in SCRUB.names:
            assert np.array_equal(recs[f], exp[f]), (k, f)
        assert int(cnt.item()) == 0
    assert sc.model(l3, r3, 4).info["fatal"] == 1 and len(sc.model(local, r2, 4).remove) > 0
    del g


_CHILD = r"""
import importlib, json, sys
import numpy as np, torch
repo, tests, path = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path[:0] = [repo, tests]
hf = importlib.import_module("3fs_amd")
z = np.load(path)
dev = torch.device("cuda:0")
local = torch.from_numpy(z["local"]).to(dev)
remote = torch.from_numpy(z["remote"]).to(dev)
nl, nr = local.numel() // 48, remote.numel() // 48
write = torch.full((nl,), -1, dtype=torch.int32, device=dev)
remove = torch.full((nr,), -1, dtype=torch.int32, device=dev)
info = torch.full((16,), -1, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library call, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            hf.sync_plan(local, nl, remote, nr, int(z["chain_ver"]), info, write=write, remove=remove,
                         stream=torch.cuda.current_stream())
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "sync_plan failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
u32 = lambda t: t.cpu().numpy().view(np.uint32).tolist()
print(json.dumps({"local": local.cpu().numpy().tolist(), "remote": remote.cpu().numpy().tolist(),
                  "info": u32(info), "write": u32(write), "remove": u32(remove)}))
"""


def test_sync_plan_first_call_in_process_is_captured(tmp_path):
    """A fresh process whose first library call is a sync_plan inside
    torch.cuda.graph(capture_error_mode="global"): the context and the call's scratch are first
    allocated during the capture.  The child replays the graph once; the plan is exact."""
    local, remote, cv, flags, want = _random(257, 256, 61)
    path = str(tmp_path / "tables.npz")
    np.savez(path, local=local.view(np.uint8), remote=remote.view(np.uint8), chain_ver=cv)
    p = subprocess.run([sys.executable, "-c", _CHILD, REPO, os.path.join(REPO, "tests"), path],
                       capture_output=True, text=True, timeout=150, env=dict(os.environ), cwd=REPO)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    got = lines[0]
    as_meta = lambda b: np.array(b, dtype=np.uint8).view(sc.META)  # noqa: E731
    pad = lambda a, n: np.concatenate([np.array(a, dtype=np.uint32), np.full(GUARD, CANARY, np.uint32)])  # noqa: E731
    info = np.concatenate([np.array(got["info"], dtype=np.uint32), np.full(GUARD, CANARY, np.uint32)])
    wl = np.where(np.array(got["write"], dtype=np.uint32) == 0xFFFFFFFF, CANARY, np.array(got["write"], dtype=np.uint32))
    rl = np.where(np.array(got["remove"], dtype=np.uint32) == 0xFFFFFFFF, CANARY,
                  np.array(got["remove"], dtype=np.uint32))
    _check((as_meta(got["local"]), as_meta(got["remote"]), info, pad(wl, 0), pad(rl, 0)), local, remote, want,
           "first call captured")

