"""hf3fs_crc_update_cow_batch and HF3FS_UPDATE_FLAG_SYNCING on the GPU (tests/cow_cases.py).

After every batch the WHOLE arena -- source chunks, destinations and the canary between them --
must equal the expected image, the payloads and the records' input fields must be unchanged and
every output field must be the oracle's.  Chunk capacities 64 and 128 KiB, 32 IOs per batch.
"""
import functools
import time

import numpy as np
import pytest

import cow_cases as cc
import update_footprint as fp

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
LINE = 16 << 10
_T0 = time.time()
_COUNT = [0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _counted():
    _COUNT[0] += 1
    yield


@pytest.fixture(scope="module", autouse=True)
def _module_end(hf):
    yield
    a = hf._lib.anomalies()
    print(f"\n[test_gpu_update_cow] {_COUNT[0]} tests in {time.time() - _T0:.1f} s")
    assert a["count"] == 0, a


class Gpu:
    """Device buffers of one scenario: arena on a 16 KiB line, payloads, records, destinations."""

    def __init__(self, hf, dev, scn, ctype, mode):
        self.hf, self.dev, self.scn, self.ctype, self.mode = hf, dev, scn, ctype, mode
        arena = scn.image_before(0)
        raw = torch.empty(arena.size + LINE, dtype=torch.uint8, device=dev)
        lift = (-raw.data_ptr()) % LINE
        self.raw, self.arena = raw, raw[lift:lift + arena.size]
        self.arena.copy_(self._up(arena))
        self.pay = self._up(scn.payload_image(0))
        self.arena_addr, self.pay_addr = self.arena.data_ptr(), self.pay.data_ptr()

    def _up(self, a):
        return torch.from_numpy(np.array(a)).to(self.dev)

    def fetch(self, *more):
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (self.arena, self.pay) + more]


def _run_cow(hf, dev, scn, ctype, mode, stream=None):
    g = Gpu(hf, dev, scn, ctype, mode)
    sent = scn.record_buffer(g.arena_addr, g.pay_addr)
    sent_dst = scn.dst_buffer(g.arena_addr)
    rec, dst = g._up(sent), g._up(sent_dst)
    torch.cuda.synchronize()
    hf.update_cow(ctype, rec.data_ptr() + fp.REC_GUARD, dst.data_ptr() + cc.DST_GUARD, scn.n, scn.max_len,
                  mode=mode, stream=stream or torch.cuda.current_stream())
    arena, pay, got_rec, got_dst = g.fetch(rec, dst)
    cc.check(scn, arena, pay, got_rec, sent, got_dst, sent_dst)
    return got_rec


@functools.lru_cache(maxsize=None)
def _main(orc, max_len, piece_kib, kind, variant):
    ctype = fp.CRC32 if kind == "crc32" else fp.CRC32C
    return cc.main_scenario(orc, max_len, piece_kib << 10, ctype, engine=kind == "engine", rot=variant % 16,
                            variant=variant)


@functools.lru_cache(maxsize=None)
def _sync(orc, max_len, kind, rot):
    ctype = fp.CRC32 if kind == "crc32" else fp.CRC32C
    return cc.syncing_scenario(orc, max_len, ctype, engine=kind == "engine", rot=rot)


def _main_variants():
    """(max_len, piece KiB, kind, mode, apply_grid, variant): every combination of capacity, piece
    size, checksum kind, mode and the two grids the call distinguishes (apply_grid 2, and any
    other value: -1 and 1 alternate); `variant` 0..15 rotates the destination residues and the
    prefix / suffix pairs, so the 72 cases reach all 256 residue pairs and every edge pair."""
    out, k = [], 0
    for max_len in (64 << 10, 128 << 10):
        for piece in (4, 8, 16):
            for kind in ("crc32c", "crc32", "engine"):
                for mode in (0, 1):
                    for grid in (2, (-1, 1)[k % 2]):
                        out.append((max_len, piece, kind, mode, grid, k % 16))
                        k += 1
    return out


MAIN = _main_variants()


@pytest.mark.parametrize("v", MAIN, ids=[f"{m >> 10}K-p{p}-{kd}-mode{mo}-grid{g}-v{k}" for m, p, kd, mo, g, k in MAIN])
def test_cow_out_of_place(hf, orc, dev, opts, v):
    max_len, piece, kind, mode, grid, variant = v
    opts("apply_piece_kib", piece)
    opts("apply_grid", grid)
    opts("apply_nt", 6 + variant % 2)
    scn = _main(orc, max_len, piece, kind, variant)
    ctype = fp.CRC32 if kind == "crc32" else fp.CRC32C
    res = np.frombuffer(_run_cow(hf, dev, scn, ctype, mode)[fp.REC_GUARD:fp.REC_GUARD + 32 * 56].tobytes(), dtype=fp.REC)
    assert int(res["status"][21]) == fp.CHECKSUM_MISMATCH and int(res["status"][22]) == fp.INVALID_ARG


def test_cow_cases_cover_residues_and_edges(orc):
    """The 72 cases above reach every (source, destination) residue pair mod 16 and, for each piece
    size, every old-prefix and old-suffix length of cow_cases.edge_lengths."""
    pairs, pre, suf = set(), {4: set(), 8: set(), 16: set()}, {4: set(), 8: set(), 16: set()}
    for max_len, piece, kind, mode, grid, variant in MAIN:
        scn = _main(orc, max_len, piece, kind, variant)
        r = scn.rounds[0]
        for c in range(scn.n):
            if r.place[c] != cc.OUT_OF_PLACE:
                continue
            pairs.add((scn.lay.bases[c] % 16, int(r.dst[c]) % 16))
            op = r.ops[c]
            if op["kind"] == "W" and r.expect[c][0] == fp.OK:
                s0 = r.sizes_before[c]
                pre[piece].add(min(op["off"], s0))
                suf[piece].add(s0 - min(op["off"] + op["ln"], s0))
    assert len(pairs) == 256
    for piece in (4, 8, 16):
        assert set(cc.edge_lengths(piece << 10)) <= pre[piece], (piece, sorted(pre[piece]))
        assert set(cc.edge_lengths(piece << 10)) <= suf[piece], (piece, sorted(suf[piece]))


SYNC = [(m, kd, mo) for m in (64 << 10, 128 << 10) for kd in ("crc32c", "crc32", "engine") for mo in (0, 1)]


@pytest.mark.parametrize("v", SYNC, ids=[f"{m >> 10}K-{kd}-mode{mo}" for m, kd, mo in SYNC])
def test_cow_syncing(hf, orc, dev, opts, v):
    max_len, kind, mode = v
    scn = _sync(orc, max_len, kind, 3 + mode)
    _run_cow(hf, dev, scn, fp.CRC32 if kind == "crc32" else fp.CRC32C, mode)


@pytest.mark.parametrize("entry", ["update_batch", "update_ordered"])
@pytest.mark.parametrize("pipeline", ["fused", "unfused"])
@pytest.mark.parametrize("kind", ["crc32c", "engine"])
def test_syncing_through_in_place_entry_points(hf, orc, dev, opts, kind, pipeline, entry):
    """The syncing IOs of the scenario, every one in place, through update_batch and update_ordered."""
    opts("update_pipeline", pipeline)
    base = _sync(orc, 64 << 10, kind, 3)
    scn = base.in_place_twin()
    ops = [dict(op, place=cc.IN_PLACE_ZERO) for op in base.rounds[0].ops[:base.n]]
    scn.build(ops)
    g = Gpu(hf, dev, scn, fp.CRC32C, 1)
    sent = scn.record_buffer(g.arena_addr, g.pay_addr)
    rec = g._up(sent)
    torch.cuda.synchronize()
    if entry == "update_batch":
        hf._lib.update_batch(fp.CRC32C, rec.data_ptr() + fp.REC_GUARD, scn.n, scn.max_len, mode=1,
                             stream=torch.cuda.current_stream())
    else:
        hf.update_ordered(fp.CRC32C, rec.data_ptr() + fp.REC_GUARD, scn.n, scn.max_len, 2, mode=1,
                          stream=torch.cuda.current_stream())
    arena, pay, got = g.fetch(rec)
    cc.check(scn, arena, pay, got, sent)


# ---- in place: byte-identical to update_batch ---------------------------------------------------------
class _PairBackend:
    """update_footprint.run_scenario's backend that runs update_batch on one arena and
    update_cow_batch on a second one at every step, and compares the two byte for byte."""

    def __init__(self, hf, dev, mode, dst_kind):
        self.hf, self.dev, self.mode, self.dst_kind = hf, dev, mode, dst_kind

    def _up(self, a):
        return torch.from_numpy(np.array(a)).to(self.dev)

    def start(self, arena, pay_size, recbuf_size):
        raw = torch.empty(arena.size + LINE, dtype=torch.uint8, device=self.dev)
        lift = (-raw.data_ptr()) % LINE
        self.raw, self.a1 = raw, raw[lift:lift + arena.size]
        self.a1.copy_(self._up(arena))
        self.pay = torch.empty(pay_size, dtype=torch.uint8, device=self.dev)
        return self.a1.data_ptr(), self.pay.data_ptr()

    def step(self, pay, recbuf, n, max_len):
        self.pay.copy_(self._up(pay))
        raw2 = torch.empty(self.a1.numel() + LINE, dtype=torch.uint8, device=self.dev)
        lift = (-raw2.data_ptr()) % LINE
        a2 = raw2[lift:lift + self.a1.numel()]   # the COW call's arena: same bytes, records re-based onto it
        a2.copy_(self.a1)
        delta = a2.data_ptr() - self.a1.data_ptr()
        rec1 = self._up(recbuf)
        rb2 = recbuf.copy()
        r2 = rb2[fp.REC_GUARD:fp.REC_GUARD + n * 56].view(fp.REC)
        r2["chunk"] = (r2["chunk"].astype(np.int64) + delta).astype(np.uint64)
        rec2 = self._up(rb2)
        dst = None
        if self.dst_kind == "zero":
            dst = torch.zeros(n, dtype=torch.int64, device=self.dev)
        elif self.dst_kind == "own":
            dst = self._up(r2["chunk"].astype(np.int64))
        torch.cuda.synchronize()
        st = torch.cuda.current_stream()
        self.hf._lib.update_batch(fp.CRC32C, rec1.data_ptr() + fp.REC_GUARD, n, max_len, mode=self.mode, stream=st)
        self.hf.update_cow(fp.CRC32C, rec2.data_ptr() + fp.REC_GUARD, dst, n, max_len, mode=self.mode, stream=st)
        torch.cuda.synchronize()
        assert torch.equal(self.a1, a2), "update_cow_batch in place left other chunk bytes than update_batch"
        g1, g2 = rec1.cpu().numpy(), rec2.cpu().numpy()
        o1 = g1[fp.REC_GUARD:fp.REC_GUARD + n * 56].view(fp.REC)
        o2 = g2[fp.REC_GUARD:fp.REC_GUARD + n * 56].view(fp.REC).copy()
        o2["chunk"] = (o2["chunk"].astype(np.int64) - delta).astype(np.uint64)
        assert o1.tobytes() == o2.tobytes(), "records differ between update_batch and update_cow_batch in place"
        assert np.array_equal(g1[:fp.REC_GUARD], g2[:fp.REC_GUARD]) and np.array_equal(g1[-fp.REC_GUARD:], g2[-fp.REC_GUARD:])
        return self.a1.cpu().numpy(), self.pay.cpu().numpy(), g1


@functools.lru_cache(maxsize=None)
def _in_place(orc):
    return dict(cc.in_place_scenarios(orc))


@pytest.mark.parametrize("dst_kind", ["null", "zero", "own"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["tiny", "rows", "rounds"])
def test_cow_in_place_equals_update_batch(hf, orc, dev, opts, name, mode, dst_kind):
    fp.run_scenario(_in_place(orc)[name], _PairBackend(hf, dev, mode, dst_kind))


def test_cow_argument_errors(hf, dev):
    L = hf._lib
    for args in ((7, 1, None, 1, 4096, 0), (fp.CRC32C, 1, None, 1, 4096, 5), (fp.CRC32C, None, None, 1, 4096, 0)):
        with pytest.raises(hf.Hf3fsCrcError) as e:
            L.update_cow(args[0], args[1], args[2], args[3], args[4], mode=args[5])
        assert e.value.code == fp.INVALID_ARG
    assert L.update_cow(fp.CRC32C, None, None, 0, 4096, mode=0) == 0
    assert L.update_cow_scratch_bytes(0, 4096, 0) == 0 and L.update_cow_scratch_bytes(4, 4096, 9) == 0


# ---- contexts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_cow_poisoned_scratch(hf, orc, dev, opts, mode):
    """Two different poison values: identical (and correct) results, so no scratch word is read unwritten."""
    scn = _main(orc, 64 << 10, 8, "crc32c", 5)
    outs = []
    for poison in (0xA5A5A5A5, 0x00000001):
        opts("poison", poison)
        outs.append(_run_cow(hf, dev, scn, fp.CRC32C, mode).tobytes())
    n = scn.n * 56
    a = np.frombuffer(outs[0], dtype=np.uint8)[fp.REC_GUARD:fp.REC_GUARD + n].view(fp.REC)
    b = np.frombuffer(outs[1], dtype=np.uint8)[fp.REC_GUARD:fp.REC_GUARD + n].view(fp.REC)
    for f in fp.OUTPUT_FIELDS:
        assert np.array_equal(a[f], b[f]), f


@pytest.mark.parametrize("mode", [0, 1])
def test_cow_captured_and_replayed(hf, orc, dev, opts, mode):
    """One captured call, replayed three times; between replays the destinations are re-filled
    with canary and the payloads (and the records' client checksums) replaced."""
    scns = [_main(orc, 64 << 10, 8, "crc32c", 7)]
    g = Gpu(hf, dev, scns[0], fp.CRC32C, mode)
    sent = scns[0].record_buffer(g.arena_addr, g.pay_addr)
    sent_dst = scns[0].dst_buffer(g.arena_addr)
    rec, dst = g._up(sent), g._up(sent_dst)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream(dev)):
        hf.update_cow(fp.CRC32C, rec.data_ptr() + fp.REC_GUARD, dst.data_ptr() + cc.DST_GUARD, 32, 64 << 10, mode=mode,
                      stream=torch.cuda.current_stream())
    for k in range(3):
        # the same shapes with other payload bytes: a twin built from another seed (same sizes, so
        # the same addresses), whose records carry the new client checksums
        scn = scns[0]
        if k:
            base = scns[0]
            scn = base.in_place_twin()
            scn.rng = np.random.default_rng(1000 + k)
            scn.build([dict(op) for op in base.rounds[0].ops[:base.n]])
            assert scn.pay_size == base.pay_size
        sent = scn.record_buffer(g.arena_addr, g.pay_addr)
        g.arena.copy_(g._up(scn.image_before(0)))
        g.pay.copy_(g._up(scn.payload_image(0)))
        rec.copy_(g._up(sent))
        torch.cuda.synchronize()
        graph.replay()
        arena, pay, got_rec, got_dst = g.fetch(rec, dst)
        cc.check(scn, arena, pay, got_rec, sent, got_dst, sent_dst)
    del graph


@pytest.mark.parametrize("mode", [0, 1])
def test_cow_scratch_bytes_covers_every_smaller_call(hf, orc, dev, opts, mode):
    """After one call of the largest shape the pair's buffer does not grow: no allocation over
    smaller and equal calls in the same mode, and the buffer is at least what cow_scratch_bytes
    promised."""
    L = hf._lib
    big = _main(orc, 128 << 10, 4, "crc32c", 2)
    opts("apply_piece_kib", 4)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        _run_cow(hf, dev, big, fp.CRC32C, mode, stream=st)
        st0 = L.pair_scratch_stats(st)
        assert st0["call_bytes"] >= L.update_cow_scratch_bytes(32, 128 << 10, mode) > 0
        for scn in (_main(orc, 64 << 10, 4, "crc32c", 2), big, _sync(orc, 64 << 10, "crc32c", 3), big):
            assert L.update_cow_scratch_bytes(scn.n, scn.max_len, mode) <= st0["call_bytes"]
            _run_cow(hf, dev, scn, fp.CRC32C, mode, stream=st)
        st1 = L.pair_scratch_stats(st)
    assert st1 == st0
    L.release_stream(st)


def test_plain_update_batch_plans_as_before_around_a_cow_call(hf, orc, dev, opts):
    """A plain update_batch on the pair before and after a COW call stays right: three rounds of
    mixed traffic, a COW call between them, the whole arena and every record checked after each.
    What this cannot show: that the COW call leaves the plain call's hint word alone.  A plain
    call planned from the COW call's piece count (four ranges per IO) would only launch a larger
    one-shot grid, whose surplus workgroups exit at once, so no result differs; the separation is
    by construction (PairState::hint[2], plan_update) and is not verified here."""
    opts("update_pipeline", "unfused")
    plain = fp.rounds_scenario(orc, n=32, max_len=64 << 10, rounds=3, seed=0xE7)
    cow = _main(orc, 64 << 10, 8, "crc32c", 9)
    from test_gpu_update_footprint import GpuBackend
    be = GpuBackend(hf, dev, fp.CRC32C, 1)
    chunk_addr, pay_addr = be.start(plain.image_before(0), plain.pay_size, 2 * fp.REC_GUARD + 32 * 56)
    for k in range(3):
        sent = plain.record_buffer(k, chunk_addr, pay_addr)
        got = be.step(plain.payload_image(k), sent.copy(), 32, 64 << 10)
        fp.check_round(plain, k, got[0], got[1], got[2], sent)
        if k < 2:
            _run_cow(hf, dev, cow, fp.CRC32C, 1)


# ---- the first library call of a process, captured ------------------------------------------------
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
dst = z["dst"].copy()
dst[z["place"] == 2] += np.uint64(arena.data_ptr())
dst[z["place"] == 1] = rec["chunk"][z["place"] == 1]
n = rec.size
d_ios = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
d_dst = torch.from_numpy(dst.view(np.int64).copy()).to(dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library call, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            hf.update_cow(hf.CRC32C, d_ios, d_dst, n, int(z["max_len"]), mode=mode, stream=torch.cuda.current_stream())
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "update_cow_batch failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
res = np.frombuffer(d_ios.cpu().numpy().tobytes(), dtype=fp.REC)
print(json.dumps({"status": res["status"].tolist(), "case": res["checksum_case"].tolist(),
                  "size": res["out_size"].tolist(), "checksum": res["out_checksum"].tolist(),
                  "ctype": res["out_checksum_type"].tolist(),
                  "arena_sha256": hashlib.sha256(arena.cpu().numpy().tobytes()).hexdigest()}))
"""


def test_cow_first_call_in_process_is_captured(orc, tmp_path):
    """A fresh process whose first library call is a DELTA update_cow_batch inside
    torch.cuda.graph(capture_error_mode="global"): context, hint slab, side stream and scratch are
    all first allocated during the capture.  One replay; statuses, cases, sizes, checksums and a
    digest of the whole arena (sources, destinations, canary) equal the oracle's."""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scn = _main(orc, 64 << 10, 8, "crc32c", 3)
    r = scn.rounds[0]
    path = str(tmp_path / "inputs.npz")
    np.savez(path, arena=scn.image_before(0), pay=scn.payload_image(0), rec=r.rec, has_payload=r.has_payload,
             dst=r.dst, place=r.place, max_len=scn.max_len)
    p = subprocess.run([sys.executable, "-c", _CHILD, repo, os.path.join(repo, "tests"), path, "1"],
                       capture_output=True, text=True, timeout=150, cwd=repo)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    got = lines[0]
    assert got["status"] == [e[0] for e in r.expect]
    assert got["case"] == [e[3] for e in r.expect]
    assert got["size"] == [e[1] for e in r.expect]
    assert list(zip(got["ctype"], got["checksum"])) == [tuple(e[2]) for e in r.expect]
    assert got["arena_sha256"] == hashlib.sha256(scn.image_after(0).tobytes()).hexdigest()
