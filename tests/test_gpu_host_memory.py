"""The library on the memory include/hf3fs_crc.h allows and 3FS deploys: d_* arguments in host
memory registered with hf3fs_crc_host_register (the RDMA BufferPool's slabs, the pinned IO
records), next to the same runs on HBM.

  test_case_images        every batch case of tests/batch_cases.py, arena and each buffer in an
                          allocation of its own between canary guards, in HBM and in registered
                          memory: the outputs are the oracle's and no byte outside the header's
                          output fields changed (tests/host_memory.py; the checker itself is
                          checked in tests/test_host_memory_model.py).
  test_update_*           update_batch, update_cow_batch and update_ordered with the payloads and
                          the IO records registered (and, once, the chunks too), under
                          update_footprint.check_round, cow_cases.check and expected_records.
  test_create_host_*      hf3fs_crc_create_host at the piece and stage limits of its pinned ring.

Everything is bit-exact against the oracle."""
import functools
import threading
import zlib

import numpy as np
import pytest

import batch_cases as bc
import cow_cases as cc
import host_memory as hm
import ordered_cases as oc
import update_footprint as fp

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
LINE = 16 << 10
K_STAGE = 32 << 20      # Context::kStage, 3fs_amd/csrc/hf3fs_crc_api.hip
K_MAX_PIECES = 4096     # kMaxPieces, create_host_staged in 3fs_amd/csrc/hf3fs_crc_api.hip
NT0 = (("nt", "0"),)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


class Hbm:
    """host_memory.Plain's interface on device memory (a torch tensor)."""

    def __init__(self, dev, nbytes, align=hm.PAGE, lead=0):
        self._t = torch.empty(nbytes + align + lead, dtype=torch.uint8, device=dev)
        k = (-self._t.data_ptr()) % align + lead
        self._v = self._t[k:k + nbytes]
        self.dev = self._v.data_ptr()

    def write(self, image):
        self._v.copy_(torch.from_numpy(np.array(image)))
        torch.cuda.synchronize()

    def read(self):
        return self._v.cpu().numpy()

    def close(self):
        self._t = self._v = None


# ---- 2. every batch case, whole images ---------------------------------------------------------
_BUILT = {}


def _built(name, cus):
    """(inputs, reference) of the case at scale 1: computed once, shared by every kind and row, never written."""
    if (name, cus) not in _BUILT:
        case = bc.CASES[name]
        inp = case.build(cus, np.random.default_rng(zlib.crc32(name.encode()) + 1000), 1)
        _BUILT[(name, cus)] = (inp, case.reference(inp))
    return _BUILT[(name, cus)]


IMAGES = [(n, k, r) for n in bc.CASES for k in ("hbm", "registered")
          for r in ["default"] + (["nt=0"] if n in bc.SWITCHES[NT0]["cases"] else [])]


@pytest.mark.parametrize("name,kind,row", IMAGES, ids=[f"{n}-{k}-{r}" for n, k, r in IMAGES])
def test_case_images(hf, opts, dev, cus, name, kind, row):
    """One eager call on buffers that are each their own allocation at an odd lead between 4 KiB
    canary guards.  In `registered` every one of them -- the arena, the records, d_out,
    d_mismatch, d_mismatch_count, d_computed -- is registered host memory, as the header's
    Conventions allow; load nt = 0 is the one switch whose path depends on where the bytes live."""
    L, case = hf._lib, bc.CASES[name]
    inp, ref = _built(name, cus)
    assert bc.switch_key(NT0) == "nt=0"
    if row != "default":
        opts("nt", "0")
    if case.records:
        L.anomalies(0, reset=True)
    alloc = hm.Registered if kind == "registered" else functools.partial(Hbm, dev)
    pl = hm.Placed(case, inp, alloc)
    try:
        try:
            case.call(L, inp, pl.pointers(), torch.cuda.current_stream())
        finally:
            torch.cuda.synchronize()   # before any buffer goes: nothing is unregistered under a kernel
        pl.check(pl.fetch(), ref, f"{name} [{kind}, {row}]")
        if case.records:
            a = L.anomalies(0)
            assert a["count"] == 0 and a["kinds"] == 0, a
    finally:
        pl.close()


# ---- 3. the update calls with the deployed placement ------------------------------------------
class PlacedBackend:
    """update_footprint.run_scenario's backend with the deployed placement: the chunk arena in HBM
    on a 16 KiB line, the payload arena and the record buffer in registered host memory (both on
    a page, so the scenario's (src - dst) mod 16 stays what it claims).  all_host: the chunk arena
    is registered too."""

    def __init__(self, hf, dev, ctype, mode, all_host=False):
        self.hf, self.dev, self.ctype, self.mode, self.all_host = hf, dev, ctype, mode, all_host
        self.mem = []

    def _take(self, nbytes, align=hm.PAGE, host=True):
        m = hm.Registered(nbytes, align) if host else Hbm(self.dev, nbytes, align)
        self.mem.append(m)
        return m

    def start(self, arena, pay_size, recbuf_size):
        self.arena = self._take(arena.size, LINE, host=self.all_host)
        self.arena.write(arena)
        self.pay, self.rec = self._take(pay_size), self._take(recbuf_size)
        return self.arena.dev, self.pay.dev

    def step(self, pay, recbuf, n, max_len):
        self.pay.write(pay)
        self.rec.write(recbuf)
        try:
            self.hf._lib.update_batch(self.ctype, self.rec.dev + fp.REC_GUARD, n, max_len, mode=self.mode,
                                      stream=torch.cuda.current_stream())
        finally:
            torch.cuda.synchronize()
        return self.arena.read(), self.pay.read(), self.rec.read()

    def close(self):
        torch.cuda.synchronize()
        mem, self.mem = self.mem, []
        for m in mem:
            m.close()


@functools.lru_cache(maxsize=None)
def _scenario(orc, name, ctype):
    return {"tiny": fp.tiny_scenario, "rounds": fp.rounds_scenario}[name](orc, ctype)


def _clean(L):
    a = L.anomalies(0)
    assert a["count"] == 0, a


DEPLOYED = [(s, m, p, nt, fp.CRC32C) for s in ("tiny", "rounds") for m in (0, 1)
            for p in ("fused", "ticketed", "oneshot8") for nt in (0, 7)] + \
    [("rounds", m, "fused", 0, fp.CRC32) for m in (0, 1)]


@pytest.mark.parametrize("v", DEPLOYED, ids=[f"{s}-mode{m}-{p}-nt{nt}-{'crc32c' if t == fp.CRC32C else 'crc32'}"
                                             for s, m, p, nt, t in DEPLOYED])
def test_update_batch_deployed(hf, orc, dev, opts, v):
    """update_batch with its payloads and IO records in registered host memory, chunks in HBM:
    every byte of the chunk arena, the payload arena and the record buffer after every batch."""
    name, mode, pipeline, nt, ctype = v
    L = hf._lib
    L.anomalies(0, reset=True)
    fp.set_pipeline(opts, pipeline)
    opts("apply_nt", nt)
    be = PlacedBackend(hf, dev, ctype, mode)
    try:
        fp.run_scenario(_scenario(orc, name, ctype), be)
        _clean(L)
    finally:
        be.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_update_batch_all_host(hf, orc, dev, mode):
    """The same with the chunk arena registered as well: the apply writes host memory."""
    L = hf._lib
    L.anomalies(0, reset=True)
    be = PlacedBackend(hf, dev, fp.CRC32C, mode, all_host=True)
    try:
        fp.run_scenario(_scenario(orc, "tiny", fp.CRC32C), be)
        _clean(L)
    finally:
        be.close()


@functools.lru_cache(maxsize=None)
def _cow(orc, which):
    if which == "main":
        return cc.main_scenario(orc, 16 << 10, 4 << 10)
    return cc.syncing_scenario(orc, 16 << 10, rot=3)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["main", "syncing"])
def test_update_cow_deployed(hf, orc, dev, opts, which, mode):
    """update_cow_batch: payloads, IO records and the destination array registered; the source
    chunks and the destinations in HBM.  cow_cases.check: the whole arena, payloads, records."""
    L = hf._lib
    L.anomalies(0, reset=True)
    opts("apply_piece_kib", 4)
    scn = _cow(orc, which)
    arena = Hbm(dev, scn.image_before(0).size, LINE)
    mem = []
    try:
        arena.write(scn.image_before(0))
        pay = hm.Registered(scn.payload_image(0).size)
        mem.append(pay)
        pay.write(scn.payload_image(0))
        sent, sent_dst = scn.record_buffer(arena.dev, pay.dev), scn.dst_buffer(arena.dev)
        rec, dst = hm.Registered(sent.size), hm.Registered(sent_dst.size)
        mem += [rec, dst]
        rec.write(sent)
        dst.write(sent_dst)
        try:
            hf.update_cow(scn.ctype, rec.dev + fp.REC_GUARD, dst.dev + cc.DST_GUARD, scn.n, scn.max_len, mode=mode,
                          stream=torch.cuda.current_stream())
        finally:
            torch.cuda.synchronize()
        cc.check(scn, arena.read(), pay.read(), rec.read(), sent, dst.read(), sent_dst)
        _clean(L)
    finally:
        torch.cuda.synchronize()
        for m in mem:
            m.close()


ORDERED_MAX_LEN = 512   # the smallest max_len of test_gpu_update_ordered.py (SIZES)


@functools.lru_cache(maxsize=None)
def _ordered_case(orc, which):
    b = (oc.chains if which == "chains" else oc.failures)(orc, ORDERED_MAX_LEN)
    for a in (b.rec, b.pay, b.arena0, b.arena1):
        a.setflags(write=False)
    return b


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["chains", "failures"])
def test_update_ordered_deployed(hf, orc, dev, which, mode):
    """update_ordered hands the chunk state from one IO of a chunk to the next through the
    records, between kernels: here the records (and the payloads) are registered host memory.
    The whole record array against expected_records -- outputs, and the three input fields the
    call rewrites for later IOs of a chunk -- the chunk bytes, the payloads, d_info (HBM)."""
    L = hf._lib
    L.anomalies(0, reset=True)
    b = _ordered_case(orc, which)
    arena = Hbm(dev, b.arena0.size, LINE)
    info = torch.full((2,), 0x7777, dtype=torch.int32, device=dev)
    mem = []
    try:
        arena.write(b.arena0)
        pay = hm.Registered(b.pay.size)
        mem.append(pay)
        pay.write(b.pay)
        sent = oc.record_array(b, arena.dev, pay.dev)
        rec = hm.Registered(sent.nbytes)
        mem.append(rec)
        rec.write(sent.view(np.uint8))
        try:
            L.update_ordered(b.ctype, rec.dev, b.n, b.max_len, b.max_rounds, mode=mode, info=info,
                             stream=torch.cuda.current_stream())
        finally:
            torch.cuda.synchronize()
        got = rec.read().view(fp.REC)
        want = oc.expected_records(b, sent)
        for f in fp.REC.names:
            bad = np.flatnonzero((got[f] != want[f]).reshape(got.size, -1).any(axis=1))
            assert not bad.size, f"{b.name}: {bad.size} IOs differ in {f}, first IO {int(bad[0])}: got " \
                                 f"{got[f][bad[0]]}, want {want[f][bad[0]]}"
        assert got.tobytes() == want.tobytes()
        got_arena = arena.read()
        diff = np.flatnonzero(got_arena != b.arena1)
        assert not diff.size, f"{b.name}: arena differs at {int(diff[0])}"
        assert tuple(int(x) for x in info.cpu().numpy()) == b.info
        assert pay.read().tobytes() == b.pay.tobytes(), "a payload byte changed"
        if which == "failures":
            assert {oc.CHECKSUM_MISMATCH, oc.INVALID_ARG, oc.OK} == set(int(s) for s in got["status"])
        _clean(L)
    finally:
        torch.cuda.synchronize()
        for m in mem:
            m.close()


# ---- 4. hf3fs_crc_create_host at its piece and stage limits -----------------------------------
def _create_host(L, ctype, base, offs, lens, starts=None):
    """hf3fs_crc_create_host on host addresses base + offs (no copies: the residues are the test's)."""
    import ctypes
    n = len(lens)
    ptrs = (ctypes.c_void_p * n)(*[base + int(o) for o in offs])
    ln = (ctypes.c_uint64 * n)(*[int(x) for x in lens])
    st = (ctypes.c_uint32 * n)(*[int(x) for x in starts]) if starts is not None else None
    out = (ctypes.c_uint32 * n)()
    L.check(L.load().hf3fs_crc_create_host(ctype, ptrs, ln, st, out, n))
    return [int(x) for x in out]


@functools.lru_cache(maxsize=None)
def _big():
    """2 * kStage + 17 random bytes behind a lead of 3 (an odd host pointer), made once."""
    a = np.random.default_rng(0x57A6E).integers(0, 256, 2 * K_STAGE + 17 + 3, dtype=np.uint8)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("ctype", [1, 2], ids=["crc32c", "crc32"])
@pytest.mark.parametrize("n", [2 * K_MAX_PIECES + 5, 3 * K_MAX_PIECES + 7])
def test_create_host_piece_limit(hf, orc, ctype, n):
    """More buffers than one stage holds pieces (kMaxPieces = 4096): lengths cycle through 0, 1,
    15, 16, 17, 40, explicit starts, host pointers at every residue mod 16.  A zero-length buffer
    makes no piece, so of 2 * 4096 + 5 buffers 6831 do and two fills are bounded by the piece
    count; 3 * 4096 + 7 buffers make 10246 pieces: three fills, the third reuses (and first
    drains) stage 0."""
    L = hf._lib
    rng = np.random.default_rng(n + ctype)
    lens = np.array([(0, 1, 15, 16, 17, 40)[i % 6] for i in range(n)])
    offs = np.arange(n) * 64 + np.arange(n) % 16
    raw = rng.integers(0, 256, n * 64 + 128, dtype=np.uint8)
    pad = (-raw.ctypes.data) % 16
    data = raw[pad:]
    assert set(((data.ctypes.data + offs) % 16).tolist()) == set(range(16))
    pieces = int(np.count_nonzero(lens))
    assert -(-pieces // K_MAX_PIECES) == (2 if n == 2 * K_MAX_PIECES + 5 else 3)
    starts = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    got = _create_host(L, ctype, data.ctypes.data, offs, lens, starts)
    want = [orc.create(ctype, data[o:o + ln], int(s))[1] for o, ln, s in zip(offs.tolist(), lens.tolist(), starts.tolist())]
    assert got == want, next((i, int(lens[i]), got[i], want[i]) for i in range(n) if got[i] != want[i])


SINGLE = [(K_STAGE - 1, 1), (K_STAGE, 1), (K_STAGE + 1, 1), (2 * K_STAGE + 17, 1), (K_STAGE, 2)]


@pytest.mark.parametrize("ln,ctype", SINGLE, ids=[f"{ln - K_STAGE:+d}-{'crc32c' if t == 1 else 'crc32'}" for ln, t in SINGLE])
def test_create_host_single_buffer_at_stage_boundary(hf, orc, ln, ctype):
    """One buffer of kStage - 1, kStage, kStage + 1 and 2 kStage + 17 bytes (kStage = 32 MiB): one
    piece that ends a byte before the stage does, one that fills it, pieces stitched with
    x^(8 * tail) across two and three stages (the third refills stage 0)."""
    data = _big()[3:3 + ln]
    assert data.ctypes.data % 2
    got = _create_host(hf._lib, ctype, data.ctypes.data, [0], [ln])
    assert got == [orc.create(ctype, data)[1]]


SPLITS = {"end-5": [K_STAGE - 5, 11, 0, 3, 0], "cut-32": [K_STAGE - 32, 43, 0, 3, 0]}


@pytest.mark.parametrize("ctype", [1, 2], ids=["crc32c", "crc32"])
@pytest.mark.parametrize("layout", list(SPLITS))
def test_create_host_split_before_stage_end(hf, orc, layout, ctype):
    """end-5: [kStage - 5, 11, 0, 3, 0].  The first buffer ends five bytes before the stage does;
    pieces start on 16 B granules, so nothing fits behind it and the 11 bytes open the next
    stage, followed by a zero-length buffer at that boundary and one at the end.  cut-32: the
    first buffer leaves 32 bytes of the stage, so the 43-byte buffer is cut there and its last
    11 bytes are stitched on from the next stage."""
    lens = SPLITS[layout]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) + 3
    big = _big()
    starts = [0xFFFFFFFF, 0x12345678, 0xCAFEF00D, 0, 0x9ABCDEF0]
    got = _create_host(hf._lib, ctype, big.ctypes.data, offs, lens, starts)
    want = [orc.create(ctype, big[o:o + ln], s)[1] for o, ln, s in zip(offs.tolist(), lens, starts)]
    assert got == want


def test_create_host_two_threads(hf, orc):
    """Two threads, three calls each of about 40 MiB in mixed lengths at the same time: the calls
    share the context's two pinned stages under stage_mu, so every value must come out right."""
    L = hf._lib
    lens = [(24 << 20) + 13, 0, 1, 4097, (1 << 20) + 1, 65536, (14 << 20) + 7, 17]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    big = _big()
    bases = [3, 3 + (20 << 20) + 5]   # (two overlapping windows of the shared bytes)
    assert bases[1] + sum(lens) <= big.size
    want = {(t, c): [orc.create(c, big[bases[t] + o:bases[t] + o + ln])[1] for o, ln in zip(offs.tolist(), lens)]
            for t in (0, 1) for c in (1, 2)}
    got, errs = {}, []

    def work(t):
        try:
            for k in range(3):
                c = 2 if k == 1 else 1
                order = np.roll(np.arange(len(lens)), k + t)
                vals = _create_host(L, c, big.ctypes.data + bases[t], offs[order], [lens[i] for i in order])
                got[(t, k)] = (c, order, vals)
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errs.append(e)

    ths = [threading.Thread(target=work, args=(t,), daemon=True) for t in (0, 1)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=120)
        assert not th.is_alive(), "a create_host call did not return"
    assert not errs, errs
    for (t, k), (c, order, vals) in sorted(got.items()):
        assert vals == [want[(t, c)][i] for i in order], (t, k)
    assert len(got) == 6
