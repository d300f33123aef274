"""GPU parity of the per-IO request coalescer.

Many threads submit single ChecksumInfo::create requests, as 3FS's 32
AioReadWorker / UpdateWorker threads do per IO (BatchReadJob.cc:24-35,
ChunkReplica.cc:193-207); every value must equal the oracle's create over the
same bytes, whether the bytes sit in HBM, in registered host memory (zero
copy) or in plain host memory copied into the pinned stage.
"""
import ctypes
import random
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _requests(rng, arena_len, count):
    """(offset, length, start, type) tuples; lengths cover 0, tiny, KV-block and >1 MiB sizes."""
    out = []
    for _ in range(count):
        r = rng.random()
        if r < 0.05:
            ln = 0
        elif r < 0.3:
            ln = rng.randrange(1, 200)
        elif r < 0.95:
            ln = rng.choice([4, 8, 16, 32, 64]) * 1024 + rng.randrange(-3, 4)
        else:
            ln = rng.randrange(1 << 20, 3 << 20)
        off = rng.randrange(0, arena_len - ln)
        start = M32 if rng.random() < 0.7 else rng.getrandbits(32)
        ctype = 2 if rng.random() < 0.15 else 1
        out.append((off, ln, start, ctype))
    return out


def _run_threads(nthreads, fn):
    errs = []

    def wrap(t):
        try:
            fn(t)
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errs.append(e)

    ths = [threading.Thread(target=wrap, args=(t,)) for t in range(nthreads)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    if errs:
        raise errs[0]


@pytest.mark.parametrize("service_wgs", [0, 8])
@pytest.mark.parametrize("where", ["hbm", "host_copy", "registered"])
def test_threads_create_one_vs_oracle(hf, orc, dev, where, service_wgs):
    L = hf._lib
    rng = np.random.default_rng(7)
    arena_len = 8 << 20
    host = rng.integers(0, 256, arena_len, dtype=np.uint8)
    keep = None
    if where == "hbm":
        d = torch.from_numpy(host).to(dev)
        keep = d
        base = d.data_ptr()
        flags = 0
    elif where == "registered":
        base = L.host_register(host.ctypes.data, arena_len)
        flags = 0
    else:
        base = host.ctypes.data
        flags = L.REQ_HOST_COPY
    results = {}
    nthreads, per = 16, 60
    reqs = {t: _requests(random.Random(100 + t), arena_len, per) for t in range(nthreads)}
    # small stage: exercises full-slot sealing; service mode: small ring exercises slot reuse, and
    # requests over service_stage / CRC32 ones take the batch path beside it
    with L.Coalescer(device=0, stage_bytes=4 << 20, service_wgs=service_wgs, service_ring=64,
                     service_stage=32 << 10) as co:

        def worker(t):
            for k, (off, ln, start, ctype) in enumerate(reqs[t]):
                results[(t, k)] = co.create_one(ctype, base + off, ln, start, flags)

        _run_threads(nthreads, worker)
        st = co.stats()
    if where == "registered":
        L.host_unregister(host.ctypes.data)
    del keep
    for t in range(nthreads):
        for k, (off, ln, start, ctype) in enumerate(reqs[t]):
            want = orc.create(ctype, host[off:off + ln], start)[1]
            assert results[(t, k)] == want, (where, t, k, ln, ctype)
    assert st["batches"] >= 1 and st["requests"] <= nthreads * per
    with_bytes = [ln for t in range(nthreads) for (_off, ln, _start, _ctype) in reqs[t] if ln > 0]
    assert st["requests"] == len(with_bytes) and st["bytes"] == sum(with_bytes), st  # every route counts


def test_async_submit_drains_on_destroy(hf, orc, dev):
    """Callbacks fire once each with the right value; destroy completes what is pending."""
    L = hf._lib
    rng = np.random.default_rng(11)
    n = 3000
    lens = rng.integers(1, 70000, n)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    host = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    d = torch.from_numpy(host).to(dev)
    got = {}
    lock = threading.Lock()

    @L.DONE_FN
    def cb(arg, status, value):
        with lock:
            got[arg] = (status, value)

    co = L.Coalescer(device=0, max_batch=512)
    for i in range(n):
        rc = L.load().hf3fs_crc_coalescer_submit(co._h, 1, d.data_ptr() + int(offs[i]), int(lens[i]), M32, 0, cb,
                                                  i + 1)
        assert rc == 0
    st = co.stats()
    co.close()
    assert len(got) == n
    assert st["max_batch"] <= 512
    for i in range(0, n, 7):
        o, ln = int(offs[i]), int(lens[i])
        assert got[i + 1] == (0, orc.crc32c_raw(host[o:o + ln])), i


def test_special_cases_and_large_host_copy(hf, orc, dev):
    L = hf._lib
    data = np.random.default_rng(3).integers(0, 256, (3 << 20) + 5, dtype=np.uint8)
    with L.Coalescer(device=0, stage_bytes=1 << 20) as co:
        assert co.create_one(0, data, 100, flags=L.REQ_HOST_COPY) == 0            # NONE -> {NONE, 0}
        assert co.create_one(1, data, 0, start=0x1234, flags=L.REQ_HOST_COPY) == 0x1234  # len 0 -> start
        big = co.create_one(1, data, data.size, flags=L.REQ_HOST_COPY)             # > stage: staged host path
        assert big == orc.crc32c_raw(data)
        assert co.create_one(2, data, 4097, start=7, flags=L.REQ_HOST_COPY) == \
            orc.create(2, data[:4097], 7)[1]
        with pytest.raises(L.Hf3fsCrcError):
            co.create_one(5, data, 10, flags=L.REQ_HOST_COPY)


def test_options_rejected(hf):
    L = hf._lib
    with pytest.raises(L.Hf3fsCrcError):
        L.Coalescer(device=0, slots=1)
    with pytest.raises(L.Hf3fsCrcError):
        L.Coalescer(device=0, inflight=4, slots=4)


def test_service_async_idle_relaunch(hf, orc, dev):
    """Service mode: every async callback fires once with the right value, and
    requests after the kernel's idle exit relaunch it."""
    import time
    L = hf._lib
    rng = np.random.default_rng(12)
    host = rng.integers(0, 256, 4 << 20, dtype=np.uint8)
    d = torch.from_numpy(host).to(dev)
    got = {}
    lock = threading.Lock()

    @L.DONE_FN
    def cb(arg, status, value):
        with lock:
            got[arg] = (status, value)

    with L.Coalescer(device=0, service_wgs=4, service_ring=128, service_idle_us=500) as co:
        reqs = []
        for rnd in range(3):
            for i in range(300):
                off, ln = int(rng.integers(0, 3 << 20)), int(rng.integers(1, 200000))
                key = len(reqs) + 1
                reqs.append((off, ln))
                assert L.load().hf3fs_crc_coalescer_submit(co._h, 1, d.data_ptr() + off, ln, M32, 0, cb, key) == 0
            v = co.create_one(1, d.data_ptr() + 5, 1000)
            assert v == orc.crc32c_raw(host[5:1005])
            time.sleep(0.05)  # > idle timeout: the kernel exits; the next round relaunches it
        st = co.stats()
    assert len(got) == len(reqs)
    for k, (off, ln) in enumerate(reqs):
        assert got[k + 1] == (0, orc.crc32c_raw(host[off:off + ln])), k
    assert st["requests"] >= len(reqs)


# ---- routing limits, from single-threaded submit sequences --------------------------------------
HC = 1  # HF3FS_CRC_REQ_HOST_COPY


class _Sequence:
    """Requests submitted one after another from one thread, so which slot, ring entry or route
    takes each of them follows from the sequence.  Callbacks record (key, status, value) in the
    order they fire; expected values are orc.create's."""

    def __init__(self, L, orc, co):
        self.L, self.orc, self.co = L, orc, co
        self.fired, self.want, self.types, self.lock = [], {}, {}, threading.Lock()
        self.all_done = threading.Event()
        self.requests = self.bytes = 0
        seq = self

        @L.DONE_FN
        def cb(arg, status, value):
            with seq.lock:
                seq.fired.append((arg, status, value))
                if len(seq.fired) == len(seq.want):
                    seq.all_done.set()

        self.cb = cb

    def _expect(self, ctype, host_bytes, start):
        if ctype in (1, 2) and len(host_bytes):
            self.requests += 1
            self.bytes += len(host_bytes)
        return 0 if ctype == 0 else self.orc.create(ctype, host_bytes, start)[1]

    def submit(self, ctype, addr, host_bytes, start=M32, flags=0):
        key = len(self.want) + 1
        self.want[key] = self._expect(ctype, host_bytes, start)
        self.types[key] = ctype
        self.all_done.clear()
        rc = self.L.load().hf3fs_crc_coalescer_submit(self.co._h, ctype, addr, len(host_bytes), start, flags, self.cb, key)
        assert rc == 0, (key, rc)
        return key

    def create_one(self, ctype, addr, host_bytes, start=M32, flags=0):
        want = self._expect(ctype, host_bytes, start)
        assert self.co.create_one(ctype, addr, len(host_bytes), start, flags) == want, (ctype, len(host_bytes))

    def finish(self, in_order=()):
        """Every callback fired exactly once with status 0 and the oracle's value; the keys of
        `in_order` (one type's requests on one route) fired in the order they were submitted."""
        assert self.all_done.wait(timeout=60), f"{len(self.fired)} of {len(self.want)} callbacks fired"
        with self.lock:
            fired = list(self.fired)
        assert sorted(k for k, _, _ in fired) == sorted(self.want), "a callback fired twice or never"
        for k, status, value in fired:
            assert (status, value) == (0, self.want[k]), (k, status, value, self.want[k])
        for keys in in_order:
            pos = [i for i, (k, _, _) in enumerate(fired) if k in keys]
            assert [fired[i][0] for i in pos] == sorted(keys), "callbacks of one type left the launch order"

    def check_stats(self, st, max_batch):
        """requests: the accepted requests with bytes to hash (typed, len > 0), whichever route took
        them; bytes: the sum of their lengths (hf3fs_crc_coalescer_stats, include/hf3fs_crc.h)."""
        assert st["requests"] == self.requests and st["bytes"] == self.bytes, (st, self.requests, self.bytes)
        assert st["max_batch"] <= max_batch, st


def test_batch_mode_stage_and_batch_limits(hf, orc, dev):
    """stage_bytes 4096, max_batch 4.  In order: 4079 + 16 bytes fill a stage exactly (4080 + 16
    granule bytes); 4079 then 17 overflows it by one granule, so the 17 seals the slot and opens
    the next; 4096 takes a whole stage and 4097 the create_host route; then six small requests of
    both types until the fourth CRC32C one seals the slot on max_batch.  A long max_wait_us keeps
    an unsealed slot open, so the seals above are what launches (5 launches at least)."""
    L = hf._lib
    data = np.random.default_rng(21).integers(0, 256, 8192, dtype=np.uint8)
    with L.Coalescer(device=0, stage_bytes=4096, max_batch=4, max_wait_us=200000) as co:
        q = _Sequence(L, orc, co)
        steps = [(1, 4079, M32), (2, 16, 0x1234), (1, 4079, 7), (1, 17, M32), (2, 4096, M32), (1, 4097, 0xABCDEF01),
                 (2, 4097, M32), (0, 100, M32), (1, 0, 0x55), (1, 1, M32), (2, 5, 9), (1, 6, M32), (2, 7, M32),
                 (1, 8, 0xFFFF0000), (1, 9, M32)]
        keys = {1: [], 2: []}
        for i, (ctype, ln, start) in enumerate(steps):
            off = i * 3 + 1   # odd host addresses too
            k = q.submit(ctype, data.ctypes.data + off, data[off:off + ln], start, HC)
            if ctype in keys and 0 < ln <= 4096:
                keys[ctype].append(k)   # (the batch path; the others complete inside submit)
        q.finish(in_order=[set(keys[1]), set(keys[2])])
        st = co.stats()
        q.check_stats(st, 4)
        assert 5 <= st["batches"] <= len(keys[1]) + len(keys[2]), st


def test_service_mode_slice_edges_and_ring_reuse(hf, orc, dev):
    """service_wgs 2, ring 2, service_stage 1024.  HOST_COPY of 1023 and 1024 bytes takes a ring
    slot's stage, 1025 and every CRC32 request the batch path.  Device-resident lengths around
    1 KiB, 16 KiB (wg_hash's 16-wave split) and 64 KiB at address residues 0, 1 and 15, first
    blocking and then asynchronous: 48 service requests on a ring of 2."""
    L = hf._lib
    rng = np.random.default_rng(22)
    host = rng.integers(0, 256, (64 << 10) + 64, dtype=np.uint8)
    d = torch.from_numpy(host).to(dev)
    assert d.data_ptr() % 16 == 0
    lens = [1, 1023, 1024, 1025, (16 << 10) - 1, 16 << 10, (16 << 10) + 1, (64 << 10) + 3]
    errs = []

    def run():
        try:
            with L.Coalescer(device=0, stage_bytes=4096, max_batch=4, service_wgs=2, service_ring=2,
                             service_stage=1024) as co:
                q = _Sequence(L, orc, co)
                for ln in (1023, 1024, 1025):
                    q.create_one(1, host.ctypes.data + 5, host[5:5 + ln], 0x89ABCDEF, HC)
                    q.create_one(2, host.ctypes.data + 7, host[7:7 + ln], M32, HC)
                for r in (0, 1, 15):
                    for ln in lens:
                        q.create_one(1, d.data_ptr() + r, host[r:r + ln], M32 if r else 0x1357)
                service = set()
                for r in (15, 1, 0):
                    for ln in lens:
                        service.add(q.submit(1, d.data_ptr() + r, host[r:r + ln], 0x2468 if r else M32))
                    q.submit(2, d.data_ptr() + r, host[r:r + 1025])
                    q.submit(1, host.ctypes.data + r, host[r:r + 1024], M32, HC)
                assert len(service) + 24 >= 8 * 2
                q.finish(in_order=[service])
                q.check_stats(co.stats(), 4)
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errs.append(e)

    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(timeout=120)   # (the library bounds every spin at kServiceTimeout; this bounds the test)
    assert not th.is_alive(), "the service-mode sequence did not finish"
    if errs:
        raise errs[0]


def test_max_wait_collects_quick_requests(hf, orc, dev):
    """max_wait_us 2000, inflight 1: three quick requests, then a blocking one.  No timing is
    asserted: the values are right and between 1 and 4 batches were launched."""
    L = hf._lib
    host = np.random.default_rng(23).integers(0, 256, 70000, dtype=np.uint8)
    d = torch.from_numpy(host).to(dev)
    with L.Coalescer(device=0, max_wait_us=2000, inflight=1) as co:
        q = _Sequence(L, orc, co)
        for off, ln, ctype in ((0, 5000, 1), (3, 65536, 2), (17, 1, 1)):
            q.submit(ctype, d.data_ptr() + off, host[off:off + ln])
        q.create_one(1, d.data_ptr() + 9, host[9:9 + 40000], 0x42)
        q.finish()
        st = co.stats()
        q.check_stats(st, 4096)
        assert 1 <= st["batches"] <= 4, st
