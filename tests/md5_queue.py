"""Builders, runs and checkers for hf3fs_crc_md5_batch at large file counts, queued without waits
and from seeded states: shared by tests/test_md5_queue_model.py (a stand-in library made of hashlib
and md5_cases.State, right and deliberately wrong) and tests/test_gpu_md5_queue.py (the library).

A `Batch` is one call's records as numpy arrays over one arena, built vectorised: md5_cases.records
loops in Python and is too slow at 10^6 files.  A run takes a backend -- upload / full / read /
md5_batch / ready / wait, addresses as integers, 0 = NULL -- so the same code queues the calls and
checks the results on the GPU and on the stand-in.  Every digest is compared with hashlib.md5 of
the file's bytes (holes as zeros) per file index, every state with md5_cases.State, outputs start
from a sentinel between guard bytes, and a failure names the first differing files and their
lengths.  Numpy only: no GPU, no torch.
"""
import bisect
import functools
import hashlib
import struct

import numpy as np

import md5_cases as mc

GUARD, CANARY, SENTINEL = 64, 0xEE, 0x5E
BOTH = mc.INIT | mc.FINAL
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]  # md5_stage x md5_sort
M64 = 2 ** 64

# ---- the passes' geometry, restated from 3fs_amd/csrc/md5_kernels.hip --------------------------------
SHARES_MAX = 256      # kMd5SharesMax (md5_kernels.h): waves of the count and scatter passes
TILE = 64             # shares_of: a share is a multiple of 64 files
PREP_BLOCKS_MAX = 4096  # grid_of: k_md5_prep's grid is capped at 4096 workgroups ...
PREP_THREADS = 256      # ... of 256 threads, one file per thread and grid stride


def shares_of(n):
    tiles = (n + TILE - 1) // TILE
    shares = min(max(tiles, 1), SHARES_MAX)
    return shares, (tiles + shares - 1) // shares * TILE  # (shares, files per share)


def grid_of(n):
    return min(max((n + PREP_THREADS - 1) // PREP_THREADS, 1), PREP_BLOCKS_MAX)


def geometry(n):
    """What the count / scatter passes and prep see at n files: share s owns [s per, min(n, (s + 1) per))."""
    shares, per = shares_of(n)
    sizes = [max(0, min(n, (s + 1) * per) - s * per) for s in range(shares)]
    return dict(shares=shares, tiles_per_share=per // TILE, empty=sum(1 for x in sizes if x == 0),
                partial=[s for s, x in enumerate(sizes) if x % TILE],  # shares whose last tile is not full
                partial_behind_full=[s for s, x in enumerate(sizes) if x % TILE and x > TILE],
                prep_grid=grid_of(n), prep_strides=n > grid_of(n) * PREP_THREADS)


COUNTS = (16384, 16385, 32769, 70001, (1 << 20) + 300)  # 16384: the last count of one tile per share
SPREAD_COUNTS = (16385, 70001)
TWO_CALL_COUNT = 70001

BUCKETS = 256  # kMd5Buckets (md5_core.h)


def md5_bucket(blocks):
    """md5_bucket of md5_core.h: four sub-buckets per octave of the block count, the longest first."""
    if blocks == 0:
        return BUCKETS - 1
    o = blocks.bit_length() - 1
    sub = (blocks >> (o - 2)) & 3 if o >= 2 else (blocks << (2 - o)) & 3
    return BUCKETS - 2 - min(4 * o + sub, BUCKETS - 2)


def call_blocks(tail_len, new_bytes, final):
    """md5_call_blocks of md5_core.h."""
    m = tail_len + new_bytes
    return m // 64 + ((1 if m % 64 < 56 else 2) if final else 0)


# ---- one call's records ----------------------------------------------------------------------------------
class Batch:
    """n files over one arena.  Segment k lies at arena offset seg_at[k] (-1: a hole) and has
    seg_len[k] bytes; file f owns segments [file_off[f], file_off[f + 1])."""

    def __init__(self, arena, seg_at, seg_len, file_off):
        self.arena = arena
        self.seg_at = np.asarray(seg_at, dtype=np.int64)
        self.seg_len = np.asarray(seg_len, dtype=np.uint64)
        self.file_off = np.asarray(file_off, dtype=np.uint64)
        self.n, self.n_segs = self.file_off.size - 1, self.seg_at.size
        assert self.seg_len.size == self.n_segs and int(self.file_off[-1]) == self.n_segs and self.file_off[0] == 0
        real = self.seg_at >= 0
        assert (self.seg_at[real] + self.seg_len[real].astype(np.int64) <= arena.size).all()

    @classmethod
    def of_files(cls, arena, files):
        """From md5_cases' form: per file a list of (arena offset or None, length)."""
        segs = [s for f in files for s in f]
        off = np.cumsum([0] + [len(f) for f in files])
        return cls(arena, [-1 if o is None else o for o, _ in segs], [n for _, n in segs], off)

    def records(self, base):
        """(hf3fs_crc_md5_seg array, d_file_off) for an arena at address `base`."""
        segs = np.zeros(self.n_segs, dtype=mc.SEG)
        segs["data"] = np.where(self.seg_at < 0, 0, self.seg_at + base).astype(np.uint64)
        segs["length"] = self.seg_len
        return segs, self.file_off.copy()

    @functools.cached_property
    def lengths(self):
        run = np.concatenate([[0], np.cumsum(self.seg_len.astype(np.int64))])
        off = self.file_off.astype(np.int64)
        return run[off[1:]] - run[off[:-1]]

    def contents(self):
        """The message of every file: its segments' bytes in order, holes as zeros."""
        raw, at, ln, off = self.arena.tobytes(), self.seg_at.tolist(), self.seg_len.tolist(), self.file_off.tolist()
        out = []
        for f in range(self.n):
            parts = [bytes(ln[k]) if at[k] < 0 else raw[at[k]:at[k] + ln[k]] for k in range(off[f], off[f + 1])]
            out.append(parts[0] if len(parts) == 1 else b"".join(parts))
        return out

    @functools.cached_property
    def digests(self):
        """hashlib's digest of every file, 16 n bytes; computed once."""
        return b"".join(hashlib.md5(c).digest() for c in self.contents())


@functools.lru_cache(maxsize=None)
def _arena(seed, size=1 << 20):
    a = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def tiny(n, seed=11):
    """A1: each file one segment of 0..130 bytes at a random offset, of any residue, in one shared
    1 MiB arena of random bytes (segments overlap: nothing writes them).  Files 16 j + 5 are one
    empty segment, files 16 j + 11 have no segment at all."""
    rng = np.random.default_rng(seed * 1000003 + n)
    i = np.arange(n)
    length = rng.integers(0, 131, n)
    length[i % 16 == 5] = 0
    at = rng.integers(0, (1 << 20) - 130, n)
    has = i % 16 != 11
    return Batch(_arena(seed), at[has], length[has], np.concatenate([[0], np.cumsum(has)]))


LONG_HOLE = (2 << 20) + 17


@functools.lru_cache(maxsize=None)
def spread(n, seed=12):
    """A2: per file a hole, then 1..200 real bytes at any residue; files 8 j + 3 have the two the
    other way round and files 16 j + 7 are the hole alone.  Hole lengths are log-uniform in
    0..16 KiB, file n // 3 has one of 2 MiB + 17 bytes.  That distribution ends at 260 blocks, which
    is 30 buckets at the most (md5_bucket has four per octave), so files 256 j + 9 take their hole
    log-uniform from 16 KiB..1 MiB instead: another six octaves at a cost of about 70 MB of zeros
    for hashlib at 70,001 files.  At the counts of the tests the block counts must occupy at least
    40 buckets and at least 100 of the 256 shares must hold 8 or more (spread_occupancy)."""
    rng = np.random.default_rng(seed * 1000003 + n)
    i = np.arange(n)
    hole = np.floor(2.0 ** rng.uniform(0, 14, n)).astype(np.int64) - 1
    ladder = i % 256 == 9
    hole[ladder] = np.floor(2.0 ** rng.uniform(14, 20, int(ladder.sum()))).astype(np.int64)
    hole[n // 3] = LONG_HOLE
    real_len, real_at = rng.integers(1, 201, n), rng.integers(0, (1 << 20) - 200, n)
    alone = i % 16 == 7
    turned = i % 8 == 3
    off = np.concatenate([[0], np.cumsum(np.where(alone, 1, 2))])
    seg_at, seg_len = np.full(off[-1], -1, dtype=np.int64), np.zeros(off[-1], dtype=np.int64)
    first = off[:-1]
    hole_seg = np.where(turned, first + 1, first)
    real_seg = np.where(turned, first, first + 1)[~alone]
    seg_len[hole_seg] = hole
    seg_at[real_seg], seg_len[real_seg] = real_at[~alone], real_len[~alone]
    b = Batch(_arena(seed), seg_at, seg_len, off)
    if n in SPREAD_COUNTS:
        buckets, wide = spread_occupancy(b)
        assert buckets >= 40 and wide >= 100, (n, buckets, wide)
    return b


def spread_occupancy(batch, final=True):
    """(distinct values of md5_bucket over the files' block counts, shares that hold 8 or more)."""
    blocks = batch.lengths // 64 + (np.where(batch.lengths % 64 < 56, 1, 2) if final else 0)
    uniq, inv = np.unique(blocks, return_inverse=True)
    bucket = np.array([md5_bucket(int(b)) for b in uniq])[inv]
    shares, per = shares_of(batch.n)
    wide = sum(1 for s in range(shares) if np.unique(bucket[s * per:(s + 1) * per]).size >= 8)
    return int(np.unique(bucket).size), wide


@functools.lru_cache(maxsize=None)
def head(n, seed=13):
    """A3's first call: per file one segment of 0..63 bytes (files 16 j + 2: no segment), so the
    state after INIT is (H0, length, the bytes) without any compression.  In spread(n)'s arena."""
    rng = np.random.default_rng(seed * 1000003 + n)
    i = np.arange(n)
    has = i % 16 != 2
    return Batch(spread(n).arena, rng.integers(0, (1 << 20) - 64, n)[has], rng.integers(0, 64, n)[has],
                 np.concatenate([[0], np.cumsum(has)]))


def head_states(batch):
    """The 96 n bytes of state after an INIT call of files shorter than 64 bytes, built in numpy."""
    assert batch.lengths.max() < 64 and (np.diff(batch.file_off.astype(np.int64)) <= 1).all()
    st = np.zeros(batch.n, dtype=mc.STATE)
    st["h"] = np.array(mc._H0, dtype=np.uint32)
    st["total"] = batch.lengths
    has = np.diff(batch.file_off.astype(np.int64)) == 1
    at = np.zeros(batch.n, dtype=np.int64)
    at[has] = batch.seg_at
    col = np.arange(64)
    take = batch.arena[np.minimum(at[:, None] + col, batch.arena.size - 1)]
    st["tail"] = np.where(col < batch.lengths[:, None], take, 0)
    return st.tobytes()


@functools.lru_cache(maxsize=None)
def two_call_digests(n):
    """hashlib over head(n)'s bytes followed by spread(n)'s, per file."""
    return b"".join(hashlib.md5(a + b).digest() for a, b in zip(head(n).contents(), spread(n).contents()))


# ---- the four-call loop (md5_cases.stream_four_calls) ----------------------------------------------------------
class Loop:
    """INIT, update, update, FINAL over one arena: the calls as Batches, the digests hashlib's of
    each file's bytes over all calls, the states the model's after the third call."""

    def __init__(self, arena, calls, want_states=None):
        self.arena, self.calls, self.n = arena, calls, calls[0].n
        parts = [c.contents() for c in calls]
        self.messages = [b"".join(p[f] for p in parts) for f in range(self.n)]
        self.lengths = np.array([len(m) for m in self.messages])
        self.digests = b"".join(hashlib.md5(m).digest() for m in self.messages)
        if want_states is None:
            want_states = b"".join(mc.State().update(b"".join(p[f] for p in parts[:-1])).pack() for f in range(self.n))
        self.states = want_states


@functools.lru_cache(maxsize=None)
def four_calls(n_bytes, n_files=48, seed=7):
    """stream_four_calls: every file the same content, the states the prefix at the third cut."""
    arena, content, calls, cuts = mc.stream_four_calls(n_bytes, n_files, seed)
    arena.setflags(write=False)
    prefixes = mc.prefix_states(content)
    loop = Loop(arena, [Batch.of_files(arena, c) for c in calls], b"".join(prefixes[c[3]].pack() for c in cuts))
    assert loop.digests == hashlib.md5(content).digest() * n_files
    return loop


def moved_boundary(loop, arena2):
    """The loop over other bytes and with one d_file_off entry of its second call one lower: the
    last segment of a file of two goes to the file behind it.  -> (Loop, file, new d_file_off)"""
    second = loop.calls[1]
    per = np.diff(second.file_off.astype(np.int64))
    f = int(np.flatnonzero((per[:-1] == 2) & (second.seg_len[second.file_off[1:-1].astype(np.int64) - 1] > 0))[0])
    off = second.file_off.copy()
    off[f + 1] -= 1
    calls = [Batch(arena2, c.seg_at, c.seg_len, c.file_off) for c in loop.calls]
    calls[1] = Batch(arena2, second.seg_at, second.seg_len, off)
    return Loop(arena2, calls), f, off


# ---- seeded states: totals that need the upper word of the bit length ----------------------------------------
# A hole-only file of N bytes just before the padding, {h, total} as tests/cpp/fuzz_md5.cpp prints
# them after walking the hole through md5_core.h, and hashlib's digest of N zero bytes
# (tests/test_md5_sanitized.py holds both to the program and to hashlib).
LONG_HOLES = {
    (1 << 29) - 1: ((1167939552, 2415650564, 3953036401, 344166272), "c6c4834a7b0928878ad48c867a1e24d6"),
    (1 << 29): ((4030756232, 2922712292, 1993860534, 371049071), "aa559b4e3523a6c931f08f4df52d58f2"),
    (1 << 29) + 57: ((4030756232, 2922712292, 1993860534, 371049071), "0ccd318f88830d9d2aaa95e416efd8b8"),
    (1 << 32) + 5: ((3173903626, 2891250690, 408419566, 1639655148), "968a8809aa0886d87f385d88733a98d2"),
}
SEED_TOTALS = [(1 << 29) - 64 + k for k in (0, 1, 55, 56, 63)] + [(1 << 32) - 1, (1 << 32) + 63, (1 << 61) - 1,
                                                                   M64 - 64 + 9]
SEED_COPIES = 8  # every seed as this many files, each with an update of its own length


def pack_state(s):
    """State.pack with total as the 64-bit field holds it: mod 2^64 (M64 - 64 + 9 plus 200 bytes
    wraps; total % 64 and total * 8 mod 2^64 are the same either way)."""
    return struct.pack("<4IQ", *s.h, s.total % M64) + s.tail.ljust(64, b"\0") + bytes(8)


class Seeded:
    """E2: files that start from a seeded state.  seeds[f] is the State, known[f] hashlib's digest
    of the seed finalised where hashlib can know it (LONG_HOLES), update the Batch of 0..200 bytes."""

    def __init__(self, seed=14):
        rng = np.random.default_rng(seed)
        kinds = [(tuple(int(x) for x in rng.integers(0, 1 << 32, 4)), t,
                  rng.integers(0, 256, t % 64, dtype=np.uint8).tobytes(), None) for t in SEED_TOTALS]
        kinds += [(h, n, bytes(n % 64), bytes.fromhex(d)) for n, (h, d) in LONG_HOLES.items()]
        self.seeds, self.known = [], []
        for h, total, tail, known in kinds:
            self.seeds += [mc.State(h, total, tail)] * SEED_COPIES
            self.known += [known] * SEED_COPIES
        self.n = len(self.seeds)
        self.totals = np.array([s.total for s in self.seeds], dtype=object)
        length = rng.integers(0, 201, self.n)
        length[0::SEED_COPIES], length[1::SEED_COPIES] = 0, 200
        arena = _arena(seed, 1 << 16)
        self.update = Batch(arena, rng.integers(0, (1 << 16) - 200, self.n), length, np.arange(self.n + 1))
        self.packed = b"".join(pack_state(s) for s in self.seeds)
        after = [s.update(c) for s, c in zip(self.seeds, self.update.contents())]
        self.final_alone = b"".join(s.digest() for s in self.seeds)
        self.after_packed = b"".join(pack_state(s) for s in after)
        self.after_final = b"".join(s.digest() for s in after)
        for s, k in zip(self.seeds, self.known):
            assert k is None or s.digest() == k


@functools.lru_cache(maxsize=None)
def seeded():
    return Seeded()


# ---- checkers -------------------------------------------------------------------------------------------------
def _rows(raw, width):
    return np.frombuffer(bytes(raw), dtype=np.uint8).reshape(-1, width)


def check_digests(got, want, lengths, what):
    """16 n bytes against 16 n bytes, per file index."""
    assert len(got) == len(want) == 16 * len(lengths), (what, len(got), len(want), len(lengths))
    g, w = _rows(got, 16), _rows(want, 16)
    bad = np.flatnonzero((g != w).any(axis=1))
    if bad.size:
        blank = int((g[bad] == SENTINEL).all(axis=1).sum())
        raise AssertionError(f"{what}: {bad.size} of {len(lengths)} digests differ ({blank} of them never written), "
                             f"first files {bad[:8].tolist()} (lengths {[int(lengths[i]) for i in bad[:8]]})")


def check_states(got, want, lengths, what):
    """96 n bytes against 96 n bytes, per file index; names the field that differs first."""
    assert len(got) == len(want) == 96 * len(lengths), (what, len(got), len(want), len(lengths))
    g, w = _rows(got, 96), _rows(want, 96)
    bad = np.flatnonzero((g != w).any(axis=1))
    if bad.size:
        f = int(bad[0])
        gs, ws = np.frombuffer(g[f].tobytes(), dtype=mc.STATE)[0], np.frombuffer(w[f].tobytes(), dtype=mc.STATE)[0]
        field = next(k for k in mc.STATE.names if not np.array_equal(gs[k], ws[k]))
        raise AssertionError(f"{what}: {bad.size} of {len(lengths)} states differ, first files {bad[:8].tolist()} "
                             f"(lengths {[int(lengths[i]) for i in bad[:8]]}); file {f} differs in {field}: "
                             f"got {gs[field].tolist()}, want {ws[field].tolist()}")


def guarded(be, n_bytes, fill=SENTINEL):
    """A buffer of n_bytes of `fill` between two guards; its payload is at .addr + GUARD."""
    return be.upload(_image(n_bytes, fill))


def unguard(be, buf, n_bytes, what):
    raw = be.read(buf)
    assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + n_bytes:] == CANARY).all(), f"{what}: a guard was written"
    return raw[GUARD:GUARD + n_bytes].tobytes()


# ---- runs: the same calls on the library and on the stand-in ---------------------------------------------------
def _place(be, batch, arena=None):
    """(segs address, offsets address, the buffers) of the batch with its arena uploaded (or at `arena`)."""
    arena = arena if arena is not None else be.upload(batch.arena)
    segs, off = batch.records(arena.addr)
    d_segs, d_off = (be.upload(segs) if batch.n_segs else None), be.upload(off)
    return d_segs.addr if d_segs else 0, d_off.addr, (arena, d_segs, d_off)


def _image(n_bytes, fill):
    image = np.full(n_bytes + 2 * GUARD, CANARY, dtype=np.uint8)
    image[GUARD:GUARD + n_bytes] = fill
    return image


class OneShot:
    """A batch placed for the one-shot form (INIT | FINAL, no state): queue() is the call alone, so
    a test can put it between other work on the backend's stream; check() is hashlib per file."""

    def __init__(self, be, batch, arena=None):
        self.be, self.batch = be, batch
        self.segs, self.off, self.keep = _place(be, batch, arena)
        self.out = guarded(be, 16 * batch.n)

    def reset(self):
        self.be.write(self.out, _image(16 * self.batch.n, SENTINEL))

    def queue(self):
        self.be.md5_batch(self.segs, self.off, self.batch.n, self.batch.n_segs, out=self.out.addr + GUARD)

    def check(self, what):
        batch = self.batch
        check_digests(unguard(self.be, self.out, 16 * batch.n, what), batch.digests, batch.lengths, what)


def run_one_shot(be, batch, what):
    """A1 / A2: every digest of the one-shot form against hashlib."""
    run = OneShot(be, batch)
    be.ready()
    run.queue()
    be.wait()
    run.check(what)


def run_two_calls(be, first, rest, want_digests, what):
    """A3: INIT over `first`, FINAL over `rest`, queued without a wait between them.  The states
    are read after both calls: they are the first call's, which FINAL leaves unchanged."""
    n = first.n
    arena = be.upload(first.arena)
    assert rest.arena is first.arena and rest.n == n
    s1, o1, keep1 = _place(be, first, arena)
    s2, o2, keep2 = _place(be, rest, arena)
    state, out = guarded(be, 96 * n, 0xA5), guarded(be, 16 * n)
    be.ready()
    be.md5_batch(s1, o1, n, first.n_segs, state=state.addr + GUARD, flags=mc.INIT)
    be.md5_batch(s2, o2, n, rest.n_segs, out=out.addr + GUARD, state=state.addr + GUARD, flags=mc.FINAL)
    be.wait()
    lengths = first.lengths + rest.lengths
    check_states(unguard(be, state, 96 * n, what), head_states(first), first.lengths, f"{what}: states after INIT and FINAL")
    check_digests(unguard(be, out, 16 * n, what), want_digests, lengths, what)


class LoopRun:
    """A Loop with every call's records resident: queue() puts INIT, the updates and FINAL onto the
    backend's stream with no host step between them (wait_each: the twin that waits after each)."""

    def __init__(self, be, loop):
        self.be, self.loop, self.n = be, loop, loop.n
        self.arena = be.upload(loop.arena)
        self.placed = [_place(be, c, self.arena) for c in loop.calls]
        self.state, self.out = guarded(be, 96 * self.n, 0xA5), guarded(be, 16 * self.n)

    def reset(self):
        """The sentinel back into d_out, 0xA5 into d_state (INIT must not read it)."""
        self.be.write(self.state, _image(96 * self.n, 0xA5))
        self.be.write(self.out, _image(16 * self.n, SENTINEL))

    def queue(self, wait_each=False):
        for k, (c, (segs, off, _)) in enumerate(zip(self.loop.calls, self.placed)):
            flags = mc.INIT if k == 0 else mc.FINAL if k == len(self.placed) - 1 else 0
            self.be.md5_batch(segs, off, self.n, c.n_segs, out=self.out.addr + GUARD, state=self.state.addr + GUARD,
                              flags=flags)
            if wait_each:
                self.be.wait()

    def check(self, what, loop=None):
        """Digests against hashlib, states against the model after the last call but one (FINAL
        leaves them).  `loop`: what the records and bytes have been rewritten to.  -> the output bytes"""
        loop = loop or self.loop
        got_out, got_state = unguard(self.be, self.out, 16 * self.n, what), unguard(self.be, self.state, 96 * self.n, what)
        check_digests(got_out, loop.digests, loop.lengths, what)
        check_states(got_state, loop.states, loop.lengths, f"{what}: states after the last call but one")
        return got_out + got_state


def run_loop(be, loop, what, wait_each=False):
    """B1: the four calls queued, one wait, everything checked.  -> the output bytes (digests + states)"""
    run = LoopRun(be, loop)
    be.ready()
    run.queue(wait_each)
    be.wait()
    return run.check(what)


def run_seeded(be, case, what):
    """E2: FINAL alone; an update, then FINAL, queued; an update alone."""
    n, zero_off = case.n, be.upload(np.zeros(case.n + 1, dtype=np.uint64))
    segs, off, keep = _place(be, case.update)
    states = [guarded(be, 96 * n, 0xA5) for _ in range(3)]
    outs = [guarded(be, 16 * n) for _ in range(2)]
    seeds = np.frombuffer(case.packed, dtype=np.uint8)
    for s in states:
        be.write(s, seeds, GUARD)
    be.ready()
    be.md5_batch(0, zero_off.addr, n, 0, out=outs[0].addr + GUARD, state=states[0].addr + GUARD, flags=mc.FINAL)
    be.md5_batch(segs, off, n, case.update.n_segs, state=states[1].addr + GUARD, flags=0)
    be.md5_batch(0, zero_off.addr, n, 0, out=outs[1].addr + GUARD, state=states[1].addr + GUARD, flags=mc.FINAL)
    be.md5_batch(segs, off, n, case.update.n_segs, state=states[2].addr + GUARD, flags=0)
    be.wait()
    names = [f"total {t % M64:#x}" for t in case.totals]
    label = lambda form: f"{what}, {form} (seeds of files 0, {SEED_COPIES}, ..: {names[::SEED_COPIES]})"  # noqa: E731
    check_digests(unguard(be, outs[0], 16 * n, what), case.final_alone, case.update.lengths * 0, label("FINAL alone"))
    check_states(unguard(be, states[0], 96 * n, what), case.packed, case.update.lengths * 0, label("FINAL alone: d_state"))
    check_digests(unguard(be, outs[1], 16 * n, what), case.after_final, case.update.lengths, label("update, FINAL"))
    check_states(unguard(be, states[1], 96 * n, what), case.after_packed, case.update.lengths, label("update, FINAL: d_state"))
    check_states(unguard(be, states[2], 96 * n, what), case.after_packed, case.update.lengths, label("update alone"))


# ---- the stand-in library ------------------------------------------------------------------------------------
class HostBuf:
    def __init__(self, addr, a):
        self.addr, self.a = addr, a


FAULTS = ("second_tile_skipped", "place_doubled", "offsets_stop_at_2^20", "state_of_two_calls_earlier",
          "total_32_bits", "final_writes_state")


class StandIn:
    """hf3fs_crc_md5_batch made of hashlib and md5_cases.State over host memory: it reads the same
    record arrays, at made-up addresses, that the GPU gets.  `fault` makes it wrong in one way:
      second_tile_skipped         the files of every share's second 64-file tile are never taken
      place_doubled               one place of the permutation names its neighbour's file: one file
                                  is written twice, one never
      offsets_stop_at_2^20        files from 2^20 on are never taken
      state_of_two_calls_earlier  a call reads d_state as it was before the previous call wrote it
      total_32_bits               the byte count is kept in 32 bits
      final_writes_state          FINAL stores the state it padded from"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault, self.bufs, self.next, self.before = fault, [], 0x7F0000000000, []

    # -- the backend the runs use
    def upload(self, array):
        a = np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()
        buf = HostBuf(self.next, a)
        self.bufs.append(buf)
        self.next += (a.size + 4096 + 255) // 256 * 256
        return buf

    def write(self, buf, array, at=0):
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        buf.a[at:at + raw.size] = raw

    def read(self, buf):
        return buf.a.copy()

    def ready(self):
        pass

    def wait(self):
        pass

    # -- the call
    def _mem(self, addr, n_bytes):
        k = bisect.bisect_right([b.addr for b in self.bufs], addr) - 1
        assert k >= 0 and addr + n_bytes <= self.bufs[k].addr + self.bufs[k].a.size, "an address outside every buffer"
        at = addr - self.bufs[k].addr
        return self.bufs[k].a[at:at + n_bytes]

    def _taken(self, n):
        files = np.arange(n)
        if self.fault == "second_tile_skipped":
            files = files[files % shares_of(n)[1] // TILE != 1]
        elif self.fault == "place_doubled":
            files = files[files != n // 2]
        elif self.fault == "offsets_stop_at_2^20":
            files = files[files < 1 << 20]
        return files

    def _messages(self, segs, off, n, n_segs, files):
        seg = self._mem(segs, 16 * n_segs).view(mc.SEG) if n_segs else np.zeros(0, dtype=mc.SEG)
        bounds = np.minimum(self._mem(off, 8 * (n + 1)).view("<u8"), n_segs).tolist()
        data, ln = seg["data"].astype(np.int64), seg["length"].tolist()
        bases = np.array([b.addr for b in self.bufs])
        which = np.where(data == 0, -1, np.searchsorted(bases, data, side="right") - 1)
        rel = (data - bases[np.maximum(which, 0)]).tolist()
        raws = {int(k): self.bufs[int(k)].a.tobytes() for k in np.unique(which) if k >= 0}
        for k in raws:
            inside = which == k
            assert (np.asarray(rel)[inside] + seg["length"][inside].astype(np.int64) <= len(raws[k])).all()
        which = which.tolist()
        for f in files:
            parts = [bytes(ln[k]) if which[k] < 0 else raws[which[k]][rel[k]:rel[k] + ln[k]]
                     for k in range(bounds[f], bounds[f + 1])]
            yield parts[0] if len(parts) == 1 else b"".join(parts)

    def md5_batch(self, segs, off, n, n_segs, out=0, state=0, flags=BOTH):
        init, final = bool(flags & mc.INIT), bool(flags & mc.FINAL)
        assert off and (segs or not n_segs) and (state or flags == BOTH) and (out or not final)
        files = self._taken(n).tolist()
        st = self._mem(state, 96 * n).reshape(n, 96) if state else None
        read = st
        if state and not init:
            if self.fault == "state_of_two_calls_earlier" and self.before:
                read = self.before[-1]
        if state:
            self.before.append(st.copy())
        digests, states = [], []
        if init and final:  # the one-shot form, 10^6 files of it: hashlib and nothing else per file
            digests = [hashlib.md5(m).digest() for m in self._messages(segs, off, n, n_segs, files)]
            self._mem(out, 16 * n).reshape(n, 16)[files] = _rows(b"".join(digests), 16)
            return
        for f, msg in zip(files, self._messages(segs, off, n, n_segs, files)):
            if init:
                s = mc.State()
            else:
                s = mc.State.unpack(read[f].tobytes())
                if self.fault == "total_32_bits":
                    s = mc.State(s.h, s.total % 2 ** 32, s.tail)
            if final and s.total < 64 and s.h == mc._H0:
                digests.append(hashlib.md5(s.tail + msg).digest())  # nothing compressed yet: hashlib from the start
                if self.fault == "final_writes_state":  # (h as it came: any write is the fault, and
                    rest = (s.tail + msg)[-((s.total + len(msg)) % 64) or len(s.tail + msg):]  # Python is slow)
                    states.append(pack_state(mc.State(s.h, s.total + len(msg), rest)))
                continue
            s = s.update(msg)
            if self.fault == "total_32_bits":
                s = mc.State(s.h, s.total % 2 ** 32, s.tail)
            if final:
                digests.append(s.digest())
            if not final or self.fault == "final_writes_state":
                states.append(pack_state(s))
        if digests:
            self._mem(out, 16 * n).reshape(n, 16)[files] = _rows(b"".join(digests), 16)
        if states:
            st[files] = _rows(b"".join(states), 96)
