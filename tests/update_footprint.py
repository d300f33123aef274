"""Write-footprint model of hf3fs_crc_update_batch, shared by tests/test_gpu_update_footprint.py
(the HIP library) and tests/test_update_footprint_model.py (numpy stand-ins that check the checker);
tests/stream_queue.py builds its queued rounds from the same scenarios and checkers.

Every buffer the call may touch sits inside a canary -- a never-zero function of the byte
position that differs between neighbouring bytes and neighbouring 16-byte granules -- so a
zero-fill, a shifted copy or a repeated granule anywhere outside what the IO owns changes a
byte the expected image still holds:

  chunk arena    chunk c owns max_len bytes at bases[c] (residue c % 16, offsets inside the
                 1/4/8/16 KiB lines varied), regions `gap` bytes of canary apart, MARGIN at both
                 ends.  The expected image starts as the canary; the oracle's chunk bytearrays
                 are initialised from it, so after a round the WHOLE bytearray (not [:size]) is
                 the expected content of the region: ChunkReplica::update restated writes the
                 payload and the zero gap and nothing else, and nothing at all for a failed IO.
  payload arena  payloads placed so that (src - dst) mod 16 is what the case asks for.
  record buffer  the IO records with REC_GUARD bytes of canary before and after.

Numpy only: no GPU, no torch.  Addresses in a Scenario are relative to the arenas; a backend
(`start`, `step`) adds its own.
"""
import bisect

import numpy as np

MARGIN = 64 << 10      # 4 x the largest unit one workgroup writes at a time (4 x 256 x 16 B; a 16 KiB piece)
REC_GUARD = 4 << 10
PAY_GUARD = 4 << 10
SALT_CHUNKS, SALT_PAYLOAD, SALT_RECORDS = 0, 0x51, 0xA7  # the three canaries differ byte for byte

WRITE, TRUNCATE, EXTEND = 1, 4, 8                  # HF3FS_UPDATE_*
OK, INVALID_ARG, CHECKSUM_MISMATCH = 0, 3, 4080    # status codes (include/hf3fs_crc.h)
NONE, CRC32C, CRC32 = 0, 1, 2
FLAG_ENGINE = 1
M32 = 0xFFFFFFFF

# hf3fs_crc_update_io (include/hf3fs_crc.h; the model test compares the offsets with the ctypes mirror)
REC = np.dtype([("chunk", "<u8"), ("payload", "<u8"), ("offset", "<u4"), ("length", "<u4"), ("chunk_size", "<u4"),
                ("update_type", "u1"), ("chunk_checksum_type", "u1"), ("write_checksum_type", "u1"), ("flags", "u1"),
                ("chunk_checksum", "<u4"), ("write_checksum", "<u4"), ("out_size", "<u4"), ("out_checksum", "<u4"),
                ("out_checksum_type", "u1"), ("checksum_case", "u1"), ("reserved1", "u1", (2,)), ("status", "<i4")])
assert REC.itemsize == 56
OUTPUT_FIELDS = ("out_size", "out_checksum", "out_checksum_type", "checksum_case", "status")


def canary(n, salt=0):
    """Byte i = ((i + salt) * 0x9E3779B1 >> 24) | 1: never zero; consecutive positions step by
    0x9E.37 in the byte, positions 16 apart by 0xE3.77, so neither neighbours nor granules repeat."""
    i = np.arange(salt, salt + n, dtype=np.uint64)
    return ((((i * np.uint64(0x9E3779B1)) >> np.uint64(24)) & np.uint64(0xFF)) | np.uint64(1)).astype(np.uint8)


def _input_mask():
    m = np.ones(REC.itemsize, dtype=bool)
    for f in OUTPUT_FIELDS:
        dt, off = REC.fields[f][:2]
        m[off:off + dt.itemsize] = False
    return m


INPUT_MASK = _input_mask()


def _field_at(byte):
    for name in REC.names:
        dt, off = REC.fields[name][:2]
        if off <= byte < off + dt.itemsize:
            return name
    return "?"


class Layout:
    """Chunk regions inside the arena (offsets; the arena itself starts on a 16 KiB line)."""

    def __init__(self, n, max_len, gap):
        self.n, self.max_len, self.gap = n, max_len, gap
        self.bases = []
        cur = MARGIN
        for c in range(n):
            b = ((cur + 15) & ~15) + 16 * ((c * 389 + 7) % 1024) + c % 16
            self.bases.append(b)
            cur = b + max_len + gap
        self.size = (self.bases[-1] + max_len + MARGIN + 15) & ~15
        for c, b in enumerate(self.bases):
            assert b % 16 == c % 16
            assert c == 0 or b - (self.bases[c - 1] + max_len) >= gap
        for line in (1 << 10, 4 << 10, 8 << 10, 16 << 10):
            assert len({b % line for b in self.bases}) >= min(n, 16), line

    def where(self, pos, sizes=None):
        """Which chunk, guard or margin arena offset `pos` falls in."""
        c = bisect.bisect_right(self.bases, pos) - 1
        if c < 0:
            return f"head margin, {self.bases[0] - pos} B before chunk 0"
        rel = pos - self.bases[c]
        if rel < self.max_len:
            side = ""
            if sizes is not None:
                side = f" (below its new size {sizes[c]})" if rel < sizes[c] else f" (tail past its new size {sizes[c]})"
            return f"chunk {c} +{rel}{side}"
        past = rel - self.max_len
        if c == self.n - 1:
            return f"tail margin, {past} B past the region of chunk {c}"
        return f"guard after chunk {c}: {past} B past its region, {self.bases[c + 1] - pos} B before chunk {c + 1}"


class Round:
    pass


class Scenario:
    """A fixed sequence of update batches over n chunks and what ChunkReplica::update restated
    (oracle.replica_apply; engine=True: oracle.engine_apply) leaves in every byte of the arena."""

    def __init__(self, orc, n, max_len, gap, ctype=CRC32C, engine=False):
        self.orc, self.n, self.max_len, self.ctype, self.engine = orc, n, max_len, ctype, engine
        self.lay = Layout(n, max_len, gap)
        self.canary = canary(self.lay.size, SALT_CHUNKS)
        self.chunks = [bytearray(self.canary[b:b + max_len].tobytes()) for b in self.lay.bases]
        self.sizes = [0] * n
        self.cks = [(ctype, 0)] * n            # replica: (type, raw value)
        self.fins = [0] * n                    # engine: finalized CRC32C
        self.exists = [False] * n
        self.regions0 = None
        self.rounds = []
        self.pay_size = 0

    # -- building ------------------------------------------------------------------------------
    def preset(self, c, data):
        """Chunk c starts with `data` as its content (before the first round)."""
        assert not self.rounds and not self.engine
        self.chunks[c][:len(data)] = data
        self.sizes[c] = len(data)
        self.cks[c] = tuple(self.orc.create(self.ctype, data)) if data else (self.ctype, 0)

    def _regions(self):
        return np.stack([np.frombuffer(bytes(ch), dtype=np.uint8) for ch in self.chunks])

    def add_round(self, ops, rng):
        """ops[c]: ("W", off, ln, shift, corrupt[, without]) | ("T", target) | ("E", target);
        shift = (payload address - destination address) mod 16."""
        assert len(ops) == self.n
        if self.regions0 is None:
            self.regions0 = self._regions()
        r = Round()
        r.ops = ops
        r.sizes_before = list(self.sizes)
        rec = np.zeros(self.n, dtype=REC)
        has_payload = np.zeros(self.n, dtype=bool)
        placed, cur = [], PAY_GUARD
        expect = []
        for c, op in enumerate(ops):
            u = rec[c]
            u["chunk"] = self.lay.bases[c]
            u["chunk_size"] = self.sizes[c]
            if self.engine:
                u["chunk_checksum_type"], u["chunk_checksum"] = CRC32C, (~self.fins[c]) & M32
                u["flags"] = FLAG_ENGINE
            else:
                u["chunk_checksum_type"], u["chunk_checksum"] = self.cks[c]
            if op[0] in "TE":
                kind = TRUNCATE if op[0] == "T" else EXTEND
                u["update_type"], u["offset"], u["length"] = kind, 0, int(op[1])
                if self.engine:
                    expect.append(self.orc.engine_apply(self.chunks[c], self.sizes[c], self.fins[c], b"", int(op[1]),
                                                        self.max_len, truncate=op[0] == "T", with_case=True))
                else:
                    expect.append(self.orc.replica_apply(self.chunks[c], self.sizes[c], self.cks[c], kind, 0,
                                                         int(op[1]), with_case=True))
                continue
            off, ln, shift, corrupt = int(op[1]), int(op[2]), int(op[3]), bool(op[4])
            without = len(op) > 5 and bool(op[5])
            data = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
            p = ((cur + 15) & ~15) + (self.lay.bases[c] + off + shift) % 16
            placed.append((p, data))
            cur = p + ln + 256
            has_payload[c] = True
            u["update_type"], u["offset"], u["length"], u["payload"] = WRITE, off, ln, p
            if self.engine:
                fin = self.orc.rs_crc32c(data) ^ (0x100 if corrupt else 0)
                if without:
                    u["write_checksum_type"], u["write_checksum"] = NONE, 0
                else:
                    u["write_checksum_type"], u["write_checksum"] = CRC32C, (~fin) & M32
                expect.append(self.orc.engine_apply(self.chunks[c], self.sizes[c], self.fins[c], data, off,
                                                    self.max_len, exists=self.exists[c], data_ck=fin, with_case=True))
            else:
                wck = tuple(self.orc.create(self.ctype, data))
                if corrupt:
                    wck = (wck[0], wck[1] ^ 0x10)
                u["write_checksum_type"], u["write_checksum"] = wck
                expect.append(self.orc.replica_apply(self.chunks[c], self.sizes[c], self.cks[c], WRITE, off, ln,
                                                     data, wck, chunk_size=self.max_len, with_case=True))
        pay = canary(cur + PAY_GUARD, SALT_PAYLOAD)
        for p, data in placed:
            pay[p:p + len(data)] = np.frombuffer(data, dtype=np.uint8)
        self.pay_size = max(self.pay_size, pay.size)
        for c, e in enumerate(expect):  # the state the next round starts from
            if self.engine:
                if e[0] == OK:
                    self.sizes[c], self.fins[c], self.exists[c] = e[1], e[2], True
            else:
                self.sizes[c], self.cks[c] = e[1], tuple(e[2])
        r.rec, r.has_payload, r.pay, r.expect = rec, has_payload, pay, expect
        r.regions = self._regions()
        r.sizes_after = list(self.sizes)
        self.rounds.append(r)
        return r

    # -- images --------------------------------------------------------------------------------
    def image(self, regions):
        img = self.canary.copy()
        for c, b in enumerate(self.lay.bases):
            img[b:b + self.max_len] = regions[c]
        return img

    def image_before(self, k):
        return self.image(self.regions0) if k == 0 else self.image_after(k - 1)

    def image_after(self, k):
        """The expected arena after round k (kept: every variant of a case compares with it)."""
        r = self.rounds[k]
        if getattr(r, "image", None) is None:
            r.image = self.image(r.regions)
            r.image.setflags(write=False)
        return r.image

    def payload_image(self, k):
        r = self.rounds[k]
        if getattr(r, "pay_full", None) is None or r.pay_full.size != self.pay_size:
            r.pay_full = canary(self.pay_size, SALT_PAYLOAD)
            r.pay_full[:r.pay.size] = r.pay
            r.pay_full.setflags(write=False)
        return r.pay_full

    def record_buffer(self, k, chunk_addr, pay_addr):
        """The record array of round k with absolute addresses, inside its canary buffer."""
        r = self.rounds[k]
        rec = r.rec.copy()
        rec["chunk"] += np.uint64(chunk_addr)
        rec["payload"][r.has_payload] += np.uint64(pay_addr)
        buf = canary(2 * REC_GUARD + rec.nbytes, SALT_RECORDS)
        buf[REC_GUARD:REC_GUARD + rec.nbytes] = rec.view(np.uint8)
        return buf


# ---- the checker ------------------------------------------------------------------------------
def _diff(got, want):
    d = np.flatnonzero(got != want)
    return int(d[0]), int(d[-1]), int(d.size)


def check_arena(scn, k, got_arena):
    """The whole chunk arena against the oracle's image after round k."""
    r, lay = scn.rounds[k], scn.lay
    want = scn.image_after(k)
    assert got_arena.shape == want.shape
    if not np.array_equal(got_arena, want):
        first, last, cnt = _diff(got_arena, want)
        raise AssertionError(
            f"round {k}: chunk arena differs in {cnt} bytes; first at arena offset {first} = "
            f"{lay.where(first, r.sizes_after)} (got {int(got_arena[first]):#04x}, want {int(want[first]):#04x}), "
            f"last at {last} = {lay.where(last, r.sizes_after)}; ops {r.ops[_chunk_of(lay, first)]!r} / "
            f"{r.ops[_chunk_of(lay, last)]!r}")


def check_payload(scn, k, got_pay):
    """Round k's payload arena is unchanged."""
    want_pay = scn.payload_image(k)
    if not np.array_equal(got_pay, want_pay):
        first, last, cnt = _diff(got_pay, want_pay)
        raise AssertionError(f"round {k}: payload arena changed in {cnt} bytes, offsets {first}..{last}")


def check_records(scn, k, got_recbuf, sent_recbuf, n=None):
    """Round k's record buffer: both guards and every input field as sent, every output field what
    the oracle expects.  n: the batch held only the records of chunks 0..n-1 (default: all)."""
    r = scn.rounds[k]
    n = scn.n if n is None else n
    nb = n * REC.itemsize
    assert got_recbuf.shape == sent_recbuf.shape == (2 * REC_GUARD + nb,)
    for name, sl, edge in (("before", slice(0, REC_GUARD), "in front of the record of chunk 0"),
                           ("after", slice(REC_GUARD + nb, None), f"behind the record of chunk {n - 1}")):
        if not np.array_equal(got_recbuf[sl], sent_recbuf[sl]):
            first, last, cnt = _diff(got_recbuf[sl], sent_recbuf[sl])
            raise AssertionError(f"round {k}: record guard {name} the array changed in {cnt} bytes, "
                                 f"guard offsets {first}..{last} ({edge})")
    got_b = got_recbuf[REC_GUARD:REC_GUARD + nb].reshape(n, REC.itemsize)
    sent_b = sent_recbuf[REC_GUARD:REC_GUARD + nb].reshape(n, REC.itemsize)
    bad = (got_b != sent_b) & INPUT_MASK[None, :]
    if bad.any():
        i, byte = (int(x[0]) for x in np.nonzero(bad))
        raise AssertionError(f"round {k}: record {i} input field {_field_at(byte)} changed (byte {byte}: sent "
                             f"{int(sent_b[i, byte]):#04x}, got {int(got_b[i, byte]):#04x})")
    res = np.frombuffer(got_b.tobytes(), dtype=REC)
    for c in range(n):
        e, g, what = r.expect[c], res[c], f"round {k}: chunk {c} {r.ops[c]!r}"
        assert int(g["status"]) == e[0], (what, "status", int(g["status"]), e)
        assert int(g["checksum_case"]) == e[3], (what, "case", int(g["checksum_case"]), e)
        if scn.engine:
            if e[0] == OK:
                assert int(g["out_size"]) == e[1], (what, "size", int(g["out_size"]), e)
                assert int(g["out_checksum_type"]) == CRC32C, (what, "type")
                assert (~int(g["out_checksum"])) & M32 == e[2], (what, "checksum", hex(int(g["out_checksum"])), e)
        else:
            assert int(g["out_size"]) == e[1], (what, "size", int(g["out_size"]), e)
            assert (int(g["out_checksum_type"]), int(g["out_checksum"])) == tuple(e[2]), (what, "checksum", e)


def check_round(scn, k, got_arena, got_pay, got_recbuf, sent_recbuf):
    """Everything the call may and may not have changed in round k (raises AssertionError)."""
    check_arena(scn, k, got_arena)
    check_payload(scn, k, got_pay)
    check_records(scn, k, got_recbuf, sent_recbuf)


def _chunk_of(lay, pos):
    return max(0, bisect.bisect_right(lay.bases, pos) - 1)


def run_scenario(scn, backend, rounds=None):
    """Drive `backend` through the scenario, checking every byte after every batch.
    backend.start(arena_image, pay_size, recbuf_size) -> (chunk_addr, pay_addr);
    backend.step(pay_image, recbuf, n, max_len) -> (arena, pay, recbuf) as numpy arrays."""
    nb = 2 * REC_GUARD + scn.n * REC.itemsize
    chunk_addr, pay_addr = backend.start(scn.image_before(0), scn.pay_size, nb)
    assert chunk_addr % (16 << 10) == 0, "the arena starts on a 16 KiB line (Layout's offsets are address residues)"
    assert pay_addr % 16 == 0
    for k in range(len(scn.rounds) if rounds is None else rounds):
        sent = scn.record_buffer(k, chunk_addr, pay_addr)
        got = backend.step(scn.payload_image(k), sent.copy(), scn.n, scn.max_len)
        check_round(scn, k, got[0], got[1], got[2], sent)


# ---- the update pipelines a GPU backend can be run under -------------------------------------
def set_pipeline(opts, pipeline):
    """opts(name, value) sets a library switch (conftest's `opts`).  The option sets of
    test_gpu_parity.py's _set_pipeline; "ticketed": the three-pass pipeline
    with the ticketed apply on every call; "oneshot<K>": one-shot apply, K KiB pieces, every call."""
    opts("update_pipeline", "fused" if pipeline == "fused" else "unfused")
    if pipeline == "ticketed":
        opts("apply_grid", 0)
    if pipeline == "unfused_fine":
        opts("apply_grid", 0)
        opts("apply_pieces", 64)
        opts("apply_min_kib", 1)
    if pipeline == "oneshot_loop":
        opts("apply_grid", 2)
        opts("apply_piece_kib", 4)
    if pipeline.startswith("oneshot") and pipeline != "oneshot_loop":
        opts("apply_grid", 1)
        opts("apply_piece_kib", int(pipeline[len("oneshot"):]))


# ---- the cases ----------------------------------------------------------------------------------
def _random_ios(rng, n_chunks, chunk_size, sizes, cks, pattern):
    """tests/test_gpu_parity.py's generator, unchanged."""
    ios = []
    for c in range(n_chunks):
        size = sizes[c]
        r = rng.random()
        if pattern == "mixed" and r < 0.08:
            ios.append(("T", rng.integers(0, chunk_size + 1)))
        elif pattern == "mixed" and r < 0.12:
            ios.append(("E", rng.integers(0, chunk_size + 1)))
        else:
            if pattern == "seq" or r < 0.3:
                off = size
            else:
                off = int(rng.integers(0, chunk_size))
            if off >= chunk_size:
                off = int(rng.integers(0, chunk_size))
            ln = int(rng.integers(1, chunk_size - off + 1))
            ln = min(ln, max(1, int(rng.integers(1, chunk_size // 2 + 2))))
            ios.append(("W", off, ln))
    return ios


TINY_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47)


def tiny_scenario(orc, ctype=CRC32C):
    """B1: one batch on empty or short 4 KiB chunks.  IO k < 160: length TINY_LENGTHS[k % 10],
    destination residue k // 10 (through base residue k % 16 and the offset), source residue
    (7 k + 3) % 16, one of four kinds by k % 4: a write into an empty chunk behind a gap from 0,
    an append, a write past the size (a gap that starts at residue (k // 4) % 16), an overwrite
    inside the content.  IOs 160..175 end exactly at max_len."""
    max_len, n = 4096, 176
    scn = Scenario(orc, n, max_len, gap=2048, ctype=ctype)
    rng = np.random.default_rng(0xB1 + ctype)
    ops = []
    for k in range(n):
        base_res = k % 16
        if k >= 160:
            ln = TINY_LENGTHS[k % 10] if k % 2 else 16 * (k - 159) + k % 3
            size = 0 if k % 4 == 0 else max_len - ln - (k % 5) * 7   # append (k % 5 == 0) or gap up to the last bytes
            size = max(size, 0)
            if size:
                scn.preset(k, rng.integers(0, 256, size, dtype=np.uint8).tobytes())
            ops.append(("W", max_len - ln, ln, (7 * k + 3 - (base_res + max_len - ln)) % 16, False))
            continue
        ln, want_res, kind = TINY_LENGTHS[k % 10], k // 10, k % 4
        lift = (want_res - base_res) % 16  # offsets of this residue put dst on want_res
        if kind == 0:
            size, off = 0, lift + 16 * (1 + k % 7)
        elif kind == 1:
            size = off = (lift + 16 * (k % 5)) or 16   # (an append needs content: never at offset 0)
        elif kind == 2:
            size = ((k // 4) - base_res) % 16 + 16 * (k % 3)   # gap starts at residue (k // 4) % 16
            off = lift + 16 * (size // 16 + 1 + k % 6)
        else:
            size = lift + 16 * (2 + k % 4) + ln + k % 9
            off = lift + 16 * (k % 2)
        if size:
            scn.preset(k, rng.integers(0, 256, size, dtype=np.uint8).tobytes())
        src_res = (7 * k + 3) % 16
        ops.append(("W", off, ln, (src_res - (base_res + off)) % 16, False))
    scn.add_round(ops, rng)
    return scn


def tiny_coverage(scn):
    """Residue sets the tiny case reaches: destination, source, gap start, gap end, and ends at max_len."""
    r, lay = scn.rounds[0], scn.lay
    dst, src, g0, g1, at_end = set(), set(), set(), set(), 0
    for c, op in enumerate(r.ops):
        off, ln, shift = op[1], op[2], op[3]
        d = lay.bases[c] + off
        dst.add(d % 16)
        src.add((d + shift) % 16)
        assert int(r.rec[c]["payload"]) % 16 == (d + shift) % 16
        if off > r.sizes_before[c]:
            g0.add((lay.bases[c] + r.sizes_before[c]) % 16)
            g1.add(d % 16)
        at_end += off + ln == scn.max_len
    return dst, src, g0, g1, at_end


ROW_GRANULES = (831, 832, 833, 1855, 1856, 1857, 3135, 3136, 3137, 7231, 7232, 7233)
ROW_EDGES = tuple((h, t) for h in (0, 1, 15) for t in (0, 1, 15))


def rows_shapes(lay):
    """B2's 48 write shapes (off, ln, shift) for the chunks of `lay`: 36 with ROW_GRANULES[k % 12]
    full destination granules between a head of h and a tail of t bytes (ROW_EDGES[k % 9]); the
    first 24 of them put their first full granule on a 1 KiB destination line, where the copy
    loops' unrolled rows begin, so the count is the rows' own.  Then for each cut size P in 4, 8,
    16 KiB four writes around destination addresses that are multiples of P: across one line,
    across two, ending one byte before a line, ending one byte after it.  shift = k % 16."""
    shapes = []
    for k in range(36):
        ng, (h, t) = ROW_GRANULES[k % 12], ROW_EDGES[k % 9]
        if k < 24:
            off = (-h - lay.bases[k]) % 1024 + 1024 * (k % 3)   # dst + h on a 1 KiB line
        else:
            off = (-h - lay.bases[k]) % 16 + 16 * (1 + k % 5)   # dst = 16 m - h: the head is h bytes
        shapes.append((off, h + 16 * ng + t, k % 16))
    for j, P in enumerate((4 << 10, 8 << 10, 16 << 10)):
        for q in range(4):
            k = 36 + 4 * j + q
            cut = (lay.bases[k] // P + 2) * P - lay.bases[k]   # chunk offset of a destination multiple of P
            if q == 0:
                off, ln = cut - 100 - k, 200 + k          # across one line
            elif q == 1:
                off, ln = cut - 100 - k, P + 200 + k      # across two
            elif q == 2:
                off, ln = cut - 3000 - k, 3000 + k - 1    # ends one byte before the line
            else:
                off, ln = cut - 3000 - k, 3000 + k + 1    # ends one byte after it
            shapes.append((off, ln, k % 16))
    return shapes


def rows_scenario(orc, ctype=CRC32C):
    """B2: two batches of the rows_shapes writes over 192 KiB chunks: the first on empty chunks
    (every write with off > 0 sits behind a zero gap), the second at the same destinations with
    the source shifted on by 5, over the content of the first (old bytes under every write)."""
    n, max_len = 48, 192 << 10
    scn = Scenario(orc, n, max_len, gap=MARGIN, ctype=ctype)
    rng = np.random.default_rng(0xB2 + ctype)
    shapes = rows_shapes(scn.lay)
    scn.add_round([("W", off, ln, sh, False) for off, ln, sh in shapes], rng)
    scn.add_round([("W", off, ln, (sh + 5) % 16, False) for off, ln, sh in shapes], rng)
    return scn


def rounds_scenario(orc, ctype=CRC32C, n=32, max_len=128 << 10, rounds=6, seed=0xB3):
    """B3: `rounds` batches of _random_ios "mixed" traffic (writes, appends, gaps, truncates,
    extends); 9 % of the writes carry a corrupted client checksum; three IOs per round are
    INVALID_ARG (offset >= max_len, offset + length > max_len twice)."""
    scn = Scenario(orc, n, max_len, gap=MARGIN, ctype=ctype)
    rng = np.random.default_rng(seed + ctype)
    for rnd in range(rounds):
        ops = []
        for io in _random_ios(rng, n, max_len, scn.sizes, scn.cks, "mixed"):
            if io[0] == "W":
                ops.append(("W", io[1], io[2], int(rng.integers(0, 16)), rng.random() < 0.09))
            else:
                ops.append((io[0], int(io[1])))
        bad = rng.choice(n, 3, replace=False)
        ops[bad[0]] = ("W", max_len + int(rng.integers(0, 100)), 5, rnd, False)
        ops[bad[1]] = ("W", max_len - 10, 11 + int(rng.integers(0, 50)), rnd + 1, False)
        ops[bad[2]] = ("W", int(rng.integers(1, max_len)), max_len, rnd + 2, False)
        scn.add_round(ops, rng)
    return scn


def engine_scenario(orc, n=32, cap=64 << 10, rounds=6, seed=0xB4):
    """B4: chunk-engine IOs built as test_update_engine_flag_vs_engine_oracle builds them."""
    scn = Scenario(orc, n, cap, gap=MARGIN, ctype=CRC32C, engine=True)
    rng = np.random.default_rng(seed)
    for _ in range(rounds):
        ops = []
        for c in range(n):
            r = rng.random()
            if scn.exists[c] and r < 0.15:  # truncate / extend to a target length
                ops.append(("T" if r < 0.10 else "E", int(rng.integers(0, cap + 1))))
                continue
            off = scn.sizes[c] if r < 0.45 else int(rng.integers(0, min(cap - 1, scn.sizes[c] + 5000) + 1))
            ln = int(rng.choice([rng.integers(1, 3000), 4096, 8192]))
            ln = min(ln, cap - off)
            if ln <= 0:
                off, ln = 0, 1
            without = rng.random() < 0.3
            bad = (not without) and rng.random() < 0.09
            ops.append(("W", off, ln, int(rng.integers(0, 16)), bad, without))
        scn.add_round(ops, rng)
    return scn
