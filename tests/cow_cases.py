"""Scenarios of hf3fs_crc_update_cow_batch (and of HF3FS_UPDATE_FLAG_SYNCING), shared by
tests/test_gpu_update_cow.py (the HIP library) and tests/test_update_cow_model.py (a numpy
restatement of the planner, which checks the checker).

On the pattern of tests/update_footprint.py, whose canary, Layout, REC and check_round are used
as they are: one arena holds the n source chunks (regions 0..n-1) and the n destinations
(regions n..2n-1), every region at a base of residue (region index) mod 16 and regions a canary
gap apart.  IO c's destination is region n + (c + rot) % n, so over rot = 0..15 every pair of
source / destination residues mod 16 occurs.  Payloads and the record array sit in canaries of
their own.

Expected state: the oracle (oracle.replica_apply / oracle.engine_apply) runs on a COPY of the
source region; for an out-of-place IO whose status is OK, bytes [0, out_size) of the result are
placed at the destination and the source region stays what it was; a failed IO leaves both.  An
in-place IO (destination entry 0 or the chunk's own address) leaves the oracle's whole region in
the source region.  For replica IOs with the syncing flag the state is written out here from
ChunkReplica.cc:289,334-339,392 (oracle.create gives the value); engine syncing IOs go through
oracle.engine_apply(is_syncing=True).

Numpy only: no GPU, no torch.
"""
import numpy as np

import update_footprint as fp

FLAG_SYNCING = 2
DST_GUARD = 1 << 10
SALT_DST = 0x3D

IN_PLACE_ZERO, IN_PLACE_SELF, OUT_OF_PLACE = 0, 1, 2


def edge_lengths(piece):
    """Old-prefix / old-suffix lengths the cases must reach: 0, 1, 15, 16, 17 and several pieces +- 1."""
    return (0, 1, 15, 16, 17, 2 * piece - 1, 2 * piece + 1)


class Round:
    pass


class CowScenario:
    """One batch of n IOs.  Duck-types what update_footprint.check_round reads of a Scenario
    (lay, n, engine, rounds, image_after, payload_image), with 2 n regions in the layout."""

    def __init__(self, orc, n, max_len, ctype=fp.CRC32C, engine=False, rot=0, seed=1):
        self.orc, self.n, self.max_len, self.ctype, self.engine, self.rot = orc, n, max_len, ctype, engine, rot
        self.lay = fp.Layout(2 * n, max_len, gap=fp.MARGIN)
        self.canary = fp.canary(self.lay.size, fp.SALT_CHUNKS)
        self.rng = np.random.default_rng(seed)
        self.regions = [bytearray(self.canary[b:b + max_len].tobytes()) for b in self.lay.bases]
        self.sizes = [0] * n
        self.cks = [(ctype, 0)] * n
        self.fins = [0] * n
        self.rounds = []

    def dst_region(self, c):
        return self.n + (c + self.rot) % self.n

    def preset(self, c, size):
        data = self.rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        self.regions[c][:size] = data
        self.sizes[c] = size
        if self.engine:
            self.fins[c] = self.orc.rs_crc32c(data)
        else:
            self.cks[c] = tuple(self.orc.create(self.ctype, data)) if size else (self.ctype, 0)

    def _image(self, regions):
        img = self.canary.copy()
        for r, b in enumerate(self.lay.bases):
            img[b:b + self.max_len] = np.frombuffer(bytes(regions[r]), dtype=np.uint8)
        return img

    # ops[c]: dict(kind="W"|"T"|"E", off, ln, shift, corrupt, without, sync, place, target, wnone)
    def build(self, ops):
        assert len(ops) == self.n and not self.rounds
        n, orc = self.n, self.orc
        self.before = self._image(self.regions)
        self.before.setflags(write=False)
        r = Round()
        rec = np.zeros(n, dtype=fp.REC)
        has_payload = np.zeros(n, dtype=bool)
        dst = np.zeros(n, dtype=np.uint64)        # arena-relative; 0 = entry 0; place decides
        place = np.zeros(n, dtype=np.int64)
        placed, cur, expect = [], fp.PAY_GUARD, []
        after = [bytearray(x) for x in self.regions]
        sizes_after = [0] * (2 * n)
        for c, op in enumerate(ops):
            u = rec[c]
            kind = op["kind"]
            place[c] = op.get("place", OUT_OF_PLACE)
            oop = place[c] == OUT_OF_PLACE
            image_region = self.dst_region(c) if oop else c
            u["chunk"] = self.lay.bases[c]
            u["chunk_size"] = self.sizes[c]
            sync = bool(op.get("sync"))
            if self.engine:
                u["chunk_checksum_type"], u["chunk_checksum"] = fp.CRC32C, (~self.fins[c]) & fp.M32
                u["flags"] = fp.FLAG_ENGINE
            else:
                u["chunk_checksum_type"], u["chunk_checksum"] = self.cks[c]
            if sync:
                u["flags"] |= FLAG_SYNCING
            work = bytearray(self.regions[c])   # the oracle's copy of the source region
            if kind in "TE":
                code = fp.TRUNCATE if kind == "T" else fp.EXTEND
                target = int(op["target"])
                u["update_type"], u["offset"], u["length"] = code, 0, target
                if sync:   # the flag is valid on a write only
                    e = (fp.INVALID_ARG, self.sizes[c], self.cks[c], 0)
                elif self.engine:
                    e = orc.engine_apply(work, self.sizes[c], self.fins[c], b"", target, self.max_len,
                                         truncate=kind == "T", with_case=True)
                else:
                    e = orc.replica_apply(work, self.sizes[c], self.cks[c], code, 0, target, with_case=True)
            else:
                off, ln, shift = int(op["off"]), int(op["ln"]), int(op.get("shift", 0))
                corrupt, without = bool(op.get("corrupt")), bool(op.get("without"))
                data = self.rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
                p = ((cur + 15) & ~15) + (self.lay.bases[image_region] + off + shift) % 16
                placed.append((p, data))
                cur = p + ln + 256
                has_payload[c] = True
                u["update_type"], u["offset"], u["length"], u["payload"] = fp.WRITE, off, ln, p
                if self.engine:
                    fin = orc.rs_crc32c(data) ^ (0x100 if corrupt else 0)
                    if without:
                        u["write_checksum_type"], u["write_checksum"] = fp.NONE, 0
                    else:
                        u["write_checksum_type"], u["write_checksum"] = fp.CRC32C, (~fin) & fp.M32
                    if off >= self.max_len or off + ln > self.max_len or (sync and off != 0):
                        e = (fp.INVALID_ARG, self.sizes[c], self.fins[c], 0)
                    else:
                        e = orc.engine_apply(work, self.sizes[c], self.fins[c], data, off, self.max_len,
                                             is_syncing=sync, exists=self.sizes[c] > 0 or sync, data_ck=fin,
                                             with_case=True)
                else:
                    wck = tuple(orc.create(self.ctype, data)) if not without else (fp.NONE, 0)
                    if corrupt:
                        wck = (wck[0], wck[1] ^ 0x10)
                    u["write_checksum_type"], u["write_checksum"] = wck
                    if sync:
                        e = self._replica_syncing(work, c, off, ln, data, wck)
                    else:
                        e = orc.replica_apply(work, self.sizes[c], self.cks[c], fp.WRITE, off, ln, data, wck,
                                              chunk_size=self.max_len, with_case=True)
            expect.append(e)
            ok = e[0] == fp.OK
            if oop:
                dst[c] = self.lay.bases[image_region]
                if ok:
                    after[image_region][:e[1]] = work[:e[1]]
                    sizes_after[image_region] = e[1]
            else:
                after[c] = work
            sizes_after[c] = e[1] if ok and not oop else self.sizes[c]
        pay = fp.canary(cur + fp.PAY_GUARD, fp.SALT_PAYLOAD)
        for p, data in placed:
            pay[p:p + len(data)] = np.frombuffer(data, dtype=np.uint8)
        pay.setflags(write=False)
        self.pay_size = pay.size
        r.ops = list(ops) + [ops[(q - self.rot) % n] for q in range(n)]   # (by region, for check_round's messages)
        r.rec, r.has_payload, r.pay, r.expect = rec, has_payload, pay, expect
        r.dst, r.place = dst, place
        r.sizes_before, r.sizes_after = list(self.sizes), sizes_after
        r.image = self._image(after)
        r.image.setflags(write=False)
        self.rounds.append(r)
        return self

    def _replica_syncing(self, work, c, off, ln, data, wck):
        """ChunkReplica::update with isSyncing, restated: kInvalidArg for the shapes the ABI rejects
        (offset != 0) and ChunkReplica.cc:139-145; payload verify (:193-207); meta.size =
        writeIO.length (:289); updateChecksum with that size (:334-339: NONE type or size 0 ->
        none, else offset 0 and length == size -> reuse), type = the write's (:392)."""
        if off != 0 or off >= self.max_len or off + ln > self.max_len:
            return (fp.INVALID_ARG, self.sizes[c], self.cks[c], 0)
        if wck[0] != fp.NONE and ln != 0 and tuple(self.orc.create(wck[0], data)) != tuple(wck):
            return (fp.CHECKSUM_MISMATCH, self.sizes[c], self.cks[c], 0)
        work[:ln] = data
        if wck[0] == fp.NONE or ln == 0:
            return (fp.OK, ln, (wck[0], 0), 1)
        return (fp.OK, ln, (wck[0], tuple(self.orc.create(wck[0], data))[1]), 2)

    # -- what check_round and the backends read -------------------------------------------------
    def image_before(self, k=0):
        return self.before

    def image_after(self, k=0):
        return self.rounds[0].image

    def payload_image(self, k=0):
        return self.rounds[0].pay

    def record_buffer(self, chunk_addr, pay_addr):
        r = self.rounds[0]
        rec = r.rec.copy()
        rec["chunk"] += np.uint64(chunk_addr)
        rec["payload"][r.has_payload] += np.uint64(pay_addr)
        buf = fp.canary(2 * fp.REC_GUARD + rec.nbytes, fp.SALT_RECORDS)
        buf[fp.REC_GUARD:fp.REC_GUARD + rec.nbytes] = rec.view(np.uint8)
        return buf

    def dst_buffer(self, chunk_addr):
        """The destination array with absolute addresses inside a canary: entry 0 for
        IN_PLACE_ZERO, the chunk's own address for IN_PLACE_SELF."""
        r = self.rounds[0]
        d = np.zeros(self.n, dtype=np.uint64)
        oop = r.place == OUT_OF_PLACE
        d[oop] = r.dst[oop] + np.uint64(chunk_addr)
        own = r.place == IN_PLACE_SELF
        d[own] = r.rec["chunk"][own] + np.uint64(chunk_addr)
        buf = fp.canary(2 * DST_GUARD + d.nbytes, SALT_DST)
        buf[DST_GUARD:DST_GUARD + d.nbytes] = d.view(np.uint8)
        return buf

    def in_place_twin(self):
        """The same IOs, every one in place (what update_batch does with the records)."""
        twin = CowScenario(self.orc, self.n, self.max_len, self.ctype, self.engine, self.rot)
        twin.regions = [bytearray(x) for x in self.regions]
        twin.sizes, twin.cks, twin.fins = list(self.sizes), list(self.cks), list(self.fins)
        twin.rng = np.random.default_rng(0)
        return twin


def check(scn, got_arena, got_pay, got_recbuf, sent_recbuf, got_dstbuf=None, sent_dstbuf=None):
    fp.check_round(scn, 0, got_arena, got_pay, got_recbuf, sent_recbuf)
    if got_dstbuf is not None:
        assert np.array_equal(got_dstbuf, sent_dstbuf), "the destination array or its guards changed"


# ---- the cases -----------------------------------------------------------------------------------
def _w(off, ln, shift=0, **kw):
    return dict(kind="W", off=off, ln=ln, shift=shift, **kw)


def edge_pairs(max_len, piece, mid=300):
    """(prefix, suffix) pairs of edge_lengths that fit a chunk of max_len around a write of `mid`."""
    E = edge_lengths(piece)
    return [(p, s) for p in E for s in E if p + s + mid <= max_len]


def main_scenario(orc, max_len, piece, ctype=fp.CRC32C, engine=False, rot=0, variant=0):
    """32 IOs, out of place unless said: [0] a write covering the whole chunk, [1] an append, [2] a
    write past a gap, [3..14] overwrites in the middle with old prefix / old suffix lengths from
    edge_pairs (rotated by `variant`, so the variants of a shape cover every pair), [15] a length-0
    write, [16] a write into an empty chunk, [17..19] truncate shorter / equal / longer, [20] an
    extend, [21] a bad payload checksum, [22] an INVALID_ARG IO, [23] an overwrite in place (entry
    0), [24] an append in place (entry = chunk), [25] an overwrite running past the old size, [26]
    an overwrite whose prefix ends and [27] whose suffix starts on a piece line of the destination,
    [28] a truncate to 0, [29] a one-byte write at offset 0 of a one-byte chunk, [30] a write ending
    at max_len, [31] a length-0 write in place."""
    n = 32
    scn = CowScenario(orc, n, max_len, ctype, engine, rot, seed=0xC0 + 131 * variant + max_len // 1024 + piece + ctype)
    pairs = edge_pairs(max_len, piece)
    ops = [None] * n
    wo = (lambda c: engine and c % 3 == 0)   # engine: every third write "without_checksum"

    def put(c, size, op):
        if size:
            scn.preset(c, size)
        if op["kind"] == "W" and wo(c):
            op["without"] = True
        ops[c] = op

    put(0, 5000 + variant, _w(0, 5000 + variant + (variant % 2) * 77, 1))
    put(1, 3000 + 16 * variant + variant, _w(3000 + 16 * variant + variant, 4097 + variant, 2))
    put(2, 1000 + variant, _w(1000 + variant + 2 * piece + 5, 333, 3))
    for j in range(12):
        p, s = pairs[(12 * variant + j) % len(pairs)]
        mid = 200 + 7 * j
        put(3 + j, p + mid + s, _w(p, mid, (j + variant) % 16))
    put(15, 4321, _w(1234, 0, 4))
    put(16, 0, _w(0, 2 * piece + 17, 5))
    put(17, 3 * piece + 100, dict(kind="T", target=piece + 50 + variant))
    put(18, 2222 + variant, dict(kind="T", target=2222 + variant))
    put(19, 700, dict(kind="T", target=700 + 2 * piece + 3))
    put(20, 900 + variant, dict(kind="E", target=900 + variant + piece + 1))
    put(21, 6000, _w(100, 3000, 6, corrupt=True))
    put(22, 6000, _w(max_len + 3, 5, 7))
    put(23, 2 * piece + 999, _w(piece - 5, 777, 8, place=IN_PLACE_ZERO))
    put(24, 1500, _w(1500, 2000, 9, place=IN_PLACE_SELF))
    put(25, 5000, _w(4000 + variant, 3 * piece + 1, 10))
    base26 = scn.lay.bases[scn.dst_region(26)]
    pre26 = (-base26) % piece + piece             # dst + prefix on a piece line
    put(26, pre26 + 600, _w(pre26, 300, 11))
    base27 = scn.lay.bases[scn.dst_region(27)]
    end27 = (-base27) % piece + piece             # dst + offset + length on a piece line
    put(27, end27 + 1000, _w(end27 - 400, 400, 12))
    put(28, 5555, dict(kind="T", target=0))
    put(29, 1, _w(0, 1, 13))
    put(30, max_len - 3000, _w(max_len - 4000, 4000, 14))
    put(31, 800, _w(300, 0, 15, place=IN_PLACE_ZERO))
    if engine:
        ops[21]["without"] = False   # (a corrupt checksum needs a typed write)
    return scn.build(ops)


def syncing_scenario(orc, max_len, ctype=fp.CRC32C, engine=False, rot=0):
    """32 IOs.  Syncing writes, in place (even c) and out of place (odd c), typed and NONE write
    checksums, lengths 0, 1, chunk_size, shorter and longer than chunk_size; bad checksums; the
    flag at offset != 0 and on a truncate / extend (status 3, bytes untouched); plain IOs between."""
    n = 32
    scn = CowScenario(orc, n, max_len, ctype, engine, rot, seed=0x5C + max_len // 1024 + ctype + (7 if engine else 0))
    ops = [None] * n
    c = 0
    for s0, ln in ((3000, 0), (3000, 1), (3000, 3000), (9000, 2017), (2000, 9001)):
        for without in (False, True):
            for place in (IN_PLACE_ZERO, OUT_OF_PLACE):
                scn.preset(c, s0)
                ops[c] = _w(0, ln, c % 16, sync=True, without=without, place=place)
                c += 1
    assert c == 20
    for place in (IN_PLACE_SELF, OUT_OF_PLACE):          # bad checksum
        scn.preset(c, 4000)
        ops[c] = _w(0, 2500, 3, sync=True, corrupt=True, place=place)
        c += 1
    for place in (IN_PLACE_ZERO, OUT_OF_PLACE):          # offset != 0
        scn.preset(c, 4000)
        ops[c] = _w(16 if place else 1, 1000, 5, sync=True, place=place)
        c += 1
    for kind, place in (("T", IN_PLACE_ZERO), ("T", OUT_OF_PLACE), ("E", OUT_OF_PLACE)):   # the flag on a truncate / extend
        scn.preset(c, 4000)
        ops[c] = dict(kind=kind, target=1000 if kind == "T" else 6000, sync=True, place=place)
        c += 1
    scn.preset(c, max_len - 100)                          # a whole-capacity resync
    ops[c] = _w(0, max_len, 1, sync=True)
    c += 1
    ops[c] = _w(0, 5000, 2, sync=True)                    # onto an empty chunk
    c += 1
    while c < n:                                          # plain IOs between
        scn.preset(c, 3000 + c)
        ops[c] = _w(1000, 500 + c, c % 16, place=OUT_OF_PLACE if c % 2 else IN_PLACE_ZERO)
        c += 1
    return scn.build(ops)


def in_place_scenarios(orc):
    """(name, update_footprint scenario) whose records drive the d_dst == NULL / all-zero / all-own
    comparison with hf3fs_crc_update_batch: tiny, rows and mixed rounds."""
    return [("tiny", fp.tiny_scenario(orc)), ("rows", fp.rows_scenario(orc)),
            ("rounds", fp.rounds_scenario(orc, n=32, max_len=128 << 10, rounds=3))]
