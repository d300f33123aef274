"""tests/stream_queue.py checked on the CPU.  A numpy stand-in plays the library for a whole queue
of update rounds (every round's payloads and records resident at once, one arena): the faithful
one must pass check_queue, and each stand-in seeded with an ordering or lifetime defect of the
kind a queue can hide must be rejected with a message naming the round and the chunk.  The
follow-up records and the chain builders' expected values are compared with the oracle."""
import re

import numpy as np
import pytest

import batch_cases as bc
import stream_queue as sq
import update_footprint as fp

M32 = 0xFFFFFFFF


class QueueStandIn:
    """Applies the rounds with orc.replica_apply / orc.engine_apply from the IO records alone."""
    CHUNK_ADDR, PAY_ADDR, PAY_STEP = 0x7F0000000000, 0x7E0000000000, 1 << 32

    def __init__(self, orc, scn):
        self.orc, self.scn = orc, scn
        self.pay_addrs = [self.PAY_ADDR + k * self.PAY_STEP for k in range(len(scn.rounds))]
        self.sent = sq.queue_records(scn, self.CHUNK_ADDR, self.pay_addrs)

    def apply(self, k, arena, pay, recbuf, exists, keep_failed_bytes=None):
        scn = self.scn
        m = sq.round_counts(scn)[k]
        rec = recbuf[fp.REC_GUARD:fp.REC_GUARD + m * fp.REC.itemsize].view(fp.REC)
        for i in range(m):
            u = rec[i]
            base, s0 = int(u["chunk"]) - self.CHUNK_ADDR, int(u["chunk_size"])
            off, ln, kind = int(u["offset"]), int(u["length"]), int(u["update_type"])
            data = b""
            if kind == fp.WRITE and off + ln <= scn.max_len:
                p = int(u["payload"]) - self.pay_addrs[k]
                data = pay[p:p + ln].tobytes()
            scratch = bytearray(arena[base:base + scn.max_len].tobytes())
            if int(u["flags"]) & fp.FLAG_ENGINE:
                fin = (~int(u["chunk_checksum"])) & M32
                if kind == fp.WRITE:
                    dck = (~int(u["write_checksum"])) & M32 if int(u["write_checksum_type"]) == fp.CRC32C else None
                    rc, size, out, kase = self.orc.engine_apply(scratch, s0, fin, data, off, scn.max_len,
                                                                exists=exists[i], data_ck=dck, with_case=True)
                else:
                    rc, size, out, kase = self.orc.engine_apply(scratch, s0, fin, b"", ln, scn.max_len,
                                                                truncate=kind == fp.TRUNCATE, with_case=True)
                if rc == fp.OK:
                    exists[i] = True
                out = (fp.CRC32C, (~out) & M32)
            else:
                ck = (int(u["chunk_checksum_type"]), int(u["chunk_checksum"]))
                wck = (int(u["write_checksum_type"]), int(u["write_checksum"]))
                rc, size, out, kase = self.orc.replica_apply(scratch, s0, ck, kind, off, ln, data, wck, with_case=True)
            u["status"], u["checksum_case"], u["out_size"] = rc, kase, size
            u["out_checksum_type"], u["out_checksum"] = out
            if rc == fp.OK:
                arena[base:base + scn.max_len] = np.frombuffer(bytes(scratch), dtype=np.uint8)
            elif keep_failed_bytes == i and data:
                arena[base + off:base + off + ln] = np.frombuffer(data, dtype=np.uint8)

    def run(self, fault=None, at=None):
        """-> (arena, pays, recbufs, sent recbufs) after the whole queue; fault seeds one defect."""
        scn, rounds = self.scn, len(self.scn.rounds)
        arena = scn.image_before(0).copy()
        pays = [scn.payload_image(k).copy() for k in range(rounds)]
        got = [b.copy() for b in self.sent]
        exists = [False] * scn.n
        order = list(range(rounds))
        if fault == "reordered":
            order[at], order[at + 1] = order[at + 1], order[at]
        if fault == "last_skipped":
            order = order[:-1]
        for k in order:
            self.apply(k, arena, pays[k], got[k], exists,
                       keep_failed_bytes=at[1] if fault == "failed_io_written" and at[0] == k else None)
        if fault == "stale_outputs":  # round `at` reports what round at - 1 reported
            a = got[at][fp.REC_GUARD:-fp.REC_GUARD].view(fp.REC)
            b = got[at - 1][fp.REC_GUARD:-fp.REC_GUARD].view(fp.REC)
            m = min(a.size, b.size)
            for f in fp.OUTPUT_FIELDS:
                a[f][:m] = b[f][:m]
        if fault == "guard_byte":     # a write meant for round at + 1 lands in round at's tail guard
            got[at][-fp.REC_GUARD] ^= 0x40
        return arena, pays, got, self.sent


@pytest.fixture(scope="module")
def mixed(orc):
    return fp.rounds_scenario(orc, n=24, max_len=8192, rounds=4)


def _scenario(orc, mixed, name):
    return {"mixed": lambda: mixed,
            "crc32": lambda: fp.rounds_scenario(orc, fp.CRC32, n=12, max_len=4096, rounds=3),
            "engine": lambda: fp.engine_scenario(orc, n=16, cap=16 << 10, rounds=4),
            "growth": lambda: sq.growth_scenario(orc, counts=(3, 12, 2, 12, 6, 12), max_len=4096)}[name]()


@pytest.mark.parametrize("name", ["mixed", "crc32", "engine", "growth"])
def test_faithful_stand_in_passes(orc, mixed, name):
    scn = _scenario(orc, mixed, name)
    sq.check_queue(scn, *QueueStandIn(orc, scn).run())


def test_growth_scenario_sends_the_first_records_only(orc):
    scn = sq.growth_scenario(orc, counts=(3, 12, 2, 12, 6, 12), max_len=4096)
    assert sq.round_counts(scn) == [3, 12, 2, 12, 6, 12] and scn.n == 12
    sent = sq.queue_records(scn, 0x10000, [0x20000] * 6)
    assert [b.size for b in sent] == [2 * fp.REC_GUARD + m * fp.REC.itemsize for m in sq.round_counts(scn)]
    full = scn.record_buffer(2, 0x10000, 0x20000)
    assert np.array_equal(sent[2][:fp.REC_GUARD + 2 * 56], full[:fp.REC_GUARD + 2 * 56])
    assert sq.GROWTH_COUNTS == (8, 32, 4, 32, 16, 32)
    statuses = {e[0] for r in scn.rounds for e in r.expect[:r.count]}
    assert statuses >= {fp.OK, fp.CHECKSUM_MISMATCH}


def _find(scn, pred):
    for k, r in enumerate(scn.rounds):
        for i, op in enumerate(r.ops):
            if pred(k, r, i, op):
                return k, i
    raise AssertionError("the scenario has no such IO")


def test_seeded_stand_ins_are_rejected(orc, mixed):
    si = QueueStandIn(orc, mixed)
    last = len(mixed.rounds) - 1
    named = r"round (\d+): .*chunk (\d+)"

    # rounds applied in another order: round 2 before round 1
    with pytest.raises(AssertionError, match=named) as e:
        sq.check_queue(mixed, *si.run("reordered", 1))
    assert int(re.search(named, str(e.value)).group(1)) in (1, 2)

    # a failed IO's round leaving its bytes changed (in the last round: nothing rewrites them)
    k, i = _find(mixed, lambda k, r, i, op: k == last and r.expect[i][0] == fp.CHECKSUM_MISMATCH)
    with pytest.raises(AssertionError, match=rf"round {last}: chunk arena differs .* = chunk {i} \+"):
        sq.check_queue(mixed, *si.run("failed_io_written", (k, i)))
    # (bytes a later round rewrites are out of a queue's sight: test_gpu_update_footprint.py checks
    # the arena after every single call)

    # round k's records holding round k - 1's outputs
    with pytest.raises(AssertionError, match=r"round 2: chunk \d+ "):
        sq.check_queue(mixed, *si.run("stale_outputs", 2))

    # one byte written into another round's record guard
    with pytest.raises(AssertionError, match=rf"round 1: record guard after the array changed in 1 bytes, guard offsets "
                                             rf"0\.\.0 \(behind the record of chunk {mixed.n - 1}\)"):
        sq.check_queue(mixed, *si.run("guard_byte", 1))

    # the last round skipped
    with pytest.raises(AssertionError, match=rf"round {last}: chunk \d+ "):
        sq.check_queue(mixed, *si.run("last_skipped"))


def test_engine_queue_rejects_reordered_rounds(orc):
    scn = fp.engine_scenario(orc, n=16, cap=16 << 10, rounds=4)
    with pytest.raises(AssertionError, match=r"round \d+: .*chunk \d+"):
        sq.check_queue(scn, *QueueStandIn(orc, scn).run("reordered", 1))


# ---- follow-up records -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "crc32", "engine"])
def test_followup_records_match_oracle(orc, mixed, name):
    """scrub / read_result of the oracle on the final image: status 0 and the stored value."""
    scn = _scenario(orc, mixed, name)
    base = 0x7F0000000000
    fu = sq.followup_records(scn, base)
    img = scn.image_after(len(scn.rounds) - 1)
    unchecked = 0
    for c in range(scn.n):
        s, r = fu["scrub"][c], fu["read"][c]
        o, ln = int(s["data"]) - base, int(s["length"])
        assert o == scn.lay.bases[c] and ln == scn.rounds[-1].sizes_after[c]
        rc, computed = orc.scrub(int(s["checksum_type"]), int(s["fin"]), img[o:o + ln], int(s["checksum"]))
        assert (rc, computed) == (fp.OK, int(fu["computed"][c])), c
        assert int(r["data"]) - base == o and int(r["offset"]) == 0 and int(r["length"]) == int(r["chunk_len"]) == ln
        rc, out = orc.read_result(int(r["batch_checksum_type"]), (int(r["chunk_checksum_type"]), int(r["chunk_checksum"])),
                                  0, img[o:o + ln], ln, full_chunk=img[o:o + ln], recalculate=bool(r["recalculate"]))
        assert (rc, out) == (fp.OK, (int(fu["types"][c]), int(fu["computed"][c]))), c
        if int(s["checksum_type"]) == fp.NONE:
            unchecked += 1
            assert ln == 0 or not scn.engine and scn.cks[c][0] == fp.NONE
        else:
            assert int(r["recalculate"]) == 1 and int(s["checksum_type"]) == scn.ctype
    assert unchecked < scn.n // 2
    # the faithful results pass check_followup, a stale chunk does not
    got_s, got_r = fu["scrub"].copy(), fu["read"].copy()
    got_s["status"], got_r["status"] = 0, 0
    got_s["computed"], got_r["out_checksum"], got_r["out_checksum_type"] = fu["computed"], fu["computed"], fu["types"]
    sq.check_followup(fu, got_s, got_r, 0)
    c = int(np.flatnonzero(fu["types"] != fp.NONE)[0])
    got_s["status"][c] = fp.CHECKSUM_MISMATCH
    with pytest.raises(AssertionError, match=rf"scrub: chunk {c} status 4080"):
        sq.check_followup(fu, got_s, got_r, 0)
    with pytest.raises(AssertionError, match="1 mismatches"):
        sq.check_followup(fu, got_s, got_r, 1)


# ---- chain builders --------------------------------------------------------------------------------
def test_frames_chain_matches_calc_serde(orc):
    inp = sq.frames_chain(np.random.default_rng(5), n=400, max_size=20 << 10)
    f, a = inp["frames"], inp["arena"]
    assert set(np.unique(f["checksum"])) == {0, 1} and int(f["size"].max()) == 20 << 10 and int(f["size"].min()) == 0
    end = 0
    for i in range(f.size):
        o, sz = int(f["offset"][i]), int(f["size"][i])
        assert o == end + 8  # walked: a header's 8 bytes between payloads
        end = o + sz
        assert int(inp["computed"][i]) == orc.calc_serde(a[o:o + sz], compressed=bool(f["checksum"][i])), i
    assert end <= a.size
    assert not np.any(inp["computed"] == f["checksum"])  # the first pass reports every frame


@pytest.mark.parametrize("kind", ["wave", "split"])
def test_digest_chain_matches_oracle(orc, kind):
    d = sq.digest_chain(np.random.default_rng(6), kind)
    b, a = d["blocks"], d["arena"]
    assert not b["checksum"].any() and np.array_equal(b["read_len"], b["block_len"])
    nb = np.diff(d["file_off"].astype(np.int64))
    assert (nb.min(), nb.max()) == ((1, 64) if kind == "wave" else (4100, 4100)) and d["max_blocks"] == nb.max()
    assert nb.size == (200 if kind == "wave" else 1)
    # the checksum column as the device chain fills it: create over every block's byte range
    b = b.copy()
    b["checksum"] = bc.crc_ranges(bc.CRC32C, a, d["block_ranges"][:, 0], d["block_ranges"][:, 1])
    res = orc.file_digest_batch(b, d["file_off"])
    whole = bc.crc_ranges(bc.CRC32C, a, d["file_ranges"][:, 0], d["file_ranges"][:, 1])
    for f in range(nb.size):
        o, ln = (int(x) for x in d["file_ranges"][f])
        blk = d["block_ranges"][int(d["file_off"][f]):int(d["file_off"][f + 1])]
        assert int(blk[0, 0]) == o and int(blk[:, 1].sum()) == ln and ln <= d["max_file_len"]
        assert (int(res["status"][f]), int(res["type"][f])) == (0, bc.CRC32C)
        assert int(res["value"][f]) == orc.crc32c_raw(a[o:o + ln]) == int(whole[f]), f


def test_halves_chain_combines_to_the_whole(orc):
    h = sq.halves_chain(np.random.default_rng(7))
    a = h["arena"]
    assert h["whole"].shape == (256, 2)
    assert np.array_equal(h["first"][:, 0], h["whole"][:, 0])
    assert np.array_equal(h["first"][:, 1], h["whole"][:, 1] // 2 + 7)
    assert np.array_equal(h["second"][:, 0], h["first"][:, 0] + h["first"][:, 1])
    assert np.array_equal(h["first"][:, 1] + h["second"][:, 1], h["whole"][:, 1])
    assert int((h["whole"][:, 0] + h["whole"][:, 1]).max()) <= a.size and h["max_len"] == int(h["whole"][:, 1].max())
    for ctype, poly, raw in ((bc.CRC32C, orc.POLY_CRC32C, orc.crc32c_raw), (bc.CRC32, orc.POLY_CRC32, orc.crc32_raw)):
        c1 = bc.crc_ranges(ctype, a, h["first"][:, 0], h["first"][:, 1])
        c2 = bc.crc_ranges(ctype, a, h["second"][:, 0], h["second"][:, 1])
        acc = orc.combine_batch(c1, c2, h["second"][:, 1], poly=poly)
        want = np.array([raw(a[int(o):int(o + ln)]) for o, ln in h["whole"]], dtype=np.uint32)
        assert np.array_equal(acc, want)
