"""The write-footprint checker (tests/update_footprint.py) checked on the CPU: the same
run_scenario / check_round the GPU tests use, driven by a numpy stand-in for the library.
A correct stand-in passes every scenario; each deliberately wrong one is flagged at the
right place.  The stand-in writes its bytes with plain numpy slices from the IO record alone
(only its output fields come from the oracle), so the scenarios' expected images -- the
oracle's bytearrays laid over the canary -- are checked against a second statement of
ChunkReplica::update's write rules (ChunkReplica.cc:139-145,193-207,255-292)."""
import re

import numpy as np
import pytest

import update_footprint as fp


class StandIn:
    CHUNK_ADDR, PAY_ADDR = 0x7F0000000000, 0x7E0000000000

    def __init__(self, orc, fault=None, at=None):
        self.orc, self.fault, self.at, self.k = orc, fault, at, -1

    def start(self, arena, pay_size, recbuf_size):
        self.arena = arena.copy()
        return self.CHUNK_ADDR, self.PAY_ADDR

    def step(self, pay, recbuf, n, max_len):
        self.k += 1
        pay = pay.copy()
        rec = recbuf[fp.REC_GUARD:fp.REC_GUARD + n * fp.REC.itemsize].view(fp.REC)
        a = self.arena
        for i in range(n):
            u = rec[i]
            fault = self.fault if (self.k, i) == self.at else None
            base, s0 = int(u["chunk"]) - self.CHUNK_ADDR, int(u["chunk_size"])
            off, ln, kind = int(u["offset"]), int(u["length"]), int(u["update_type"])
            ck = (int(u["chunk_checksum_type"]), int(u["chunk_checksum"]))
            wck = (int(u["write_checksum_type"]), int(u["write_checksum"]))
            data = b""
            if kind == fp.WRITE and off + ln <= max_len:
                p = int(u["payload"]) - self.PAY_ADDR
                data = pay[p:p + ln].tobytes()
            scratch = bytearray(a[base:base + max_len].tobytes())
            rc, size, out, kase = self.orc.replica_apply(scratch, s0, ck, kind, off, ln, data, wck, with_case=True)
            u["status"], u["checksum_case"], u["out_size"] = rc, kase, size
            u["out_checksum_type"], u["out_checksum"] = out
            if fault == "field_changed":
                u["offset"] ^= 1
            if rc != fp.OK and fault != "ignore_mismatch":
                continue  # a failed IO leaves the chunk alone
            if kind == fp.WRITE:
                if off > s0 and fault != "gap_unzeroed":
                    a[base + s0:base + off] = 0
                a[base + off:base + off + ln] = np.frombuffer(data, dtype=np.uint8)
                if fault == "byte_before_base":
                    a[base - 1] = 0
                if fault == "granule_past_end":
                    e = base + off + ln
                    a[e:(e + 15) & ~15] = 0
            else:
                if ln > s0:
                    a[base + s0:base + ln] = 0
                elif fault == "tail_zeroed":
                    a[base + ln:base + s0] = 0
        return a.copy(), pay, recbuf


@pytest.fixture(scope="module")
def mixed(orc):
    return fp.rounds_scenario(orc, n=24, max_len=8192, rounds=4)


def test_record_mirror_matches_abi(hf):
    for name in fp.REC.names:
        assert fp.REC.fields[name][1] == getattr(hf.UpdateIO, name).offset, name
    assert (fp.WRITE, fp.TRUNCATE, fp.EXTEND) == (hf.UPDATE_WRITE, hf.UPDATE_TRUNCATE, hf.UPDATE_EXTEND)
    assert (fp.OK, fp.INVALID_ARG, fp.CHECKSUM_MISMATCH) == (hf.OK, hf.INVALID_ARG, hf.CHECKSUM_MISMATCH)
    assert fp.FLAG_ENGINE == hf._lib.UPDATE_FLAG_ENGINE
    assert int(fp.INPUT_MASK.sum()) == 56 - (4 + 4 + 1 + 1 + 4)  # reserved1 counts as input: it must stay


def test_canary_properties():
    for salt in (fp.SALT_CHUNKS, fp.SALT_PAYLOAD, fp.SALT_RECORDS):
        c = fp.canary(1 << 20, salt)
        assert c.min() >= 1
        assert (c[1:] != c[:-1]).all() and (c[16:] != c[:-16]).all()
    assert (fp.canary(4096, fp.SALT_CHUNKS) != fp.canary(4096, fp.SALT_PAYLOAD)).mean() > 0.9


def test_tiny_case_covers_every_residue(orc):
    scn = fp.tiny_scenario(orc)
    dst, src, g0, g1, at_end = fp.tiny_coverage(scn)
    every = set(range(16))
    assert dst == every and src == every and g0 == every and g1 == every
    assert at_end >= 16
    assert {op[2] for op in scn.rounds[0].ops} >= set(fp.TINY_LENGTHS)
    assert all(e[0] == fp.OK for e in scn.rounds[0].expect)


def test_rows_case_shapes(orc):
    lay = fp.Layout(48, 192 << 10, fp.MARGIN)
    shapes = fp.rows_shapes(lay)
    seen, first_on_line = set(), set()
    for k, (off, ln, sh) in enumerate(shapes[:36]):
        d0, d1 = lay.bases[k] + off, lay.bases[k] + off + ln
        g0, g1 = (d0 + 15) & ~15, d1 & ~15
        seen.add(((g1 - g0) // 16, g0 - d0, d1 - g1))
        if g0 % 1024 == 0:
            first_on_line.add((g1 - g0) // 16)
    assert {s[0] for s in seen} == set(fp.ROW_GRANULES) and first_on_line == set(fp.ROW_GRANULES)
    assert {(s[1], s[2]) for s in seen} == set(fp.ROW_EDGES)
    assert {sh for _, _, sh in shapes} == set(range(16))
    for j, P in enumerate((4 << 10, 8 << 10, 16 << 10)):
        crossed = []
        for q in range(4):
            k = 36 + 4 * j + q
            off, ln, _ = shapes[k]
            d0, d1 = lay.bases[k] + off, lay.bases[k] + off + ln
            assert off >= 0 and off + ln <= lay.max_len
            crossed.append(((d1 - 1) // P - d0 // P, d1 % P))
        assert crossed[0][0] == 1 and crossed[1][0] == 2
        assert crossed[2] == (0, P - 1) and crossed[3] == (1, 1)


@pytest.mark.parametrize("case", ["tiny", "tiny_crc32", "rows", "mixed", "engine_layout"])
def test_correct_stand_in_passes(orc, mixed, case):
    if case == "engine_layout":  # (the stand-in has no engine semantics: only the scenario is built)
        scn = fp.engine_scenario(orc, n=8, cap=16 << 10, rounds=3)
        assert len(scn.rounds) == 3 and any(e[0] == fp.OK for e in scn.rounds[0].expect)
        return
    scn = {"tiny": lambda: fp.tiny_scenario(orc), "tiny_crc32": lambda: fp.tiny_scenario(orc, fp.CRC32),
           "rows": lambda: fp.rows_scenario(orc), "mixed": lambda: mixed}[case]()
    fp.run_scenario(scn, StandIn(orc))


def _find(scn, pred):
    for k, r in enumerate(scn.rounds):
        for i, op in enumerate(r.ops):
            if pred(k, r, i, op):
                return k, i
    raise AssertionError("the scenario has no such IO")


def test_mixed_scenario_has_every_kind(mixed):
    st = [e[0] for r in mixed.rounds for e in r.expect]
    assert st.count(fp.CHECKSUM_MISMATCH) >= 2 and st.count(fp.INVALID_ARG) == 3 * len(mixed.rounds)
    kinds = {op[0] for r in mixed.rounds for op in r.ops}
    assert kinds == {"W", "T", "E"}


def test_wrong_stand_ins_are_flagged(orc, mixed):
    ok = lambda r, i: r.expect[i][0] == fp.OK  # noqa: E731
    M = mixed.max_len

    # one byte written before the base
    k, i = _find(mixed, lambda k, r, i, op: op[0] == "W" and ok(r, i) and i > 0)
    with pytest.raises(AssertionError, match=rf"first at arena offset \d+ = guard after chunk {i - 1}: .* 1 B before chunk {i} "):
        fp.run_scenario(mixed, StandIn(orc, "byte_before_base", (k, i)))

    # a 16-byte granule rounded up past the end of an appending / extending write
    k, i = _find(mixed, lambda k, r, i, op: op[0] == "W" and ok(r, i) and op[1] + op[2] == r.sizes_after[i]
                 and op[1] + op[2] < M - 16 and (mixed.lay.bases[i] + op[1] + op[2]) % 16)
    end = mixed.rounds[k].ops[i][1] + mixed.rounds[k].ops[i][2]
    with pytest.raises(AssertionError, match=rf"round {k}: .*first at arena offset \d+ = chunk {i} \+{end} "
                                             rf"\(tail past its new size {end}\)"):
        fp.run_scenario(mixed, StandIn(orc, "granule_past_end", (k, i)))

    # a write applied despite a corrupted checksum
    k, i = _find(mixed, lambda k, r, i, op: r.expect[i][0] == fp.CHECKSUM_MISMATCH)
    with pytest.raises(AssertionError, match=rf"round {k}: chunk arena differs .*first at arena offset \d+ = chunk {i} \+"):
        fp.run_scenario(mixed, StandIn(orc, "ignore_mismatch", (k, i)))

    # a gap left unzeroed
    k, i = _find(mixed, lambda k, r, i, op: op[0] == "W" and ok(r, i) and op[1] > r.sizes_before[i])
    s0 = mixed.rounds[k].sizes_before[i]
    with pytest.raises(AssertionError, match=rf"round {k}: .*first at arena offset \d+ = chunk {i} \+{s0} \(below its new size"):
        fp.run_scenario(mixed, StandIn(orc, "gap_unzeroed", (k, i)))

    # a truncated tail zeroed
    k, i = _find(mixed, lambda k, r, i, op: op[0] == "T" and op[1] < r.sizes_before[i] and r.regions[i][op[1]] != 0)
    t = mixed.rounds[k].ops[i][1]
    with pytest.raises(AssertionError, match=rf"round {k}: .*first at arena offset \d+ = chunk {i} \+{t} "
                                             rf"\(tail past its new size {t}\)"):
        fp.run_scenario(mixed, StandIn(orc, "tail_zeroed", (k, i)))

    # one input field of a record changed
    with pytest.raises(AssertionError, match=r"round 1: record 5 input field offset changed"):
        fp.run_scenario(mixed, StandIn(orc, "field_changed", (1, 5)))


def test_where_names_margins_and_guards():
    lay = fp.Layout(3, 4096, 2048)
    assert re.match(r"head margin, 1 B before chunk 0", lay.where(lay.bases[0] - 1))
    assert lay.where(lay.bases[1] + 7) == "chunk 1 +7"
    assert lay.where(lay.bases[1] + 4096).startswith("guard after chunk 1: 0 B past its region")
    assert lay.where(lay.bases[2] + 4096 + 9) == "tail margin, 9 B past the region of chunk 2"
