"""The COW planner restated in numpy (on the pattern of expected_schedule in tests/batch_cases.py)
against the expected images of tests/cow_cases.py: for every scenario the GPU tests run, the
planned pieces, played into the arena the batch starts from, give exactly the expected arena --
every expected byte written once, nothing else touched.  Deliberately wrong planners are caught,
so the scenarios can tell a right implementation from the likely wrong ones.  No GPU.
"""
import numpy as np
import pytest

import cow_cases as cc
import update_footprint as fp

PIECES = (4, 8, 16)


def plan_ranges(u, dst, ok, bug=None):
    """update_plan.h plan_ranges restated: [(dst, src kind, src, len)] of one IO.  u: the record
    (arena-relative addresses), dst: its destination entry (0 / chunk: in place), ok: the IO passes
    its argument checks and its payload verify (a failed one plays nothing)."""
    if not ok:
        return []
    chunk, s0 = int(u["chunk"]), int(u["chunk_size"])
    image = int(dst) if int(dst) else chunk
    sync = bool(u["flags"] & cc.FLAG_SYNCING)
    out = []
    if u["update_type"] == fp.WRITE:
        off, ln = int(u["offset"]), int(u["length"])
        out.append((image + off, "pay", int(u["payload"]), ln))
        if off > s0:
            gap_at = chunk if bug == "gap_at_chunk" else image
            out.append((gap_at + s0, "zero", 0, off - s0))
        if image != chunk and not sync:
            pre = off if bug == "prefix_unclipped" else min(off, s0)
            suf = min(off + ln, s0) + (1 if bug == "suffix_off_by_one" else 0)
            out.append((image, "old", chunk, pre))
            out.append((image + suf, "old", chunk + suf, max(s0 - suf, 0)))
    else:
        target = int(u["length"])
        s1 = target if (target > s0 or u["update_type"] == fp.TRUNCATE) else s0
        if target > s0:
            out.append((image + s0, "zero", 0, target - s0))
        if image != chunk:
            out.append((image, "old", chunk, min(s0, s1)))
    return [r for r in out if r[3] > 0]


def pieces(dst, ln, piece):
    """One-shot pieces of a range: cut at every piece-aligned destination address."""
    cuts, a = [], dst
    while a < dst + ln:
        b = min((a // piece + 1) * piece, dst + ln)
        cuts.append((a, b))
        a = b
    return cuts


def play(scn, piece, bug=None):
    """The arena after the planned pieces of every IO, and how often each byte was written."""
    r = scn.rounds[0]
    arena = scn.image_before(0).copy()
    before = scn.image_before(0)
    pay = scn.payload_image(0)
    count = np.zeros(arena.size, dtype=np.uint8)
    for c in range(scn.n):
        u = r.rec[c]
        d = int(r.dst[c]) if r.place[c] == cc.OUT_OF_PLACE else (0 if r.place[c] == cc.IN_PLACE_ZERO else int(u["chunk"]))
        for dst, kind, src, ln in plan_ranges(u, d, r.expect[c][0] == fp.OK, bug):
            for a, b in pieces(dst, ln, piece):
                if kind == "zero":
                    arena[a:b] = 0
                elif kind == "pay":
                    arena[a:b] = pay[src + a - dst:src + b - dst]
                else:
                    arena[a:b] = before[src + a - dst:src + b - dst]
                count[a:b] += 1
    return arena, count


def written_mask(scn):
    """The bytes the call is expected to write: an out-of-place OK IO's [0, out_size) of its
    destination; in place the payload and the zero-filled gap / extension."""
    r = scn.rounds[0]
    m = np.zeros(scn.image_before(0).size, dtype=bool)
    for c in range(scn.n):
        e, u = r.expect[c], r.rec[c]
        if e[0] != fp.OK:
            continue
        if r.place[c] == cc.OUT_OF_PLACE:
            m[int(r.dst[c]):int(r.dst[c]) + e[1]] = True
            continue
        base, s0 = int(u["chunk"]), int(u["chunk_size"])
        if u["update_type"] == fp.WRITE:
            m[base + int(u["offset"]):base + int(u["offset"]) + int(u["length"])] = True
            if int(u["offset"]) > s0:
                m[base + s0:base + int(u["offset"])] = True
        elif int(u["length"]) > s0:
            m[base + s0:base + int(u["length"])] = True
    return m


def _scenarios(orc):
    out = []
    k = 0
    for max_len in (64 << 10, 128 << 10):
        for piece in PIECES:
            for kind in ("crc32c", "crc32", "engine"):
                for _ in range(4):   # (the GPU module's 72 cases: mode and grid do not change the images)
                    ctype = fp.CRC32 if kind == "crc32" else fp.CRC32C
                    if k % 4 == 0 or k % 16 in (5, 10, 15):   # a third of them, every piece size / kind / capacity
                        out.append((cc.main_scenario(orc, max_len, piece << 10, ctype, engine=kind == "engine",
                                                     rot=k % 16, variant=k % 16), piece << 10))
                    k += 1
        for kind in ("crc32c", "engine"):
            ctype = fp.CRC32C
            out.append((cc.syncing_scenario(orc, max_len, ctype, engine=kind == "engine", rot=3), 8 << 10))
    return out


@pytest.fixture(scope="module")
def scenarios(orc):
    return _scenarios(orc)


def test_planned_pieces_tile_the_expected_bytes_exactly_once(scenarios):
    for scn, piece in scenarios:
        arena, count = play(scn, piece)
        assert np.array_equal(arena, scn.image_after(0)), (scn.max_len, piece, scn.engine)
        mask = written_mask(scn)
        assert np.array_equal(count, mask.astype(np.uint8)), (scn.max_len, piece, scn.engine)


@pytest.mark.parametrize("bug", ["suffix_off_by_one", "prefix_unclipped", "gap_at_chunk"])
def test_wrong_planners_are_caught(scenarios, bug):
    """Each wrong planner leaves a wrong arena (or writes a byte twice / not at all) in at least one
    main scenario -- and in every one of them for the suffix and the gap, which every batch has."""
    caught = 0
    mains = [(s, p) for s, p in scenarios if not any(op.get("sync") for op in s.rounds[0].ops)]
    for scn, piece in mains:
        arena, count = play(scn, piece, bug)
        bad = not np.array_equal(arena, scn.image_after(0)) or not np.array_equal(count, written_mask(scn).astype(np.uint8))
        caught += bad
    assert caught == len(mains), (bug, caught, len(mains))


def test_record_layout_and_flag(hf):
    L = hf._lib
    assert cc.FLAG_SYNCING == L.UPDATE_FLAG_SYNCING == hf.FLAG_SYNCING == 2
    assert fp.REC.itemsize == 56
